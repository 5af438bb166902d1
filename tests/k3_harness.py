"""ctypes side of tests/native/k3_harness.cpp (lcpc_amd/lib/liblcpc_k3_harness.so, built by lcpc_amd/csrc/Makefile): the BLAKE3 column-hash
(K3), Merkle-tree (K4) and path-gather launchers of lcpc_amd/csrc/kernels.h on buffers a test builds.  Elements cross as (.., L) uint64
arrays of limbs, digests and chaining values as (.., 8) uint32 arrays; in / out buffers are modified in place.  Every call returns
after the device has finished and raises on any hipError_t; BadArgs means the harness refused the call before touching the device."""
import ctypes as C
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB_PATH = os.path.join(ROOT, "lcpc_amd", "lib", "liblcpc_k3_harness.so")
NL = {0: 2, 1: 4, 2: 6, 3: 8}
HIP_ERROR_INVALID_VALUE = 1


class BadArgs(ValueError):
    pass


class HipError(RuntimeError):
    def __init__(self, what, code):
        RuntimeError.__init__(self, "%s: hipError_t %d" % (what, code))
        self.code = code


_vp, _u64, _i64, _u32, _i32 = C.c_void_p, C.c_uint64, C.c_int64, C.c_uint32, C.c_int
_LEAF = [_i32, _vp, _u64, _u64, _u64, _u64, _i64, _u64, _u64, _u32, _u32, _u32, _i32]
SYMBOLS = {
    "k3h_device_count": [],
    "k3h_leaf_chunks": _LEAF + [_vp, _u64, _u64],
    "k3h_leaf_finish": [_vp, _u32, _u64, _vp, _u64],
    "k3h_leaf_finish_nodes": [_vp, _u64, _vp, _vp, _u32, _u64, _u64, _u64, _vp, _u64, _i32],
    "k3h_leaf_tree_supported": [_u64, _u64, _u32, _u32, _u32],
    "k3h_leaf_tree": _LEAF + [_vp, _u64],
    "k3h_merkle_tree_from": [_vp, _u64, _u32, _vp],
    "k3h_gather_paths": [_vp, _u64, _u32, _vp, _u32, _vp],
}
_lib = None


def lib():
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise RuntimeError("%s is missing -- `make -C lcpc_amd/csrc` (or __graft_entry__.build()) builds it beside the product" % LIB_PATH)
        try:
            import torch  # noqa: F401  (its bundled HIP runtime must be the first one loaded: lcpc_amd/_lib.py)
        except ImportError:
            pass
        L = C.CDLL(LIB_PATH)
        for name, args in SYMBOLS.items():
            fn = getattr(L, name)
            fn.restype, fn.argtypes = _i32, args
        _lib = L
    return _lib


def _ptr(a):
    return None if a is None else a.ctypes.data_as(_vp)


def _words(a, n=None):
    assert a.dtype == np.uint32 and a.flags.c_contiguous and (n is None or a.size == n), (a.dtype, a.shape, n)
    return _ptr(a)


def _check(what, rc):
    if rc == -1:
        raise BadArgs(what)
    if rc:
        raise HipError(what, rc)


class Leaf:
    """every LeafArgs field but `out`: comm is a flat (comm_elems, L) uint64 array, element (r, c) at (r - row_base) row_stride + c col_stride"""

    def __init__(self, fid, comm, row_stride, col_stride, n_cols, row_base, n_rows_local, n_rows_total, chunk_begin, n_chunks_local,
                 n_chunks_total, canon_in):
        assert comm.dtype == np.uint64 and comm.flags.c_contiguous and comm.ndim == 2 and comm.shape[1] * 2 == NL[fid], (comm.dtype, comm.shape)
        self.fid, self.comm = fid, comm
        self.tail = (row_stride, col_stride, n_cols, row_base, n_rows_local, n_rows_total, chunk_begin, n_chunks_local, n_chunks_total,
                     int(canon_in))
        self.n_cols, self.n_chunks_local = n_cols, n_chunks_local

    def args(self):
        return (NL[self.fid], _ptr(self.comm), self.comm.shape[0]) + self.tail


def leaf_chunks(leaf, out, out_slot0=0):
    """out (out_slots, n_cols, 8) uint32 in / out: slots [out_slot0, out_slot0 + n_chunks_local) receive the CVs (one chunk in all: the digests)"""
    assert out.ndim == 3 and out.shape[1:] == (leaf.n_cols, 8)
    _check("k3h_leaf_chunks", lib().k3h_leaf_chunks(*leaf.args(), _words(out), out.shape[0], out_slot0))


def leaf_finish(cvs, digests):
    """cvs (n_chunks, n_cols, 8) in / out (clobbered: the kernel's stack); digests (>= n_cols, 8) in / out"""
    n_chunks, n_cols = cvs.shape[:2]
    _check("k3h_leaf_finish", lib().k3h_leaf_finish(_words(cvs, n_chunks * n_cols * 8), n_chunks, n_cols, _words(digests), digests.shape[0]))


def leaf_finish_nodes(cvs, node_slot, node_log, n_nodes, chunk0, n_chunks, out, root):
    """cvs (n_slots, n_cols, 8) in / out; node_slot / node_log: uint32 arrays of n_nodes or None; out (>= n_cols, 8) in / out"""
    n_slots, n_cols = cvs.shape[:2]
    for t in (node_slot, node_log):
        assert t is None or (t.dtype == np.uint32 and t.shape == (n_nodes,) and t.flags.c_contiguous)
    _check("k3h_leaf_finish_nodes", lib().k3h_leaf_finish_nodes(_words(cvs, n_slots * n_cols * 8), n_slots, _ptr(node_slot), _ptr(node_log),
                                                                n_nodes, chunk0, n_chunks, n_cols, _words(out), out.shape[0], int(root)))


def leaf_tree_supported(n_cols, np2, chunk_begin, n_chunks_local, n_chunks_total):
    return bool(lib().k3h_leaf_tree_supported(n_cols, np2, chunk_begin, n_chunks_local, n_chunks_total))


def leaf_tree(leaf, hashes, np2):
    """hashes (2 np2 - 1, 8) uint32 in / out: leaves and the first six levels"""
    _check("k3h_leaf_tree", lib().k3h_leaf_tree(*leaf.args(), _words(hashes, (2 * np2 - 1) * 8), np2))


def merkle_tree_from(hashes, np2, levels_done, root_out=None):
    """hashes (2 np2 - 1, 8) in / out; root_out (16,) uint32 in / out (the launcher is handed its first 8 words) or None"""
    _check("k3h_merkle_tree_from", lib().k3h_merkle_tree_from(_words(hashes, (2 * np2 - 1) * 8), np2, levels_done,
                                                              None if root_out is None else _words(root_out, 16)))


def gather_paths(hashes, np2, path_len, cols, paths):
    """cols (n,) uint64; paths (n, path_len, 8) in / out"""
    assert cols.dtype == np.uint64 and cols.flags.c_contiguous and paths.shape == (len(cols), path_len, 8)
    _check("k3h_gather_paths", lib().k3h_gather_paths(_words(hashes, (2 * np2 - 1) * 8), np2, path_len, _ptr(cols), len(cols), _words(paths)))

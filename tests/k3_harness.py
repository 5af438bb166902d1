"""ctypes side of tests/native/k3_harness.cpp (lcpc_amd/lib/liblcpc_k3_harness.so, built by lcpc_amd/csrc/Makefile): the BLAKE3 column-hash
(K3), Merkle-tree (K4) and path-gather launchers of lcpc_amd/csrc/kernels.h, and their batch forms, on buffers a test builds.  Elements cross as (.., L) uint64
arrays of limbs, digests and chaining values as (.., 8) uint32 arrays; in / out buffers are modified in place.  Every call returns
after the device has finished and raises on any hipError_t; BadArgs means the harness refused the call before touching the device."""
import ctypes as C

import numpy as np

import harness_kit as K
from harness_kit import BadArgs, HipError, check as _check, ptr as _ptr  # noqa: F401

LIB_PATH = K.lib_path("k3")
NL = {0: 2, 1: 4, 2: 6, 3: 8}
HIP_ERROR_INVALID_VALUE = 1


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
    "k3h_leaf_chunks_batch": _LEAF + [_vp, _u64, _u64, _u32, _u64, _u64],
    "k3h_leaf_tree_batch": _LEAF + [_vp, _u64, _u32, _u64, _u64, _u32],
    "k3h_leaf_finish_batch": [_vp, _u32, _u64, _u64, _vp, _u64, _u64, _u32],
    "k3h_merkle_tree_from_batch": [_vp, _u64, _u32, _u32, _u64, _vp],
    "k3h_batch_place": [_vp, _u64, _u64, _vp, _u64, _u64, _u32],
}


def lib():
    return K.load("k3", SYMBOLS)


def _words(a, n=None):
    assert a.dtype == np.uint32 and a.flags.c_contiguous and (n is None or a.size == n), (a.dtype, a.shape, n)
    return _ptr(a)


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


# ---- the batch forms (lcpc_amd/csrc/kernels.hip, BATCH = true).  A batched buffer is an (n_batch, stride) uint32 array -- member i in the first
# words of row i, its gap behind it -- and a stride is in 32-bit words, as kernels.h defines it
def batch_comm(comms, comm_stride, fill=0xFFFFFFFF):
    """the members' comms, (n_batch, comm_elems, L) uint64 (Leaf's layout per member) -> (n_batch, comm_stride) uint32, the gaps all ones:
    no reduced element, so a load that strays into a gap changes a digest"""
    assert comms.dtype == np.uint64 and comms.ndim == 3
    flat = np.ascontiguousarray(comms).reshape(comms.shape[0], -1).view(np.uint32)
    buf = np.full((comms.shape[0], comm_stride), fill, np.uint32)
    buf[:, :flat.shape[1]] = flat
    return buf


class LeafBatch:
    """Leaf for every member: `leaf` describes member 0's shape (its comm array stands for the element count only), `comm` is batch_comm's"""

    def __init__(self, leaf, comm):
        assert comm.dtype == np.uint32 and comm.ndim == 2 and comm.flags.c_contiguous
        self.leaf, self.comm, self.n_batch, self.comm_stride = leaf, comm, comm.shape[0], comm.shape[1]

    def args(self):
        return (NL[self.leaf.fid], _ptr(self.comm), self.leaf.comm.shape[0]) + self.leaf.tail


def _batched(a, n_batch):
    assert a.dtype == np.uint32 and a.ndim == 2 and a.shape[0] == n_batch and a.flags.c_contiguous, (a.dtype, a.shape, n_batch)
    return _ptr(a), a.shape[1]


def leaf_chunks_batch(lb, out, out_slots, out_slot0=0):
    """out (n_batch, out_stride) in / out: member i's out_slots x n_cols x 8 words in front of row i, of which slots
    [out_slot0, out_slot0 + n_chunks_local) receive the CVs"""
    p, out_stride = _batched(out, lb.n_batch)
    _check("k3h_leaf_chunks_batch", lib().k3h_leaf_chunks_batch(*lb.args(), p, out_slots, out_slot0, lb.n_batch, lb.comm_stride, out_stride))


def leaf_tree_batch(lb, hashes, np2, told=None):
    """hashes (n_batch, hashes_stride) in / out; told: the member count the launcher hears instead of n_batch (0 or above 65535 only)"""
    p, hashes_stride = _batched(hashes, lb.n_batch)
    _check("k3h_leaf_tree_batch", lib().k3h_leaf_tree_batch(*lb.args(), p, np2, lb.n_batch, lb.comm_stride, hashes_stride,
                                                            lb.n_batch if told is None else told))


def leaf_finish_batch(cvs, n_chunks, n_cols, digests, dig_cols):
    """cvs (n_batch, cvs_stride) in / out (the kernel's stack), digests (n_batch, digests_stride) in / out: dig_cols >= n_cols columns each"""
    n_batch = cvs.shape[0]
    pc, cvs_stride = _batched(cvs, n_batch)
    pd, dig_stride = _batched(digests, n_batch)
    _check("k3h_leaf_finish_batch", lib().k3h_leaf_finish_batch(pc, n_chunks, n_cols, cvs_stride, pd, dig_cols, dig_stride, n_batch))


def merkle_tree_from_batch(hashes, np2, levels_done, root_out=None):
    """hashes (n_batch, hashes_stride) in / out; root_out (n_batch + 1, 8) in / out -- the last row is no member's -- or None"""
    n_batch = hashes.shape[0]
    p, hashes_stride = _batched(hashes, n_batch)
    assert root_out is None or root_out.shape == (n_batch + 1, 8)
    _check("k3h_merkle_tree_from_batch", lib().k3h_merkle_tree_from_batch(p, np2, levels_done, n_batch, hashes_stride,
                                                                          None if root_out is None else _words(root_out)))


def batch_place(src, n_valid, dst, dst_stride):
    """src (n_batch, src_stride) uint64; dst flat uint64 of >= n_batch * dst_stride words, in / out"""
    for a in (src, dst):
        assert a.dtype == np.uint64 and a.flags.c_contiguous
    assert src.ndim == 2 and dst.ndim == 1
    _check("k3h_batch_place", lib().k3h_batch_place(_ptr(src), src.shape[1], n_valid, _ptr(dst), dst_stride, dst.size, src.shape[0]))

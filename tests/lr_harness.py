"""ctypes side of tests/native/lr_harness.cpp (lcpc_amd/lib/liblcpc_lr_harness.so, built by lcpc_amd/csrc/Makefile): the column hash of
SHA3-256 / Keccak-256 / SHA-256 / BLAKE2b -- resumable, one-shot and batched -- and their Merkle tree (launch_chain_* of
lcpc_amd/csrc/kernels.h) on buffers a test builds.  Elements cross as (.., L) uint64 arrays of limbs, the chaining state, the digests
and the hashes as flat uint32 arrays that are modified in place.  Every call returns after the device has finished and raises on any
hipError_t; BadArgs means the harness refused the call before touching the device."""
import ctypes as C

import numpy as np

import harness_kit as K
from harness_kit import BadArgs, HipError, check as _check, ptr as _ptr  # noqa: F401

LIB_PATH = K.lib_path("lr")
NL = {0: 2, 1: 4, 2: 6, 3: 8}
FAMILY = {"sha3_256": 0, "keccak256": 1, "sha256": 2, "blake2b": 3}
# per digest: 64-bit words of zero prefix, 64-bit words per block, 32-bit words of chaining state per column, 32-bit words per digest
SHAPE = {"sha3_256": (4, 17, 50, 8), "keccak256": (4, 17, 50, 8), "sha256": (4, 8, 8, 8), "blake2b": (8, 16, 16, 16)}


_vp, _u64, _i32, _u32 = C.c_void_p, C.c_uint64, C.c_int, C.c_uint32
SYMBOLS = {
    "lrh_device_count": (_i32, []),
    "lrh_leaf_blocks": (_u64, [_i32, _i32, _u64]),
    "lrh_leaf_range": (_i32, [_i32, _i32, _vp, _u64, _u64, _u64, _u64, _u64, _u64, _u64, _i32, _vp, _u64, _u64, _vp, _u64, _u64]),
    "lrh_leaves": (_i32, [_i32, _i32, _vp, _u64, _u64, _u64, _u64, _u64, _i32, _u32, _u64, _u64, _vp, _u64, _u64]),
    "lrh_merkle_tree": (_i32, [_i32, _u64, _u32, _u64, _vp, _u64, _u64, _vp, _u64, _u64]),
}


def lib():
    return K.load("lr", SYMBOLS)


def leaf_blocks(digest, fid, n_rows):
    """blocks of the whole leaf message, padding blocks included (0: refused)"""
    return int(lib().lrh_leaf_blocks(FAMILY[digest], NL[fid], n_rows))


def leaf_range(digest, fid, comm, row_stride, col_stride, n_cols, n_rows_total, blk_begin, blk_end, canon_in, state, state_off, out, out_off):
    """one launch of blocks [blk_begin, blk_end).  comm: flat (comm_elems, L) uint64, element (r, c) at r row_stride + c col_stride -- it
    has to hold the rows the range reads, no more.  state / out: flat uint32 arrays, in / out; the kernel's regions start at word
    state_off / out_off"""
    assert comm.dtype == np.uint64 and comm.flags.c_contiguous and comm.ndim == 2 and comm.shape[1] * 2 == NL[fid], (comm.dtype, comm.shape)
    for a in (state, out):
        assert a.dtype == np.uint32 and a.flags.c_contiguous and a.ndim == 1
    rc = lib().lrh_leaf_range(FAMILY[digest], NL[fid], comm.ctypes.data_as(_vp), comm.shape[0], row_stride, col_stride, n_cols, n_rows_total,
                              blk_begin, blk_end, int(canon_in), state.ctypes.data_as(_vp), state.size, state_off, out.ctypes.data_as(_vp),
                              out.size, out_off)
    if rc == -1:
        raise BadArgs("lrh_leaf_range")
    if rc:
        raise HipError("lrh_leaf_range", rc)


def leaves(digest, fid, comm, row_stride, col_stride, n_cols, n_rows_total, canon_in, out, out_off, n_batch=0, comm_stride=0, out_stride=0):
    """the whole column hash in one launch: the one-shot launcher (n_batch == 0) or the batch launcher over n_batch members.  comm: flat
    uint32 words of all members, member i starting comm_stride * i words in; its digests start at word out_off + i * out_stride of out"""
    assert comm.dtype == np.uint32 and comm.flags.c_contiguous and comm.ndim == 1
    assert out.dtype == np.uint32 and out.flags.c_contiguous and out.ndim == 1
    _check("lrh_leaves", lib().lrh_leaves(FAMILY[digest], NL[fid], comm.ctypes.data_as(_vp), comm.size, row_stride, col_stride, n_cols, n_rows_total,
                                          int(canon_in), n_batch, comm_stride, out_stride, out.ctypes.data_as(_vp), out.size, out_off))


def merkle_tree(digest, np2, hashes, hashes_off, root=None, root_off=0, n_batch=0, hashes_stride=0):
    """the tree above np2 leaf digests: the one-shot launcher (n_batch == 0) or the batch launcher.  hashes: flat uint32, member i's
    [2 np2 - 1][digest words] starting at word hashes_off + i * hashes_stride; root (None: a null root_out): member i's root at word
    root_off + i * digest words"""
    assert hashes.dtype == np.uint32 and hashes.flags.c_contiguous and hashes.ndim == 1
    assert root is None or (root.dtype == np.uint32 and root.flags.c_contiguous and root.ndim == 1)
    _check("lrh_merkle_tree", lib().lrh_merkle_tree(FAMILY[digest], np2, n_batch, hashes_stride, hashes.ctypes.data_as(_vp), hashes.size, hashes_off,
                                                    None if root is None else root.ctypes.data_as(_vp), 0 if root is None else root.size, root_off))

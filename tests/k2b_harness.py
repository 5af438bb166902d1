"""ctypes side of tests/native/k2b_harness.cpp (lcpc_amd/lib/liblcpc_k2b_harness.so, built by lcpc_amd/csrc/Makefile): the batch forms
of the position-major Brakedown launchers of lcpc_amd/csrc/kernels.h (launch_transpose_to_t_batch, launch_spmm_t_batch,
launch_sdig_rs_t_batch) on matrices and operands a test builds.  A batch buffer is an (n_batch, stride_elems, L) uint64 array: member
i's elements first, whatever the test put behind them (a sentinel) up to the stride; in / out buffers are modified in place.  The
launchers take member strides in 32-bit words: stride_elems * 2 L here.  Errors as in tests/harness_kit.py."""
import ctypes as C

import numpy as np

import harness_kit as K
from harness_kit import BadArgs, HipError, check as _check, ptr as _ptr  # noqa: F401
from k2_harness import NL, Csr, _elems, field_consts  # noqa: F401

LIB_PATH = K.lib_path("k2b")
HIP_SUCCESS, HIP_ERROR_INVALID_VALUE = 0, 1
TRANSPOSE, SPMM, SDIG_RS = 0, 1, 2

_vp, _u64, _u32, _i32 = C.c_void_p, C.c_uint64, C.c_uint32, C.c_int
SYMBOLS = {
    "k2bh_device_count": [],
    "k2bh_spmm_t": [_i32, _vp, _u32, _u64, _u64, _u64, _u64, _u64, _u64, _vp, _u64, _vp, _vp, _vp, _u64, _u64, _i32, _vp],
    "k2bh_sdig_rs_t": [_i32, _vp, _u64, _u32, _vp, _u64, _u64, _u64, _u32, _u64, _vp, _u32],
    "k2bh_transpose_to_t": [_i32, _vp, _u64, _u64, _u64, _u64, _vp, _u64, _u32, _u64, _vp, _i32],
    "k2bh_refusal": [_i32, _i32, _u32, _u64, _u64, _i32],
}


def lib():
    return K.load("k2b", SYMBOLS)


def _members(a, fid):
    """(pointer, n_batch, member stride in 32-bit words) of an (n_batch, stride_elems, L) buffer"""
    assert a.ndim == 3
    return _elems(a, fid), a.shape[0], a.shape[1] * NL[fid]


def spmm_t(fid, t, n_pos, n_rows, n_in, in_off, out_off, csr, limb, out_alt=None):
    """t (n_batch, stride_elems >= n_pos * n_rows, L) in / out; out_alt (n_batch, stride_elems >= m * n_rows, L) in / out or None"""
    tp, n_batch, t_stride = _members(t, fid)
    ap, ab, a_stride = _members(out_alt, fid) if out_alt is not None else (None, n_batch, 0)
    assert ab == n_batch
    rp, _ = field_consts(fid)
    _check("k2bh_spmm_t", lib().k2bh_spmm_t(NL[fid], tp, n_batch, t_stride, n_pos, n_rows, in_off, n_in, out_off, ap, a_stride,
                                            *csr.args(), int(limb), _ptr(rp) if limb else None))


def sdig_rs_t(fid, in_t, n_in, t, n_pos, n_rows, out_off, n_out):
    """in_t (n_batch, stride_elems >= n_in * n_rows, L); t (n_batch, stride_elems >= n_pos * n_rows, L) in / out"""
    ip, n_batch, in_stride = _members(in_t, fid)
    tp, tb, t_stride = _members(t, fid)
    assert tb == n_batch
    _, r2 = field_consts(fid)
    _check("k2bh_sdig_rs_t", lib().k2bh_sdig_rs_t(NL[fid], ip, in_stride, n_in, tp, t_stride, n_pos, out_off, n_out, n_rows, _ptr(r2), n_batch))


def transpose_to_t(fid, src, src_stride, n_valid, n_rows, t, n_src_total=None, copy_dst=None, canon=False):
    """src (src_elems, L) flat: the members' rows stacked; t (n_batch, stride_elems >= n_valid * n_rows, L) in / out; copy_dst like src,
    in / out, or None; n_src_total counts inside a member"""
    total = (1 << 64) - 1 if n_src_total is None else n_src_total
    tp, n_batch, t_stride = _members(t, fid)
    _check("k2bh_transpose_to_t", lib().k2bh_transpose_to_t(NL[fid], _elems(src, fid), src.shape[0], src_stride, n_valid, n_rows, tp, t_stride,
                                                            n_batch, total, None if copy_dst is None else _elems(copy_dst, fid, src.shape[0]),
                                                            int(canon)))


def refusal(which, fid, n_batch, n_rows, work=1, limb=True):
    """the hipError_t of a launcher on a job it must settle before any launch (null buffers; no device is touched); BadArgs when the
    job is one a correct launcher would launch"""
    rc = lib().k2bh_refusal(which, NL[fid], n_batch, n_rows, work, int(limb))
    if rc == -1:
        raise BadArgs("k2bh_refusal")
    return rc

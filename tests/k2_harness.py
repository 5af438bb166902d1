"""ctypes side of tests/native/k2_harness.cpp (lcpc_amd/lib/liblcpc_k2_harness.so, built by lcpc_amd/csrc/Makefile): the Brakedown (K2)
launchers of lcpc_amd/csrc/kernels.h on matrices and operands a test builds.  Elements cross as (n, L) uint64 arrays of stored
(Montgomery) limbs, like everywhere at the C ABI; in / out buffers are modified in place.  Every call returns after the device has
finished and raises on any hipError_t; BadArgs means the harness refused the call before touching the device."""
import ctypes as C

import numpy as np

import harness_kit as K
from harness_kit import BadArgs, HipError, check as _check, ptr as _ptr  # noqa: F401

LIB_PATH = K.lib_path("k2")
NL = {0: 2, 1: 4, 2: 6, 3: 8}
HIP_ERROR_INVALID_VALUE = 1


_vp, _u64, _u32, _i32 = C.c_void_p, C.c_uint64, C.c_uint32, C.c_int
SYMBOLS = {
    "k2h_device_count": [],
    "k2h_limb_form": [_i32, _vp, _u64, _vp, _vp],
    "k2h_spmv": [_i32, _vp, _u64, _u64, _u64, _u64, _u64, _vp, _u64, _vp, _vp, _vp, _u64, _u64, _i32, _vp],
    "k2h_spmm_t": [_i32, _vp, _u64, _u64, _u64, _u64, _u64, _vp, _vp, _vp, _vp, _u64, _u64, _i32, _vp],
    "k2h_sdig_rs": [_i32, _vp, _u64, _u32, _vp, _u64, _u64, _u32, _u64, _vp],
    "k2h_sdig_rs_t": [_i32, _vp, _u32, _vp, _u64, _u64, _u32, _u64, _vp],
    "k2h_transpose_to_t": [_i32, _vp, _u64, _u64, _u64, _u64, _vp, _u64, _vp, _i32],
    "k2h_transpose_from_t": [_i32, _vp, _u64, _u64, _vp, _u64],
    "k2h_pad_rows": [_i32, _vp, _u64, _vp, _u64, _u64, _u64],
}


def lib():
    return K.load("k2", SYMBOLS)


def _elems(a, fid, n=None):
    assert a.dtype == np.uint64 and a.flags.c_contiguous and a.shape[-1] * 2 == NL[fid], (a.dtype, a.shape)
    assert n is None or a.size == n * a.shape[-1], (a.shape, n)
    return _ptr(a)


def field_consts(fid):
    """(R' mod p, R^2 mod p) as (1, L) limb arrays: R = 2^(64 L), R' = 2^(N W) of field_ln.h (None for Ft63, which has no limb form
    in K2)"""
    from common import field_p, to_limbs, FIELD_L, LN_SHAPE
    p, L = field_p(fid), FIELD_L[fid]
    N, W = LN_SHAPE[fid]
    rp = to_limbs([pow(2, N * W, p)], L) if fid != 0 else None
    return rp, to_limbs([pow(2, 128 * L, p)], L)


class Csr:
    """CSR-by-output matrix: rowptr (m + 1), colidx (nnz), vals (nnz, L) stored limbs"""

    def __init__(self, fid, rowptr, colidx, vals):
        self.fid = fid
        self.rowptr = np.ascontiguousarray(rowptr, np.uint32)
        self.colidx = np.ascontiguousarray(colidx, np.uint32)
        self.vals = np.ascontiguousarray(vals, np.uint64).reshape(len(self.colidx), NL[fid] // 2)
        self.m, self.nnz = len(self.rowptr) - 1, len(self.colidx)

    def args(self):
        colidx = self.colidx if self.nnz else np.zeros(1, np.uint32)
        vals = self.vals if self.nnz else np.zeros((1, NL[self.fid] // 2), np.uint64)
        return _ptr(self.rowptr), _ptr(colidx), _ptr(vals), self.m, self.nnz


def limb_form(fid, vals):
    """the limb form ctx.cpp derives for matrix values: (n, stride) uint32"""
    from common import LN_STRIDE
    rp, _ = field_consts(fid)
    n = vals.shape[0]
    out = np.zeros((n, LN_STRIDE[fid]), np.uint32)
    _check("k2h_limb_form", lib().k2h_limb_form(NL[fid], _elems(vals, fid), n, _ptr(rp), _ptr(out)))
    return out


def spmv(fid, mat, n_in, in_off, out_off, csr, limb, out_alt=None):
    """mat (n_rows, stride, L) in / out; out_alt (n_rows, out_alt_stride, L) in / out or None"""
    n_rows, stride = mat.shape[:2]
    rp, _ = field_consts(fid)
    _check("k2h_spmv", lib().k2h_spmv(NL[fid], _elems(mat, fid), stride, n_rows, in_off, n_in, out_off,
                                      None if out_alt is None else _elems(out_alt, fid, n_rows * out_alt.shape[1]),
                                      0 if out_alt is None else out_alt.shape[1], *csr.args(), int(limb), _ptr(rp) if limb else None))


def spmm_t(fid, t, n_in, in_off, out_off, csr, limb, out_alt=None):
    """t (n_pos, n_rows, L) in / out; out_alt (m, n_rows, L) in / out or None"""
    n_pos, n_rows = t.shape[:2]
    rp, _ = field_consts(fid)
    _check("k2h_spmm_t", lib().k2h_spmm_t(NL[fid], _elems(t, fid), n_pos, n_rows, in_off, n_in, out_off,
                                          None if out_alt is None else _elems(out_alt, fid, csr.m * n_rows),
                                          *csr.args(), int(limb), _ptr(rp) if limb else None))


def sdig_rs(fid, inp, n_in, mat, out_off, n_out):
    """inp (n_rows, in_stride, L); mat (n_rows, stride, L) in / out"""
    n_rows, in_stride = inp.shape[:2]
    assert mat.shape[0] == n_rows
    _, r2 = field_consts(fid)
    _check("k2h_sdig_rs", lib().k2h_sdig_rs(NL[fid], _elems(inp, fid), in_stride, n_in, _elems(mat, fid), mat.shape[1], out_off, n_out,
                                            n_rows, _ptr(r2)))


def sdig_rs_t(fid, in_t, t, out_off, n_out):
    """in_t (n_in, n_rows, L); t (n_pos, n_rows, L) in / out"""
    n_in, n_rows = in_t.shape[:2]
    assert t.shape[1] == n_rows
    _, r2 = field_consts(fid)
    _check("k2h_sdig_rs_t", lib().k2h_sdig_rs_t(NL[fid], _elems(in_t, fid), n_in, _elems(t, fid), t.shape[0], out_off, n_out, n_rows,
                                                _ptr(r2)))


def transpose_to_t(fid, src, src_stride, n_valid, n_rows, t, n_src_total=None, copy_dst=None, canon=False):
    """src (src_elems, L) flat; t (n_valid, n_rows, L) in / out; copy_dst like src, in / out, or None"""
    total = (1 << 64) - 1 if n_src_total is None else n_src_total
    _check("k2h_transpose_to_t", lib().k2h_transpose_to_t(NL[fid], _elems(src, fid), src.shape[0], src_stride, n_valid, n_rows,
                                                          _elems(t, fid, n_valid * n_rows), total,
                                                          None if copy_dst is None else _elems(copy_dst, fid, src.shape[0]), int(canon)))


def transpose_from_t(fid, t, dst):
    """t (n_pos, n_rows, L); dst (n_rows, dst_stride, L) in / out"""
    n_pos, n_rows = t.shape[:2]
    assert dst.shape[0] == n_rows
    _check("k2h_transpose_from_t", lib().k2h_transpose_from_t(NL[fid], _elems(t, fid), n_pos, n_rows, _elems(dst, fid), dst.shape[1]))


def pad_rows(fid, src, dst, n_valid):
    """src (n_rows, src_stride, L); dst (n_rows, dst_stride, L) in / out"""
    assert src.shape[0] == dst.shape[0]
    _check("k2h_pad_rows", lib().k2h_pad_rows(NL[fid], _elems(src, fid), src.shape[1], _elems(dst, fid), dst.shape[1], n_valid,
                                              src.shape[0]))

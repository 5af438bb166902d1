"""ctypes side of tests/native/k14_harness.cpp (lcpc_amd/lib/liblcpc_k14_harness.so, built by lcpc_amd/csrc/Makefile): the coset
transform and the extension (K14, launch_coset_fft / launch_extend of lcpc_amd/csrc/kernels.h) with a tile size and with twiddle and
shift tables of the test's choice, and the launchers' refusals.  The tables are built here in Python bignum from the layout kernels.h
documents, so the kernels are held to tables the product's host code had no part in.  Errors as in tests/harness_kit.py."""
import ctypes as C

import numpy as np

import fft_cases as FC
import harness_kit as K
from harness_kit import BadArgs, HipError, check as _check, ptr as _ptr  # noqa: F401
import k12_harness as K12

LIB_PATH = K.lib_path("k14")
HIP_SUCCESS, HIP_ERROR_INVALID_VALUE = 0, 1
FORMS = FC.FORMS
CANARY, PAD = K.CANARY, K.PAD                      # the canary elements around an output: harness_kit.padded

_vp, _u64, _u32, _i32 = C.c_void_p, C.c_uint64, C.c_uint32, C.c_int
SYMBOLS = {
    "k14h_device_count": (_i32, []),
    "k14h_ext_src_log": (_u32, [_u64]),
    "k14h_ext_log_n": (_u32, [_u64, _u32]),
    "k14h_coset_fft": (_i32, [_i32, _i32, _u32, _u32, _u32, _vp, _vp, _u64, _u64, _i32, _vp, _vp, _u64, _vp]),
    "k14h_extend": (_i32, [_i32, _u64, _u32, _i32, _u32, _u32, _vp, _u64, _vp, _u64, _u64, _vp, _u64, _vp, _u64, _vp]),
    "k14h_coset_refusal": (_i32, [_i32, _i32, _u32, _u32, _u32, _u32, _u32, _i32]),
    "k14h_extend_refusal": (_i32, [_i32, _u64, _u32, _i32, _u32, _u32, _u32, _u32, _i32]),
}


def lib():
    return K.load("k14", SYMBOLS)


def ext_log_n(n_coeffs, log_m):
    return lib().k14h_ext_log_n(n_coeffs, log_m)


_tables = {}


def shift_table(fid, s, log_n, inverse):
    """the two-level shift table of kernels.h as (elems, L) limbs: t^i for i < 2^h, then c t^(i 2^h) for i < 2^(log_n - h); forward
    t = s, c = 1, inverse t = s^-1, c = n^-1"""
    key = (fid, s, log_n, inverse)
    if key not in _tables:
        F = FC.field(fid)
        h = K12.lib().k12h_tab_split(log_n)
        t = pow(s, -1, F.p) if inverse else s
        c = pow(1 << log_n, -1, F.p) if inverse else 1
        vals = [pow(t, i, F.p) for i in range(1 << h)] + [c * pow(t, i << h, F.p) % F.p for i in range(1 << (log_n - h))]
        assert len(vals) == K12.lib().k12h_tab_elems(log_n)
        _tables[key] = FC.mont(fid, vals)
    return _tables[key]


def run_coset(fid, form, log_n, log_tile, x, s, in_place=False):
    """launch_coset_fft on the device.  x: (n_vecs, 2^log_n, L) limbs, s: the canonical shift.  Returns (out of x's shape, launches);
    the canaries around the output must come back untouched, and so must the input of an out-of-place run"""
    F = FC.field(fid)
    x = np.ascontiguousarray(x, np.uint64).reshape(-1, 1 << log_n, F.L)
    inverse = form.startswith("ifft")
    tab, stab = K12.table(fid, log_n, inverse), shift_table(fid, s, log_n, inverse)
    buf = K.padded(x.shape[0] * x.shape[1], F.L)
    keep = x.copy()
    launches = C.c_uint32(0xFFFFFFFF)
    _check("k14h_coset_fft", lib().k14h_coset_fft(2 * F.L, FORMS.index(form), log_n, log_tile, x.shape[0], _ptr(x), _ptr(buf), buf.size * 2,
                                                  PAD * F.L * 2, int(in_place), _ptr(tab), _ptr(stab), tab.shape[0], C.byref(launches)))
    out = K.inner(buf)
    assert (x == keep).all(), "the input of the transform was written"
    return out.reshape(x.shape).copy(), launches.value


def run_extend(fid, coeffs, n_coeffs, log_m, order, log_tile, s):
    """launch_extend on the device.  coeffs: (n_vecs, 2^ceil(log2 n_coeffs), L) limbs of which the last vector is handed over only up
    to n_coeffs elements -- whatever the kernels read beyond the mask lies outside the device buffer.  Returns ((n_vecs, 2^log_m, L),
    launches)"""
    F = FC.field(fid)
    src_log = lib().k14h_ext_src_log(n_coeffs)
    c = np.ascontiguousarray(coeffs, np.uint64).reshape(-1, 1 << src_log, F.L)
    n_vecs = c.shape[0]
    flat = c.reshape(-1, F.L)[:((n_vecs - 1) << src_log) + n_coeffs].copy()
    keep = flat.copy()
    log_n = ext_log_n(n_coeffs, log_m)
    tab, stab = K12.table(fid, log_m, False), shift_table(fid, s, log_n, False)
    buf = K.padded((n_vecs << log_m), F.L)
    launches = C.c_uint32(0xFFFFFFFF)
    _check("k14h_extend", lib().k14h_extend(2 * F.L, n_coeffs, log_m, int(order == "natural"), log_tile, n_vecs, _ptr(flat), flat.size * 2,
                                            _ptr(buf), buf.size * 2, PAD * F.L * 2, _ptr(tab), tab.shape[0], _ptr(stab), stab.shape[0],
                                            C.byref(launches)))
    out = K.inner(buf)
    assert (flat == keep).all(), "the coefficients were written"
    return out.reshape(n_vecs, 1 << log_m, F.L).copy(), launches.value


def coset_refusal(nl, form, log_n, log_tile, n_vecs, null_mask=0, misalign=0, overlap=0):
    """the hipError_t of launch_coset_fft on a job it must settle before any launch (never-read buffers; no device is touched);
    BadArgs when the job is one a correct launcher would launch.  bits: 0 in, 1 out, 2 tab, 3 stab"""
    rc = lib().k14h_coset_refusal(nl, form, log_n, log_tile, n_vecs, null_mask, misalign, overlap)
    if rc == -1:
        raise BadArgs("k14h_coset_refusal")
    return rc


def extend_refusal(nl, n_coeffs, log_m, natural, log_tile, n_vecs, null_mask=0, misalign=0, overlap=0):
    """the same for launch_extend; bits: 0 coeffs, 1 out, 2 tab_m, 3 stab"""
    rc = lib().k14h_extend_refusal(nl, n_coeffs, log_m, natural, log_tile, n_vecs, null_mask, misalign, overlap)
    if rc == -1:
        raise BadArgs("k14h_extend_refusal")
    return rc

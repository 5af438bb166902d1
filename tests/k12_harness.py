"""ctypes side of tests/native/k12_harness.cpp (lcpc_amd/lib/liblcpc_k12_harness.so, built by lcpc_amd/csrc/Makefile): the
whole-vector transform (K12 / K13, launch_fft of lcpc_amd/csrc/kernels.h) with a tile size and a twiddle table of the test's choice,
the product's own stage split (fft_plan), and the launcher's refusals.  The two-level table is built here in Python bignum from the
layout kernels.h documents, so the kernels are held to a table the product's host code had no part in.  Errors as in
tests/harness_kit.py."""
import ctypes as C

import numpy as np

import fft_cases as FC
import harness_kit as K
from harness_kit import BadArgs, HipError, check as _check, ptr as _ptr  # noqa: F401

LIB_PATH = K.lib_path("k12")
HIP_SUCCESS, HIP_ERROR_INVALID_VALUE = 0, 1
FORMS = FC.FORMS                                    # the launcher's form numbers are lcpcf_form's
CANARY, PAD = K.CANARY, K.PAD                      # the canary elements around an output: harness_kit.padded

_vp, _u64, _u32, _i32 = C.c_void_p, C.c_uint64, C.c_uint32, C.c_int
SYMBOLS = {
    "k12h_device_count": (_i32, []),
    "k12h_max_log_tile": (_i32, []),
    "k12h_max_passes": (_i32, []),
    "k12h_tab_split": (_u32, [_u32]),
    "k12h_tab_elems": (_u64, [_u32]),
    "k12h_plan": (_i32, [_u32, _u32, _vp]),
    "k12h_fft": (_i32, [_i32, _i32, _u32, _u32, _u32, _vp, _vp, _u64, _u64, _i32, _vp, _u64, _vp, _vp]),
    "k12h_refusal": (_i32, [_i32, _i32, _u32, _u32, _u32, _u32, _u32]),
}


def lib():
    return K.load("k12", SYMBOLS)


def max_log_tile():
    return lib().k12h_max_log_tile()


def plan(log_n, log_tile):
    """the product's stage split, decimation-in-frequency order; None where the launcher refuses log_tile or log_n"""
    s = np.zeros(lib().k12h_max_passes(), np.uint32)
    n = lib().k12h_plan(log_n, log_tile, _ptr(s))
    return None if n < 0 else [int(v) for v in s[:n]]


_tables = {}


def table(fid, log_n, inverse):
    """the two-level table of kernels.h as (elems, L) limbs: v^i for i < 2^h, then v^(i 2^h) for i < 2^(log_n - h), v = w or w^-1"""
    key = (fid, log_n, inverse)
    if key not in _tables:
        F = FC.field(fid)
        h = lib().k12h_tab_split(log_n)
        v = FC.root(fid, log_n)
        if inverse:
            v = pow(v, -1, F.p)
        vals = [pow(v, i, F.p) for i in range(1 << h)] + [pow(v, i << h, F.p) for i in range(1 << (log_n - h))]
        assert len(vals) == lib().k12h_tab_elems(log_n) and len(vals) <= 1 << ((log_n + 1) // 2 + 1)
        _tables[key] = FC.mont(fid, vals)
    return _tables[key]


def run(fid, form, log_n, log_tile, x, in_place=False):
    """launch_fft on the device.  x: (n_vecs, 2^log_n, L) limbs.  Returns (out of x's shape, launches); the canaries in front of
    and behind the output must come back untouched, and so must the input of an out-of-place run"""
    F = FC.field(fid)
    x = np.ascontiguousarray(x, np.uint64).reshape(-1, 1 << log_n, F.L)
    n_vecs = x.shape[0]
    inverse = form.startswith("ifft")
    tab = table(fid, log_n, inverse)
    n_inv = FC.mont(fid, [pow(1 << log_n, -1, F.p)])
    buf = K.padded(x.shape[0] * x.shape[1], F.L)
    keep = x.copy()
    launches = C.c_uint32(0xFFFFFFFF)
    _check("k12h_fft", lib().k12h_fft(2 * F.L, FORMS.index(form), log_n, log_tile, n_vecs, _ptr(x), _ptr(buf), buf.size * 2, PAD * F.L * 2,
                                      int(in_place), _ptr(tab), tab.shape[0], _ptr(n_inv), C.byref(launches)))
    out = K.inner(buf)
    assert (x == keep).all()
    return out.reshape(x.shape).copy(), launches.value


def refusal(nl, form, log_n, log_tile, n_vecs, null_mask=0, misalign=0):
    """the hipError_t of the launcher on a job it must settle before any launch (never-read buffers; no device is touched); BadArgs
    when the job is one a correct launcher would launch.  null_mask: bit 0 in, 1 out, 2 tab, 3 n_inv; misalign: bit 0 in, 1 out, 2 tab"""
    rc = lib().k12h_refusal(nl, form, log_n, log_tile, n_vecs, null_mask, misalign)
    if rc == -1:
        raise BadArgs("k12h_refusal")
    return rc

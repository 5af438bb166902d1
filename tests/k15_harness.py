"""ctypes side of tests/native/k15_harness.cpp (lcpc_amd/lib/liblcpc_k15_harness.so, built by lcpc_amd/csrc/Makefile): the inverse,
pointwise and domain-quotient launchers (K15 / K16, launch_batch_inverse / launch_pointwise / launch_domain_quotient of
lcpc_amd/csrc/kernels.h) with canaries around the output, a twiddle table built here in Python bignum (tests/k12_harness.py's
builder), and the launchers' refusals.  Errors as in tests/harness_kit.py."""
import ctypes as C

import numpy as np

import fft_cases as FC
import harness_kit as K
from harness_kit import BadArgs, HipError, check as _check, ptr as _ptr  # noqa: F401
import k12_harness as K12

LIB_PATH = K.lib_path("k15")
HIP_SUCCESS, HIP_ERROR_INVALID_VALUE = 0, 1
CANARY, PAD = K.CANARY, K.PAD                      # the canary elements around an output: harness_kit.padded
OPS = {"inverse": -1, "add": 0, "sub": 1, "mul": 2, "div": 3}
KINDS = {"linear": 0, "vanishing": 1}

_vp, _u64, _u32, _i32 = C.c_void_p, C.c_uint64, C.c_uint32, C.c_int
SYMBOLS = {
    "k15h_device_count": (_i32, []),
    "k15h_cu_count": (_i32, []),
    "k15h_tile": (_u32, [_i32]),
    "k15h_pointwise": (_i32, [_i32, _i32, _vp, _vp, _u64, _vp, _u64, _u64, _i32]),
    "k15h_domain_quotient": (_i32, [_i32, _i32, _i32, _u32, _u32, _u32, _vp, _vp, _u64, _u64, _i32, _vp, _u64, _vp, _vp, _vp]),
    "k15h_pointwise_refusal": (_i32, [_i32, _i32, _u64, _u32, _u32, _i32]),
    "k15h_quotient_refusal": (_i32, [_i32, _i32, _u32, _u32, _u32, _u32, _u32, _i32]),
}


def lib():
    return K.load("k15", SYMBOLS)


def tile(nl):
    """the elements of a workgroup's tile"""
    return lib().k15h_tile(nl)


def cu_count():
    return lib().k15h_cu_count()


def run_pointwise(fid, op, a, b, in_place=0):
    """launch_pointwise (op "add" / "sub" / "mul" / "div") or launch_batch_inverse (op "inverse": a is None) on the device.  a, b:
    (n, L) limbs.  in_place: 1 the output is where a is, 2 where b is.  Returns the (n, L) output; the canaries around it must come
    back untouched, and so must every operand that is not the output"""
    F = FC.field(fid)
    b = np.ascontiguousarray(b, np.uint64).reshape(-1, F.L)
    a = None if a is None else np.ascontiguousarray(a, np.uint64).reshape(-1, F.L)
    keep_a, keep_b = None if a is None else a.copy(), b.copy()
    buf = K.padded(b.shape[0], F.L)
    _check("k15h_pointwise", lib().k15h_pointwise(2 * F.L, OPS[op], None if a is None else _ptr(a), _ptr(b), b.shape[0], _ptr(buf), buf.size * 2,
                                                  PAD * F.L * 2, in_place))
    out = K.inner(buf)
    assert (b == keep_b).all() and (a is None or (a == keep_a).all()), "an operand was written"
    return out.copy()


def run_quotient(fid, kind, order, log_m, log_n, vals, s, z=0, y=(), in_place=False):
    """launch_domain_quotient on the device.  vals: (n_vecs, 2^log_m, L) limbs; s: the canonical shift (None: the NULL shift of the
    linear kind); z canonical, y: n_vecs canonical ints.  Returns the output of vals' shape"""
    F = FC.field(fid)
    v = np.ascontiguousarray(vals, np.uint64).reshape(-1, 1 << log_m, F.L)
    keep = v.copy()
    tab = K12.table(fid, log_m, False)
    if kind == "vanishing":
        sl = FC.mont(fid, [pow(s, 1 << log_n, F.p)])
    else:
        sl = None if s is None else FC.mont(fid, [s])
    zl, yl = FC.mont(fid, [z]), FC.mont(fid, list(y) or [0])
    buf = K.padded(v.shape[0] * v.shape[1], F.L)
    _check("k15h_domain_quotient", lib().k15h_domain_quotient(2 * F.L, KINDS[kind], int(order == "bitrev"), log_m, log_n, v.shape[0], _ptr(v), _ptr(buf),
                                                              buf.size * 2, PAD * F.L * 2, int(in_place), _ptr(tab), tab.shape[0],
                                                              None if sl is None else _ptr(sl), _ptr(zl), _ptr(yl)))
    out = K.inner(buf)
    assert (v == keep).all(), "the input was written"
    return out.reshape(v.shape).copy()


def pointwise_refusal(nl, op, n, null_mask=0, misalign=0, overlap=0):
    """the hipError_t of launch_pointwise / launch_batch_inverse on a job it must settle before any launch (never-read buffers; no
    device is touched); BadArgs when the job is one a correct launcher would launch.  bits: 0 a, 1 b, 2 out"""
    rc = lib().k15h_pointwise_refusal(nl, OPS.get(op, op), n, null_mask, misalign, overlap)
    if rc == -1:
        raise BadArgs("k15h_pointwise_refusal")
    return rc


def quotient_refusal(nl, kind, log_m, log_n, n_vecs, null_mask=0, misalign=0, overlap=0):
    """the same for launch_domain_quotient; bits: 0 in, 1 out, 2 tab, 3 y, 4 shift, 5 z"""
    rc = lib().k15h_quotient_refusal(nl, KINDS.get(kind, kind), log_m, log_n, n_vecs, null_mask, misalign, overlap)
    if rc == -1:
        raise BadArgs("k15h_quotient_refusal")
    return rc

"""ctypes side of tests/native/fe_harness.cpp (lcpc_amd/lib/liblcpc_fe_harness.so, built by lcpc_amd/csrc/Makefile): every device field
primitive of lcpc_amd/csrc/field_dev.h / field_ln.h called once per lane on operands a test builds, and host_field.h's arithmetic.
Operands and results cross as Python ints: a packed element is one int < 2^(32 NL), a limb-form element a list of N signed limbs
(two's complement u32 on the device).  Every device call runs ONE launch over the whole list; the output buffer is pre-filled with a
sentinel and carries one spare element, which must come back untouched.  BadArgs means the harness refused the call before touching the
device; any hipError_t raises HipError."""
import ctypes as C
import os

import numpy as np

import harness_kit as K
from harness_kit import BadArgs, HipError, check as _check, ptr as _ptr  # noqa: F401

LIB_PATH = K.lib_path("fe")
NL = {0: 2, 1: 4, 2: 6, 3: 8}
SENTINEL = 0xA5C3F00D
WT_STRIDE = 96
OP_ADD, OP_SUB, OP_MUL, OP_CANON = 0, 1, 2, 3


_vp, _u64, _u32, _i32 = C.c_void_p, C.c_uint64, C.c_uint32, C.c_int
SYMBOLS = {
    "feh_device_count": [],
    "feh_binop": [_i32, _i32, _vp, _vp, _vp, _u32, _u32],
    "feh_canon": [_i32, _vp, _vp, _u32, _u32],
    "feh_reduce_once": [_i32, _vp, _vp, _vp, _u32, _u32],
    "feh_wide_dot": [_i32, _vp, _vp, _u32, _vp, _u32, _u32],
    "feh_from_packed": [_i32, _vp, _vp, _u32, _u32],
    "feh_to_packed": [_i32, _vp, _vp, _u32, _u32],
    "feh_normalize": [_i32, _vp, _vp, _u32, _u32],
    "feh_clamp_qa": [_i32, _vp, _vp, _vp, _vp, _u32, _u32],
    "feh_mul": [_i32, _vp, _vp, _vp, _u32, _u32],
    "feh_mul_u": [_i32, _vp, _vp, _u32, _vp, _u32, _u32],
    "feh_lazy_dot": [_i32, _vp, _vp, _u32, _u32, _vp, _u32, _u32],
    "feh_clamp9": [_i32, _vp, _vp, _vp, _u32, _u32],
    "feh_mul_r29": [_vp, _vp, _vp, _u32, _u32],
    "feh_canon_r29": [_vp, _vp, _u32, _u32],
    "feh_host_op": [_i32, _i32, _vp, _vp, _vp, _u64],
}
def available():
    return os.path.exists(LIB_PATH)


def lib():
    return K.load("fe", SYMBOLS)


# ---- Python ints <-> device words ---------------------------------------------------------------------------------------------------
def pack_words(vals, nw):
    """ints in [0, 2^(32 nw)) -> (n, nw) uint32, little-endian words"""
    try:
        buf = b"".join(v.to_bytes(4 * nw, "little") for v in vals)
    except OverflowError:
        raise AssertionError("a value outside [0, 2^%d)" % (32 * nw))
    return np.frombuffer(buf, "<u4").astype(np.uint32).reshape(len(vals), nw)


def unpack_words(arr):
    nb = 4 * arr.shape[1]
    buf = np.ascontiguousarray(arr, "<u4").tobytes()
    return [int.from_bytes(buf[i:i + nb], "little") for i in range(0, len(buf), nb)]


def pack_limbs(rows, N):
    """lists of N signed limbs (each in [-2^31, 2^32)) -> (n, N) uint32 two's complement"""
    a = np.array(rows, np.int64).reshape(len(rows), N)
    assert ((a >= -(1 << 31)) & (a < 1 << 32)).all()
    return (a & 0xFFFFFFFF).astype(np.uint32)


def unpack_limbs(arr, signed_top=True):
    """(n, N) uint32 -> lists of limbs: lower limbs as unsigned words, the top limb as a signed 32-bit value"""
    a = arr.astype(np.int64)
    if signed_top:
        a[:, -1] -= (a[:, -1] >> 31) << 32
    return a.tolist()


def _out(n, width):
    return np.full((n + 1, width), SENTINEL, np.uint32)


def _done(out, n):
    assert (out[n] == SENTINEL).all(), "the spare output element was written: %s" % [hex(int(x)) for x in out[n]]
    return out[:n]


# ---- packed layer -------------------------------------------------------------------------------------------------------------------
def binop(op, fid, a, b):
    nl, n = NL[fid], len(a)
    assert len(b) == n
    A, B, out = pack_words(a, nl), pack_words(b, nl), _out(n, nl)
    _check("feh_binop", lib().feh_binop(op, nl, _ptr(A), _ptr(B), _ptr(out), n, n + 1))
    return unpack_words(_done(out, n))


def canon(fid, a):
    nl, n = NL[fid], len(a)
    A, out = pack_words(a, nl), _out(n, nl)
    _check("feh_canon", lib().feh_canon(nl, _ptr(A), _ptr(out), n, n + 1))
    return unpack_words(_done(out, n))


def reduce_once(fid, t, top=None):
    """t: the low NL words; top: the top words (the (t, top) form) or None (the one-argument form)"""
    nl, n = NL[fid], len(t)
    T, out = pack_words(t, nl), _out(n, nl)
    TOP = None if top is None else np.array(top, np.uint32)
    assert TOP is None or TOP.shape == (n,)
    _check("feh_reduce_once", lib().feh_reduce_once(nl, _ptr(T), _ptr(TOP), _ptr(out), n, n + 1))
    return unpack_words(_done(out, n))


def wide_dot(fid, a, b, k):
    """a, b: n lists of k elements each"""
    nl, n = NL[fid], len(a)
    assert all(len(r) == k for r in a) and all(len(r) == k for r in b) and len(b) == n
    A = pack_words([v for r in a for v in r], nl)
    B = pack_words([v for r in b for v in r], nl)
    out = _out(n, nl)
    _check("feh_wide_dot", lib().feh_wide_dot(nl, _ptr(A), _ptr(B), k, _ptr(out), n, n + 1))
    return unpack_words(_done(out, n))


# ---- limb layer ---------------------------------------------------------------------------------------------------------------------
def from_packed(fid, N, a):
    n = len(a)
    A, out = pack_words(a, NL[fid]), _out(n, N)
    _check("feh_from_packed", lib().feh_from_packed(fid, _ptr(A), _ptr(out), n, n + 1))
    return unpack_limbs(_done(out, n), signed_top=False)


def to_packed(fid, N, rows):
    n = len(rows)
    A, out = pack_limbs(rows, N), _out(n, NL[fid])
    _check("feh_to_packed", lib().feh_to_packed(fid, _ptr(A), _ptr(out), n, n + 1))
    return unpack_words(_done(out, n))


def normalize(fid, N, rows):
    n = len(rows)
    A, out = pack_limbs(rows, N), _out(n, N)
    _check("feh_normalize", lib().feh_normalize(fid, _ptr(A), _ptr(out), n, n + 1))
    return unpack_limbs(_done(out, n))


def clamp_qa(fid, N, rows, nqp):
    """nqp: (64, STRIDE) uint32, the limb-wise negated table.  -> (limb rows, clamp_q's indices)"""
    n = len(rows)
    assert nqp.dtype == np.uint32 and nqp.shape[0] == 64 and nqp.flags.c_contiguous
    A, out, q = pack_limbs(rows, N), _out(n, N), _out(n, 1)
    _check("feh_clamp_qa", lib().feh_clamp_qa(fid, _ptr(A), _ptr(nqp), _ptr(out), _ptr(q), n, n + 1))
    return unpack_limbs(_done(out, n)), [int(x) for x in _done(q, n)[:, 0]]


def mul(fid, N, a, w):
    n = len(a)
    assert len(w) == n
    A, Wt, out = pack_limbs(a, N), pack_limbs(w, N), _out(n, N)
    _check("feh_mul", lib().feh_mul(fid, _ptr(A), _ptr(Wt), _ptr(out), n, n + 1))
    return unpack_limbs(_done(out, n))


def mul_u(fid, N, a, tabs):
    """tabs: lists of N^2 words; the 256 lanes of block b multiply by tabs[b % len(tabs)]"""
    n = len(a)
    Wt = np.zeros((len(tabs), WT_STRIDE), np.uint32)
    for i, t in enumerate(tabs):
        assert len(t) == N * N
        Wt[i, :N * N] = [x & 0xFFFFFFFF for x in t]
    A, out = pack_limbs(a, N), _out(n, N)
    _check("feh_mul_u", lib().feh_mul_u(fid, _ptr(A), _ptr(Wt), len(tabs), _ptr(out), n, n + 1))
    return unpack_limbs(_done(out, n))


def lazy_dot(fid, N, x, v, k, c):
    """x: n lists of k packed elements; v: n lists of k limb rows"""
    n = len(x)
    assert len(v) == n and all(len(r) == k for r in x) and all(len(r) == k for r in v)
    X = pack_words([e for r in x for e in r], NL[fid])
    V = pack_limbs([e for r in v for e in r], N) if n * k else np.zeros((0, N), np.uint32)
    out = _out(n, NL[fid])
    _check("feh_lazy_dot", lib().feh_lazy_dot(fid, _ptr(X), _ptr(V), k, c, _ptr(out), n, n + 1))
    return unpack_words(_done(out, n))


# ---- Ft255 only -----------------------------------------------------------------------------------------------------------------------
def clamp9(rows, qp, reduced=False):
    """qp: (64, 12) uint32, the (i - QOFF) p table.  reduced: ln::to_packed_reduced (packed ints) instead of ln::clamp (limb rows)"""
    n = len(rows)
    assert qp.dtype == np.uint32 and qp.shape == (64, 12) and qp.flags.c_contiguous
    A, out = pack_limbs(rows, 9), _out(n, 8 if reduced else 9)
    _check("feh_clamp9", lib().feh_clamp9(int(reduced), _ptr(A), _ptr(qp), _ptr(out), n, n + 1))
    return unpack_words(_done(out, n)) if reduced else unpack_limbs(_done(out, n))


def mul_r29(a, b):
    n = len(a)
    A, B, out = pack_words(a, 8), pack_limbs(b, 9), _out(n, 8)
    _check("feh_mul_r29", lib().feh_mul_r29(_ptr(A), _ptr(B), _ptr(out), n, n + 1))
    return unpack_words(_done(out, n))


def canon_r29(a):
    n = len(a)
    A, out = pack_words(a, 8), _out(n, 8)
    _check("feh_canon_r29", lib().feh_canon_r29(_ptr(A), _ptr(out), n, n + 1))
    return unpack_words(_done(out, n))


# ---- host_field.h -----------------------------------------------------------------------------------------------------------------------
def host_op(op, fid, a, b=None):
    L, n = NL[fid] // 2, len(a)

    def limbs(vals):
        return np.array([[(v >> (64 * k)) & ((1 << 64) - 1) for k in range(L)] for v in vals], np.uint64).reshape(-1, L)

    A, B, out = limbs(a), None if b is None else limbs(b), np.zeros((n, L), np.uint64)
    _check("feh_host_op", lib().feh_host_op(op, fid, _ptr(A), _ptr(B), _ptr(out), n))
    return [sum(int(x) << (64 * k) for k, x in enumerate(r)) for r in out]

"""Shared by tests/test_fft_abi.py, tests/test_gpu_k12_kernels.py and tests/test_gpu_fft.py: the six forms of include/lcpc_hip_fft.h
in Python bignum, their inputs, and the ctypes call of lcpcf_fft.  Everything is exact: canonical Python ints mod p, turned into
Montgomery limbs by ints_cases.reference.  The fast reference is oracle/pyref.py's fft_io (the oracle-pinned encoder transform) for
the forward direction and a transform of the same shape written here for any root; test_fft_abi.py holds both to the direct sum
X[k] = sum_j x[j] w^(jk) at the sizes where that is affordable."""
import ctypes as C
import random

import numpy as np

from lcpc_amd import _lib

import ints_cases as IC
import oracle_lib as O
import pyref as P

FIELDS = IC.FIELDS
FORMS = ("fft_ii", "fft_io", "fft_oi", "ifft_ii", "ifft_io", "ifft_oi")
# a form and the form that undoes it
PAIRS = (("fft_io", "ifft_oi"), ("fft_oi", "ifft_io"), ("fft_ii", "ifft_ii"), ("ifft_io", "fft_oi"), ("ifft_oi", "fft_io"), ("ifft_ii", "fft_ii"))
CANARY = 0x5A5A5A5A5A5A5A5A
ERR_ARG, ERR_STATE = -7, -8


def vp(a):
    return a.ctypes.data_as(C.c_void_p) if a is not None else None


def field(fid):
    return P.FIELDS[fid]


def mont(fid, vals):
    """(n, L) Montgomery limbs of canonical ints"""
    return IC.reference(fid, vals).reshape(len(vals), O.limbs(fid))


def canon(fid, limbs):
    """canonical ints of (n, L) Montgomery limbs"""
    F = field(fid)
    return [F.from_mont(v) for v in O.limbs_to_ints(np.asarray(limbs, np.uint64).reshape(-1, F.L))]


def rng(*key):
    return random.Random(repr(key))


def root(fid, log_n):
    """w = ROOT_OF_UNITY^(2^(S - log_n)), canonical"""
    F = field(fid)
    return pow(F.root_of_unity, 1 << (F.S - log_n), F.p)


def rev(i, bits):
    return P.bitrev(i, bits)


_revs = {}


def rev_table(log_n):
    if log_n not in _revs:
        _revs[log_n] = [rev(i, log_n) for i in range(1 << log_n)]
    return _revs[log_n]


def permute(v, log_n):
    """out[rev(i)] = v[i] (its own inverse)"""
    assert len(v) == 1 << log_n
    return [v[j] for j in rev_table(log_n)]


def dft_direct(fid, x, inverse=False):
    """X[k] = sum_j x[j] v^(jk) by the sum itself, natural order both ways; inverse: v = w^-1 and the factor n^-1"""
    F = field(fid)
    n = len(x)
    log_n = n.bit_length() - 1
    v = root(fid, log_n)
    if inverse:
        v = pow(v, -1, F.p)
    pw = [pow(v, i, F.p) for i in range(n)]
    out = [sum(x[j] * pw[j * k % n] for j in range(n)) % F.p for k in range(n)]
    return [o * pow(n, -1, F.p) % F.p for o in out] if inverse else out


def dft(fid, x, inverse=False):
    """the same in O(n log n): decimation in frequency with root v, then the permutation"""
    F = field(fid)
    n = len(x)
    log_n = n.bit_length() - 1
    v = root(fid, log_n)
    if inverse:
        v = pow(v, -1, F.p)
    roots = [1] * max(1, n // 2)
    for i in range(1, len(roots)):
        roots[i] = roots[i - 1] * v % F.p
    out = permute(P.fft_io(F, list(x), roots), log_n)
    return [o * pow(n, -1, F.p) % F.p for o in out] if inverse else out


def apply_form(fid, form, x, transform=dft):
    """the form's definition: the input read in its order, the transform in natural order, the output stored in its order"""
    log_n = len(x).bit_length() - 1
    nat_in = permute(x, log_n) if form[-2] == "o" else list(x)
    y = transform(fid, nat_in, inverse=form.startswith("ifft"))
    return permute(y, log_n) if form[-1] == "o" else y


def random_vector(fid, log_n, *key):
    """canonical ints: random elements with 0, 1 and p - 1 among them where there is room"""
    F = field(fid)
    rnd = rng("fft", fid, log_n, *key)
    x = [rnd.randrange(F.p) for _ in range(1 << log_n)]
    for v in (0, 1, F.p - 1):
        if len(x) >= 8:
            x[rnd.randrange(len(x))] = v
    return x


_pairs = {}


def pair(fid, log_n, *key):
    """(x, X): a random vector and its forward transform, both natural, canonical ints -- every form's input and output is one of
    the two or its permutation (io_of).  Computed once per key and never changed"""
    k = (fid, log_n) + key
    if k not in _pairs:
        x = random_vector(fid, log_n, *key)
        _pairs[k] = (tuple(x), tuple(dft(fid, x)))
    return _pairs[k]


def io_of(form, x, X):
    """(input, expected output) of `form` from a natural pair x, X = DFT(x)"""
    log_n = len(x).bit_length() - 1
    a, b = (X, x) if form.startswith("ifft") else (x, X)
    return (permute(a, log_n) if form[-2] == "o" else list(a)), (permute(b, log_n) if form[-1] == "o" else list(b))


def host_fft(fid, form, x_limbs, log_n, out=None, expect=0):
    """lcpcf_fft with a canary-filled output (or `out`, for the in-place call): rc checked -> the n output elements"""
    L = x_limbs.shape[-1]
    n = 1 << log_n
    f = _lib.FFT_FORMS[form] if isinstance(form, str) else form
    if out is not None:
        assert _lib.lib().lcpcf_fft(fid, f, vp(x_limbs), vp(out), log_n) == expect
        return out
    buf = np.full((n + 2, L), CANARY, np.uint64)
    rc = _lib.lib().lcpcf_fft(fid, f, vp(x_limbs), vp(buf), log_n)
    assert rc == expect, rc
    assert (buf[n:] == CANARY).all()
    if expect:
        assert (buf == CANARY).all(), "an output was written on an error"
    return buf[:n]

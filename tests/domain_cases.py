"""Shared by tests/test_domain_abi.py, tests/test_gpu_k14_kernels.py and tests/test_gpu_domain.py: the coset forms and the extension of
include/lcpc_hip_domain.h in Python bignum, over tests/fft_cases.py, and the ctypes calls of the host entry points with canary-filled
outputs.  Everything is exact: canonical Python ints mod p."""
import numpy as np

from lcpc_amd import _lib

import fft_cases as FC

FIELDS = FC.FIELDS
FORMS = FC.FORMS
PAIRS = FC.PAIRS
CANARY = FC.CANARY
ERR_ARG, ERR_STATE = FC.ERR_ARG, FC.ERR_STATE
GENERATORS = {0: 10, 1: 3, 2: 5, 3: 5}              # PrimeFieldGenerator of the four test fields
ORDERS = ("natural", "bitrev")
vp = FC.vp


def shifts(fid, *key):
    """name -> canonical shift: 1, the generator, p - 1 and one seeded random element"""
    F = FC.field(fid)
    return {"one": 1, "gen": GENERATORS[fid], "minus_one": F.p - 1, "random": FC.rng("shift", fid, *key).randrange(2, F.p - 1)}


def shift_limbs(fid, s):
    return FC.mont(fid, [s])[0].copy()


def scale(fid, x, t):
    """x[j] t^j"""
    F = FC.field(fid)
    out, pw = [], 1
    for v in x:
        out.append(v * pw % F.p)
        pw = pw * t % F.p
    return out


def coset_direct(fid, x, s, inverse=False):
    """the definitions themselves, natural order both ways: X[k] = sum_j x[j] s^j w^(jk); x[j] = s^-j n^-1 sum_k X[k] w^(-jk)"""
    F = FC.field(fid)
    n = len(x)
    w = FC.root(fid, n.bit_length() - 1)
    if not inverse:
        sp = [pow(s, j, F.p) for j in range(n)]
        wp = [pow(w, i, F.p) for i in range(n)]
        return [sum(x[j] * sp[j] * wp[j * k % n] for j in range(n)) % F.p for k in range(n)]
    si, ni = pow(s, -1, F.p), pow(n, -1, F.p)
    wip = [pow(w, -i % n, F.p) for i in range(n)]
    return [pow(si, j, F.p) * ni * sum(x[k] * wip[j * k % n] for k in range(n)) % F.p for j in range(n)]


def coset_dft(fid, x, s, inverse=False):
    """the same through fft_cases.dft on the vector scaled beforehand (forward) or afterwards (inverse)"""
    F = FC.field(fid)
    if not inverse:
        return FC.dft(fid, scale(fid, x, s))
    return scale(fid, FC.dft(fid, x, inverse=True), pow(s, -1, F.p))


def apply_form(fid, form, x, s, transform=coset_dft):
    log_n = len(x).bit_length() - 1
    nat_in = FC.permute(x, log_n) if form[-2] == "o" else list(x)
    y = transform(fid, nat_in, s, inverse=form.startswith("ifft"))
    return FC.permute(y, log_n) if form[-1] == "o" else y


def extend_horner(fid, coeffs, s, log_m, order="natural"):
    """Y[k] = p(s w_m^k) by Horner's rule; order "bitrev": Y[k] at [rev_m(k)]"""
    F = FC.field(fid)
    w = FC.root(fid, log_m)
    out = []
    for k in range(1 << log_m):
        z, acc = s * pow(w, k, F.p) % F.p, 0
        for c in reversed(coeffs):
            acc = (acc * z + c) % F.p
        out.append(acc)
    return FC.permute(out, log_m) if order == "bitrev" else out


def extend_fast(fid, coeffs, s, log_m, order="natural"):
    """the same in O(m log m): the transform of the scaled, zero-padded coefficients"""
    y = FC.dft(fid, scale(fid, list(coeffs), s) + [0] * ((1 << log_m) - len(coeffs)))
    return FC.permute(y, log_m) if order == "bitrev" else y


def ceil_log2(n):
    return (n - 1).bit_length()


def host_generator(fid):
    out = np.full(FC.field(fid).L + 1, CANARY, np.uint64)
    assert _lib.lib().lcpcd_generator(fid, vp(out)) == 0 and out[-1] == CANARY
    return out[:-1].copy()


def host_coset_fft(fid, form, shift_limbs_, x_limbs, log_n, out=None, expect=0):
    """lcpcd_coset_fft with a canary-filled output (or `out`, for the in-place call): rc checked -> the n output elements"""
    L = x_limbs.shape[-1]
    n = 1 << log_n
    f = _lib.FFT_FORMS[form] if isinstance(form, str) else form
    if out is not None:
        assert _lib.lib().lcpcd_coset_fft(fid, f, vp(shift_limbs_), vp(x_limbs), vp(out), log_n) == expect
        return out
    buf = np.full((n + 2, L), CANARY, np.uint64)
    rc = _lib.lib().lcpcd_coset_fft(fid, f, vp(shift_limbs_), vp(x_limbs), vp(buf), log_n)
    assert rc == expect, rc
    assert (buf[n:] == CANARY).all()
    if expect:
        assert (buf == CANARY).all(), "an output was written on an error"
    return buf[:n]


def host_extend(fid, shift_limbs_, c_limbs, n_coeffs, log_m, order, expect=0, room=None):
    """lcpcd_extend into a canary-filled buffer -> the m output elements"""
    L = np.asarray(c_limbs).shape[-1]
    m = room if room is not None else 1 << log_m
    o = _lib.DOMAIN_ORDERS[order] if isinstance(order, str) else order
    buf = np.full((m + 2, L), CANARY, np.uint64)
    rc = _lib.lib().lcpcd_extend(fid, vp(shift_limbs_), vp(c_limbs), n_coeffs, log_m, o, vp(buf))
    assert rc == expect, rc
    assert (buf[m:] == CANARY).all()
    if expect:
        assert (buf == CANARY).all(), "an output was written on an error"
    return buf[:m]

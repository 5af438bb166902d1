"""Shared by tests/test_eval_abi.py and tests/test_gpu_eval.py: the bases of include/lcpc_hip_eval.h in Python bignum -- tensors of a
point, the weight of a coefficient, the value of a polynomial -- and the ctypes call of lcpce_tensors.  Everything is exact: canonical
Python ints mod p, turned into Montgomery limbs by ints_cases.reference."""
import ctypes as C
import random

import numpy as np

from lcpc_amd import _lib

import ints_cases as IC
import oracle_lib as O

FIELDS = IC.FIELDS
BASES = ("powers", "ml_monomial", "ml_lagrange")
ML_BASES = BASES[1:]
CANARY = 0x5A5A5A5A5A5A5A5A


def vp(a):
    return a.ctypes.data_as(C.c_void_p) if a is not None else None


def mont(fid, vals):
    """(n, L) Montgomery limbs of canonical ints"""
    return IC.reference(fid, vals).reshape(len(vals), O.limbs(fid))


def canon(fid, limbs):
    """canonical ints of (n, L) Montgomery limbs"""
    p = IC.modulus(fid)
    rinv = pow(1 << (64 * O.limbs(fid)), -1, p)
    return [v * rinv % p for v in O.limbs_to_ints(np.asarray(limbs, np.uint64).reshape(-1, O.limbs(fid)))]


def log2(n):
    assert n >= 1 and n & (n - 1) == 0
    return n.bit_length() - 1


def n_point(basis, n_rows, n_per_row):
    return 1 if basis == "powers" else log2(n_rows) + log2(n_per_row)


def random_point(basis, fid, n_rows, n_per_row, rnd):
    """canonical ints: one x, or one z_k per variable drawn from {0, 1, p - 1, random}"""
    p = IC.modulus(fid)
    if basis == "powers":
        return [rnd.randrange(p)]
    return [rnd.choice((0, 1, p - 1, rnd.randrange(p), rnd.randrange(p))) for _ in range(n_point(basis, n_rows, n_per_row))]


def expand_ref(basis, p, zs, n):
    """[prod_k (bit k of i ? hi_k : lo_k) for i < n] over the variables zs, canonical ints"""
    out = [1]
    for z in zs:
        lo = (1 - z) % p if basis == "ml_lagrange" else 1
        out = [v * lo % p for v in out] + [v * z % p for v in out]
    assert len(out) == n
    return out


def tensors_ref(basis, fid, point, n_rows, n_per_row):
    """(outer, inner) as canonical ints"""
    p = IC.modulus(fid)
    if basis == "powers":
        x = point[0]
        return [pow(x, r * n_per_row, p) for r in range(n_rows)], [pow(x, j, p) for j in range(n_per_row)]
    a = log2(n_per_row)
    return expand_ref(basis, p, point[a:], n_rows), expand_ref(basis, p, point[:a], n_per_row)


def eval_ref(basis, fid, coeffs, point, n_rows, n_per_row):
    """sum_e coeffs[e] * w(e) mod p for canonical coefficients (a short last row counts as zeros)"""
    p = IC.modulus(fid)
    outer, inner = tensors_ref(basis, fid, point, n_rows, n_per_row)
    acc = 0
    for e, c in enumerate(coeffs):
        acc += c * outer[e // n_per_row] * inner[e % n_per_row]
    return acc % p


def host_tensors(fid, basis, point_limbs, n_pt, n_rows, n_per_row, want_outer=True, want_inner=True, expect=0):
    """lcpce_tensors with canary-filled outputs: (rc checked) -> (outer, inner) arrays incl. 2 canary elements behind each"""
    L = O.limbs(fid)
    outer = np.full((n_rows + 2, L), CANARY, np.uint64)
    inner = np.full((n_per_row + 2, L), CANARY, np.uint64)
    rc = _lib.lib().lcpce_tensors(fid, _lib.EVAL_BASES[basis] if isinstance(basis, str) else basis, vp(point_limbs), n_pt, n_rows, n_per_row,
                                  vp(outer) if want_outer else None, vp(inner) if want_inner else None)
    assert rc == expect, rc
    assert (outer[n_rows:] == CANARY).all() and (inner[n_per_row:] == CANARY).all()
    return outer[:n_rows], inner[:n_per_row]


def rng(*key):
    return random.Random(repr(key))

"""Shared by tests/test_ints_abi.py and tests/test_gpu_ints.py: the integer kinds of include/lcpc_hip_ints.h, their edge values and
the bignum reference of a conversion -- (v % p) * R % p as limbs, p from the oracle's field_info."""
import random

import numpy as np

import oracle_lib as O

KINDS = ("u32", "i32", "u64", "i64", "wide")
DTYPES = {"u32": np.uint32, "i32": np.int32, "u64": np.uint64, "i64": np.int64}
FIELDS = (0, 1, 2, 3)


def modulus(fid):
    return O.limbs_to_ints(O.field_info(fid)["modulus"].reshape(1, -1))[0]


def value_range(kind, L):
    """[lo, hi] of one integer of `kind`"""
    if kind == "wide":
        return 0, (1 << (64 * L)) - 1
    bits = 32 if kind in ("u32", "i32") else 64
    return (-(1 << (bits - 1)), (1 << (bits - 1)) - 1) if kind[0] == "i" else (0, (1 << bits) - 1)


def edges(kind, fid):
    """the edge set E(kind): 0, 1, 2^29 - 1, 2^29, 2^32 - 1; signed kinds -1, min, max; 64-bit kinds with Ft63 p - 1, p, p + 1, 2^63,
    2^64 - 1; WIDE p - 1, p, p + 1, 2p, 2^(64 L) - 1 and a value whose low limb alone is all ones -- each where the kind can hold it"""
    L = O.limbs(fid)
    p = modulus(fid)
    lo, hi = value_range(kind, L)
    e = [0, 1, (1 << 29) - 1, 1 << 29, (1 << 32) - 1]
    if kind[0] == "i":
        e += [-1, lo, hi]
    if kind in ("u64", "i64") and fid == 0:
        e += [p - 1, p, p + 1, 1 << 63, (1 << 64) - 1]
    if kind == "wide":
        e += [p - 1, p, p + 1, 2 * p, (1 << (64 * L)) - 1, (1 << 64) - 1]
    return [v for v in e if lo <= v <= hi]


def random_values(kind, fid, n, seed):
    lo, hi = value_range(kind, O.limbs(fid))
    rnd = random.Random(seed)
    return [rnd.randint(lo, hi) for _ in range(n)]


def pack(kind, vals, L):
    """Python ints -> the array a caller of `kind` holds ((n,) of the kind's dtype; wide: (n, L) uint64)"""
    if kind == "wide":
        return O.ints_to_limbs(vals, L)
    return np.array(vals, dtype=object).astype(DTYPES[kind]) if len(vals) else np.zeros(0, DTYPES[kind])


def reference(fid, vals):
    """(n, L) Montgomery limbs of v mod p, by Python bignum"""
    L = O.limbs(fid)
    p = modulus(fid)
    R = 1 << (64 * L)
    return O.ints_to_limbs([(v % p) * R % p for v in vals], L)

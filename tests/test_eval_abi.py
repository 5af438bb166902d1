"""The evaluation extension of the C ABI (include/lcpc_hip_eval.h): its own prefix, table and version, exported by the product library
next to the core ABI, and its host call -- no device is touched here -- against Python bignum."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import lcpc_amd
from lcpc_amd import _lib

import eval_cases as EC
import ints_cases as IC
import oracle_lib as O
from common import powers

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "lcpc_hip_eval.h")
ERR_ARG = -7
vp = EC.vp

POWERS_SHAPES = ((1, 1), (1, 7), (5, 1), (3, 6), (17, 64), (130, 96))
ML_SHAPES = ((1, 1), (1, 8), (8, 1), (4, 16), (64, 32))


def declarations():
    return re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)


def test_header_symbols_equal_the_table_and_the_exports():
    syms = sorted(set(re.findall(r"\b(lcpce_[a-z0-9_]+)\s*\(", declarations())))
    assert syms == sorted(_lib.EVAL_SYMBOLS) and "lcpce_eval" in syms and len(syms) == 7
    L = _lib.lib()
    for s in syms:
        assert hasattr(L, s), "missing export: " + s
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert sorted(l.split()[2] for l in out.splitlines() if " T lcpce_" in l) == syms
    for other in (_lib.SYMBOLS, _lib.BATCH_SYMBOLS, _lib.VERIFY_SYMBOLS, _lib.COLUMNS_SYMBOLS, _lib.INTS_SYMBOLS):
        assert not set(_lib.EVAL_SYMBOLS) & set(other)


def test_version_and_bases():
    hdr = open(HEADER).read()
    assert _lib.lib().lcpce_version() == int(re.search(r"#define LCPCE_VERSION (\d+)", hdr).group(1)) == _lib.EVAL_VERSION
    assert sorted(_lib.EVAL_BASES) == sorted(EC.BASES)
    for name, k in _lib.EVAL_BASES.items():
        assert int(re.search(r"LCPCE_%s = (\d+)" % name.upper(), hdr).group(1)) == k


def test_header_adds_nothing_to_the_core_abi():
    """no text of the header, comments included, matches the pattern the core ABI's pins count"""
    assert not re.findall(r"\blcpc_[a-z0-9_]+\s*\(", open(HEADER).read())
    assert '#include "lcpc_hip.h"' in declarations() and "LCPC_ABI_VERSION" not in declarations()
    assert _lib.lib().lcpc_abi_version() == 5 and len(_lib.SYMBOLS) == 58


@pytest.mark.parametrize("fid", EC.FIELDS)
def test_powers_against_bignum(fid):
    """outer[r] = x^(r n_per_row), inner[j] = x^j by pow(), and the limbs of the sequential chain the tests' helper builds"""
    p = IC.modulus(fid)
    for n_rows, n_per_row in POWERS_SHAPES:
        for x in (0, 1, 2, p - 1, EC.rng("powers", fid, n_rows, n_per_row).randrange(p)):
            outer, inner = EC.host_tensors(fid, "powers", EC.mont(fid, [x]), 1, n_rows, n_per_row)
            wo, wi = EC.tensors_ref("powers", fid, [x], n_rows, n_per_row)
            assert (outer == EC.mont(fid, wo)).all() and (inner == EC.mont(fid, wi)).all(), (n_rows, n_per_row, x)
            assert (inner == powers(O, fid, x, n_per_row)).all()
            assert (outer == powers(O, fid, x, n_rows, n_per_row)).all()


@pytest.mark.parametrize("fid", EC.FIELDS)
def test_powers_exponents_above_32_bits(fid):
    n_rows, n_per_row = 5000, 1 << 20
    assert (n_rows - 1) * n_per_row > 1 << 32
    p = IC.modulus(fid)
    rnd = EC.rng("big", fid)
    x = rnd.randrange(p)
    outer, inner = EC.host_tensors(fid, "powers", EC.mont(fid, [x]), 1, n_rows, n_per_row)
    rows = sorted({0, 1, 2, 4095, 4096, 4097, n_rows - 2, n_rows - 1} | {rnd.randrange(n_rows) for _ in range(24)})
    assert (outer[rows] == EC.mont(fid, [pow(x, r * n_per_row, p) for r in rows])).all()
    cols = sorted({0, 1, 255, 256, 65535, 65536, n_per_row - 1} | {rnd.randrange(n_per_row) for _ in range(24)})
    assert (inner[cols] == EC.mont(fid, [pow(x, j, p) for j in cols])).all()


@pytest.mark.parametrize("fid", EC.FIELDS)
@pytest.mark.parametrize("basis", EC.ML_BASES)
def test_multilinear_against_bignum(fid, basis):
    """both tensors = the product over the bits of the index, variable k = bit k of e: inner from z_0.., outer from z_a.."""
    for n_rows, n_per_row in ML_SHAPES:
        for trial in range(4):
            pt = EC.random_point(basis, fid, n_rows, n_per_row, EC.rng(basis, fid, n_rows, n_per_row, trial))
            outer, inner = EC.host_tensors(fid, basis, EC.mont(fid, pt) if pt else None, len(pt), n_rows, n_per_row)
            wo, wi = EC.tensors_ref(basis, fid, pt, n_rows, n_per_row)
            assert (outer == EC.mont(fid, wo)).all() and (inner == EC.mont(fid, wi)).all(), (n_rows, n_per_row, pt)
            # the weight of coefficient e, straight from the definition
            p = IC.modulus(fid)
            co, ci = EC.canon(fid, outer), EC.canon(fid, inner)
            n = n_rows * n_per_row
            for e in {0, min(1, n - 1), n_per_row - 1, n - 1, n // 3}:
                w = 1
                for k, z in enumerate(pt):
                    w = w * (z if (e >> k) & 1 else ((1 - z) % p if basis == "ml_lagrange" else 1)) % p
                assert co[e // n_per_row] * ci[e % n_per_row] % p == w


@pytest.mark.parametrize("fid", EC.FIELDS)
def test_lagrange_indicators_and_partition_of_unity(fid):
    p = IC.modulus(fid)
    one = EC.mont(fid, [1])[0]
    for n_rows, n_per_row in ML_SHAPES:
        a, nv = EC.log2(n_per_row), EC.n_point("ml_lagrange", n_rows, n_per_row)
        rnd = EC.rng("ind", fid, n_rows, n_per_row)
        for e in {0, n_rows * n_per_row - 1, rnd.randrange(n_rows * n_per_row)}:
            pt = [(e >> k) & 1 for k in range(nv)]
            outer, inner = EC.host_tensors(fid, "ml_lagrange", EC.mont(fid, pt) if pt else None, nv, n_rows, n_per_row)
            for t, hot in ((outer, e >> a), (inner, e & (n_per_row - 1))):
                assert (t[hot] == one).all() and (np.delete(t, hot, axis=0) == 0).all()
        pt = [rnd.randrange(p) for _ in range(nv)]
        outer, inner = EC.host_tensors(fid, "ml_lagrange", EC.mont(fid, pt) if pt else None, nv, n_rows, n_per_row)
        assert sum(EC.canon(fid, outer)) % p == 1 and sum(EC.canon(fid, inner)) % p == 1


def test_either_output_may_be_null():
    for fid in EC.FIELDS:
        for basis, (n_rows, n_per_row) in (("powers", (17, 64)), ("ml_monomial", (4, 16)), ("ml_lagrange", (64, 32))):
            pt = EC.random_point(basis, fid, n_rows, n_per_row, EC.rng("null", fid, basis))
            pl = EC.mont(fid, pt)
            outer, inner = EC.host_tensors(fid, basis, pl, len(pt), n_rows, n_per_row)
            o2, i2 = EC.host_tensors(fid, basis, pl, len(pt), n_rows, n_per_row, want_inner=False)
            assert (o2 == outer).all() and (i2 == EC.CANARY).all()
            o3, i3 = EC.host_tensors(fid, basis, pl, len(pt), n_rows, n_per_row, want_outer=False)
            assert (i3 == inner).all() and (o3 == EC.CANARY).all()


def test_python_tensors_is_the_ctypes_call():
    for fid in EC.FIELDS:
        for basis, (n_rows, n_per_row) in (("powers", (130, 96)), ("ml_monomial", (4, 16)), ("ml_lagrange", (64, 32)), ("ml_lagrange", (1, 1))):
            pt = EC.random_point(basis, fid, n_rows, n_per_row, EC.rng("py", fid, basis))
            pl = EC.mont(fid, pt)
            outer, inner = EC.host_tensors(fid, basis, pl if pt else None, len(pt), n_rows, n_per_row)
            po, pi = lcpc_amd.tensors(fid, pl, n_rows, n_per_row, basis=basis)
            assert po.shape == outer.shape and pi.shape == inner.shape and (po == outer).all() and (pi == inner).all()
    with pytest.raises(ValueError):
        lcpc_amd.tensors(0, np.zeros((1, 1), np.uint64), 2, 2, basis="chebyshev")
    with pytest.raises(lcpc_amd.LcpcError) as e:
        lcpc_amd.tensors(0, np.zeros((1, 1), np.uint64), 3, 2, basis="ml_monomial")
    assert e.value.code == ERR_ARG


def test_arg_errors_leave_the_outputs_untouched():
    fid, L = 3, 4
    p = IC.modulus(fid)
    x = EC.mont(fid, [5])
    z4 = EC.mont(fid, [2, 3, 4, 5])

    def refused(f, basis, point, n_pt, n_rows, n_per_row, **kw):
        """every shape asked for here fits 8 elements, or is refused for its size"""
        o = np.full((8, L), EC.CANARY, np.uint64)
        i = np.full((8, L), EC.CANARY, np.uint64)
        rc = _lib.lib().lcpce_tensors(f, basis, vp(point), n_pt, n_rows, n_per_row, vp(o) if kw.get("outer", True) else None,
                                      vp(i) if kw.get("inner", True) else None)
        assert rc == ERR_ARG, rc
        assert (o == EC.CANARY).all() and (i == EC.CANARY).all()

    refused(4, 0, x, 1, 2, 2)                       # unknown field
    refused(fid, 3, x, 1, 2, 2)                     # unknown basis
    refused(fid, 0, None, 1, 2, 2)                  # NULL point
    refused(fid, 0, x, 1, 2, 2, outer=False, inner=False)     # nothing asked for
    refused(fid, 0, x, 1, 0, 2)                     # empty dimensions
    refused(fid, 0, x, 1, 2, 0)
    refused(fid, 0, x, 0, 2, 2)                     # powers: exactly one element
    refused(fid, 0, z4, 2, 2, 2)
    refused(fid, 0, x, 1, 1 << 40, 1 << 40)         # the largest exponent does not fit 64 bits (refused before anything is written)
    for basis in (1, 2):
        refused(fid, basis, z4, 3, 4, 4)            # n_point != a + b
        refused(fid, basis, z4, 4, 2, 4)
        refused(fid, basis, z4, 4, 3, 4)            # a dimension that is not a power of two
        refused(fid, basis, z4, 4, 4, 6)
        refused(fid, basis, None, 4, 4, 4)
    # limb patterns >= p: p itself, all ones, and p in one variable of several
    for bad in (p, (1 << 256) - 1):
        refused(fid, 0, O.ints_to_limbs([bad], L), 1, 2, 2)
    mixed = z4.copy()
    mixed[2] = O.ints_to_limbs([p], L)[0]
    refused(fid, 1, mixed, 4, 4, 4)
    refused(fid, 2, mixed, 4, 4, 4)
    for f in EC.FIELDS:                              # p - 1 is the largest pattern taken, p the smallest refused, in every field
        q, Lf = IC.modulus(f), O.limbs(f)
        o = np.zeros((2, Lf), np.uint64)
        assert _lib.lib().lcpce_tensors(f, 0, vp(O.ints_to_limbs([q - 1], Lf)), 1, 2, 1, vp(o), None) == 0
        assert _lib.lib().lcpce_tensors(f, 0, vp(O.ints_to_limbs([q], Lf)), 1, 2, 1, vp(o), None) == ERR_ARG
    # the device entry points settle their arguments before any device is touched
    Lb = _lib.lib()
    a = np.zeros(8, np.uint64)
    assert Lb.lcpce_tensors_device(None, 0, vp(a), 1, 1, 2, 2, vp(a), vp(a), None) == ERR_ARG
    assert Lb.lcpce_dot_device(None, vp(a), 0, vp(a), 0, 1, 1, vp(a), None) == ERR_ARG
    assert Lb.lcpce_eval_tensors_device(None, vp(a), vp(a), 1, None, vp(a)) == ERR_ARG
    assert Lb.lcpce_eval_device(None, 0, vp(a), 1, 1, None, vp(a)) == ERR_ARG
    assert Lb.lcpce_eval(None, 0, vp(a), 1, 1, vp(a)) == ERR_ARG

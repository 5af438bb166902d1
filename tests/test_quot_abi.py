"""The quotient extension of the C ABI (include/lcpc_hip_quot.h): its own prefix, table and version, exported by the product library
next to the core ABI, and its host calls -- no device is touched here -- against Python bignum (tests/quot_cases.py): pow(x, p - 2, p)
and the definitions of the two quotients point by point.  Every comparison is for equality."""
import os
import re
import subprocess

import numpy as np
import pytest

import lcpc_amd
from lcpc_amd import _lib

import domain_cases as DC
import fft_cases as FC
import quot_cases as QC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "lcpc_hip_quot.h")
ERR_ARG = QC.ERR_ARG
vp = QC.vp
NS = (1, 2, 3, 64, 1000)
LOG_MS = range(0, 11)


def declarations():
    return re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)


def test_header_symbols_equal_the_table_and_the_exports():
    syms = sorted(set(re.findall(r"\b(lcpcq_[a-z0-9_]+)\s*\(", declarations())))
    assert syms == sorted(_lib.QUOT_SYMBOLS) and "lcpcq_divide_vanishing_device" in syms and len(syms) == 9
    L = _lib.lib()
    for s in syms:
        assert hasattr(L, s), "missing export: " + s
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert sorted(l.split()[2] for l in out.splitlines() if " T lcpcq_" in l) == syms
    for other in (_lib.SYMBOLS, _lib.BATCH_SYMBOLS, _lib.VERIFY_SYMBOLS, _lib.COLUMNS_SYMBOLS, _lib.INTS_SYMBOLS, _lib.EVAL_SYMBOLS,
                  _lib.FFT_SYMBOLS, _lib.DOMAIN_SYMBOLS):
        assert not set(_lib.QUOT_SYMBOLS) & set(other)
    assert len(_lib.DOMAIN_SYMBOLS) == 10


def test_version_and_ops():
    hdr = open(HEADER).read()
    assert _lib.lib().lcpcq_version() == int(re.search(r"#define LCPCQ_VERSION (\d+)", hdr).group(1)) == _lib.QUOT_VERSION == 1
    for name, k in _lib.QUOT_OPS.items():
        assert int(re.search(r"LCPCQ_%s = (\d+)" % name.upper(), hdr).group(1)) == k
    assert sorted(_lib.QUOT_OPS) == sorted(QC.OPS) and [_lib.QUOT_OPS[o] for o in QC.OPS] == [0, 1, 2, 3]


def test_header_adds_nothing_to_the_core_abi():
    """no text of the header, comments included, matches the pattern the core ABI's pins count"""
    assert not re.findall(r"\blcpc_[a-z0-9_]+\s*\(", open(HEADER).read())
    assert '#include "lcpc_hip.h"' in declarations() and "LCPC_ABI_VERSION" not in declarations()
    assert _lib.lib().lcpc_abi_version() == 5 and len(_lib.SYMBOLS) == 58


@pytest.mark.parametrize("fid", QC.FIELDS)
def test_inverse_and_ops_against_bignum(fid):
    F = FC.field(fid)
    for n in NS:
        for name in QC.SETS:
            x = QC.operands(fid, name, n, 64, 8)
            xm = FC.mont(fid, x)
            want = FC.mont(fid, QC.inverse_ref(fid, x))
            got = QC.host_inverse(fid, xm)
            assert np.array_equal(got, want), (n, name)
            assert np.array_equal(lcpc_amd.batch_inverse(fid, xm), want)
            inp = xm.copy()
            assert np.array_equal(QC.host_inverse(fid, inp, out=inp), want), (n, name, "in place")
            # x inv(x) == 1 off the zeros, 0 on them
            prod = FC.canon(fid, QC.host_pointwise(fid, "mul", xm, got))
            assert prod == [1 if v else 0 for v in x]
            a = QC.operands(fid, "random", n, 64, 8, "a", name)
            am = FC.mont(fid, a)
            for op in QC.OPS:
                w = FC.mont(fid, QC.pointwise_ref(fid, op, a, x))
                assert np.array_equal(QC.host_pointwise(fid, op, am, xm), w), (n, name, op)
                assert np.array_equal(lcpc_amd.pointwise(fid, op, am, xm), w)
                oa, ob = am.copy(), xm.copy()
                assert np.array_equal(QC.host_pointwise(fid, op, oa, xm, out=oa), w), (n, name, op, "out == a")
                assert np.array_equal(QC.host_pointwise(fid, op, am, ob, out=ob), w), (n, name, op, "out == b")
            # DIV(a, b) == MUL(a, inverse(b))
            assert np.array_equal(QC.host_pointwise(fid, "div", am, xm), QC.host_pointwise(fid, "mul", am, got))
    assert (F.p - 1) * (F.p - 1) % F.p == 1


@pytest.mark.parametrize("fid", QC.FIELDS)
def test_divide_linear_against_bignum(fid):
    F = FC.field(fid)
    for log_m in LOG_MS:
        vals = FC.random_vector(fid, log_m, "qlin")
        vm = FC.mont(fid, vals)
        sh = QC.coset_shifts(fid, log_m, "lin")
        for s, sl in ((1, None), (sh["gen"], DC.shift_limbs(fid, sh["gen"])), (sh["random"], DC.shift_limbs(fid, sh["random"]))):
            z = QC.off_domain(fid, s, log_m)
            y = FC.rng("qy", fid, log_m).randrange(F.p)
            zl, yl = DC.shift_limbs(fid, z), DC.shift_limbs(fid, y)
            for order in QC.ORDERS:
                want = FC.mont(fid, QC.linear_ref(fid, vals, s, z, y, order))
                assert np.array_equal(QC.host_divide_linear(fid, sl, order, vm, log_m, zl, yl), want), (log_m, s, order)
                assert np.array_equal(lcpc_amd.divide_linear(fid, vm, sl, zl, yl, order), want)
                inp = vm.copy()
                assert np.array_equal(QC.host_divide_linear(fid, sl, order, inp, log_m, zl, yl, out=inp), want)


@pytest.mark.parametrize("fid", QC.FIELDS)
def test_divide_vanishing_against_bignum(fid):
    for log_m in LOG_MS:
        vals = FC.random_vector(fid, log_m, "qvan")
        vm = FC.mont(fid, vals)
        sh = QC.coset_shifts(fid, log_m, "van")
        for name in ("gen", "random"):
            s, sl = sh[name], DC.shift_limbs(fid, sh[name])
            for log_n in range(0, log_m + 1):
                for order in QC.ORDERS:
                    want = FC.mont(fid, QC.vanishing_ref(fid, vals, s, log_n, order))
                    assert np.array_equal(QC.host_divide_vanishing(fid, sl, order, vm, log_m, log_n), want), (log_m, log_n, name, order)
                    if log_n in (0, log_m):
                        assert np.array_equal(lcpc_amd.divide_vanishing(fid, vm, sl, log_n, order), want)
                        inp = vm.copy()
                        assert np.array_equal(QC.host_divide_vanishing(fid, sl, order, inp, log_m, log_n, out=inp), want)


@pytest.mark.parametrize("fid", QC.FIELDS)
def test_refusals_write_nothing(fid):
    F = FC.field(fid)
    L, log_m = F.L, 4
    m = 1 << log_m
    lib = _lib.lib()
    vals = FC.random_vector(fid, log_m, "qref")
    vm = FC.mont(fid, vals)
    g = DC.shift_limbs(fid, DC.GENERATORS[fid])
    one, zero = DC.shift_limbs(fid, 1), np.zeros(L, np.uint64)
    big = np.full(L, 0xFFFFFFFFFFFFFFFF, np.uint64)          # a limb pattern >= p
    w = FC.root(fid, log_m)
    z_ok, y = DC.shift_limbs(fid, QC.off_domain(fid, DC.GENERATORS[fid], log_m)), DC.shift_limbs(fid, 7)
    # z on the domain: shift w^5, and w^5 on the subgroup itself
    QC.host_divide_linear(fid, g, "natural", vm, log_m, DC.shift_limbs(fid, DC.GENERATORS[fid] * pow(w, 5, F.p) % F.p), y, expect=ERR_ARG)
    QC.host_divide_linear(fid, None, "bitrev", vm, log_m, DC.shift_limbs(fid, pow(w, 5, F.p)), y, expect=ERR_ARG)
    # the vanishing form on the subgroup: a shift of 1, NULL, and a shift with shift^m == 1
    for sl in (one, None, DC.shift_limbs(fid, FC.root(fid, log_m)), DC.shift_limbs(fid, F.p - 1)):
        QC.host_divide_vanishing(fid, sl, "natural", vm, log_m, 2, expect=ERR_ARG)
    QC.host_divide_vanishing(fid, g, "natural", vm, log_m, log_m + 1, expect=ERR_ARG)
    QC.host_divide_vanishing(fid, g, "natural", vm, F.S + 1, 0, expect=ERR_ARG)
    QC.host_divide_linear(fid, g, "natural", vm, F.S + 1, z_ok, y, expect=ERR_ARG)
    # limbs >= p: an input element, the shift, z, y
    bad = vm.copy()
    bad[m - 1] = big
    QC.host_inverse(fid, bad, expect=ERR_ARG)
    for op in QC.OPS:
        QC.host_pointwise(fid, op, bad, vm, expect=ERR_ARG)
        QC.host_pointwise(fid, op, vm, bad, expect=ERR_ARG)
    QC.host_divide_linear(fid, g, "natural", bad, log_m, z_ok, y, expect=ERR_ARG)
    QC.host_divide_linear(fid, big, "natural", vm, log_m, z_ok, y, expect=ERR_ARG)
    QC.host_divide_linear(fid, g, "natural", vm, log_m, big, y, expect=ERR_ARG)
    QC.host_divide_linear(fid, g, "natural", vm, log_m, z_ok, big, expect=ERR_ARG)
    QC.host_divide_vanishing(fid, g, "natural", bad, log_m, 1, expect=ERR_ARG)
    QC.host_divide_vanishing(fid, big, "natural", vm, log_m, 1, expect=ERR_ARG)
    # a zero shift
    QC.host_divide_linear(fid, zero, "natural", vm, log_m, z_ok, y, expect=ERR_ARG)
    QC.host_divide_vanishing(fid, zero, "natural", vm, log_m, 1, expect=ERR_ARG)
    # n == 0, an unknown op, order or field, NULL pointers
    QC.host_inverse(fid, vm, n=0, expect=ERR_ARG)
    QC.host_pointwise(fid, "mul", vm, vm, n=0, expect=ERR_ARG)
    QC.host_pointwise(fid, 4, vm, vm, expect=ERR_ARG)
    QC.host_divide_linear(fid, g, 2, vm, log_m, z_ok, y, expect=ERR_ARG)
    QC.host_divide_vanishing(fid, g, 2, vm, log_m, 1, expect=ERR_ARG)
    QC.host_inverse(4, vm, expect=ERR_ARG)
    QC.host_pointwise(4, "add", vm, vm, expect=ERR_ARG)
    QC.host_divide_linear(4, g, "natural", vm, log_m, z_ok, y, expect=ERR_ARG)
    QC.host_divide_vanishing(4, g, "natural", vm, log_m, 1, expect=ERR_ARG)
    out = np.full((m, L), QC.CANARY, np.uint64)
    assert lib.lcpcq_batch_inverse(fid, None, vp(out), m) == ERR_ARG and lib.lcpcq_batch_inverse(fid, vp(vm), None, m) == ERR_ARG
    assert lib.lcpcq_pointwise(fid, 0, None, vp(vm), vp(out), m) == ERR_ARG and lib.lcpcq_pointwise(fid, 0, vp(vm), None, vp(out), m) == ERR_ARG
    assert lib.lcpcq_pointwise(fid, 0, vp(vm), vp(vm), None, m) == ERR_ARG
    assert lib.lcpcq_divide_linear(fid, vp(g), 0, None, log_m, vp(z_ok), vp(y), vp(out)) == ERR_ARG
    assert lib.lcpcq_divide_linear(fid, vp(g), 0, vp(vm), log_m, None, vp(y), vp(out)) == ERR_ARG
    assert lib.lcpcq_divide_linear(fid, vp(g), 0, vp(vm), log_m, vp(z_ok), None, vp(out)) == ERR_ARG
    assert lib.lcpcq_divide_linear(fid, vp(g), 0, vp(vm), log_m, vp(z_ok), vp(y), None) == ERR_ARG
    assert lib.lcpcq_divide_vanishing(fid, vp(g), 0, None, log_m, 1, vp(out)) == ERR_ARG
    assert lib.lcpcq_divide_vanishing(fid, vp(g), 0, vp(vm), log_m, 1, None) == ERR_ARG
    assert (out == QC.CANARY).all()
    # partial overlap: the output one element into an input, and the reverse
    buf = np.concatenate([vm, vm, vm])
    keep = buf.copy()
    for off in (1, m - 1):
        assert lib.lcpcq_batch_inverse(fid, vp(buf), vp(buf[off:]), m) == ERR_ARG and lib.lcpcq_batch_inverse(fid, vp(buf[off:]), vp(buf), m) == ERR_ARG
        for op in range(4):
            assert lib.lcpcq_pointwise(fid, op, vp(buf), vp(buf[2 * m:]), vp(buf[off:]), m) == ERR_ARG
            assert lib.lcpcq_pointwise(fid, op, vp(buf[2 * m:]), vp(buf[off:]), vp(buf), m) == ERR_ARG
        assert lib.lcpcq_divide_linear(fid, vp(g), 0, vp(buf), log_m, vp(z_ok), vp(y), vp(buf[off:])) == ERR_ARG
        assert lib.lcpcq_divide_vanishing(fid, vp(g), 0, vp(buf[off:]), log_m, 1, vp(buf)) == ERR_ARG
    assert (buf == keep).all()
    assert lib.lcpcq_batch_inverse(fid, vp(buf), vp(buf[m:]), m) == 0          # (adjacent ranges do not overlap)
    assert (buf[:m] == keep[:m]).all() and np.array_equal(buf[m:2 * m], FC.mont(fid, QC.inverse_ref(fid, vals)))
    with pytest.raises(ValueError):
        lcpc_amd.pointwise(fid, "pow", vm, vm)
    with pytest.raises(ValueError):
        lcpc_amd.divide_vanishing(fid, vm, g, 1, order="reversed")

"""The sumcheck extension of the C ABI (include/lcpc_hip_sumcheck.h): its own prefix, table and version, exported by the product
library next to the core ABI, and its host calls -- no device is touched here -- against Python bignum (tests/sumcheck_cases.py) and
against the properties a sumcheck prover relies on.  Every comparison is for equality."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import lcpc_amd
from lcpc_amd import _lib

import fft_cases as FC
import sumcheck_cases as MC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "lcpc_hip_sumcheck.h")
ERR_ARG = MC.ERR_ARG
vp = MC.vp
NS = (2, 4, 8, 64, 1024)


def declarations():
    return re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)


def exports(prefix):
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    return sorted(l.split()[2] for l in out.splitlines() if " T %s" % prefix in l)


def test_header_symbols_equal_the_table_and_the_exports():
    syms = sorted(set(re.findall(r"\b(lcpcm_[a-z0-9_]+)\s*\(", declarations())))
    assert syms == sorted(_lib.SUMCHECK_SYMBOLS) and "lcpcm_bind_round_device" in syms and len(syms) == 7
    L = _lib.lib()
    for s in syms:
        assert hasattr(L, s), "missing export: " + s
    assert exports("lcpcm_") == syms
    for other in (_lib.SYMBOLS, _lib.BATCH_SYMBOLS, _lib.VERIFY_SYMBOLS, _lib.COLUMNS_SYMBOLS, _lib.INTS_SYMBOLS, _lib.EVAL_SYMBOLS,
                  _lib.FFT_SYMBOLS, _lib.DOMAIN_SYMBOLS, _lib.QUOT_SYMBOLS, _lib.SCAN_SYMBOLS):
        assert not set(_lib.SUMCHECK_SYMBOLS) & set(other)


def test_version_orders_and_limits():
    hdr = open(HEADER).read()
    assert _lib.lib().lcpcm_version() == int(re.search(r"#define LCPCM_VERSION (\d+)", hdr).group(1)) == _lib.SUMCHECK_VERSION == 1
    for name, k in _lib.SUMCHECK_ORDERS.items():
        assert int(re.search(r"LCPCM_%s_FIRST = (\d+)" % name.upper(), hdr).group(1)) == k
    assert [_lib.SUMCHECK_ORDERS[o] for o in MC.ORDERS] == [0, 1]
    for name, k in (("TABLES", _lib.SUMCHECK_MAX_TABLES), ("TERMS", _lib.SUMCHECK_MAX_TERMS), ("FACTORS", _lib.SUMCHECK_MAX_FACTORS)):
        assert int(re.search(r"#define LCPCM_MAX_%s (\d+)" % name, hdr).group(1)) == k
    assert C.sizeof(_lib.LcpcmTerm) == 4 * (1 + _lib.SUMCHECK_MAX_FACTORS)
    assert re.search(r"typedef struct \{ uint32_t n_factors; uint32_t table\[LCPCM_MAX_FACTORS\]; \} lcpcm_term;", hdr)


def test_header_adds_nothing_to_the_core_abi_or_the_other_extensions():
    """no text of the header, comments included, matches the pattern the core ABI's pins count; the exports with the core prefix and
    with the other extensions' prefixes are the tables they were"""
    assert not re.findall(r"\blcpc_[a-z0-9_]+\s*\(", open(HEADER).read())
    assert '#include "lcpc_hip.h"' in declarations() and "LCPC_ABI_VERSION" not in declarations()
    assert _lib.lib().lcpc_abi_version() == 5 and len(_lib.SYMBOLS) == 58
    assert exports("lcpc_") == sorted(_lib.SYMBOLS)
    for prefix, table, count in (("lcpcq_", _lib.QUOT_SYMBOLS, 9), ("lcpcd_", _lib.DOMAIN_SYMBOLS, 10), ("lcpcf_", _lib.FFT_SYMBOLS, 6),
                                 ("lcpcs_", _lib.SCAN_SYMBOLS, 6), ("lcpce_", _lib.EVAL_SYMBOLS, None), ("lcpci_", _lib.INTS_SYMBOLS, None)):
        assert exports(prefix) == sorted(table) and (count is None or len(table) == count)
    # the new prefixes match none of the patterns the existing pins search with
    for prefix in ("lcpc_", "lcpcq_", "lcpcd_", "lcpcf_", "lcpcs_", "lcpce_", "lcpci_", "lcpcx_", "lcpcv_", "lcpcp_", "k17h_"):
        assert not "lcpcm_".startswith(prefix) and not "k18h_".startswith(prefix)


@pytest.mark.parametrize("order", MC.ORDERS)
@pytest.mark.parametrize("fid", MC.FIELDS)
def test_bind_and_round_against_bignum(fid, order):
    F = FC.field(fid)
    r = FC.rng("sumcheck-r", fid, order).randrange(F.p)
    rl = MC.elem(fid, r)
    for n in NS:
        for name in MC.SETS:
            tabs = MC.tables(fid, name, order, 8, n)
            tm = [FC.mont(fid, t) for t in tabs]
            keep = [t.copy() for t in tm]
            for j in (0, 7):
                want = FC.mont(fid, MC.bind_ref(fid, order, tabs[j], r))
                assert np.array_equal(MC.host_bind(fid, order, tm[j], rl), want), (n, name, j)
                io = tm[j].copy()
                MC.host_bind(fid, order, io, rl, out=io)                 # in place, both orders
                assert np.array_equal(io[:n // 2], want) and np.array_equal(io[n // 2:], tm[j][n // 2:]), (n, name, j, "in place")
                assert np.array_equal(lcpc_amd.sumcheck_bind(fid, tm[j], rl, order), want), (n, name, j, "wrapper")
            for tname in MC.TERM_LISTS:
                n_tables, terms = MC.terms_of(fid, tname)
                want = FC.mont(fid, MC.round_ref(fid, order, tabs[:n_tables], terms))
                got = MC.host_round(fid, order, tm[:n_tables], terms)
                assert np.array_equal(got, want), (n, name, tname)
                got = lcpc_amd.sumcheck_round(fid, tm[:n_tables], MC.wrapper_terms(fid, terms), order)
                assert np.array_equal(got, want), (n, name, tname, "wrapper")
            assert all(np.array_equal(a, b) for a, b in zip(tm, keep)), "an input was written"


@pytest.mark.parametrize("order", MC.ORDERS)
@pytest.mark.parametrize("fid", MC.FIELDS)
def test_round_polynomial_properties(fid, order):
    """g(0) + g(1) is the plain sum of the composition; after a bind by r the next round's g'(0) + g'(1) is g(r)"""
    F = FC.field(fid)
    n = 64
    for tname in MC.TERM_LISTS:
        n_tables, terms = MC.terms_of(fid, tname)
        tabs = MC.tables(fid, "random", order, n_tables, n, "props")
        tm = [FC.mont(fid, t) for t in tabs]
        claim = MC.composition_sum(fid, tabs, terms)
        rnd = FC.rng("sumcheck-props", fid, order, tname)
        while tm[0].shape[0] >= 2:
            g = FC.canon(fid, MC.host_round(fid, order, tm, terms))
            assert (g[0] + g[1]) % F.p == claim, (tname, tm[0].shape[0])
            r = rnd.randrange(F.p)
            claim = MC.interpolate(fid, g, r)
            tm = [MC.host_bind(fid, order, t, MC.elem(fid, r)).copy() for t in tm]
        # one value per table is left: the composition of those values is the last claim
        last = [FC.canon(fid, t)[0] for t in tm]
        assert MC.composition_sum(fid, [[v] for v in last], terms) == claim, tname


@pytest.mark.parametrize("order", MC.ORDERS)
@pytest.mark.parametrize("fid", MC.FIELDS)
def test_all_binds_end_in_the_multilinear_evaluation(fid, order):
    """after v binds the one value left is the dot product of the table with lcpce_tensors(ML_LAGRANGE) at the point z_k = r_k (low
    first) or z_(v-1-k) = r_k (high first): the variable order is that of include/lcpc_hip_eval.h"""
    F = FC.field(fid)
    v = 6
    n = 1 << v
    table = MC.tables(fid, "random", order, 1, n, "eval")[0]
    rs = [FC.rng("sumcheck-eval", fid, order, k).randrange(F.p) for k in range(v)]
    t = FC.mont(fid, table)
    for r in rs:
        t = MC.host_bind(fid, order, t, MC.elem(fid, r)).copy()
    z = rs if order == "low" else rs[::-1]
    # the whole point as one inner tensor: n_rows = 1, n_per_row = n
    outer, inner = lcpc_amd.tensors(fid, FC.mont(fid, z), 1, n, basis="ml_lagrange")
    lag = FC.canon(fid, inner)
    assert FC.canon(fid, outer) == [1]
    assert FC.canon(fid, t) == [sum(a * b for a, b in zip(table, lag)) % F.p]


@pytest.mark.parametrize("fid", MC.FIELDS)
def test_host_refusals_write_nothing(fid):
    F = FC.field(fid)
    L, n = F.L, 16
    lib = _lib.lib()
    tabs = [FC.mont(fid, t) for t in MC.tables(fid, "random", "low", 2, n, "ref")]
    big = np.full(L, 0xFFFFFFFFFFFFFFFF, np.uint64)                     # a limb pattern >= p
    bad = tabs[1].copy()
    bad[n - 1] = big
    r = MC.elem(fid, 7)
    terms = [(3, [0, 1]), (4, [1])]
    for order in (0, 1):
        MC.host_bind(fid, order, bad, r, expect=ERR_ARG)
        MC.host_bind(fid, order, tabs[0], big, expect=ERR_ARG)
        for k in (0, 1, 3, 6, 12, 1 << 39):
            MC.host_bind(fid, order, tabs[0], r, n=k, expect=ERR_ARG)
            MC.host_round(fid, order, tabs, terms, n=k, expect=ERR_ARG)
        MC.host_round(fid, order, [tabs[0], bad], terms, expect=ERR_ARG)
        arr, n_terms, cs, d = MC.c_terms(fid, terms)
        bad_cs = cs.copy()
        bad_cs[1] = big
        MC.host_round(fid, order, tabs, None, carr=(arr, n_terms, bad_cs, d), expect=ERR_ARG)
        MC.host_round(fid, order, tabs, None, carr=(arr, 0, cs, d), expect=ERR_ARG)
        MC.host_round(fid, order, tabs, None, carr=(arr, 5, cs, d), expect=ERR_ARG)
        MC.host_round(fid, order, tabs, None, carr=(None, 2, cs, d), expect=ERR_ARG)
        for nf, idx in ((0, 0), (5, 0), (2, 2)):                         # n_factors of 0 or beyond the limit; a table index >= n_tables
            a2 = (_lib.LcpcmTerm * 2)()
            a2[0].n_factors, a2[1].n_factors = 1, nf
            a2[1].table[1] = idx
            MC.host_round(fid, order, tabs, None, carr=(a2, 2, None, 2), expect=ERR_ARG)
    # an unknown order or field
    MC.host_bind(fid, 2, tabs[0], r, expect=ERR_ARG)
    MC.host_bind(4, 0, tabs[0], r, expect=ERR_ARG)
    MC.host_round(fid, 2, tabs, terms, expect=ERR_ARG)
    MC.host_round(4, 0, tabs, None, carr=MC.c_terms(fid, terms), expect=ERR_ARG)
    # NULL pointers, no table, too many tables
    out = np.full((n, L), MC.CANARY, np.uint64)
    arr, n_terms, cs, _ = MC.c_terms(fid, terms)
    ptrs = (C.c_void_p * 9)(*([tabs[0].ctypes.data, tabs[1].ctypes.data] + [tabs[0].ctypes.data] * 7))
    nul = (C.c_void_p * 2)(tabs[0].ctypes.data, None)
    assert lib.lcpcm_bind(fid, 0, None, vp(out), n, vp(r)) == ERR_ARG and lib.lcpcm_bind(fid, 0, vp(tabs[0]), None, n, vp(r)) == ERR_ARG
    assert lib.lcpcm_bind(fid, 0, vp(tabs[0]), vp(out), n, None) == ERR_ARG
    assert lib.lcpcm_round(fid, 0, None, 2, arr, n_terms, vp(cs), n, vp(out)) == ERR_ARG
    assert lib.lcpcm_round(fid, 0, nul, 2, arr, n_terms, vp(cs), n, vp(out)) == ERR_ARG
    assert lib.lcpcm_round(fid, 0, ptrs, 2, arr, n_terms, vp(cs), n, None) == ERR_ARG
    assert lib.lcpcm_round(fid, 0, ptrs, 0, arr, n_terms, vp(cs), n, vp(out)) == ERR_ARG
    assert lib.lcpcm_round(fid, 0, ptrs, 9, arr, n_terms, vp(cs), n, vp(out)) == ERR_ARG
    assert (out == MC.CANARY).all()
    # partial overlap of the output with the input; out == in and adjacent ranges are fine
    buf = np.concatenate([tabs[0], tabs[1]])
    keep = buf.copy()
    for order in (0, 1):
        for off in (1, n // 2, n - 1):
            assert lib.lcpcm_bind(fid, order, vp(buf), vp(buf[off:]), n, vp(r)) == ERR_ARG
        assert lib.lcpcm_bind(fid, order, vp(buf[n // 2 - 1:]), vp(buf), n, vp(r)) == ERR_ARG
    assert (buf == keep).all()
    assert lib.lcpcm_bind(fid, 0, vp(buf), vp(buf[n:]), n, vp(r)) == 0
    assert (buf[:n] == keep[:n]).all() and (buf[n + n // 2:] == keep[n + n // 2:]).all()
    with pytest.raises(ValueError):
        lcpc_amd.sumcheck_bind(fid, tabs[0], r, "middle")
    with pytest.raises(ValueError):
        lcpc_amd.sumcheck_round(fid, tabs, [(None, [0]), (r, [1])])
    with pytest.raises(ValueError):
        lcpc_amd.sumcheck_round(fid, [tabs[0], tabs[1][:8]], [(None, [0, 1])])


def test_device_forms_refuse_a_null_context_without_a_device():
    """what needs no context (one cannot be made without a device); tests/test_gpu_sumcheck.py runs every other refusal of the device
    forms (sumcheck_cases.device_refusals)"""
    lib = _lib.lib()
    a = np.zeros((8, 4), np.uint64)
    o = np.zeros((8, 4), np.uint64)
    arr, n_terms, _, _ = MC.c_terms(0, [(None, [0])])
    ins, outs = (C.c_void_p * 1)(a.ctypes.data), (C.c_void_p * 1)(o.ctypes.data)
    for n in (2, 4, 8, 1 << 20):
        for k in (1, 4):
            assert lib.lcpcm_round_work_bytes(None, n, k) == 0
    for order in (0, 1):
        assert lib.lcpcm_bind_device(None, order, ins, outs, 1, 8, vp(o), None) == ERR_ARG
        assert lib.lcpcm_round_device(None, order, ins, 1, arr, n_terms, None, 8, vp(o), vp(o[4:]), 1 << 20, None) == ERR_ARG
        assert lib.lcpcm_bind_round_device(None, order, ins, outs, 1, arr, n_terms, None, 8, vp(o[6:]), vp(o), vp(o[4:]), 1 << 20, None) == ERR_ARG
    assert not a.any() and not o.any()

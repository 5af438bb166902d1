"""The scan extension of the C ABI (include/lcpc_hip_scan.h): its own prefix, table and version, exported by the product library next
to the core ABI, and its host calls -- no device is touched here -- against Python bignum (tests/scan_cases.py): running sums and
products by the definition.  Every comparison is for equality."""
import os
import re
import subprocess

import numpy as np
import pytest

import lcpc_amd
from lcpc_amd import _lib

import fft_cases as FC
import scan_cases as SC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "lcpc_hip_scan.h")
ERR_ARG = SC.ERR_ARG
vp = SC.vp
NS = (1, 2, 3, 64, 1000)


def declarations():
    return re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)


def exports(prefix):
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    return sorted(l.split()[2] for l in out.splitlines() if " T %s" % prefix in l)


def test_header_symbols_equal_the_table_and_the_exports():
    syms = sorted(set(re.findall(r"\b(lcpcs_[a-z0-9_]+)\s*\(", declarations())))
    assert syms == sorted(_lib.SCAN_SYMBOLS) and "lcpcs_scan_ratio_device" in syms and len(syms) == 6
    L = _lib.lib()
    for s in syms:
        assert hasattr(L, s), "missing export: " + s
    assert exports("lcpcs_") == syms
    for other in (_lib.SYMBOLS, _lib.BATCH_SYMBOLS, _lib.VERIFY_SYMBOLS, _lib.COLUMNS_SYMBOLS, _lib.INTS_SYMBOLS, _lib.EVAL_SYMBOLS,
                  _lib.FFT_SYMBOLS, _lib.DOMAIN_SYMBOLS, _lib.QUOT_SYMBOLS):
        assert not set(_lib.SCAN_SYMBOLS) & set(other)


def test_version_ops_and_modes():
    hdr = open(HEADER).read()
    assert _lib.lib().lcpcs_version() == int(re.search(r"#define LCPCS_VERSION (\d+)", hdr).group(1)) == _lib.SCAN_VERSION == 1
    for name, k in list(_lib.SCAN_OPS.items()) + list(_lib.SCAN_MODES.items()):
        assert int(re.search(r"LCPCS_%s = (\d+)" % name.upper(), hdr).group(1)) == k
    assert [_lib.SCAN_OPS[o] for o in SC.OPS] == [0, 1] and [_lib.SCAN_MODES[m] for m in SC.MODES] == [0, 1]


def test_header_adds_nothing_to_the_core_abi_or_the_other_extensions():
    """no text of the header, comments included, matches the pattern the core ABI's pins count; the exports with the core prefix and
    with the other extensions' prefixes are the tables they were"""
    assert not re.findall(r"\blcpc_[a-z0-9_]+\s*\(", open(HEADER).read())
    assert '#include "lcpc_hip.h"' in declarations() and "LCPC_ABI_VERSION" not in declarations()
    assert _lib.lib().lcpc_abi_version() == 5 and len(_lib.SYMBOLS) == 58
    assert exports("lcpc_") == sorted(_lib.SYMBOLS)
    for prefix, table, count in (("lcpcq_", _lib.QUOT_SYMBOLS, 9), ("lcpcd_", _lib.DOMAIN_SYMBOLS, 10), ("lcpcf_", _lib.FFT_SYMBOLS, 6),
                                 ("lcpce_", _lib.EVAL_SYMBOLS, None), ("lcpci_", _lib.INTS_SYMBOLS, None)):
        assert exports(prefix) == sorted(table) and (count is None or len(table) == count)


@pytest.mark.parametrize("fid", SC.FIELDS)
def test_scan_against_bignum(fid):
    F = FC.field(fid)
    c = FC.rng("scan-init", fid).randrange(F.p)
    for n in NS:
        for name in SC.SETS:
            x = SC.operands(fid, name, n, 64, 8)
            xm = FC.mont(fid, x)
            keep = xm.copy()
            for op in SC.OPS:
                for mode in SC.MODES:
                    for init in (None, c):
                        want, wtot = SC.scan_ref(fid, op, mode, x, init)
                        wm, wt = FC.mont(fid, want), SC.elem(fid, wtot)
                        tag = (n, name, op, mode, init is not None)
                        got, tot = SC.host_scan(fid, op, mode, xm, SC.elem(fid, init))
                        assert np.array_equal(got, wm) and np.array_equal(tot, wt), tag
                        got, tot = SC.host_scan(fid, op, mode, xm, SC.elem(fid, init), want_total=False)
                        assert np.array_equal(got, wm) and tot is None, tag
                        inp = xm.copy()
                        got, tot = SC.host_scan(fid, op, mode, inp, SC.elem(fid, init), out=inp)
                        assert np.array_equal(inp, wm) and np.array_equal(tot, wt), (tag, "in place")
                        o, t = lcpc_amd.scan(fid, xm, op, exclusive=mode == "exclusive", init=SC.elem(fid, init))
                        assert np.array_equal(o, wm) and np.array_equal(t, wt), (tag, "wrapper")
            assert np.array_equal(xm, keep), "an input was written"


@pytest.mark.parametrize("fid", SC.FIELDS)
def test_scan_ratio_against_bignum(fid):
    F = FC.field(fid)
    c = FC.rng("ratio-init", fid).randrange(F.p)
    for n in NS:
        for name in SC.SETS:
            den = SC.operands(fid, name, n, 64, 8, "den")              # (the zeros of the sets stand among the denominators)
            num = SC.operands(fid, "random", n, 64, 8, "num", name)
            terms = SC.ratio_terms(fid, num, den)
            nm, dm = FC.mont(fid, num), FC.mont(fid, den)
            keep_n, keep_d = nm.copy(), dm.copy()
            for op in SC.OPS:
                for mode in SC.MODES:
                    for init in (None, c):
                        want, wtot = SC.scan_ref(fid, op, mode, terms, init)
                        wm, wt = FC.mont(fid, want), SC.elem(fid, wtot)
                        tag = (n, name, op, mode, init is not None)
                        got, tot = SC.host_scan_ratio(fid, op, mode, nm, dm, SC.elem(fid, init))
                        assert np.array_equal(got, wm) and np.array_equal(tot, wt), tag
                        got, tot = SC.host_scan_ratio(fid, op, mode, nm, dm, SC.elem(fid, init), want_total=False)
                        assert np.array_equal(got, wm) and tot is None, tag
                        on, od = nm.copy(), dm.copy()
                        _, tot = SC.host_scan_ratio(fid, op, mode, on, dm, SC.elem(fid, init), out=on)
                        assert np.array_equal(on, wm) and np.array_equal(tot, wt), (tag, "out == num")
                        _, tot = SC.host_scan_ratio(fid, op, mode, nm, od, SC.elem(fid, init), out=od)
                        assert np.array_equal(od, wm) and np.array_equal(tot, wt), (tag, "out == den")
                        o, t = lcpc_amd.scan_ratio(fid, nm, dm, op, exclusive=mode == "exclusive", init=SC.elem(fid, init))
                        assert np.array_equal(o, wm) and np.array_equal(t, wt), (tag, "wrapper")
            assert np.array_equal(nm, keep_n) and np.array_equal(dm, keep_d), "an input was written"


@pytest.mark.parametrize("fid", SC.FIELDS)
def test_two_calls_chained_through_the_total_equal_one(fid):
    n, cut = 1000, 377
    x = SC.operands(fid, "random", n, 64, 8, "chain")
    x[5] = x[700] = 1                                                  # (no zero: the product stays alive across the cut)
    x = [v or 3 for v in x]
    xm = FC.mont(fid, x)
    for op in SC.OPS:
        for mode in SC.MODES:
            whole, wtot = SC.host_scan(fid, op, mode, xm)
            a, ta = SC.host_scan(fid, op, mode, xm[:cut])
            b, tb = SC.host_scan(fid, op, mode, xm[cut:], ta)
            assert np.array_equal(np.concatenate([a, b]), whole) and np.array_equal(tb, wtot), (op, mode)
            assert np.array_equal(whole, FC.mont(fid, SC.scan_ref(fid, op, mode, x)[0]))
    # init and total inside the output: init is read first, total written last
    for mode in SC.MODES:
        want, wtot = SC.scan_ref(fid, "product", mode, x[:8], x[3])
        io = xm[:8].copy()
        assert _lib.lib().lcpcs_scan(fid, 1, _lib.SCAN_MODES[mode], vp(io), vp(io), 8, vp(io[3:]), vp(io[6:])) == 0
        wm = FC.mont(fid, want)
        wm[6] = SC.elem(fid, wtot)
        assert np.array_equal(io, wm), mode


@pytest.mark.parametrize("fid", SC.FIELDS)
def test_host_refusals_write_nothing(fid):
    F = FC.field(fid)
    L, n = F.L, 16
    lib = _lib.lib()
    xm = FC.mont(fid, SC.operands(fid, "random", n, 64, 8, "ref"))
    big = np.full(L, 0xFFFFFFFFFFFFFFFF, np.uint64)                     # a limb pattern >= p
    bad = xm.copy()
    bad[n - 1] = big
    for op in SC.OPS:
        for mode in SC.MODES:
            SC.host_scan(fid, op, mode, bad, expect=ERR_ARG)
            SC.host_scan(fid, op, mode, xm, big, expect=ERR_ARG)
            SC.host_scan(fid, op, mode, xm, n=0, expect=ERR_ARG)
            SC.host_scan(fid, op, mode, xm, n=1 << 39, expect=ERR_ARG)
            SC.host_scan_ratio(fid, op, mode, bad, xm, expect=ERR_ARG)
            SC.host_scan_ratio(fid, op, mode, xm, bad, expect=ERR_ARG)
            SC.host_scan_ratio(fid, op, mode, xm, xm, big, expect=ERR_ARG)
            SC.host_scan_ratio(fid, op, mode, xm, xm, n=0, expect=ERR_ARG)
            SC.host_scan_ratio(fid, op, mode, xm, xm, n=1 << 39, expect=ERR_ARG)
    # an unknown op, mode or field
    SC.host_scan(fid, 2, 0, xm, expect=ERR_ARG)
    SC.host_scan(fid, 0, 2, xm, expect=ERR_ARG)
    SC.host_scan(4, 0, 0, xm, expect=ERR_ARG)
    SC.host_scan_ratio(fid, 2, 0, xm, xm, expect=ERR_ARG)
    SC.host_scan_ratio(fid, 0, 2, xm, xm, expect=ERR_ARG)
    SC.host_scan_ratio(4, 0, 0, xm, xm, expect=ERR_ARG)
    # NULL pointers
    out = np.full((n, L), SC.CANARY, np.uint64)
    assert lib.lcpcs_scan(fid, 0, 0, None, vp(out), n, None, None) == ERR_ARG and lib.lcpcs_scan(fid, 0, 0, vp(xm), None, n, None, None) == ERR_ARG
    assert lib.lcpcs_scan_ratio(fid, 0, 0, None, vp(xm), vp(out), n, None, None) == ERR_ARG
    assert lib.lcpcs_scan_ratio(fid, 0, 0, vp(xm), None, vp(out), n, None, None) == ERR_ARG
    assert lib.lcpcs_scan_ratio(fid, 0, 0, vp(xm), vp(xm), None, n, None, None) == ERR_ARG
    assert (out == SC.CANARY).all()
    # partial overlap: the output one element into an input, and the reverse
    buf = np.concatenate([xm, xm, xm])
    keep = buf.copy()
    for off in (1, n - 1):
        for mode in (0, 1):
            assert lib.lcpcs_scan(fid, 1, mode, vp(buf), vp(buf[off:]), n, None, None) == ERR_ARG
            assert lib.lcpcs_scan(fid, 1, mode, vp(buf[off:]), vp(buf), n, None, None) == ERR_ARG
            assert lib.lcpcs_scan_ratio(fid, 1, mode, vp(buf), vp(buf[2 * n:]), vp(buf[off:]), n, None, None) == ERR_ARG
            assert lib.lcpcs_scan_ratio(fid, 1, mode, vp(buf[2 * n:]), vp(buf[off:]), vp(buf), n, None, None) == ERR_ARG
    assert (buf == keep).all()
    assert lib.lcpcs_scan(fid, 0, 0, vp(buf), vp(buf[n:]), n, None, None) == 0            # (adjacent ranges do not overlap)
    assert (buf[:n] == keep[:n]).all() and (buf[2 * n:] == keep[2 * n:]).all()
    with pytest.raises(ValueError):
        lcpc_amd.scan(fid, xm, "max")
    with pytest.raises(ValueError):
        lcpc_amd.scan_ratio(fid, xm, xm[:3], "sum")


def test_device_forms_refuse_a_null_context_without_a_device():
    """what needs no context (one cannot be made without a device); tests/test_gpu_scan.py runs every other refusal of the device forms (scan_cases.device_refusals), and
    tests/test_k17_cases.py holds the size of the workspace to its definition"""
    lib = _lib.lib()
    a = np.zeros((4, 4), np.uint64)
    assert lib.lcpcs_scan_work_bytes(None, 4, 1) == 0
    for op in (0, 1):
        for mode in (0, 1):
            assert lib.lcpcs_scan_device(None, op, mode, vp(a), vp(a), 4, 1, None, None, vp(a), 1 << 20, None) == ERR_ARG
            assert lib.lcpcs_scan_ratio_device(None, op, mode, vp(a), vp(a), vp(a), 4, 1, None, None, vp(a), 1 << 20, None) == ERR_ARG
    assert not a.any()

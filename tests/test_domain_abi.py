"""The domain extension of the C ABI (include/lcpc_hip_domain.h): its own prefix, table and version, exported by the product library
next to the core ABI, and its host calls -- no device is touched here -- against Python bignum: the definitions by direct sum and by
Horner's rule, tests/fft_cases.py's transform on vectors scaled beforehand, and lcpcf_fft at shift 1."""
import os
import re
import subprocess

import numpy as np
import pytest

import lcpc_amd
from lcpc_amd import _lib

import domain_cases as DC
import fft_cases as FC
import oracle_lib as O
import pyref as P

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "lcpc_hip_domain.h")
ERR_ARG = DC.ERR_ARG
vp = DC.vp
LOG_NS = range(0, 11)


def declarations():
    return re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)


def test_header_symbols_equal_the_table_and_the_exports():
    syms = sorted(set(re.findall(r"\b(lcpcd_[a-z0-9_]+)\s*\(", declarations())))
    assert syms == sorted(_lib.DOMAIN_SYMBOLS) and "lcpcd_lde_device" in syms and len(syms) == 10
    L = _lib.lib()
    for s in syms:
        assert hasattr(L, s), "missing export: " + s
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert sorted(l.split()[2] for l in out.splitlines() if " T lcpcd_" in l) == syms
    for other in (_lib.SYMBOLS, _lib.BATCH_SYMBOLS, _lib.VERIFY_SYMBOLS, _lib.COLUMNS_SYMBOLS, _lib.INTS_SYMBOLS, _lib.EVAL_SYMBOLS,
                  _lib.FFT_SYMBOLS):
        assert not set(_lib.DOMAIN_SYMBOLS) & set(other)
    assert len(_lib.FFT_SYMBOLS) == 6


def test_version_forms_and_orders():
    hdr = open(HEADER).read()
    assert _lib.lib().lcpcd_version() == int(re.search(r"#define LCPCD_VERSION (\d+)", hdr).group(1)) == _lib.DOMAIN_VERSION == 1
    for name, k in list(_lib.FFT_FORMS.items()) + list(_lib.DOMAIN_ORDERS.items()):
        assert int(re.search(r"LCPCD_%s = (\d+)" % name.upper(), hdr).group(1)) == k
    assert sorted(_lib.DOMAIN_ORDERS) == sorted(DC.ORDERS)


def test_header_adds_nothing_to_the_core_abi():
    """no text of the header, comments included, matches the pattern the core ABI's pins count"""
    assert not re.findall(r"\blcpc_[a-z0-9_]+\s*\(", open(HEADER).read())
    assert '#include "lcpc_hip.h"' in declarations() and "LCPC_ABI_VERSION" not in declarations()
    assert _lib.lib().lcpc_abi_version() == 5 and len(_lib.SYMBOLS) == 58


def test_generator():
    """10, 3, 5, 5 (PrimeFieldGenerator), in Montgomery limbs; a generator is no square: g^((p - 1) / 2) != 1"""
    for fid in DC.FIELDS:
        F = P.FIELDS[fid]
        g = FC.canon(fid, DC.host_generator(fid).reshape(1, -1))[0]
        assert g == DC.GENERATORS[fid] == (10, 3, 5, 5)[fid]
        assert pow(g, (F.p - 1) // 2, F.p) == F.p - 1 != 1
        assert (lcpc_amd.generator(fid) == DC.shift_limbs(fid, g)).all()
    assert _lib.lib().lcpcd_generator(4, vp(np.zeros(4, np.uint64))) == ERR_ARG and _lib.lib().lcpcd_generator(0, None) == ERR_ARG


@pytest.mark.parametrize("fid", DC.FIELDS)
@pytest.mark.parametrize("form", DC.FORMS)
def test_every_form_is_the_definition(fid, form):
    """log_n <= 6: the sums of the header themselves; above, fft_cases.dft on the vector scaled beforehand (or afterwards)"""
    for log_n in LOG_NS:
        x = FC.random_vector(fid, log_n, "coset", form)
        xm = FC.mont(fid, x)
        for name, s in DC.shifts(fid, log_n, form).items():
            want = DC.apply_form(fid, form, x, s, DC.coset_direct if log_n <= 6 else DC.coset_dft)
            got = DC.host_coset_fft(fid, form, DC.shift_limbs(fid, s), xm, log_n)
            assert (got == FC.mont(fid, want)).all(), (log_n, name)
            assert (lcpc_amd.coset_fft(fid, xm, DC.shift_limbs(fid, s), form) == got).all()
            if name == "one":
                assert (got == FC.host_fft(fid, form, xm, log_n)).all(), log_n            # lcpcf_'s limbs exactly


def test_the_fast_reference_is_the_definition():
    for fid in DC.FIELDS:
        for log_n in range(0, 7):
            x = FC.random_vector(fid, log_n, "cref")
            for s in DC.shifts(fid, log_n).values():
                assert DC.coset_dft(fid, x, s) == DC.coset_direct(fid, x, s)
                assert DC.coset_dft(fid, x, s, True) == DC.coset_direct(fid, x, s, True)
                assert DC.coset_dft(fid, DC.coset_dft(fid, x, s), s, True) == x


@pytest.mark.parametrize("fid", DC.FIELDS)
def test_round_trips_and_in_place(fid):
    for log_n in LOG_NS:
        xm = FC.mont(fid, FC.random_vector(fid, log_n, "ctrip"))
        for s in DC.shifts(fid, log_n, "trip").values():
            sl = DC.shift_limbs(fid, s)
            for a, b in DC.PAIRS:
                y = DC.host_coset_fft(fid, a, sl, xm, log_n)
                assert (DC.host_coset_fft(fid, b, sl, y, log_n) == xm).all(), (a, b, log_n)
                buf = xm.copy()
                DC.host_coset_fft(fid, a, sl, buf, log_n, out=buf)
                assert (buf == y).all(), (a, log_n)


N_COEFFS = (1, 2, 3, 5, 8, 13, 16)


@pytest.mark.parametrize("fid", DC.FIELDS)
@pytest.mark.parametrize("order", DC.ORDERS)
def test_extend_is_horner(fid, order):
    for nc in N_COEFFS:
        coeffs = FC.random_vector(fid, 4, "ext", nc)[:nc]
        cm = FC.mont(fid, coeffs)
        for log_m in range(DC.ceil_log2(nc), DC.ceil_log2(nc) + 4):
            for name, s in DC.shifts(fid, nc, log_m).items():
                want = DC.extend_horner(fid, coeffs, s, log_m, order)
                got = DC.host_extend(fid, DC.shift_limbs(fid, s), cm, nc, log_m, order)
                assert (got == FC.mont(fid, want)).all(), (nc, log_m, name)
                assert want == DC.extend_fast(fid, coeffs, s, log_m, order)
                assert (lcpc_amd.extend(fid, cm, DC.shift_limbs(fid, s), log_m, order) == got).all()


@pytest.mark.parametrize("fid", DC.FIELDS)
def test_block_property(fid):
    """block c of the bit-reversed extension is the FFT_IO coset transform of the zero-padded coefficients with the shift
    s w_m^rev_b(c) -- what the device kernels compute"""
    F = P.FIELDS[fid]
    for nc in N_COEFFS:
        log_n = DC.ceil_log2(nc)
        coeffs = FC.random_vector(fid, 4, "blk", nc)[:nc]
        padded = FC.mont(fid, coeffs + [0] * ((1 << log_n) - nc))
        for b in range(0, 4):
            log_m = log_n + b
            s = DC.shifts(fid, nc, b)["random"]
            ext = DC.host_extend(fid, DC.shift_limbs(fid, s), FC.mont(fid, coeffs), nc, log_m, "bitrev")
            for c in range(1 << b):
                sc = s * pow(FC.root(fid, log_m), FC.rev(c, b), F.p) % F.p
                blk = DC.host_coset_fft(fid, "fft_io", DC.shift_limbs(fid, sc), padded, log_n)
                assert (ext[c << log_n:(c + 1) << log_n] == blk).all(), (nc, b, c)


@pytest.mark.parametrize("fid", DC.FIELDS)
def test_errors_leave_the_output_alone(fid):
    F = P.FIELDS[fid]
    L, log_n = F.L, 4
    n = 1 << log_n
    lib = _lib.lib()
    xm = FC.mont(fid, FC.random_vector(fid, log_n, "cerr"))
    g = DC.host_generator(fid)
    zero = np.zeros(L, np.uint64)
    big = [O.ints_to_limbs([v], L)[0] for v in (F.p, F.p + 1, (1 << (64 * L)) - 1)]
    for bad_shift in [zero, None] + big:                                     # shift 0, NULL, a limb pattern >= p
        DC.host_coset_fft(fid, "fft_io", bad_shift, xm, log_n, expect=ERR_ARG)
        DC.host_extend(fid, bad_shift, xm, n, log_n + 1, "natural", expect=ERR_ARG)
    DC.host_coset_fft(9, "fft_io", g, xm, log_n, expect=ERR_ARG)              # an unknown field, form, order
    DC.host_coset_fft(fid, 6, g, xm, log_n, expect=ERR_ARG)
    DC.host_extend(9, g, xm, n, log_n, "natural", expect=ERR_ARG)
    DC.host_extend(fid, g, xm, n, log_n, 2, expect=ERR_ARG)
    out = np.full((2 * n, L), DC.CANARY, np.uint64)                           # NULL pointers
    assert lib.lcpcd_coset_fft(fid, 1, vp(g), None, vp(out), log_n) == ERR_ARG and lib.lcpcd_coset_fft(fid, 1, vp(g), vp(xm), None, log_n) == ERR_ARG
    assert lib.lcpcd_extend(fid, vp(g), None, n, log_n, 0, vp(out)) == ERR_ARG and lib.lcpcd_extend(fid, vp(g), vp(xm), n, log_n, 0, None) == ERR_ARG
    assert (out == DC.CANARY).all()
    one = np.full((1, L), DC.CANARY, np.uint64)                              # log_n, log_m > S are settled before anything is read
    for big_log in (F.S + 1, 0xFFFFFFFF):
        assert lib.lcpcd_coset_fft(fid, 1, vp(g), vp(one), vp(one), big_log) == ERR_ARG
        assert lib.lcpcd_extend(fid, vp(g), vp(xm), 1, big_log, 0, vp(one)) == ERR_ARG
    assert (one == DC.CANARY).all()
    DC.host_extend(fid, g, xm, 0, log_n, "natural", expect=ERR_ARG)           # n_coeffs 0 and > m
    DC.host_extend(fid, g, xm, n, log_n - 1, "bitrev", expect=ERR_ARG, room=n)
    DC.host_extend(fid, g, xm, n // 2 + 1, log_n - 1, "bitrev", expect=ERR_ARG, room=n)
    for bad in big:                                                          # input elements >= p
        for at in (0, 7, n - 1):
            x = xm.copy()
            x[at] = bad
            DC.host_coset_fft(fid, "ifft_ii", g, x, log_n, expect=ERR_ARG)
            DC.host_extend(fid, g, x, n, log_n, "natural", expect=ERR_ARG)
            keep = x.copy()
            assert lib.lcpcd_coset_fft(fid, 0, vp(g), vp(x), vp(x), log_n) == ERR_ARG and (x == keep).all()
    DC.host_extend(fid, g, np.concatenate([xm[:8], big[0][None]]), 8, 3, "natural")        # (elements past n_coeffs are not read)
    buf = np.concatenate([xm, xm, xm])                                       # ranges that overlap without being equal
    keep = buf.copy()
    for off in (1, n - 1):
        assert lib.lcpcd_coset_fft(fid, 1, vp(g), vp(buf), vp(buf[off:]), log_n) == ERR_ARG
        assert lib.lcpcd_coset_fft(fid, 1, vp(g), vp(buf[off:]), vp(buf), log_n) == ERR_ARG
        assert lib.lcpcd_extend(fid, vp(g), vp(buf[off:]), n, log_n + 1, 0, vp(buf)) == ERR_ARG
        assert lib.lcpcd_extend(fid, vp(g), vp(buf), n, log_n + 1, 0, vp(buf[off:])) == ERR_ARG
    assert lib.lcpcd_extend(fid, vp(g), vp(buf[2 * n - 1:]), n, log_n + 1, 0, vp(buf)) == ERR_ARG     # the LAST output element meets the first input
    assert (buf == keep).all()
    assert lib.lcpcd_coset_fft(fid, 1, vp(g), vp(buf), vp(buf[n:]), log_n) == 0          # (adjacent ranges do not overlap)
    buf = np.concatenate([xm, xm, xm])
    assert lib.lcpcd_extend(fid, vp(g), vp(buf[2 * n:]), n, log_n + 1, 1, vp(buf)) == 0
    assert (buf[:2 * n] == DC.host_extend(fid, g, xm, n, log_n + 1, "bitrev")).all() and (buf[2 * n:] == xm).all()
    buf = np.concatenate([xm, xm])                                           # coeffs == out: the extension in place
    assert lib.lcpcd_extend(fid, vp(g), vp(buf), n, log_n + 1, 0, vp(buf)) == 0
    assert (buf == DC.host_extend(fid, g, xm, n, log_n + 1, "natural")).all()


def test_k14_harness_is_a_separate_library():
    """lib/liblcpc_k14_harness.so (tests/native/k14_harness.cpp) exports the k14h_* entry points of tests/k14_harness.py and nothing of
    the product, which it links against instead of carrying a copy"""
    from test_abi import _harness_is_a_separate_library
    _harness_is_a_separate_library("k14_harness", "k14h_", "tests/native/k14_harness.cpp", "K14H_OUT")

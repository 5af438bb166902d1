"""The transform extension of the C ABI (include/lcpc_hip_fft.h): its own prefix, table and version, exported by the product library
next to the core ABI, and its host call -- no device is touched here -- against Python bignum and oracle/pyref.py's fft_io."""
import os
import re
import subprocess

import numpy as np
import pytest

import lcpc_amd
from lcpc_amd import _lib

import fft_cases as FC
import oracle_lib as O
import pyref as P

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "lcpc_hip_fft.h")
ERR_ARG = FC.ERR_ARG
vp = FC.vp
LOG_NS = range(0, 11)


def declarations():
    return re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)


def test_header_symbols_equal_the_table_and_the_exports():
    syms = sorted(set(re.findall(r"\b(lcpcf_[a-z0-9_]+)\s*\(", declarations())))
    assert syms == sorted(_lib.FFT_SYMBOLS) and "lcpcf_fft_device" in syms and len(syms) == 6
    L = _lib.lib()
    for s in syms:
        assert hasattr(L, s), "missing export: " + s
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert sorted(l.split()[2] for l in out.splitlines() if " T lcpcf_" in l) == syms
    for other in (_lib.SYMBOLS, _lib.BATCH_SYMBOLS, _lib.VERIFY_SYMBOLS, _lib.COLUMNS_SYMBOLS, _lib.INTS_SYMBOLS, _lib.EVAL_SYMBOLS):
        assert not set(_lib.FFT_SYMBOLS) & set(other)


def test_version_forms_and_orders():
    hdr = open(HEADER).read()
    assert _lib.lib().lcpcf_version() == int(re.search(r"#define LCPCF_VERSION (\d+)", hdr).group(1)) == _lib.FFT_VERSION
    assert sorted(_lib.FFT_FORMS) == sorted(FC.FORMS)
    for name, k in list(_lib.FFT_FORMS.items()) + list(_lib.FFT_ORDERS.items()):
        assert int(re.search(r"LCPCF_%s = (\d+)" % name.upper(), hdr).group(1)) == k


def test_header_adds_nothing_to_the_core_abi():
    """no text of the header, comments included, matches the pattern the core ABI's pins count"""
    assert not re.findall(r"\blcpc_[a-z0-9_]+\s*\(", open(HEADER).read())
    assert '#include "lcpc_hip.h"' in declarations() and "LCPC_ABI_VERSION" not in declarations()
    assert _lib.lib().lcpc_abi_version() == 5 and len(_lib.SYMBOLS) == 58


def test_max_log_n_is_the_two_adicity():
    assert [_lib.lib().lcpcf_max_log_n(fid) for fid in FC.FIELDS] == [P.FIELDS[fid].S for fid in FC.FIELDS] == [41, 40, 41, 41]
    assert [O.field_info(fid)["S"] for fid in FC.FIELDS] == [41, 40, 41, 41]
    assert _lib.lib().lcpcf_max_log_n(4) == 0 and _lib.lib().lcpcf_max_log_n(0xFFFFFFFF) == 0


def test_the_fast_reference_is_the_direct_sum():
    """fft_cases.dft (what the larger sizes are compared with) against the sum it abbreviates, both directions"""
    for fid in FC.FIELDS:
        for log_n in range(0, 7):
            x = FC.random_vector(fid, log_n, "ref")
            assert FC.dft(fid, x) == FC.dft_direct(fid, x) and FC.dft(fid, x, True) == FC.dft_direct(fid, x, True)
            assert FC.dft(fid, FC.dft(fid, x), True) == x


@pytest.mark.parametrize("fid", FC.FIELDS)
def test_fft_io_is_pyrefs(fid):
    F = P.FIELDS[fid]
    for log_n in LOG_NS:
        x = FC.random_vector(fid, log_n, "io")
        got = FC.host_fft(fid, "fft_io", FC.mont(fid, x), log_n)
        assert (got == FC.mont(fid, P.fft_io(F, list(x)))).all(), log_n
        assert lcpc_amd.fft(fid, FC.mont(fid, x)).tolist() == got.tolist()


@pytest.mark.parametrize("fid", FC.FIELDS)
@pytest.mark.parametrize("form", FC.FORMS)
def test_every_form_is_the_direct_dft(fid, form):
    """log_n <= 6: the sum itself with the form's permutations; above, the O(n log n) bignum transform the test above holds to it"""
    for log_n in LOG_NS:
        x = FC.random_vector(fid, log_n, form)
        want = FC.apply_form(fid, form, x, FC.dft_direct if log_n <= 6 else FC.dft)
        assert (FC.host_fft(fid, form, FC.mont(fid, x), log_n) == FC.mont(fid, want)).all(), log_n
        assert (lcpc_amd.fft(fid, FC.mont(fid, x), form) == FC.mont(fid, want)).all()


def test_order_rule_examples():
    """FFT_IO stores X[k] at out[rev(k)]; IFFT_OI reads X[k] from in[rev(k)] and stores x[j] at out[j]"""
    fid, log_n = 1, 5
    x, X = FC.pair(fid, log_n, "order")
    io = FC.canon(fid, FC.host_fft(fid, "fft_io", FC.mont(fid, x), log_n))
    assert all(io[FC.rev(k, log_n)] == X[k] for k in range(1 << log_n))
    assert FC.canon(fid, FC.host_fft(fid, "ifft_oi", FC.mont(fid, io), log_n)) == list(x)


@pytest.mark.parametrize("fid", FC.FIELDS)
def test_round_trips(fid):
    for log_n in LOG_NS:
        xm = FC.mont(fid, FC.random_vector(fid, log_n, "trip"))
        for a, b in FC.PAIRS:
            assert (FC.host_fft(fid, b, FC.host_fft(fid, a, xm, log_n), log_n) == xm).all(), (a, b, log_n)


@pytest.mark.parametrize("fid", FC.FIELDS)
def test_all_p_minus_one(fid):
    """every element p - 1: X[0] = n (p - 1) mod p and zero elsewhere; with it a vector whose STORED limbs are p - 1"""
    F = P.FIELDS[fid]
    for log_n in LOG_NS:
        n = 1 << log_n
        got = FC.canon(fid, FC.host_fft(fid, "fft_ii", FC.mont(fid, [F.p - 1] * n), log_n))
        assert got == [n * (F.p - 1) % F.p] + [0] * (n - 1)
        stored = np.tile(O.ints_to_limbs([F.p - 1], F.L), (n, 1))
        x = FC.canon(fid, stored)
        for form in FC.FORMS:
            assert (FC.host_fft(fid, form, stored, log_n) == FC.mont(fid, FC.apply_form(fid, form, x))).all(), (form, log_n)


@pytest.mark.parametrize("fid", FC.FIELDS)
def test_in_place_equals_out_of_place(fid):
    for log_n in LOG_NS:
        xm = FC.mont(fid, FC.random_vector(fid, log_n, "inplace"))
        for form in FC.FORMS:
            buf = xm.copy()
            FC.host_fft(fid, form, buf, log_n, out=buf)
            assert (buf == FC.host_fft(fid, form, xm, log_n)).all(), (form, log_n)


@pytest.mark.parametrize("fid", FC.FIELDS)
def test_errors_leave_the_output_alone(fid):
    F = P.FIELDS[fid]
    L, log_n = F.L, 4
    xm = FC.mont(fid, FC.random_vector(fid, log_n, "err"))
    lib = _lib.lib()
    FC.host_fft(9, "fft_io", xm, log_n, expect=ERR_ARG)                      # an unknown field
    FC.host_fft(fid, 6, xm, log_n, expect=ERR_ARG)                           # an unknown form
    FC.host_fft(fid, 0xFFFFFFFF, xm, log_n, expect=ERR_ARG)
    out = np.full((1 << log_n, L), FC.CANARY, np.uint64)
    assert lib.lcpcf_fft(fid, 1, None, vp(out), log_n) == ERR_ARG and (out == FC.CANARY).all()
    assert lib.lcpcf_fft(fid, 1, vp(xm), None, log_n) == ERR_ARG
    one = np.full((1, L), FC.CANARY, np.uint64)                              # log_n > S is settled before anything is read
    assert lib.lcpcf_fft(fid, 1, vp(one), vp(one), F.S + 1) == ERR_ARG and lib.lcpcf_fft(fid, 1, vp(one), vp(one), 0xFFFFFFFF) == ERR_ARG
    assert (one == FC.CANARY).all()
    for bad in (F.p, F.p + 1, (1 << (64 * L)) - 1):                          # a limb pattern >= p, first, in the middle and last
        for at in (0, 7, (1 << log_n) - 1):
            x = xm.copy()
            x[at] = O.ints_to_limbs([bad], L)[0]
            FC.host_fft(fid, "ifft_ii", x, log_n, expect=ERR_ARG)
            keep = x.copy()
            assert lib.lcpcf_fft(fid, 0, vp(x), vp(x), log_n) == ERR_ARG and (x == keep).all()
    buf = np.concatenate([xm, xm])                                           # ranges that overlap without being equal
    keep = buf.copy()
    for off in (1, (1 << log_n) - 1):
        assert lib.lcpcf_fft(fid, 1, vp(buf), vp(buf[off:]), log_n) == ERR_ARG
        assert lib.lcpcf_fft(fid, 1, vp(buf[off:]), vp(buf), log_n) == ERR_ARG
    assert (buf == keep).all()
    assert lib.lcpcf_fft(fid, 1, vp(buf), vp(buf[1 << log_n:]), log_n) == 0    # (adjacent ranges do not overlap)

"""The plain-integer extension of the C ABI (include/lcpc_hip_ints.h): its own prefix, table and version, exported by the product
library next to the core ABI, and its two host calls -- no device is touched here -- against Python bignum."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import lcpc_amd
from lcpc_amd import _lib

import ints_cases as IC
import oracle_lib as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "lcpc_hip_ints.h")
ERR_ARG = -7


def declarations():
    return re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)


def vp(a):
    return a.ctypes.data_as(C.c_void_p)


def test_header_symbols_equal_the_table_and_the_exports():
    syms = sorted(set(re.findall(r"\b(lcpci_[a-z0-9_]+)\s*\(", declarations())))
    assert syms == sorted(_lib.INTS_SYMBOLS) and "lcpci_commit_ints" in syms
    L = _lib.lib()
    for s in syms:
        assert hasattr(L, s), "missing export: " + s
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert sorted(l.split()[2] for l in out.splitlines() if " T lcpci_" in l) == syms
    for other in (_lib.SYMBOLS, _lib.BATCH_SYMBOLS, _lib.VERIFY_SYMBOLS, _lib.COLUMNS_SYMBOLS):
        assert not set(_lib.INTS_SYMBOLS) & set(other)


def test_version_and_kinds():
    hdr = open(HEADER).read()
    assert _lib.lib().lcpci_version() == int(re.search(r"#define LCPCI_VERSION (\d+)", hdr).group(1)) == _lib.INTS_VERSION
    for name, k in _lib.INTS_KINDS.items():
        assert int(re.search(r"LCPCI_%s = (\d+)" % name.upper(), hdr).group(1)) == k


def test_header_adds_nothing_to_the_core_abi():
    """no text of the header, comments included, matches the pattern the core ABI's pins count"""
    assert not re.findall(r"\blcpc_[a-z0-9_]+\s*\(", open(HEADER).read())
    assert '#include "lcpc_hip.h"' in declarations() and "LCPC_ABI_VERSION" not in declarations()
    assert _lib.lib().lcpc_abi_version() == 5 and len(_lib.SYMBOLS) == 58


def test_python_moduli_are_the_fields():
    for fid in IC.FIELDS:
        assert lcpc_amd.FIELD_MODULUS[fid] == IC.modulus(fid)


@pytest.mark.parametrize("fid", IC.FIELDS)
@pytest.mark.parametrize("kind", IC.KINDS)
def test_from_ints_against_bignum(fid, kind):
    """lcpci_from_ints on E(kind) and 200 seeded random values = (v % p) * R % p, and lcpci_to_canon brings v mod p back"""
    L = O.limbs(fid)
    p = IC.modulus(fid)
    vals = IC.edges(kind, fid) + IC.random_values(kind, fid, 200, 1000 + 10 * fid + IC.KINDS.index(kind))
    a = IC.pack(kind, vals, L)
    out = np.full((len(vals), L), 0xA5A5A5A5A5A5A5A5, np.uint64)
    assert _lib.lib().lcpci_from_ints(fid, _lib.INTS_KINDS[kind], vp(a), len(vals), vp(out)) == 0
    assert (out == IC.reference(fid, vals)).all()
    assert (out == O.to_mont(fid, [v % p for v in vals])).all()
    canon = np.zeros_like(out)
    assert _lib.lib().lcpci_to_canon(fid, vp(out), len(vals), vp(canon)) == 0
    assert O.limbs_to_ints(canon) == [v % p for v in vals]


def test_from_ints_reads_any_element_offset():
    """an input needs its element's alignment only: a slice that starts 1, 2, 3 elements into an array"""
    for kind in ("u32", "i64", "wide"):
        vals = IC.random_values(kind, 3, 40, 7)
        a = IC.pack(kind, vals, 4)
        for off in (1, 2, 3):
            out = np.zeros((len(vals) - off, 4), np.uint64)
            assert _lib.lib().lcpci_from_ints(3, _lib.INTS_KINDS[kind], vp(a[off:]), len(vals) - off, vp(out)) == 0
            assert (out == IC.reference(3, vals[off:])).all()


def test_arg_errors():
    L = _lib.lib()
    a, out = np.zeros(4, np.uint64), np.full((4, 4), 7, np.uint64)
    assert L.lcpci_from_ints(4, 0, vp(a), 1, vp(out)) == ERR_ARG          # unknown field
    assert L.lcpci_from_ints(0, 5, vp(a), 1, vp(out)) == ERR_ARG          # unknown kind
    assert L.lcpci_from_ints(0, 0, None, 1, vp(out)) == ERR_ARG
    assert L.lcpci_from_ints(0, 0, vp(a), 1, None) == ERR_ARG
    assert L.lcpci_from_ints(0, 0, None, 0, None) == 0                    # n == 0: nothing is read
    assert L.lcpci_to_canon(4, vp(a), 1, vp(out)) == ERR_ARG
    assert L.lcpci_to_canon(0, None, 1, vp(out)) == ERR_ARG
    assert L.lcpci_to_canon(0, vp(a), 1, None) == ERR_ARG
    assert L.lcpci_to_canon(0, None, 0, None) == 0
    assert (out == 7).all()
    # the commit entry points settle their arguments before any device is touched
    assert L.lcpci_commit_ints(None, 0, vp(a), 1, None) == ERR_ARG
    assert L.lcpci_commit_ints_device(None, 0, vp(a), 1, None, None) == ERR_ARG
    assert L.lcpci_from_ints_device(None, 0, vp(a), 1, vp(out), None) == ERR_ARG


def test_python_from_ints_and_to_ints_need_no_device():
    """enc.from_ints / enc.to_ints are methods of an encoder, which needs a device; the conversions underneath do not -- Python ints of
    any size and sign through the same reduction the methods apply"""
    for fid in IC.FIELDS:
        p, Lf = IC.modulus(fid), O.limbs(fid)
        vals = [0, -1, p, -p, 3 * p + 5, -(1 << 300), 1 << 300, -(1 << 63)]
        red = O.ints_to_limbs([v % p for v in vals], Lf)
        out = np.zeros_like(red)
        assert _lib.lib().lcpci_from_ints(fid, _lib.INTS_KINDS["wide"], vp(red), len(vals), vp(out)) == 0
        assert (out == IC.reference(fid, vals)).all()

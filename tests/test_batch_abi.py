"""The batch extension of the C ABI (include/lcpc_hip_batch.h): its own prefix, table and version, exported by the product
library next to the core ABI, which it leaves exactly as it is."""
import os
import re
import subprocess

from lcpc_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "lcpc_hip_batch.h")


def declarations():
    src = open(HEADER).read()
    return re.sub(r"/\*.*?\*/", "", src, flags=re.S)


def test_header_symbols_equal_the_table_and_the_exports():
    syms = sorted(set(re.findall(r"\b(lcpcx_[a-z0-9_]+)\s*\(", declarations())))
    assert syms == sorted(_lib.BATCH_SYMBOLS) and "lcpcx_commit_batch_device" in syms
    L = _lib.lib()
    for s in syms:
        assert hasattr(L, s), "missing export: " + s
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = sorted(l.split()[2] for l in out.splitlines() if " T lcpcx_" in l)
    assert exported == syms
    assert not set(_lib.BATCH_SYMBOLS) & set(_lib.SYMBOLS)


def test_batch_version():
    ver = int(re.search(r"#define LCPCX_BATCH_VERSION (\d+)", open(HEADER).read()).group(1))
    assert _lib.lib().lcpcx_batch_version() == ver == _lib.BATCH_VERSION


def test_header_adds_nothing_to_the_core_abi():
    """no declaration of the extension header matches the pattern the core ABI's pins count (lcpc_[a-z0-9_]+ followed by a
    parenthesis), comments included: the 58 symbols and version 5 of include/lcpc_hip.h keep holding"""
    assert not re.findall(r"\blcpc_[a-z0-9_]+\s*\(", declarations())
    assert not re.findall(r"\blcpc_[a-z0-9_]+\s*\(", open(HEADER).read())
    assert '#include "lcpc_hip.h"' in declarations()
    assert "LCPC_ABI_VERSION" not in declarations()

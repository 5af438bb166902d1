"""lcpcx_prove_batch at the ABI (include/lcpc_hip_batch.h, version 2): exported, in the loader's table, and refusing NULL and
zero-count arguments before it touches a device."""
import ctypes as C
import os
import re
import subprocess

from lcpc_amd import ERR_ARG, _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "lcpc_hip_batch.h")


def test_symbol_is_exported_and_in_the_table():
    assert "lcpcx_prove_batch" in _lib.BATCH_SYMBOLS
    assert hasattr(_lib.lib(), "lcpcx_prove_batch")
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert any(l.split()[1:] == ["T", "lcpcx_prove_batch"] for l in out.splitlines())
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    assert re.search(r"\bint\s+lcpcx_prove_batch\s*\(", src) and "lcpcx_prove_stats" in src


def test_version_is_two_in_all_three_places():
    ver = int(re.search(r"#define LCPCX_BATCH_VERSION (\d+)", open(HEADER).read()).group(1))
    assert ver == 2 and _lib.BATCH_VERSION == 2 and _lib.lib().lcpcx_batch_version() == 2


def test_stats_struct_and_budget_match_the_header():
    src = open(HEADER).read()
    body = re.search(r"typedef struct \{(.*?)\} lcpcx_prove_stats;", src, flags=re.S).group(1)
    fields = re.findall(r"uint32_t\s+(\w+);", body)
    assert fields == [f[0] for f in _lib.LcpcxProveStats._fields_] and C.sizeof(_lib.LcpcxProveStats) == 4 * len(fields)
    shift = int(re.search(r"#define LCPCX_PROVE_ARENA_BUDGET \(\(uint64_t\)64 << (\d+)\)", src).group(1))
    assert _lib.PROVE_ARENA_BUDGET == 64 << shift == 64 << 20


def test_null_and_zero_count_arguments_are_refused_without_a_device():
    f = _lib.lib().lcpcx_prove_batch
    one = (C.c_void_p * 1)(None)                 # arrays of one NULL member / transcript / proof
    lens = (C.c_uint64 * 1)()
    outer = (C.c_uint64 * 4)()
    o = C.cast(outer, C.c_void_p)
    assert f(None, 1, o, 1, 0, one, one, lens, None, None) == ERR_ARG          # NULL cms
    assert f(one, 1, o, 1, 0, None, one, lens, None, None) == ERR_ARG          # NULL trs
    assert f(one, 1, None, 1, 0, one, one, lens, None, None) == ERR_ARG        # NULL outer tensor
    assert f(one, 1, o, 1, 0, one, None, lens, None, None) == ERR_ARG          # NULL proofs
    assert f(one, 1, o, 1, 0, one, one, None, None, None) == ERR_ARG           # NULL proof_lens
    assert f(one, 0, o, 1, 0, one, one, lens, None, None) == ERR_ARG           # n_batch == 0
    assert f(one, 65536, o, 1, 0, one, one, lens, None, None) == ERR_ARG       # n_batch > 65535 (nothing is dereferenced)
    assert f(one, 1, o, 1, 0, one, one, lens, None, None) == ERR_ARG           # a NULL member
    sentinel = (C.c_void_p * 1)(1)
    assert f(one, 1, o, 1, 0, one, sentinel, lens, None, None) == ERR_ARG and sentinel[0] is None     # no proof is returned

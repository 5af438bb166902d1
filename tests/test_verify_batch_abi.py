"""lcpcv_verify_batch at the ABI (include/lcpc_hip_verify.h, version 1): the extension's own header, prefix, version and loader table;
exported by the product beside the core and batch symbols, which do not move; refusing bad arguments before it touches a device."""
import ctypes as C
import os
import re
import subprocess

from lcpc_amd import ERR_ARG, _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "lcpc_hip_verify.h")


def _code(path=HEADER):
    return re.sub(r"/\*.*?\*/", "", open(path).read(), flags=re.S)


def _exports(prefix):
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    return sorted(l.split()[2] for l in out.splitlines() if len(l.split()) == 3 and l.split()[1] == "T" and l.split()[2].startswith(prefix))


def test_symbols_of_header_table_and_library_agree():
    declared = sorted(set(re.findall(r"\b(lcpcv_[a-z0-9_]+)\s*\(", _code())))
    assert declared == sorted(_lib.VERIFY_SYMBOLS) == _exports("lcpcv_") == ["lcpcv_verify_batch", "lcpcv_version"]
    assert all(hasattr(_lib.lib(), name) for name in declared)


def test_version_is_one_in_all_three_places():
    ver = int(re.search(r"#define LCPCV_VERSION (\d+)", open(HEADER).read()).group(1))
    assert ver == 1 and _lib.VERIFY_VERSION == 1 and _lib.lib().lcpcv_version() == 1


def test_stats_struct_and_budget_match_the_header():
    src = open(HEADER).read()
    body = re.search(r"typedef struct \{(.*?)\} lcpcv_verify_stats;", src, flags=re.S).group(1)
    fields = re.findall(r"uint32_t\s+(\w+);", body)
    assert fields == ["groups", "encode_launches", "hash_launches", "check_launches", "host_syncs"]
    assert fields == [f[0] for f in _lib.LcpcvVerifyStats._fields_] and C.sizeof(_lib.LcpcvVerifyStats) == 4 * len(fields)
    shift = int(re.search(r"#define LCPCV_ARENA_BUDGET \(\(uint64_t\)64 << (\d+)\)", src).group(1))
    assert _lib.VERIFY_ARENA_BUDGET == 64 << shift == 64 << 20


def test_the_other_headers_do_not_move():
    """the extension adds nothing to the core header and nothing but a pointer to the batch header: 58 core symbols at version 5, batch
    version 2 with its three symbols"""
    core = _code(os.path.join(ROOT, "include", "lcpc_hip.h"))
    assert int(re.search(r"#define LCPC_ABI_VERSION (\d+)", core).group(1)) == 5 == _lib.ABI_VERSION == _lib.lib().lcpc_abi_version()
    assert "lcpcv_" not in core and "lcpc_hip_verify" not in core
    assert len(_exports("lcpc_")) == 58 == len(_lib.SYMBOLS)
    batch = open(os.path.join(ROOT, "include", "lcpc_hip_batch.h")).read()
    assert int(re.search(r"#define LCPCX_BATCH_VERSION (\d+)", batch).group(1)) == 2 == _lib.BATCH_VERSION == _lib.lib().lcpcx_batch_version()
    assert _exports("lcpcx_") == sorted(_lib.BATCH_SYMBOLS)
    assert "lcpcv_" not in re.sub(r"/\*.*?\*/", "", batch, flags=re.S)           # (its comment points here; its code does not)
    assert "lcpc_hip_verify.h" in batch


def test_header_declares_nothing_of_the_core():
    """it includes lcpc_hip.h and names no core function as a declaration or call, in code or comment"""
    src = open(HEADER).read()
    assert '#include "lcpc_hip.h"' in src
    assert not re.search(r"\blcpc_[a-z0-9_]+\s*\(", src)


def test_bad_arguments_are_refused_without_a_device():
    f = _lib.lib().lcpcv_verify_batch
    vp = lambda a: C.cast(a, C.c_void_p)
    words = (C.c_uint64 * 16)()
    roots, outer, inner, evals = vp((C.c_uint8 * 64)()), vp(words), vp(words), vp((C.c_uint64 * 8)())
    status = (C.c_int32 * 2)(7, 7)
    st = vp(status)
    proof = (C.c_uint8 * 8)()
    proofs = (C.c_void_p * 2)(C.addressof(proof), C.addressof(proof))
    lens = (C.c_uint64 * 2)(8, 8)
    # no call below may dereference the context or a transcript: the addresses are made up
    ctx = C.c_void_p(0x1000)
    trs = (C.c_void_p * 2)(0x2000, 0x3000)
    good = dict(ctx=ctx, n=2, roots=roots, outer=outer, n_outer=4, os=0, inner=inner, n_inner=4, is_=0, proofs=proofs, lens=lens, trs=trs,
                evals=evals, status=st)

    def call(**kw):
        a = dict(good)
        a.update(kw)
        return f(a["ctx"], a["n"], a["roots"], a["outer"], a["n_outer"], a["os"], a["inner"], a["n_inner"], a["is_"], a["proofs"], a["lens"],
                 a["trs"], a["evals"], a["status"], None)

    for name in ("ctx", "roots", "outer", "inner", "proofs", "lens", "trs", "evals", "status"):
        assert call(**{name: None}) == ERR_ARG, name
    assert call(n=0) == ERR_ARG and call(n=65536) == ERR_ARG
    assert call(proofs=(C.c_void_p * 2)(C.addressof(proof), None)) == ERR_ARG          # a NULL member proof
    assert call(trs=(C.c_void_p * 2)(0x2000, None)) == ERR_ARG                         # a NULL member transcript
    assert call(trs=(C.c_void_p * 2)(0x2000, 0x2000)) == ERR_ARG                       # a transcript listed twice
    assert call(os=3) == ERR_ARG and call(is_=1) == ERR_ARG                            # 0 < stride < n
    assert list(status) == [7, 7]                                                      # an argument error judges nobody

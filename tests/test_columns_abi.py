"""lcpcp_check_columns at the ABI (include/lcpc_hip_columns.h, version 1): the extension's own header, prefix, version and loader table;
exported by the product beside the core, batch and verify symbols, which do not move; refusing bad arguments before it touches a
device.  And the K8 kernel harness as a library of its own."""
import ctypes as C
import os
import re
import subprocess

from lcpc_amd import ERR_ARG, _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "lcpc_hip_columns.h")
HARNESS = os.path.join(ROOT, "lcpc_amd", "lib", "liblcpc_k8_harness.so")


def _code(path=HEADER):
    return re.sub(r"/\*.*?\*/", "", open(path).read(), flags=re.S)


def _defined(path):
    out = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True, check=True).stdout
    return [l.split() for l in out.splitlines() if len(l.split()) == 3]


def _exports(prefix, path=None):
    return sorted(s[2] for s in _defined(path or _lib.LIB_PATH) if s[1] == "T" and s[2].startswith(prefix))


def test_symbols_of_header_table_and_library_agree():
    declared = sorted(set(re.findall(r"\b(lcpcp_[a-z0-9_]+)\s*\(", _code())))
    assert declared == sorted(_lib.COLUMNS_SYMBOLS) == _exports("lcpcp_") == ["lcpcp_check_columns", "lcpcp_version"]
    assert all(hasattr(_lib.lib(), name) for name in declared)


def test_version_is_one_in_all_three_places():
    ver = int(re.search(r"#define LCPCP_VERSION (\d+)", open(HEADER).read()).group(1))
    assert ver == 1 and _lib.COLUMNS_VERSION == 1 and _lib.lib().lcpcp_version() == 1


def test_the_other_headers_do_not_move():
    core = _code(os.path.join(ROOT, "include", "lcpc_hip.h"))
    assert int(re.search(r"#define LCPC_ABI_VERSION (\d+)", core).group(1)) == 5 == _lib.ABI_VERSION == _lib.lib().lcpc_abi_version()
    assert "lcpcp_" not in core and "lcpc_hip_columns" not in core
    assert len(_exports("lcpc_")) == 58 == len(_lib.SYMBOLS)
    assert _lib.BATCH_VERSION == 2 == _lib.lib().lcpcx_batch_version() and _exports("lcpcx_") == sorted(_lib.BATCH_SYMBOLS)
    assert _lib.VERIFY_VERSION == 1 == _lib.lib().lcpcv_version() and _exports("lcpcv_") == sorted(_lib.VERIFY_SYMBOLS)
    for name in ("lcpc_hip_batch.h", "lcpc_hip_verify.h"):
        assert "lcpcp_" not in open(os.path.join(ROOT, "include", name)).read()


def test_path_budget_matches_the_verify_header():
    src = open(os.path.join(ROOT, "include", "lcpc_hip_verify.h")).read()
    shift = int(re.search(r"#define LCPCV_PATH_BUDGET \(\(uint64_t\)64 << (\d+)\)", src).group(1))
    assert _lib.VERIFY_PATH_BUDGET == 64 << shift == 64 << 20


def test_header_declares_nothing_of_the_core():
    """it includes lcpc_hip.h and names no core function as a declaration or call, in code or comment"""
    src = open(HEADER).read()
    assert '#include "lcpc_hip.h"' in src
    assert not re.search(r"\blcpc_[a-z0-9_]+\s*\(", src)


def test_bad_arguments_are_refused_without_a_device():
    f = _lib.lib().lcpcp_check_columns
    vp = lambda a: C.cast(a, C.c_void_p)
    root, cols, vals, paths = vp((C.c_uint8 * 64)()), vp((C.c_uint64 * 2)()), vp((C.c_uint64 * 16)()), vp((C.c_uint8 * 128)())
    okb = (C.c_uint8 * 2)(7, 7)
    # no call below may dereference the context: the address is made up
    good = dict(ctx=C.c_void_p(0x1000), root=root, cols=cols, n=2, n_rows=2, vals=vals, paths=paths, ok=vp(okb))

    def call(**kw):
        a = dict(good)
        a.update(kw)
        return f(a["ctx"], a["root"], a["cols"], a["n"], a["n_rows"], a["vals"], a["paths"], a["ok"])

    for name in ("ctx", "root", "cols", "vals", "paths", "ok"):
        assert call(**{name: None}) == ERR_ARG, name
    assert call(n_rows=0) == ERR_ARG
    assert call(n=0, n_rows=0) == ERR_ARG and call(n=0, ok=None) == ERR_ARG       # the pointers and n_rows come first
    assert call(n=0) == 0                                                          # nothing to judge: no device, nothing written
    assert list(okb) == [7, 7]


def test_k8_harness_is_a_library_of_its_own():
    """k8h_ only, no name of the product's, NEEDED-linked to the product, whose binary does not know the prefix"""
    from test_abi import _harness_is_a_separate_library
    _harness_is_a_separate_library("k8_harness", "k8h_", "tests/native/k8_harness.cpp", "K8H_OUT")
    import k8_harness
    assert sorted(k8_harness.SYMBOLS) == ["k8h_device_count", "k8h_fold_paths", "k8h_refusal"] and k8_harness.LIB_PATH == HARNESS
    clean = subprocess.check_output(["make", "-n", "-C", os.path.join(ROOT, "lcpc_amd", "csrc"), "clean"], text=True)
    assert "../lib/liblcpc_k8_harness.so" in clean.split()

"""ctypes side of tests/native/k1_harness.cpp (lcpc_amd/lib/liblcpc_k1_harness.so, built by lcpc_amd/csrc/Makefile): a real Ligero
context made by lcpc_ctx_create, and read-only copies of what its row NTT (K1) reads -- the plan, the twiddle / clamp / fourth-root tables
at their full stride, the lane-varying entries of a pass's pack as the product's pack_get loads them, and the packs' shifted-multiples
tables.  The LCPC_NTT_* switches are read when a context is created: `Ctx(..., env=...)` sets them around that call and takes them back.
Errors as in tests/harness_kit.py; BadArgs means the harness refused the request before it touched the device."""
import ctypes as C
import os

import numpy as np

import harness_kit as K
from harness_kit import BadArgs, HipError, check as _check, ptr as _ptr  # noqa: F401

LIB_PATH = K.lib_path("k1")
K1H_BAD_ARGS = -1000
TABLES = ["d_roots", "d_rootsl", "d_rootslc", "d_rootsls", "d_rootslcs", "d_qpl", "d_wq_w"]      # the harness's table numbers
KINDS = ["general", "K1s", "K1n"]
SWITCHES = ("LCPC_NTT_GENERAL", "LCPC_NTT_FORM", "LCPC_NTT_MUL", "LCPC_NTT_MID_MAX_MB", "LCPC_DEBUG_TIMING")

_vp, _u64, _u32, _i32 = C.c_void_p, C.c_uint64, C.c_uint32, C.c_int
SYMBOLS = {
    "k1h_device_count": [],
    "k1h_open": [_u32, _u64, _u64, _u32, _u32, _vp],
    "k1h_close": [_vp],
    "k1h_info": [_vp, _vp, _u32],
    "k1h_tables": [_vp, _vp, _u32],
    "k1h_plan": [_vp, _u32, _vp, _u32],
    "k1h_table": [_vp, _i32, _u64, _u64, _vp, _u64],
    "k1h_pack_entries": [_vp, _u32, _vp, _u32, _vp, _u64],
    "k1h_uniform": [_vp, _u32, _vp, _u32, _vp, _u64],
    "k1h_last_error": [_vp],
}


def lib():
    L = K.load("k1", SYMBOLS)
    L.k1h_close.restype = None
    L.k1h_last_error.restype = C.c_char_p
    return L


def _check(what, rc, h=None):
    if rc == K1H_BAD_ARGS:
        raise BadArgs(what)
    if rc >= 1000:
        raise HipError(what, rc - 1000)
    if rc:
        detail = lib().k1h_last_error(h).decode() if h else ""
        raise RuntimeError("%s: lcpc status %d %s" % (what, rc, detail))


class Pass:
    """one pass of the plan as k1h_plan reports it"""

    def __init__(self, index, w):
        self.index = index
        self.kind, self.first = KINDS[w[0]], bool(w[1])
        self.log_n, self.t0, self.s, self.log_tj, self.form = (int(x) for x in w[2:7])
        self.round_off = [int(x) for x in w[7:15]]
        self.class_words, self.u_off, self.mul2, self.n_classes, self.log_tile = (int(x) for x in w[15:20])
        self.records, self.n_utabs = int(w[20]), int(w[21])

    def __repr__(self):
        return "pass %d: %s first=%d log_n=%d t0=%d s=%d form=%d mul2=%d classes=%d" % (
            self.index, self.kind, self.first, self.log_n, self.t0, self.s, self.form, self.mul2, self.n_classes)


class Ctx:
    """a Ligero context of field `fid` with new_from_dims(n_per_row, n_cols); env: the LCPC_NTT_* switches it is created under (the
    others are taken out of the environment for the call)"""

    def __init__(self, fid, n_per_row, n_cols, rho=(1, 2), env=None):
        L = lib()
        saved = {k: os.environ.pop(k) for k in SWITCHES if k in os.environ}
        os.environ.update(env or {})
        h = _vp()
        try:
            rc = L.k1h_open(fid, n_per_row, n_cols, rho[0], rho[1], C.byref(h))
        finally:
            for k in env or {}:
                del os.environ[k]
            os.environ.update(saved)
        _check("k1h_open", rc)
        self.h, self.fid = h, fid
        info = np.zeros(8, np.uint32)
        _check("k1h_info", L.k1h_info(self.h, _ptr(info), 8))
        self.NL, self.N, self.W, self.STRIDE, self.log_n, n_pass, canon, self.U_SLOT = (int(x) for x in info)
        self.comm_canon = bool(canon)
        ent = np.zeros(7, np.uint64)
        _check("k1h_tables", L.k1h_tables(self.h, _ptr(ent), 7))
        self.entries = {name: int(n) for name, n in zip(TABLES, ent)}        # 0: the context has no such table
        self.passes = []
        for i in range(n_pass):
            w = np.zeros(24, np.uint32)
            _check("k1h_plan", L.k1h_plan(self.h, i, _ptr(w), 24), self.h)
            self.passes.append(Pass(i, w))

    def close(self):
        if self.h:
            lib().k1h_close(self.h)
            self.h = None

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def words(self, name):
        return {"d_roots": self.NL, "d_wq_w": 96}.get(name, self.STRIDE)

    def table(self, name, first=0, count=None):
        """entries [first, first + count) of a table, (count, words per entry) uint32, pad words included"""
        count = self.entries[name] - first if count is None else count
        out = np.full((max(count, 0), self.words(name)), 0xA5A5A5A5, np.uint32)
        _check("k1h_table " + name, lib().k1h_table(self.h, TABLES.index(name), first, count, _ptr(out), out.size), self.h)
        return out

    def pack_entries(self, pas, classes):
        """every lane-varying entry of a pass for the classes listed: (records, 4 + N) uint32 -- class, slot, variant, jl, limbs"""
        cls = np.ascontiguousarray(classes, np.uint32)
        out = np.full((len(cls) * (self.passes[pas].records if pas < len(self.passes) else 1), 4 + self.N), 0xA5A5A5A5, np.uint32)
        _check("k1h_pack_entries", lib().k1h_pack_entries(self.h, pas, _ptr(cls), len(cls), _ptr(out), out.size), self.h)
        return out

    def uniform(self, pas, classes):
        """every shifted-multiples table of a pass for the classes listed: (records, 4 + U_SLOT) uint32 -- class, round, position, v,
        raw words"""
        cls = np.ascontiguousarray(classes, np.uint32)
        out = np.full((len(cls) * (self.passes[pas].n_utabs if pas < len(self.passes) else 1), 4 + self.U_SLOT), 0xA5A5A5A5, np.uint32)
        _check("k1h_uniform", lib().k1h_uniform(self.h, pas, _ptr(cls), len(cls), _ptr(out), out.size), self.h)
        return out

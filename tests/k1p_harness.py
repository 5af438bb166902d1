"""ctypes side of tests/native/k1p_harness.cpp (lcpc_amd/lib/liblcpc_k1p_harness.so, built by lcpc_amd/csrc/Makefile): a real Ligero
context made by lcpc_ctx_create, ONE pass kernel of its row-NTT plan per call through the product's launcher, the general kernel on a
free split of the stages, and the launchers' documented refusals.  The LCPC_NTT_* switches are read when a context is created:
`Ctx(..., env=...)` sets them around that call and takes them back.  Errors as in tests/harness_kit.py; BadArgs means the harness
refused the request before it touched the device.

Every buffer a pass may write comes back whole as a `Buf`: the canary words in front of and behind it and the body, gaps between rows
included; `Buf.untouched(mask)` says whether every word outside `mask` still holds the canary."""
import ctypes as C
import os

import numpy as np

import harness_kit as K
from harness_kit import BadArgs, HipError, check as _check, ptr as _ptr  # noqa: F401

LIB_PATH = K.lib_path("k1p")
K1P_BAD_ARGS = -1000
KINDS = ["general", "K1s", "K1n"]
SWITCHES = ("LCPC_NTT_GENERAL", "LCPC_NTT_FORM", "LCPC_NTT_MUL", "LCPC_NTT_MID_MAX_MB", "LCPC_DEBUG_TIMING")
CANARY = 0xA5A5A5A5
UNLIMITED = (1 << 64) - 1
F_COPY, F_CANON, F_MID, F_INPLACE, F_MONTWORD = 1, 2, 4, 8, 16
HIP_ERROR_INVALID_VALUE = 1
REFUSALS = ["general: s + log_tj > log_tile", "K1s last pass with mont_prefix", "K1s first pass: tile_group too large",
            "K1s three-pass first pass with form", "K1s pure pass S in (2, 7, 9) with mul2", "K1n last pass with tile_group"]

_vp, _u64, _u32, _i32 = C.c_void_p, C.c_uint64, C.c_uint32, C.c_int
SYMBOLS = {
    "k1p_device_count": [],
    "k1p_canary_words": [],
    "k1p_open": [_u32, _u64, _u64, _u32, _u32, _vp],
    "k1p_close": [_vp],
    "k1p_last_error": [_vp],
    "k1p_info": [_vp, _vp, _u32],
    "k1p_plan": [_vp, _u32, _vp, _u32],
    "k1p_run_step": [_vp, _u32, _vp, _u32, _vp, _u64, _vp, _u64, _vp, _u64, _vp, _u64],
    "k1p_run_general": [_vp, _vp, _u32, _vp, _u64, _vp, _u64, _vp, _u64],
    "k1p_refused": [_vp, _u32, _vp, _u32],
}


def lib():
    L = K.load("k1p", SYMBOLS)
    L.k1p_close.restype = None
    L.k1p_last_error.restype = C.c_char_p
    L.k1p_canary_words.restype = _u64
    return L


def _check(what, rc, h=None):
    if rc == K1P_BAD_ARGS:
        raise BadArgs(what)
    if rc >= 1000:
        raise HipError(what, rc - 1000)
    if rc:
        detail = lib().k1p_last_error(h).decode() if h else ""
        raise RuntimeError("%s: lcpc status %d %s" % (what, rc, detail))


class Step:
    """one step of the plan as k1p_plan reports it"""
    FIELDS = ("log_n", "t0", "s", "log_tj", "log_tile", "form", "mul2", "mont_prefix", "blk0_gone", "canon_row_mask", "tile_group",
              "n_classes")

    def __init__(self, index, w):
        self.index = index
        self.kind, self.first = KINDS[w[0]], bool(w[1])
        for name, x in zip(self.FIELDS, w[2:14]):
            setattr(self, name, int(x))
        self.can_canon = bool(w[14])

    def __repr__(self):
        return "step %d: %s first=%d %s" % (self.index, self.kind, self.first, " ".join("%s=%d" % (f, getattr(self, f)) for f in self.FIELDS))


class Buf:
    """[canary | body | canary] as the device held it after the launch"""

    def __init__(self, words, can):
        self.all = np.full(words + 2 * can, 0x5A5A5A5A, np.uint32)       # (not the canary: a copy that never happened shows)
        self.can = can

    @property
    def body(self):
        return self.all[self.can:len(self.all) - self.can]

    def canaries_intact(self):
        return bool((self.all[:self.can] == CANARY).all() and (self.all[len(self.all) - self.can:] == CANARY).all())

    def untouched(self, written=None):
        """the canaries, and every body word outside the boolean mask `written` (None: the whole body), still hold the canary"""
        if not self.canaries_intact():
            return False
        b = self.body
        return bool((b == CANARY).all()) if written is None else bool((b[~written] == CANARY).all())


class Ctx:
    """a Ligero context of field `fid` with new_from_dims(n_per_row, n_cols); env: the LCPC_NTT_* switches it is created under (the
    others are taken out of the environment for the call)"""

    def __init__(self, fid, n_per_row, n_cols, rho=(1, 2), env=None):
        L = lib()
        saved = {k: os.environ.pop(k) for k in SWITCHES if k in os.environ}
        os.environ.update(env or {})
        h = _vp()
        try:
            rc = L.k1p_open(fid, n_per_row, n_cols, rho[0], rho[1], C.byref(h))
        finally:
            for k in env or {}:
                del os.environ[k]
            os.environ.update(saved)
        _check("k1p_open", rc)
        self.h, self.fid = h, fid
        info = np.zeros(8, np.uint32)
        _check("k1p_info", L.k1p_info(self.h, _ptr(info), 8))
        self.NL, self.N, self.W, self.STRIDE, self.log_n, n_step, canon, limb = (int(x) for x in info)
        self.comm_canon, self.limb_tables = bool(canon), bool(limb)
        self.can = int(L.k1p_canary_words())
        self.steps = []
        for i in range(n_step):
            w = np.zeros(16, np.uint32)
            _check("k1p_plan", L.k1p_plan(self.h, i, _ptr(w), 16), self.h)
            self.steps.append(Step(i, w))

    def close(self):
        if self.h:
            lib().k1p_close(self.h)
            self.h = None

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def run_step(self, step, src, n_rows=1, src_stride=None, dst_stride=None, n_valid=None, n_src_total=UNLIMITED, flags=0):
        """one step.  src: uint32 words (packed elements, or the K1s last pass's limb records).  Strides and n_valid default to the
        (sub-)row length.  -> (dst, mid or None, copy_dst or None) as Buf"""
        ln = 1 << (self.steps[step].log_n if step < len(self.steps) else self.log_n)
        n_sub = n_rows << (self.log_n - (self.steps[step].log_n if step < len(self.steps) else self.log_n))
        src_stride = ln if src_stride is None else src_stride
        dst_stride = ln if dst_stride is None else dst_stride
        n_valid = ln if n_valid is None else n_valid
        req = np.array([n_rows, src_stride, dst_stride, n_valid, n_src_total, flags], np.uint64)
        src = np.ascontiguousarray(src, np.uint32).reshape(-1)
        dst = Buf(n_sub * dst_stride * self.NL, self.can)
        mid = Buf(n_sub * ln * 9, self.can) if flags & F_MID else None
        cp = Buf(n_rows * src_stride * self.NL, self.can) if flags & F_COPY else None
        rc = lib().k1p_run_step(self.h, step, _ptr(req), 6, _ptr(src), src.size, _ptr(dst.all), dst.all.size,
                                _ptr(mid.all) if mid else None, mid.all.size if mid else 0, _ptr(cp.all) if cp else None, cp.all.size if cp else 0)
        _check("k1p_run_step %d" % step, rc, self.h)
        return dst, mid, cp

    def run_general(self, src, log_tile, t0, s, log_tj, n_rows=1, src_stride=None, dst_stride=None, n_valid=None, n_src_total=UNLIMITED, flags=0):
        """launch_ntt_pass on a free split.  -> (dst, copy_dst or None) as Buf"""
        ln = 1 << self.log_n
        src_stride = ln if src_stride is None else src_stride
        dst_stride = ln if dst_stride is None else dst_stride
        n_valid = ln if n_valid is None else n_valid
        req = np.array([n_rows, src_stride, dst_stride, n_valid, n_src_total, flags, log_tile, t0, s, log_tj], np.uint64)
        src = np.ascontiguousarray(src, np.uint32).reshape(-1)
        dst = Buf(n_rows * dst_stride * self.NL, self.can)
        cp = Buf(n_rows * src_stride * self.NL, self.can) if flags & F_COPY else None
        rc = lib().k1p_run_general(self.h, _ptr(req), 10, _ptr(src), src.size, _ptr(dst.all), dst.all.size,
                                   _ptr(cp.all) if cp else None, cp.all.size if cp else 0)
        _check("k1p_run_general", rc, self.h)
        return dst, cp

    def refused(self, which):
        """-> (the hipError_t the launcher returned, every output word still canary)"""
        out = np.zeros(2, np.uint32)
        _check("k1p_refused %d" % which, lib().k1p_refused(self.h, which, _ptr(out), 2), self.h)
        return int(out[0]), bool(out[1])

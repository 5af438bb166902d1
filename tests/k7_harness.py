"""ctypes side of tests/native/k7_harness.cpp (lcpc_amd/lib/liblcpc_k7_harness.so, built by lcpc_amd/csrc/Makefile): the column check of
the batched verify (K7b, launch_verify_columns_batch of lcpc_amd/csrc/kernels.h) on operands a test builds, and the case builder with
its Python-int expectations.  Elements cross as uint64 arrays of stored (Montgomery) limbs, last axis L.  Errors as in
tests/harness_kit.py."""
import ctypes as C
import random

import numpy as np

import harness_kit as K
from harness_kit import BadArgs, HipError, check as _check, ptr as _ptr  # noqa: F401
from k2_harness import NL  # noqa: F401

LIB_PATH = K.lib_path("k7")
HIP_SUCCESS, HIP_ERROR_INVALID_VALUE = 0, 1
DEGREE_BIT, EVAL_BIT = 1, 2
POISON = (1 << 64) - 1           # all-ones limbs: not a reduced element; must never be read

_vp, _u64, _u32, _i32 = C.c_void_p, C.c_uint64, C.c_uint32, C.c_int
SYMBOLS = {
    "k7h_device_count": [],
    "k7h_verify_columns": [_i32, _vp, _u64, _vp, _vp, _vp, _vp, _u64, _u64, _u32, _u32, _u32],
    "k7h_refusal": [_i32, _u32, _u32, _u32, _i32],
}


def lib():
    return K.load("k7", SYMBOLS)


class Case:
    """One launch of K7b.  Stored (Montgomery) integers: cols[m][i][k], tensors[m][d][k], enc[m][d][c]; drawn[m][i]; stride = the
    member stride of cols in elements (>= n_open * n_rows; the gap is poison).  An opened column's values are those of the column
    number it was drawn for, so a number drawn twice opens the same values twice, as in a proof."""

    def __init__(self, fid, n_rows, n_t, n_cols, drawn, stride=None, fill="random", seed=1):
        from common import FIELD_L, field_p
        self.fid, self.L, self.p = fid, FIELD_L[fid], field_p(fid)
        self.n_rows, self.n_t, self.n_cols = n_rows, n_t, n_cols
        self.drawn = [list(d) for d in drawn]
        self.n_batch, self.n_open = len(self.drawn), len(self.drawn[0])
        assert all(len(d) == self.n_open for d in self.drawn)
        self.stride = self.n_open * n_rows if stride is None else stride
        assert self.stride >= self.n_open * n_rows
        rng = random.Random(seed)
        p = self.p
        value = {"random": lambda: rng.randrange(p), "max": lambda: p - 1, "zero": lambda: 0}[fill]
        self.tensors = [[[value() for _ in range(n_rows)] for _ in range(n_t)] for _ in range(self.n_batch)]
        self.cols = []
        for m in range(self.n_batch):
            by_number = {}
            for cn in self.drawn[m]:
                if cn not in by_number:
                    by_number[cn] = [value() for _ in range(n_rows)]
            self.cols.append([by_number[cn] for cn in self.drawn[m]])
        # the encoded rows: random, and at every drawn column the dot products themselves
        self.enc = [[[rng.randrange(p) for _ in range(n_cols)] for _ in range(n_t)] for _ in range(self.n_batch)]
        for m in range(self.n_batch):
            for i, cn in enumerate(self.drawn[m]):
                if cn < n_cols:
                    for d in range(n_t):
                        self.enc[m][d][cn] = self.dot(m, i, d)

    def dot(self, m, i, d):
        """<tensor d, opened column i> of member m as the STORED value of the product: sum (t R)(c R) / R mod p"""
        R = 1 << (64 * self.L)
        s = sum(t * c for t, c in zip(self.tensors[m][d], self.cols[m][i]))
        return s * pow(R, -1, self.p) % self.p

    def plant(self, m, i, d):
        """make tensor d disagree at member m's opened column i (and at every other opening of the same column number)"""
        cn = self.drawn[m][i]
        self.enc[m][d][cn] = (self.enc[m][d][cn] + 1) % self.p

    def expected(self):
        """status[m][i] by Python integers"""
        out = np.zeros((self.n_batch, self.n_open), np.uint32)
        for m in range(self.n_batch):
            for i, cn in enumerate(self.drawn[m]):
                if cn >= self.n_cols:
                    out[m, i] = (DEGREE_BIT if self.n_t > 1 else 0) | EVAL_BIT
                    continue
                for d in range(self.n_t):
                    if self.dot(m, i, d) != self.enc[m][d][cn]:
                        out[m, i] |= EVAL_BIT if d == self.n_t - 1 else DEGREE_BIT
        return out

    def arrays(self):
        """(cols (n_batch, stride, L), tensors (n_batch, n_t, n_rows, L), enc (n_batch, n_t, n_cols, L), drawn (n_batch, n_open)), uint64"""
        from common import to_limbs
        L = self.L
        cols = np.full((self.n_batch, self.stride, L), POISON, np.uint64)
        for m in range(self.n_batch):
            flat = [v for col in self.cols[m] for v in col]
            cols[m, :len(flat)] = to_limbs(flat, L)
        tensors = np.stack([np.stack([to_limbs(t, L) for t in self.tensors[m]]) for m in range(self.n_batch)])
        enc = np.stack([np.stack([to_limbs(e, L) for e in self.enc[m]]) for m in range(self.n_batch)])
        return cols, tensors, enc, np.array(self.drawn, np.uint64).reshape(self.n_batch, self.n_open)

    def run(self, prefill=0xdeadbeef):
        """K7b on the device: status (n_batch, n_open) uint32"""
        cols, tensors, enc, drawn = self.arrays()
        status = np.full((self.n_batch, self.n_open), prefill, np.uint32)
        _check("k7h_verify_columns", lib().k7h_verify_columns(NL[self.fid], _ptr(cols), self.stride, _ptr(tensors), _ptr(enc), _ptr(drawn),
                                                              _ptr(status), self.n_rows, self.n_cols, self.n_open, self.n_t, self.n_batch))
        return status


def refusal(fid, n_batch, n_open, n_t, limb=True):
    """the hipError_t of the launcher on a job it must settle before any launch (null buffers; no device is touched); BadArgs when the
    job is one a correct launcher would launch"""
    rc = lib().k7h_refusal(NL[fid], n_batch, n_open, n_t, int(limb))
    if rc == -1:
        raise BadArgs("k7h_refusal")
    return rc

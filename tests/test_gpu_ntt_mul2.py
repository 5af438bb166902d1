"""K1s's two multipliers for lane-varying twiddles (lcpc_amd/csrc/ntt_l9s.hip, template flag M2): LCPC_NTT_MUL=split (ln::mul2 on two-table
packs: b0 = w c 2^145, b1 = w c 2^290, five Montgomery digits) against LCPC_NTT_MUL=mont (ln::mul on w c 2^261, nine digits) and against
the oracle, bit for bit, through the public path: commit (canonical output: comm, hashes, root) and encode (Montgomery-form rows).

Shapes: 2^11 and 2^13 (S = 1, 3: the radix-2 round), 2^12 (S = 2: I alone -- only the coset pass multiplies by ln::mul2), 2^15 (S = 5: radix-2
and one lane-varying radix-4 round, with the I-only round straight behind it), 2^16 (S = 6: the first lane-varying pure round before a
uniform one), 2^17 and 2^19 (S = 7, 9: the plan keeps ln::mul in these first passes -- their ln::mul2 instantiations need scratch -- and
splits the coset pass alone), 2^18 (S = 8: the headline's two instantiations), 2^20 (S = 10: three lane-varying pure rounds).  The pure /
coset form is forced below 2^16 columns, where the default plan is the DIF form (which has no ln::mul2).  Fills: a quarter, a half and
all of n_cols (the API wants n_per_row < n_cols: n_cols - 1); 1 and 3 rows.  The switches are read when an encoder is created, so both
multipliers live in one process.

Worst-case operands: rows whose values entering a DIF stage are all p - 1, alternating 0 / p - 1, or the element with every low limb of
the limb form at 2^29 - 1 (tests/common.py stage_input_rows), at stage 0, both sides of the pass boundary and inside the last pass.

ln::mul2 itself, once per lane at the extremes of its stated input ranges, through tests/native/mul2_harness.cpp."""
import ctypes as C
import os
import random

import numpy as np
import pytest

import harness_kit as K
from common import field_p, ntt_maxlimb, stage_input_rows
from lcpc_amd import LcCommit, LigeroEncoding

pytestmark = pytest.mark.gpu
FID = 3
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _enc(mul, n_per_row, n_cols, rho):
    env = {"LCPC_NTT_MUL": mul}
    if n_cols < 1 << 16:
        env["LCPC_NTT_FORM"] = "coset"
    os.environ.update(env)                               # (switches are read once, when an encoder is created)
    try:
        return LigeroEncoding.new_from_dims(FID, n_per_row, n_cols, rho=rho)
    finally:
        for k in env:
            del os.environ[k]


FILLS = {"quarter": lambda n: (n // 4, (1, 4)), "half": lambda n: (n // 2, (1, 2)), "full": lambda n: (n - 1, (38, 39))}


def _check(O, coeffs, n_rows, n_per_row, n_cols, rho, what):
    oc = O.Commit.commit(coeffs, O.Encoding.ligero_from_dims(FID, n_per_row, n_cols, rho=rho), n_threads=16)
    rows = np.zeros((n_rows, n_cols, 4), np.uint64)
    rows[:, :n_per_row] = coeffs.reshape(n_rows, n_per_row, 4)
    rows = rows.reshape(-1, 4)
    got = {}
    for mul in ("split", "mont"):
        enc = _enc(mul, n_per_row, n_cols, rho)
        c = LcCommit.commit(coeffs, enc)
        got[mul] = (c.comm(), c.get_root(), enc.encode(rows))
        assert (got[mul][0] == oc.comm()).all(), (what, mul, "comm")
        assert (c.hashes() == oc.hashes()).all() and got[mul][1] == oc.get_root(), (what, mul, "root")
        assert (got[mul][2] == oc.comm()).all(), (what, mul, "encode")      # the Montgomery-output path: the oracle's comm is in that form
    assert (got["split"][0] == got["mont"][0]).all() and got["split"][1] == got["mont"][1] and (got["split"][2] == got["mont"][2]).all()


@pytest.mark.parametrize("n_rows", [1, 3])
@pytest.mark.parametrize("fill", list(FILLS))
@pytest.mark.parametrize("log_n", [11, 12, 13, 15, 16, 17, 18, 19, 20])
def test_split_is_the_oracle_and_mont(oracle, log_n, fill, n_rows):
    O = oracle
    n_cols = 1 << log_n
    n_per_row, rho = FILLS[fill](n_cols)
    coeffs = O.random_elems(FID, n_rows * n_per_row, log_n * 7 + len(fill) + n_rows)
    _check(O, coeffs, n_rows, n_per_row, n_cols, rho, (log_n, fill, n_rows))


def _worst_stages(log_n):
    S = log_n - 10
    if log_n == 20:
        return [0, S - 1, S + 4]
    return sorted({0, S - 1, S, S + 4, S + 5, log_n - 1})


@pytest.mark.parametrize("log_n", [11, 13, 15, 16, 18, 20])
def test_split_worst_case_operands(oracle, log_n):
    """one row per (pattern, stage); rate 1/2.  The patterns are what the existing worst-case row-NTT test feeds ln::mul."""
    O = oracle
    p, n = field_p(FID), 1 << log_n
    stages = _worst_stages(log_n)
    pats = [[p - 1], [0, p - 1]] + ([[ntt_maxlimb(FID)]] if log_n < 20 else [])
    rows = np.concatenate([stage_input_rows(FID, log_n, stages, pat, 1) for pat in pats])
    _check(O, rows.reshape(-1, 4), rows.shape[0], n // 2, n, (1, 2), (log_n, "worst"))


PLAN_LOGS = (11, 12, 13, 15, 16, 17, 18, 19, 20)
PLAN_ENVS = [{"LCPC_NTT_MUL": "split", "LCPC_NTT_FORM": "coset"}, {"LCPC_NTT_MUL": "mont", "LCPC_NTT_FORM": "coset"},
             {"LCPC_NTT_MUL": "split-pure", "LCPC_NTT_FORM": "coset"}, {"LCPC_NTT_MUL": "split-coset", "LCPC_NTT_FORM": "coset"},
             {"LCPC_NTT_MUL": "split"}, {}]
PLAN_CHILD = """
import os, sys
sys.path[:0] = %r
from lcpc_amd import LigeroEncoding
for i, env in enumerate(%r):
    os.write(2, b"== env %%d\\n" %% i)
    os.environ.update(env)                 # (read when an encoder is created)
    for log_n in %r:
        LigeroEncoding.new_from_dims(3, 1 << (log_n - 1), 1 << log_n)
    for k in env:
        del os.environ[k]
"""


def _plans():
    """per PLAN_ENVS entry {log_n: [(form, mul2) of the first pass, of the last pass]}, as the context reports its plan on stderr under
    LCPC_DEBUG_TIMING (ctx.cpp build_limb_plan); one child process creates every encoder"""
    import re
    import subprocess
    import sys
    paths = [ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "oracle")]
    e = dict(os.environ, LCPC_DEBUG_TIMING="1")
    for k in ("LCPC_NTT_MUL", "LCPC_NTT_FORM"):
        e.pop(k, None)
    r = subprocess.run([sys.executable, "-c", PLAN_CHILD % (paths, PLAN_ENVS, PLAN_LOGS)], capture_output=True, text=True, env=e, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    parts = r.stderr.split("== env ")[1:]
    assert len(parts) == len(PLAN_ENVS), r.stderr[-3000:]
    res = []
    for part in parts:
        out = {}
        for m in re.finditer(r"ntt plan 2\^(\d+) pass (\d)/2: K1s s=(\d+) form=(\d) mul2=(\d)", part):
            out.setdefault(int(m.group(1)), []).append((int(m.group(4)), int(m.group(5))))
        assert sorted(out) == list(PLAN_LOGS) and all(len(v) == 2 for v in out.values()), part[-3000:]
        res.append(out)
    return res


def test_the_plan_selects_mul2_where_the_cases_above_say():
    """what the comparisons above cannot see: that `split` really runs ln::mul2.  Forced with the coset form: both passes of every shape but
    the first passes of 2^12, 2^17, 2^19 (no instantiation); `mont`: none; one pass alone; `split` without the form forced: the DIF
    form below 2^16 columns has no ln::mul2; unset: nothing below 2^16 columns, and only passes that have the instantiation."""
    no_first = {12, 17, 19}
    split, mont, pure, coset, split_free, dflt = _plans()
    assert split == {k: [(1, 0 if k in no_first else 1), (1, 1)] for k in PLAN_LOGS}
    assert mont == {k: [(1, 0), (1, 0)] for k in PLAN_LOGS}
    assert pure == {k: [(1, 0 if k in no_first else 1), (1, 0)] for k in PLAN_LOGS}
    assert coset == {k: [(1, 0), (1, 1)] for k in PLAN_LOGS}
    assert split_free == {k: [(0, 0), (0, 0)] if k < 16 else split[k] for k in PLAN_LOGS}
    assert all(dflt[k] == [(0, 0), (0, 0)] for k in PLAN_LOGS if k < 16)
    assert all(f == 1 for k in PLAN_LOGS if k >= 16 for f, _ in dflt[k])
    assert all(dflt[k][i][1] <= split[k][i][1] for k in PLAN_LOGS for i in (0, 1))
    assert dflt[18] == [(1, 1), (1, 1)]                       # (the headline; LABNOTES has the measurements the rest follows)


# ---- ln::mul2 and ln::mul2_pair, one call per lane --------------------------------------------------------------------------------------
W, N = 29, 9
M = (1 << W) - 1


M2H_SYMBOLS = {"m2h_device_count": [], "m2h_mul2": [C.c_void_p] * 4 + [C.c_uint32] * 2, "m2h_pair": [C.c_void_p] * 3 + [C.c_uint32] * 2}


def _h():
    return K.load("mul2", M2H_SYMBOLS)


def _arr(elems):
    return np.array([[v & 0xffffffff for v in e] for e in elems], np.uint32)


def _val(limbs):
    return sum((int(v) - (1 << 32) if k == N - 1 and int(v) >> 31 else int(v)) << (W * k) for k, v in enumerate(limbs))


def _limbs(v):
    return [(v >> (W * k)) & M for k in range(N)]


def test_mul2_primitive_at_its_input_extremes():
    p = field_p(FID)
    rng = random.Random(2)
    T = (1 << 30) - 1
    ws = [p - 1, 0, 1, (p - 1) // 2] + [rng.randrange(p) for _ in range(4)]
    xs, lo_hi = [], []
    for s in range(1 << N):                               # every limb at +-(2^30 - 1)
        xs.append([T if (s >> k) & 1 else -T for k in range(N)])
        lo_hi.append((-3.01, 2.01))
    for _ in range(256):                                  # differences of two normalised values: limbs 0-7 at +-(2^29 - 1) or random
        xs.append([rng.choice([-M, M, 0, rng.randrange(-M, M + 1)]) for _ in range(N - 1)] + [rng.randrange(-(1 << 25), 1 << 25)])
        lo_hi.append((-2.01, 1.01))
    for v in [0, p - 1, 4 * p - 1, -(4 * p - 1), -1] + [rng.randrange(-4 * p + 1, 4 * p) for _ in range(251)]:   # normalised, |value| < 4p
        xs.append([(v >> (W * k)) & M for k in range(N - 1)] + [v >> (W * (N - 1))])
        lo_hi.append((-1.01, 1.01))
    n = len(xs)
    wl = [ws[i % len(ws)] if i % 3 else p - 1 for i in range(n)]
    x = _arr(xs)
    b0, b1 = _arr([_limbs((w << 145) % p) for w in wl]), _arr([_limbs((w << 290) % p) for w in wl])
    out = np.full((n + 1, N), 0xA5C3F00D, np.uint32)
    L = _h()
    assert L.m2h_mul2(x.ctypes.data, b0.ctypes.data, b1.ctypes.data, out.ctypes.data, n, n + 1) == 0
    assert (out[n] == 0xA5C3F00D).all()
    for i in range(n):
        xv = sum(v << (W * k) for k, v in enumerate(xs[i]))
        if lo_hi[i][0] == -2.01 and abs(xv) >= 8 * p:
            continue                                      # (the stated range is for |value| < 8p; the limb-only bound holds regardless)
        r = _val(out[i])
        assert all(int(v) <= M for v in out[i][:N - 1]), i
        assert (r - xv * wl[i]) % p == 0, i
        assert lo_hi[i][0] * p < r < lo_hi[i][1] * p, (i, r / p)
    # the pack kernels' pair from a table entry e = w 2^261 (and from the converting entry w 2^5): fully reduced b0, b1
    es = [(w << 261) % p for w in ws] + [(w << 5) % p for w in ws]
    e = _arr([_limbs(v) for v in es])
    o0 = np.zeros((len(es), N), np.uint32)
    o1 = np.zeros((len(es), N), np.uint32)
    assert L.m2h_pair(e.ctypes.data, o0.ctypes.data, o1.ctypes.data, len(es), len(es)) == 0
    i116 = pow(2, -116, p)
    for i, v in enumerate(es):
        assert _val(o0[i]) == v * i116 % p and _val(o1[i]) == (v << 29) % p, i
        assert all(int(t) <= M for t in o0[i][:N - 1]) and all(int(t) <= M for t in o1[i][:N - 1])

"""Operand sets and Python-int models for the direct tests of the device field primitives (lcpc_amd/csrc/field_dev.h, field_ln.h; the
arithmetic `#[derive(PrimeField)]` gives the reference's four test fields, lcpc-test-fields/src/lib.rs:13-59).  CPU only.

Every primitive states a contract in its comment: the operands it accepts, the value it returns and the range that value lies in.
This file holds, per primitive, the exact model of that contract as Python integers (m_*), the precondition (pre_*) and the operand
sets that sit on the edges of the precondition and never outside it; tests/test_gpu_fe_primitives.py runs the sets on the device
through tests/fe_harness.py and tests/test_host_field.py runs the packed ones through host_field.h.  The tests of this file check the
sets against the models alone: every operand is in contract, the models agree with oracle/pyref.py, and each set reaches the
branches it was built for.

The tables the limb primitives read (the clamp table (i - QOFF) p, its limb-wise negation, the shifted multiples of mul_u) are built
here from the layouts field_ln.h and ctx.cpp describe, not by ctx.cpp: the primitives are tested on these models of the tables.  That
the tables the product builds for itself (ctx.cpp, kernels.hip, ntt_lns.hip) ARE these models, word for word, is what
tests/test_gpu_k1_tables.py checks on real contexts, with clamp_table and shifted_multiples below as its references."""
import functools
import os
import random
import re
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path[:0] = [HERE, os.path.join(ROOT, "oracle")]
import common as CM  # noqa: E402
import pyref as P  # noqa: E402
import wmul_sim as G  # noqa: E402

FIDS = [0, 1, 2, 3]
LIMB_DOT_FIDS = [1, 2, 3]          # has_mul_u; the fields whose kernels use lazy_mac / lazy_reduce
FIELD_NAME = {0: "ft63", 1: "ft127", 2: "ft191", 3: "ft255"}
WIDE_KS = [0, 1, 2, 7, 8, 9, 64, 255]
LAZY_KS = [0, 1, 5, 6, 7, 59, 60]


# The clamp contract as field_ln.h states it, written out here and not read from the header: clamp table entry i = (i - QOFF) p, and the
# quotient estimate floor((top limb - QBIAS) / (PTOP + 1)).  The models below follow these two numbers, so a header that drifts from its
# documented contract makes the device disagree with them (test_documented_clamp_constants checks the header's text on the CPU as well).
QOFF, QBIAS = 24, 40


class Fld:
    """the constants of one field in both device forms: NL packed 32-bit words (R = 2^(32 NL)) and N limbs of W bits (R' = 2^(N W))"""

    def __init__(self, fid):
        self.fid, self.p = fid, P.FIELDS[fid].p
        self.NL = 2 * CM.FIELD_L[fid]
        self.N, self.W = CM.LN_SHAPE[fid]
        self.STRIDE = CM.LN_STRIDE[fid]
        self.M = (1 << self.W) - 1
        self.R = 1 << (32 * self.NL)
        self.Rinv = pow(self.R, -1, self.p)
        self.pinv = pow(self.p, -1, self.R)
        self.Rl = 1 << (self.N * self.W)
        self.Rlinv = pow(self.Rl, -1, self.p)
        self.B = 1 << (self.W * (self.N - 1))
        self.PTOP1 = self.p // self.B + 1
        assert 2 * self.p < self.R and self.p < self.Rl and self.p % (1 << 32) == 1

    # limb form
    def limbs(self, v):
        """the normalised limbs of a signed integer: limbs 0..N-2 in [0, 2^W), the top limb takes the rest (signed)"""
        return [(v >> (self.W * k)) & self.M for k in range(self.N - 1)] + [v >> (self.W * (self.N - 1))]

    def value(self, l):
        return sum(x << (self.W * k) for k, x in enumerate(l))

    def normalised(self, l):
        return all(0 <= x <= self.M for x in l[:-1]) and -(1 << 31) <= l[-1] < 1 << 31


@functools.lru_cache(None)
def fld(fid):
    return Fld(fid)


def rng(fid, salt):
    return random.Random(0xFE0000 + 97 * salt + fid)


# ---- models: packed layer -----------------------------------------------------------------------------------------------------------
def m_add(F, a, b):
    return (a + b) % F.p


def m_sub(F, a, b):
    return (a - b) % F.p


def m_cios(F, a, b):
    """the value fe_mul hands fe_reduce_once: (a b + m p) / R with m = -a b / p mod R, in [0, 2p)"""
    ab = a * b
    m = (-ab * F.pinv) % F.R
    t, rem = divmod(ab + m * F.p, F.R)
    assert rem == 0 and 0 <= t < 2 * F.p
    return t


def m_mul(F, a, b):
    return m_cios(F, a, b) % F.p


def m_canon(F, a):
    return a * F.Rinv % F.p


def pre_reduce_once(F, T):
    return 0 <= T < 2 * F.p


def m_reduce_once(F, T):
    return T - F.p if T >= F.p else T


def m_wide(F, a, b):
    """wide_mac over the pairs, then wide_reduce: V = (S + m p) / R kept as (top word : NL words), then p subtracted while V >= p.
    -> (result, top word before the loop, subtractions)"""
    S = sum(x * y for x, y in zip(a, b))
    assert S < 1 << (32 * (2 * F.NL + 1))
    m = (-S * F.pinv) % F.R
    V, rem = divmod(S + m * F.p, F.R)
    assert rem == 0 and V < 1 << (32 * (F.NL + 1))
    return V % F.p, V >> (32 * F.NL), V // F.p


# ---- models: limb layer -------------------------------------------------------------------------------------------------------------
def m_from_packed(F, a):
    return F.limbs(a)


def pre_to_packed(F, l):
    return all(0 <= x <= F.M for x in l[:-1]) and l[-1] >= 0 and F.value(l) < F.R


def pre_normalize(F, l):
    """|limb| < 2^31, and no carry pushes the next limb out of an i32"""
    c = 0
    for k, x in enumerate(l):
        if not -(1 << 31) < x < 1 << 31 or not -(1 << 31) <= x + c < 1 << 31:
            return False
        c = (x + c) >> F.W
    return True


def m_normalize(F, l):
    return F.limbs(F.value(l))


def clamp_low_max(F):
    """the largest lower limb of a clamp_q / clamp_apply operand: the sum of four normalised values"""
    return 4 * F.M


def pre_clamp_qa(F, l):
    return all(0 <= x <= clamp_low_max(F) for x in l[:-1]) and -(1 << 31) <= l[-1] < 1 << 31 and abs(F.value(l)) < 16 * F.p


def m_clamp_q(F, top):
    """the table index: floor((top - QBIAS) / (PTOP + 1)) + QOFF"""
    return (top - QBIAS) // F.PTOP1 + QOFF


def m_clamp_qa(F, l):
    """-> (normalised limbs of V - q p, the index); promised range [0, p + 64 B)"""
    i = m_clamp_q(F, l[-1])
    return F.limbs(F.value(l) - (i - QOFF) * F.p), i


def clamp_qa_range(F):
    return 0, F.p + 64 * F.B


def pre_clamp9(F, l):
    return F.fid == 3 and F.normalised(l) and abs(F.value(l)) < 16 * F.p


def m_clamp9(F, l):
    """ln::clamp: normalised in, V - q p out; promised range [0, p + 2^239)"""
    return F.limbs(F.value(l) - (m_clamp_q(F, l[-1]) - QOFF) * F.p)


def pre_mul(F, a, w):
    lim = 1 << (F.W + 1)
    return all(-lim < x < lim for x in a) and abs(F.value(a)) < 16 * F.p and F.normalised(w) and 0 <= F.value(w) < F.p


def mul_range(F):
    """(lo, hi] of ln::mul's result: (-p - eps, eps], eps = 16 p^2 / R'"""
    eps = -(-16 * F.p * F.p // F.Rl)
    return -F.p - eps, eps


def m_mul_mod(F, a, w):
    return F.value(a) * F.value(w) * F.Rlinv % F.p


def pre_mul_u(F, a):
    return sum(abs(x) for x in a) < F.N << F.W and all(-(1 << 31) <= x < 1 << 31 for x in a)


def mul_u_range(F):
    """[lo, hi) of mul_u's result, from the generator's own proof (tests/wmul_sim.py wmul_bounds)"""
    lo, hi = G.wmul_bounds(FIELD_NAME[F.fid])
    return lo * F.p, hi * F.p


def m_lazy_dot(F, x, v):
    return sum(a * F.value(b) for a, b in zip(x, v)) * F.Rlinv % F.p


def pre_lazy_operand(F, x, v):
    return 0 <= x < F.p and all(0 <= l <= F.M for l in v) and F.value(v) < F.p


# ---- tables, built from the layouts in field_ln.h / ctx.cpp's comments -----------------------------------------------------------------
def clamp_table(F):
    """entry i = (i - QOFF) p as normalised signed limbs, STRIDE words per entry: (64, STRIDE) uint32"""
    t = np.zeros((64, F.STRIDE), np.uint32)
    for i in range(64):
        t[i, :F.N] = [x & 0xFFFFFFFF for x in F.limbs((i - QOFF) * F.p)]
    return t


def clamp_table_negated(F):
    """what the row-NTT kernels keep in LDS: every word of the table negated"""
    return ((1 << 32) - clamp_table(F).astype(np.uint64)).astype(np.uint32)


def shifted_multiples(F, w):
    """mul_u's table of the plain residue w: word N k + j = limb k of balanced(w 2^(W j) mod p)"""
    tab = []
    for k in range(F.N):
        for j in range(F.N):
            v = (w << (F.W * j)) % F.p
            if v > (F.p - 1) // 2:
                v -= F.p
            tab.append(F.limbs(v)[k] & 0xFFFFFFFF)
    return tab


# ---- the edge set -------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(None)
def edge_set(fid):
    F = fld(fid)
    p, r = F.p, rng(fid, 1)
    v = {0, 1, 2, p - 1, p - 2, (p - 1) // 2, (p + 1) // 2}
    for s in sorted({32 * i for i in range(1, F.NL)} | {F.W * k for k in range(1, F.N)}):
        if 1 << s < p:
            v |= {(1 << s) - 1, 1 << s, (1 << s) + 1, p - (1 << s) - 1, p - (1 << s), p - (1 << s) + 1}
    v |= {CM.maxc(fid), CM.maxt(fid), CM.ln_maxx(fid), CM.ln_maxv(fid)}
    v |= {CM.maximal_limbs(fid, 32, n) for n in range(1, F.NL)} | {CM.maximal_limbs(fid, F.W, n) for n in range(1, F.N)}
    for i in range(1, F.NL):                    # low i words all ones, word i zero, the words above as p has them
        hi = (p >> (32 * (i + 1))) << (32 * (i + 1))
        v.add(hi | ((1 << (32 * i)) - 1))
    rnd = [r.randrange(p) for _ in range(50)]
    out = sorted(x for x in v if 0 <= x < p)
    return out + [x for x in rnd if x not in v]


def random_set(fid, n=50):
    return edge_set(fid)[-n:]


@functools.lru_cache(None)
def binary_pairs(fid, op):
    """E x E and the pairs built to sit on the final subtraction / the borrow"""
    F, E = fld(fid), edge_set(fid)
    pairs = [(a, b) for a in E for b in E]
    if op == "add":
        for a in E:
            pairs += [(a, (F.p - a + d) % F.p) for d in (0, -1, 1) if 0 <= F.p - a + d < F.p]
    elif op == "sub":
        for a in E:
            pairs += [(a, a), (0, a), (a, 0)] + ([(a, a + 1)] if a + 1 < F.p else [])
    return pairs


@functools.lru_cache(None)
def reduce_once_set(fid):
    """T in [0, 2p): the corners, every edge value below p and shifted into [p, 2p)"""
    F = fld(fid)
    p = F.p
    return [0, 1, p - 1, p, p + 1, 2 * p - 1] + list(edge_set(fid)) + [p + e for e in edge_set(fid)]


def split_top(F, T):
    """(low NL words, top word) of the (t, top) form.  No field here has 2p > 2^(32 NL), so inside the contract [0, 2p) the top word
    is 0 for every one of them (checked in test_reduce_once_set)"""
    return T % F.R, T // F.R


def _dot_lanes(fid, k, big, salt):
    """the operand rows of a k-term dot product: all p - 1, all `big`, mixed and random ones"""
    F, r = fld(fid), rng(fid, salt + k)
    pool = [F.p - 1, big]
    rows = [([F.p - 1] * k, [F.p - 1] * k), ([big] * k, [big] * k)]
    for _ in range(3):
        rows.append(([r.choice(pool) if r.random() < 0.8 else r.randrange(F.p) for _ in range(k)],
                     [r.choice(pool) if r.random() < 0.8 else r.randrange(F.p) for _ in range(k)]))
    for _ in range(3):
        rows.append(([r.randrange(F.p) for _ in range(k)], [r.randrange(F.p) for _ in range(k)]))
    rows.append(([0] * k, [F.p - 1] * k))
    return rows


@functools.lru_cache(None)
def wide_dot_set(fid, k):
    return _dot_lanes(fid, k, CM.maxc(fid), 1000)


@functools.lru_cache(None)
def lazy_dot_set(fid, k):
    """x: packed elements; v: limb rows of values < p (the R'-form matrix / tensor values)"""
    F = fld(fid)
    return [(x, [F.limbs(b) for b in v]) for x, v in _dot_lanes(fid, k, CM.ln_maxx(fid), 2000)]


# ---- limb-layer operand sets ----------------------------------------------------------------------------------------------------------
def _normalised_values(fid):
    """normalised values on the edge of |value| < 16 p and around every multiple of p inside it"""
    F = fld(fid)
    p = F.p
    v = {16 * p - 1, -(16 * p - 1), 0, -1}
    for k in range(-15, 16):
        v |= {k * p - 1, k * p, k * p + 1}
    return sorted(v)


@functools.lru_cache(None)
def packed_any_set(fid):
    """values < 2^(32 NL) for from_packed / to_packed: the edge set, all ones, and a set bit on either side of every limb / word straddle"""
    F = fld(fid)
    v = set(edge_set(fid)) | {F.R - 1, F.R - 2, F.R >> 1, (F.R >> 1) - 1}
    for s in sorted({32 * i for i in range(1, F.NL)} | {F.W * k for k in range(1, F.N)}):
        v |= {1 << s, 1 << (s - 1), (1 << s) - 1, (1 << (s + 1)) - 1, F.R - (1 << s), F.R - 1 - (1 << s), F.R - 1 - (1 << (s - 1))}
    return sorted(x for x in v if 0 <= x < F.R)


@functools.lru_cache(None)
def normalize_set(fid):
    F, r = fld(fid), rng(fid, 3)
    nv = [F.limbs(v) for v in _normalised_values(fid)]
    rows = list(nv)
    some = nv + [F.limbs(r.randrange(-4 * F.p, 4 * F.p)) for _ in range(20)] + [F.limbs(CM.ln_maxx(fid)), F.limbs(-CM.ln_maxx(fid) - 1)]
    for _ in range(60):                               # sums of four, differences of two
        a, b, c, d = (r.choice(some) for _ in range(4))
        rows.append([w + x + y + z for w, x, y, z in zip(a, b, c, d)])
        rows.append([w - x for w, x in zip(a, b)])
        rows.append([w - x - y - z for w, x, y, z in zip(a, b, c, d)])
    big = (1 << 31) - 64                              # the carry out of a limb of this size is < 2^(31 - W) <= 32
    for sg in (1, -1):
        rows.append([sg * big] * (F.N - 1) + [sg * 5])
        rows.append([sg * big * (-1) ** k for k in range(F.N - 1)] + [-sg * 7])
        rows.append([sg * F.M] * (F.N - 1) + [sg])
        rows.append([sg * (F.M + 1)] * (F.N - 1) + [0])
        rows.append([sg] + [0] * (F.N - 1))
    rows.append([-1] * F.N)
    return [l for l in rows if pre_normalize(F, l)]


def clamp_q_allowed(F, low_max_value):
    """every table index a top limb can give under |V| < 16 p, V = t B + low, 0 <= low <= low_max_value"""
    t_min = -((16 * F.p - 1 + low_max_value) // F.B)
    t_max = (16 * F.p - 1) // F.B
    return set(range(m_clamp_q(F, t_min), m_clamp_q(F, t_max) + 1))


def _clamp_rows(fid, low_patterns):
    """top limbs on both sides of every step of the quotient estimate (t - QBIAS == 0, -1 mod PTOP + 1) and at the two ends of
    |V| < 16 p, over the given lower-limb patterns"""
    F = fld(fid)
    rows = []
    for low in low_patterns:
        lv = F.value(low + [0])
        t_lo, t_hi = -((16 * F.p - 1 + lv) // F.B), (16 * F.p - 1 - lv) // F.B
        tops = {t_lo, t_lo + 1, t_hi - 1, t_hi, 0, -1, 1}
        for i in range(64):
            t = QBIAS + (i - QOFF) * F.PTOP1
            tops |= {t - 1, t, t + 1, t + F.PTOP1 // 2}
        rows += [low + [t] for t in sorted(tops) if t_lo <= t <= t_hi]
    return rows


@functools.lru_cache(None)
def clamp_qa_set(fid):
    """clamp_q + clamp_apply: un-normalised sums of four normalised values (lower limbs up to 4 (2^W - 1)), |V| < 16 p"""
    F, r = fld(fid), rng(fid, 4)
    n1, top = F.N - 1, clamp_low_max(F)
    pats = [[0] * n1, [top] * n1, [F.M] * n1, [F.M + 1] * n1, [top if k % 2 else 0 for k in range(n1)], [1] + [0] * (n1 - 1)]
    pats += [[r.randrange(top + 1) for _ in range(n1)] for _ in range(2)]
    rows = _clamp_rows(fid, pats)
    nv = [F.limbs(v) for v in _normalised_values(fid)]
    rows += nv
    quarter = [F.limbs(r.randrange(-4 * F.p + 1, 4 * F.p)) for _ in range(40)] + [F.limbs(4 * F.p - 1), F.limbs(-4 * F.p + 1), F.limbs(CM.ln_maxx(fid))]
    for _ in range(80):
        a, b, c, d = (r.choice(quarter) for _ in range(4))
        rows.append([w + x + y + z for w, x, y, z in zip(a, b, c, d)])
    rows.append([4 * x for x in F.limbs(4 * F.p - 1)])
    rows.append([4 * x for x in F.limbs(-4 * F.p + 1)])
    return [l for l in rows if pre_clamp_qa(F, l)]


@functools.lru_cache(None)
def clamp9_set():
    """ln::clamp / ln::to_packed_reduced (Ft255): normalised values, |V| < 16 p"""
    F, r = fld(3), rng(3, 5)
    n1 = F.N - 1
    pats = [[0] * n1, [F.M] * n1, [F.M if k % 2 else 0 for k in range(n1)], [1] + [0] * (n1 - 1)]
    pats += [[r.randrange(F.M + 1) for _ in range(n1)] for _ in range(2)]
    rows = _clamp_rows(3, pats) + [F.limbs(v) for v in _normalised_values(3)]
    rows += [F.limbs(r.randrange(-16 * F.p + 1, 16 * F.p)) for _ in range(60)]
    rows += [F.limbs(e) for e in edge_set(3)]
    return [l for l in rows if pre_clamp9(F, l)]


@functools.lru_cache(None)
def mul_a_set(fid):
    """ln::mul's left operand: limbs in (-2^(W+1), 2^(W+1)), |value| < 16 p"""
    F, r = fld(fid), rng(fid, 6)
    n1, big = F.N - 1, (1 << (F.W + 1)) - 1
    rows = [F.limbs(v) for v in _normalised_values(fid)]
    t16 = (16 * F.p) // F.B
    for sg in (1, -1):
        for top in (0, sg * (t16 - 3), -sg * (t16 - 3), sg * (t16 // 2)):
            rows.append([sg * big] * n1 + [top])
            rows.append([sg * big * (-1) ** k for k in range(n1)] + [top])
        rows.append([sg * big] + [0] * n1)
        rows.append([0] * (n1 - 1) + [sg * big, 0])
    some = [F.limbs(r.randrange(-4 * F.p, 4 * F.p)) for _ in range(12)] + [F.limbs(CM.ln_maxx(fid))]
    for _ in range(12):
        a, b = r.choice(some), r.choice(some)
        rows.append([x + y for x, y in zip(a, b)])
        rows.append([x - y for x, y in zip(a, b)])
    w0 = F.limbs(0)
    return [l for l in rows if pre_mul(F, l, w0)]


@functools.lru_cache(None)
def mul_set(fid):
    """(a, w) pairs: every a against every edge value as w"""
    F = fld(fid)
    return [(a, F.limbs(w)) for a in mul_a_set(fid) for w in edge_set(fid)]


@functools.lru_cache(None)
def mul_u_ws(fid):
    F, r = fld(fid), rng(fid, 7)
    p = F.p
    return [1, p - 1, (p - 1) // 2, (p + 1) // 2, 2, p - 2, CM.ln_maxx(fid), pow(2, F.W, p)] + [r.randrange(1, p) for _ in range(4)]


@functools.lru_cache(None)
def mul_u_a_set(fid):
    """mul_u's left operand: a normalised value (|value| < 4 p, invariant I) or the difference of two"""
    F, r = fld(fid), rng(fid, 8)
    p = F.p
    vals = [0, 1, -1, p, -p, p - 1, 1 - p, 4 * p - 1, 1 - 4 * p, 2 * p, -2 * p, CM.ln_maxx(fid), -CM.ln_maxx(fid) - 1, F.B - 1, -F.B,
            4 * p - F.B, ((4 * p - 1) >> (F.W * (F.N - 1)) << (F.W * (F.N - 1))) - 1]
    vals += [r.randrange(-4 * p + 1, 4 * p) for _ in range(40)]
    nv = [F.limbs(v) for v in vals if abs(v) < 4 * p]
    rows = list(nv)
    for i, a in enumerate(nv):
        b = nv[(7 * i + 3) % len(nv)]
        rows.append([x - y for x, y in zip(a, b)])
    rows.append([x - y for x, y in zip(F.limbs(F.B - 1), F.limbs(-F.B))])          # every lower limb at its extreme
    rows.append([y - x for x, y in zip(F.limbs(F.B - 1), F.limbs(-F.B))])
    return [l for l in rows if pre_mul_u(F, l)]


@functools.lru_cache(None)
def r29_set():
    """fe_mul_r29: (packed a < p, b as 9 limbs < 2^29 of a value < p)"""
    F = fld(3)
    E = edge_set(3)
    return [(a, F.limbs(b)) for a in E for b in E]


# ---- the tests of this file ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fid", FIDS)
def test_edge_set(fid):
    F, E = fld(fid), edge_set(fid)
    assert all(0 <= v < F.p for v in E) and len(set(E)) == len(E) and 70 <= len(E) <= 220
    for v in (0, 1, F.p - 1, (F.p + 1) // 2, CM.maxc(fid), CM.ln_maxx(fid), (1 << 32) - 1, 1 << 32, F.p - (1 << 32)):
        assert v in E
    words = lambda v: [(v >> (32 * i)) & 0xFFFFFFFF for i in range(F.NL)]
    for i in range(1, F.NL):                    # low i words all ones with a zero word above them: a carry ripples through and stops
        assert any(words(v)[:i] == [0xFFFFFFFF] * i and words(v)[i] == 0 for v in E), i


def test_documented_clamp_constants():
    """field_ln.h declares the constants the models state"""
    t = open(os.path.join(ROOT, "lcpc_amd", "csrc", "field_ln.h")).read()
    got = {n: int(re.search(r"constexpr int %s = (\d+);" % n, t).group(1)) for n in ("QOFF", "QBIAS")}
    assert got == {"QOFF": QOFF, "QBIAS": QBIAS}


@pytest.mark.parametrize("fid", FIDS)
def test_models_agree_with_pyref(fid):
    F, PF, r = fld(fid), P.FIELDS[fid], rng(fid, 9)
    assert F.R % F.p == PF.R and F.NL * 32 == PF.L * 64
    for _ in range(200):
        a, b = r.randrange(F.p), r.randrange(F.p)
        ca, cb = PF.from_mont(a), PF.from_mont(b)
        assert m_add(F, a, b) == PF.to_mont((ca + cb) % F.p)
        assert m_sub(F, a, b) == PF.to_mont((ca - cb) % F.p)
        assert m_mul(F, a, b) == PF.to_mont(ca * cb % F.p)
        assert m_canon(F, a) == ca
        assert m_wide(F, [a, b], [b, a])[0] == PF.to_mont(2 * ca * cb % F.p)
        assert F.value(F.limbs(a - b)) == a - b and F.normalised(F.limbs(a - b))
        # the limb multiplies keep the stored form when the twiddle is pre-scaled: REDC_R'(a R * w R') = (a w) R
        w_rl = cb * F.Rl % F.p
        assert m_mul_mod(F, F.limbs(a), F.limbs(w_rl)) == PF.to_mont(ca * cb % F.p)
        assert m_lazy_dot(F, [a], [F.limbs(w_rl)]) == PF.to_mont(ca * cb % F.p)


@pytest.mark.parametrize("fid", FIDS)
def test_binary_sets_reach_both_branches(fid):
    F = fld(fid)
    add, sub = binary_pairs(fid, "add"), binary_pairs(fid, "sub")
    assert all(0 <= a < F.p and 0 <= b < F.p for a, b in add + sub)
    assert len(edge_set(fid)) ** 2 < len(add) < 60000
    sums = {a + b for a, b in add}
    assert F.p in sums and F.p - 1 in sums and F.p + 1 in sums and any(s < F.p for s in sums) and any(s > F.p for s in sums)
    assert any(a == b and a for a, b in sub) and any(a + 1 == b for a, b in sub) and any(a > b for a, b in sub) and any(a < b for a, b in sub)
    cios = [m_cios(F, a, b) for a, b in binary_pairs(fid, "mul")]
    assert any(t >= F.p for t in cios) and any(t < F.p for t in cios)


@pytest.mark.parametrize("fid", FIDS)
def test_reduce_once_set(fid):
    F = fld(fid)
    S = reduce_once_set(fid)
    assert all(pre_reduce_once(F, T) for T in S)
    assert {0, F.p - 1, F.p, F.p + 1, 2 * F.p - 1} <= set(S)
    assert all(0 <= m_reduce_once(F, T) < F.p and (m_reduce_once(F, T) - T) % F.p == 0 for T in S)
    # 2p < 2^(32 NL) for every field: no value of [0, 2p) has a top word, so the (t, top) form is in contract with top = 0 only
    assert 2 * F.p <= F.R and {split_top(F, T)[1] for T in S} == {0}


@pytest.mark.parametrize("fid", FIDS)
def test_wide_dot_sets(fid):
    F = fld(fid)
    tops, loops = 0, 0
    for k in WIDE_KS:
        for a, b in wide_dot_set(fid, k):
            assert len(a) == k == len(b) and all(0 <= x < F.p for x in a + b)
            res, top, n_sub = m_wide(F, a, b)
            assert res == sum(x * y for x, y in zip(a, b)) * F.Rinv % F.p
            tops, loops = max(tops, top), max(loops, n_sub)
    assert tops > 0 and loops >= 3


@pytest.mark.parametrize("fid", LIMB_DOT_FIDS)
def test_lazy_dot_sets(fid):
    import test_lazy_bounds as LB
    F = fld(fid)
    assert {v[0][0] for v in LB.lazy29_cadences().values()} == {6} and max(LAZY_KS) <= 60
    acc = LB.ln_acc(fid)
    for k in LAZY_KS:
        for x, v in lazy_dot_set(fid, k):
            assert len(x) == k == len(v) and all(pre_lazy_operand(F, a, b) for a, b in zip(x, v))
            assert m_lazy_dot(F, x, v) == acc.replay(x, [F.value(b) for b in v], 6, 60)
    assert any(all(l == F.M for l in b[:-1]) for _, v in lazy_dot_set(fid, 60) for b in v)


@pytest.mark.parametrize("fid", FIDS)
def test_conversion_and_normalize_sets(fid):
    F = fld(fid)
    S = packed_any_set(fid)
    assert F.R - 1 in S and all(pre_to_packed(F, m_from_packed(F, v)) and F.value(m_from_packed(F, v)) == v for v in S)
    for s in {32 * i for i in range(1, F.NL)} | {F.W * k for k in range(1, F.N)}:
        assert 1 << s in S and 1 << (s - 1) in S
    N = normalize_set(fid)
    assert all(pre_normalize(F, l) for l in N) and len(N) > 200
    out = [m_normalize(F, l) for l in N]
    assert all(F.normalised(o) and F.value(o) == F.value(l) for o, l in zip(out, N))
    assert any(min(l) < -(1 << 30) for l in N) and any(max(l) > 1 << 30 for l in N) and any(o[-1] < 0 for o in out)


@pytest.mark.parametrize("fid", FIDS)
def test_clamp_qa_set(fid):
    F = fld(fid)
    S = clamp_qa_set(fid)
    assert all(pre_clamp_qa(F, l) for l in S)
    lo, hi = clamp_qa_range(F)
    qs = set()
    for l in S:
        out, i = m_clamp_qa(F, l)
        assert 0 <= i < 64 and F.normalised(out) and lo <= F.value(out) < hi and (F.value(out) - F.value(l)) % F.p == 0, (l, i)
        qs.add(i)
    allowed = clamp_q_allowed(F, F.value([clamp_low_max(F)] * (F.N - 1) + [0]))
    assert qs == allowed and len(allowed) >= 32 and all(abs(i - QOFF) <= 18 for i in allowed)
    assert any(max(l[:-1]) == clamp_low_max(F) for l in S)
    # both sides of every step of the estimate
    tops = {l[-1] for l in S}
    for i in sorted(allowed)[1:]:                      # (the lowest index starts at the end of the range, not at a step)
        t = QBIAS + (i - QOFF) * F.PTOP1
        assert t in tops and t - 1 in tops and m_clamp_q(F, t) == i and m_clamp_q(F, t - 1) == i - 1
    # the tables: entry i is (i - QOFF) p, the negated form cancels it word by word
    T, NT = clamp_table(F), clamp_table_negated(F)
    assert T.shape == (64, F.STRIDE) and ((T.astype(np.uint64) + NT) % (1 << 32) == 0).all()
    for i in (0, QOFF - 1, QOFF, QOFF + 1, 63):
        l = [int(x) for x in T[i, :F.N]]
        l[-1] -= (l[-1] >> 31) << 32
        assert F.value(l) == (i - QOFF) * F.p and F.normalised(l)


def test_clamp9_set():
    F = fld(3)
    S = clamp9_set()
    assert all(pre_clamp9(F, l) for l in S)
    qs = set()
    for l in S:
        out = m_clamp9(F, l)
        assert F.normalised(out) and 0 <= F.value(out) < F.p + (1 << 239) and (F.value(out) - F.value(l)) % F.p == 0
        assert pre_to_packed(F, out) and pre_reduce_once(F, F.value(out))          # what to_packed_reduced does next
        qs.add(m_clamp_q(F, l[-1]))
    assert qs == clamp_q_allowed(F, F.B - 1) and len(qs) >= 32
    tops = {l[-1] for l in S}
    for i in sorted(qs)[1:]:
        t = QBIAS + (i - QOFF) * F.PTOP1
        assert t in tops and t - 1 in tops


@pytest.mark.parametrize("fid", FIDS)
def test_mul_sets(fid):
    F = fld(fid)
    A = mul_a_set(fid)
    big = (1 << (F.W + 1)) - 1
    assert len(A) > 100 and any(max(a[:-1]) == big for a in A) and any(min(a[:-1]) == -big for a in A)
    assert any(abs(F.value(a)) == 16 * F.p - 1 for a in A)
    S = mul_set(fid)
    assert len(S) < 60000 and all(pre_mul(F, a, w) for a, w in S)
    assert all(pre_mul(F, a, F.limbs(F.p - 1)) for a in A)
    lo, hi = mul_range(F)
    assert -2 * F.p < lo < -F.p and 0 < hi < F.p // 4
    if fid == 3:
        assert lo > -1.2 * F.p and hi < 0.2 * F.p                                  # field_ln.h: (-1.2p, 0.2p]


@pytest.mark.parametrize("fid", LIMB_DOT_FIDS)
def test_mul_u_sets(fid):
    F = fld(fid)
    A = mul_u_a_set(fid)
    assert all(pre_mul_u(F, a) for a in A) and len(A) <= 256 and len(A) % 64 != 0
    assert any(not F.normalised(a) or min(a[:-1]) < 0 for a in A) and any(max(abs(x) for x in a[:-1]) == F.M for a in A)
    lo, hi = mul_u_range(F)
    assert -2.5 * F.p <= lo < -F.p and F.p < hi <= 1.6 * F.p
    name = FIELD_NAME[fid]
    for w in mul_u_ws(fid):
        tab = shifted_multiples(F, w)
        assert tab == G.shifted_multiples(name, w)
        for j in range(F.N):
            l = [tab[F.N * k + j] for k in range(F.N)]
            l[-1] -= (l[-1] >> 31) << 32
            assert (F.value(l) - (w << (F.W * j))) % F.p == 0 and abs(F.value(l)) <= (F.p - 1) // 2
    # the generator's own instruction list, run as Python integers, keeps the contract on this set
    ins = G.build(name)
    for w in mul_u_ws(fid)[:4]:
        tab = shifted_multiples(F, w)
        for a in A[::5]:
            r = G.simulate(name, a, tab, ins)
            assert F.normalised(r) and (F.value(r) - F.value(a) * w) % F.p == 0 and lo <= F.value(r) < hi


def test_r29_set():
    F = fld(3)
    assert all(0 <= a < F.p and pre_lazy_operand(F, a, b) for a, b in r29_set())
    a, b = r29_set()[12345]
    assert F.value(b) * a * F.Rlinv % F.p == m_lazy_dot(F, [a], [b])
    assert F.Rl == 1 << 261 and m_canon(F, 32 * 5 % F.p) == 32 * 5 * pow(1 << 256, -1, F.p) % F.p

"""ln::clamp_q / clamp_row / clamp_apply (lcpc_amd/csrc/field_ln.h) on the inputs K1s hands them un-normalised, as Python integers
with the 32-bit wrap-around the device code has.  CPU only.

The rounds of ntt_l9s.hip that store from the registers (the pure first pass's I-only round, the final rounds of both last passes)
clamp each output of their butterfly once, straight from its sums: nothing carry-propagates in front of the clamp, whose own carry
pass is signed.  The clamp's header comment names two input classes for Ft255 (9 limbs of 29 bits, B = 2^232):
  (a) sums of four normalised values: limbs 0-7 in [0, 2^31 - 4], |value| < 16p;
  (b) limbs 0-7 signed, in (-2^30, 2^30), |value| < 16p (12.04p in the pure pass's I-only round, 9.04p in the coset pass's last).
Checked for every input: the table index lies in [0, 64) and is floor((t - QBIAS) / (PTOP + 1)) + QOFF; every intermediate d of the
carry pass fits an int32; limbs 0-7 of the result lie in [0, 2^29) and the top limb is >= 0; 0 <= result < p + 64 B < 2^256 (what
to_packed takes); result == input (mod p).

QOFF, QBIAS and the limb layout are read out of field_ln.h, and the model takes QBIAS as a parameter: the lower bound is
V - q p >= (QBIAS - |q| - 2.01) B, and test_a_lowered_qbias_breaks_the_lower_bound shows that the class (b) extremes used here give
a NEGATIVE result once QBIAS is lowered past what they need -- so lowering the constant in the header to where the bound breaks fails
test_clamp_takes_both_classes on these same inputs."""
import os
import random
import re

import pytest

from common import field_p

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
M32 = (1 << 32) - 1
FID = 3


def _header():
    t = open(os.path.join(ROOT, "lcpc_amd", "csrc", "field_ln.h")).read()
    m = re.search(r"struct LnField<FT255> \{\s*static constexpr int FID = FT255, N = (\d+), W = (\d+), NL = (\d+), WAVES = \d+, STRIDE = (\d+);", t)
    N, W, NL, STRIDE = (int(v) for v in m.groups())
    qoff = int(re.search(r"constexpr int QOFF = (\d+);", t).group(1))
    qbias = int(re.search(r"constexpr int QBIAS = (\d+);", t).group(1))
    # the code the model restates: the biased index, the magic division, the signed carry pass
    assert "const u32 n = top + (u32)(QOFF * PTOP1 - QBIAS);" in t and "return __umulhi(n, MAGIC) >> SH;" in t
    assert "const int32_t d = (int32_t)(a.v[k] + nt.v[k] + (u32)c);" in t and "c = d >> FT::W;" in t
    return N, W, NL, STRIDE, qoff, qbias


N, W, NL, STRIDE, QOFF, QBIAS = _header()
P = field_p(FID)
M = (1 << W) - 1
B = 1 << (W * (N - 1))
PTOP1 = (P >> (W * (N - 1))) + 1
SH = PTOP1.bit_length() - 1
MAGIC = ((1 << (32 + SH)) + PTOP1 - 1) // PTOP1


def s32(x):
    x &= M32
    return x - (1 << 32) if x >> 31 else x


def value(limbs):
    return sum(v << (W * k) for k, v in enumerate(limbs))


def norm_limbs(v):
    """invariant I's layout: limbs 0..N-2 in [0, 2^W), the top limb signed"""
    return [(v >> (W * k)) & M for k in range(N - 1)] + [v >> (W * (N - 1))]


# ctx.cpp clamp_table: (i - QOFF) p as normalised signed limbs; the kernel negates every word when it copies the table to LDS
NQP = [[(-l) & M32 for l in norm_limbs((i - QOFF) * P)] for i in range(64)]


def clamp(limbs, qbias=QBIAS):
    """(result limbs, table index, the carry pass's d values) of clamp_apply(a, clamp_row(nqp, clamp_q(top))) on signed Python ints"""
    assert all(-(1 << 31) <= v < 1 << 31 for v in limbs)
    a = [v & M32 for v in limbs]
    n = (a[N - 1] + QOFF * PTOP1 - qbias) & M32
    q = ((n * MAGIC) >> 32) >> SH
    if not 0 <= q < 64:
        return None, q, []
    nt = NQP[q]
    c, ds, out = 0, [], []
    for k in range(N - 1):
        exact = s32(a[k]) + s32(nt[k]) + c
        ds.append(exact)
        d = s32(a[k] + nt[k] + (c & M32))
        out.append(d & M)
        c = d >> W
    out.append(s32(a[N - 1] + nt[N - 1] + (c & M32)))
    return out, q, ds


def check(limbs, qbias=QBIAS):
    """None if the clamp keeps every promise on this input, else the first one it breaks"""
    v = value(limbs)
    out, q, ds = clamp(limbs, qbias)
    if out is None:
        return "index %d" % q
    if q != (limbs[N - 1] - qbias) // PTOP1 + QOFF:
        return "quotient"
    if not all(-(1 << 31) <= d < 1 << 31 for d in ds):
        return "d leaves int32"
    if not all(0 <= x <= M for x in out[:N - 1]):
        return "low limbs"
    if out[N - 1] < 0:
        return "negative"
    r = value(out)
    if not 0 <= r < P + 64 * B:
        return "range"
    if (r - v) % P:
        return "value"
    return None


def with_value(low, v):
    """low limbs as given, the top limb the smallest (v >= 0) or largest (v < 0) that puts the value at or just inside v"""
    lo = value(low)
    t = (v - lo) // B if v >= 0 else -((-v + lo) // B)
    return low + [t]


T30 = (1 << 30) - 1
BOUNDS = (1204, 904, 1600)            # |value| bounds in hundredths of p: the pure pass's I-only round, the coset pass's last round, the clamp's own


def bound(f):
    return abs(f) * P // 100


def class_a(rng, n_random):
    """sums of four normalised values: limbs 0-7 in [0, 4 (2^29 - 1)] = [0, 2^31 - 4], the top limb whatever |value| < 16p leaves"""
    top = 4 * M
    out = []
    for low in ([top] * 8, [0] * 8, [top, 0] * 4, [0, top] * 4):
        for f in (-1600, -1204, -904, 0, 904, 1204, 1600):
            v = bound(f) - 1 if f else 0
            out.append(with_value(low, v if f >= 0 else -v))
    for _ in range(n_random):
        xs = [rng.randrange(-4 * P + 1, 4 * P) for _ in range(4)]
        out.append([sum(c) for c in zip(*(norm_limbs(x) for x in xs))])
        out.append(with_value([rng.choice([0, top, rng.randrange(top + 1)]) for _ in range(8)], rng.randrange(-16 * P + 1, 16 * P)))
    return out


def class_b(rng, n_random):
    """limbs 0-7 at +-(2^30 - 1) in all 512 sign patterns of limbs 0-8 (the sign of limb 8 is the sign of the value), the top limb
    set so that |value| lies just inside each bound; then random members"""
    out = []
    for s in range(1 << N):
        low = [T30 if (s >> k) & 1 else -T30 for k in range(N - 1)]
        for f in BOUNDS:
            v = bound(f) - 1
            out.append(with_value(low, v if (s >> (N - 1)) & 1 else -v))
    for _ in range(n_random):
        low = [rng.choice([-T30, T30, 0, rng.randrange(-T30, T30 + 1)]) for _ in range(N - 1)]
        out.append(with_value(low, rng.randrange(-16 * P + 1, 16 * P)))
    return out


def residues(lows):
    """the inputs at which the quotient estimate is loosest: top limbs t = q (PTOP + 1) + r for every q the range allows and every small
    r on both sides of 0, so that whatever QBIAS < 64 the header holds, rem = (t - QBIAS) mod (PTOP + 1) takes 0 (the lower bound's
    case) and PTOP (the upper bound's) for every q; over the extreme low limbs of the class; |value| < 16p"""
    out = [low + [q * PTOP1 + r] for low in lows for q in range(-17, 18) for r in range(-64, 64)]
    return [x for x in out if _inside(x)]


RES_A = ([0] * (N - 1), [4 * M] * (N - 1))
RES_B = ([-T30] * (N - 1), [T30] * (N - 1))


def _inside(limbs):
    return abs(value(limbs)) < 16 * P


def test_header_constants():
    assert (N, W, NL, STRIDE) == (9, 29, 8, 12) and P % (1 << W) == 1
    assert 64 * PTOP1 * PTOP1 < 1 << (32 + SH) and MAGIC < 1 << 32            # clamp_q's static_assert
    assert P + 64 * B < 1 << (32 * NL)
    assert all(0 <= s32(-w) <= M for row in NQP for w in row[:N - 1])          # the negated rows' low limbs: (-2^W, 0]


@pytest.mark.parametrize("cls", ["a", "b"])
def test_clamp_takes_both_classes(cls):
    rng = random.Random(11 if cls == "a" else 12)
    xs = class_a(rng, 2000) + residues(RES_A) if cls == "a" else class_b(rng, 4000) + residues(RES_B)
    assert len(xs) >= 4000 and all(_inside(x) for x in xs)
    if cls == "a":
        assert all(0 <= v <= (1 << 31) - 4 for x in xs for v in x[:N - 1])
        assert max(max(x[:N - 1]) for x in xs) == (1 << 31) - 4
    else:
        assert all(abs(v) <= T30 for x in xs for v in x[:N - 1])
        # the boundary values: within one B of 12.04p, 9.04p and 16p on both sides
        for f in BOUNDS:
            assert any(0 < bound(f) - value(x) <= B for x in xs) and any(0 < bound(f) + value(x) <= B for x in xs)
    bad = [(x, check(x)) for x in xs if check(x) is not None]
    assert not bad, bad[:3]


def test_a_lowered_qbias_breaks_the_lower_bound():
    """the inputs above reach the bound QBIAS stands for.  Every promise holds at the header's QBIAS; `need`, the smallest QBIAS at
    which the residue inputs of class (b) all pass, is well above 0, and one below it the all-negative low limbs come out NEGATIVE
    (V - q p = q (B - plow) + (rem + QBIAS) B + low with rem = 0, low = -2 B, q = -15: the header's bound (QBIAS - |q| - 2.01) B is
    this with B - plow rounded up to B).  So a header whose QBIAS is lowered to where the lower bound breaks fails
    test_clamp_takes_both_classes, which runs the same inputs at the header's value."""
    xs = residues(RES_B)
    assert all(check(x) is None for x in xs)
    neg = [x for x in xs if x[0] < 0 and x[N - 1] < -12 * PTOP1]               # (the lower bound's end of the range)
    need = min(b for b in range(QBIAS + 1) if all(check(x, qbias=b) is None for x in neg))
    assert 0 < need <= QBIAS and all(check(x, qbias=need) is None for x in xs)
    assert need == 2 + -(-15 * (B - P % B) // B)                              # 2.0 B of low limbs and 15 (B - plow), rounded up
    assert {check(x, qbias=need - 1) for x in xs} == {None, "negative"}

"""The two-table Montgomery multiply of lcpc_amd/csrc/gen/gen_r29_asm.py (r29_mul2s, ln::mul2<LnField<FT255>>: the lane-varying
twiddle multiply of K1s's split plans) on Python integers: the generator's own instruction list runs in the interpreter of
tests/wmul_sim.py (32 / 64-bit wrap-around) beside an exact model of the same columns on unbounded integers.

  x = XL + 2^145 XH (limbs 0-4 | 5-8), a = w 2^145 mod p, b = w 2^290 mod p, Z = XL a + XH b, r = (Z - M p) / 2^145 with the
  five digits M = sum m_k 2^(29 k) in [0, 2^145), so r lies in (Z / 2^145 - p, Z / 2^145] and r == x w (mod p).

Proved output intervals (a, b in [0, p); 2^29 - 1 > 2^29 (1 - 2^-28)):
  * signed limbs |x_k| < 2^30: |XL| < 2^146 (1 + 2^-28), |XH| < 2^117 (1 + 2^-28), so |Z| / 2^145 < (2 + 2^-28)(1 + 2^-28) p
    and r in (-3.01p, 2.01p);
  * a difference of two normalised values (limbs 0-7 in (-2^29, 2^29), |value| < 8p): |XL| < 2^145, |XH| < 8p / 2^145 + 1 < 2^113,
    so |Z| / 2^145 < (1 + 2^-32) p and r in (-2.01p, 1.01p);
  * a normalised value (limbs 0-7 in [0, 2^29), |value| < 4p): XL >= 0 as well, r in (-1.01p, 1.01p).
Accumulator: a column holds at most 9 products below 2^59, 5 reduction products below 2^58 and a carry below 2^35: inside i64."""
import importlib.util
import os
import random
from fractions import Fraction as Fr

from wmul_sim import simulate

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_spec = importlib.util.spec_from_file_location("gen_r29_asm", os.path.join(ROOT, "lcpc_amd", "csrc", "gen", "gen_r29_asm.py"))
gen = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(gen)

P = gen.FT255_P
N, W, ND = 9, 29, 5
M = (1 << W) - 1
INS = gen.mul2()


def limbs_of(v):
    """v in [0, p) -> 9 unsigned limbs"""
    return [(v >> (W * k)) & M for k in range(N)]


def value_of(l):
    return sum(int(v) << (W * k) for k, v in enumerate(l))


def run_sim(x, a, b):
    pre = ["v_mov_b32 %%[a%d], 0x%x" % (j, v) for j, v in enumerate(a)] + ["v_mov_b32 %%[r%d], 0x%x" % (j, v) for j, v in enumerate(b)]
    return simulate("ft255", x, [], ins=pre + INS)


def run_exact(x, a, b):
    """the same columns on unbounded integers -> (limbs, largest |accumulator| met)"""
    npj = [-((P >> (W * j)) & M) for j in range(N)]
    acc, worst, m, r = 0, 0, [], []
    for k in range(N + ND - 1):
        acc += sum(x[i] * a[k - i] for i in range(ND) if 0 <= k - i < N)
        acc += sum(x[ND + i] * b[k - i] for i in range(N - ND) if 0 <= k - i < N)
        acc += sum(m[i] * npj[k - i] for i in range(min(k, ND)) if 1 <= k - i < N)
        worst = max(worst, abs(acc))
        (m if k < ND else r).append(acc & M)
        acc >>= W
    r.append(acc)
    return r, worst


def cases():
    rng = random.Random(0x29145)
    T = (1 << 30) - 1
    ws = [P - 1, 0, 1, 2, (P - 1) // 2, P - 2] + [rng.randrange(P) for _ in range(6)]
    out = []
    # every limb at its extreme: all 2^9 sign patterns of |x_k| = 2^30 - 1, against the largest twiddle and a few more
    for s in range(1 << N):
        x = [T if (s >> k) & 1 else -T for k in range(N)]
        out.append(("signed", x, ws[s % len(ws)] if s & 3 else P - 1))
    # one limb at an extreme, the others zero / random
    for k in range(N):
        for e in (T, -T):
            out.append(("signed", [e if i == k else 0 for i in range(N)], P - 1))
            out.append(("signed", [e if i == k else rng.randrange(-T, T + 1) for i in range(N)], rng.randrange(P)))
    for _ in range(700):
        out.append(("signed", [rng.randrange(-T, T + 1) for _ in range(N)], rng.choice(ws) if rng.random() < 0.3 else rng.randrange(P)))
    # differences of two normalised values, |value| < 8p
    for _ in range(300):
        v = rng.choice([-1, 1]) * rng.randrange(8 * P)
        low = [rng.choice([-M, M, 0]) if rng.random() < 0.3 else rng.randrange(-M, M + 1) for _ in range(N - 1)]
        top = (v - value_of(low)) >> (W * (N - 1))
        out.append(("diff", low + [top], rng.choice(ws) if rng.random() < 0.3 else rng.randrange(P)))
    # normalised values, |value| < 4p (the extremes among them)
    for v in [0, 1, P - 1, P, 4 * P - 1, -(4 * P - 1), -1, -P] + [rng.randrange(-4 * P + 1, 4 * P) for _ in range(300)]:
        low = [(v >> (W * k)) & M for k in range(N - 1)]
        out.append(("norm", low + [v >> (W * (N - 1))], rng.choice(ws) if rng.random() < 0.3 else rng.randrange(P)))
    return out


BOUNDS = {"signed": (Fr(-301, 100), Fr(201, 100)), "diff": (Fr(-201, 100), Fr(101, 100)), "norm": (Fr(-101, 100), Fr(101, 100))}


def test_instruction_counts():
    mads = [t for t in INS if t.startswith("v_mad_i64_i32")]
    assert len(mads) == 121
    assert len(INS) - 8 == 148            # (the eight s_mov of the negated modulus limbs aside)


def test_mul2_residue_range_and_accumulator():
    cs = cases()
    assert len(cs) >= 1500
    worst_acc = 0
    for kind, x, w in cs:
        a, b = limbs_of((w << 145) % P), limbs_of((w << 290) % P)
        got = run_sim(x, a, b)
        want, worst = run_exact(x, a, b)
        worst_acc = max(worst_acc, worst)
        assert worst < 1 << 63, (kind, x, w)
        assert got == want, (kind, x, w)
        assert all(0 <= v <= M for v in got[:8]) and -(1 << 31) <= got[8] < (1 << 31)
        r = value_of(got)
        assert (r - value_of(x) * w) % P == 0, (kind, x, w)
        lo, hi = BOUNDS[kind]
        assert lo * P < r < hi * P, (kind, x, w, Fr(r, P))
    print("largest accumulator: 2^%.2f" % (worst_acc.bit_length() - 1 + 0.0))


def test_pack_constants():
    """the constants the generator emits into the header (R29_MUL2_KA / _KB, read back from its output): a table entry e = w c 2^261
    becomes a = e KA 2^-261 = w c 2^145 and b = e KB 2^-261 = w c 2^290 by ln::mul"""
    import re
    import subprocess
    import sys
    hdr = subprocess.run([sys.executable, os.path.join(ROOT, "lcpc_amd", "csrc", "gen", "gen_r29_asm.py")], capture_output=True, text=True,
                         check=True).stdout
    k = {}
    for nm in ("R29_MUL2_KA", "R29_MUL2_KB"):
        m = re.search(r"constexpr u32 %s\[9\] = \{([^}]*)\};" % nm, hdr)
        assert m, nm
        limbs = [int(t.strip().rstrip("u"), 16) for t in m.group(1).split(",")]
        assert len(limbs) == N and all(0 <= v <= M for v in limbs)
        k[nm] = value_of(limbs)
        assert k[nm] < P
    inv = pow(2, -261, P)
    for w in (1, 0x1234567, P - 1):
        for c in (1, pow(2, 5 - 261, P)):
            e = (w * c << 261) % P
            assert (e * k["R29_MUL2_KA"] * inv) % P == (w * c << 145) % P and (e * k["R29_MUL2_KB"] * inv) % P == (w * c << 290) % P

"""The short tails of the two Ft255 multiplier statements the K1s kernels run (lcpc_amd/csrc/ntt_l9s.hip), on Python integers:

  * gen_wmul_asm.build("ft255", short_tail=True) (wmul_us, ln::mul_us): the top limb is A.lo + C.lo + lo(Q * np2_top) by v_mul_lo_u32 and
    v_add3_u32 instead of the 64-bit add of column C, the mad and the closing move;
  * gen_r29_asm.mul2(short_tail=True) (r29_mul2s, ln::mul2): the top limb is bits 29 .. 60 of the accumulator by one v_alignbit_b32 instead
    of the last 64-bit shift and the closing move.

Both must return, limb for limb, what the long lists return -- those are the lists tests/test_gen_wmul.py and tests/test_gen_r29_mul2.py
hold to their residues and ranges in the interpreter of tests/wmul_sim.py, which does not know the three new instructions; the
interpreter below is that one plus them (32 / 64-bit wrap-around).  The same inputs as those tests: their extremes and sweeps."""
import random
import re

import test_gen_r29_mul2 as T2
import wmul_sim as G
from test_gen_wmul import _limbs

M32, M64 = (1 << 32) - 1, (1 << 64) - 1
s32 = lambda v: ((v + (1 << 31)) & M32) - (1 << 31)
s64 = lambda v: ((v + (1 << 63)) & M64) - (1 << 63)


def run(ins, named, wtab=()):
    """named: the %[..] operands (u32 values), updated in place; wtab: what s_load_dword reads"""
    vg, sg, vcc = {}, {}, 0

    def rd(op):
        if op.startswith("%["):
            return named[op[2:-1]]
        if op.startswith("v["):
            lo = int(op[2:op.index(":")])
            return vg.get(lo, 0) | (vg.get(lo + 1, 0) << 32)
        if op.startswith("v"):
            return vg.get(int(op[1:]), 0)
        if op.startswith("s"):
            return sg[int(op[1:])]
        return int(op, 0) & M32

    def wr(op, val, wide=False):
        if op.startswith("%["):
            named[op[2:-1]] = val & M32
        elif wide:
            lo = int(op[2:op.index(":")])
            vg[lo], vg[lo + 1] = val & M32, (val >> 32) & M32
        else:
            vg[int(op[1:])] = val & M32

    for line in ins:
        mn, rest = line.split(" ", 1)
        ops = [o.strip() for o in re.split(r",\s*(?![^\[]*\])", rest)]
        if mn.startswith("s_load_dword"):
            n = 1 if mn == "s_load_dword" else int(mn[len("s_load_dwordx"):])
            base = int(ops[0][1:]) if n == 1 else int(ops[0][2:ops[0].index(":")])
            for i in range(n):
                sg[base + i] = wtab[int(ops[2], 0) // 4 + i] if int(ops[2], 0) // 4 + i < len(wtab) else 0
        elif mn == "s_mov_b32":
            sg[int(ops[0][1:])] = int(ops[1], 0) & M32
        elif mn == "s_waitcnt":
            pass
        elif mn == "v_mad_i64_i32":
            wr(ops[0], (s32(rd(ops[2])) * s32(rd(ops[3])) + (0 if ops[4] == "0" else s64(rd(ops[4])))) & M64, True)
        elif mn == "v_ashrrev_i64":
            wr(ops[0], (s64(rd(ops[2])) >> int(ops[1])) & M64, True)
        elif mn == "v_add_co_u32":
            t = rd(ops[2]) + rd(ops[3])
            vcc = t >> 32
            wr(ops[0], t)
        elif mn == "v_addc_co_u32":
            t = rd(ops[2]) + rd(ops[3]) + vcc
            vcc = t >> 32
            wr(ops[0], t)
        elif mn == "v_and_b32":
            wr(ops[0], rd(ops[1]) & rd(ops[2]))
        elif mn == "v_add_u32":
            wr(ops[0], rd(ops[1]) + rd(ops[2]))
        elif mn == "v_mov_b32":
            wr(ops[0], rd(ops[1]))
        elif mn == "v_mul_lo_u32":
            wr(ops[0], rd(ops[1]) * rd(ops[2]))
        elif mn == "v_add3_u32":
            wr(ops[0], rd(ops[1]) + rd(ops[2]) + rd(ops[3]))
        elif mn == "v_alignbit_b32":                     # D = ({S0, S1} >> S2[4:0]) & 0xffffffff
            wr(ops[0], ((rd(ops[1]) << 32) | rd(ops[2])) >> (rd(ops[3]) & 31))
        else:
            raise ValueError(line)
    return named


def wmul_run(ins, x, tab):
    P, N, W, VB, s1, s2, MU = G.params("ft255")
    named = {"x%d" % j: x[j] & M32 for j in range(N)}
    for k in range(N):
        named["n%d" % k] = (-(((2 * P) >> (W * k)) & (((1 << W) - 1) if k < N - 1 else M32))) & M32
    run(ins, named, tab)
    return [named["r%d" % k] if k < N - 1 else s32(named["r%d" % k]) for k in range(N)]


def test_the_interpreter_is_wmul_sims_on_the_long_lists():
    P, N, W = G.params("ft255")[:3]
    rng = random.Random(5)
    long_list = G.build("ft255")
    for _ in range(50):
        x, tab = _limbs(rng.randrange(-4 * P, 4 * P), N, W), G.shifted_multiples("ft255", rng.randrange(1, P))
        assert wmul_run(long_list, x, tab) == G.simulate("ft255", x, tab, long_list)


def test_wmul_short_tail_is_the_long_one():
    """the inputs of tests/test_gen_wmul.py test_wmul_simulated (its five modes), both lists, equal limbs and the residue"""
    P, N, W = G.params("ft255")[:3]
    long_list, short_list = G.build("ft255"), G.build("ft255", short_tail=True)
    assert len(short_list) == len(long_list) - 2
    assert short_list[:-2] == long_list[:-4] and [t.split()[0] for t in short_list[-2:]] == ["v_mul_lo_u32", "v_add3_u32"]
    assert sum(t.startswith("v_add_co_u32") for t in short_list) == 2 and sum(t.startswith("v_mov_b32") for t in short_list) == 0
    rng = random.Random(0xC0FFEE + N)
    ptop, top = P >> (W * (N - 1)), (1 << W) - 1
    for it in range(1500):
        w = rng.randrange(1, P) if it % 7 else rng.choice([1, P - 1, (P - 1) // 2, (P + 1) // 2, 2, P - 2])
        tab = G.shifted_multiples("ft255", w)
        mode = it % 5
        if mode == 0:
            x = _limbs(rng.randrange(-4 * P, 4 * P), N, W)
        elif mode == 1:
            x = [a - b for a, b in zip(_limbs(rng.randrange(-4 * P, 4 * P), N, W), _limbs(rng.randrange(-4 * P, 4 * P), N, W))]
        elif mode == 2:
            sg = rng.choice([1, -1])
            x = [sg * top] * (N - 1) + [sg * rng.randrange(0, 8 * ptop)]
        elif mode == 3:
            x = [rng.choice([-1, 1]) * rng.randrange(0, 1 << W) for _ in range(N - 1)] + [rng.randrange(-8 * ptop, 8 * ptop)]
        else:
            x = [rng.choice([-top, top, 0]) for _ in range(N - 1)] + [rng.choice([-1, 1]) * 8 * ptop]
        r = wmul_run(short_list, x, tab)
        assert r == wmul_run(long_list, x, tab), (x, w)
        assert (sum(l << (W * k) for k, l in enumerate(r)) - sum(l << (W * k) for k, l in enumerate(x)) * w) % P == 0


def test_mul2_short_tail_is_the_long_one():
    """every case of tests/test_gen_r29_mul2.py (all 512 sign patterns of the extreme limbs among them)"""
    long_list, short_list = T2.gen.mul2(), T2.gen.mul2(short_tail=True)
    assert len(short_list) == len(long_list) - 1 and short_list[:-1] == long_list[:-2]
    assert short_list[-1].startswith("v_alignbit_b32 %[r8], v127, v126, 29")
    assert sum(t.startswith("v_mad_i64_i32") for t in short_list) == 121 and len(short_list) - 8 == 147
    cs = T2.cases()
    assert len(cs) >= 1500
    for kind, x, w in cs:
        a, b = T2.limbs_of((w << 145) % T2.P), T2.limbs_of((w << 290) % T2.P)
        want, _ = T2.run_exact(x, a, b)
        for ins in (short_list, long_list):
            named = {"x%d" % j: x[j] & M32 for j in range(9)}
            named.update({"a%d" % j: a[j] for j in range(9)})
            named.update({"r%d" % j: b[j] for j in range(9)})
            run(ins, named)
            got = [named["r%d" % k] if k < 8 else s32(named["r8"]) for k in range(9)]
            assert got == want, (kind, x, w)

"""The checkers of tests/k1_tables.py bite: on tables built from the models they find nothing, and each representation fault a table
builder could leave -- the right residue in the wrong form, which no end-to-end comparison notices -- is reported by the checker meant
to catch it.  CPU only; tests/test_gpu_k1_tables.py runs the same checkers on the product's tables."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [HERE, os.path.join(os.path.dirname(HERE), "oracle")]
import common as CM  # noqa: E402
import k1_tables as T  # noqa: E402
import ntt_coset_rules as NR  # noqa: E402
from test_fe_cases import clamp_table, fld  # noqa: E402

LOG_N = 6                                    # the twiddle tables of the fault tests: 32 entries


def _tables(fid):
    F = fld(fid)
    w = CM.ntt_root(fid, LOG_N)
    n = 1 << (LOG_N - 1)
    return F, w, T.model_roots(F, w, n), T.model_limb_table(F, w, n, False), T.model_limb_table(F, w, n, True)


COSET = T.PassDesc("K1s", False, 12, 2, 10, form=1)
COSET_SPLIT = T.PassDesc("K1s", False, 12, 2, 10, form=1, mul2=1)
PURE = T.PassDesc("K1s", True, 16, 0, 6, form=1)
PURE_SPLIT = T.PassDesc("K1s", True, 13, 0, 3, form=1, mul2=1)
DIF_FIRST = T.PassDesc("K1n", True, 18, 0, 8)                # Ft127: LBT = 2, one uniform round
DIF_LAST = T.PassDesc("K1n", False, 18, 8, 10)
PACKS = [(3, COSET, [0, 3]), (3, COSET_SPLIT, [1]), (3, PURE, [0]), (3, PURE_SPLIT, [0]), (1, DIF_FIRST, [0, 201]), (1, DIF_LAST, [0]),
         (0, T.PassDesc("K1n", True, 21, 0, 1), [0, 2047]), (2, T.PassDesc("K1n", True, 19, 0, 9), [5])]


@pytest.mark.parametrize("fid", [0, 1, 2, 3])
def test_model_tables_have_no_findings(fid):
    F, w, roots, rl, rlc = _tables(fid)
    idx = range(len(roots))
    assert T.check_roots(F, w, roots, idx) == []
    assert T.check_limb_table(F, w, rl, idx, False) == [] and T.check_limb_table(F, w, rlc, idx, True, name="d_rootslc") == []
    assert T.check_clamp(F, clamp_table(F)) == [] and T.check_wq(F, T.model_wq(F)) == []
    assert T.check_subtable(rl[::4].copy(), rl, 2) == []
    if fid == 3:
        assert T.scales(F) == ((1 << 261) % F.p, 32)


@pytest.mark.parametrize("fid,d,classes", PACKS)
def test_model_packs_have_no_findings(fid, d, classes):
    F, w = fld(fid), CM.ntt_root(fid, d.log_n)
    recs = T.model_pack_entries(F, d, classes, w)
    assert len(recs) and T.check_pack_entries(F, d, recs, classes, w) == []
    if T.pass_slots(F, d)[1]:
        assert T.check_uniform(F, d, T.model_uniform(F, d, classes, w), classes, w) == []


def test_pass_shapes():
    """record counts of the shapes above, by hand from ntt_ln_dev.h"""
    F3, F1, F0 = fld(3), fld(1), fld(0)
    assert T.pass_slots(F3, COSET) == ([(2, 3, 16), (3, 3, 64), (4, 3, 256)], [(0, 0, 0), (0, 0, 1), (0, 0, 2)] + [(1, m, v) for m in range(4) for v in range(3)])
    assert T.pass_slots(F3, PURE)[0] == [(0, 6, 16), (1, 6, 4), (2, 6, 1)] and len(T.pass_slots(F3, PURE)[1]) == 12
    assert T.pass_slots(F3, PURE_SPLIT) == ([(0, 2, 4), (1, 6, 1)], [])
    assert T.pass_slots(F1, DIF_FIRST) == ([(r, 6, 256 >> (2 * r)) for r in range(4)], [(0, j, v) for j in range(4) for v in range(3)])
    # a last pass: the final round (stages k-2, k-1) is not packed, neither as entries nor as its uniform tables
    assert T.pass_slots(F1, DIF_LAST) == ([(r, 6, 256 >> (2 * r)) for r in range(4)], [(0, j, v) for j in range(4) for v in range(3)])
    assert T.pass_slots(F0, DIF_LAST)[1] == []                                      # Ft63 has no mul_u
    assert len(T.pack_heads(F3, COSET_SPLIT, [0, 1])) == 2 * 2 * 3 * (16 + 64 + 256)
    assert T.classes_of(COSET) == 4 and T.classes_of(PURE) == 1 and T.classes_of(DIF_FIRST) == 256 and T.classes_of(DIF_LAST) == 1


def test_lazy_table_is_the_rules_table():
    p, w = CM.field_p(3), CM.ntt_root(3, 7)
    a, b = NR.Table(w, 7, p), T.LazyTable(w, 7, p)
    assert [a(i) for i in range(128)] == [b(i) for i in range(128)]


def test_sampling():
    assert T.sample_classes(16, 1) == list(range(16))
    s = T.sample_classes(1024, 1)
    assert s[:4] == [0, 1, 1023, 0b0101010101] and len(s) == 16 == len(set(s)) and s == T.sample_classes(1024, 1) != T.sample_classes(1024, 2)
    assert T.sample_indices(8192, 14, 0) == list(range(8192))
    ix = T.sample_indices(1 << 19, 20, 0)
    assert {0, 1, 2, (1 << 18) - 1, 1 << 18, (1 << 19) - 1} <= set(ix) and 4000 < len(ix) <= 4102


# ---- one fault at a time -------------------------------------------------------------------------------------------------------------------
def _one(findings, *words):
    assert findings and all(any(wd in f for f in findings) for wd in words), findings
    return findings


def test_fault_entry_plus_p():
    """the right residue in [p, 2p): where p + entry still fits the limbs / the words"""
    for fid in (0, 1, 2, 3):
        F, w, roots, rl, rlc = _tables(fid)
        i = next(i for i in range(len(rl)) if T.limb_value(F, rl[i, :F.N]) + F.p < F.Rl)
        rl[i, :F.N] = T.to_limbs(F, T.limb_value(F, rl[i, :F.N]) + F.p)
        _one(T.check_limb_table(F, w, rl, [], False), "d_rootsl[%d]: value is not below p" % i)
        _one(T.check_limb_table(F, w, rl, [i], False), "(same residue)")
        v = T.packed_value(roots[3]) + F.p
        roots[3] = [(v >> (32 * k)) & 0xFFFFFFFF for k in range(F.NL)]
        _one(T.check_roots(F, w, roots, []), "d_roots[3]: not below p")
    F, w = fld(3), CM.ntt_root(3, 12)
    recs = T.model_pack_entries(F, COSET, [0, 3], w)
    i = next(i for i in range(len(recs)) if T.limb_value(F, recs[i, 4:]) + F.p < F.Rl)
    recs[i, 4:] = T.to_limbs(F, T.limb_value(F, recs[i, 4:]) + F.p)
    _one(T.check_pack_entries(F, COSET, recs, [0, 3], w, exact=False), "is not in (0, p)")


def test_fault_carry_between_limbs():
    """the same value, un-normalised: 2^W moved from limb k + 1 down into limb k"""
    F, w, _, rl, _ = _tables(1)
    i, k = next((i, k) for i in range(len(rl)) for k in range(F.N - 1) if rl[i, k + 1])
    v = T.limb_value(F, rl[i, :F.N])
    rl[i, k] += 1 << F.W
    rl[i, k + 1] -= 1
    assert T.limb_value(F, rl[i, :F.N]) == v
    _one(T.check_limb_table(F, w, rl, range(len(rl)), False), "d_rootsl[%d]: limb %d" % (i, k), "is not below 2^29")
    F, w = fld(1), CM.ntt_root(1, 18)
    recs = T.model_pack_entries(F, DIF_FIRST, [0, 201], w)
    i = next(i for i in range(len(recs)) if recs[i, 4 + 3])
    recs[i, 4 + 2] += 1 << F.W
    recs[i, 4 + 3] -= 1
    _one(T.check_pack_entries(F, DIF_FIRST, recs, [0, 201], w), "limb 2", "is not below 2^29")


def test_fault_other_representative_of_a_shifted_multiple():
    for fid, d, classes in ((3, COSET, [3]), (3, PURE, [0]), (1, DIF_FIRST, [201])):
        F, w = fld(fid), CM.ntt_root(fid, d.log_n)
        recs = T.model_uniform(F, d, classes, w)
        j, N = 2, F.N
        V = T.signed_value(F, [int(recs[5, 4 + N * k + j]) for k in range(N)])
        other = F.limbs(V + F.p if V < 0 else V - F.p)
        for k in range(N):
            recs[5, 4 + N * k + j] = other[k] & 0xFFFFFFFF
        f = _one(T.check_uniform(F, d, recs, classes, w, exact=False), "W_2", "outside the balanced range")
        assert not any("is not W_0" in x for x in f)                 # (still the right residue)
    F = fld(3)
    wq = T.model_wq(F)
    V = T.signed_value(F, [int(wq[F.N * k + 4]) for k in range(F.N)])
    other = F.limbs(V + F.p if V < 0 else V - F.p)
    for k in range(F.N):
        wq[F.N * k + 4] = other[k] & 0xFFFFFFFF
    _one(T.check_wq(F, wq), "of W_4")


def test_fault_negation_on_the_wrong_half():
    """p - entry applied to the indices below n / 2 instead of those from n / 2 on: every entry is still +- a power of w"""
    F, w = fld(3), CM.ntt_root(3, 12)

    class Wrong(T.LazyTable):
        def __call__(self, ix):
            v = pow(self.w, ix % self.half, self.p)
            return self.p - v if ix < self.half and ix else v

    recs = T.model_pack_entries(F, COSET, [0, 3], w, table=Wrong(w, 12, F.p))
    assert T.check_pack_entries(F, COSET, recs, [0, 3], w, exact=False) == []      # representation and membership cannot see it
    _one(T.check_pack_entries(F, COSET, recs, [0, 3], w), "(the negated value)")


def test_fault_borrow_of_the_negation():
    """a p - entry whose borrow stops one limb early: no longer a power of w at all"""
    F, w = fld(3), CM.ntt_root(3, 12)
    recs = T.model_pack_entries(F, COSET, [3], w)
    i = next(i for i in range(len(recs)) if T.entry_exp(COSET, *recs[i, :4].tolist())[0] >= 1 << 11)
    recs[i, 4 + 4] = (int(recs[i, 4 + 4]) + 1) & F.M
    _one(T.check_pack_entries(F, COSET, recs, [3], w, exact=False), "not a power of w")


def test_fault_pad_words():
    F, w, _, rl, rlc = _tables(3)
    rlc[7, 10] = 1
    _one(T.check_limb_table(F, w, rlc, [], True, name="d_rootslc"), "d_rootslc[7]: pad word 10")
    F1 = fld(1)
    _, _, _, rl1, _ = _tables(1)
    rl1[0, 5] = 0x80000000
    _one(T.check_limb_repr(F1, rl1), "d_rootsl[0]: pad word 5")
    wq = T.model_wq(F)
    wq[95] = 9
    _one(T.check_wq(F, wq), "word 95 (pad)")
    recs = T.model_uniform(F, PURE, [0], CM.ntt_root(3, 16))
    recs[11, 4 + 81] = 1
    _one(T.check_uniform(F, PURE, recs, [0], CM.ntt_root(3, 16)), "position 3 v 2: pad word 81")


def test_fault_b1_swapped_for_b0():
    F = fld(3)
    for d, classes in ((COSET_SPLIT, [1]), (PURE_SPLIT, [0])):
        w = CM.ntt_root(3, d.log_n)
        recs = T.model_pack_entries(F, d, classes, w)
        slot, nv, period = T.pass_slots(F, d)[0][-1]
        h = recs[:, :4]
        i0 = int(np.flatnonzero((h[:, 1] == slot) & (h[:, 2] == 1) & (h[:, 3] == 0))[0])
        i1 = int(np.flatnonzero((h[:, 1] == slot) & (h[:, 2] == nv + 1) & (h[:, 3] == 0))[0])
        recs[[i0, i1], 4:] = recs[[i1, i0], 4:]
        f = _one(T.check_pack_entries(F, d, recs, classes, w), "expected b0 = e 2^-116", "expected b1 = e 2^29")
        assert len([x for x in f if "expected b" in x]) == 2


def test_fault_subtable_at_half_the_shift():
    F, w, _, rl, _ = _tables(3)
    s0 = 2
    assert T.check_subtable(rl[::4].copy(), rl, s0) == []
    _one(T.check_subtable(rl[::2][:len(rl) // 4].copy(), rl, s0), "d_rootsls[1] word 0", "entry 4 of the full table")


def test_fault_clamp_row_with_an_unsigned_top_limb():
    for fid in (0, 1, 2, 3):
        F = fld(fid)
        t = clamp_table(F)
        t[23, F.N - 1] &= F.M                                     # q = -1: the top limb masked like the others, not sign-extended
        _one(T.check_clamp(F, t), "d_qpl[23] (q = -1) word %d" % (F.N - 1))
        t = clamp_table(F)
        t[40, F.STRIDE - 1] = 1
        _one(T.check_clamp(F, t), "d_qpl[40] (q = 16) word %d" % (F.STRIDE - 1))


def test_membership_rejects_a_non_member():
    for fid in (0, 1, 2, 3):
        F = fld(fid)
        w, w2n = CM.ntt_root(fid, 12), CM.ntt_root(fid, 13)       # w2n: a 2n-th root of unity, w2n^2 == w
        assert w2n * w2n % F.p == w
        assert T.is_member(F, w, 12) and T.is_member(F, F.p - w, 12) and T.is_member(F, pow(w, 12345, F.p), 12)
        assert not T.is_member(F, w2n, 12) and not T.is_member(F, 3, 12) and not T.is_member(F, 0, 12)
    F, w = fld(3), CM.ntt_root(3, 12)
    recs = T.model_pack_entries(F, COSET, [0], w)
    recs[100, 4:] = T.to_limbs(F, CM.ntt_root(3, 13) * T.scales(F)[0] % F.p)
    _one(T.check_pack_entries(F, COSET, recs, [0], w, exact=False), "slot 3", "not a power of w")
    urecs = T.model_uniform(F, COSET, [0], w)
    urecs[0, 4:4 + 81] = T.shifted_multiples(F, CM.ntt_root(3, 13))
    _one(T.check_uniform(F, COSET, urecs, [0], w, exact=False), "W_0^n != 1")


def test_records_of_another_shape_are_refused():
    F, w = fld(3), CM.ntt_root(3, 12)
    recs = T.model_pack_entries(F, COSET, [0, 3], w)
    _one(T.check_pack_entries(F, COSET, recs[:-1], [0, 3], w), "not those of the pass shape")
    _one(T.check_pack_entries(F, COSET, recs, [0, 2], w), "not those of the pass shape")


def test_k1_harness_is_a_library_of_its_own():
    """k1h_ only, no name of the product's, NEEDED-linked to the product, whose binary does not know the prefix; built without the
    test hooks, like the product whose context it reads"""
    from test_abi import _harness_is_a_separate_library
    _harness_is_a_separate_library("k1_harness", "k1h_", "tests/native/k1_harness.cpp", "K1H_OUT")
    import subprocess
    make = lambda target: subprocess.check_output(["make", "-n", "-B", "-C", os.path.join(os.path.dirname(HERE), "lcpc_amd", "csrc"), target], text=True)
    assert "../lib/liblcpc_k1_harness.so" in make("clean").split()
    rule, = [l for l in make("all").splitlines() if " -o ../lib/liblcpc_k1_harness.so " in l]
    assert "LCPC_TEST_HOOKS" not in rule and "-llcpc_hip" in rule
    # `all` links it, behind the product, from a clean tree (it is in `all` wherever its source is there)
    out = make("all")
    names = [l.split("-o ../lib/")[1].split()[0] for l in out.splitlines() if "-o ../lib/" in l and "-shared" in l]
    assert "liblcpc_k1_harness.so" in names and names.index("liblcpc_hip.so") < names.index("liblcpc_k1_harness.so")

"""CPU side of the per-pass tests of the Ligero row NTT (tests/k1_pass_model.py, tests/test_gpu_k1_passes.py): the model of one pass is
held to the oracle's whole transform and to Python integers, the representation rule to the plan's own fields, the decoders of the limb
intermediate to their encoders, and the case list of the GPU module to the instantiations it has to reach.  Nothing here needs a GPU."""
import os

import numpy as np
import pytest

import common as CM
import k1_pass_model as M

HERE = os.path.dirname(os.path.abspath(__file__))
PLAN_CASES = M.plan_cases()


def _steps(fid, k, env, general):
    return M.restated_steps(fid, k, general, env.get("LCPC_NTT_FORM"))


@pytest.mark.parametrize("case", PLAN_CASES, ids=[c[0] for c in PLAN_CASES])
def test_models_chained_over_a_plan_are_the_transform(oracle, case):
    """every step's model, one after the other, gives lo_fft_io's bits (Montgomery limbs in, Montgomery limbs out)"""
    O = oracle
    _, fid, k, env, general = case
    rows = 1 if k >= 19 else 2
    L, n = CM.FIELD_L[fid], 1 << k
    x = O.random_elems(fid, rows * n, 7 + k).reshape(rows, n, L)
    want = x.copy()
    for r in range(rows):
        assert O.lib().lo_fft_io(fid, O.ptr(want[r]), k) == 0
    steps = _steps(fid, k, env, general)
    assert M.stages_done(steps, len(steps) - 1) == k
    for st in steps:
        x = M.model_step(O, fid, st, x)
    assert (x == want).all()


SMALL = [c for c in PLAN_CASES if c[2] <= 12]


@pytest.mark.parametrize("case", SMALL, ids=[c[0] for c in SMALL])
def test_models_in_python_integers(oracle, case):
    """up to 2^12 columns each step's model is computed a second time in plain Python integers (common.dif_stage; ntt_coset_rules
    run_pure / run_coset, the two halves of the transform test_ntt_coset_model.py holds to the direct DFT)"""
    O = oracle
    _, fid, k, env, general = case
    L, n, p = CM.FIELD_L[fid], 1 << k, CM.field_p(fid)
    x = O.random_elems(fid, n, 3 * k + fid).reshape(1, n, L)
    for st in _steps(fid, k, env, general):
        y = M.model_step(O, fid, st, x)
        assert M.model_step_ints(fid, st, M.to_ints(x[0])) == M.to_ints(y[0]), st
        x = y
    assert all(v < p for v in M.to_ints(x[0]))


@pytest.mark.parametrize("case", PLAN_CASES, ids=[c[0] for c in PLAN_CASES])
def test_representation_rule_ends_all_canonical_or_all_montgomery(case):
    _, fid, k, env, general = case
    steps = _steps(fid, k, env, general)
    M.check_plan_fields(fid, k, steps)
    # block 0 shrinks by the stages of each pass and is never larger than what the pass before left
    left = 1 << k
    for i in range(len(steps)):
        now = int(M.mont_mask_after(fid, k, steps, i, True).sum())
        assert now in (0, (1 << k) >> M.stages_done(steps, i)) and now <= left
        left = max(now, 0)


def test_rule_on_the_shapes_the_kernels_name():
    """spot values of the rule, read off ntt_l9s.hip / ntt_lns.hip / kernels.hip by hand"""
    def left(fid, k, general=False, form=None):
        st = M.restated_steps(fid, k, general, form)
        return [int(M.mont_mask_after(fid, k, st, i, True).sum()) for i in range(len(st))]
    assert left(3, 14) == [1 << 10, 0]                             # K1s DIF, S = 4: block 0 = one tile
    assert left(3, 18, form="dif") == [0, 0]                       # S = 8: the uniform round's predecessor converts the pure sum
    assert left(3, 14, form="coset") == [0, 0] and left(3, 18) == [0, 0]
    assert left(0, 18) == [1 << 10, 0] and left(1, 18) == [0, 0] and left(1, 17) == [1 << 10, 0]   # Ft63 has no uniform round
    assert left(3, 21) == [1 << 20, 0, 0] and left(0, 22) == [1 << 20, 1 << 10, 0]
    assert left(3, 21, general=True) == [(1 << 21) >> s for s in np.cumsum([s for _, s, _, _ in CM.general_passes(3, 21, True)])[:-1]] + [0]


def test_mid_records_decode_and_encode(oracle):
    rng = np.random.default_rng(5)
    limbs = rng.integers(-(1 << 31), 1 << 31, size=(3, 4096, 9), dtype=np.int64).astype(np.int32)
    words = M.mid_encode(limbs)
    assert words.dtype == np.uint32 and words.size == 3 * 4096 * 9
    assert (M.mid_decode(words, 3, 12) == limbs).all()
    assert (M.mid_encode(M.mid_decode(words, 3, 12)) == words).all()
    # the layout of ntt_l9s.hip: element g of a row at tile g >> 10, position g & 1023; limbs 0-3 | 4-7 | 8
    g, row = 1024 * 2 + 77, 1
    base = (row * 4096 + 2 * 1024) * 9
    assert list(words[base + 77 * 4:base + 77 * 4 + 4].view(np.int32)) == list(limbs[row, g, 0:4])
    assert list(words[base + (1024 + 77) * 4:base + (1024 + 77) * 4 + 4].view(np.int32)) == list(limbs[row, g, 4:8])
    assert words[base + 8 * 1024 + 77].view(np.int32) == limbs[row, g, 8]


def test_mid_values_are_python_integers():
    p = CM.field_p(3)
    rng = np.random.default_rng(6)
    vals = [0, 1, -1, p, -p, 4 * p - 1, -(4 * p - 1), 4 * p, -4 * p, 4 * p + 5, -(4 * p) - 5, 2 * p - 1, 3 * p + 1]
    vals += [int(rng.integers(0, 1 << 62)) * (1 << 190) * (1 if i % 2 else -1) + int(rng.integers(0, 1 << 62)) for i in range(200)]
    limbs = np.array([M.mid_limbs_of(v) for v in vals], np.int64).astype(np.int32)
    assert [M.mid_value_int(l) for l in limbs] == vals
    res, norm, in_range = M.mid_values(limbs, p)
    assert norm.all()
    assert list(in_range) == [abs(v) < 4 * p for v in vals]
    ok = [i for i, v in enumerate(vals) if abs(v) < 4 * p]
    assert [M.to_ints(res[i:i + 1])[0] for i in ok] == [vals[i] % p for i in ok]
    # the pure / coset form's bound: 12.04p, not a multiple of p
    b = M.mid_bound(p, 1)
    assert M.mid_bound(p, 0) == 4 * p and 100 * (b - 1) < 1204 * p <= 100 * b
    vals2 = [b - 1, -(b - 1), b, -b, 12 * p, -12 * p, 13 * p, 16 * p - 1, 4 * p, 0]
    limbs2 = np.array([M.mid_limbs_of(v) for v in vals2], np.int64).astype(np.int32)
    res2, _, in2 = M.mid_values(limbs2, p, b)
    assert list(in2) == [abs(v) < b for v in vals2]
    assert [M.to_ints(res2[i:i + 1])[0] for i in range(len(vals2)) if in2[i]] == [v % p for v in vals2 if abs(v) < b]
    bad = limbs.copy()
    bad[3, 2] = 1 << 29                                            # a low limb outside [0, 2^29)
    bad[5, 7] = -1
    assert list(np.nonzero(~M.mid_values(bad, p)[1])[0]) == [3, 5]


def test_numpy_integers():
    rng = np.random.default_rng(7)
    for fid in range(4):
        p, L = CM.field_p(fid), CM.FIELD_L[fid]
        vals = [0, 1, p - 1, p, p + 1, 2 * p - 1, (1 << (64 * L)) - 1] + [int.from_bytes(rng.bytes(8 * L), "little") for _ in range(100)]
        a = CM.to_limbs(vals, L)
        assert M.to_ints(a) == vals
        assert list(M.ge_const(a, p)) == [v >= p for v in vals]
        small = [v for v in vals if v < 2 * p]
        assert M.to_ints(M.reduce_once(CM.to_limbs(small, L), p)) == [v % p for v in small]
        assert (M.words_to_limbs(M.limbs_to_words(a), L) == a).all()
        b = M.store_bound(fid, "K1s" if fid == 3 else "K1n", False)
        assert p < b < min(2 * p, 1 << (64 * L))


def test_padded_source():
    src = np.arange(1, 23, dtype=np.uint64).reshape(22, 1)
    got = M.padded_source(src, 3, 8, 10, 5, 22, 1)[:, :, 0]
    assert got.tolist() == [[1, 2, 3, 4, 5, 0, 0, 0], [11, 12, 13, 14, 15, 0, 0, 0], [21, 22, 0, 0, 0, 0, 0, 0]]


def test_case_list_reaches_every_instantiation():
    """an assertion on the list: every name of common.ntt_required_instantiations() and the general-kernel instantiations the GPU
    module is there for"""
    reached = M.reached_instantiations()
    assert not CM.ntt_required_instantiations() - reached, sorted(CM.ntt_required_instantiations() - reached)
    assert not M.GENERAL_REQUIRED - reached, sorted(M.GENERAL_REQUIRED - reached)
    ids = [c[0] for c in PLAN_CASES]
    assert len(set(ids)) == len(ids)
    # K1s: ten first-pass shapes, each in the DIF and in the pure / coset form, the latter with both multipliers where the pass has both
    k1s = [(c[2], c[3].get("LCPC_NTT_FORM"), c[3].get("LCPC_NTT_MUL")) for c in PLAN_CASES if c[0].startswith("K1s")]
    for k in range(11, 21):
        forms = {"coset" if M.restated_steps(3, k, False, f)[0].form else "dif" for kk, f, _ in k1s if kk == k}
        assert forms == ({"dif"} if k == 11 else {"dif", "coset"}), (k, forms)
        if k >= 12:
            assert {m for kk, f, m in k1s if kk == k and m} == {"split", "mont"}


def test_saturating_cases_fill_a_device_and_reach_every_instantiation():
    """the case list of tests/test_gpu_k1_saturated.py on a nominal MI355X of 256 CUs: every context up to 2^20 columns and both
    Montgomery-word sizes are there, every launch has 2 x 256 x 8 workgroups with a row count that is odd and no multiple of 3, no
    launch holds 1 GiB, and the launches reach every instantiation those sizes have -- the general kernel in its BS = 256 form"""
    cus = M.SAT_NOMINAL_CUS
    assert M.sat_tiles(cus) == 4096
    cases = M.sat_plan_cases()
    ids = [c[0] for c in cases]
    assert len(set(ids)) == len(ids)
    assert not {c[0] for c in PLAN_CASES if c[2] <= 20} - set(ids)
    assert not [c for c in PLAN_CASES if c[2] > 20 and not c[0].startswith("3pass-") and not c[4]]   # (only three-pass plans stay out)
    for _, fid, k, env, general in cases:
        tpr = M.sat_tiles_per_row(fid, k, general)
        R = M.sat_rows(tpr, cus)
        assert R % 2 == 1 and R % 3 != 0 and R * tpr >= M.sat_tiles(cus), (fid, k, R)
        assert all(r % 2 == 0 or r % 3 == 0 for r in range(-(-M.sat_tiles(cus) // tpr), R)), (fid, k, R)         # the smallest such
        for st in M.restated_steps(fid, k, general, env.get("LCPC_NTT_FORM")):
            wg = R << (k - st.s - st.log_tj) if st.kind == "general" else R << (k - 10)    # workgroups of this step's launch
            assert wg >= M.sat_tiles(cus), (fid, k, st)
            if st.kind == "general":
                assert ", 1024>" not in M.general_instantiation(fid, st.log_tile, st.s, st.log_tj, R, k)
        # the strided run (5 elements between rows) and the fills (a source stride of n / 2 + 3 <= n + 3)
        assert M.sat_case_bytes(fid, k, general, R, gap=5, src_extra=3) < M.SAT_MAX_BYTES, (fid, k, R)
    for k in M.MONTWORD_SIZES:
        assert M.sat_montword_splits(k)
        for passes in M.sat_montword_splits(k):
            assert sum(s for _, _, s, _ in passes) == k
            for lt, t0, s, ltj in passes:
                R = M.sat_rows(max(1, (1 << k) >> lt), cus)
                assert R % 2 == 1 and R % 3 != 0 and R << (k - s - ltj) >= M.sat_tiles(cus)
                assert 3 * R * (32 << k) < M.SAT_MAX_BYTES
    for fid, k in M.sat_commit_cases():
        R = M.sat_rows(M.sat_tiles_per_row(fid, k, False), cus)
        assert R % 2 == 1 and R % 3 != 0 and R * max(1, (1 << k) >> 10) >= M.sat_tiles(cus)
    assert {k for f, k in M.sat_commit_cases() if f == 3} == {5, 10} | set(range(11, 21))
    # the instantiations: exactly the required ones of these sizes and the ones the lists have no name for
    reached = M.sat_reached_instantiations(cus)
    assert not M.sat_required_instantiations() - reached, sorted(M.sat_required_instantiations() - reached)
    assert reached - M.sat_required_instantiations() == M.SAT_ALSO, sorted(reached - M.sat_required_instantiations())
    assert not [x for x in reached if ", 1024>" in x]
    assert {x for x in M.GENERAL_REQUIRED if ", 1024>" not in x} <= reached
    # ... and with the three-pass cases, the free splits and the one-row general launches of test_gpu_k1_passes.py: everything
    assert not (CM.ntt_required_instantiations() | M.GENERAL_REQUIRED) - (reached | M.reached_instantiations())


def test_saturating_row_counts():
    assert [M.sat_rows(t, 256) for t in (1, 2, 4, 8, 256, 512, 1024)] == [4097, 2051, 1025, 515, 17, 11, 5]
    assert M.sat_rows(1, 304) == 4865 and M.sat_rows(1024, 304) == 5 and M.sat_rows(1, 1) == 17


def test_free_splits_reach_the_paths_of_the_general_kernel():
    """what the free splits at 2^12 .. 2^14 columns reach, stated in tests/test_gpu_k1_passes.py's head"""
    want = {"s=1", "s odd", "s even", "lb < log_tj", "trivial last stages in a radix-4 round", "trivial last stage in the radix-2 tail"}
    for fid in range(4):
        for lt in M.free_tiles(fid):
            got = set()
            for k in M.FREE_SPLIT_SIZES:
                sp = M.free_splits(k, lt)
                assert all(s + ltj <= lt and t0 + s <= k for t0, s, ltj in sp) and len(set(sp)) == len(sp)
                for t0, s, ltj in sp:
                    got |= M.free_split_features(k, t0, s, ltj)
                # plan_passes' own split is one of them
                assert all((t0, s, ltj) in sp for t0, s, ltj, l in CM.general_passes(fid, k, True) if l == lt)
            assert got == want, (fid, lt, want - got)


def test_k1p_harness_is_a_library_of_its_own():
    """k1p_ only, no name of the product's, NEEDED-linked to the product, whose binary does not know the prefix; built without the test
    hooks, like the product whose context it reads"""
    from test_abi import _harness_is_a_separate_library
    _harness_is_a_separate_library("k1p_harness", "k1p_", "tests/native/k1p_harness.cpp", "K1PH_OUT")
    import subprocess
    make = lambda target: subprocess.check_output(["make", "-n", "-B", "-C", os.path.join(os.path.dirname(HERE), "lcpc_amd", "csrc"), target], text=True)
    assert "../lib/liblcpc_k1p_harness.so" in make("clean").split()
    rule, = [l for l in make("all").splitlines() if " -o ../lib/liblcpc_k1p_harness.so " in l]
    assert "LCPC_TEST_HOOKS" not in rule and "-llcpc_hip" in rule

"""K18 / K19, the sumcheck kernels (kernels.h launch_sumcheck_round, launch_sumcheck_bind, launch_sumcheck_bind_round), directly against
Python bignum (tests/sumcheck_cases.py, held to itself by tests/test_k18_cases.py) through tests/k18_harness.py.  Every stored element
and every evaluation must equal bignum; there is no tolerance.

With P the pairs a workgroup takes per stride (k18h_tile_pairs), the sizes stand at the edges of the structure: one pair, two, half a
wave, a wave, two waves, half a tile, a tile (the largest single launch), two tiles (two workgroups, a second launch) and four tiles
over three workgroups (a grid-stride loop with a ragged last stride).  For the fused form the same counts are its lanes, n / 4.  The
canaries around every output, the evals and the workspace and the inputs are checked by the harness at every call."""
import functools

import numpy as np
import pytest

import fft_cases as FC
import k18_harness as K18
import sumcheck_cases as MC

gpu = pytest.mark.gpu
MODES = ("bind", "round", "fused")
SIZE_TERMS = "eq_ab_minus_c"


def P(fid):
    return K18.tile_pairs(2 * FC.field(fid).L)


def lane_counts(fid):
    p = P(fid)
    return sorted({1, 2, 32, 64, 128, p // 2, p, 2 * p, 4 * p})


def length(mode, lanes):
    return (4 if mode == "fused" else 2) * lanes


@functools.lru_cache(maxsize=None)
def case(fid, name, order, n_tables, n):
    """(table limbs (n_tables, n, L), canonical tables): computed once"""
    tabs = MC.tables(fid, name, order, n_tables, n, "k18")
    return np.stack([FC.mont(fid, t) for t in tabs]), tuple(tuple(t) for t in tabs)


def seed(fid, *key):
    return FC.rng("k18-r", fid, *key).randrange(FC.field(fid).p)


@functools.lru_cache(maxsize=None)
def reference(fid, mode, name, order, tname, n):
    """(bound limbs or None, evals limbs or None) of the bignum model: computed once"""
    n_tables, terms = MC.terms_of(fid, tname)
    tabs = [list(t) for t in case(fid, name, order, n_tables, n)[1]]
    bound = evals = None
    if mode != "round":
        r = seed(fid, order, n)
        tabs = [MC.bind_ref(fid, order, t, r) for t in tabs]
        bound = np.stack([FC.mont(fid, t) for t in tabs])
    if mode != "bind":
        evals = FC.mont(fid, MC.round_ref(fid, order, tabs, terms))
    return bound, evals


def run(fid, mode, name, order, tname, n, max_groups=None, in_place=False):
    n_tables, terms = MC.terms_of(fid, tname)
    return K18.run(mode, fid, order, case(fid, name, order, n_tables, n)[0], terms, None if mode == "round" else seed(fid, order, n), max_groups, in_place)


def check(fid, mode, name, order, tname, n, got, tag):
    bound, evals = reference(fid, mode, name, order, tname, n)
    if bound is not None:
        assert np.array_equal(got[0], bound), (tag, np.argwhere((got[0] != bound).any(-1))[:8].tolist())
    if evals is not None:
        assert np.array_equal(got[1], evals), (tag, FC.canon(fid, got[1]), FC.canon(fid, evals))


@gpu
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("order", MC.ORDERS)
@pytest.mark.parametrize("fid", MC.FIELDS)
def test_sizes_at_the_edges_of_the_structure(fid, order, mode):
    p = P(fid)
    for lanes in lane_counts(fid):
        n = length(mode, lanes)
        cap = 3 if lanes == 4 * p else None
        got = run(fid, mode, "random", order, SIZE_TERMS, n, cap)
        check(fid, mode, "random", order, SIZE_TERMS, n, got, (lanes, cap))
        if mode != "bind":
            assert got[2] == (1 if lanes <= p else 2), (lanes, got[2])       # one workgroup finishes its sums itself
    if mode != "bind":
        # the same four tiles under other caps: one workgroup walks them all (one launch), four take one each; the limbs do not
        # depend on the grid
        n = length(mode, 4 * p)
        for cap, launches in ((1, 1), (4, 2), (K18.default_groups(), 2)):
            got = run(fid, mode, "random", order, SIZE_TERMS, n, cap)
            check(fid, mode, "random", order, SIZE_TERMS, n, got, ("cap", cap))
            assert got[2] == launches, (cap, got[2])


@gpu
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("order", MC.ORDERS)
@pytest.mark.parametrize("fid", MC.FIELDS)
def test_operand_sets_at_two_tiles(fid, order, mode):
    n = length(mode, 2 * P(fid))
    for name in MC.SETS:
        for tname in ("ab", SIZE_TERMS):
            check(fid, mode, name, order, tname, n, run(fid, mode, name, order, tname, n), (name, tname))


@gpu
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("order", MC.ORDERS)
@pytest.mark.parametrize("fid", MC.FIELDS)
def test_every_term_list_at_one_tile(fid, order, mode):
    n = length(mode, P(fid))
    for tname in MC.TERM_LISTS:
        got = run(fid, mode, "random", order, tname, n)
        check(fid, mode, "random", order, tname, n, got, tname)
        assert mode == "bind" or got[2] == 1


@gpu
@pytest.mark.parametrize("order", MC.ORDERS)
@pytest.mark.parametrize("fid", MC.FIELDS)
def test_fused_equals_bind_then_round(fid, order):
    """byte for byte: the stores of the bind, and the evals of the round on its output"""
    p = P(fid)
    for tname, lanes, cap in (("full", p // 2, None), (SIZE_TERMS, 2 * p, None), ("abcd", 4 * p, 3)):
        n = 4 * lanes
        n_tables, terms = MC.terms_of(fid, tname)
        tabs, r = case(fid, "random", order, n_tables, n)[0], seed(fid, order, n)
        bound, _, _ = K18.run("bind", fid, order, tabs, r=r)
        _, evals, launches = K18.run("round", fid, order, bound, terms, max_groups=cap)
        f_bound, f_evals, f_launches = K18.run("fused", fid, order, tabs, terms, r, cap)
        assert np.array_equal(f_bound, bound) and np.array_equal(f_evals, evals) and f_launches == launches, (tname, lanes)


@gpu
@pytest.mark.parametrize("mode", ("bind", "fused"))
@pytest.mark.parametrize("fid", MC.FIELDS)
def test_high_order_in_place_equals_out_of_place(fid, mode):
    p = P(fid)
    for lanes, cap in ((1, None), (p, None), (4 * p, 3)):
        n = length(mode, lanes)
        got = run(fid, mode, "random", "high", SIZE_TERMS, n, cap, in_place=True)
        check(fid, mode, "random", "high", SIZE_TERMS, n, got, ("in place", lanes))
        out = run(fid, mode, "random", "high", SIZE_TERMS, n, cap)
        assert np.array_equal(got[0], out[0]) and (mode == "bind" or np.array_equal(got[1], out[1]))


@gpu
@pytest.mark.parametrize("order", MC.ORDERS)
def test_saturated_grid_in_ft255(order):
    """h = the power of two at or above 2 x CUs x 4 x P pairs: every workgroup of the product's default cap runs its loop more than
    once.  Term a b, against the host form"""
    fid = 3
    F = FC.field(fid)
    cus = K18.lib().k18h_cu_count()
    assert cus > 0
    h = 1 << (2 * cus * 4 * P(fid) - 1).bit_length()
    n = 2 * h
    rng = np.random.default_rng(18)
    tabs = rng.integers(0, 1 << 64, size=(2, n, F.L), dtype=np.uint64)
    tabs[:, :, F.L - 1] = rng.integers(0, F.p >> (64 * (F.L - 1)), size=(2, n), dtype=np.uint64)     # (any value below p is a Montgomery form)
    terms = [(None, [0, 1])]
    want = MC.host_round(fid, order, [tabs[0], tabs[1]], terms)
    _, evals, launches = K18.run("round", fid, order, tabs, terms)
    assert launches == 2 and np.array_equal(evals, want)

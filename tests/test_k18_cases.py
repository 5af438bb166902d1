"""The cases of the sumcheck tests (tests/sumcheck_cases.py) and the constants the K18 harness reports, on the CPU: the builders do
what their names say, the bignum model agrees with itself (the two orders after a bit reversal of the tables, g(0) + g(1) against the
plain sum), the size of the workspace follows its definition, and the launchers settle every refusal before a launch
(k18h_refusal: never-read buffers, no device)."""
import numpy as np
import pytest

import fft_cases as FC
import k18_harness as K18
import sumcheck_cases as MC
from k18_harness import BadArgs

INVALID = K18.HIP_ERROR_INVALID_VALUE


def test_harness_constants():
    G = K18.default_groups()
    assert G >= 256 and K18.tile_pairs(3) == K18.tile_pairs(0) == 0
    for fid in MC.FIELDS:
        P = K18.tile_pairs(2 * FC.field(fid).L)
        assert P >= 64 and P % 64 == 0
        for pairs in (1, 2, P - 1, P, P + 1, 2 * P, 3 * P + 1, 4 * P, G * P, G * P + 1, 1 << 38):
            for cap in (1, 3, G):
                groups = min(-(-pairs // P), cap)
                for n_terms in (1, 4):
                    assert K18.work_elems(pairs, n_terms, cap) == groups * n_terms * 5, (pairs, cap, n_terms)
    assert K18.work_elems(0, 1, 4) == K18.work_elems(8, 0, 4) == K18.work_elems(8, 5, 4) == K18.work_elems(8, 1, 0) == 0


@pytest.mark.parametrize("fid", MC.FIELDS)
def test_builders_do_what_their_names_say(fid):
    F = FC.field(fid)
    for order in MC.ORDERS:
        for n in (2, 4, 8, 64):
            h = n // 2
            for name in MC.SETS:
                tabs = MC.tables(fid, name, order, 3, n)
                assert len(tabs) == 3 and all(len(t) == n and all(0 <= v < F.p for v in t) for t in tabs), (name, n)
                assert tabs == MC.tables(fid, name, order, 3, n), "the sets are seeded"
            for t in MC.tables(fid, "equal_halves", order, 2, n):
                assert all(t[MC.places(order, i, h)[0]] == t[MC.places(order, i, h)[1]] for i in range(h))
            for t in MC.tables(fid, "descending", order, 2, n):
                assert all(t[MC.places(order, i, h)[0]] > t[MC.places(order, i, h)[1]] for i in range(h))
    # the wrap set: a product with table 0 once is p - 1 at every t, so the running sums are p - 1, p - 2, ... : every step wraps
    tabs = MC.tables(fid, "wrap", "low", 2, 8)
    assert MC.round_ref(fid, "low", tabs, [(None, [0, 1])]) == [F.p - 4] * 3
    assert MC.round_ref(fid, "low", MC.tables(fid, "max", "low", 2, 8), [(None, [0, 1])]) == [4] * 3
    assert MC.round_ref(fid, "high", MC.tables(fid, "zeros", "high", 1, 8), [(None, [0])]) == [0, 0]
    for name in MC.TERM_LISTS:
        n_tables, terms = MC.terms_of(fid, name)
        assert 1 <= len(terms) <= 4 and all(1 <= len(idx) <= 4 and max(idx) < n_tables <= 8 for _, idx in terms)
        assert {k for _, idx in terms for k in idx} == set(range(n_tables)), "every table is used"
    assert MC.terms_of(fid, "eq_ab_minus_c")[1] == [(1, [0, 1, 2]), (F.p - 1, [0, 3])]
    assert len(MC.terms_of(fid, "full")[1]) == 4 and MC.terms_of(fid, "full")[0] == 8


@pytest.mark.parametrize("fid", MC.FIELDS)
def test_model_agrees_with_itself(fid):
    F = FC.field(fid)
    r = FC.rng("k18-cases", fid).randrange(F.p)
    for n in (2, 4, 32):
        v = n.bit_length() - 1
        for name in MC.TERM_LISTS:
            n_tables, terms = MC.terms_of(fid, name)
            tabs = MC.tables(fid, "random", "low", n_tables, n, "self")
            rev = [MC.bitrev_table(t) for t in tabs]
            # the two orders after a bit reversal of the tables: the same pairs, so the same round and the same bound values
            g = MC.round_ref(fid, "low", tabs, terms)
            assert g == MC.round_ref(fid, "high", rev, terms), (n, name)
            assert len(g) == MC.degree(terms) + 1 and (g[0] + g[1]) % F.p == MC.composition_sum(fid, tabs, terms)
            for t, tr in zip(tabs, rev):
                lo = MC.bind_ref(fid, "low", t, r)
                assert len(lo) == n // 2 and (MC.bitrev_table(lo) if v > 1 else lo) == MC.bind_ref(fid, "high", tr, r)
            # binding to 0 and to 1 selects the halves; the next round's sum is g(r)
            assert MC.bind_ref(fid, "high", tabs[0], 0) == tabs[0][:n // 2] and MC.bind_ref(fid, "high", tabs[0], 1) == tabs[0][n // 2:]
            assert MC.bind_ref(fid, "low", tabs[0], 0) == tabs[0][0::2] and MC.bind_ref(fid, "low", tabs[0], 1) == tabs[0][1::2]
            bound = [MC.bind_ref(fid, "low", t, r) for t in tabs]
            assert MC.composition_sum(fid, bound, terms) == MC.interpolate(fid, g, r), (n, name)
    assert MC.interpolate(fid, [3, 5, 11], 2) == 11 and MC.interpolate(fid, [7], 12345) == 7


@pytest.mark.parametrize("fid", MC.FIELDS)
def test_launchers_settle_their_refusals_before_any_launch(fid):
    nl = 2 * FC.field(fid).L
    n = 1 << 12
    for mode in ("bind", "round", "fused"):
        bind, rnd = mode != "round", mode != "bind"
        ref = lambda **kw: K18.refusal(mode, nl, kw.pop("order", "high"), kw.pop("n", n), **kw)
        with pytest.raises(BadArgs):
            ref()                                                        # a job the launcher would launch is not handed over
        assert K18.refusal(mode, 3, "high", n) == INVALID and K18.refusal(mode, 10, "low", n) == INVALID
        assert ref(order=2) == INVALID
        for bad_n in (0, 1, 3, n - 1, n + 2, 1 << 39, 1 << 40):
            assert ref(n=bad_n) == INVALID, bad_n
        if mode == "fused":
            assert ref(n=2) == INVALID
        assert ref(n_tables=0) == INVALID and ref(n_tables=9) == INVALID
        assert ref(null_mask=1) == INVALID and ref(null_mask=2) == INVALID and ref(misalign=2) == INVALID
        if bind:
            assert ref(null_mask=4) == INVALID and ref(null_mask=8) == INVALID and ref(misalign=8) == INVALID and ref(null_mask=128) == INVALID
            for order in ("low", "high"):
                for overlap in (2, 3, 7, 8, 9):
                    assert ref(order=order, overlap=overlap) == INVALID, (order, overlap)
            assert ref(order="low", overlap=1) == INVALID                # in place under low first
            with pytest.raises(BadArgs):
                ref(order="high", overlap=1)                             # in place under high first is a job
        if rnd:
            assert ref(null_mask=16) == INVALID and ref(null_mask=32) == INVALID and ref(null_mask=64) == INVALID and ref(null_mask=256) == INVALID
            assert ref(misalign=16) == INVALID and ref(misalign=32) == INVALID
            assert ref(short_work=1) == INVALID and ref(max_groups=0) == INVALID
            assert ref(n_terms=0) == INVALID and ref(terms=np.zeros((5, 5), np.uint32) + 1, n_terms=5) == INVALID
            for rec in ([0, 0, 0, 0, 0], [5, 0, 0, 0, 0], [2, 0, 2, 0, 0], [4, 0, 1, 0, 9]):      # n_factors, a table index
                assert ref(terms=np.array([[1, 0, 0, 0, 0], rec], np.uint32), n_terms=2) == INVALID, rec
            for overlap in (4, 6) + ((5, 10) if bind else ()):
                assert ref(overlap=overlap) == INVALID, overlap

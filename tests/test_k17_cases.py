"""The cases of the scan tests (tests/scan_cases.py) and the constants the K17 harness reports, on the CPU: the builders stay in range
and put their zeros where they say, the bignum references agree with each other (inclusive against exclusive shifted by one, a scan
cut in two and chained against the whole), and the size of the workspace is the sum of the tile counts of every level."""
import pytest

import fft_cases as FC
import k17_harness as K17
import scan_cases as SC


def geometry(fid):
    nl = 2 * FC.field(fid).L
    return nl, K17.tile(nl), K17.lane_elems(nl), K17.mid_chunk(nl)


@pytest.mark.parametrize("fid", SC.FIELDS)
def test_harness_constants(fid):
    nl, T, c, M = geometry(fid)
    assert T == 256 * c and c in (8, 16) and M == T
    assert K17.tile(3) == K17.lane_elems(5) == K17.mid_chunk(7) == 0
    tiles = lambda n: -(-n // T)
    last = 0
    for n in list(range(1, 40)) + [T - 1, T, T + 1, 2 * T + 17, T * T - 1, T * T, T * T + 1, (M + 1) * T + 5, 1 << 30, (1 << 39) - 1]:
        want, t = 0, n
        while True:
            t = tiles(t)
            want += t
            if t == 1:
                break
        assert K17.work_elems(nl, n) == want >= last and K17.work_elems(nl, n, 3) == 3 * want, n
        last = want
    assert K17.work_elems(nl, 0) == K17.work_elems(nl, 1 << 39) == K17.work_elems(nl, 5, 0) == K17.work_elems(nl, 5, 65536) == 0


@pytest.mark.parametrize("fid", SC.FIELDS)
def test_builders_stay_in_range_and_place_their_zeros(fid):
    F = FC.field(fid)
    _, T, c, _ = geometry(fid)
    for n in (1, 2, c - 1, c, c + 1, 63, 64, 65, 64 * c - 1, 64 * c + 1, T - 1, T, T + 1, 2 * T + 17):
        for name in SC.SETS:
            x = SC.operands(fid, name, n, T, c)
            assert len(x) == n and all(0 <= v < F.p for v in x), (n, name)
            assert x == SC.operands(fid, name, n, T, c), "the sets are seeded"
            if name in SC.EDGES:
                at = SC.edge_position(name, n, T, c)
                assert [i for i, v in enumerate(x) if v == 0] == [at], (n, name)
        assert set(SC.operands(fid, "all_pm1_sum", n, T, c)) <= {1, F.p - 1}
    n = 2 * T + 17
    at = {name: SC.edge_position(name, n, T, c) for name in SC.EDGES}
    assert at["zero_lane_first"] % c == 0 and at["zero_lane_last"] % c == c - 1 and at["zero_lane_first"] // c == at["zero_lane_last"] // c
    assert at["zero_tile_first"] == T and at["zero_tile_last"] == 2 * T - 1 and at["zero_vec_first"] == 0 and at["zero_vec_last"] == n - 1
    assert len(set(at.values())) == 6


@pytest.mark.parametrize("fid", SC.FIELDS)
def test_references_agree_with_each_other(fid):
    F = FC.field(fid)
    c = FC.rng("k17-cases", fid).randrange(1, F.p)
    for name in SC.SETS:
        x = SC.operands(fid, name, 300, 64, 8)
        for op in SC.OPS:
            e = 0 if op == "sum" else 1
            for init in (None, c):
                inc, t_inc = SC.scan_ref(fid, op, "inclusive", x, init)
                exc, t_exc = SC.scan_ref(fid, op, "exclusive", x, init)
                assert t_inc == t_exc == inc[-1] and exc == [e if init is None else init] + inc[:-1], (name, op)
                for mode in SC.MODES:
                    whole, total = SC.scan_ref(fid, op, mode, x, init)
                    a, ta = SC.scan_ref(fid, op, mode, x[:113], init)
                    b, tb = SC.scan_ref(fid, op, mode, x[113:], ta)
                    assert a + b == whole and tb == total, (name, op, mode)
    # the sets do what their names say
    ones = SC.scan_ref(fid, "product", "inclusive", SC.operands(fid, "minus_ones", 6), None)[0]
    assert ones == [F.p - 1, 1] * 3
    sums = SC.scan_ref(fid, "sum", "inclusive", SC.operands(fid, "minus_ones", 3), None)[0]
    assert sums == [F.p - 1, F.p - 2, F.p - 3]
    x = SC.operands(fid, "zero_lane_last", 100, 64, 8)
    at = SC.edge_position("zero_lane_last", 100, 64, 8)
    prod = SC.scan_ref(fid, "product", "inclusive", x)[0]
    assert all(prod[:at]) and not any(prod[at:])
    assert SC.ratio_terms(fid, [5, 7], [0, 1]) == [0, 7]

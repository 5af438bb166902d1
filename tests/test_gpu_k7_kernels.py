"""K7b, the column check of the batched verify (kernels.hip launch_verify_columns_batch), directly against Python-int expectations
(tests/k7_harness.py Case, itself checked by tests/test_k7_cases.py), for every field.

The kernel gives one wave to an opened column: lane l takes rows l, l + 64, ..., accumulates unreduced and reduces every 8 terms
(Ft255: normalises every 6 terms, reduces every 60), and the lanes' sums are added across the wave.  So the row counts are: a single
row, a partly filled wave, the collapse kernels' 60-row block and one past it, a full wave, more rows than lanes, and the first row
counts at which a lane reaches its second reduction block (8 * 64 + 1), Ft255's second normalisation (6 * 64 + 1) and Ft255's second
60-term block (60 * 64 + 1)."""
import numpy as np
import pytest

import k7_harness as H

pytestmark = pytest.mark.gpu

FIELDS = [0, 1, 2, 3]
N_COLS = 16
DRAWN = [0, N_COLS - 1, 5, 5, 0, 9, N_COLS + 3]          # first, last, duplicates, one that does not exist


def check(case):
    got = case.run()
    want = case.expected()
    assert np.array_equal(got, want), (got.tolist(), want.tolist())
    return got


@pytest.mark.parametrize("n_rows", [1, 8, 60, 61, 64, 100, 300, 385, 513])
@pytest.mark.parametrize("fid", FIELDS)
def test_row_counts(fid, n_rows):
    """honest columns pass, the column that does not exist reports a mismatch (and nothing faults), at two tensors"""
    c = H.Case(fid, n_rows, 2, N_COLS, [DRAWN], seed=n_rows)
    got = check(c)
    assert got[0, :-1].tolist() == [0] * (len(DRAWN) - 1) and got[0, -1] == (H.DEGREE_BIT | H.EVAL_BIT)


def test_second_lazy_block_of_a_lane():
    """Ft255: 60 * 64 + 1 rows, lane 0 reduces its first 60 terms and starts a second block; worst-case operands as well"""
    for fill in ("random", "max"):
        check(H.Case(3, 60 * 64 + 1, 2, N_COLS, [[3, 0]], fill=fill))


@pytest.mark.parametrize("n_t", [1, 2, 4, 5])
@pytest.mark.parametrize("fid", FIELDS)
def test_tensor_counts(fid, n_t):
    """1, 2 and 4 tensors in one pass over the column; 5: a second pass.  A mismatch planted in exactly one (column, tensor) pair sets
    exactly that column's bit: bit 0 for a degree row, bit 1 for the last tensor"""
    for d in range(n_t):
        c = H.Case(fid, 100, n_t, N_COLS, [[0, 15, 7, 3, 20]], seed=10 * n_t + d)
        c.plant(0, 2, d)
        got = check(c)
        bit = H.EVAL_BIT if d == n_t - 1 else H.DEGREE_BIT
        assert got[0].tolist() == [0, 0, bit, 0, (H.DEGREE_BIT if n_t > 1 else 0) | H.EVAL_BIT]


@pytest.mark.parametrize("fill", ["max", "zero"])
@pytest.mark.parametrize("n_rows", [61, 300, 513])
@pytest.mark.parametrize("fid", FIELDS)
def test_worst_case_operands(fid, n_rows, fill):
    """every tensor and column element p - 1 (the largest products the lazy accumulators can meet), and all zero; with a planted
    mismatch, so that a kernel that compared nothing would be seen"""
    c = H.Case(fid, n_rows, 4, N_COLS, [[0, 15, 5, 5, 16]], fill=fill)
    c.plant(0, 1, 3)
    c.plant(0, 2, 1)
    got = check(c)
    assert got[0].tolist() == [0, H.EVAL_BIT, H.DEGREE_BIT, H.DEGREE_BIT, H.DEGREE_BIT | H.EVAL_BIT]


@pytest.mark.parametrize("fid", FIELDS)
def test_members_with_differing_data_and_a_poisoned_gap(fid):
    """3 members, each with its own tensors, columns, encoded rows and drawn numbers; the member stride of the columns is larger than
    their extent (an odd one: members of Ft63 / Ft191 then sit at 8-byte, not 16-byte, offsets) with all-ones limbs in the gap;
    5 opened columns: the last workgroup of four waves is partly filled"""
    n_rows, n_open = 100, 5
    drawn = [[0, 1, 2, 3, 4], [15, 15, 0, 8, 99], [7, 6, 5, 4, 3]]
    stride = n_open * n_rows + (8 if fid in (1, 3) else 7)
    c = H.Case(fid, n_rows, 3, N_COLS, drawn, stride=stride, seed=77)
    c.plant(1, 3, 2)
    c.plant(2, 0, 0)
    c.plant(2, 4, 1)
    c.plant(2, 4, 2)
    got = check(c)
    assert got.tolist() == [[0, 0, 0, 0, 0], [0, 0, 0, H.EVAL_BIT, H.DEGREE_BIT | H.EVAL_BIT],
                            [H.DEGREE_BIT, 0, 0, 0, H.DEGREE_BIT | H.EVAL_BIT]]


def test_many_opened_columns():
    """Brakedown opens thousands of columns: 6593 of 8 rows, two members -- 1649 workgroups per member, the last with one wave"""
    import random
    rng = random.Random(5)
    n_cols = 8000
    drawn = [[rng.randrange(n_cols) for _ in range(6593)] for _ in range(2)]
    c = H.Case(0, 8, 2, n_cols, drawn, seed=6)
    c.plant(1, 6592, 1)
    c.plant(0, 4000, 0)
    got = check(c)
    assert got[1, 6592] == H.EVAL_BIT and got[0, 4000] == H.DEGREE_BIT

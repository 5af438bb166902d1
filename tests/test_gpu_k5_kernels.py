"""The prover's kernels (K5 / K6 of lcpc_amd/csrc/kernels.h), launcher by launcher, against Python-int expectations (tests/k5_harness.py,
itself checked by tests/test_k5_cases.py): collapse in the single and the batch form, to_r29, the split sum in both forms, to_mont /
to_canon, the column and path gathers in both forms, assemble_columns.  Every comparison is equality of the WHOLE output array with the
expected one: the values the kernel must write, bit for bit, and the pre-filled sentinel everywhere it must not write.

The shapes are the smallest at which each path exists: 300 columns (one ragged 256-lane block); rows per split across the collapse's
reduction cadences (tests/test_lazy_bounds.py); split counts that are no power of two and splits with no row; column ranges with
j0 > 0 at both output strides; members of a batch with distinct data, in memory in another order than in the batch, poison between
them; canonical beside Montgomery and row-major beside position-major members; 16384 + 257 rows (the grid-stride loop behind 64 row
blocks) and 32768 + 3 opened columns (the second slice) for the column gathers.

Out of scope: the grid-stride loops of to_mont / to_canon start beyond 2^24 elements (65536 blocks of 256), which is more than the
harness takes.

Measured on an MI355X: the 266 tests of this file take 8.3 s together; the slowest, 1.8 s, is the first to run
(test_collapse_single[0-1]: it loads the library and opens the device), every other stays under 0.25 s."""
import random

import numpy as np
import pytest

import k5_harness as H
from common import field_p, maxt

pytestmark = pytest.mark.gpu

FIELDS = [0, 1, 2, 3]


def check(case, what=None):
    got, want = case.run(), case.expected()
    if not np.array_equal(got, want):
        bad = np.nonzero((got != want).reshape(len(got), -1).any(axis=1))[0]
        raise AssertionError("%s: %d of %d entries differ, the first at %d: got %s, expected %s"
                             % (what or type(case).__name__, len(bad), len(got), bad[0], got[bad[0]].tolist(), want[bad[0]].tolist()))


def _view_id(v):
    return "nt%d-[%d,%d)-stride%d-%s" % (v.n_tensors, v.j0, v.j1, v.out_stride, "limb" if v.limb else "words")


# ---- K5 / K5b ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_splits", [1, 2, 3, 64])
@pytest.mark.parametrize("fid", FIELDS)
def test_collapse_single(fid, n_splits):
    """launch_collapse on one set of coefficients: every split's partial sums (n_splits > 1: [split][tensor][out_stride]; a split with
    no row writes zeros), 1 and 2 tensors, the whole row by the launcher's defaults and the range [37, 293) at the row stride and
    packed, MAXC / p - 1 / random rows against MAXT / p - 1 / random tensor entries.  Ft255 runs collapse29_kernel (tensors29 from
    launch_to_r29) and collapse_kernel<8, NT> (tensors29 null): both must give the reference."""
    for n_rows, ns in H.collapse_single_shapes(fid, n_splits):
        data = H.CollapseData(fid, n_rows, H.N_PER_ROW, seed=n_rows)
        for v in H.collapse_views(data, ns):
            check(v, "%d rows, %d splits, %s" % (n_rows, ns, _view_id(v)))


@pytest.mark.parametrize("fid,shape", [(f, s) for f in FIELDS for s in H.collapse_batch_shapes(f)],
                         ids=lambda x: "rows%d-splits%d-batch%d" % x if isinstance(x, tuple) else "ft%d" % x)
def test_collapse_batch(fid, shape):
    """CollapseArgs.members: member z reads its own coefficients through its descriptor (the buffers sit in memory in another order
    than in the batch, poison around them; CollapseArgs.coeffs is null), its own tensors at z * n_tensors * n_rows and writes at
    z * n_splits * n_tensors * out_stride"""
    n_rows, n_splits, n_batch = shape
    data = H.CollapseData(fid, n_rows, H.N_PER_ROW, n_batch, seed=n_rows)
    for v in H.collapse_views(data, n_splits, n_batch):
        check(v, _view_id(v))


def test_to_r29():
    """0, 1, p - 1, MAXT (whose 32-fold is the collapse's largest multiplier), the values around ceil(p / 32) where 32 t first wraps,
    around every further multiple of p / 32 near the top, and 300 random ones (two blocks, the second ragged)"""
    p = field_p(3)
    w = -(-p // 32)
    rng = random.Random(29)
    vals = [0, 1, 2, p - 1, p - 2, maxt(3), w - 2, w - 1, w, w + 1, 2 * w - 1, 2 * w, 31 * w - 1, 31 * w, (1 << 255) % p, (1 << 224) - 1]
    vals += [rng.randrange(p) for _ in range(300)]
    assert all(0 <= v < p for v in vals)
    got = H.to_r29(vals)
    assert np.array_equal(got, H.r29_expected(vals, len(got)))


# ---- the split sum ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_elems", [1, 255, 257])
@pytest.mark.parametrize("n_parts", [1, 2, 3, 63, 64])
@pytest.mark.parametrize("fid", FIELDS)
def test_split_sum(fid, n_parts, n_elems):
    """launch_field_sum and launch_field_sum_batch: 1, 255 and 257 elements, every part p - 1 (n_parts (p - 1) mod p: the most
    reductions) and random parts; 1, 3 and 7 members; the sums right behind the parts and nothing behind the sums"""
    for fill in ("max", "random"):
        for n_batch in (None, 1, 3, 7):
            check(H.SumCase(fid, n_parts, n_elems, n_batch, fill, seed=n_elems), "%s, batch %s" % (fill, n_batch))


# ---- to_mont / to_canon -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 255, 257, 1000])
@pytest.mark.parametrize("fid", FIELDS)
def test_representation_changes(fid, n):
    """x R and x / R mod p of 0, 1, p - 1, R mod p and random values, out of place and in place (in == out)"""
    p = field_p(fid)
    rng = random.Random(n)
    special = [0, 1, p - 1, H.mont_r(fid) % p, p - 2, 2]
    lists = [(special + [rng.randrange(p) for _ in range(n)])[:n]] if n > 1 else [[v] for v in special]
    for vals in lists:
        for to_mont in (False, True):
            want = H.convert_expected(fid, vals, to_mont)
            for in_place in (False, True):
                got = H.convert(fid, vals, to_mont, in_place)
                assert np.array_equal(got, want), (to_mont, in_place, np.nonzero((got != want).any(axis=1))[0][:5])


# ---- K6 / K6b ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("canon", [False, True], ids=["montgomery", "canonical"])
@pytest.mark.parametrize("layout", ["row", "pos"])
@pytest.mark.parametrize("fid", FIELDS)
def test_gather_columns_single(fid, layout, canon):
    """launch_gather_columns on a row-major and a position-major matrix, with r2 (canonical values come out times R) and without:
    1, 255 and 257 rows with column lists holding 0, n_cols - 1 and duplicates; 16384 + 257 rows, two columns: the grid-stride
    loop behind 64 row blocks; 32768 + 3 opened columns of 2 rows: the second slice's cols + s0 and vals + s0 * n_rows * nl"""
    for n_rows in (1, 255, 257):
        check(H.GatherCase(fid, n_rows, 6, [H.col_list(7, 6)], [layout], [canon], batch=False, seed=n_rows), "%d rows" % n_rows)
    check(H.GatherCase(fid, 16384 + 257, 3, [[2, 0]], [layout], [canon], batch=False, seed=11), "16641 rows")
    check(H.GatherCase(fid, 2, 7, [H.col_list(H.SLICE + 3, 7)], [layout], [canon], batch=False, seed=12), "two slices")


@pytest.mark.parametrize("name", list(H.gather_batch_cases(0)))
@pytest.mark.parametrize("fid", FIELDS)
def test_gather_columns_batch(fid, name):
    """launch_gather_columns_batch: 1, 3 and 5 members with their own column lists; canonical beside Montgomery members (r2 by the
    descriptor) and row-major beside position-major ones in one batch; the grid-stride loop; the second slice at two members"""
    check(H.gather_batch_cases(fid)[name](), name)


def test_gather_paths_single_at_16_words():
    """launch_gather_paths with 64-byte digests (8 words: tests/test_gpu_k3_kernels.py), the whole path and one level short of it"""
    for np2 in (2, 64, 4096):
        depth = np2.bit_length() - 1
        for path_len in (depth, depth - 1):
            for n_open in (1, 5):
                check(H.PathsCase(16, np2, path_len, [H.path_cols(n_open, np2, 0)], batch=False, seed=np2), (np2, path_len, n_open))
    check(H.PathsCase(16, 4096, 12, [[(37 * k) % 4096 for k in range(300)]], batch=False, seed=3), "300 columns")


@pytest.mark.parametrize("name", list(H.paths_batch_cases(8)))
@pytest.mark.parametrize("dw", [8, 16])
def test_gather_paths_batch(dw, name):
    """launch_gather_paths_batch: one flat launch over [member][opened column][level], n_open * path_len no multiple of 256, the
    members' trees in shuffled order, their column lists differing"""
    check(H.paths_batch_cases(dw)[name](), name)


# ---- assemble_columns -------------------------------------------------------------------------------------------------------------------------
ROW_BOUNDS = {
    "one-rank": [0, 7],
    "two-uneven": [0, 5, 7],
    "two-first-empty": [0, 0, 7],
    "two-last-empty": [0, 7, 7],
    "eight-uneven": [0, 1, 4, 5, 9, 12, 13, 20, 21],
    "eight-empty-first-middle-last": [0, 0, 3, 3, 3, 8, 9, 9, 9],
    "eight-fewer-rows-than-ranks": [0, 0, 1, 1, 2, 2, 2, 3, 3],
    "eight-one-row": [0, 0, 0, 0, 0, 1, 1, 1, 1],
    "two-three-blocks": [0, 300, 601],
}


@pytest.mark.parametrize("bounds", list(ROW_BOUNDS))
@pytest.mark.parametrize("fid", FIELDS)
def test_assemble_columns(fid, bounds):
    """[rank][k][rows of rank] -> [k][all rows] for 1, 2 and 8 ranks with uneven and empty shares, 1 and 3 opened columns, blocks as
    large as the largest rank needs and larger (poison in the slack)"""
    for n in (1, 3):
        for slack in (0, 6):
            check(H.AssembleCase(fid, ROW_BOUNDS[bounds], n, slack=slack, seed=n + slack), "n = %d, slack %d" % (n, slack))

"""K12 / K13, the whole-vector transform (kernels.h launch_fft), directly against Python bignum (tests/fft_cases.py, itself held to
the direct sum by tests/test_fft_abi.py) through tests/k12_harness.py: four fields x six forms x log_n 0 .. 13 x the tile sizes 2, 4,
8, 32 and the product's own.  Every stored element must equal bignum; there is no tolerance.

The small tiles put every shape a pass kernel has at the smallest sizes: transforms shorter than a tile, a last pass with fewer
stages than the others, one, two, three and up to thirteen passes, strided tiles with fewer columns than a wave and column lists
that end inside a workgroup (three vectors).  The twiddle table is built by the test, not by the product."""
import functools

import numpy as np
import pytest

import fft_cases as FC
import k12_harness as K12

gpu = pytest.mark.gpu
OK, INVALID = K12.HIP_SUCCESS, K12.HIP_ERROR_INVALID_VALUE
LOG_NS = range(0, 14)
LOG_TILES = [1, 2, 3, 5, "largest"]


def log_tile_of(t):
    return K12.max_log_tile() if t == "largest" else t


@functools.lru_cache(maxsize=None)
def vector_case(fid, form, log_n, v):
    """(input, expected output) of vector v as (n, L) limbs: the pair (fid, log_n, v) of fft_cases, computed once and left unchanged"""
    a, b = FC.io_of(form, *FC.pair(fid, log_n, v))
    return FC.mont(fid, a), FC.mont(fid, b)


def case(fid, form, log_n, n_vecs):
    """(input, expected output) as (n_vecs, n, L) limbs"""
    ins, outs = zip(*(vector_case(fid, form, log_n, v) for v in range(n_vecs)))
    return np.stack(ins), np.stack(outs)


def test_plan_is_the_documented_split():
    """ceil(log_n / log_tile) passes of log_tile stages, the last with the remainder; refused outside the launcher's range"""
    top = K12.max_log_tile()
    assert top >= 5
    for log_tile in range(1, top + 1):
        for log_n in range(0, 33):
            s = K12.plan(log_n, log_tile)
            assert len(s) == -(-log_n // log_tile) and sum(s) == log_n
            assert all(v == log_tile for v in s[:-1]) and (not s or 1 <= s[-1] <= log_tile)
    assert K12.plan(5, 0) is None and K12.plan(5, top + 1) is None and K12.plan(33, top) is None


def test_table_is_within_the_bound():
    for log_n in range(0, 33):
        assert K12.lib().k12h_tab_elems(log_n) <= 1 << ((log_n + 1) // 2 + 1)
        h = K12.lib().k12h_tab_split(log_n)
        assert K12.lib().k12h_tab_elems(log_n) == (1 << h) + (1 << (log_n - h))


@pytest.mark.parametrize("nl", [2, 4, 6, 8])
def test_launcher_refusals(nl):
    """what the launcher settles before any launch, on null or never-read buffers: no device is touched"""
    top = K12.max_log_tile()
    assert K12.refusal(3, 1, 4, top, 1) == INVALID and K12.refusal(nl + 1, 1, 4, top, 1) == INVALID
    assert K12.refusal(nl, -1, 4, top, 1) == INVALID and K12.refusal(nl, 6, 4, top, 1) == INVALID
    assert K12.refusal(nl, 1, 4, 0, 1) == INVALID and K12.refusal(nl, 1, 4, top + 1, 1) == INVALID
    assert K12.refusal(nl, 1, 33, top, 1) == INVALID
    assert K12.refusal(nl, 1, 4, top, 0) == INVALID and K12.refusal(nl, 1, 4, top, 65536) == INVALID
    assert K12.refusal(nl, 1, 32, top, 128) == INVALID and K12.refusal(nl, 1, 24, top, 32768) == INVALID      # 2^39 elements
    for form in range(6):
        for bit in range(3):
            assert K12.refusal(nl, form, 4, top, 1, 1 << bit) == INVALID, (form, bit)
            assert K12.refusal(nl, form, 4, top, 1, 0, 1 << bit) == INVALID, (form, bit)
        if form >= 3:
            assert K12.refusal(nl, form, 4, top, 1, 8) == INVALID
        assert K12.refusal(nl, form, 0, top, 1, 1) == INVALID and K12.refusal(nl, form, 0, top, 1, 0, 2) == INVALID
    with pytest.raises(K12.BadArgs):
        K12.refusal(nl, 1, 4, top, 1)             # a job a correct launcher would launch is not for this entry point


@gpu
@pytest.mark.parametrize("log_tile", LOG_TILES)
@pytest.mark.parametrize("fid", FC.FIELDS)
def test_every_form_every_size(fid, log_tile):
    """one vector and three, out of place: every element equals bignum, the canaries stand, the launches are the plan's passes (one
    more for the forms that permute)"""
    lt = log_tile_of(log_tile)
    for log_n in LOG_NS:
        passes = len(K12.plan(log_n, lt))
        assert passes == -(-log_n // lt)
        for form in FC.FORMS:
            for n_vecs in (1, 3):
                x, want = case(fid, form, log_n, n_vecs)
                got, launches = K12.run(fid, form, log_n, lt, x)
                assert np.array_equal(got, want), (form, log_n, n_vecs, np.argwhere((got != want).any(-1))[:8].tolist())
                assert passes <= launches <= passes + 1, (form, log_n, launches)
                if form[-2:] != "ii" or log_n == 0:
                    assert launches == passes, (form, log_n, launches)


@gpu
@pytest.mark.parametrize("log_tile", LOG_TILES)
@pytest.mark.parametrize("fid", FC.FIELDS)
def test_in_place(fid, log_tile):
    lt = log_tile_of(log_tile)
    for log_n in (0, 1, 2, 5, 6, 7, 11, 13):
        for form in FC.FORMS:
            for n_vecs in (1, 3):
                x, want = case(fid, form, log_n, n_vecs)
                got, _ = K12.run(fid, form, log_n, lt, x, in_place=True)
                assert np.array_equal(got, want), (form, log_n, n_vecs)


@gpu
@pytest.mark.parametrize("fid", FC.FIELDS)
def test_65535_vectors_of_two_points(fid):
    """the largest vector count: X = (a + b, a - b), the inverse halves it"""
    F = FC.field(fid)
    rnd = FC.rng("many", fid)
    a = [rnd.randrange(F.p) for _ in range(2 * 65535)]
    a[0], a[1], a[2], a[3] = F.p - 1, F.p - 1, 0, F.p - 1
    x = FC.mont(fid, a).reshape(65535, 2, F.L)
    fwd = FC.mont(fid, [v for i in range(65535) for v in ((a[2 * i] + a[2 * i + 1]) % F.p, (a[2 * i] - a[2 * i + 1]) % F.p)]).reshape(x.shape)
    for form in FC.FORMS:
        for lt in (1, K12.max_log_tile()):
            if form.startswith("ifft"):
                got, _ = K12.run(fid, form, 1, lt, fwd)
                assert np.array_equal(got, x), form
            else:
                got, _ = K12.run(fid, form, 1, lt, x)
                assert np.array_equal(got, fwd), form


@gpu
@pytest.mark.parametrize("fid", FC.FIELDS)
def test_worst_case_operands(fid):
    """every element p - 1 (X[0] = n (p - 1), zero elsewhere) and every STORED limb pattern p - 1, at a three-pass size"""
    F = FC.field(fid)
    log_n = 9
    n = 1 << log_n
    got, _ = K12.run(fid, "fft_ii", log_n, 3, FC.mont(fid, [F.p - 1] * n))
    assert np.array_equal(got[0], FC.mont(fid, [n * (F.p - 1) % F.p] + [0] * (n - 1)))
    import oracle_lib as O
    stored = np.tile(O.ints_to_limbs([F.p - 1], F.L), (n, 1))
    x = FC.canon(fid, stored)
    for form in FC.FORMS:
        got, _ = K12.run(fid, form, log_n, 3, stored)
        assert np.array_equal(got[0], FC.mont(fid, FC.apply_form(fid, form, x))), form

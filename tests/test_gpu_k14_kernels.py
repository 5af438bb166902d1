"""K14, the coset transform and the extension (kernels.h launch_coset_fft / launch_extend), directly against Python bignum
(tests/domain_cases.py over tests/fft_cases.py, held to the definitions by tests/test_domain_abi.py) through tests/k14_harness.py.
Every stored element must equal bignum; there is no tolerance.

The small tiles put every shape a pass has at the smallest sizes: one to eleven passes, a short last pass, column lists that end
inside a workgroup (three vectors), and for the extension blocks whose shift differs within one workgroup's column list and, with
tiles of 2, 4 and 8 points, across workgroups.  The twiddle and shift tables are built by the test, not by the product.  The launch
counts are the header's promises: a coset transform takes the launches of the plain one (K12's own count is asked for beside it),
a bit-reversed extension those of an FFT_IO of 2^ceil(log2 n_coeffs) points whatever b is, the natural order one more."""
import functools

import numpy as np
import pytest

import domain_cases as DC
import fft_cases as FC
import k12_harness as K12
import k14_harness as K14

gpu = pytest.mark.gpu
INVALID = K14.HIP_ERROR_INVALID_VALUE
LOG_NS = range(0, 12)
LOG_TILES = [1, 2, 3, 5, "largest"]
SHIFTS = ("gen", "random")


def log_tile_of(t):
    return K12.max_log_tile() if t == "largest" else t


@functools.lru_cache(maxsize=None)
def vector_case(fid, form, log_n, v, shift):
    """(input, expected output, canonical shift) of vector v: x random, X its coset transform, both natural; computed once"""
    s = DC.shifts(fid, "k14", log_n)[shift]
    x = FC.random_vector(fid, log_n, "k14", v)
    a, b = FC.io_of(form, x, DC.coset_dft(fid, x, s))
    return FC.mont(fid, a), FC.mont(fid, b), s


def case(fid, form, log_n, n_vecs, shift):
    ins, outs, s = zip(*(vector_case(fid, form, log_n, v, shift) for v in range(n_vecs)))
    return np.stack(ins), np.stack(outs), s[0]


def n_coeffs_of(k):
    """the counts whose source vectors are 2^k long: the power itself and the non-powers 2^k - 1 and 2^(k-1) + 1"""
    return sorted({n for n in (1 << k, (1 << k) - 1, (1 << k >> 1) + 1) if n >= 1 and DC.ceil_log2(n) == k})


@functools.lru_cache(maxsize=None)
def extend_case(fid, nc, log_m, v):
    """(a random source vector of 2^ceil(log2 nc) elements, of which the mask must hide those from nc on; the natural values; the shift)"""
    k = DC.ceil_log2(nc)
    s = DC.shifts(fid, "k14x", nc, log_m)["random"]
    full = FC.random_vector(fid, k, "k14x", nc, v)
    return FC.mont(fid, full), tuple(DC.extend_fast(fid, list(full[:nc]), s, log_m)), s


@pytest.mark.parametrize("nl", [2, 4, 6, 8])
def test_launcher_refusals(nl):
    """what the launchers settle before any launch, on null or never-read buffers: no device is touched"""
    top = K12.max_log_tile()
    R, X = K14.coset_refusal, K14.extend_refusal
    assert R(3, 1, 4, top, 1) == INVALID and R(nl + 1, 1, 4, top, 1) == INVALID
    assert R(nl, -1, 4, top, 1) == INVALID and R(nl, 6, 4, top, 1) == INVALID
    assert R(nl, 1, 4, 0, 1) == INVALID and R(nl, 1, 4, top + 1, 1) == INVALID and R(nl, 1, 33, top, 1) == INVALID
    assert R(nl, 1, 4, top, 0) == INVALID and R(nl, 1, 4, top, 65536) == INVALID
    assert R(nl, 1, 32, top, 128) == INVALID and R(nl, 1, 24, top, 32768) == INVALID                  # 2^39 elements
    for form in range(6):
        for bit in range(4):
            assert R(nl, form, 4, top, 1, 1 << bit) == INVALID and R(nl, form, 4, top, 1, 0, 1 << bit) == INVALID, (form, bit)
        assert R(nl, form, 0, top, 1, 1) == INVALID and R(nl, form, 0, top, 1, 0, 2) == INVALID
        assert R(nl, form, 4, top, 1, overlap=1) == INVALID
    with pytest.raises(K14.BadArgs):
        R(nl, 1, 4, top, 1)                          # a job a correct launcher would launch is not for this entry point
    assert X(3, 4, 4, 0, top, 1) == INVALID and X(nl, 0, 4, 0, top, 1) == INVALID and X(nl, 17, 4, 0, top, 1) == INVALID
    assert X(nl, 4, 33, 0, top, 1) == INVALID and X(nl, 4, 4, 2, top, 1) == INVALID and X(nl, 4, 4, 0, 0, 1) == INVALID
    assert X(nl, 4, 4, 0, top + 1, 1) == INVALID and X(nl, 4, 4, 0, top, 0) == INVALID
    assert X(nl, 16, 20, 1, top, 1) == INVALID                                                         # 2^16 blocks
    assert X(nl, 1 << 20, 20, 1, top, 65536) == INVALID and X(nl, 3, 18, 1, top, 1) == INVALID
    assert X(nl, 1 << 30, 30, 0, top, 512) == INVALID                                                  # 2^39 elements
    for bit in range(4):
        assert X(nl, 5, 4, 1, top, 2, 1 << bit) == INVALID and X(nl, 5, 4, 1, top, 2, 0, 1 << bit) == INVALID, bit
    assert X(nl, 1, 0, 0, top, 1, 2) == INVALID and X(nl, 5, 4, 0, top, 1, overlap=1) == INVALID
    with pytest.raises(K14.BadArgs):
        X(nl, 5, 4, 0, top, 2)


@gpu
@pytest.mark.parametrize("shift", SHIFTS)
@pytest.mark.parametrize("log_tile", LOG_TILES)
@pytest.mark.parametrize("fid", FC.FIELDS)
def test_coset_every_form_every_size(fid, log_tile, shift):
    """one vector and three, out of place and in place: every element equals bignum, the canaries stand, an out-of-place input is
    unchanged, the launches are the plan's passes (one more for the forms that permute)"""
    lt = log_tile_of(log_tile)
    for log_n in LOG_NS:
        passes = len(K12.plan(log_n, lt))
        for form in FC.FORMS:
            for n_vecs in (1, 3):
                x, want, s = case(fid, form, log_n, n_vecs, shift)
                for in_place in (False, True):
                    got, launches = K14.run_coset(fid, form, log_n, lt, x, s, in_place=in_place)
                    assert np.array_equal(got, want), (form, log_n, n_vecs, in_place, np.argwhere((got != want).any(-1))[:8].tolist())
                    assert launches == passes + (1 if form[-2:] == "ii" and log_n else 0), (form, log_n, launches)


@gpu
@pytest.mark.parametrize("log_tile", LOG_TILES)
def test_coset_launches_are_k12s(log_tile):
    """the plain transform of the same form, size and tile, asked for its own count; and shift 1 gives its limbs"""
    fid, lt = 1, log_tile_of(log_tile)
    for log_n in LOG_NS:
        for form in FC.FORMS:
            x, _ = FC.io_of(form, *FC.pair(fid, log_n, "k14one"))
            plain, n12 = K12.run(fid, form, log_n, lt, FC.mont(fid, x))
            got, n14 = K14.run_coset(fid, form, log_n, lt, FC.mont(fid, x), 1)
            assert n14 == n12 and np.array_equal(got, plain), (form, log_n)


@gpu
@pytest.mark.parametrize("order", DC.ORDERS)
@pytest.mark.parametrize("log_tile", LOG_TILES)
@pytest.mark.parametrize("fid", FC.FIELDS)
def test_extend_every_size(fid, log_tile, order):
    lt = log_tile_of(log_tile)
    for k in range(0, 8):
        for nc in n_coeffs_of(k):
            for b in range(0, 5):
                log_m = k + b
                passes = len(K12.plan(k, lt))
                if k == 0 and log_m:
                    passes = 1                       # one coefficient over m > 1 values: the two-point plan
                for n_vecs in (1, 3):
                    cs, ys, s = zip(*(extend_case(fid, nc, log_m, v) for v in range(n_vecs)))
                    want = np.stack([FC.mont(fid, FC.permute(list(y), log_m) if order == "bitrev" else list(y)) for y in ys])
                    got, launches = K14.run_extend(fid, np.stack(cs), nc, log_m, order, lt, s[0])
                    assert np.array_equal(got, want), (nc, log_m, n_vecs, np.argwhere((got != want).any(-1))[:8].tolist())
                    assert launches == passes + (1 if order == "natural" and log_m else 0), (nc, log_m, launches)


@gpu
@pytest.mark.parametrize("fid", FC.FIELDS)
def test_worst_case_operands(fid):
    """every STORED limb pattern p - 1 with the shift p - 1, at a three-pass size, every form; and the extension of it"""
    import oracle_lib as O
    F = FC.field(fid)
    log_n = 9
    stored = np.tile(O.ints_to_limbs([F.p - 1], F.L), (1 << log_n, 1))
    x = FC.canon(fid, stored)
    for form in FC.FORMS:
        got, _ = K14.run_coset(fid, form, log_n, 3, stored, F.p - 1)
        assert np.array_equal(got[0], FC.mont(fid, DC.apply_form(fid, form, x, F.p - 1))), form
    got, _ = K14.run_extend(fid, stored, 1 << log_n, log_n + 2, "bitrev", 3, F.p - 1)
    assert np.array_equal(got[0], FC.mont(fid, DC.extend_fast(fid, x, F.p - 1, log_n + 2, "bitrev")))

"""K15 and K16, the inverse / pointwise and the domain-quotient kernels (kernels.h launch_batch_inverse, launch_pointwise,
launch_domain_quotient), directly against Python bignum (tests/quot_cases.py, held to the host forms by tests/test_quot_abi.py)
through tests/k15_harness.py.  Every stored element must equal bignum; there is no tolerance.

The sizes stand around the edges of the structure: one element, one wave's width, a workgroup's tile T (k15h_tile) less one, exactly
and plus one, and three tiles with a ragged fourth; the zeros of the operand sets stand at the first and last position of a lane's
chunk, of a tile and of the vector, and one set leaves a single nonzero element per tile.  K16 reads a twiddle table built by the
test, at one point, two, a wave, two waves, two tiles and 2^13."""
import functools

import numpy as np
import pytest

import fft_cases as FC
import k15_harness as K15
import quot_cases as QC

gpu = pytest.mark.gpu
INVALID = K15.HIP_ERROR_INVALID_VALUE


def sizes(fid):
    T = K15.tile(2 * FC.field(fid).L)
    return (1, 63, 64, 65, T - 1, T, T + 1, 3 * T + 17)


@functools.lru_cache(maxsize=None)
def inverse_case(fid, name, n):
    """(operand limbs, inverse limbs, canonical operands): computed once"""
    T = K15.tile(2 * FC.field(fid).L)
    x = QC.operands(fid, name, n, T, T // 8)
    return FC.mont(fid, x), FC.mont(fid, QC.inverse_ref(fid, x)), tuple(x)


def where(got, want):
    return np.argwhere((got != want).any(-1))[:8].tolist()


@pytest.mark.parametrize("nl", [2, 4, 6, 8])
def test_launcher_refusals(nl):
    """what the launchers settle before any launch, on null or never-read buffers: no device is touched"""
    P, Q = K15.pointwise_refusal, K15.quotient_refusal
    for op in ("inverse", "add", "sub", "mul", "div"):
        assert P(3, op, 8) == INVALID and P(nl + 1, op, 8) == INVALID                    # a bad nl
        assert P(nl, op, 0) == INVALID and P(nl, op, 1 << 39) == INVALID                 # n == 0, n >= 2^39
        for bit in ((1, 2) if op == "inverse" else (0, 1, 2)):
            assert P(nl, op, 8, 1 << bit) == INVALID and P(nl, op, 8, 0, 1 << bit) == INVALID, (op, bit)      # NULL, misaligned
        assert P(nl, op, 8, overlap=1) == INVALID
        with pytest.raises(K15.BadArgs):
            P(nl, op, 8)                             # a job a correct launcher would launch is not for this entry point
    assert P(nl, 4, 8) == INVALID and P(nl, -2, 8) == INVALID                            # an unknown op
    for kind in ("linear", "vanishing"):
        assert Q(3, kind, 4, 2, 1) == INVALID and Q(nl + 1, kind, 4, 2, 1) == INVALID
        assert Q(nl, kind, 33, 2, 1) == INVALID and Q(nl, kind, 4, 2, 0) == INVALID and Q(nl, kind, 4, 2, 65536) == INVALID
        assert Q(nl, kind, 32, 2, 128) == INVALID and Q(nl, kind, 24, 2, 32768) == INVALID          # 2^39 elements
        for bit in range(3):
            assert Q(nl, kind, 4, 2, 1, 1 << bit) == INVALID and Q(nl, kind, 4, 2, 1, 0, 1 << bit) == INVALID, (kind, bit)
        assert Q(nl, kind, 4, 2, 1, overlap=1) == INVALID
        with pytest.raises(K15.BadArgs):
            Q(nl, kind, 4, 2, 1)
    assert Q(nl, 2, 4, 2, 1) == INVALID
    assert Q(nl, "linear", 4, 0, 1, 8) == INVALID and Q(nl, "linear", 4, 0, 1, 0, 8) == INVALID and Q(nl, "linear", 4, 0, 1, 32) == INVALID   # y, z
    assert Q(nl, "vanishing", 4, 5, 1) == INVALID and Q(nl, "vanishing", 4, 2, 1, 16) == INVALID    # log_n > log_m, no shift^n
    with pytest.raises(K15.BadArgs):
        Q(nl, "linear", 0, 0, 1, 4)                  # one point: the table is not read


@gpu
@pytest.mark.parametrize("name", QC.SETS)
@pytest.mark.parametrize("fid", FC.FIELDS)
def test_inverse_every_size(fid, name):
    """out of place and in place: every element equals bignum, the canaries stand, an out-of-place input is unchanged"""
    for n in sizes(fid):
        x, want, _ = inverse_case(fid, name, n)
        for in_place in (0, 2):
            got = K15.run_pointwise(fid, "inverse", None, x, in_place)
            assert np.array_equal(got, want), (n, in_place, where(got, want))


@gpu
@pytest.mark.parametrize("fid", FC.FIELDS)
def test_pointwise_every_op(fid):
    """the four ops at every size, out of place, out == a and out == b; b carries zeros for DIV"""
    for n in sizes(fid):
        b, _, bc = inverse_case(fid, "edge_zeros" if n > 64 else "random", n)
        ac = QC.operands(fid, "random", n, 4096, 512, "a")
        a = FC.mont(fid, ac)
        for op in QC.OPS:
            want = FC.mont(fid, QC.pointwise_ref(fid, op, ac, bc))
            for in_place in (0, 1, 2):
                got = K15.run_pointwise(fid, op, a, b, in_place)
                assert np.array_equal(got, want), (n, op, in_place, where(got, want))


@gpu
@pytest.mark.parametrize("name", QC.SETS)
@pytest.mark.parametrize("fid", FC.FIELDS)
def test_div_every_operand_set(fid, name):
    """a / b with b from every operand set, at a tile plus one and at three tiles and a ragged fourth; zero where b is zero"""
    F = FC.field(fid)
    T = K15.tile(2 * F.L)
    for n in (T + 1, 3 * T + 17):
        b, binv, bc = inverse_case(fid, name, n)
        ac = QC.operands(fid, "random", n, 4096, 512, "a")
        want = FC.mont(fid, [u * v % F.p for u, v in zip(ac, FC.canon(fid, binv))])
        got = K15.run_pointwise(fid, "div", FC.mont(fid, ac), b)
        assert np.array_equal(got, want), (n, where(got, want))


@functools.lru_cache(maxsize=None)
def column(fid, log_m, v):
    return tuple(FC.random_vector(fid, log_m, "k16", v))


@gpu
@pytest.mark.parametrize("kind", ("linear", "vanishing"))
@pytest.mark.parametrize("fid", FC.FIELDS)
def test_domain_quotient(fid, kind):
    """one vector and three (with three different y), both orders, the generator and a random shift (and the NULL shift of the linear
    kind), out of place and in place"""
    F = FC.field(fid)
    log_t = K15.tile(2 * F.L).bit_length() - 1
    for log_m in sorted({0, 1, 6, 7, log_t + 1, 13}):
        sh = QC.coset_shifts(fid, log_m, "k16")
        big = log_m > 7
        for n_vecs in (1, 3):
            cols = [column(fid, log_m, v) for v in range(n_vecs)]
            vals = np.stack([FC.mont(fid, c) for c in cols])
            for order in QC.ORDERS:
                for name in (("random",) if big else ("gen", "random", None)):
                    if kind == "linear":
                        s = 1 if name is None else sh[name]
                        z = QC.off_domain(fid, s, log_m, "k16")
                        y = [FC.rng("k16y", fid, log_m, v).randrange(F.p) for v in range(n_vecs)]
                        want = np.stack([FC.mont(fid, QC.linear_ref(fid, c, s, z, y[v], order)) for v, c in enumerate(cols)])
                        run = lambda ip: K15.run_quotient(fid, kind, order, log_m, 0, vals, None if name is None else s, z, y, in_place=ip)
                        tag = (log_m, n_vecs, order, name)
                        got = run(False)
                        assert np.array_equal(got, want), (tag, where(got[0], want[0]))
                        if order == "natural":
                            assert np.array_equal(run(True), want), (tag, "in place")
                    elif name is not None:
                        for log_n in sorted({0, log_m // 2, log_m}) if not big else (log_m - 2,):
                            want = np.stack([FC.mont(fid, QC.vanishing_ref(fid, c, sh[name], log_n, order)) for c in cols])
                            got = K15.run_quotient(fid, kind, order, log_m, log_n, vals, sh[name])
                            assert np.array_equal(got, want), (log_m, log_n, n_vecs, order, name, where(got[0], want[0]))
                            if order == "bitrev":
                                got = K15.run_quotient(fid, kind, order, log_m, log_n, vals, sh[name], in_place=True)
                                assert np.array_equal(got, want), (log_m, log_n, n_vecs, order, name, "in place")


@gpu
def test_saturated_device():
    """2 x CUs x 8 tiles, each a copy of a tile that was checked against bignum: every workgroup of a full device, byte for byte"""
    fid = 3
    T = K15.tile(2 * FC.field(fid).L)
    x, want, _ = inverse_case(fid, "random", T)
    tiles = 2 * K15.cu_count() * 8
    assert tiles >= 16
    got = K15.run_pointwise(fid, "inverse", None, x)
    assert np.array_equal(got, want)
    got = K15.run_pointwise(fid, "inverse", None, np.tile(x, (tiles, 1)))
    assert got.tobytes() == np.tile(want, (tiles, 1)).tobytes()

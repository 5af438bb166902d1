"""K17, the scan kernels (kernels.h launch_scan), directly against Python bignum (tests/scan_cases.py, held to itself by
tests/test_k17_cases.py) through tests/k17_harness.py.  Every stored element and every total must equal bignum; there is no
tolerance.

With T a workgroup's tile (k17h_tile), C the consecutive elements of a lane (k17h_lane_elems) and M the totals K17b takes per level
(k17h_mid_chunk), the sizes stand at the edges of the structure -- a lane's chunk, a wave (64 lanes, 64 C elements), a tile, two tiles
and a ragged third: the smallest sizes at which each carry can go wrong.  Three vectors of T + 5 elements start off the tile grid, each
with its own init.  K17b runs alone on 1, M - 1, M, M + 1 and 2 M + 3 synthetic totals.  The canaries around the output, the totals
and the workspace and an out-of-place input are checked by the harness at every call."""
import functools

import numpy as np
import pytest

import fft_cases as FC
import k17_harness as K17
import scan_cases as SC

gpu = pytest.mark.gpu
INVALID = K17.HIP_ERROR_INVALID_VALUE


def geometry(fid):
    nl = 2 * FC.field(fid).L
    return K17.tile(nl), K17.lane_elems(nl), K17.mid_chunk(nl)


def sizes(fid):
    T, c, _ = geometry(fid)
    return (1, 2, c - 1, c, c + 1, 63, 64, 65, 64 * c - 1, 64 * c + 1, T - 1, T, T + 1, 2 * T + 17)


@functools.lru_cache(maxsize=None)
def case(fid, name, n, *key):
    """(operand limbs, canonical operands): computed once"""
    T, c, _ = geometry(fid)
    x = SC.operands(fid, name, n, T, c, *key)
    return FC.mont(fid, x), tuple(x)


@functools.lru_cache(maxsize=None)
def reference(fid, name, n, op, mode, init, *key):
    """(output limbs, total limbs) of the bignum scan: computed once"""
    out, total = SC.scan_ref(fid, op, mode, case(fid, name, n, *key)[1], init)
    return FC.mont(fid, out), FC.mont(fid, [total])


def seed(fid, *key):
    return FC.rng("k17-init", fid, *key).randrange(1, FC.field(fid).p)


def where(got, want):
    return np.argwhere((got != want).any(-1))[:8].tolist()


@pytest.mark.parametrize("nl", [2, 4, 6, 8])
def test_launcher_refusals(nl):
    """what the launcher settles before any launch, on null or never-read buffers: no device is touched"""
    R = K17.scan_refusal
    for op in SC.OPS:
        for mode in SC.MODES:
            assert R(3, op, mode, 8) == INVALID and R(nl + 1, op, mode, 8) == INVALID                        # a bad nl
            assert R(nl, op, mode, 0) == INVALID and R(nl, op, mode, 1 << 39) == INVALID                      # n == 0, n >= 2^39
            assert R(nl, op, mode, 8, 0) == INVALID and R(nl, op, mode, 8, 65536) == INVALID                  # n_vecs
            assert R(nl, op, mode, 1 << 36) == INVALID and R(nl, op, mode, K17.tile(nl) << 24) == INVALID     # 2^24 tiles: the grid
            assert R(nl, op, mode, 1 << 38, 2) == INVALID and R(nl, op, mode, 1 << 24, 32768) == INVALID      # 2^39 elements
            for bit in (0, 1, 2, 5):
                assert R(nl, op, mode, 8, 1, 1 << bit) == INVALID, (op, mode, bit)                           # NULL
            for bit in range(5):
                assert R(nl, op, mode, 8, 1, 0, 1 << bit) == INVALID, (op, mode, bit)                        # misaligned
            for overlap in range(1, 6):
                assert R(nl, op, mode, 8, 3, overlap=overlap) == INVALID, (op, mode, overlap)
            for n in (8, K17.tile(nl) + 1, K17.tile(nl) * K17.mid_chunk(nl) + 1):
                assert R(nl, op, mode, n, 2, short_work=1) == INVALID, (op, mode, n)
            with pytest.raises(K17.BadArgs):
                R(nl, op, mode, 8)                   # a job a correct launcher would launch is not for this entry point
            with pytest.raises(K17.BadArgs):
                R(nl, op, mode, 8, 1, 24)            # init and total may be NULL
    assert R(nl, 2, 0, 8) == INVALID and R(nl, -1, 0, 8) == INVALID and R(nl, 0, 2, 8) == INVALID and R(nl, 0, -1, 8) == INVALID


@gpu
@pytest.mark.parametrize("op", SC.OPS)
@pytest.mark.parametrize("fid", FC.FIELDS)
def test_every_size(fid, op):
    """one vector at every edge, both modes, with and without init, out of place and in place; the launches are one for a tile and
    three beyond"""
    T = geometry(fid)[0]
    for n in sizes(fid):
        x, _ = case(fid, "nonzero", n)
        for mode in SC.MODES:
            for init in (None, seed(fid, n)):
                want, wtot = reference(fid, "nonzero", n, op, mode, init)
                for in_place in (False, True):
                    got, tot, launches = K17.run_scan(fid, op, mode, x, None if init is None else FC.mont(fid, [init]), in_place)
                    tag = (n, mode, init is not None, in_place)
                    assert np.array_equal(got, want), (tag, where(got, want))
                    assert np.array_equal(tot, wtot), tag
                    assert launches == (1 if n <= T else 3), tag


@gpu
@pytest.mark.parametrize("fid", FC.FIELDS)
def test_three_vectors_off_the_tile_grid(fid):
    """n = T + 5: the second and third vector start inside a tile's stride, and a carry that leaked from one vector into the next would
    show; every vector has its own init and its own total"""
    T = geometry(fid)[0]
    n = T + 5
    x = np.stack([case(fid, "nonzero", n, v)[0] for v in range(3)])
    inits = [seed(fid, "vec", v) for v in range(3)]
    for op in SC.OPS:
        for mode in SC.MODES:
            refs = [reference(fid, "nonzero", n, op, mode, inits[v], v) for v in range(3)]
            want, wtot = np.stack([r[0] for r in refs]), np.concatenate([r[1] for r in refs])
            for in_place in (False, True):
                got, tot, _ = K17.run_scan(fid, op, mode, x, FC.mont(fid, inits), in_place)
                assert np.array_equal(got, want), (op, mode, in_place, where(got.reshape(-1, got.shape[-1]), want.reshape(-1, want.shape[-1])))
                assert np.array_equal(tot, wtot), (op, mode, in_place)
            refs = [reference(fid, "nonzero", n, op, mode, None, v) for v in range(3)]
            got, tot, _ = K17.run_scan(fid, op, mode, x)
            assert np.array_equal(got, np.stack([r[0] for r in refs])) and np.array_equal(tot, np.concatenate([r[1] for r in refs])), (op, mode, "no init")


@gpu
@pytest.mark.parametrize("op", SC.OPS)
@pytest.mark.parametrize("fid", FC.FIELDS)
def test_totals_scan_alone(fid, op):
    """K17b on synthetic tile totals, one vector and three: their exclusive scan in place, seeded with init, and the vectors' totals --
    at M + 1 and 2 M + 3 totals it goes one level down, which the whole scan reaches only beyond M T elements"""
    M = geometry(fid)[2]
    for n in (1, M - 1, M, M + 1, 2 * M + 3):
        for n_vecs in (1, 3):
            x = np.stack([case(fid, "nonzero", n, "totals", v)[0] for v in range(n_vecs)])
            inits = [seed(fid, "totals", v) for v in range(n_vecs)]
            refs = [reference(fid, "nonzero", n, op, "exclusive", inits[v], "totals", v) for v in range(n_vecs)]
            got, tot, _ = K17.run_scan(fid, op, "exclusive", x, FC.mont(fid, inits), totals_only=True)
            want = np.stack([r[0] for r in refs])
            assert np.array_equal(got, want), (n, n_vecs, where(got.reshape(-1, got.shape[-1]), want.reshape(-1, want.shape[-1])))
            assert np.array_equal(tot, np.concatenate([r[1] for r in refs])), (n, n_vecs)


@gpu
@pytest.mark.parametrize("name", SC.SETS)
@pytest.mark.parametrize("fid", FC.FIELDS)
def test_every_operand_set(fid, name):
    """two tiles and a ragged third: the single zero of the edge sets turns a product to zero from exactly its place on, sums wrap at
    every step or walk around zero"""
    T = geometry(fid)[0]
    n = 2 * T + 17
    x, _ = case(fid, name, n)
    for op in SC.OPS:
        for mode in SC.MODES:
            want, wtot = reference(fid, name, n, op, mode, None)
            got, tot, _ = K17.run_scan(fid, op, mode, x)
            assert np.array_equal(got, want), (op, mode, where(got, want))
            assert np.array_equal(tot, wtot), (op, mode)
    if name in SC.EDGES:
        at = SC.edge_position(name, n, T, geometry(fid)[1])
        got = K17.run_scan(fid, "product", "inclusive", x)[0]
        assert got[:at].any(-1).all() and not got[at:].any()


@gpu
def test_saturated_device():
    """2 x CUs x 4 tiles of one vector, against the host form (held to bignum by tests/test_scan_abi.py): every workgroup of a full
    device, and a totals array longer than the device is wide"""
    fid = 3
    T = geometry(fid)[0]
    tiles = 2 * K17.lib().k17h_cu_count() * 4
    assert tiles >= 16
    x, _ = case(fid, "nonzero", T)
    big = np.tile(x, (tiles, 1))
    for op in SC.OPS:
        want, wtot = SC.host_scan(fid, op, "exclusive", big)
        got, tot, launches = K17.run_scan(fid, op, "exclusive", big)
        assert got.tobytes() == want.tobytes() and np.array_equal(tot[0], wtot) and launches == 3

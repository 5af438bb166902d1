"""The case builders of tests/k5_harness.py against the field arithmetic of oracle/pyref.py, their array layouts, the harness's own
argument checks, the launchers' refusals (lcpc_amd/csrc/kernels.h: what K5 / K6 settle before any launch), the separation of
lib/liblcpc_k5_harness.so from the product -- and that the batched cases of tests/test_gpu_k5_kernels.py can see the faults they are
there to catch.  No GPU."""
import random

import numpy as np
import pytest

import k5_harness as H
import pyref as P
from common import to_int, to_limbs
from test_abi import _harness_is_a_separate_library

FIELDS = [0, 1, 2, 3]
OK, INVALID = H.HIP_SUCCESS, H.HIP_ERROR_INVALID_VALUE


def test_k5_harness_is_a_separate_library():
    """lib/liblcpc_k5_harness.so (tests/native/k5_harness.cpp) exports the k5h_* entry points of tests/k5_harness.py and nothing of the
    product, which it links against instead of carrying a copy"""
    _harness_is_a_separate_library("k5_harness", "k5h_", "tests/native/k5_harness.cpp", "K5H_OUT")


def test_pack_is_to_limbs():
    rng = random.Random(1)
    for L in (1, 2, 3, 4):
        vals = [0, 1, (1 << (64 * L)) - 1] + [rng.getrandbits(64 * L) for _ in range(20)]
        assert np.array_equal(H.pack(vals, L), to_limbs(vals, L))
    assert H.pack([], 3).shape == (0, 3)


# ---- expectations against pyref -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fid", FIELDS)
def test_collapse_expectation_is_the_field_dot_product(fid):
    """CollapseData.dots is the stored form of sum_r tensor[r] * coeffs[r][j] over the field, by canonical arithmetic; a case's expected
    array holds it at ((member * n_splits + split) * n_tensors + tensor) * out_stride + (j - j0), zeros for a split with no row, and
    SENTINEL everywhere else"""
    F = P.FIELDS[fid]
    d = H.CollapseData(fid, 5, 11, n_members=3, seed=2)
    c = H.CollapseCase(d, 2, 4, n_batch=3, j0=2, j1=9, out_stride=8)
    assert c.splits() == [(0, 2), (2, 4), (4, 5), (5, 5)]            # ceil(5 / 4) = 2 rows per split: the last holds none
    e = c.expected()
    assert e.shape == (3 * 4 * 2 * 8 + 5, d.L)
    seen = np.zeros(len(e), bool)
    for m in range(3):
        for z, (r0, r1) in enumerate(c.splits()):
            for t in range(2):
                at = ((m * 4 + z) * 2 + t) * 8
                for j in range(2, 9):
                    want = sum(F.from_mont(d.tensors[m][t][r]) * F.from_mont(d.coeffs[m][r][j]) for r in range(r0, r1)) % F.p
                    assert F.from_mont(to_int(e[at + j - 2])) == want
                    seen[at + j - 2] = True
                if z == 3:
                    assert not e[at:at + 7].any()
    assert (e[~seen] == np.uint64(H.SENTINEL)).all() and (~seen).sum() == 3 * 4 * 2 + 5
    # the launcher's defaults: the whole row at the row stride
    w = H.CollapseCase(d, 1, 1, n_batch=3)
    assert (w.ej0, w.ej1, w.es, w.len) == (0, 11, 11, 11) and w.limb == (fid == 3)


@pytest.mark.parametrize("fid", FIELDS)
def test_collapse_layout(fid):
    """members at the offsets the descriptors say, in an order unlike the batch order, poison in every gap; operands hold the extremes"""
    from common import field_p, maxc, maxt
    d = H.CollapseData(fid, 9, 4, n_members=3, seed=3)
    c = H.CollapseCase(d, 2, 1, n_batch=3)
    coeffs, off, tensors = c.arrays()
    assert off.tolist() == [H.GAP + q * (36 + H.GAP) for q in (1, 0, 2)] and c.pos == [1, 0, 2]
    member = np.zeros(len(coeffs), bool)
    for m in range(3):
        o = int(off[m])
        member[o:o + 36] = True
        assert [to_int(x) for x in coeffs[o:o + 36]] == [v for row in d.coeffs[m] for v in row]
        assert [[to_int(x) for x in tensors[m, t]] for t in range(2)] == d.tensors[m]
    assert (coeffs[~member] == np.uint64(H.POISON)).all() and (~member).sum() == 4 * H.GAP
    flat = {v for m in range(3) for row in d.coeffs[m] for v in row}
    assert {maxc(fid), field_p(fid) - 1} < flat
    assert {maxt(fid), field_p(fid) - 1} < {v for m in range(3) for t in range(2) for v in d.tensors[m][t]}
    one = H.CollapseCase(H.CollapseData(fid, 9, 4), 1, 1)
    assert not one.batch and one.off == [H.GAP]


def test_collapse_shapes_cross_the_cadences():
    """rows per split 7, 8, 9 for every field and 6, 7, 60, 61, 121 for Ft255 (tests/test_lazy_bounds.py: the reduce-every-8 and the
    normalise-every-6 / reduce-every-60 cadences), under 1, 2 and 3 splits; 64 splits of 61 rows: one row each and three with none"""
    for fid in FIELDS:
        per = {-(-r // s) for ns in (1, 2, 3) for r, s in H.collapse_single_shapes(fid, ns)}
        assert {7, 8, 9} <= per and (fid != 3 or {6, 7, 60, 61, 121} <= per)
        assert H.collapse_single_shapes(fid, 64) == [(61, 64)]
        b = H.collapse_batch_shapes(fid)
        assert {nb for _, _, nb in b} == {1, 3, 5} and {ns for _, ns, _ in b} == {1, 2, 3, 64}
        assert fid != 3 or {6, 60, 61, 121} <= {-(-r // s) for r, s, _ in b}
    c = H.CollapseCase(H.CollapseData(0, 61, 2), 1, 64)
    assert [r1 - r0 for r0, r1 in c.splits()] == [1] * 61 + [0] * 3
    views = H.collapse_views(H.CollapseData(3, 7, H.N_PER_ROW), 1)
    assert {(v.n_tensors, v.ej0, v.ej1, v.es, v.limb) for v in views} == {
        (nt, j0, j1, es, limb) for nt in (1, 2) for j0, j1, es in ((0, 300, 300), (37, 293, 300), (37, 293, 256)) for limb in (True, False)}
    assert {(v.j0, v.j1, v.out_stride) for v in views} == set(H.RANGES)


def test_r29_expectation():
    """nine 29-bit limbs of 32 t mod p (the stored t R times 2^5: t 2^261), words 9 to 11 zero"""
    F = P.FIELDS[3]
    rng = random.Random(4)
    vals = [0, 1, F.p - 1] + [rng.randrange(F.p) for _ in range(10)]
    e = H.r29_expected(vals, len(vals) + 2)
    for i, t in enumerate(vals):
        x = sum(int(w) << (29 * k) for k, w in enumerate(e[i, :9]))
        assert x < F.p and x == F.from_mont(t) * (1 << 261) % F.p and not e[i, 9:].any() and (e[i, :9] < (1 << 29)).all()
    assert (e[len(vals):] == H.SENTINEL & 0xFFFFFFFF).all()


@pytest.mark.parametrize("fid", FIELDS)
def test_convert_and_sum_expectations(fid):
    F = P.FIELDS[fid]
    rng = random.Random(5)
    vals = [0, 1, F.p - 1, H.mont_r(fid) % F.p] + [rng.randrange(F.p) for _ in range(10)]
    canon = H.convert_expected(fid, vals, False)
    mont = H.convert_expected(fid, vals, True)
    for i, v in enumerate(vals):
        assert to_int(canon[i]) == F.from_mont(v) and F.from_mont(to_int(mont[i])) == v
    assert (canon[len(vals):] == np.uint64(H.SENTINEL)).all() and len(canon) == len(vals) + 3
    assert to_int(H.r2_limbs(fid)[0]) == F.to_mont(H.mont_r(fid) % F.p)
    s = H.SumCase(fid, 3, 5, n_batch=3, fill="max", seed=6)
    buf, e = s.buffer(), s.expected()
    assert buf.shape == (3 * 3 * 5 + 3 * 5 + 4, s.L) and np.array_equal(buf[:45], e[:45]) and (buf[45:] == np.uint64(H.SENTINEL)).all()
    for m in range(3):
        for q in range(3):
            assert [to_int(x) for x in buf[(m * 3 + q) * 5:(m * 3 + q + 1) * 5]] == s.parts[m][q]
            assert (q == m % 3) or s.parts[m][q] == [F.p - 1] * 5
        for i in range(5):
            assert F.from_mont(to_int(e[45 + m * 5 + i])) == sum(F.from_mont(s.parts[m][q][i]) for q in range(3)) % F.p
    assert (e[60:] == np.uint64(H.SENTINEL)).all()
    assert H.SumCase(fid, 2, 3, fill="max").parts == [[[F.p - 1] * 3] * 2]


@pytest.mark.parametrize("fid", FIELDS)
def test_gather_layout_and_expectation(fid):
    """row-major and position-major members at their offsets with poison between them; a canonical member's values come out times R"""
    F = P.FIELDS[fid]
    cols = [[0, 3, 3], [2, 0, 1], [3, 3, 0]]
    g = H.GatherCase(fid, 5, 4, cols, ["row", "pos", "row"], [False, True, True], seed=7)
    comm, off, rs, cs, canon, c = g.arrays()
    assert rs.tolist() == [4, 1, 4] and cs.tolist() == [1, 5, 1] and canon.tolist() == [0, 1, 1] and c.tolist() == cols
    assert off.tolist() == [H.GAP + q * (20 + H.GAP) for q in (1, 0, 2)]
    member = np.zeros(len(comm), bool)
    e = g.expected()
    for m in range(3):
        o = int(off[m])
        member[o:o + 20] = True
        for r in range(5):
            for col in range(4):
                assert to_int(comm[o + r * int(rs[m]) + col * int(cs[m])]) == g.comm[m][r][col]
        for k in range(3):
            for r in range(5):
                got = to_int(e[(m * 3 + k) * 5 + r])
                x = g.comm[m][r][cols[m][k]]
                assert got == (F.to_mont(x) if g.canon[m] else x)
    assert (comm[~member] == np.uint64(H.POISON)).all() and (e[45:] == np.uint64(H.SENTINEL)).all() and len(e) == 45 + 4
    lst = H.col_list(H.SLICE + 3, 7, 1)
    assert {0, 6} <= set(lst[:7]) and len(set(lst[:7])) < 7 and all(lst[k] != lst[k - H.SLICE] for k in range(H.SLICE, H.SLICE + 3))
    assert H.col_list(7, 6, 0) != H.col_list(7, 6, 1)


@pytest.mark.parametrize("dw", [8, 16])
def test_paths_layout_and_expectation(dw):
    p = H.PathsCase(dw, 8, 3, [[0, 7, 5], [6, 1, 2]], seed=8)
    h, off, cols = p.arrays()
    assert off.tolist() == [H.GAP + 15 + H.GAP, H.GAP] and h.shape == (2 * (15 + H.GAP) + H.GAP, dw)
    for m in range(2):
        assert np.array_equal(h[int(off[m]):int(off[m]) + 15], p.hashes[m])
    assert (h[:H.GAP] == 0xFFFFFFFF).all() and (h[H.GAP + 15:2 * H.GAP + 15] == 0xFFFFFFFF).all() and (h[-H.GAP:] == 0xFFFFFFFF).all()
    e = p.expected()
    # column 5 of member 0: sibling leaf 4, then node 8 + (2 ^ 1) = 11, then node 12 + (1 ^ 1) = 12
    assert [e[2 * 3 + lvl].tolist() for lvl in range(3)] == [p.hashes[0][i].tolist() for i in (4, 11, 12)]
    assert [e[(3 + 1) * 3 + lvl].tolist() for lvl in range(3)] == [p.hashes[1][i].tolist() for i in (0, 9, 13)]
    assert (e[18:] == H.SENTINEL & 0xFFFFFFFF).all() and len(e) == 20


@pytest.mark.parametrize("fid", FIELDS)
def test_assemble_layout_and_expectation(fid):
    a = H.AssembleCase(fid, [0, 0, 3, 3, 4], 2, slack=6, seed=9)
    recv = a.recv()
    assert (a.G, a.n_rows, a.block_words) == (4, 4, 2 * 3 * 2 * a.L + 6) and recv.shape == (4, a.block_words // 2)
    assert (recv[0] == np.uint64(H.POISON)).all() and (recv[2] == np.uint64(H.POISON)).all()
    assert (recv[1, 6 * a.L:] == np.uint64(H.POISON)).all() and (recv[3, 2 * a.L:] == np.uint64(H.POISON)).all()
    e = a.expected()
    for k in range(2):
        assert [to_int(x) for x in e[k * 4:k * 4 + 4]] == a.data[1][k] + a.data[3][k]
        assert [to_int(x) for x in recv[1, :6 * a.L].reshape(-1, a.L)[k * 3:k * 3 + 3]] == a.data[1][k]
    assert (e[8:] == np.uint64(H.SENTINEL)).all() and len(e) == 11


# ---- the batched cases can see what they are there to catch ---------------------------------------------------------------------------------
def _changes(case, fault):
    return not np.array_equal(case.expected(), case.expected(fault))


@pytest.mark.parametrize("fid", FIELDS)
def test_collapse_batches_see_a_swapped_member_and_a_dropped_j0(fid):
    """every batch-form collapse launch of tests/test_gpu_k5_kernels.py: with two members or more, exchanging the coefficients of
    members 0 and 1 changes the expectation; with j0 > 0, reading column j - j0 instead of j does"""
    n = 0
    for n_rows, n_splits, n_batch in H.collapse_batch_shapes(fid):
        d = H.CollapseData(fid, n_rows, H.N_PER_ROW, n_batch, seed=n_rows)
        for v in H.collapse_views(d, n_splits, n_batch):
            if v.limb != (fid == 3):
                continue                      # the expectation does not depend on the limb form
            if n_batch > 1:
                assert _changes(v, "swap"), (n_rows, n_splits, n_batch)
            if v.ej0:
                assert _changes(v, "no_j0"), (n_rows, n_splits, n_batch)
                n += 1
    assert n


@pytest.mark.parametrize("fid", FIELDS)
def test_gather_and_sum_batches_see_a_swapped_member_and_a_dropped_slice(fid):
    n_slice = 0
    for name, make in H.gather_batch_cases(fid).items():
        c = make()
        if c.n_batch > 1:
            assert _changes(c, "swap"), name
        if c.n_open > H.SLICE:
            assert _changes(c, "no_slice"), name
            n_slice += 1
    assert n_slice == 1
    for n_batch in (3, 7):
        for fill in ("max", "random"):
            assert _changes(H.SumCase(fid, 3, 5, n_batch, fill), "swap")


@pytest.mark.parametrize("dw", [8, 16])
def test_paths_batches_see_a_swapped_member(dw):
    n = 0
    for name, make in H.paths_batch_cases(dw).items():
        c = make()
        if c.n_batch > 1 and c.path_len:        # (np2 = 2 at the depth minus 1 has no path entry to get wrong)
            assert _changes(c, "swap"), name
            n += 1
    assert n == 10


# ---- the harness's own checks -----------------------------------------------------------------------------------------------------------------
def test_harness_refuses_what_it_cannot_bound():
    """tests/native/k5_harness.cpp checks its arguments before it touches the device: no GPU is needed to refuse"""
    L = H.lib()
    a = np.zeros((64, 4), np.uint64)
    off = np.zeros(4, np.uint64)
    one = np.ones(4, np.uint64)
    flag = np.zeros(4, np.uint32)
    P_ = H._ptr

    def collapse(**kw):
        k = dict(nl=2, ce=64, n_rows=2, npr=8, nt=1, ns=1, j0=0, j1=0, st=0, oe=64, nb=1, bf=0, limb=0, off=off)
        k.update(kw)
        return L.k5h_collapse(k["nl"], P_(a), k["ce"], P_(k["off"]), P_(a), P_(a), k["oe"], k["n_rows"], k["npr"], k["nt"], k["ns"], k["j0"], k["j1"],
                              k["st"], k["nb"], k["bf"], k["limb"])
    far = np.array([49, 0, 0, 0], np.uint64)
    for bad in (dict(nl=3), dict(nt=0), dict(nt=3), dict(ns=0), dict(ns=65536), dict(n_rows=0), dict(npr=0), dict(j1=9), dict(j0=4, j1=4),
                dict(j0=1, j1=8, st=6), dict(ce=15), dict(off=far), dict(oe=7), dict(ns=9), dict(nb=2), dict(nb=0, bf=1), dict(nb=65536, bf=1),
                dict(limb=1), dict(ce=(1 << 24) + 1), dict(n_rows=1 << 20, npr=1 << 20)):
        assert collapse(**bad) == -1, bad
    assert L.k5h_to_r29(P_(a), 0, P_(a), 4) == -1 and L.k5h_to_r29(P_(a), 5, P_(a), 4) == -1
    for args in ((3, 64, 1, 4, 1, 0), (2, 64, 0, 4, 1, 0), (2, 64, 1, 0, 1, 0), (2, 7, 1, 4, 1, 0), (2, 64, 1, 4, 2, 0), (2, 64, 1, 4, 0, 1),
                 (2, 64, 16, 4, 1, 0), (2, 64, 8, 4, 2, 1)):
        assert L.k5h_field_sum(args[0], P_(a), *args[1:]) == -1, args
    for args in ((3, 0, 4, 4, 0), (2, 0, 0, 4, 0), (2, 0, 5, 4, 0), (2, 1, 4, 4, 0), (2, 0, 4, (1 << 24) + 1, 0)):
        nl, to_mont, n, oe, inplace = args
        assert L.k5h_convert(nl, to_mont, P_(a), n, None, P_(a), oe, inplace) == -1, args
    assert L.k5h_convert(2, 0, None, 4, None, P_(a), 4, 0) == -1

    def gather(**kw):
        k = dict(nl=2, ce=64, off=off, rs=one * 8, cs=one, canon=flag, n_rows=8, n_cols=8, cols=off, n_open=2, r2=None, ve=64, nb=1, bf=0)
        k.update(kw)
        return L.k5h_gather_columns(k["nl"], P_(a), k["ce"], P_(k["off"]), P_(k["rs"]), P_(k["cs"]), P_(k["canon"]), k["n_rows"], k["n_cols"],
                                    P_(k["cols"]), k["n_open"], P_(k["r2"]), P_(a), k["ve"], k["nb"], k["bf"])
    for bad in (dict(nl=5), dict(n_rows=0), dict(n_cols=0), dict(n_open=0), dict(ce=63), dict(off=one), dict(rs=one * 9), dict(cs=one * 2),
                dict(canon=np.ones(4, np.uint32)), dict(cols=one * 8), dict(ve=15), dict(nb=2), dict(nb=0, bf=1), dict(n_rows=9)):
        assert gather(**bad) == -1, bad

    def paths(**kw):
        k = dict(hd=64, off=off, np2=8, pl=3, cols=off, n_open=2, pd=64, dw=8, nb=1, bf=0)
        k.update(kw)
        return L.k5h_gather_paths(P_(a), k["hd"], P_(k["off"]), k["np2"], k["pl"], P_(k["cols"]), k["n_open"], P_(a), k["pd"], k["dw"], k["nb"], k["bf"])
    for bad in (dict(dw=4), dict(dw=12), dict(np2=1), dict(np2=6), dict(pl=4), dict(hd=14), dict(off=one * 50), dict(cols=one * 8), dict(pd=5),
                dict(n_open=0), dict(nb=3), dict(nb=0, bf=1)):
        assert paths(**bad) == -1, bad

    def assemble(**kw):
        k = dict(nl=2, bw=16, rb=np.array([0, 2, 4], np.uint64), G=2, n=2, n_rows=4, oe=8)
        k.update(kw)
        return L.k5h_assemble_columns(k["nl"], P_(a), k["bw"], P_(k["rb"]), k["G"], k["n"], k["n_rows"], P_(a), k["oe"])
    for bad in (dict(nl=7), dict(G=0), dict(n=0), dict(n_rows=0), dict(bw=15), dict(bw=6), dict(oe=7), dict(rb=np.array([1, 2, 4], np.uint64)),
                dict(rb=np.array([0, 3, 2], np.uint64)), dict(rb=np.array([0, 2, 3], np.uint64)), dict(rb=np.array([0, 5, 4], np.uint64))):
        assert assemble(**bad) == -1, bad
    # jobs a correct launcher would launch are not for the refusal entry points
    for f, args in ((H.refuse_collapse, (2,)), (H.refuse_field_sum, (2, 1, 1)), (H.refuse_gather_columns, (2, 1, 1)),
                    (H.refuse_gather_paths, (8, 1, 1)), (H.refuse_convert, (2, "canon", 1)), (H.refuse_convert, (2, "r29", 1)),
                    (H.refuse_assemble_columns, (2, 1, 1))):
        with pytest.raises(H.BadArgs):
            f(*args)


# ---- what the launchers settle before any launch (kernels.h) ----------------------------------------------------------------------------------
@pytest.mark.parametrize("nl", [2, 4, 6, 8])
def test_collapse_refusals(nl):
    for batch in (None, 3):
        assert H.refuse_collapse(nl, n_splits=0, n_batch=batch) == INVALID            # a zero grid y
        assert H.refuse_collapse(nl, n_splits=65536, n_batch=batch) == INVALID
        assert H.refuse_collapse(nl, n_tensors=0, n_batch=batch) == INVALID
        assert H.refuse_collapse(nl, n_tensors=3, n_batch=batch) == INVALID
        assert H.refuse_collapse(nl, j0=0, j1=301, n_batch=batch) == INVALID          # j1 > n_per_row
        assert H.refuse_collapse(nl, j0=37, j1=37, n_batch=batch) == INVALID          # j0 >= j1
        assert H.refuse_collapse(nl, j0=38, j1=37, n_batch=batch) == INVALID
        assert H.refuse_collapse(nl, n_per_row=0, n_batch=batch) == INVALID           # the default range of an empty row
    assert H.refuse_collapse(nl, n_batch=0) == INVALID                                # members without a member
    assert H.refuse_collapse(nl, n_batch=65536) == INVALID                            # more members than grid z
    if nl == 8:
        assert H.refuse_collapse(nl, n_splits=0, limb=True) == INVALID
        assert H.refuse_collapse(nl, n_tensors=3, limb=True) == INVALID
        assert H.refuse_collapse(nl, n_tensors=3, n_batch=2, limb=True) == INVALID


@pytest.mark.parametrize("nl", [2, 4, 6, 8])
def test_split_sum_and_conversion_refusals(nl):
    for batch in (None, 3):
        assert H.refuse_field_sum(nl, 4, 0, n_batch=batch) == OK                      # nothing to add: no launch
        assert H.refuse_field_sum(nl, 0, 0, n_batch=batch) == OK
        assert H.refuse_field_sum(nl, 0, 300, n_batch=batch) == INVALID               # the kernel starts from parts[0]
    assert H.refuse_field_sum(nl, 4, 300, n_batch=0) == OK
    assert H.refuse_field_sum(nl, 4, 300, n_batch=65536) == INVALID
    for which in ("canon", "mont", "r29"):
        assert H.refuse_convert(nl, which, 0) == OK


@pytest.mark.parametrize("nl", [2, 4, 6, 8])
def test_gather_refusals(nl):
    for batch in (None, 3):
        assert H.refuse_gather_columns(nl, 0, 5, n_batch=batch) == OK                 # no row: a zero grid x
        assert H.refuse_gather_columns(nl, 7, 0, n_batch=batch) == OK                 # no opened column
    assert H.refuse_gather_columns(nl, 7, 5, n_batch=0) == OK
    assert H.refuse_gather_columns(nl, 7, 5, n_batch=65536) == INVALID
    assert H.refuse_assemble_columns(nl, 0, 7) == OK and H.refuse_assemble_columns(nl, 3, 0) == OK


def test_bad_limb_counts_and_digest_sizes_are_refused():
    for nl in (0, 1, 3, 5, 7, 10, -2):
        assert H.refuse_collapse(nl) == INVALID and H.refuse_collapse(nl, n_batch=2) == INVALID
        assert H.refuse_field_sum(nl, 4, 300) == INVALID and H.refuse_field_sum(nl, 4, 300, n_batch=2) == INVALID
        assert H.refuse_gather_columns(nl, 7, 5) == INVALID and H.refuse_gather_columns(nl, 7, 5, n_batch=2) == INVALID
        assert H.refuse_convert(nl, "canon", 9) == INVALID and H.refuse_convert(nl, "mont", 9) == INVALID
        assert H.refuse_assemble_columns(nl, 3, 7) == INVALID
    for dw in (0, 4, 12, 32):
        for batch in (None, 2):
            assert H.refuse_gather_paths(dw, 3, 5, n_batch=batch) == INVALID
            assert H.refuse_gather_paths(dw, 0, 0, n_batch=batch) == INVALID          # whatever else is asked
    for dw in (8, 16):
        for batch in (None, 2):
            assert H.refuse_gather_paths(dw, 0, 5, n_batch=batch) == OK
            assert H.refuse_gather_paths(dw, 3, 0, n_batch=batch) == OK
        assert H.refuse_gather_paths(dw, 3, 5, n_batch=0) == OK

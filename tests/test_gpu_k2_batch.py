"""The batch forms of the position-major Brakedown kernels (kernels.hip K2b: lane = batch row R = member * n_rows + row) called directly
(tests/k2b_harness.py over tests/native/k2b_harness.cpp).

The reference is the ONE-SHOT launcher of each kernel run once per member through tests/k2_harness.py: tests/test_gpu_k2_kernels.py pins
those to Python-int arithmetic, and they are not the code under test.  The matrices and operands are the builders' of
tests/test_k2_cases.py -- term counts on every normalise / REDC-chunk / slice boundary, operands at their largest limbs -- with one
operand table built for n_batch * n_rows rows, so that member i's rows follow other patterns than member 0's and no two rows of the
batch are equal: a member mix-up cannot cancel.  Every member sits at a stride larger than its extent with a sentinel behind it; whole
buffers are compared, so whatever a kernel writes outside a member's outputs shows.  Exact arithmetic: equality is the only tolerance."""
import numpy as np
import pytest

import common as CM
import k2_harness as H
import k2b_harness as B
import test_k2_cases as K

pytestmark = pytest.mark.gpu
SENTINEL = np.uint64(0xA5A5A5A5A5A5A5A5)

# n_rows x n_batch: waves straddle one and two member boundaries (37 x 3: lanes 0..63 hold members 0 and 1, 64..110 members 1 and 2;
# 24 x 5: the first wave holds three members); 24 x 3 = 72 batch rows leaves the second wave partial; 65 x 2 puts the 128-lane
# workgroup boundary inside member 1; 64 x n: members on wave boundaries; 101 x 5 = 505 rows: four workgroups
ROWS, BATCHES = (24, 37, 63, 64, 65, 101), (1, 2, 3, 5)
# m ON launch_spmm_t_batch's selection thresholds, as tests/test_k2_cases.py SPMM_CASES: spmm_t_kernel<NL, 4, true> from 8192, the sliced
# forms with 2 / 4 / 8 slices for (2048, 8192), (256, 2048], [.., 256]
MS = (8192, 8191, 2049, 2048, 257, 256, 100)


def _spmm_cases():
    """every (field, m) pair with every (n_rows, n_batch) pair at least once, out_alt on and off for every m and every field; in_off = 0"""
    pairs = [(fid, m) for fid in range(4) for m in MS]                       # 28
    shapes = [(r, b) for r in ROWS for b in BATCHES]                         # 24
    out = []
    for k in range(2 * len(pairs)):                                          # 56 cases: both lists more than once round
        fid, m = pairs[k % len(pairs)]
        n_rows, n_batch = shapes[(5 * k + k // len(pairs)) % len(shapes)]
        out.append((fid, m, n_rows, n_batch, bool((k + k // len(pairs)) & 1)))
    return out


SPMM = _spmm_cases()


def test_case_table_covers_what_it_says():
    assert {(r, b) for _, _, r, b, _ in SPMM} == {(r, b) for r in ROWS for b in BATCHES}
    assert {(f, m) for f, m, _, _, _ in SPMM} == {(f, m) for f in range(4) for m in MS}
    for key in (0, 1):                                                       # out_alt on and off in every field, at every m
        assert {(c[key], c[4]) for c in SPMM} == {(v, a) for v in (range(4) if key == 0 else MS) for a in (False, True)}
    assert len(set(SPMM)) == len(SPMM)


def _stride(extent):
    """elements between members: more than the extent (a sentinel in between), even (a multiple of 16 bytes in every field)"""
    return (extent + 7) & ~1


def _members_of(t, n_batch, shape):
    """views of the members' extents of a batch buffer"""
    n = shape[0] * shape[1]
    return [t[i, :n].reshape(shape + (t.shape[-1],)) for i in range(n_batch)]


@pytest.mark.parametrize("fid,m,n_rows,n_batch,alt", SPMM, ids=["%s-m%d-r%d-b%d%s" % (K.FT[f], m, r, b, "-alt" if a else "") for f, m, r, b, a in SPMM])
def test_spmm_equals_the_one_shot_launcher_member_by_member(fid, m, n_rows, n_batch, alt):
    L = CM.FIELD_L[fid]
    c = K._case("spmm", fid, m, n_rows, in_off=0, alt=alt)
    rowptr, colidx, vpat = K.build_structure(c)
    vals = K.build_values(c, rowptr, vpat)
    csr = H.Csr(fid, rowptr, colidx, K.ints_to_elems(vals, L))
    X = K.build_rows(c._replace(n_rows=n_batch * n_rows))                    # [position][batch row], no two batch rows equal
    x = K.ints_to_elems([v for pos in X for v in pos], L).reshape(c.n_in, n_batch * n_rows, L)
    n_pos = (c.n_in if alt else c.out_off + m) + 2
    t = np.full((n_batch, _stride(n_pos * n_rows), L), SENTINEL, np.uint64)
    o = np.full((n_batch, _stride(m * n_rows), L), SENTINEL, np.uint64) if alt else None
    for i, tm in enumerate(_members_of(t, n_batch, (n_pos, n_rows))):
        tm[:c.n_in] = x[:, i * n_rows:(i + 1) * n_rows]
    want_t, want_o = t.copy(), None if o is None else o.copy()
    for i in range(n_batch):                                                 # the reference: launch_spmm_t on member i alone
        tm = np.ascontiguousarray(_members_of(want_t, n_batch, (n_pos, n_rows))[i])
        om = np.full((m, n_rows, L), SENTINEL, np.uint64) if alt else None
        H.spmm_t(fid, tm, c.n_in, c.in_off, c.out_off, csr, c.limb, om)
        _members_of(want_t, n_batch, (n_pos, n_rows))[i][:] = tm
        if alt:
            _members_of(want_o, n_batch, (m, n_rows))[i][:] = om
    B.spmm_t(fid, t, n_pos, n_rows, c.n_in, c.in_off, c.out_off, csr, c.limb, o)
    got, want = (o, want_o) if alt else (t, want_t)
    bad = np.argwhere((got != want).any(axis=-1))
    assert len(bad) == 0, "%d elements differ, first (member, element): %s" % (len(bad), bad[:8].tolist())
    assert (t == want_t).all(), "T written outside the outputs"
    out = got[:, :m * n_rows] if alt else got[:, c.out_off * n_rows:(c.out_off + m) * n_rows]
    assert (out != SENTINEL).any(axis=-1).all()                              # (and the reference did write every output)


def test_launcher_refuses_ft255_without_the_limb_form():
    c = K._case("spmm", 3, 300, 24, in_off=0)
    rowptr, colidx, _ = K.build_structure(c)
    n_pos = c.out_off + c.m
    t = np.full((2, _stride(n_pos * 24), 4), SENTINEL, np.uint64)
    with pytest.raises(H.HipError) as e:
        B.spmm_t(3, t, n_pos, 24, c.n_in, 0, c.out_off, H.Csr(3, rowptr, colidx, K.ints_to_elems([1] * len(colidx), 4)), False)
    assert e.value.code == B.HIP_ERROR_INVALID_VALUE and (t == SENTINEL).all()


def _mixed(fid, n, seed):
    import random
    p = CM.field_p(fid)
    rnd = random.Random(seed)
    consts = [p - 1, CM.maximal_limbs(fid, 32, 2 * CM.FIELD_L[fid] - 1), 0, 1]
    return K.ints_to_elems([consts[i % 7] if i % 7 < 4 else rnd.randrange(p) for i in range(n)], CM.FIELD_L[fid])


# (n_rows, n_batch, n_valid, src_stride): 24 x 3 -- 72 batch rows in tiles of 32, the last tile partial, members 0 | 1 and 1 | 2 inside
# a tile; 10 x 4 -- one tile holds four members; 37 x 2 and 65 x 2 -- a member boundary off every tile edge; n_valid = 45, 33: the
# second tile of positions is partial; 64: whole tiles
T_SHAPES = [(24, 3, 45, 50), (10, 4, 33, 33), (37, 2, 64, 70), (65, 2, 45, 45)]


@pytest.mark.parametrize("canon", [False, True], ids=["mont", "canon"])
@pytest.mark.parametrize("copy", [False, True], ids=["nocopy", "copy"])
@pytest.mark.parametrize("n_rows,n_batch,n_valid,src_stride", T_SHAPES)
@pytest.mark.parametrize("fid", [0, 1, 2, 3])
def test_transpose_equals_the_one_shot_launcher_member_by_member(fid, n_rows, n_batch, n_valid, src_stride, copy, canon):
    L = CM.FIELD_L[fid]
    n_total = n_batch * n_rows
    src = _mixed(fid, n_total * src_stride, n_rows * 100 + n_valid)
    # one member-local bound for the ragged form: a member's last row reads zero from its 8th element on
    for n_src_total in (None, (n_rows - 1) * src_stride + 7):
        t = np.full((n_batch, _stride(n_valid * n_rows), L), SENTINEL, np.uint64)
        cp = np.full_like(src, SENTINEL) if copy else None
        want_t, want_cp = t.copy(), None if cp is None else cp.copy()
        for i in range(n_batch):
            lo, hi = i * n_rows * src_stride, (i + 1) * n_rows * src_stride
            tm = np.ascontiguousarray(_members_of(want_t, n_batch, (n_valid, n_rows))[i])
            cm = np.ascontiguousarray(want_cp[lo:hi]) if copy else None
            H.transpose_to_t(fid, np.ascontiguousarray(src[lo:hi]), src_stride, n_valid, n_rows, tm, n_src_total, cm, canon)
            _members_of(want_t, n_batch, (n_valid, n_rows))[i][:] = tm
            if copy:
                want_cp[lo:hi] = cm
        B.transpose_to_t(fid, src, src_stride, n_valid, n_rows, t, n_src_total, cp, canon)
        assert (t == want_t).all(), np.argwhere((t != want_t).any(axis=-1))[:8].tolist()
        assert (t[:, :n_valid * n_rows] != SENTINEL).any(axis=-1).all()
        if copy:
            assert (cp == want_cp).all(), np.argwhere((cp != want_cp).any(axis=-1))[:8].tolist()


@pytest.mark.parametrize("n_in,n_out", [(1, 63), (10, 65)])
@pytest.mark.parametrize("n_rows,n_batch", [(24, 3), (37, 5), (65, 2), (64, 1)])
@pytest.mark.parametrize("fid", [0, 1, 2, 3])
def test_rs_base_case_equals_the_one_shot_launcher_member_by_member(fid, n_rows, n_batch, n_in, n_out):
    L = CM.FIELD_L[fid]
    out_off = 7
    n_pos = out_off + n_out + 1
    in_t = np.full((n_batch, _stride(n_in * n_rows), L), SENTINEL, np.uint64)
    in_t[:, :n_in * n_rows] = _mixed(fid, n_batch * n_in * n_rows, n_rows + n_in).reshape(n_batch, n_in * n_rows, L)
    t = np.full((n_batch, _stride(n_pos * n_rows), L), SENTINEL, np.uint64)
    want = t.copy()
    for i in range(n_batch):
        tm = np.ascontiguousarray(_members_of(want, n_batch, (n_pos, n_rows))[i])
        H.sdig_rs_t(fid, np.ascontiguousarray(_members_of(in_t, n_batch, (n_in, n_rows))[i]), tm, out_off, n_out)
        _members_of(want, n_batch, (n_pos, n_rows))[i][:] = tm
    B.sdig_rs_t(fid, in_t, n_in, t, n_pos, n_rows, out_off, n_out)
    assert (t == want).all(), np.argwhere((t != want).any(axis=-1))[:8].tolist()
    assert (t[:, out_off * n_rows:(out_off + n_out) * n_rows] != SENTINEL).any(axis=-1).all()

"""The Brakedown (K2) kernels called directly (tests/k2_harness.py over tests/native/k2_harness.cpp) on the matrices and operands of
tests/test_k2_cases.py: term counts on every normalise / REDC-chunk / Wide-batch / slice boundary, operands at their largest limbs on
BOTH sides, empty outputs, every kernel instantiation of launch_spmm_t and launch_spmv, the R-S base case, the transposes and pad_rows.
The C ABI cannot reach these cases (matgen decides the matrices, and only pre[0] sees the message).

Every output of every row is compared with Python-int arithmetic (test_k2_cases.ref_matvec / ref_rs, pinned there against the C oracle),
and so is every element around the outputs that the kernel must leave alone.  The arithmetic is exact: equality is the only tolerance."""
import numpy as np
import pytest

import common as CM
import k2_harness as H
import test_k2_cases as K

pytestmark = pytest.mark.gpu
SENTINEL = np.uint64(0xA5A5A5A5A5A5A5A5)


def _flat(rows_of_lists):
    return [v for row in rows_of_lists for v in row]


def _report(bad, c, rowptr, vpat):
    ln = np.diff(rowptr)
    return ["output %d (%d terms, values %s, %s) row %d (%s)" % (o, ln[o], vpat[o], K.arithmetic(c, int(ln[o])), r, K.XPATS[r % 6])
            for o, r in bad[:12]]


@pytest.mark.parametrize("c", K.CASES, ids=K.case_id)
def test_every_output_of_every_row(c):
    fid, L, m, n_rows = c.fid, CM.FIELD_L[c.fid], c.m, c.n_rows
    rowptr, colidx, vpat = K.build_structure(c)
    vals = K.build_values(c, rowptr, vpat)
    X = K.build_rows(c)                                          # [input position][row]
    want = K.ref_matvec(fid, rowptr, colidx, vals, X)            # [output][row]
    csr = H.Csr(fid, rowptr, colidx, K.ints_to_elems(vals, L) if vals else np.zeros((0, L), np.uint64))
    x_t = K.ints_to_elems(_flat(X), L).reshape(c.n_in, n_rows, L)
    want_t = K.ints_to_elems(_flat(want), L).reshape(m, n_rows, L)
    n_pos = (c.in_off + c.n_in if c.alt else c.out_off + m) + 2
    if c.path == "spmm":
        buf = np.full((n_pos, n_rows, L), SENTINEL, np.uint64)
        buf[c.in_off:c.in_off + c.n_in] = x_t
        alt = np.full((m, n_rows, L), SENTINEL, np.uint64) if c.alt else None
        expect, expect_alt = buf.copy(), want_t
        if not c.alt:
            expect[c.out_off:c.out_off + m] = want_t
        H.spmm_t(fid, buf, c.n_in, c.in_off, c.out_off, csr, c.limb, alt)
        got_out = alt if c.alt else buf[c.out_off:c.out_off + m]
    else:
        buf = np.full((n_rows, n_pos, L), SENTINEL, np.uint64)
        buf[:, c.in_off:c.in_off + c.n_in] = x_t.transpose(1, 0, 2)
        alt = np.full((n_rows, m + 3, L), SENTINEL, np.uint64) if c.alt else None     # (out_alt_stride > m)
        expect = buf.copy()
        if c.alt:
            expect_alt = alt.copy()
            expect_alt[:, :m] = want_t.transpose(1, 0, 2)
        else:
            expect[:, c.out_off:c.out_off + m] = want_t.transpose(1, 0, 2)
        H.spmv(fid, buf, c.n_in, c.in_off, c.out_off, csr, c.limb, alt)
        got_out = (alt[:, :m] if c.alt else buf[:, c.out_off:c.out_off + m]).transpose(1, 0, 2)
    bad = np.argwhere((got_out != want_t).any(axis=-1))
    assert len(bad) == 0, "%d of %d outputs wrong: %s" % (len(bad), m * n_rows, _report(bad.tolist(), c, rowptr, vpat))
    assert (buf == expect).all(), "written outside the outputs"
    if c.alt:
        assert (alt == expect_alt).all()


def test_launcher_refuses_ft255_without_the_limb_form():
    """spmm_t_terms<8> has the limb path only and reads vals29 unasked: launch_spmm_t returns hipErrorInvalidValue and launches nothing"""
    c = K._case("spmm", 3, 300, 24, limb=False)
    rowptr, colidx, vpat = K.build_structure(c._replace(limb=True))
    vals = K.ints_to_elems([1] * len(colidx), 4)
    buf = np.full((c.out_off + c.m, 24, 4), SENTINEL, np.uint64)
    with pytest.raises(H.HipError) as e:
        H.spmm_t(3, buf, c.n_in, c.in_off, c.out_off, H.Csr(3, rowptr, colidx, vals), False)
    assert e.value.code == H.HIP_ERROR_INVALID_VALUE and (buf == SENTINEL).all()


@pytest.mark.parametrize("fid", [1, 2, 3])
def test_limb_form_of_the_extremes_on_the_device(fid):
    """what ctx.cpp's upload makes of matrix values (launch_to_r29 / launch_ntt_lns_roots with R' mod p): the limbs of v R' / R mod p,
    zero-padded to the table stride -- for ln_maxv all ones below the top limb"""
    p, L = CM.field_p(fid), CM.FIELD_L[fid]
    N, W = CM.LN_SHAPE[fid]
    vals = [CM.ln_maxv(fid), p - 1, 0, 1, CM.ln_maxx(fid), pow(3, 200, p)]
    got = H.limb_form(fid, K.ints_to_elems(vals, L))
    for v, row in zip(vals, got):
        vl = v * pow(2, N * W, p) * pow(2, -64 * L, p) % p
        limbs = [(vl >> (W * k)) & ((1 << W) - 1) for k in range(N - 1)] + [vl >> (W * (N - 1))]
        assert row.tolist() == limbs + [0] * (CM.LN_STRIDE[fid] - N)
    assert got[0, :N - 1].tolist() == [(1 << W) - 1] * (N - 1)


def _rs_inputs(fid, n_in, n_rows):
    """[j][row]: rows of all p - 1, all of each extreme, random, in turn; no two rows equal from the second entry on"""
    import random
    p = CM.field_p(fid)
    rnd = random.Random(n_in * 1000 + n_rows)
    consts = [p - 1, CM.maximal_limbs(fid, 32, 2 * CM.FIELD_L[fid] - 1), CM.ln_maxx(fid) if fid else p - 2]
    rows = []
    for r in range(n_rows):
        x = [consts[r % 4]] * n_in if r % 4 < 3 else [rnd.randrange(p) for _ in range(n_in)]
        if n_in > 1 and r >= 4:
            x[1 + r % (n_in - 1)] = r
        rows.append(x)
    return [list(col) for col in zip(*rows)]


RS_SHAPES = [(1, 63), (2, 64), (10, 65), (107, 130)]


@pytest.mark.parametrize("n_in,n_out", RS_SHAPES)
@pytest.mark.parametrize("n_rows", [1, 23])
@pytest.mark.parametrize("fid", [0, 1, 2, 3])
def test_rs_base_case_row_major(fid, n_rows, n_in, n_out):
    L = CM.FIELD_L[fid]
    inp = _rs_inputs(fid, n_in, n_rows)
    want = K.ints_to_elems(_flat(K.ref_rs(fid, inp, n_out)), L).reshape(n_out, n_rows, L).transpose(1, 0, 2)
    in_stride, out_off = n_in + 3, 5
    src = np.full((n_rows, in_stride, L), SENTINEL, np.uint64)
    src[:, :n_in] = K.ints_to_elems(_flat(inp), L).reshape(n_in, n_rows, L).transpose(1, 0, 2)
    mat = np.full((n_rows, out_off + n_out + 2, L), SENTINEL, np.uint64)
    expect = mat.copy()
    expect[:, out_off:out_off + n_out] = want
    H.sdig_rs(fid, src, n_in, mat, out_off, n_out)
    assert (mat == expect).all(), np.argwhere((mat != expect).any(axis=-1))[:8].tolist()


@pytest.mark.parametrize("n_in,n_out", RS_SHAPES)
@pytest.mark.parametrize("n_rows", [24, 65, 130, 257])
@pytest.mark.parametrize("fid", [0, 1, 2, 3])
def test_rs_base_case_position_major(fid, n_rows, n_in, n_out):
    L = CM.FIELD_L[fid]
    inp = _rs_inputs(fid, n_in, n_rows)
    want = K.ints_to_elems(_flat(K.ref_rs(fid, inp, n_out)), L).reshape(n_out, n_rows, L)
    in_t = K.ints_to_elems(_flat(inp), L).reshape(n_in, n_rows, L)
    out_off = 7
    t = np.full((out_off + n_out + 1, n_rows, L), SENTINEL, np.uint64)
    expect = t.copy()
    expect[out_off:out_off + n_out] = want
    H.sdig_rs_t(fid, in_t, t, out_off, n_out)
    assert (t == expect).all(), np.argwhere((t != expect).any(axis=-1))[:8].tolist()


def _mixed_elems(fid, n, seed):
    """n stored elements: p - 1, the extremes, 0, 1 and random ones in turn, as (ints, (n, L) limbs)"""
    import random
    p = CM.field_p(fid)
    rnd = random.Random(seed)
    consts = [p - 1, CM.maximal_limbs(fid, 32, 2 * CM.FIELD_L[fid] - 1), CM.ntt_maxlimb(fid), 0, 1]
    vals = [consts[i % 8] if i % 8 < 5 else rnd.randrange(p) for i in range(n)]
    return vals, K.ints_to_elems(vals, CM.FIELD_L[fid])


@pytest.mark.parametrize("canon", [False, True], ids=["mont", "canon"])
@pytest.mark.parametrize("n_rows,n_valid,stride,ragged", [(24, 45, 50, 0), (33, 70, 70, 9), (65, 31, 37, 40), (130, 97, 97, 0)])
@pytest.mark.parametrize("fid", [0, 1, 2, 3])
def test_transpose_to_t(fid, n_rows, n_valid, stride, ragged, canon):
    """rows and positions that are no multiples of the 32 x 32 tile, n_valid < stride, a ragged n_src_total (the source ends `ragged`
    elements before the last row does: those read as zero), copy_dst, and canon (T receives x / R mod p; copy_dst the values as read)"""
    L, p = CM.FIELD_L[fid], CM.field_p(fid)
    span = (n_rows - 1) * stride + n_valid
    total = span - ragged
    vals, src = _mixed_elems(fid, span, n_rows + n_valid)
    rinv = pow(2, -64 * L, p)
    seen = [v if i < total else 0 for i, v in enumerate(vals)]
    want_t = np.full((n_valid, n_rows, L), SENTINEL, np.uint64)
    want_copy = np.full((span, L), SENTINEL, np.uint64)
    as_t = K.ints_to_elems([s * rinv % p for s in seen] if canon else seen, L)
    as_read = K.ints_to_elems(seen, L)
    for r in range(n_rows):
        want_t[:, r] = as_t[r * stride:r * stride + n_valid]
        want_copy[r * stride:r * stride + n_valid] = as_read[r * stride:r * stride + n_valid]
    src[total:] = SENTINEL                                       # (never read: flat elements >= n_src_total)
    t = np.full((n_valid, n_rows, L), SENTINEL, np.uint64)
    copy = np.full((span, L), SENTINEL, np.uint64)
    H.transpose_to_t(fid, src, stride, n_valid, n_rows, t, total if ragged else None, copy, canon)
    assert (t == want_t).all() and (copy == want_copy).all()
    t2 = np.full((n_valid, n_rows, L), SENTINEL, np.uint64)
    H.transpose_to_t(fid, src, stride, n_valid, n_rows, t2, total if ragged else None, None, canon)
    assert (t2 == want_t).all()
    # and back: the round trip gives the rows as read (the padding of a wider destination row stays as it was)
    dst = np.full((n_rows, n_valid + 4, L), SENTINEL, np.uint64)
    H.transpose_from_t(fid, t, dst)
    assert (dst[:, :n_valid] == want_t.transpose(1, 0, 2)).all() and (dst[:, n_valid:] == SENTINEL).all()


@pytest.mark.parametrize("n_rows,n_valid,src_stride,dst_stride", [(1, 45, 45, 60), (23, 300, 301, 300), (5, 1, 2, 3), (2, 262200, 262200, 262201)])
@pytest.mark.parametrize("fid", [0, 3])
def test_pad_rows(fid, n_rows, n_valid, src_stride, dst_stride):
    """dst[row][0 .. n_valid) = src[row][..]; what lies behind in a dst row is left alone (the encode fills it).  262200 elements: the
    grid-stride loop runs more than once (1024 x 256 threads)"""
    L = CM.FIELD_L[fid]
    _, src = _mixed_elems(fid, n_rows * src_stride, n_valid)
    src = src.reshape(n_rows, src_stride, L)
    dst = np.full((n_rows, dst_stride, L), SENTINEL, np.uint64)
    H.pad_rows(fid, src, dst, n_valid)
    assert (dst[:, :n_valid] == src[:, :n_valid]).all() and (dst[:, n_valid:] == SENTINEL).all()


@pytest.mark.parametrize("n_rows", [3, 24, 65])
@pytest.mark.parametrize("fid", [1, 3])
def test_deep_levels_through_the_api_at_extremes(oracle, fid, n_rows):
    """The real encode (SdigEncoding + LcCommit.commit, ctx.cpp's level chain) on messages SOLVED so that pre[0]'s outputs -- what
    pre[1] gathers -- are all limb-extreme, all p - 1, or 0 / extreme alternating (test_k2_cases.solve_message): the codeword holds
    those targets, pre[1]'s outputs equal the Python-int reference on them, and the whole comm is the oracle's.  3 rows: spmv_kernel;
    24 / 65 rows: the position-major path (pre[1] has 32 outputs: spmm_t_sliced_kernel<NL, 8>)."""
    from lcpc_amd import LcCommit, SdigEncoding
    O = oracle
    oenc, n_cols, pre, targets, msgs = K.deep_level_case(O, fid)
    L, n, m0, m1 = CM.FIELD_L[fid], K.DEEP_N_PER_ROW, pre[0][3], pre[1][3]
    assert pre[1][4] == m0
    which = [r % 3 for r in range(n_rows)]
    coeffs = np.concatenate([K.ints_to_elems(msgs[w], L) for w in which])
    enc = SdigEncoding.new_from_dims(fid, n, n_cols, 21, 3)
    c = LcCommit.commit(coeffs, enc)
    assert c.n_rows == n_rows
    comm = np.asarray(c.comm()).reshape(n_rows, n_cols, L)
    want1 = K.ref_matvec(fid, pre[1][0], pre[1][1], pre[1][2], [list(col) for col in zip(*targets)])      # [output][target]
    for r, w in enumerate(which):
        assert K.elems_to_ints(comm[r, n:n + m0]) == targets[w], r
        assert K.elems_to_ints(comm[r, n + m0:n + m0 + m1]) == [o[w] for o in want1], r
    oc = O.Commit.commit(coeffs, oenc, n_threads=8)
    assert (comm.reshape(-1, L) == oc.comm()).all() and c.get_root() == oc.get_root()

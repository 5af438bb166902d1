"""The batch forms of the BLAKE3 column-hash and Merkle-tree kernels and the placement kernel (lcpc_amd/csrc/kernels.hip), launched
directly through tests/k3_harness.py on the batch tables of tests/test_k3_cases.py and compared word for word with its references.  What
lcpcx_commit_batch_device never hands them is handed here: strides with gaps, column counts that leave the last workgroup partly filled,
chunk ranges, row bases, position-major comm, trees that are not the commitment's, member counts at the grid limit, and both forms of the
chunk kernel on either side of their threshold.  Every member has its own data.  A batched buffer is an (n_batch, stride) word array,
sentinel-filled and compared whole: the expected array keeps the sentinel wherever the kernel must not write, the gaps behind every
member included."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import common as CM  # noqa: E402
import k3_harness as H  # noqa: E402
import test_k3_cases as K  # noqa: E402

pytestmark = pytest.mark.gpu
S = K.SENTINEL


def _buf(n_batch, stride):
    return np.full((n_batch, stride), S, np.uint32)


def _with(buf, members):
    """a copy of the batched buffer `buf` with `members` ((n_batch, ..) words) in front of every row"""
    out = buf.copy()
    flat = members.reshape(members.shape[0], -1)
    out[:, :flat.shape[1]] = flat
    return out


def _leaf_batch(c, idx, begin, count, whole, comm_gap):
    nc = CM.leaf_n_chunks(c.fid, c.n_rows)
    row_base, n_local = K.launch_rows(c, begin, count, whole)
    comms, rs, cs = K.batch_comm_buffer(c.fid, idx, row_base, n_local, c.layout, c.canon)
    leaf = H.Leaf(c.fid, comms[0], rs, cs, c.n_cols, row_base, n_local, c.n_rows, begin, count, nc, c.canon)
    return H.LeafBatch(leaf, H.batch_comm(comms, K.batch_stride(2 * comms[0].size, comm_gap)))


def _ref_cvs(c, idx):
    """(n_batch, n_chunks, n_cols, 8): the reference chaining values (one chunk: digests) of every member"""
    nc = CM.leaf_n_chunks(c.fid, c.n_rows)
    cvs = K.ref_chunk_cvs(K.batch_message_words(c.fid, idx), CM.leaf_len(c.fid, c.n_rows), range(nc), nc)
    return np.ascontiguousarray(cvs.reshape(nc, c.n_batch, c.n_cols, 8).transpose(1, 0, 2, 3))


def _check_leaf_chunks(c):
    """a whole-message launch, then the ranges of the split in reverse order into one buffer: after every launch the buffer is the one
    before it with the reference in that launch's slots -- the slot before and the slot behind every member's, the other slots and the
    gaps keep what they held"""
    nc = CM.leaf_n_chunks(c.fid, c.n_rows)
    idx = K.batch_index(c.fid, c.n_rows, c.n_cols, c.n_batch, 1)
    want = _ref_cvs(c, idx)
    slots = nc + 2
    out_stride = K.batch_stride(slots * c.n_cols * 8, c.out_gap)
    members = np.full((c.n_batch, slots, c.n_cols, 8), S, np.uint32)
    members[:, 1:1 + nc] = want
    blank = _buf(c.n_batch, out_stride)
    whole, expect = blank.copy(), _with(blank, members)
    H.leaf_chunks_batch(_leaf_batch(c, idx, 0, nc, True, c.comm_gap), whole, slots, 1)
    assert np.array_equal(whole, expect), "whole-message launch"
    if nc == 1:
        return
    split = blank.copy()
    members[:] = S
    for begin, count in reversed(c.split):
        members[:, 1 + begin:1 + begin + count] = want[:, begin:begin + count]
        H.leaf_chunks_batch(_leaf_batch(c, idx, begin, count, False, c.comm_gap), split, slots, 1 + begin)
        assert np.array_equal(split, _with(blank, members)), "range (%d, %d)" % (begin, count)
    assert np.array_equal(split, expect)


@pytest.mark.parametrize("c", [pytest.param(c, id=K.batch_case_id(c)) for c in K.batch_leaf_cases()])
def test_leaf_chunks_batch_quad(c):
    """four lanes per column: every field, both CANON values, every batch size, stride kind and column count of the tables"""
    assert all(l[0] for l in K._batch_launches(c))
    _check_leaf_chunks(c)


@pytest.mark.parametrize("c", [pytest.param(c, id=K.batch_case_id(c)) for c in K.batch_lane_cases()])
def test_leaf_chunks_batch_at_the_form_border(c):
    """65536 (column, chunk) pairs in the batch and just above: one lane per column for every field and CANON value, the same three-chunk
    shape in both forms"""
    _check_leaf_chunks(c)


def test_leaf_chunks_batch_grid_limit():
    c = K.GRID_LIMIT_LEAF
    assert c.n_batch == 65535
    _check_leaf_chunks(c)


def _tree_batch(fid, n_rows, n_cols, canon, layout, n_batch, comm_gap, begin=0, count=None):
    c = K.BatchLeafCase(fid, n_rows, n_cols, canon, layout, None, n_batch, comm_gap, None)
    nc = CM.leaf_n_chunks(fid, n_rows)
    idx = K.batch_index(fid, n_rows, n_cols, n_batch, 2)
    return c, idx, _leaf_batch(c, idx, begin, nc if count is None else count, True, comm_gap)


@pytest.mark.parametrize("fid,n_rows,n_cols,canon,layout,n_batch,comm_gap,hashes_gap", K.leaf_tree_batch_cases())
def test_leaf_tree_batch(fid, n_rows, n_cols, canon, layout, n_batch, comm_gap, hashes_gap):
    """leaf digests and six levels of every member in one launch, the rest of every member and the gaps untouched; then
    launch_merkle_tree_from_batch(6) completes every member"""
    nc = CM.leaf_n_chunks(fid, n_rows)
    c, idx, lb = _tree_batch(fid, n_rows, n_cols, canon, layout, n_batch, comm_gap)
    cvs = _ref_cvs(c, idx)
    n_slots = 2 * n_cols - 1
    done = sum(n_cols >> j for j in range(7))
    part = np.full((n_batch, n_slots, 8), S, np.uint32)
    full = np.empty_like(part)
    for m in range(n_batch):
        part[m, :n_cols] = cvs[m, 0] if nc == 1 else K.ref_parent(cvs[m, 0], cvs[m, 1], True)
        full[m] = K.ref_tree(part[m].copy(), n_cols)
        part[m, n_cols:done] = full[m, n_cols:done]
    hashes = _buf(n_batch, K.batch_stride(n_slots * 8, hashes_gap))
    blank = hashes.copy()
    H.leaf_tree_batch(lb, hashes, n_cols)
    assert np.array_equal(hashes, _with(blank, part))
    if done < n_slots:
        roots = np.full((n_batch + 1, 8), S, np.uint32)
        H.merkle_tree_from_batch(hashes, n_cols, 6, roots)
        assert np.array_equal(hashes, _with(blank, full))
        assert np.array_equal(roots[:n_batch], full[:, -1]) and (roots[n_batch] == S).all()


def test_leaf_tree_batch_refuses_what_it_does_not_support():
    """launch_leaf_tree_batch answers hipErrorInvalidValue -- and writes nothing -- outside leaf_tree_supported, for no member and for
    more members than a grid dimension holds"""
    def refused(lb, np2, told=None):
        hashes = _buf(lb.n_batch, K.batch_stride((2 * np2 - 1) * 8, 4))
        with pytest.raises(H.HipError) as e:
            H.leaf_tree_batch(lb, hashes, np2, told)
        assert e.value.code == H.HIP_ERROR_INVALID_VALUE and (hashes == S).all()

    for fid, n_rows, n_cols, np2, begin, count in ((0, 10, 64, 64, 0, None), (0, 10, 192, 256, 0, None), (3, 10, 100, 128, 0, None),
                                                   (1, 130, 256, 256, 0, None), (0, 130, 256, 256, 0, 1), (0, 130, 256, 256, 1, 1),
                                                   (0, 130, 256, 512, 0, None)):
        _, _, lb = _tree_batch(fid, n_rows, n_cols, False, "row", 2, 0, begin, count)
        assert not CM.leaf_tree_supported(n_cols, np2, begin, lb.leaf.n_chunks_local, CM.leaf_n_chunks(fid, n_rows))
        refused(lb, np2)
    _, _, lb = _tree_batch(0, 10, 128, False, "row", 2, 0)
    assert CM.leaf_tree_supported(128, 128, 0, 1, 1)
    refused(lb, 128, 0)
    refused(lb, 128, 65536)


def _random_words(shape, seed):
    return np.random.default_rng(seed).integers(0, 1 << 32, shape, dtype=np.uint64).astype(np.uint32)


@pytest.mark.parametrize("n_chunks", K.CHUNK_COUNTS)
def test_leaf_finish_batch(n_chunks):
    """launch_leaf_finish_batch folds every member's chunk CVs into its digests (300 columns: a second, partly empty workgroup); the
    digest slot past n_cols and the gaps keep their sentinel.  The cvs buffer is the kernel's stack: the gaps, and in every member the
    slots the stack never reaches, keep what they held"""
    n_cols, i = 300, K.CHUNK_COUNTS.index(n_chunks)
    keep = sorted(set(range(n_chunks)) - K.finish_stack_slots(n_chunks))
    for j, n_batch in enumerate((1, 2, 5)):
        cv_gap, dig_gap = K.BATCH_GAPS[(i + j) % 5]
        cvs = _random_words((n_batch, n_chunks, n_cols, 8), 16 * n_chunks + n_batch)
        dig = np.full((n_batch, n_cols + 1, 8), S, np.uint32)
        cv_buf = _with(_buf(n_batch, K.batch_stride(n_chunks * n_cols * 8, cv_gap)), cvs)
        blank = _buf(n_batch, K.batch_stride((n_cols + 1) * 8, dig_gap))
        dig_buf, before = blank.copy(), cv_buf.copy()
        H.leaf_finish_batch(cv_buf, n_chunks, n_cols, dig_buf, n_cols + 1)
        for m in range(n_batch):
            dig[m, :n_cols] = K.ref_subtree(cvs[m], 0, n_chunks, True)
        assert np.array_equal(dig_buf, _with(blank, dig))
        member = cvs[0].size
        assert np.array_equal(cv_buf[:, member:], before[:, member:]), "the gaps behind the members' CVs"
        got = cv_buf[:, :member].reshape(cvs.shape)
        assert np.array_equal(got[:, keep], cvs[:, keep]), "slots the stack does not reach"


@pytest.mark.parametrize("np2,levels_done,n_batch,gap", K.tree_batch_cases())
def test_merkle_tree_from_batch(np2, levels_done, n_batch, gap):
    """every member's whole hashes array is the reference's, the levels below levels_done as given; root_out[i] is member i's last slot
    and the words behind the last root keep their sentinel; the run without a root_out agrees"""
    n_slots = 2 * np2 - 1
    given = sum(np2 >> j for j in range(levels_done + 1))
    assert given < n_slots
    base = np.full((n_batch, n_slots, 8), S, np.uint32)
    base[:, :np2] = _random_words((n_batch, np2, 8), np2 + levels_done + n_batch)
    want = np.stack([K.ref_tree(base[m].copy(), np2) for m in range(n_batch)])
    base[:, :given] = want[:, :given]
    blank = _buf(n_batch, K.batch_stride(n_slots * 8, gap))
    h1, roots = _with(blank, base), np.full((n_batch + 1, 8), S, np.uint32)
    H.merkle_tree_from_batch(h1, np2, levels_done, roots)
    assert np.array_equal(h1, _with(blank, want))
    assert np.array_equal(roots[:n_batch], want[:, -1]) and (roots[n_batch] == S).all()
    h2 = _with(blank, base)
    H.merkle_tree_from_batch(h2, np2, levels_done)
    assert np.array_equal(h2, h1)


def test_merkle_tree_from_batch_grid_limit():
    n_batch, np2 = CM.K3B_MAX_BATCH, 2
    base = np.full((n_batch, 3, 8), S, np.uint32)
    base[:, :2] = _random_words((n_batch, 2, 8), 5)
    want = base.copy()
    want[:, 2] = K.ref_node(base[:, 0], base[:, 1])
    blank = _buf(n_batch, 24)
    h, roots = _with(blank, base), np.full((n_batch + 1, 8), S, np.uint32)
    H.merkle_tree_from_batch(h, np2, 0, roots)
    assert np.array_equal(h, _with(blank, want))
    assert np.array_equal(roots[:n_batch], want[:, 2]) and (roots[n_batch] == S).all()


S64 = np.uint64((S << 32) | S)
POISON = np.uint64((1 << 64) - 1)


@pytest.mark.parametrize("n_batch,src_stride,n_valid,dst_stride", K.place_cases())
def test_batch_place(n_batch, src_stride, n_valid, dst_stride):
    """member i's n_valid words from src + i src_stride at dst + i dst_stride, zeros up to dst_stride; what lies behind a polynomial in
    src (all ones) appears nowhere, and the words behind the last member keep their sentinel"""
    src = np.full((n_batch, src_stride), POISON, np.uint64)
    src[:, :n_valid] = np.random.default_rng([n_batch, src_stride, n_valid, dst_stride]).integers(0, 1 << 63, (n_batch, n_valid), dtype=np.uint64)
    tail = 8
    dst = np.full(n_batch * dst_stride + tail, S64, np.uint64)
    want = dst.copy()
    w = want[:n_batch * dst_stride].reshape(n_batch, dst_stride)
    w[:] = 0
    w[:, :n_valid] = src[:, :n_valid]
    H.batch_place(src, n_valid, dst, dst_stride)
    assert np.array_equal(dst, want)


def test_batch_place_refuses_a_polynomial_longer_than_its_stride():
    for src_stride, n_valid, dst_stride in ((8, 5, 4), (4, 5, 8)):
        src = np.zeros((3, src_stride), np.uint64)
        dst = np.full(3 * dst_stride + 8, S64, np.uint64)
        with pytest.raises(H.BadArgs):
            H.batch_place(src, n_valid, dst, dst_stride)
        assert (dst == S64).all()

"""The BLAKE3 column-hash (K3), Merkle-tree (K4) and path-gather kernels of lcpc_amd/csrc/kernels.hip, launched directly through
tests/k3_harness.py on the cases of tests/test_k3_cases.py and compared word for word with its references (oracle/pyref.py's BLAKE3 and
Python integers; that module checks them without a GPU).  What the C ABI cannot reach is reached here: non-canonical Ft255 comm on many
chunks, canonical comm for every field, arbitrary chunk ranges, row bases, node tables and slot tables, every tree width from either
starting level.  Buffers the kernels write are sentinel-filled first and compared whole."""
import os
import random
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import common as CM  # noqa: E402
import k3_harness as H  # noqa: E402
import test_k3_cases as K  # noqa: E402

pytestmark = pytest.mark.gpu
S = K.SENTINEL


def _leaf(c, idx, begin, count, whole):
    nc = CM.leaf_n_chunks(c.fid, c.n_rows)
    row_base, n_local = K.launch_rows(c, begin, count, whole)
    comm, rs, cs = K.comm_buffer(c.fid, idx, row_base, n_local, c.layout, c.canon)
    return H.Leaf(c.fid, comm, rs, cs, c.n_cols, row_base, n_local, c.n_rows, begin, count, nc, c.canon)


def _leaf_cases():
    return [pytest.param(c, id=K.leaf_case_id(c)) for fid in K.FIDS for c in K.leaf_cases(fid)]


@pytest.mark.parametrize("c", _leaf_cases())
def test_leaf_chunks(c):
    """the CV of every (chunk, column) -- one chunk: the digest -- from a whole-message launch and from split-range launches into one buffer;
    the slot past the range and (a launch of the first n_cols - 1 columns) the last column's words keep their sentinel"""
    nc, mlen = CM.leaf_n_chunks(c.fid, c.n_rows), CM.leaf_len(c.fid, c.n_rows)
    idx = K.case_index(c.fid, c.n_rows, c.n_cols, 1)
    want = K.ref_chunk_cvs(K.message_words(c.fid, idx), mlen, range(nc), nc)
    whole = np.full((nc + 1, c.n_cols, 8), S, np.uint32)
    H.leaf_chunks(_leaf(c, idx, 0, nc, True), whole)
    assert np.array_equal(whole[:nc], want), "whole-message launch"
    assert (whole[nc] == S).all()
    split = np.full((nc + 2, c.n_cols, 8), S, np.uint32)
    for begin, count in reversed(c.split):
        before = split.copy()
        H.leaf_chunks(_leaf(c, idx, begin, count, False), split, 1 + begin)
        before[1 + begin:1 + begin + count] = want[begin:begin + count]
        assert np.array_equal(split, before), "range (%d, %d): its slots are the reference's, every other slot is untouched" % (begin, count)
    assert np.array_equal(split[1:nc + 1], whole[:nc]) and (split[0] == S).all() and (split[nc + 1] == S).all()
    if c.n_cols > 1 and c.n_cols <= 300:
        # columns >= n_cols are not written: the same comm with n_cols - 1 columns told to the kernel (row-major: the stride stays)
        leaf = _leaf(c, idx, 0, nc, True)
        if c.layout == "row":
            narrow = H.Leaf(c.fid, leaf.comm, c.n_cols, 1, c.n_cols - 1, 0, c.n_rows, c.n_rows, 0, nc, nc, c.canon)
        else:
            narrow = H.Leaf(c.fid, leaf.comm, 1, c.n_rows, c.n_cols - 1, 0, c.n_rows, c.n_rows, 0, nc, nc, c.canon)
        out = np.full((nc + 1, c.n_cols - 1, 8), S, np.uint32)
        H.leaf_chunks(narrow, out)
        assert np.array_equal(out[:nc], want[:, :c.n_cols - 1]) and (out[nc] == S).all()


def _random_cvs(shape, seed):
    return np.random.default_rng(seed).integers(0, 1 << 32, shape, dtype=np.uint64).astype(np.uint32)


@pytest.mark.parametrize("n_chunks", K.CHUNK_COUNTS)
def test_leaf_finish(n_chunks):
    """launch_leaf_finish folds the chunk CVs of every column into its digest (non-power-of-two counts: the stack merge); 300 columns:
    a second, partly empty workgroup; the digest slot past n_cols keeps its sentinel"""
    n_cols = 300
    cvs = _random_cvs((n_chunks, n_cols, 8), n_chunks)
    want = K.ref_subtree(cvs, 0, n_chunks, True)
    dig = np.full((n_cols + 1, 8), S, np.uint32)
    H.leaf_finish(cvs.copy(), dig)
    assert np.array_equal(dig[:n_cols], want) and (dig[n_cols] == S).all()


def _run_nodes(cvs, chunk0, logs, root, rng, n_cols, permute):
    """node CVs from chunk CVs by the reference, into permuted slots of a sentinel-filled buffer; -> (out, expected)"""
    at, nodes = chunk0, []
    for l in logs:
        nodes.append(K.ref_subtree(cvs, at, at + (1 << l), False))
        at += 1 << l
    n_nodes, n_slots = len(nodes), len(nodes) + 2
    slots = rng.sample(range(n_slots), n_nodes) if permute else list(range(n_nodes))
    buf = np.full((n_slots, n_cols, 8), S, np.uint32)
    for s, cv in zip(slots, nodes):
        buf[s] = cv
    out = np.full((n_cols + 1, 8), S, np.uint32)
    ident = not permute and not any(logs)
    H.leaf_finish_nodes(buf, None if ident else np.array(slots, np.uint32), None if ident else np.array(logs, np.uint32), n_nodes, chunk0,
                        at - chunk0, out, root)
    unused = [s for s in range(n_slots) if s not in slots]
    assert (buf[unused] == S).all(), "slots outside the table are not written"
    assert (out[n_cols] == S).all()
    return out[:n_cols]


def test_leaf_finish_nodes_every_decomposition():
    """launch_leaf_finish_nodes with root: every aligned node decomposition of 1 .. 9 chunks and seeded ones of 16, 17 and 33, the nodes in
    permuted slots (the stack lives in the slots of consumed nodes), gives the digest of the whole message; a single node is its own
    answer (it carries ROOT already)"""
    rng, n_cols = random.Random(9), 70
    cases = K.finish_node_cases()
    for i, (c, logs) in enumerate(cases):
        cvs = _random_cvs((c, n_cols, 8), 100 + c)
        want = K.ref_subtree(cvs, 0, c, True) if len(logs) > 1 else K.ref_subtree(cvs, 0, c, False)
        got = _run_nodes(cvs, 0, logs, True, rng, n_cols, permute=i % 4 != 3)
        assert np.array_equal(got, want), (c, logs)
    assert any(len(l) == 1 for _, l in cases)


@pytest.mark.parametrize("chunk0,n", K.PREMERGE_RANGES)
def test_leaf_finish_nodes_premerge(chunk0, n):
    """root = false: an aligned range of chunks pre-merged into its subtree CV -- no ROOT flag -- from chunks and from mixed nodes"""
    rng, n_cols = random.Random(chunk0 + n), 130
    cvs = _random_cvs((chunk0 + n, n_cols, 8), 7 * chunk0 + n)
    want = K.ref_subtree(cvs, chunk0, chunk0 + n, False)
    assert n == 1 or not np.array_equal(want, K.ref_subtree(cvs, chunk0, chunk0 + n, True))
    for logs in ([0] * n, K.sampled_decomposition(chunk0, chunk0 + n, rng)):
        assert np.array_equal(_run_nodes(cvs, chunk0, logs, False, rng, n_cols, permute=True), want), (chunk0, n, logs)


def test_leaf_tree_supported_borders():
    for p in K.LEAF_TREE_PROBES:
        assert H.leaf_tree_supported(*p) == CM.leaf_tree_supported(*p), p


def _tree_leaf(fid, n_rows, n_cols, canon, layout, begin=0, count=None):
    nc = CM.leaf_n_chunks(fid, n_rows)
    idx = K.case_index(fid, n_rows, n_cols, 2)
    comm, rs, cs = K.comm_buffer(fid, idx, 0, n_rows, layout, canon)
    return idx, H.Leaf(fid, comm, rs, cs, n_cols, 0, n_rows, n_rows, begin, nc if count is None else count, nc, canon)


def test_leaf_tree_refuses_what_it_does_not_support():
    """launch_leaf_tree answers hipErrorInvalidValue -- and writes nothing -- outside leaf_tree_supported"""
    for fid, n_rows, n_cols, np2, begin, count in ((0, 10, 64, 64, 0, None), (0, 10, 192, 256, 0, None), (3, 10, 100, 128, 0, None),
                                                   (1, 130, 256, 256, 0, None), (0, 130, 256, 256, 0, 1), (0, 130, 256, 256, 1, 1),
                                                   (0, 130, 256, 512, 0, None)):
        _, leaf = _tree_leaf(fid, n_rows, n_cols, False, "row", begin, count)
        assert not CM.leaf_tree_supported(n_cols, np2, begin, leaf.n_chunks_local, CM.leaf_n_chunks(fid, n_rows))
        hashes = np.full((2 * np2 - 1, 8), S, np.uint32)
        with pytest.raises(H.HipError) as e:
            H.leaf_tree(leaf, hashes, np2)
        assert e.value.code == H.HIP_ERROR_INVALID_VALUE and (hashes == S).all()


@pytest.mark.parametrize("fid,n_rows,n_cols,canon,layout", K.leaf_tree_cases())
def test_leaf_tree(fid, n_rows, n_cols, canon, layout):
    """leaf digests and six levels in one launch, the rest of `hashes` untouched; then launch_merkle_tree_from(6) completes the tree"""
    nc, mlen = CM.leaf_n_chunks(fid, n_rows), CM.leaf_len(fid, n_rows)
    idx, leaf = _tree_leaf(fid, n_rows, n_cols, canon, layout)
    cvs = K.ref_chunk_cvs(K.message_words(fid, idx), mlen, range(nc), nc)
    want = np.full((2 * n_cols - 1, 8), S, np.uint32)
    want[:n_cols] = cvs[0] if nc == 1 else K.ref_parent(cvs[0], cvs[1], True)
    full = K.ref_tree(want.copy(), n_cols)
    done = sum(n_cols >> j for j in range(7))
    want[n_cols:done] = full[n_cols:done]
    hashes = np.full((2 * n_cols - 1, 8), S, np.uint32)
    H.leaf_tree(leaf, hashes, n_cols)
    assert np.array_equal(hashes, want)
    if done < 2 * n_cols - 1:
        H.merkle_tree_from(hashes, n_cols, 6)
        assert np.array_equal(hashes, full)


@pytest.mark.parametrize("levels_done", [0, 6])
def test_merkle_tree_from(levels_done):
    """every width: the whole hashes array is the reference's, the levels below levels_done are as given, root_out is the last slot (its
    eight words only), and the run without a root_out agrees"""
    g = np.random.default_rng(levels_done)
    for np2 in (K.TREE_NP2 if levels_done == 0 else K.FUSED_NP2):
        given = sum(np2 >> j for j in range(levels_done + 1))
        base = np.full((2 * np2 - 1, 8), S, np.uint32)
        base[:np2] = g.integers(0, 1 << 32, (np2, 8), dtype=np.uint64).astype(np.uint32)
        want = K.ref_tree(base.copy(), np2)
        base[:given] = want[:given]                            # the lower levels, reference-computed; above them sentinels
        assert given < 2 * np2 - 1                              # (128 leaves and six levels: one level is left)
        h1, root = base.copy(), np.full(16, S, np.uint32)
        H.merkle_tree_from(h1, np2, levels_done, root)
        assert np.array_equal(h1, want), np2
        assert np.array_equal(root[:8], want[-1]) and (root[8:] == S).all(), np2
        h2 = base.copy()
        H.merkle_tree_from(h2, np2, levels_done)
        assert np.array_equal(h2, want), np2


@pytest.mark.parametrize("np2", K.PATH_NP2)
def test_gather_paths(np2):
    g = np.random.default_rng(np2)
    hashes = g.integers(0, 1 << 32, (2 * np2 - 1, 8), dtype=np.uint64).astype(np.uint32)
    depth = np2.bit_length() - 1
    cols = np.array([0, np2 - 1, np2 // 2, max(0, np2 // 2 - 1)] + [int(x) for x in g.integers(0, np2, 60)], np.uint64)
    for path_len in sorted({depth, max(1, depth - 1)}):
        paths = np.full((len(cols), path_len, 8), S, np.uint32)
        H.gather_paths(hashes, np2, path_len, cols, paths)
        assert np.array_equal(paths, K.ref_paths(hashes, np2, path_len, cols))

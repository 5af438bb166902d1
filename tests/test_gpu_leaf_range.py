"""The resumable column hash of SHA3-256 / Keccak-256 / SHA-256 / BLAKE2b (launch_*_leaves_range of lcpc_amd/csrc/kernels.h), launched
directly through tests/lr_harness.py a block range at a time and compared with hashlib (Keccak-256: the sponge of tests/digest_more.py)
over bytes built here -- never with the one-shot kernel.  Shapes: 1 / 255 / 256 / 257 columns, every row count from one row to three
groups and two rows, all four fields, canonical and stored comm (tests/test_leaf_range_cases.py holds the tables and checks, without a
GPU, that they reach every block edge).

Every launch but a chain's last is handed a comm that ENDS with the last row its blocks hold a byte of: the harness proves from its own
index check that no later row is addressed, as the host-memory commit needs (commit.cpp hashes behind each row batch, while the rows of
the next one do not exist yet).  The state and the digests sit between sentinel words, compared whole after every launch."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import lr_harness as H  # noqa: E402
import test_leaf_range_cases as T  # noqa: E402

pytestmark = pytest.mark.gpu
S, G = T.SENTINEL, T.GUARD


class Chain:
    """one column hash of a case, launched range by range into sentinel-guarded buffers that persist between the launches"""

    def __init__(self, digest, fid, n_rows, n_cols, canon):
        self.digest, self.fid, self.n_rows, self.n_cols, self.canon = digest, fid, n_rows, n_cols, canon
        self.sw, self.dw = H.SHAPE[digest][2:]
        self.nb = T.n_blocks(digest, fid, n_rows)
        self.comm = T.comm_of(fid, n_rows, n_cols, canon)                      # (n_rows, n_cols, L)
        self.state = np.full(2 * G + self.sw * n_cols, S, np.uint32)
        self.out = np.full(2 * G + self.dw * n_cols, S, np.uint32)

    def run(self, b0, b1, comm=None):
        """blocks [b0, b1) on a comm cut behind the last row they need; asserts that nothing but the launch's own region changed"""
        if comm is None:
            comm = self.comm
        last = T.last_row_of(self.digest, self.fid, self.n_rows, b1)
        comm = comm[:1 if last is None else last + 1]
        state0, out0 = self.state.copy(), self.out.copy()
        H.leaf_range(self.digest, self.fid, np.ascontiguousarray(comm).reshape(-1, comm.shape[2]), self.n_cols, 1, self.n_cols, self.n_rows,
                     b0, b1, self.canon, self.state, G, self.out, G)
        assert (self.state[:G] == S).all() and (self.state[-G:] == S).all() and (self.out[:G] == S).all() and (self.out[-G:] == S).all()
        if b1 == self.nb and b1 > b0:
            assert np.array_equal(self.state, state0), "the final range leaves the state alone"
        else:
            assert np.array_equal(self.out, out0), "a range that is not the final one leaves the digests alone"
            if b0 == b1:
                assert np.array_equal(self.state, state0), "an empty range writes nothing"
        return self

    def digests(self):
        return self.out[G:-G].reshape(self.n_cols, self.dw)

    def saved(self):
        return self.state[G:-G].copy()


def _want(digest, fid, n_rows, n_cols):
    return T.ref_digests(digest, fid)[n_rows][:n_cols]


@pytest.mark.parametrize("n_cols", T.N_COLS)
@pytest.mark.parametrize("fid", T.FIDS)
@pytest.mark.parametrize("digest", T.DIGESTS)
def test_two_and_three_range_splits(digest, fid, n_cols):
    """every row count, both comm forms: the whole range in one launch (the state keeps its sentinel), the range split in two at every
    block boundary, and a sample of three-range splits with a one-block middle range, all give hashlib's digests"""
    for n_rows in range(1, T.max_rows(digest) + 1):
        want = _want(digest, fid, n_rows, n_cols)
        nb = T.n_blocks(digest, fid, n_rows)
        for canon in (True, False):
            c = Chain(digest, fid, n_rows, n_cols, canon).run(0, nb)
            assert np.array_equal(c.digests(), want), ("one range", n_rows, canon)
            assert (c.state == S).all()
            for b in range(1, nb):
                c = Chain(digest, fid, n_rows, n_cols, canon).run(0, b).run(b, nb)
                assert np.array_equal(c.digests(), want), ("split", n_rows, canon, b)
            for a, b in T.three_way(nb, n_rows):
                c = Chain(digest, fid, n_rows, n_cols, canon).run(0, a).run(a, b).run(b, nb)
                assert np.array_equal(c.digests(), want), ("three ranges", n_rows, canon, a, b)


@pytest.mark.parametrize("fid", T.FIDS)
@pytest.mark.parametrize("digest", T.DIGESTS)
def test_state_does_not_depend_on_rows_outside_the_range(digest, fid):
    """range 1 on a full-height comm whose rows behind the range hold garbage saves the state it saves from a comm cut behind the range,
    and from one with other garbage; with the rows restored, range 2 gives hashlib's digests from either"""
    n_cols = 257
    g = np.random.default_rng([T.DIGESTS.index(digest), fid])
    for n_rows in (T.GROUP[digest] + 3, T.max_rows(digest)):
        nb = T.n_blocks(digest, fid, n_rows)
        want = _want(digest, fid, n_rows, n_cols)
        for canon in (True, False):
            for b in sorted({1, nb // 2, nb - 1} - {0}):
                last = T.last_row_of(digest, fid, n_rows, b)
                first_free = 0 if last is None else last + 1
                cut = Chain(digest, fid, n_rows, n_cols, canon).run(0, b)
                states = []
                for fill in (0xFFFFFFFFFFFFFFFF, None):
                    c = Chain(digest, fid, n_rows, n_cols, canon)
                    dirty = c.comm.copy()
                    dirty[first_free:] = np.uint64(fill) if fill is not None else g.integers(0, 1 << 63, dirty[first_free:].shape, dtype=np.uint64)
                    # (the harness still cuts comm behind the range: the garbage rows are handed over by a launch of its own below)
                    c.run(0, b, comm=dirty)
                    states.append(c.saved())
                    full = np.ascontiguousarray(dirty).reshape(-1, dirty.shape[2])
                    H.leaf_range(digest, fid, full, n_cols, 1, n_cols, n_rows, 0, b, canon, c.state, G, c.out, G)     # comm of full height
                    assert np.array_equal(c.saved(), states[-1]) and (c.out == S).all()
                    c.run(b, nb)                                                                                 # the rows are back
                    assert np.array_equal(c.digests(), want), (n_rows, canon, b)
                assert np.array_equal(states[0], cut.saved()) and np.array_equal(states[1], cut.saved()), (n_rows, canon, b)


@pytest.mark.parametrize("digest", T.DIGESTS)
def test_batch_boundaries_of_the_host_commit(digest):
    """the ranges lcpc_commit makes of 16 row batches (blocks all of whose rows are encoded), each on a comm that ends with its batch, for
    row counts whose batches end inside a block, on a block edge and leave empty ranges behind"""
    n_cols = 256
    for fid in T.FIDS:
        for n_rows in (16, T.max_rows(digest) - 1, T.max_rows(digest)):
            rows_per = -(-n_rows // 16)
            c = Chain(digest, fid, n_rows, n_cols, fid == 3)
            done = 0
            for r1 in list(range(rows_per, n_rows, rows_per)) + [n_rows]:
                b = T.blocks_ready(digest, fid, n_rows, r1)
                last = T.last_row_of(digest, fid, n_rows, b)
                assert r1 == n_rows or last is None or last < r1
                c.run(done, b)
                done = b
            assert done == c.nb and np.array_equal(c.digests(), _want(digest, fid, n_rows, n_cols)), (fid, n_rows)


def test_empty_ranges_and_refused_calls_write_nothing():
    for digest in T.DIGESTS:
        c = Chain(digest, 1, 20, 5, False)
        for b in (0, 1, c.nb):
            c.run(b, b)
        assert (c.state == S).all() and (c.out == S).all()
        with pytest.raises(H.BadArgs):
            c.run(0, c.nb + 1)
        with pytest.raises(H.BadArgs):
            c.run(2, 1)
        short = c.comm[:1]
        with pytest.raises(H.BadArgs):
            H.leaf_range(digest, 1, np.ascontiguousarray(short).reshape(-1, 2), 5, 1, 5, 20, 0, c.nb, False, c.state, G, c.out, G)
        with pytest.raises(H.BadArgs):
            H.leaf_range(digest, 1, c.comm.reshape(-1, 2), 5, 1, 5, 20, 0, 1, False, c.state, G, c.out, G + 2)      # digests off their alignment
        assert (c.state == S).all() and (c.out == S).all()

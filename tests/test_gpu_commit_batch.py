"""lcpcx_commit_batch_device (include/lcpc_hip_batch.h): many equal-shape polynomials committed in one pipeline.

The reference is the existing path: every polynomial committed alone with lcpc_commit_device into a fresh object.  Each member
of a batch must equal it bit for bit -- root, the whole `hashes`, comm, coeffs, dims -- and must behave as a commitment of its
own afterwards.  Inputs come from random_coeffs_device (Field::random: the top of the field occurs).  Shapes are the smallest at
which each path of batch.cpp exists (chunks per leaf message = ceil((32 + F n_rows) / 1024), F = 8 L bytes)."""
import ctypes as C

import numpy as np
import pytest
import torch

from common import mk_transcript
from lcpc_amd import (BORROW_COEFFS, ERR_ARG, ERR_STATE, LcCommit, LcEvalProof, LcpcError, LigeroEncoding, SdigEncoding, Transcript,
                      _lib, commit_batch)

pytestmark = pytest.mark.gpu


def polys(enc, n_batch, n_coeffs, seed, stride=None):
    """[n_batch, stride * L] int64 on the device: polynomial i in the first n_coeffs elements of row i, poison behind it"""
    stride = n_coeffs if stride is None else stride
    t = enc.random_coeffs_device(n_batch * stride, seed=seed).reshape(n_batch, stride * enc.L)
    if stride > n_coeffs:
        t[:, n_coeffs * enc.L:] = -1          # all-ones limbs: not a reduced element; must never be read
    torch.cuda.synchronize()
    return t


def singles(enc, t, n_coeffs):
    return [LcCommit.commit_device(t[i].data_ptr(), n_coeffs, enc) for i in range(t.shape[0])]


def assert_same(got, want, what=""):
    assert (got.n_rows, got.n_per_row, got.n_cols, got.n_hashes) == (want.n_rows, want.n_per_row, want.n_cols, want.n_hashes), what
    assert got.get_root() == want.get_root(), what
    assert np.array_equal(got.hashes(), want.hashes()), what
    assert np.array_equal(got.comm(), want.comm()), what
    assert np.array_equal(got.coeffs(), want.coeffs()), what


def check_batch(enc, n_batch, n_coeffs, seed, stride=None, borrow=False):
    t = polys(enc, n_batch, n_coeffs, seed, stride)
    want = singles(enc, t, n_coeffs)
    got, roots = commit_batch(enc, t, n_coeffs=n_coeffs, borrow=borrow, return_roots=True)
    assert len(got) == n_batch
    for i in range(n_batch):
        assert roots[i] == want[i].get_root(), i
        assert_same(got[i], want[i], i)
    return t, got, want


def ligero(fid, n_per_row, n_cols, **kw):
    return LigeroEncoding.new_from_dims(fid, n_per_row, n_cols, **kw)


# (field, encoder, n_coeffs): shapes whose hash is leaf_tree_kernel's batch form (np2 == n_cols >= 128, <= 2 chunks)
TREE_SHAPES = {
    "ft63_2^16": lambda: (LigeroEncoding.new(0, 1 << 16), 1 << 16),           # C1's shape: one chunk per leaf
    "ft255_2^12": lambda: (LigeroEncoding.new(3, 1 << 12), 1 << 12),           # one chunk
    "ft255_32rows": lambda: (ligero(3, 64, 128), 32 * 64),                     # 32 + 32 * 32 = 1056 bytes: two chunks
    "ft127_2^12": lambda: (LigeroEncoding.new(1, 1 << 12), 1 << 12),
    "ft191_2^12": lambda: (LigeroEncoding.new(2, 1 << 12), 1 << 12),
    "ft191_60rows": lambda: (ligero(2, 64, 128), 60 * 64),                     # 1472 bytes: two chunks, an element straddles them
}
# shapes hashed by the batch forms of leaf_chunk_kernel (+ leaf_finish_kernel when a leaf has several chunks)
CHUNK_SHAPES = {
    "ft255_64rows_3chunks": lambda: (ligero(3, 64, 128), 64 * 64),             # 2080 bytes: three chunks
    "ft191_100rows_3chunks": lambda: (ligero(2, 64, 128), 100 * 64),           # 2432 bytes: three chunks, straddled twice
    "ft63_64cols_1chunk": lambda: (ligero(0, 32, 64), 8 * 32),                 # n_cols = 64 < leaf_tree's minimum; digests directly
    "ft255_64cols_2chunks": lambda: (ligero(3, 32, 64), 40 * 32),              # the same with a fold
}
# batches with more than 65536 (column, chunk) pairs in all -- 2048 columns x 3 chunks x 16 members = 98304 -- where the batched chunk
# kernel runs one lane per column while each single commit (6144 pairs) runs its quad form: (field, n_rows) on 1024 x 2048 encoders
LANE_SHAPES = {
    "ft255_canon": (3, 64),       # 2080 bytes; Ft255's comm holds canonical values
    "ft63": (0, 256),             # 2080 bytes; Montgomery-form comm, reduced in the hash
    "ft191": (2, 100),            # 2432 bytes; elements straddle both chunk boundaries
}


@pytest.mark.parametrize("shape", sorted(LANE_SHAPES))
def test_lane_per_column_chunk_path_equals_single_commits(shape):
    fid, n_rows = LANE_SHAPES[shape]
    enc = ligero(fid, 1024, 2048)
    chunks = (32 + 8 * enc.L * n_rows + 1023) // 1024
    assert chunks == 3 and enc.n_cols * chunks * 16 > 65536 >= enc.n_cols * chunks
    check_batch(enc, 16, n_rows * 1024, 31)


@pytest.mark.parametrize("shape", sorted(TREE_SHAPES))
def test_tree_path_equals_single_commits(shape):
    enc, n = TREE_SHAPES[shape]()
    check_batch(enc, 3, n, 11)


@pytest.mark.parametrize("shape", sorted(CHUNK_SHAPES))
def test_chunk_path_equals_single_commits(shape):
    enc, n = CHUNK_SHAPES[shape]()
    check_batch(enc, 3, n, 12)


@pytest.mark.parametrize("n_batch", [1, 2, 3, 7, 64])
def test_batch_sizes(n_batch):
    enc = LigeroEncoding.new(3, 1 << 12)
    check_batch(enc, n_batch, 1 << 12, 13)
    enc2, n2 = CHUNK_SHAPES["ft255_64rows_3chunks"]()
    check_batch(enc2, n_batch, n2, 14)


@pytest.mark.parametrize("shape", ["ft63_2^16", "ft255_32rows", "ft191_100rows_3chunks", "ft255_64cols_2chunks"])
def test_ragged_and_strided_inputs(shape):
    enc, n = dict(TREE_SHAPES, **CHUNK_SHAPES)[shape]()
    check_batch(enc, 3, n - 5, 15)                         # a power of two (whole rows) minus 5: the last row's tail reads as zero
    check_batch(enc, 3, n, 16, stride=n + 37)              # whole rows, poison between the polynomials
    check_batch(enc, 3, n - 5, 17, stride=n + 3)           # both


@pytest.mark.parametrize("stride_extra", [0, 64])
def test_borrowed_coeffs(stride_extra):
    enc = LigeroEncoding.new(3, 1 << 12)
    n = 1 << 12
    t, got, want = check_batch(enc, 3, n, 18, stride=n + stride_extra, borrow=True)
    for i, cm in enumerate(got):
        mine = t[i, :n * enc.L].cpu().numpy().view(np.uint64).reshape(n, enc.L)
        assert np.array_equal(cm.coeffs(), mine)
    # the members read the caller's buffer, not a copy: what it holds now is what they return
    t[1, :enc.L] = 5
    torch.cuda.synchronize()
    assert np.array_equal(got[1].coeffs()[0], np.full(enc.L, 5, np.uint64))
    # ragged rows: the flag is not honoured, as for the single commit
    t2, got2, _ = check_batch(enc, 2, n - 5, 19, borrow=True)
    before = got2[0].coeffs().copy()
    t2[0, :enc.L] = 5
    torch.cuda.synchronize()
    assert np.array_equal(got2[0].coeffs(), before)


def test_roots_against_the_oracle(oracle):
    O = oracle
    fid, n = 3, 1 << 12
    enc, oenc = LigeroEncoding.new(fid, n), O.Encoding.ligero(fid, n)
    t = polys(enc, 3, n, 20)
    _, roots = commit_batch(enc, t, return_roots=True)
    for i in range(3):
        coeffs = t[i].cpu().numpy().view(np.uint64).reshape(n, enc.L)
        assert roots[i] == O.Commit.commit(coeffs, oenc).get_root(), i


@pytest.mark.parametrize("shape", ["ft63_2^16", "ft255_32rows", "ft255_64rows_3chunks", "ft63_64cols_1chunk"])
def test_launch_counts_do_not_scale_with_the_batch(shape):
    """what fails if the "batch" is a loop: hash + tree launches of 64 members = those of one commit; so the encode's on whole rows"""
    enc, n = dict(TREE_SHAPES, **CHUNK_SHAPES)[shape]()
    t = polys(enc, 64, n, 21)
    one = LcCommit(enc)
    one.set_timing()
    LcCommit.commit_device(t[0].data_ptr(), n, enc, into=one)
    t1 = one.timings()
    cms = [LcCommit(enc) for _ in range(64)]
    cms[0].set_timing()
    commit_batch(enc, t, into=cms)
    for cm in (cms[0], cms[63]):                           # the batch's figures, in every member
        tb = cm.timings()
        assert tb.hash_launches + tb.merkle_launches == t1.hash_launches + t1.merkle_launches > 0
        assert tb.encode_launches == t1.encode_launches > 0
        assert tb.total_ms > 0
    assert_same(cms[63], LcCommit.commit_device(t[63].data_ptr(), n, enc))
    # ragged: one placement launch more, whatever the batch size
    commit_batch(enc, t[:, :(n - 5) * enc.L].contiguous(), into=cms)
    assert cms[5].timings().encode_launches == t1.encode_launches + 1
    assert cms[5].timings().hash_launches + cms[5].timings().merkle_launches == t1.hash_launches + t1.merkle_launches


@pytest.mark.parametrize("kind", ["brakedown", "sha256"])
def test_member_by_member_encoders(kind):
    fid, n = 3, 1 << 12
    enc = SdigEncoding.new(fid, n, 7) if kind == "brakedown" else LigeroEncoding.new(fid, n, digest="sha256")
    check_batch(enc, 3, n, 22)
    check_batch(enc, 3, n - 5, 23, stride=n + 9)


def test_members_are_real_commitments(oracle):
    O = oracle
    fid, n = 3, 1 << 12
    enc = LigeroEncoding.new(fid, n)
    nco = enc.get_n_col_opens()
    t = polys(enc, 3, n, 24)
    want = singles(enc, t, n)
    cms, roots = commit_batch(enc, t, return_roots=True)
    # prove on member 2: the single commit's bytes; the proof verifies against the root the batch call reported
    outer, inner = O.random_elems(fid, cms[2].n_rows, 31), O.random_elems(fid, cms[2].n_per_row, 32)
    pf = cms[2].prove(outer, enc, mk_transcript(Transcript, roots[2], nco)).to_bytes()
    assert pf == want[2].prove(outer, enc, mk_transcript(Transcript, roots[2], nco)).to_bytes()
    LcEvalProof.from_bytes(pf, enc.L).verify(roots[2], outer, inner, enc, mk_transcript(Transcript, roots[2], nco))
    vals, paths = cms[2].open_columns([0, 5, enc.n_cols - 1])
    wv, wp = want[2].open_columns([0, 5, enc.n_cols - 1])
    assert np.array_equal(vals, wv) and np.array_equal(paths, wp)
    assert np.array_equal(cms[0].eval_outer(outer), want[0].eval_outer(outer))
    # member 1 refilled alone at another n_coeffs: members 0 and 2 stay readable and unchanged
    t1 = polys(enc, 1, 3 * n - 5, 25)
    LcCommit.commit_device(t1[0].data_ptr(), 3 * n - 5, enc, into=cms[1])
    assert_same(cms[1], LcCommit.commit_device(t1[0].data_ptr(), 3 * n - 5, enc))
    assert_same(cms[0], want[0])
    assert_same(cms[2], want[2])
    # destroyed in the order 1, 0, 2 (the last one frees what they shared), then another batch
    h = [cm._h for cm in cms]
    for i in (1, 0, 2):
        _lib.lib().lcpc_commit_destroy(h[i])
        cms[i]._h = None                                   # (lcpc_commit_destroy(NULL) is a no-op: __del__)
        if i == 1:
            assert_same(cms[0], want[0])
            assert_same(cms[2], want[2])
    check_batch(enc, 3, n, 26)


def test_refill_on_a_second_stream_without_roots():
    """the same members refilled by a second batch of new data that is only enqueued (NULL roots) on a non-blocking stream:
    lcpc_get_root and the other readers must wait for the members' completion events"""
    enc, n = TREE_SHAPES["ft63_2^16"]()
    t = polys(enc, 7, n, 27)
    cms = commit_batch(enc, t)
    t2 = polys(enc, 7, n, 28)
    want = singles(enc, t2, n)
    s = torch.cuda.Stream()
    torch.cuda.synchronize()
    again = commit_batch(enc, t2, stream=s.cuda_stream, sync=False, into=cms)
    assert again[3] is cms[3]
    assert cms[6].get_root() == want[6].get_root()
    for i in range(7):
        assert_same(cms[i], want[i], i)
    # ... and a member of that batch joins other partners in a third one
    t3 = polys(enc, 2, n, 29)
    mixed = commit_batch(enc, t3, into=[cms[4], LcCommit(enc)])
    for got, w in zip(mixed, singles(enc, t3, n)):
        assert_same(got, w)
    assert_same(cms[3], want[3])
    s.synchronize()


def _raw(cms, n_batch, ptr, n_coeffs, stride, roots=None):
    arr = (C.c_void_p * max(len(cms), 1))(*cms)
    return _lib.lib().lcpcx_commit_batch_device(arr if cms is not None else None, n_batch, C.c_void_p(ptr), n_coeffs, stride, None, 0, roots)


def test_errors():
    enc, other = LigeroEncoding.new(0, 1 << 12), LigeroEncoding.new(0, 1 << 12)
    n = 1 << 12
    t = polys(enc, 2, n, 30)
    a, b, c = LcCommit(enc), LcCommit(enc), LcCommit(other)
    p = t.data_ptr()
    assert _raw([a._h, a._h], 2, p, n, 0) == ERR_ARG                  # a member listed twice
    assert _raw([a._h, c._h], 2, p, n, 0) == ERR_ARG                  # members of two encoders
    assert _raw([a._h, b._h], 0, p, n, 0) == ERR_ARG                  # n_batch == 0
    assert _raw([a._h, b._h], 2, p, n, n - 1) == ERR_ARG              # 0 < poly_stride < n_coeffs
    assert _raw([a._h, b._h], 2, p, 0, 0) == ERR_ARG                  # n_coeffs == 0
    assert _raw([a._h, b._h], 2, None, n, 0) == ERR_ARG               # NULL coefficients
    assert _raw([a._h, None], 2, p, n, 0) == ERR_ARG                  # a NULL member
    assert _lib.lib().lcpcx_commit_batch_device(None, 2, C.c_void_p(p), n, 0, None, 0, None) == ERR_ARG
    for cm in (a, b):                                                 # nothing was committed by any of these
        with pytest.raises(LcpcError) as e:
            cm.get_root()
        assert e.value.code == ERR_STATE
    sh = LigeroEncoding.new_from_dims(0, 64, 128, shard=(0, 2))
    x, y = LcCommit(sh), LcCommit(sh)
    assert _raw([x._h, y._h], 2, p, 64 * 8, 0) == ERR_STATE           # a sharded encoder
    with pytest.raises(LcpcError) as e:
        commit_batch(enc, t, n_coeffs=n + 1)                          # the wrapper passes the status on
    assert e.value.code == ERR_ARG
    assert _raw([a._h, b._h], 2, p, n, 0) == 0                        # and the same objects still take a good batch
    for got, w in zip((a._refresh(), b._refresh()), singles(enc, t, n)):
        assert_same(got, w)

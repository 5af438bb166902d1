"""lcpcx_commit_batch_device on Brakedown encoders (include/lcpc_hip_batch.h, batch.cpp): the stacked-row pipeline in both regimes.

The reference is every polynomial committed alone with lcpc_commit_device, compared as tests/test_gpu_commit_batch.py does: root, the
whole `hashes`, comm, coeffs, dims, bit for bit.  Short members (n_rows < 24, row-major comm) and position-major members (n_rows >= 24,
each its own T[pos][row] in the shared slab); a single commit of < 24 rows runs the row-major kernels while a batch of such members
with >= 24 STACKED rows runs the position-major ones, and at wide levels a single commit runs the packed-tail kernel where the batch
does not: equality covers that the paths agree.  Encoders as in tests/test_gpu_edges.py: n_cols from the oracle's get_dims."""
import numpy as np
import pytest
import torch

from common import mk_transcript
from lcpc_amd import LcCommit, LcEvalProof, SdigEncoding, Transcript, _lib, commit_batch
from test_gpu_commit_batch import assert_same, check_batch, polys, singles

pytestmark = pytest.mark.gpu
NPR = 900
_ENC = {}


def sdig(O, fid, n_per_row=NPR, digest="blake3", seed=5):
    key = (fid, n_per_row, digest, seed)
    if key not in _ENC:
        _, _, n_cols = O.Encoding.sdig_from_dims(fid, n_per_row, 0, seed).get_dims(n_per_row)
        _ENC[key] = SdigEncoding.new_from_dims(fid, n_per_row, n_cols, seed, digest=digest)
    return _ENC[key]


# (n_rows, n_batch): stacked rows below 24 (1 x 3, 7 x 3: the row-major kernels, as the single commits), just above (7 x 4) and well above
# (16 x 7 = 112 stacked rows in one wave and a partial one; 2 x 23: a wave of two members)
SHORT = [(1, 3), (7, 3), (7, 4), (7, 16), (23, 1), (23, 2)]


@pytest.mark.parametrize("fid", [0, 3])
@pytest.mark.parametrize("n_rows,n_batch", SHORT)
def test_short_members(oracle, fid, n_rows, n_batch):
    check_batch(sdig(oracle, fid), n_batch, n_rows * NPR, 100 + n_rows)


@pytest.mark.parametrize("fid,n_rows", [(3, 24), (3, 37), (3, 64), (3, 65), (0, 37), (1, 37), (2, 37)])
def test_position_major_members(oracle, fid, n_rows):
    enc = sdig(oracle, fid)
    _, got, _ = check_batch(enc, 3, n_rows * NPR, 200 + n_rows)
    assert got[0].n_rows == n_rows


def test_wide_levels_without_the_packed_tail_kernel(oracle):
    """levels of >= 8192 outputs, 37 rows: every single commit runs spmm_t_tail_kernel (tests/test_gpu_edges.py
    test_brakedown_packed_tail_rows), the batch of 74 stacked rows runs spmm_t_kernel's batch form alone"""
    enc = sdig(oracle, 3, 70000, seed=9)
    check_batch(enc, 2, 37 * 70000, 37)


@pytest.mark.parametrize("n_rows", [7, 37])
def test_ragged_and_strided_inputs(oracle, n_rows):
    enc = sdig(oracle, 3)
    n = n_rows * NPR
    check_batch(enc, 3, n - 5, 15)                         # the last row's tail reads as zero
    check_batch(enc, 3, n, 16, stride=n + 37)              # whole rows, poison between the polynomials
    check_batch(enc, 3, n - 5, 17, stride=n + 3)           # both
    check_batch(sdig(oracle, 0), 3, n - 5, 17, stride=n + 3)


@pytest.mark.parametrize("n_rows,n_batch", [(1, 2), (7, 3), (37, 3)])      # 2 stacked rows and 21: row-major kernels; 21 and 111
@pytest.mark.parametrize("stride_extra", [0, 64])
def test_borrowed_coeffs(oracle, n_rows, n_batch, stride_extra):
    enc = sdig(oracle, 3)
    n = n_rows * NPR
    t, got, _ = check_batch(enc, n_batch, n, 18, stride=n + stride_extra, borrow=True)
    for i, cm in enumerate(got):
        assert np.array_equal(cm.coeffs(), t[i, :n * enc.L].cpu().numpy().view(np.uint64).reshape(n, enc.L))
    t[1, :enc.L] = 5                                       # the members read the caller's buffer, not a copy
    torch.cuda.synchronize()
    assert np.array_equal(got[1].coeffs()[0], np.full(enc.L, 5, np.uint64))
    t2, got2, _ = check_batch(enc, 2, n - 5, 19, borrow=True)          # ragged rows: the flag is not honoured
    before = got2[0].coeffs().copy()
    t2[0, :enc.L] = 5
    torch.cuda.synchronize()
    assert np.array_equal(got2[0].coeffs(), before)


@pytest.mark.parametrize("n_rows", [7, 37])
@pytest.mark.parametrize("n_batch", [1, 2, 64])
def test_batch_sizes(oracle, n_rows, n_batch):
    check_batch(sdig(oracle, 3), n_batch, n_rows * NPR, 13)


def _timed_single(enc, t, n):
    one = LcCommit(enc)
    one.set_timing()
    LcCommit.commit_device(t[0].data_ptr(), n, enc, into=one)
    return one.timings()


def _timed_batch(enc, t, n_batch, n_coeffs=None):
    cms = [LcCommit(enc) for _ in range(n_batch)]
    cms[0].set_timing()
    commit_batch(enc, t[:n_batch], n_coeffs=n_coeffs, into=cms)
    return cms


def test_launch_counts_position_major(oracle):
    """what fails if the batch is a loop over the members: 16 members cost the launches of ONE commit, phase by phase"""
    enc = sdig(oracle, 3)
    n = 37 * NPR
    t = polys(enc, 16, n, 21)
    t1 = _timed_single(enc, t, n)
    cms = _timed_batch(enc, t, 16)
    for cm in (cms[0], cms[15]):                           # the batch's figures, in every member
        tb = cm.timings()
        assert (tb.encode_launches, tb.hash_launches, tb.merkle_launches) == (t1.encode_launches, t1.hash_launches, t1.merkle_launches)
        assert tb.encode_launches > 0 and tb.hash_launches > 0 and tb.merkle_launches > 0 and tb.total_ms > 0
    assert_same(cms[15], LcCommit.commit_device(t[15].data_ptr(), n, enc))
    # ragged: one placement launch more, whatever the batch size
    commit_batch(enc, t[:, :(n - 5) * enc.L].contiguous(), into=cms)
    tr = cms[5].timings()
    assert (tr.encode_launches, tr.hash_launches, tr.merkle_launches) == (t1.encode_launches + 1, t1.hash_launches, t1.merkle_launches)


def test_launch_counts_short_members(oracle):
    """7-row members, 28 and 112 stacked rows: the same launches, whatever the batch size"""
    enc = sdig(oracle, 3)
    n = 7 * NPR
    t = polys(enc, 16, n, 22)
    t4, t16 = _timed_batch(enc, t, 4)[3].timings(), _timed_batch(enc, t, 16)[15].timings()
    assert (t16.encode_launches, t16.hash_launches, t16.merkle_launches) == (t4.encode_launches, t4.hash_launches, t4.merkle_launches)
    assert t4.encode_launches > 0 and t4.hash_launches > 0 and t4.merkle_launches > 0


@pytest.mark.parametrize("digest", ["blake2b", "sha3_256"])
@pytest.mark.parametrize("n_rows", [7, 37])
def test_launch_counts_under_a_chained_digest(oracle, digest, n_rows):
    """the encode is the batch's; the hash and the tree run member by member (include/lcpc_hip_batch.h)"""
    enc = sdig(oracle, 3, digest=digest)
    n = n_rows * NPR
    t = polys(enc, 16, n, 23)
    t1 = _timed_single(enc, t, n)
    tb = _timed_batch(enc, t, 16)[9].timings()
    if n_rows >= 24:
        assert tb.encode_launches == t1.encode_launches > 0
    else:                                                  # 112 stacked rows take the position-major kernels: not one short commit's count,
        assert tb.encode_launches == _timed_batch(enc, t, 4)[0].timings().encode_launches > 0       # but a 4-member batch's
    assert tb.hash_launches == 16 * t1.hash_launches > 0
    assert tb.merkle_launches == 16 * t1.merkle_launches > 0
    assert tb.hash_ms > 0 and tb.merkle_ms > 0 and tb.total_ms >= tb.encode_ms > 0


@pytest.mark.parametrize("digest", ["sha3_256", "keccak256", "sha256", "blake2b"])
@pytest.mark.parametrize("n_rows", [7, 37])
def test_chained_digests(oracle, digest, n_rows):
    enc = sdig(oracle, 3, digest=digest)
    check_batch(enc, 3, n_rows * NPR, 67)
    check_batch(enc, 3, n_rows * NPR - 5, 68, stride=n_rows * NPR + 9)


def _read_all(cm, want, outer, root, enc, nco):
    assert_same(cm, want)
    assert cm.prove(outer, enc, mk_transcript(Transcript, root, nco)).to_bytes() == want.prove(outer, enc, mk_transcript(Transcript, root, nco)).to_bytes()


def test_members_are_real_commitments(oracle):
    O, fid = oracle, 3
    enc = sdig(O, fid)
    nco = enc.get_n_col_opens()
    n, n_short = 37 * NPR, 7 * NPR
    t = polys(enc, 3, n, 24)
    want = singles(enc, t, n)
    cms, roots = commit_batch(enc, t, return_roots=True)
    outer, inner = O.random_elems(fid, 37, 31), O.random_elems(fid, NPR, 32)
    # prove on member 2: the single commit's bytes; the proof verifies against the root the batch call reported
    pf = cms[2].prove(outer, enc, mk_transcript(Transcript, roots[2], nco)).to_bytes()
    assert pf == want[2].prove(outer, enc, mk_transcript(Transcript, roots[2], nco)).to_bytes()
    LcEvalProof.from_bytes(pf, enc.L).verify(roots[2], outer, inner, enc, mk_transcript(Transcript, roots[2], nco))
    cols = [0, 5, NPR - 1, NPR, enc.n_cols - 1]
    for got, w in zip(cms[2].open_columns(cols), want[2].open_columns(cols)):
        assert np.array_equal(got, w)
    assert np.array_equal(cms[0].eval_outer(outer), want[0].eval_outer(outer))
    # comm() -- the on-demand row-major copy of a position-major member -- twice, then every other reader on the same member and on
    # its partners: the copy is the member's own, the slab and the views of all three stay
    assert np.array_equal(cms[1].comm(), want[1].comm()) and np.array_equal(cms[1].comm(), want[1].comm())
    for i in (1, 0, 2):
        assert np.array_equal(cms[i].hashes(), want[i].hashes()) and np.array_equal(cms[i].coeffs(), want[i].coeffs())
        _read_all(cms[i], want[i], outer, roots[i], enc, nco)
    # the same members again, new data (the slab is reused; member 1 holds a row-major copy of the old commitment)
    t2 = polys(enc, 3, n, 25)
    want2 = singles(enc, t2, n)
    assert commit_batch(enc, t2, into=cms)[1] is cms[1]
    for i in range(3):
        _read_all(cms[i], want2[i], outer, want2[i].get_root(), enc, nco)
    # member 1 refilled alone at a short-regime shape: members 0 and 2 stay readable and unchanged
    t1 = polys(enc, 1, n_short - 5, 26)
    LcCommit.commit_device(t1[0].data_ptr(), n_short - 5, enc, into=cms[1])
    assert_same(cms[1], LcCommit.commit_device(t1[0].data_ptr(), n_short - 5, enc))
    assert_same(cms[0], want2[0])
    assert_same(cms[2], want2[2])
    # member 0 refilled alone from host memory (lcpc_commit), position-major again
    h = O.random_elems(fid, 40 * NPR - 3, 27)
    LcCommit.commit(h, enc, into=cms[0])
    assert_same(cms[0], LcCommit.commit(h, enc))
    assert_same(cms[2], want2[2])
    # member 2 joins another batch with another partner
    t3 = polys(enc, 2, n, 28)
    mixed = commit_batch(enc, t3, into=[cms[2], LcCommit(enc)])
    for got, w in zip(mixed, singles(enc, t3, n)):
        assert_same(got, w)
    # a position-major batch, then a short-regime batch into the same members, then position-major again
    commit_batch(enc, t, into=cms)
    ts = polys(enc, 3, n_short, 29)
    for got, w in zip(commit_batch(enc, ts, into=cms), singles(enc, ts, n_short)):
        assert_same(got, w)
    # ... of which member 0 is refilled alone at a position-major shape
    LcCommit.commit_device(t[0].data_ptr(), n, enc, into=cms[0])
    assert_same(cms[0], want[0])
    assert_same(cms[1], LcCommit.commit_device(ts[1].data_ptr(), n_short, enc))
    commit_batch(enc, t, into=cms)
    assert np.array_equal(cms[2].comm(), want[2].comm())
    # destroyed in the order 1, 0, 2 while the others are read (the last one frees what they shared), then another batch
    hs = [cm._h for cm in cms]
    for i in (1, 0, 2):
        _lib.lib().lcpc_commit_destroy(hs[i])
        cms[i]._h = None                                   # (lcpc_commit_destroy(NULL) is a no-op: __del__)
        if i == 1:
            assert_same(cms[0], want[0])
            assert_same(cms[2], want[2])
        if i == 0:
            assert_same(cms[2], want[2])
    check_batch(enc, 3, n, 30)

"""lcpcx_commit_batch_device under SHA3-256, Keccak-256, SHA-256 and BLAKE2b (include/lcpc_hip_batch.h): a Ligero batch runs the
batch forms of the serial-chain leaf kernels and of their tree kernels (sha3.hip, sha256.hip, blake2b.hip) -- one leaf launch and
one tree call for all members, hashes slots of the digest's own length.

The reference is the existing single path, as in tests/test_gpu_commit_batch.py: every polynomial committed alone with
lcpc_commit_device into a fresh object.  Each member of a batch must equal it bit for bit -- root, the whole `hashes`, comm, coeffs,
dims.  One member per digest is also held to a reference that never touches the GPU.  Shapes are the smallest at which each
kernel path exists: the block edges of the three leaf messages, both forms of comm, one / two / several tree launches."""
import numpy as np
import pytest
import torch

import blake2b_ref
import digest_more as DM
import digest_ref as DR
import sha3_ref
from common import mk_transcript
from lcpc_amd import LcCommit, LcEvalProof, LigeroEncoding, SdigEncoding, Transcript, _lib, commit_batch

pytestmark = pytest.mark.gpu

DIGESTS = ["sha3_256", "keccak256", "sha256", "blake2b"]
DLEN = {"sha3_256": 32, "keccak256": 32, "sha256": 32, "blake2b": 64}
FIELDS = [0, 1, 2, 3]

_ENC = {}


def ligero(fid, n_per_row, n_cols, digest):
    """one encoder per (field, dims, digest) for the whole module"""
    key = (fid, n_per_row, n_cols, digest)
    if key not in _ENC:
        _ENC[key] = LigeroEncoding.new_from_dims(fid, n_per_row, n_cols, digest=digest)
    return _ENC[key]


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
    dl = DLEN[enc.digest]
    for i in range(n_batch):
        assert len(roots[i]) == dl and roots[i] == want[i].get_root(), i
        assert_same(got[i], want[i], i)
    return t, got, want


def edge_row_counts(fid, digest):
    """every n_rows at which the digest's leaf message reaches one of its claimed block edges on this field, and n_rows = 1"""
    table = DR.edge_rows(fid) if digest in ("sha3_256", "blake2b") else DM.edge_rows(fid)
    rows = {r for (name, _), r in table.items() if name == digest and r is not None}
    assert rows, (fid, digest)
    return sorted(rows | {1})


# ---- 1. block edges: exactly full last block, one word left, padding in a block of its own, SHA-256's residue 7 ----------------------

@pytest.mark.parametrize("fid", FIELDS)
@pytest.mark.parametrize("digest", DIGESTS)
def test_block_edges(digest, fid):
    enc = ligero(fid, 64, 128, digest)
    for n_rows in edge_row_counts(fid, digest):
        check_batch(enc, 3, n_rows * 64, 40 + n_rows)


def test_block_edges_reach_what_they_claim():
    """the row counts above do hit the edges: a full last block (BLAKE2b residue 0), one word left, a padding block of its own
    (sponge / SHA-256 residue 0), SHA-256's residue 7 (on the odd-limb fields), several L-block groups and a partial one"""
    for fid in FIELDS:
        L = DR.LIMBS[fid]
        assert 0 in {DR.blake2b_residue(L, r) for r in edge_row_counts(fid, "blake2b")}
        for d in ("sha3_256", "keccak256"):
            res = {DR.sha3_residue(L, r) for r in edge_row_counts(fid, d)}
            assert 0 in res and (16 in res or L == 4)
            blocks = [(4 + L * r) // 17 + 1 for r in edge_row_counts(fid, d)]
            assert min(blocks) == 1 and max(blocks) > L and (L == 1 or any(b % L for b in blocks))
        res = {DM.sha256_residue(L, r) for r in edge_row_counts(fid, "sha256")}
        assert 0 in res and (7 in res) == (L % 2 == 1)


# ---- 2. both forms of comm for Ft63 / Ft127 / Ft191: Montgomery at 128 columns, canonical (the limb plan) at 8192 -------------------

@pytest.mark.parametrize("fid", [0, 1, 2])
@pytest.mark.parametrize("digest", DIGESTS)
def test_canonical_comm_at_8192_columns(digest, fid):
    n_rows = 5
    assert not DR.leaf_canon_in(fid, "ligero", 7, n_rows)          # the shapes of test_block_edges hash Montgomery-form comm
    assert DR.leaf_canon_in(fid, "ligero", 13, n_rows)
    check_batch(ligero(fid, 4096, 8192, digest), 3, n_rows * 4096, 50)


# ---- 3. tree launches: below one subtree, one launch that also gives the root, two launches, 16 subtrees and a top -------------------

@pytest.mark.parametrize("n_cols,fid", [(64, 1), (512, 2), (1024, 0), (8192, 3)])
@pytest.mark.parametrize("digest", DIGESTS)
def test_tree_launch_structure(digest, n_cols, fid):
    check_batch(ligero(fid, n_cols // 2, n_cols, digest), 3, 3 * (n_cols // 2), 51)


# ---- 4. batch sizes ------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n_batch", [1, 2, 7, 64])
@pytest.mark.parametrize("digest", DIGESTS)
def test_batch_sizes(digest, n_batch):
    check_batch(ligero(3, 64, 128, digest), n_batch, 9 * 64, 53)


# ---- 5. ragged, strided and borrowed inputs -------------------------------------------------------------------------------------------

@pytest.mark.parametrize("digest", DIGESTS)
def test_ragged_and_strided_inputs(digest):
    enc = ligero(2, 64, 128, digest)
    n = 10 * 64
    check_batch(enc, 3, n - 5, 54)                         # the last row's tail reads as zero
    check_batch(enc, 3, n, 55, stride=n + 37)              # whole rows, poison between the polynomials
    check_batch(enc, 3, n - 5, 56, stride=n + 3)           # both


@pytest.mark.parametrize("digest", DIGESTS)
def test_borrowed_coeffs(digest):
    enc = ligero(3, 64, 128, digest)
    n = 8 * 64
    t, got, _ = check_batch(enc, 3, n, 57, borrow=True)
    # the members read the caller's buffer, not a copy: what it holds now is what they return
    t[1, :enc.L] = 5
    torch.cuda.synchronize()
    assert np.array_equal(got[1].coeffs()[0], np.full(enc.L, 5, np.uint64))
    # ragged rows: the flag is not honoured, as for the single commit
    t2, got2, _ = check_batch(enc, 2, n - 5, 58, borrow=True)
    before = got2[0].coeffs().copy()
    t2[0, :enc.L] = 5
    torch.cuda.synchronize()
    assert np.array_equal(got2[0].coeffs(), before)


# ---- 6. what fails if the batch is a loop over the members ---------------------------------------------------------------------------

@pytest.mark.parametrize("shape", ["ft255_128cols", "ft63_1024cols"])
@pytest.mark.parametrize("digest", DIGESTS)
def test_launch_counts_do_not_scale_with_the_batch(digest, shape):
    """hash + tree launches of 64 members = those of one commit, and so the encode's on whole rows; member by member these are
    64 times a single commit's"""
    fid, n_per_row, n_rows = {"ft255_128cols": (3, 64, 9), "ft63_1024cols": (0, 512, 3)}[shape]
    enc = ligero(fid, n_per_row, 2 * n_per_row, digest)
    n = n_rows * n_per_row
    t = polys(enc, 64, n, 59)
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


# ---- 7. members are real commitments -------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("digest", DIGESTS)
def test_members_are_real_commitments(oracle, digest):
    O = oracle
    fid, n = 3, 1 << 12
    enc = LigeroEncoding.new(fid, n, digest=digest)
    nco = enc.get_n_col_opens()
    t = polys(enc, 3, n, 60)
    want = singles(enc, t, n)
    cms, roots = commit_batch(enc, t, return_roots=True)
    # prove on member 2: the single commit's bytes (BLAKE2b: 64-byte path entries); the proof verifies against the reported root
    outer, inner = O.random_elems(fid, cms[2].n_rows, 31), O.random_elems(fid, cms[2].n_per_row, 32)
    pf = cms[2].prove(outer, enc, mk_transcript(Transcript, roots[2], nco)).to_bytes()
    assert pf == want[2].prove(outer, enc, mk_transcript(Transcript, roots[2], nco)).to_bytes()
    LcEvalProof.from_bytes(pf, enc.L).verify(roots[2], outer, inner, enc, mk_transcript(Transcript, roots[2], nco))
    vals, paths = cms[2].open_columns([0, 5, enc.n_cols - 1])
    wv, wp = want[2].open_columns([0, 5, enc.n_cols - 1])
    assert paths.shape[2] == DLEN[digest]
    assert np.array_equal(vals, wv) and np.array_equal(paths, wp)
    assert np.array_equal(cms[0].eval_outer(outer), want[0].eval_outer(outer))
    # the same members at the same shape again (the slab is reused), with new data
    t2 = polys(enc, 3, n, 61)
    want2 = singles(enc, t2, n)
    commit_batch(enc, t2, into=cms)
    for i in range(3):
        assert_same(cms[i], want2[i], i)
    # member 1 refilled alone at another n_coeffs: members 0 and 2 stay readable and unchanged
    t1 = polys(enc, 1, 3 * n - 5, 62)
    LcCommit.commit_device(t1[0].data_ptr(), 3 * n - 5, enc, into=cms[1])
    assert_same(cms[1], LcCommit.commit_device(t1[0].data_ptr(), 3 * n - 5, enc))
    assert_same(cms[0], want2[0])
    assert_same(cms[2], want2[2])
    # destroyed in the order 1, 0, 2 (the last one frees what they shared), then another batch
    h = [cm._h for cm in cms]
    for i in (1, 0, 2):
        _lib.lib().lcpc_commit_destroy(h[i])
        cms[i]._h = None                                   # (lcpc_commit_destroy(NULL) is a no-op: __del__)
        if i == 1:
            assert_same(cms[0], want2[0])
            assert_same(cms[2], want2[2])
    check_batch(enc, 3, n, 63)


@pytest.mark.parametrize("digest", DIGESTS)
def test_refill_on_a_second_stream_without_roots(digest):
    """the same members refilled by a second batch that is only enqueued (NULL roots) on a non-blocking stream: lcpc_get_root and
    the other readers must wait for the members' completion events"""
    enc = ligero(0, 512, 1024, digest)
    n = 6 * 512
    cms = commit_batch(enc, polys(enc, 7, n, 64))
    t2 = polys(enc, 7, n, 65)
    want = singles(enc, t2, n)
    s = torch.cuda.Stream()
    torch.cuda.synchronize()
    again = commit_batch(enc, t2, stream=s.cuda_stream, sync=False, into=cms)
    assert again[3] is cms[3]
    assert cms[6].get_root() == want[6].get_root()
    for i in range(7):
        assert_same(cms[i], want[i], i)
    s.synchronize()


# ---- 8. one member per digest against a reference that does not touch the GPU --------------------------------------------------------

@pytest.mark.parametrize("digest,fid", [("sha3_256", 2), ("keccak256", 0), ("sha256", 1), ("blake2b", 3)])
def test_member_against_independent_reference(oracle, digest, fid):
    O = oracle
    n_rows, n_per_row, n_cols = 7, 64, 128
    n = n_rows * n_per_row
    enc = ligero(fid, n_per_row, n_cols, digest)
    t = polys(enc, 3, n, 66)
    cms, roots = commit_batch(enc, t, return_roots=True)
    coeffs = t[1].cpu().numpy().view(np.uint64).reshape(n, enc.L)
    oc = O.Commit.commit(coeffs, O.Encoding.ligero_from_dims(fid, n_per_row, n_cols))       # the CPU oracle's comm (Montgomery form)
    assert (oc.n_rows, oc.n_cols) == (n_rows, n_cols)
    if digest == "sha3_256":
        want = sha3_ref.tree(sha3_ref.leaves(O, fid, oc.comm(), n_rows, n_cols))
    elif digest == "blake2b":
        want = blake2b_ref.tree(blake2b_ref.leaves(O, fid, oc.comm(), n_rows, n_cols))
    else:
        want = [r.tobytes() for r in DM.hashes_ref(digest, O, fid, oc.comm(), n_rows, n_cols)]
    got = cms[1].hashes()
    assert got.shape == (len(want), DLEN[digest])
    bad = [i for i in range(len(want)) if got[i].tobytes() != want[i]]
    assert not bad, bad[:8]
    assert roots[1] == want[-1] == cms[1].get_root()


# ---- 9. Brakedown stays member by member under a chained digest -------------------------------------------------------------------

def test_brakedown_under_a_chained_digest():
    fid, n = 3, 1 << 12
    enc = SdigEncoding.new(fid, n, 7, digest="blake2b")
    check_batch(enc, 3, n, 67)
    check_batch(enc, 3, n - 5, 68, stride=n + 9)
    # member by member: the launch counts are the sums over the members
    t = polys(enc, 4, n, 69)
    one = LcCommit(enc)
    one.set_timing()
    LcCommit.commit_device(t[0].data_ptr(), n, enc, into=one)
    cms = [LcCommit(enc) for _ in range(4)]
    cms[0].set_timing()
    commit_batch(enc, t, into=cms)
    assert cms[0].timings().hash_launches == 4 * one.timings().hash_launches

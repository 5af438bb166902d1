"""The one-shot and batch column hash and the Merkle tree of SHA3-256 / Keccak-256 / SHA-256 / BLAKE2b (launch_chain_leaves,
launch_chain_leaves_batch, launch_chain_merkle_tree[_batch] of lcpc_amd/csrc/kernels.h), launched directly through tests/lr_harness.py
and compared with hashlib (Keccak-256: the sponge of tests/digest_more.py) -- never with another kernel.  These launchers share their
column body (lcpc_amd/csrc/chain_dev.h) with the resumable form that tests/test_gpu_leaf_range.py drives; whole commits reach them only
at the shapes an encoder makes.

Leaves: 1 / 255 / 257 columns, every row count from one row to three groups and two rows, all four fields, canonical and stored comm
(the references and the operand pool of tests/test_leaf_range_cases.py).  The batch form runs three members that hold different columns
of the pool, with member strides larger than a member's extent; the digests sit between sentinel words, compared whole.
Tree: 2 / 256 / 512 / 1024 leaves -- one level, fewer than nine, exactly nine, and a second launch -- one-shot and as a batch of one and
of three members, with and without a root_out; every node of every level is compared with hashlib of its two children."""
import functools
import hashlib
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import lr_harness as H  # noqa: E402
import test_leaf_range_cases as T  # noqa: E402

pytestmark = pytest.mark.gpu
S, G = T.SENTINEL, T.GUARD
N_COLS = (1, 255, 257)
N_BATCH = 3
HIP_ERROR_INVALID_VALUE = 1


def _member_cols(n_cols, i):
    """the pool columns member i holds: another window of the MAX_COLS reference columns per member"""
    return (np.arange(n_cols) + 85 * i) % T.MAX_COLS


def _words(comm):
    return np.ascontiguousarray(comm).view(np.uint32).reshape(-1)


@pytest.mark.parametrize("n_cols", N_COLS)
@pytest.mark.parametrize("fid", T.FIDS)
@pytest.mark.parametrize("digest", T.DIGESTS)
def test_one_shot_and_batch_leaves(digest, fid, n_cols):
    dw = H.SHAPE[digest][3]
    ext_out = dw * n_cols
    out_stride = ext_out + 8                                      # two sentinel quads between the members' digests
    for n_rows in range(1, T.max_rows(digest) + 1):
        ref = T.ref_digests(digest, fid)[n_rows]
        for canon in (True, False):
            full = T.comm_of(fid, n_rows, T.MAX_COLS, canon)      # (n_rows, MAX_COLS, L)
            # one-shot
            out = np.full(2 * G + ext_out, S, np.uint32)
            H.leaves(digest, fid, _words(full[:, :n_cols]), n_cols, 1, n_cols, n_rows, canon, out, G)
            assert (out[:G] == S).all() and (out[-G:] == S).all()
            assert np.array_equal(out[G:-G].reshape(n_cols, dw), ref[:n_cols]), ("one-shot", n_rows, canon)
            if fid == 3 and not canon:
                continue                                          # the batch form of this kernel does not exist: refused, below
            # batch: member i at comm_stride * i, its extent rounded up to 16 bytes plus one quad nobody reads
            members = [_words(full[:, _member_cols(n_cols, i)]) for i in range(N_BATCH)]
            comm_stride = (members[0].size + 3) // 4 * 4 + 4
            comm = np.full(N_BATCH * comm_stride, S, np.uint32)
            for i, m in enumerate(members):
                comm[i * comm_stride:i * comm_stride + m.size] = m
            out = np.full(2 * G + N_BATCH * out_stride, S, np.uint32)
            H.leaves(digest, fid, comm, n_cols, 1, n_cols, n_rows, canon, out, G, n_batch=N_BATCH, comm_stride=comm_stride, out_stride=out_stride)
            assert (out[:G] == S).all() and (out[-G:] == S).all()
            body = out[G:-G].reshape(N_BATCH, out_stride)
            assert (body[:, ext_out:] == S).all(), ("between the members", n_rows, canon)
            for i in range(N_BATCH):
                assert np.array_equal(body[i, :ext_out].reshape(n_cols, dw), ref[_member_cols(n_cols, i)]), ("batch", n_rows, canon, i)


@pytest.mark.parametrize("digest", T.DIGESTS)
def test_batch_of_one_and_position_major(digest):
    """a batch of one member with zero strides is the one-shot call; a position-major comm (column stride n_rows) gives the same digests"""
    fid, n_cols, n_rows = 1, 257, T.GROUP[digest] + 3
    dw = H.SHAPE[digest][3]
    ref = T.ref_digests(digest, fid)[n_rows][:n_cols]
    comm = T.comm_of(fid, n_rows, n_cols, False)
    for kw in (dict(n_batch=1), dict()):
        out = np.full(2 * G + dw * n_cols, S, np.uint32)
        H.leaves(digest, fid, _words(comm), n_cols, 1, n_cols, n_rows, False, out, G, **kw)
        assert (out[:G] == S).all() and (out[-G:] == S).all() and np.array_equal(out[G:-G].reshape(n_cols, dw), ref)
        out = np.full(2 * G + dw * n_cols, S, np.uint32)
        H.leaves(digest, fid, _words(comm.transpose(1, 0, 2)), 1, n_rows, n_cols, n_rows, False, out, G, **kw)
        assert (out[:G] == S).all() and (out[-G:] == S).all() and np.array_equal(out[G:-G].reshape(n_cols, dw), ref)


@pytest.mark.parametrize("digest", T.DIGESTS)
def test_refused_batch_call_writes_nothing(digest):
    """nl == 8 with a stored (non-canonical) comm has no batch kernel: hipErrorInvalidValue, and not a word of the digests changes"""
    n_cols, n_rows = 5, 20
    dw = H.SHAPE[digest][3]
    comm = _words(T.comm_of(3, n_rows, n_cols, False))
    stride = comm.size
    out = np.full(2 * G + N_BATCH * dw * n_cols, S, np.uint32)
    with pytest.raises(H.HipError) as e:
        H.leaves(digest, 3, np.tile(comm, N_BATCH), n_cols, 1, n_cols, n_rows, False, out, G, n_batch=N_BATCH, comm_stride=stride, out_stride=dw * n_cols)
    assert e.value.code == HIP_ERROR_INVALID_VALUE and (out == S).all()
    with pytest.raises(H.BadArgs):                    # members that overlap never reach the launcher
        H.leaves(digest, 1, np.zeros(4 * n_cols * n_rows * N_BATCH, np.uint32), n_cols, 1, n_cols, n_rows, True, out, G, n_batch=N_BATCH,
                 comm_stride=4 * n_cols * n_rows, out_stride=dw * n_cols - 4)
    assert (out == S).all()


# ---- the tree --------------------------------------------------------------------------------------------------------------------------
NP2 = (2, 256, 512, 1024)


def _hash_pairs(digest, pairs):
    """(n, 2 dw words) uint32 -> (n, dw) uint32: D(left || right) of every row"""
    b = np.ascontiguousarray(pairs).view(np.uint8).reshape(len(pairs), -1)
    if digest == "keccak256":
        d = T.keccak256_ragged([b])[0]
    else:
        fn = {"sha3_256": hashlib.sha3_256, "sha256": hashlib.sha256, "blake2b": hashlib.blake2b}[digest]
        d = T._hashlib_many(fn, b)
    return np.ascontiguousarray(d).view("<u4").astype(np.uint32)


@functools.lru_cache(maxsize=None)
def tree_ref(digest, np2, member):
    """[2 np2 - 1][dw] uint32: random leaves and every level above them by hashlib; computed once, never written to"""
    dw = H.SHAPE[digest][3]
    g = np.random.default_rng([T.DIGESTS.index(digest), np2, member])
    levels = [g.integers(0, 1 << 32, (np2, dw), dtype=np.uint32)]
    while len(levels[-1]) > 1:
        levels.append(_hash_pairs(digest, levels[-1].reshape(-1, 2 * dw)))
    out = np.concatenate(levels)
    assert out.shape == (2 * np2 - 1, dw)
    out.setflags(write=False)
    return out


@pytest.mark.parametrize("np2", NP2)
@pytest.mark.parametrize("digest", T.DIGESTS)
def test_merkle_tree_every_level(digest, np2):
    dw = H.SHAPE[digest][3]
    ext = (2 * np2 - 1) * dw
    stride = (ext + 3) // 4 * 4 + 8                               # sentinel words between the members' arrays
    for n_batch in (0, 1, 3):                                     # 0: the one-shot launcher
        members = max(1, n_batch)
        for with_root in (True, False):
            hashes = np.full(2 * G + members * stride, S, np.uint32)
            for i in range(members):
                hashes[G + i * stride:G + i * stride + np2 * dw] = tree_ref(digest, np2, i)[:np2].reshape(-1)
            root = np.full(2 * G + members * dw, S, np.uint32) if with_root else None
            H.merkle_tree(digest, np2, hashes, G, root, G, n_batch=n_batch, hashes_stride=stride if n_batch else 0)
            assert (hashes[:G] == S).all() and (hashes[-G:] == S).all()
            body = hashes[G:-G].reshape(members, stride)
            assert (body[:, ext:] == S).all(), ("between the members", n_batch, with_root)
            for i in range(members):
                want = tree_ref(digest, np2, i)
                got = body[i, :ext].reshape(-1, dw)
                bad = np.nonzero((got != want).any(axis=1))[0]
                assert bad.size == 0, ("nodes", n_batch, with_root, i, bad[:8])
            if with_root:
                assert (root[:G] == S).all() and (root[-G:] == S).all()
                for i in range(members):
                    assert np.array_equal(root[G + i * dw:G + (i + 1) * dw], tree_ref(digest, np2, i)[-1]), ("root_out", n_batch, i)


def test_tree_harness_refuses_bad_shapes():
    dw = 8
    hashes = np.full(3 * (7 * dw + 8), S, np.uint32)
    for kw in (dict(np2=3), dict(np2=1), dict(np2=8), dict(np2=4, n_batch=3, hashes_stride=7 * dw - 4), dict(np2=4, n_batch=3, hashes_stride=7 * dw + 2),
               dict(np2=4, hashes_off=2), dict(np2=4, n_batch=4, hashes_stride=7 * dw + 8), dict(np2=4, root=np.zeros(7, np.uint32))):
        a = dict(np2=4, hashes_off=0, root=None, root_off=0, n_batch=0, hashes_stride=0)
        a.update(kw)
        with pytest.raises(H.BadArgs):
            H.merkle_tree("sha256", a["np2"], hashes[:7 * dw] if a["np2"] == 8 else hashes, a["hashes_off"], a["root"], a["root_off"], n_batch=a["n_batch"],
                          hashes_stride=a["hashes_stride"])
    assert (hashes == S).all()

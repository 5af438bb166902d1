"""LcCommit<Blake2b, E> on the MI355X: an encoder built with LCPC_HASH_BLAKE2B (digest="blake2b", 64-byte digests) against the
hashlib reference of tests/blake2b_ref.py, and against a BLAKE3 encoder of the same shape for everything the digest must not
change (comm, the transcript, the opened columns)."""
import io
import threading

import numpy as np
import pytest

import blake2b_ref as B
import oracle_lib as O
import pyref as P
from common import mk_transcript
from lcpc_amd import (ERR_ARG, ERR_COMMIT, VERR_COLUMN_PATH, VERR_MALFORMED, LcCommit, LcEvalProof, LcpcError, LigeroEncoding,
                      SdigEncoding, Transcript, _lib, root_bincode)

pytestmark = pytest.mark.gpu

LIMBS = {0: 1, 1: 2, 2: 3, 3: 4}


def make_enc(kind, fid, n, digest, rho=(1, 2)):
    if kind == "ligero":
        return LigeroEncoding.new(fid, n, rho=rho, digest=digest)
    return SdigEncoding.new(fid, n, 5, digest=digest)


def edge_elems(fid, n, seed):
    """n random elements with p - 1, p - 2, 2^(bits - 1) and (Ft255) elements of [2^254, p) spread through them"""
    F = P.FIELDS[fid]
    x = O.random_elems(fid, n, seed)
    top = 1 << (F.num_bits - 1)
    edges = [F.p - 1, F.p - 2, top, top + 1, F.p - 1 - (seed % 97)]
    if fid == 3:
        edges += [(1 << 254) + k for k in range(3)] + [F.p - 1 - (1 << 200)]
    em = O.to_mont(fid, edges)
    for i in range(0, n, max(1, n // 64)):
        x[i] = em[i % len(em)]
    return x


def check_hashes(fid, cm):
    assert cm.enc.digest_len == 64
    comm = cm.comm()
    want = B.tree(B.leaves(O, fid, comm, cm.n_rows, cm.n_cols))
    got = cm.hashes()
    assert got.shape == (len(want), 64)
    bad = [i for i in range(len(want)) if got[i].tobytes() != want[i]]
    assert not bad, "hash slots differ from hashlib: %s" % bad[:8]
    F = P.FIELDS[fid]
    col0 = [F.from_mont(v) for v in O.limbs_to_ints(comm.reshape(cm.n_rows, cm.n_cols, -1)[:, 0])]
    assert B.leaf_from_ints(F, col0) == want[0]
    return want


def commit_both(kind, fid, n, n_coeffs=None, rho=(1, 2), seed=1):
    n_coeffs = n if n_coeffs is None else n_coeffs
    coeffs = edge_elems(fid, n_coeffs, seed)
    eb, e2 = make_enc(kind, fid, n, "blake3", rho), make_enc(kind, fid, n, "blake2b", rho)
    cb, c2 = LcCommit.commit(coeffs, eb), LcCommit.commit(coeffs, e2)
    assert np.array_equal(cb.comm(), c2.comm())
    assert cb.n_rows == c2.n_rows and cb.n_cols == c2.n_cols
    return coeffs, eb, e2, cb, c2


# ---- construction --------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("fid", [0, 1, 2, 3])
@pytest.mark.parametrize("kind,rho", [("ligero", (1, 2)), ("ligero", (1, 4)), ("sdig", None)])
def test_ctx_create_blake2b(fid, kind, rho):
    enc = make_enc(kind, fid, 1 << 12, "blake2b", rho or (1, 2))
    assert enc.digest == "blake2b" and enc.digest_len == 64
    eb = make_enc(kind, fid, 1 << 12, "blake3", rho or (1, 2))
    assert eb.digest == "blake3" and eb.digest_len == 32


def test_sharding_refused():
    with pytest.raises(LcpcError) as e:
        LigeroEncoding.new(3, 1 << 12, shard=(0, 2), digest="blake2b")
    assert e.value.code == ERR_ARG
    with pytest.raises(LcpcError) as e:
        SdigEncoding(1, 1 << 12, 5, shard=(1, 2), digest="blake2b")
    assert e.value.code == ERR_ARG


def test_sharded_entry_points_refuse_blake2b():
    import torch
    enc = LigeroEncoding.new(3, 1 << 12, digest="blake2b")
    cm = LcCommit(enc)
    coeffs = torch.zeros((1 << 12, 4), dtype=torch.int64, device="cuda")
    scratch = torch.zeros(1 << 20, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    L = _lib.lib()
    n_rows = 1
    assert L.lcpc_commit_shard_device(cm._h, coeffs.data_ptr(), n_rows, None, 0, scratch.data_ptr()) == ERR_ARG
    assert L.lcpc_commit_finish_device(cm._h, scratch.data_ptr(), n_rows, 1, None, None) == ERR_ARG
    assert L.lcpc_commit_sharded_device(cm._h, coeffs.data_ptr(), n_rows, None, 0, None) == ERR_ARG


# ---- the whole hashes array ----------------------------------------------------------------------------------------------

SHAPES = [
    # Brakedown, n_cols = 37 (< 64, not a power of two: leaf slots 37..63 are 64 zero bytes), 1 and 5 rows (ragged)
    ("sdig", 0, 24, 24), ("sdig", 3, 24, 5 * 24 - 7), ("sdig", 2, 24, 3 * 24 - 1),
    # Brakedown at and above 24 rows: the position-major commitment (col_stride = n_rows)
    ("sdig", 0, 1 << 12, 24 * 3001), ("sdig", 3, 1 << 12, 40 * 4096 - 3), ("sdig", 1, 1 << 12, 30 * 3675 - 11),
    ("sdig", 2, 1 << 10, 23 * 1024),
    # Ligero, ragged and tiny
    ("ligero", 0, 1 << 12, None), ("ligero", 3, 1 << 10, None), ("ligero", 1, 1 << 12, (1 << 12) - 5),
    ("ligero", 3, 1, None), ("ligero", 2, 16, 13),
]


@pytest.mark.parametrize("kind,fid,n,n_coeffs", SHAPES)
def test_hashes_shapes(kind, fid, n, n_coeffs):
    _, _, _, cb, c2 = commit_both(kind, fid, n, n_coeffs)
    want = check_hashes(fid, c2)
    assert c2.get_root() == want[-1]
    assert cb.get_root() != want[-1][:32]


# n_rows with an exact last block (L R = 8 mod 16) and partial ones next to it, per field
BLOCK_ROWS = {0: [8, 24, 23, 25], 1: [4, 12, 13, 11], 2: [8, 24, 25, 22], 3: [2, 6, 7, 5, 3]}


@pytest.mark.parametrize("fid", [0, 1, 2, 3])
def test_hashes_last_block_exact_and_partial(fid):
    L = LIMBS[fid]
    n_per_row, n_cols = 256, 512
    eb = LigeroEncoding.new_from_dims(fid, n_per_row, n_cols, digest="blake3")
    e2 = LigeroEncoding.new_from_dims(fid, n_per_row, n_cols, digest="blake2b")
    seen = set()
    for n_rows in BLOCK_ROWS[fid]:
        for ragged in (0, 37):
            n_coeffs = n_rows * n_per_row - ragged
            coeffs = edge_elems(fid, n_coeffs, 100 + n_rows)
            c2 = LcCommit.commit(coeffs, e2)
            assert c2.n_rows == n_rows
            seen.add(B.exact_last_block(L, n_rows))
            check_hashes(fid, c2)
            assert np.array_equal(LcCommit.commit(coeffs, eb).comm(), c2.comm())
    assert seen == {True, False}


@pytest.mark.parametrize("fid", [0, 1, 2, 3])
@pytest.mark.parametrize("log_n", [10, 12, 14, 16, 18, 20])
def test_hashes_ligero_sizes(fid, log_n):
    _, _, _, _, c2 = commit_both("ligero", fid, 1 << log_n, seed=log_n)
    check_hashes(fid, c2)


@pytest.mark.parametrize("fid,log_n", [(1, 20), (3, 18)])
def test_hashes_ligero_rate_quarter(fid, log_n):
    _, _, _, _, c2 = commit_both("ligero", fid, 1 << log_n, rho=(1, 4), seed=3)
    check_hashes(fid, c2)


@pytest.mark.parametrize("fid,log_n", [(0, 20), (3, 20), (2, 16)])
def test_hashes_brakedown_sizes(fid, log_n):
    _, _, _, _, c2 = commit_both("sdig", fid, 1 << log_n, seed=4)
    check_hashes(fid, c2)


@pytest.mark.parametrize("fid", [0, 3])
def test_hashes_2_24(fid):
    _, _, _, _, c2 = commit_both("ligero", fid, 1 << 24, seed=24)
    check_hashes(fid, c2)


def test_canonical_edges_from_parts():
    """comm elements p - 1 and in [2^254, p) straight into the column hash (lcpc_commit_from_parts)"""
    for kind, fid, n in (("ligero", 3, 1 << 12), ("ligero", 0, 1 << 12), ("sdig", 3, 1 << 12), ("ligero", 2, 1 << 10), ("ligero", 1, 1 << 10)):
        e2 = make_enc(kind, fid, n, "blake2b")
        n_rows = 30
        comm = edge_elems(fid, n_rows * e2.n_cols, 9)
        F = P.FIELDS[fid]
        comm[:e2.n_cols] = O.to_mont(fid, [F.p - 1] * e2.n_cols)       # a whole row of p - 1
        c2 = LcCommit.from_parts(e2, comm, None, n_rows)
        assert np.array_equal(c2.comm(), comm)
        check_hashes(fid, c2)


# ---- every commit entry point gives the same digests ------------------------------------------------------------------------

@pytest.mark.parametrize("kind,fid,log_n", [("ligero", 3, 21), ("ligero", 1, 16), ("sdig", 3, 14)])
def test_entry_points_same_hashes(kind, fid, log_n):
    import torch
    n = 1 << log_n
    coeffs = edge_elems(fid, n, 11)
    e2 = make_enc(kind, fid, n, "blake2b")
    pageable = LcCommit.commit(coeffs, e2)              # Ft255 2^21 = 64 MiB: the row-batch host path
    want = check_hashes(fid, pageable)
    wh = pageable.hashes()
    pinned = torch.from_numpy(coeffs.view(np.int64)).pin_memory()
    assert np.array_equal(LcCommit.commit(pinned.numpy().view(np.uint64), e2).hashes(), wh)
    fresh = np.array(coeffs, copy=True)
    refill = LcCommit.commit(fresh, e2, into=pageable)
    assert refill is pageable and refill.get_root() == want[-1]
    assert np.array_equal(refill.hashes(), wh)
    dev = torch.from_numpy(coeffs.view(np.int64)).cuda()
    torch.cuda.synchronize()
    cd = LcCommit.commit_device(dev.data_ptr(), n, e2)
    assert cd.get_root() == want[-1] and np.array_equal(cd.hashes(), wh)
    if n % e2.n_per_row == 0:
        cbor = LcCommit.commit_device(dev.data_ptr(), n, e2, borrow=True)
        assert cbor.get_root() == want[-1] and np.array_equal(cbor.hashes(), wh)
    fp = LcCommit.from_parts(e2, pageable.comm(), pageable.coeffs(), pageable.n_rows)
    assert np.array_equal(fp.hashes(), wh)
    # a refill of one object from another entry point, and back
    LcCommit.commit_device(dev.data_ptr(), n, e2, into=fp)
    assert np.array_equal(fp.hashes(), wh)


# ---- root and bincode -----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("kind,fid", [("ligero", 3), ("sdig", 1), ("ligero", 2)])
def test_root_and_bincode(kind, fid):
    n = 1 << 12
    coeffs, eb, e2, cb, c2 = commit_both(kind, fid, n, seed=12)
    root = c2.get_root()
    assert len(root) == 64 and root == c2.hashes()[-1].tobytes()
    assert root_bincode(root) == (64).to_bytes(8, "little") + root and len(root_bincode(root)) == 72
    assert len(root_bincode(cb.get_root())) == 40
    b2s, b3s = io.BytesIO(), io.BytesIO()
    c2.to_bincode(b2s)
    cb.to_bincode(b3s)
    blob = b2s.getvalue()
    assert len(blob) == c2.bincode_size() == len(b3s.getvalue()) + 32 * c2.n_hashes
    # the hashes tail: u64 len | len x (u64 64 | 64 bytes)
    tail = blob[len(blob) - 8 - 72 * c2.n_hashes:]
    assert int.from_bytes(tail[:8], "little") == c2.n_hashes
    hs = c2.hashes()
    for i in (0, c2.n_hashes // 2, c2.n_hashes - 1):
        e = tail[8 + 72 * i:8 + 72 * (i + 1)]
        assert int.from_bytes(e[:8], "little") == 64 and e[8:] == hs[i].tobytes()
    back = LcCommit.from_bincode(e2, io.BytesIO(blob))
    assert back.get_root() == root and np.array_equal(back.hashes(), hs)
    assert np.array_equal(back.comm(), c2.comm())
    # a stream of another digest into a BLAKE2b commitment, and the reverse
    es = make_enc(kind, fid, n, "sha3_256")
    bss = io.BytesIO()
    LcCommit.commit(coeffs, es).to_bincode(bss)
    for enc, other in ((e2, b3s.getvalue()), (e2, bss.getvalue()), (eb, blob), (es, blob)):
        with pytest.raises(LcpcError) as e:
            LcCommit.from_bincode(enc, io.BytesIO(other))
        assert e.value.code == ERR_COMMIT
    # one tampered digest (a leaf and the root)
    for i in (0, c2.n_hashes - 1):
        bad = bytearray(blob)
        bad[len(blob) - 72 * (c2.n_hashes - i) + 8 + 17] ^= 0x01
        with pytest.raises(LcpcError) as e:
            LcCommit.from_bincode(e2, io.BytesIO(bytes(bad)))
        assert e.value.code == ERR_COMMIT


# ---- proofs ---------------------------------------------------------------------------------------------------------------

def split_proof(blob, n_rows, n_cols, L, n_open, dl):
    """header bytes and per column (values bytes, [path digests]) of a bincode proof with dl-byte digests (lib.rs:550-609)"""
    path_len = max(0, (n_cols - 1).bit_length())
    we = 8 + dl
    col_bytes = 8 + n_rows * L * 8 + 8 + path_len * we
    head = len(blob) - n_open * col_bytes
    cols = []
    for k in range(n_open):
        q = head + k * col_bytes
        vals = blob[q:q + 8 + n_rows * L * 8 + 8]
        q += 8 + n_rows * L * 8 + 8
        ents = [blob[q + we * i:q + we * (i + 1)] for i in range(path_len)]
        assert all(int.from_bytes(e[:8], "little") == dl for e in ents)
        cols.append((vals, [e[8:] for e in ents]))
    return blob[:head], cols


def same_tr(nco):
    """the same transcript inputs under both digests (the roots differ): the test transcript with a fixed label"""
    return mk_transcript(Transcript, b"\x5a" * 32, nco)


@pytest.mark.parametrize("kind,fid,log_n", [("ligero", 3, 16), ("ligero", 0, 14), ("ligero", 2, 12), ("sdig", 1, 14), ("sdig", 2, 12)])
def test_prove_verify(kind, fid, log_n):
    n = 1 << log_n
    _, eb, e2, cb, c2 = commit_both(kind, fid, n, seed=21)
    L, nco = e2.L, e2.get_n_col_opens()
    outer = O.random_elems(fid, c2.n_rows, 22)
    pb = cb.prove(outer, eb, same_tr(nco))
    p2 = c2.prove(outer, e2, same_tr(nco))
    assert np.array_equal(pb.cols_opened, p2.cols_opened)
    want = B.tree(B.leaves(O, fid, c2.comm(), c2.n_rows, c2.n_cols))
    np2 = (len(want) + 1) // 2
    root = c2.get_root()
    assert root == want[-1]
    # the expected BLAKE2b proof: the BLAKE3 proof with every path entry replaced by u64 64 | the hashlib sibling
    hb, colb = split_proof(pb.to_bytes(), cb.n_rows, cb.n_cols, L, nco, 32)
    exp = bytearray(hb)
    for k, c in enumerate(pb.cols_opened):
        exp += colb[k][0]
        for s in B.path(want, np2, int(c)):
            exp += (64).to_bytes(8, "little") + s
    assert p2.to_bytes() == bytes(exp)
    # open_columns: the same siblings, folding to the root from the hashlib leaf
    vals, paths = c2.open_columns(p2.cols_opened[:8])
    assert paths.shape[2] == 64
    for k, c in enumerate(p2.cols_opened[:8]):
        sibs = [paths[k, i].tobytes() for i in range(paths.shape[1])]
        assert sibs == B.path(want, np2, int(c))
        assert B.fold(want[int(c)], int(c), sibs) == root
    # verify: the same evaluation as the BLAKE3 verify
    inner = O.random_elems(fid, c2.n_per_row, 23)
    ev2 = LcEvalProof.from_bytes(p2.to_bytes(), L).verify(root, outer, inner, e2, same_tr(nco))
    evb = LcEvalProof.from_bytes(pb.to_bytes(), L).verify(cb.get_root(), outer, inner, eb, same_tr(nco))
    assert np.array_equal(ev2, evb)
    # one flipped path byte (first column, first sibling, byte 40: past the first 32 bytes of a 64-byte digest)
    blob = bytearray(p2.to_bytes())
    blob[len(hb) + 8 + c2.n_rows * L * 8 + 8 + 8 + 40] ^= 0x40
    with pytest.raises(LcpcError) as e:
        LcEvalProof.from_bytes(bytes(blob), L).verify(root, outer, inner, e2, same_tr(nco))
    assert e.value.code == VERR_COLUMN_PATH
    # a wrong root: the last byte of the 64
    with pytest.raises(LcpcError) as e:
        LcEvalProof.from_bytes(p2.to_bytes(), L).verify(root[:63] + bytes([root[63] ^ 1]), outer, inner, e2, same_tr(nco))
    assert e.value.code == VERR_COLUMN_PATH
    # a BLAKE3 proof into a BLAKE2b verifier, and the reverse: path entries of the wrong length
    with pytest.raises(LcpcError) as e:
        LcEvalProof.from_bytes(pb.to_bytes(), L).verify(root, outer, inner, e2, same_tr(nco))
    assert e.value.code == VERR_MALFORMED
    with pytest.raises(LcpcError) as e:
        LcEvalProof.from_bytes(p2.to_bytes(), L).verify(cb.get_root(), outer, inner, eb, same_tr(nco))
    assert e.value.code == VERR_MALFORMED


def test_two_threads_prove_one_commitment():
    fid, n = 3, 1 << 16
    e2 = LigeroEncoding.new(fid, n, digest="blake2b")
    c2 = LcCommit.commit(edge_elems(fid, n, 31), e2)
    outer = O.random_elems(fid, c2.n_rows, 32)
    root, nco = c2.get_root(), e2.get_n_col_opens()
    want = c2.prove(outer, e2, mk_transcript(Transcript, root, nco)).to_bytes()
    got, errs = [None] * 2, []

    def run(i):
        try:
            for _ in range(3):
                b = c2.prove(outer, e2, mk_transcript(Transcript, root, nco)).to_bytes()
                if b != want:
                    got[i] = b
                    return
            got[i] = want
        except Exception as ex:       # surfaced below
            errs.append(ex)

    th = [threading.Thread(target=run, args=(i,)) for i in range(2)]
    for t in th:
        t.start()
    for t in th:
        t.join()
    assert not errs, errs
    assert got == [want, want]
    inner = O.random_elems(fid, c2.n_per_row, 33)
    LcEvalProof.from_bytes(want, e2.L).verify(root, outer, inner, e2, mk_transcript(Transcript, root, nco))


# ---- full size ------------------------------------------------------------------------------------------------------------

def test_fullsize_ft255_2_26():
    """2^26 Ft255 (512 x 262144 after encoding): 1024 sampled leaves against hashlib from the opened columns, and every tree
    level above the GPU's leaves against hashlib"""
    fid, n = 3, 1 << 26
    e2 = LigeroEncoding.new(fid, n, digest="blake2b")
    coeffs = e2.random_coeffs_device(n, 26)
    import torch
    torch.cuda.synchronize()
    c2 = LcCommit.commit_device(coeffs.data_ptr(), n, e2)
    assert (c2.n_rows, c2.n_cols) == (512, 1 << 18)
    hs = c2.hashes()
    np2 = 1 << 18
    leaves = [hs[i].tobytes() for i in range(np2)]
    tree = B.tree(leaves)
    bad = [i for i in range(np2, len(tree)) if hs[i].tobytes() != tree[i]]
    assert not bad, bad[:8]
    rng = np.random.default_rng(26)
    cols = np.unique(rng.integers(0, c2.n_cols, 1100).astype(np.uint64))[:1024]
    cols[0], cols[-1] = 0, c2.n_cols - 1
    assert len(cols) >= 1000
    vals, paths = c2.open_columns(cols)
    rep = B.repr_bytes(O, fid, vals.reshape(-1, 4)).reshape(len(cols), -1)
    for k, c in enumerate(cols):
        lf = B.b2(B.ZERO + rep[k].tobytes())
        assert lf == leaves[int(c)], int(c)
        assert B.fold(lf, int(c), [paths[k, i].tobytes() for i in range(paths.shape[1])]) == c2.get_root()

"""LcCommit<Sha3_256, E> on the MI355X: an encoder built with LCPC_HASH_SHA3_256 (digest="sha3_256") against the hashlib
reference of tests/sha3_ref.py, and against a BLAKE3 encoder of the same shape for everything the digest must not change."""
import io
import os
import subprocess
import sys

import numpy as np
import pytest

import oracle_lib as O
import pyref as P
import sha3_ref as S
from common import mk_transcript
from lcpc_amd import (ERR_ARG, ERR_COMMIT, VERR_COLUMN_PATH, LcCommit, LcEvalProof, LcpcError, LigeroEncoding, SdigEncoding,
                      Transcript)

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


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
    comm = cm.comm()
    want = S.tree(S.leaves(O, fid, comm, cm.n_rows, cm.n_cols))
    got = cm.hashes()
    assert got.shape[0] == len(want)
    bad = [i for i in range(len(want)) if got[i].tobytes() != want[i]]
    assert not bad, "hash slots differ from hashlib: %s" % bad[:8]
    # the bulk to_repr of the reference is pyref's Field.to_repr
    F = P.FIELDS[fid]
    col0 = [F.from_mont(v) for v in O.limbs_to_ints(comm.reshape(cm.n_rows, cm.n_cols, -1)[:, 0])]
    assert S.leaf_from_ints(F, col0) == want[0]
    return want


def commit_both(kind, fid, n, n_coeffs=None, rho=(1, 2), seed=1):
    n_coeffs = n if n_coeffs is None else n_coeffs
    coeffs = edge_elems(fid, n_coeffs, seed)
    eb, es = make_enc(kind, fid, n, "blake3", rho), make_enc(kind, fid, n, "sha3_256", rho)
    cb, cs = LcCommit.commit(coeffs, eb), LcCommit.commit(coeffs, es)
    assert np.array_equal(cb.comm(), cs.comm())
    assert cb.n_rows == cs.n_rows and cb.n_cols == cs.n_cols
    return coeffs, eb, es, cb, cs


# ---- construction --------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("fid", [0, 1, 2, 3])
@pytest.mark.parametrize("kind,rho", [("ligero", (1, 2)), ("ligero", (1, 4)), ("sdig", None)])
def test_ctx_create_sha3(fid, kind, rho):
    enc = make_enc(kind, fid, 1 << 12, "sha3_256", rho or (1, 2))
    assert enc.digest == "sha3_256"
    assert make_enc(kind, fid, 1 << 12, "blake3", rho or (1, 2)).digest == "blake3"


def test_sharding_refused():
    with pytest.raises(LcpcError) as e:
        LigeroEncoding.new(3, 1 << 12, shard=(0, 2), digest="sha3_256")
    assert e.value.code == ERR_ARG
    with pytest.raises(LcpcError) as e:
        SdigEncoding(1, 1 << 12, 5, shard=(1, 2), digest="sha3_256")
    assert e.value.code == ERR_ARG


# ---- the whole hashes array ----------------------------------------------------------------------------------------------

SHAPES = [
    # Brakedown, n_cols = 37 (< 64, not a power of two: leaf slots 37..63 are zero), 1 and 5 rows (ragged)
    ("sdig", 0, 24, 24), ("sdig", 3, 24, 5 * 24 - 7), ("sdig", 2, 24, 3 * 24 - 1),
    # Brakedown at and above SDIG_T_MIN_ROWS = 24 rows: the position-major commitment (col_stride = n_rows)
    ("sdig", 0, 1 << 12, 24 * 3001), ("sdig", 3, 1 << 12, 40 * 4096 - 3), ("sdig", 1, 1 << 12, 30 * 3675 - 11),
    ("sdig", 2, 1 << 10, 23 * 1024),
    # Ligero shapes where BLAKE3 takes its one-launch leaf_tree path (n_cols % 64 == 0, 128 <= n_cols, <= 2 chunks)
    ("ligero", 0, 1 << 12, None), ("ligero", 3, 1 << 10, None), ("ligero", 1, 1 << 12, (1 << 12) - 5),
    # tiny Ligero: one column pair
    ("ligero", 3, 1, None), ("ligero", 2, 16, 13),
]


@pytest.mark.parametrize("kind,fid,n,n_coeffs", SHAPES)
def test_hashes_shapes(kind, fid, n, n_coeffs):
    _, _, _, cb, cs = commit_both(kind, fid, n, n_coeffs)
    want = check_hashes(fid, cs)
    assert cs.get_root() == want[-1] != cb.get_root()


@pytest.mark.parametrize("fid", [0, 1, 2, 3])
@pytest.mark.parametrize("log_n", [10, 12, 14, 16, 18, 20])
def test_hashes_ligero_sizes(fid, log_n):
    _, _, _, _, cs = commit_both("ligero", fid, 1 << log_n, seed=log_n)
    check_hashes(fid, cs)


@pytest.mark.parametrize("fid,log_n", [(1, 20), (3, 18)])
def test_hashes_ligero_rate_quarter(fid, log_n):
    _, _, _, _, cs = commit_both("ligero", fid, 1 << log_n, rho=(1, 4), seed=3)
    check_hashes(fid, cs)


@pytest.mark.parametrize("fid,log_n", [(0, 20), (3, 20)])
def test_hashes_brakedown_sizes(fid, log_n):
    _, _, _, _, cs = commit_both("sdig", fid, 1 << log_n, seed=4)
    check_hashes(fid, cs)


def test_hashes_ft255_2_24():
    _, _, _, _, cs = commit_both("ligero", 3, 1 << 24, seed=24)
    check_hashes(3, cs)


def test_canonical_edges_from_parts():
    """comm elements p - 1 and in [2^254, p) straight into the column hash (lcpc_commit_from_parts)"""
    for kind, fid, n in (("ligero", 3, 1 << 12), ("ligero", 0, 1 << 12), ("sdig", 3, 1 << 12), ("ligero", 2, 1 << 10)):
        es = make_enc(kind, fid, n, "sha3_256")
        n_rows = 30
        comm = edge_elems(fid, n_rows * es.n_cols, 9)
        F = P.FIELDS[fid]
        hi = O.to_mont(fid, [F.p - 1] * es.n_cols)
        comm[:es.n_cols] = hi                           # a whole row of p - 1
        cs = LcCommit.from_parts(es, comm, None, n_rows)
        assert np.array_equal(cs.comm(), comm)
        check_hashes(fid, cs)


# ---- every commit entry point gives the same root --------------------------------------------------------------------------

@pytest.mark.parametrize("kind,fid,log_n", [("ligero", 3, 21), ("ligero", 1, 16), ("sdig", 3, 14)])
def test_entry_points_same_root(kind, fid, log_n):
    import torch
    n = 1 << log_n
    coeffs = edge_elems(fid, n, 11)
    es = make_enc(kind, fid, n, "sha3_256")
    pageable = LcCommit.commit(coeffs, es)              # Ft255 2^21 = 64 MiB: the batched host path, staged through the ring
    want = check_hashes(fid, pageable)[-1]
    pinned = torch.from_numpy(coeffs.view(np.int64)).pin_memory()
    assert LcCommit.commit(pinned.numpy().view(np.uint64), es).get_root() == want
    fresh = np.array(coeffs, copy=True)
    assert LcCommit.commit(fresh, es, into=pageable).get_root() == want
    dev = torch.from_numpy(coeffs.view(np.int64)).cuda()
    torch.cuda.synchronize()
    cd = LcCommit.commit_device(dev.data_ptr(), n, es)
    assert cd.get_root() == want
    fp = LcCommit.from_parts(es, pageable.comm(), pageable.coeffs(), pageable.n_rows)
    assert fp.get_root() == want


# ---- bincode ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("kind,fid", [("ligero", 3), ("sdig", 1)])
def test_bincode_round_trip_and_digest_mismatch(kind, fid):
    n = 1 << 12
    _, eb, es, cb, cs = commit_both(kind, fid, n, seed=12)
    bs, bb = io.BytesIO(), io.BytesIO()
    cs.to_bincode(bs)
    cb.to_bincode(bb)
    back = LcCommit.from_bincode(es, io.BytesIO(bs.getvalue()))
    assert back.get_root() == cs.get_root()
    assert np.array_equal(back.hashes(), cs.hashes())
    for enc, blob in ((es, bb.getvalue()), (eb, bs.getvalue())):
        with pytest.raises(LcpcError) as e:
            LcCommit.from_bincode(enc, io.BytesIO(blob))
        assert e.value.code == ERR_COMMIT


# ---- prove / verify --------------------------------------------------------------------------------------------------------

def split_proof(blob, cm, L, n_open):
    """header bytes and per column (values bytes, [path digests]) of a bincode proof (prove.cpp layout, lib.rs:550-609)"""
    path_len = max(0, (cm.n_cols - 1).bit_length())
    col_bytes = 8 + cm.n_rows * L * 8 + 8 + path_len * 40
    head = len(blob) - n_open * col_bytes
    cols = []
    for k in range(n_open):
        q = head + k * col_bytes
        vals = blob[q:q + 8 + cm.n_rows * L * 8]
        q += 8 + cm.n_rows * L * 8 + 8
        cols.append((vals, [blob[q + 40 * i + 8:q + 40 * i + 40] for i in range(path_len)]))
    return blob[:head], cols


def same_tr(nco):
    """the same transcript inputs under both digests (a root would differ): the test transcript with a fixed 32-byte label"""
    return mk_transcript(Transcript, b"\x5a" * 32, nco)


def prove_both(kind, fid, n):
    coeffs, eb, es, cb, cs = commit_both(kind, fid, n, seed=21)
    outer = O.random_elems(fid, cs.n_rows, 22)
    pb = cb.prove(outer, eb, same_tr(eb.get_n_col_opens()))
    ps = cs.prove(outer, es, same_tr(es.get_n_col_opens()))
    return coeffs, eb, es, cb, cs, outer, pb, ps


@pytest.mark.parametrize("kind,fid,log_n", [("ligero", 3, 16), ("ligero", 0, 14), ("sdig", 1, 14), ("sdig", 2, 12)])
def test_prove_verify(kind, fid, log_n):
    n = 1 << log_n
    _, eb, es, cb, cs, outer, pb, ps = prove_both(kind, fid, n)
    L = es.L
    nco = es.get_n_col_opens()
    assert np.array_equal(pb.cols_opened, ps.cols_opened)
    hb, colb = split_proof(pb.to_bytes(), cb, L, nco)
    hs, cols = split_proof(ps.to_bytes(), cs, L, nco)
    assert hb == hs                                       # n_cols, p_eval, p_random: the transcript never sees D
    want = [bytes(h) for h in cs.hashes()]
    np2 = (len(want) + 1) // 2
    for k, c in enumerate(ps.cols_opened):
        assert colb[k][0] == cols[k][0]                   # column values
        assert cols[k][1] == S.path(want, np2, int(c))    # the hashlib tree's siblings
    root = cs.get_root()
    # any inner tensor: the evaluation is <p_eval, inner>, the same under both digests
    inner = O.random_elems(fid, cs.n_per_row, 23)
    ev_s = LcEvalProof.from_bytes(ps.to_bytes(), L).verify(root, outer, inner, es, same_tr(nco))
    rb = cb.get_root()
    ev_b = LcEvalProof.from_bytes(pb.to_bytes(), L).verify(rb, outer, inner, eb, same_tr(nco))
    assert np.array_equal(ev_s, ev_b)
    # one flipped path byte
    blob = bytearray(ps.to_bytes())
    head = len(hs)
    q = head + 8 + cs.n_rows * L * 8 + 8 + 8 + 5          # first column, first sibling, byte 5
    blob[q] ^= 0x40
    with pytest.raises(LcpcError) as e:
        LcEvalProof.from_bytes(bytes(blob), L).verify(root, outer, inner, es, same_tr(nco))
    assert e.value.code == VERR_COLUMN_PATH
    # a SHA3 proof checked by a BLAKE3 encoder (same root bytes, same transcript)
    with pytest.raises(LcpcError) as e:
        LcEvalProof.from_bytes(ps.to_bytes(), L).verify(root, outer, inner, eb, same_tr(nco))
    assert e.value.code == VERR_COLUMN_PATH


CHILD = r"""
import sys
sys.path[:0] = [%r, %r, %r]
import numpy as np
import oracle_lib as O
from common import mk_transcript
from lcpc_amd import LcCommit, LcEvalProof, LigeroEncoding, Transcript
enc = LigeroEncoding.new(1, 1 << 14, digest="sha3_256")
c = LcCommit.commit(O.random_elems(1, 1 << 14, 5), enc)
outer, inner = O.random_elems(1, c.n_rows, 6), O.random_elems(1, c.n_per_row, 7)
root, nco = c.get_root(), enc.get_n_col_opens()
pf = c.prove(outer, enc, mk_transcript(Transcript, root, nco))
LcEvalProof.from_bytes(pf.to_bytes(), enc.L).verify(root, outer, inner, enc, mk_transcript(Transcript, root, nco))
print("verify ok")
"""


def test_verify_portable_keccak():
    env = dict(os.environ, LCPC_KECCAK="portable")
    code = CHILD % (ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "oracle"))
    r = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "verify ok" in r.stdout, r.stdout + r.stderr

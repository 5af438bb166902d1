"""LcCommit<Keccak256, E> and LcCommit<Sha256, E> on the MI355X: encoders built with digest="keccak256" / "sha256"
(LCPC_HASH_KECCAK256 / LCPC_HASH_SHA256) against the references of tests/digest_more.py -- hashlib.sha256, and the Keccak-256
sponge on pyref's Keccak-f -- held to what BLAKE2b is held to in test_gpu_blake2b.py and test_gpu_digests_{edges,verify}.py: the
whole `hashes` array for both encodings, all four fields and both leaf-kernel instantiations <NL, CANON>; every last-block
residue a field can reach; every commit entry point; bincode; proof bytes, verify and the mutation sweep against the
digest-generic reference; paths; threads; and the 2^26 headline shape.

SHA-256 last-block residues (4 + L n_rows) mod 8 the edge test reaches, derived by digest_more.edge_rows and asserted:

    field  L   residue 0 / 1 / 6 / 7 -> n_rows
    Ft63   1   4 / 5 / 2 / 3
    Ft127  2   2 / - / 1 / -        (4 + 2 n_rows is even)
    Ft191  3   4 / 7 / 6 / 1
    Ft255  4   1 / - / - / -        (4 + 4 n_rows is 0 or 4 mod 8)

Keccak-256 has SHA3-256's message and rate: the residues of digest_ref.SHA3_RESIDUES, at the n_rows of test_gpu_digests_edges.py."""
import io
import threading

import numpy as np
import pytest

import digest_more as DM
import digest_ref as DR
import lcpc_amd
from lcpc_amd import (ERR_ARG, ERR_COMMIT, VERR_COLUMN_PATH, VERR_MALFORMED, LcCommit, LcEvalProof, LcpcError, LigeroEncoding,
                      SdigEncoding, Transcript, _lib)

pytestmark = pytest.mark.gpu

NEW = DM.NEW_DIGESTS
ALL_FIVE = DR.DIGEST_NAMES + NEW
SHA256_EDGE_TABLE = {
    0: {("sha256", 0): 4, ("sha256", 1): 5, ("sha256", 6): 2, ("sha256", 7): 3},
    1: {("sha256", 0): 2, ("sha256", 1): None, ("sha256", 6): 1, ("sha256", 7): None},
    2: {("sha256", 0): 4, ("sha256", 1): 7, ("sha256", 6): 6, ("sha256", 7): 1},
    3: {("sha256", 0): 1, ("sha256", 1): None, ("sha256", 6): None, ("sha256", 7): None},
}
KECCAK_EDGE_TABLE = {
    0: {0: 13, 1: 14, 8: 4, 15: 11, 16: 12}, 1: {0: 15, 1: 7, 8: 2, 15: 14, 16: 6},
    2: {0: 10, 1: 16, 8: 7, 15: 15, 16: 4}, 3: {0: 16, 1: 12, 8: 1, 15: 7, 16: 3},
}


def make_enc(kind, fid, n, digest, rho=(1, 2)):
    if kind == "ligero":
        return LigeroEncoding.new(fid, n, rho=rho, digest=digest)
    return SdigEncoding.new(fid, n, 5, digest=digest)


def check_hashes(O, digest, fid, cm):
    assert cm.enc.digest == digest and cm.enc.digest_len == 32
    want = DM.hashes_ref(digest, O, fid, cm.comm(), cm.n_rows, cm.n_cols)
    got = cm.hashes()
    assert got.shape == want.shape
    bad = np.nonzero((got != want).any(axis=1))[0]
    assert bad.size == 0, "%s: hash slots differ from the reference: %s" % (digest, bad[:8])
    assert cm.get_root() == want[-1].tobytes()
    return want


# ---- construction ----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("digest", NEW)
def test_ctx_create_and_sharding_refused(digest):
    import torch
    for fid in range(4):
        for kind in ("ligero", "sdig"):
            enc = make_enc(kind, fid, 1 << 12, digest)
            assert enc.digest == digest and enc.digest_len == 32 and enc.params.hash == lcpc_amd.DIGEST_TABLE[digest][0]
    with pytest.raises(LcpcError) as e:
        LigeroEncoding.new(3, 1 << 12, shard=(0, 2), digest=digest)
    assert e.value.code == ERR_ARG
    with pytest.raises(LcpcError) as e:
        SdigEncoding(1, 1 << 12, 5, shard=(1, 2), digest=digest)
    assert e.value.code == ERR_ARG
    enc = LigeroEncoding.new(3, 1 << 12, digest=digest)
    cm = LcCommit(enc)
    coeffs = torch.zeros((1 << 12, 4), dtype=torch.int64, device="cuda")
    scratch = torch.zeros(1 << 20, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    L = _lib.lib()
    assert L.lcpc_commit_shard_device(cm._h, coeffs.data_ptr(), 1, None, 0, scratch.data_ptr()) == ERR_ARG
    assert L.lcpc_commit_finish_device(cm._h, scratch.data_ptr(), 1, 1, None, None) == ERR_ARG
    assert L.lcpc_commit_sharded_device(cm._h, coeffs.data_ptr(), 1, None, 0, None) == ERR_ARG


def test_an_unknown_hash_value_is_still_refused():
    p = lcpc_amd._params(3, lcpc_amd.ENC_LIGERO, 0, digest="sha256")
    p.n_coeffs = 1 << 12
    p.hash = 5
    with pytest.raises(LcpcError) as e:
        lcpc_amd._Encoding(p)
    assert e.value.code == ERR_ARG


# ---- the whole hashes array ------------------------------------------------------------------------------------------------------

SHAPES = [
    # Brakedown, n_cols < 64 and not a power of two, 1 and 5 rows (ragged): Montgomery-form comm, <NL, false>
    ("sdig", 0, 24, 24), ("sdig", 3, 24, 5 * 24 - 7), ("sdig", 2, 24, 3 * 24 - 1), ("sdig", 1, 24, 2 * 24 - 1),
    # Brakedown at and above 24 rows: the position-major commitment (col_stride = n_rows), canonical
    ("sdig", 0, 1 << 12, 24 * 3001), ("sdig", 3, 1 << 12, 40 * 4096 - 3), ("sdig", 1, 1 << 12, 30 * 3675 - 11), ("sdig", 2, 1 << 10, 31 * 1024 - 9),
    # Ligero, ragged and tiny; 2 columns
    ("ligero", 0, 1 << 12, None), ("ligero", 3, 1 << 10, None), ("ligero", 1, 1 << 12, (1 << 12) - 5), ("ligero", 3, 1, None),
    ("ligero", 2, 16, 13),
]


@pytest.mark.parametrize("digest", NEW)
def test_hashes_shapes(oracle, digest):
    O = oracle
    reached = set()
    for kind, fid, n, n_coeffs in SHAPES:
        enc = make_enc(kind, fid, n, digest)
        cm = LcCommit.commit(DR.edge_elems(O, fid, n if n_coeffs is None else n_coeffs, 1 + fid), enc)
        check_hashes(O, digest, fid, cm)
        if kind == "sdig":
            assert cm.n_cols & (cm.n_cols - 1)
            reached.add((fid, DR.leaf_canon_in(fid, "sdig", 0, cm.n_rows)))
    assert reached == {(f, c) for f in range(4) for c in (False, True)}      # <NL, CANON> both ways for every field


@pytest.mark.parametrize("digest", NEW)
def test_hashes_two_columns(oracle, digest):
    O = oracle
    for fid in range(4):
        oenc = O.Encoding.ligero_from_dims(fid, 1, 2)
        enc = DR.make_enc("ligero", fid, 0, digest, dims=(1, 2))
        for n in (1, 3, 9):
            DR.check_case(DR.RefCase(O, oenc, O.random_elems(fid, n, n + fid), digest), enc, "%s ft%d 1x2 n %d" % (digest, fid, n))


@pytest.mark.parametrize("digest", NEW)
@pytest.mark.parametrize("fid", [0, 1, 2, 3])
@pytest.mark.parametrize("log_n", [10, 14, 18, 20])
def test_hashes_ligero_sizes(oracle, fid, log_n, digest):
    n = 1 << log_n
    enc = LigeroEncoding.new(fid, n, digest=digest)
    cm = LcCommit.commit(DR.edge_elems(oracle, fid, n - (log_n % 3), log_n), enc)
    check_hashes(oracle, digest, fid, cm)


@pytest.mark.parametrize("digest", NEW)
@pytest.mark.parametrize("kind,fid,log_n", [("ligero", 0, 24), ("ligero", 3, 24), ("sdig", 3, 20), ("sdig", 0, 20), ("sdig", 2, 16)])
def test_hashes_large(oracle, kind, fid, log_n, digest):
    n = 1 << log_n
    enc = make_enc(kind, fid, n, digest)
    cm = LcCommit.commit(DR.edge_elems(oracle, fid, n, 24), enc)
    check_hashes(oracle, digest, fid, cm)


# ---- every last-block residue ----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("digest", NEW)
@pytest.mark.parametrize("fid", [0, 1, 2, 3])
def test_block_edges_device_and_host(oracle, fid, digest):
    O, L = oracle, DR.LIMBS[fid]
    rows = {k: v for k, v in DM.edge_rows(fid).items() if k[0] == digest}
    if digest == "sha256":
        assert rows == SHA256_EDGE_TABLE[fid]
    else:
        assert rows == {("keccak256", r): v for r, v in KECCAK_EDGE_TABLE[fid].items()}
    n_per_row, n_cols = 128, 256
    oenc = O.Encoding.ligero_from_dims(fid, n_per_row, n_cols)
    enc = DR.make_enc("ligero", fid, 0, digest, dims=(n_per_row, n_cols))
    seen = set()
    for (name, res), n_rows in sorted(rows.items(), key=str):
        if n_rows is None:
            continue
        for ragged in (0, 37):
            rc = DR.RefCase(O, oenc, DR.edge_elems(O, fid, n_rows * n_per_row - ragged, 100 + n_rows), digest)
            assert rc.n_rows == n_rows
            DR.check_case(rc, enc, "%s ft%d residue %d n_rows %d ragged %d" % (digest, fid, res, n_rows, ragged))
            seen.add((DM.sha256_residue(L, n_rows) if digest == "sha256" else DR.sha3_residue(L, n_rows), ragged))
    covered = sorted({r for r, _ in seen})
    if digest == "sha256":                                 # the (field, residue) pairs covered, stated: L = 2 reaches even residues,
        assert covered == {0: [0, 1, 6, 7], 1: [0, 6], 2: [0, 1, 6, 7], 3: [0]}[fid]     # L = 4 only 0 (and 4)
    else:
        assert covered == sorted(DR.SHA3_RESIDUES)
    assert seen == {(r, g) for r in covered for g in (0, 37)}


@pytest.mark.parametrize("digest", NEW)
@pytest.mark.parametrize("fid,lo,hi", [(0, 1, 23), (1, 1, 23), (2, 1, 23), (3, 1, 23), (0, 24, 60), (2, 24, 60), (3, 24, 60)])
def test_block_edges_brakedown(oracle, fid, lo, hi, digest):
    """Brakedown below 24 rows (row-major, Montgomery form: <NL, false>) and from 24 rows on (position-major, canonical: <NL, true>),
    n_cols not a power of two, at the smallest n_rows of the range that reaches each edge residue: Keccak-256 0 (a whole padding
    block) and 16 (one word left); SHA-256 0 (a block of padding alone), 7 (the length in one more block) and 6 (0x80 and the
    length side by side).  What a field cannot reach is stated: SHA-256 residue 7 needs an odd L, residue 6 an L that is not 4."""
    O, n_per_row, L = oracle, 40, DR.LIMBS[fid]
    fn, wanted = (DM.sha256_residue, (0, 6, 7)) if digest == "sha256" else (DR.sha3_residue, (0, 16))
    rows = {res: next((r for r in range(lo, hi + 1) if fn(L, r) == res), None) for res in wanted}
    if digest == "sha256":
        assert {r for r, v in rows.items() if v is not None} == {1: {0, 6, 7}, 2: {0, 6}, 3: {0, 6, 7}, 4: {0}}[L]
    else:
        assert all(v is not None for v in rows.values())
    assert DR.leaf_canon_in(fid, "sdig", 0, lo) == (lo >= 24) == DR.leaf_canon_in(fid, "sdig", 0, hi)
    n_rows_list = sorted(v for v in rows.values() if v is not None)
    oenc = O.Encoding.sdig_from_dims(fid, n_per_row, 0, 3, DR.SDIG_CODE)
    _, _, n_cols = oenc.get_dims(n_per_row)
    enc = SdigEncoding.new_from_dims(fid, n_per_row, n_cols, 3, DR.SDIG_CODE, digest=digest)
    for n_rows in n_rows_list:
        rc = DR.RefCase(O, oenc, DR.edge_elems(O, fid, n_rows * n_per_row - 3, 200 + n_rows), digest)
        assert rc.n_rows == n_rows and rc.n_cols & (rc.n_cols - 1)
        DR.check_case(rc, enc, "%s sdig ft%d n_rows %d" % (digest, fid, n_rows))


# ---- every commit entry point ----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("digest", NEW)
@pytest.mark.parametrize("kind,fid,log_n", [("ligero", 3, 21), ("ligero", 1, 16), ("sdig", 3, 14)])
def test_entry_points_same_hashes(oracle, kind, fid, log_n, digest):
    import torch
    n = 1 << log_n
    coeffs = DR.edge_elems(oracle, fid, n, 11)
    enc = make_enc(kind, fid, n, digest)
    pageable = LcCommit.commit(coeffs, enc)              # Ft255 2^21 = 64 MiB: the row-batch host path
    want = check_hashes(oracle, digest, fid, pageable)
    root, wh = want[-1].tobytes(), pageable.hashes()
    pinned = torch.from_numpy(coeffs.view(np.int64)).pin_memory()
    assert np.array_equal(LcCommit.commit(pinned.numpy().view(np.uint64), enc).hashes(), wh)
    refill = LcCommit.commit(np.array(coeffs, copy=True), enc, into=pageable)
    assert refill is pageable and refill.get_root() == root and np.array_equal(refill.hashes(), wh)
    dev = torch.from_numpy(coeffs.view(np.int64)).cuda()
    torch.cuda.synchronize()
    cd = LcCommit.commit_device(dev.data_ptr(), n, enc)
    assert cd.get_root() == root and np.array_equal(cd.hashes(), wh)
    if n % enc.n_per_row == 0:
        cbor = LcCommit.commit_device(dev.data_ptr(), n, enc, borrow=True)
        assert cbor.get_root() == root and np.array_equal(cbor.hashes(), wh)
    fp = LcCommit.from_parts(enc, pageable.comm(), pageable.coeffs(), pageable.n_rows)
    assert np.array_equal(fp.hashes(), wh)
    LcCommit.commit_device(dev.data_ptr(), n, enc, into=fp)
    assert np.array_equal(fp.hashes(), wh)
    buf = io.BytesIO()
    cd.to_bincode(buf)
    assert len(buf.getvalue()) == cd.bincode_size()
    back = LcCommit.from_bincode(enc, io.BytesIO(buf.getvalue()))
    assert back.get_root() == root and np.array_equal(back.hashes(), wh) and np.array_equal(back.comm(), pageable.comm())


@pytest.mark.parametrize("kind,fid", [("ligero", 3), ("sdig", 1)])
def test_bincode_of_another_digest_is_refused(oracle, kind, fid):
    n = 1 << 12
    coeffs = DR.edge_elems(oracle, fid, n, 12)
    encs = {d: make_enc(kind, fid, n, d) for d in ALL_FIVE}
    blobs, roots = {}, {}
    for d, e in encs.items():
        c = LcCommit.commit(coeffs, e)
        b = io.BytesIO()
        c.to_bincode(b)
        blobs[d], roots[d] = b.getvalue(), c.get_root()
    assert len(set(roots.values())) == 5                  # Keccak-256 is not SHA3-256: every root differs
    for d in NEW:
        for other in ALL_FIVE:
            if other == d:
                assert LcCommit.from_bincode(encs[d], io.BytesIO(blobs[d])).get_root() == roots[d]
                continue
            for enc, blob in ((encs[d], blobs[other]), (encs[other], blobs[d])):
                with pytest.raises(LcpcError) as e:
                    LcCommit.from_bincode(enc, io.BytesIO(blob))
                assert e.value.code == ERR_COMMIT, (d, other)
        for i in (0, 2 * (1 << (encs[d].n_cols - 1).bit_length()) - 2):     # one tampered digest: a leaf and the root
            nh = 2 * (1 << (encs[d].n_cols - 1).bit_length()) - 1
            bad = bytearray(blobs[d])
            bad[len(bad) - 40 * (nh - i) + 8 + 17] ^= 0x01
            with pytest.raises(LcpcError) as e:
                LcCommit.from_bincode(encs[d], io.BytesIO(bytes(bad)))
            assert e.value.code == ERR_COMMIT


# ---- proofs: bytes, verify, the mutation sweep --------------------------------------------------------------------------------------

def lib_verdict(enc, rc, blob, root=None):
    try:
        ev = LcEvalProof.from_bytes(blob, enc.L).verify(rc.root if root is None else root, rc.outer, rc.inner, enc,
                                                        DR.mk_tr(Transcript, rc.root, rc.nco))
        return 0, ev
    except LcpcError as e:
        return e.code, None


@pytest.mark.parametrize("digest", NEW)
@pytest.mark.parametrize("shape", DR.SWEEP_SHAPES, ids=DR.SWEEP_IDS)
def test_mutated_proofs_same_verdict_as_reference(oracle, shape, digest):
    O = oracle
    kind, fid, n, dims = shape
    dl = 32
    rc = DR.RefCase(O, DR.make_oenc(O, kind, fid, n, 1, dims), DR.edge_elems(O, fid, n, 5 + fid), digest)
    enc = DR.make_enc(kind, fid, n, digest, 1, dims)
    c = DR.check_case(rc, enc, "%s %s" % (digest, shape))          # hashes, proof bytes == the reference prover's, verify accepts
    pf = rc.proof
    # opened paths fold to the root, for sampled columns incl. column 0 and n_cols - 1
    cols = np.unique(np.array([0, rc.n_cols - 1] + [int(x) for x in np.random.default_rng(fid).integers(0, rc.n_cols, 6)], np.uint64))
    vals, paths = c.open_columns(cols)
    hs = rc.hashes()
    for k, col in enumerate(cols):
        sibs = [paths[k, i].tobytes() for i in range(max(0, (rc.n_cols - 1).bit_length()))]
        assert DM.fold(digest, hs[int(col)].tobytes(), int(col), sibs) == rc.root, int(col)
    cases = DR.mutation_cases(pf, rc.L, rc.n_per_row, rc.n_rows, 1000 + fid, dl, rc.n_cols)
    cases += DR.digest_cases(pf, rc.L, rc.n_per_row, rc.n_rows, rc.n_cols, dl, rc.nco)
    assert DR.count_unreduced(rc.F, cases, dl) <= len(cases) // 3
    n_strict = 0
    for name, blob in cases:
        code, _ = lib_verdict(enc, rc, blob)
        want = rc.verdict(blob)
        assert code != 0, name                             # never accepts a mutated proof
        assert isinstance(want, str), name                 # nor does the reference
        if code == VERR_MALFORMED and DR.VERR[want] != code:
            n_strict += 1                                  # stricter on purpose: unreduced limbs
            continue
        assert code == DR.VERR[want], (name, code, want)
    assert n_strict <= len(cases) // 3
    bad_root = rc.root[:-1] + bytes([rc.root[-1] ^ 1])
    assert lib_verdict(enc, rc, pf, bad_root)[0] == VERR_COLUMN_PATH == DR.VERR[rc.verdict(pf, root=bad_root)]
    # the proof handed to an encoder of each other digest, and a proof of each other 32-byte digest handed to this one
    for other in ALL_FIVE:
        if other == digest:
            continue
        eo = DR.make_enc(kind, fid, n, other, 1, dims)
        root_o = (rc.root + bytes(64))[:DR.DLEN[other]]
        code, _ = lib_verdict(eo, rc, pf, root_o)
        want = rc.verdict(pf, root=root_o, digest=DR.ref_digest(other, O))
        assert code != 0 and code == DR.VERR[want], (other, code, want)
        assert want == ("Malformed" if DR.DLEN[other] != dl else "ColumnPath")
    ro = DR.RefCase(O, rc.oenc, rc.coeffs, "sha3_256" if digest == "keccak256" else "keccak256")
    # a whole proof made under another 32-byte digest (its own root, its own transcript) -- a SHA3-256 proof under a Keccak-256
    # encoder, a Keccak-256 proof under a SHA-256 one: the paths do not fold to that root
    assert lib_verdict(enc, ro, ro.proof)[0] == VERR_COLUMN_PATH == DR.VERR[ro.verdict(ro.proof, digest=rc.D)]
    for blob in (pf, pf + b"\0", pf + bytes(13)):
        code, ev = lib_verdict(enc, rc, blob)
        assert code == 0 and np.array_equal(ev, rc.eval_limbs())


@pytest.mark.parametrize("digest", NEW)
def test_four_threads_prove_and_verify_one_commitment(oracle, digest):
    fid, n = 3, 1 << 16
    enc = LigeroEncoding.new(fid, n, digest=digest)
    c = LcCommit.commit(DR.edge_elems(oracle, fid, n, 31), enc)
    outer, inner = oracle.random_elems(fid, c.n_rows, 32), oracle.random_elems(fid, c.n_per_row, 33)
    root, nco = c.get_root(), enc.get_n_col_opens()
    want = c.prove(outer, enc, DR.mk_tr(Transcript, root, nco)).to_bytes()
    ev = LcEvalProof.from_bytes(want, enc.L).verify(root, outer, inner, enc, DR.mk_tr(Transcript, root, nco))
    got, errs = [None] * 4, []

    def run(i):
        try:
            for _ in range(3):
                b = c.prove(outer, enc, DR.mk_tr(Transcript, root, nco)).to_bytes()
                e = LcEvalProof.from_bytes(b, enc.L).verify(root, outer, inner, enc, DR.mk_tr(Transcript, root, nco))
                if b != want or not np.array_equal(e, ev):
                    got[i] = b
                    return
            got[i] = want
        except Exception as ex:       # surfaced below
            errs.append(ex)

    th = [threading.Thread(target=run, args=(i,)) for i in range(4)]
    for t in th:
        t.start()
    for t in th:
        t.join()
    assert not errs, errs
    assert got == [want] * 4


# ---- full size -------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("digest", NEW)
def test_fullsize_ft255_2_26(oracle, digest):
    """2^26 Ft255 (512 x 262144 after encoding): 64 sampled leaves (columns 0 and n_cols - 1 among them) against the reference
    computed from the columns of lcpc_get_comm, and the root and every tree level recomputed by the reference from the GPU's
    leaves (the 2^18 leaves in Python would take minutes; 64 are checked)"""
    import sha3_ref
    import torch
    fid, n = 3, 1 << 26
    enc = LigeroEncoding.new(fid, n, digest=digest)
    coeffs = enc.random_coeffs_device(n, 26)
    torch.cuda.synchronize()
    c = LcCommit.commit_device(coeffs.data_ptr(), n, enc)
    assert (c.n_rows, c.n_cols) == (512, 1 << 18)
    hs = c.hashes()
    np2 = 1 << 18
    level, off = hs[:np2], np2
    while len(level) > 1:
        level = DM.many(digest, np.ascontiguousarray(level).reshape(len(level) // 2, 64))
        assert np.array_equal(level, hs[off:off + len(level)]), len(level)
        off += len(level)
    assert c.get_root() == level[0].tobytes() == hs[-1].tobytes()
    cols = np.unique(np.random.default_rng(26).integers(0, c.n_cols, 80))[:62].tolist() + [0, c.n_cols - 1]
    cols = sorted(set(cols))
    assert len(cols) == 64
    comm = c.comm().reshape(c.n_rows, c.n_cols, 4)
    sel = np.ascontiguousarray(comm[:, cols].transpose(1, 0, 2))
    del comm
    rep = sha3_ref.repr_bytes(oracle, fid, sel.reshape(-1, 4)).reshape(len(cols), -1)
    D = DM.DIGESTS[digest]
    _, paths = c.open_columns(np.array(cols, np.uint64))
    for k, col in enumerate(cols):
        lf = D(bytes(32) + rep[k].tobytes())
        assert lf == hs[col].tobytes(), col
        assert DM.fold(digest, lf, col, [paths[k, i].tobytes() for i in range(paths.shape[1])]) == c.get_root()

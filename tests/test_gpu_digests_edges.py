"""The three digests of LcCommit<D, E> -- BLAKE3, SHA3-256, BLAKE2b-512 -- against ONE reference (oracle/pyref.py with its digest
parameter, tests/digest_ref.py), at the places where a hand-written sponge or HAIFA hash goes wrong: the last block of the leaf
message.  Every case checks the device (the whole `hashes` array) and the host (lcpc_verify hashes the opened columns with
host_crypto.cpp) at the same edge: the library's proof is the reference prover's byte for byte, and verifies to its evaluation.

The SHA3-256 leaf message is 4 + L n_rows 64-bit words absorbed 17 at a time; the BLAKE2b one 8 + L n_rows words in blocks of 16.
Residues the test reaches, derived by digest_ref.edge_rows and asserted below (n_rows in 1..70, smallest that fits):

    field  L   SHA3 residue 0 / 1 / 8 / 15 / 16 -> n_rows     BLAKE2b residue 0 / 1 / 15 -> n_rows
    Ft63   1   13 / 14 / 4 / 11 / 12                           8 / 9 / 7
    Ft127  2   15 / 7 / 2 / 14 / 6                             4 / - / -      (8 + 2 n_rows is even)
    Ft191  3   10 / 16 / 7 / 15 / 4                            8 / 3 / 13
    Ft255  4   16 / 12 / 1 / 7 / 3                             2 / - / -      (8 + 4 n_rows = 0 mod 4)
"""
import numpy as np
import pytest

import digest_ref as DR
from lcpc_amd import LcCommit, LcEvalProof, LcpcError, Transcript

pytestmark = pytest.mark.gpu

EDGE_TABLE = {
    0: {("sha3_256", 0): 13, ("sha3_256", 1): 14, ("sha3_256", 8): 4, ("sha3_256", 15): 11, ("sha3_256", 16): 12,
        ("blake2b", 0): 8, ("blake2b", 1): 9, ("blake2b", 15): 7},
    1: {("sha3_256", 0): 15, ("sha3_256", 1): 7, ("sha3_256", 8): 2, ("sha3_256", 15): 14, ("sha3_256", 16): 6,
        ("blake2b", 0): 4, ("blake2b", 1): None, ("blake2b", 15): None},
    2: {("sha3_256", 0): 10, ("sha3_256", 1): 16, ("sha3_256", 8): 7, ("sha3_256", 15): 15, ("sha3_256", 16): 4,
        ("blake2b", 0): 8, ("blake2b", 1): 3, ("blake2b", 15): 13},
    3: {("sha3_256", 0): 16, ("sha3_256", 1): 12, ("sha3_256", 8): 1, ("sha3_256", 15): 7, ("sha3_256", 16): 3,
        ("blake2b", 0): 2, ("blake2b", 1): None, ("blake2b", 15): None},
}


def check_case(O, rc, enc, label):
    return DR.check_case(rc, enc, label)


@pytest.mark.parametrize("digest", DR.DIGEST_NAMES)
@pytest.mark.parametrize("fid", [0, 1, 2, 3])
def test_block_edges_device_and_host(oracle, fid, digest):
    O, L = oracle, DR.LIMBS[fid]
    rows = DR.edge_rows(fid)
    assert rows == EDGE_TABLE[fid]                         # the table of the module docstring, derived, not hand-picked
    n_per_row, n_cols = 128, 256
    oenc = O.Encoding.ligero_from_dims(fid, n_per_row, n_cols)
    enc = DR.make_enc("ligero", fid, 0, digest, dims=(n_per_row, n_cols))
    assert enc.digest == digest and enc.digest_len == DR.DLEN[digest]
    seen = set()
    for (name, res), n_rows in sorted(rows.items(), key=str):
        if n_rows is None or (digest != "blake3" and name != digest):
            continue                                       # (BLAKE3 rides along at every n_rows of both lists)
        for ragged in (0, 37):
            coeffs = DR.edge_elems(O, fid, n_rows * n_per_row - ragged, 100 + n_rows)
            rc = DR.RefCase(O, oenc, coeffs, digest)
            assert rc.n_rows == n_rows
            check_case(O, rc, enc, "%s ft%d %s residue %d n_rows %d ragged %d" % (digest, fid, name, res, n_rows, ragged))
            seen.add((name, DR.sha3_residue(L, n_rows) if name == "sha3_256" else DR.blake2b_residue(L, n_rows), ragged))
    want = {(n, r, g) for (n, r), v in rows.items() if v is not None and (digest == "blake3" or n == digest) for g in (0, 37)}
    assert seen == want
    if digest == "sha3_256":
        assert {r for _, r, _ in seen} == set(DR.SHA3_RESIDUES)
    if digest == "blake2b":
        assert {r for _, r, _ in seen} == (set(DR.BLAKE2B_RESIDUES) if L % 2 else {0})


# Brakedown (n_per_row 40): n_rows per (digest, residue) in the row-major range 1..23 and the position-major range 24..60; BLAKE2b's
# residue 15 needs an odd L, so Ft255 has none
SDIG_EDGE_ROWS = {
    (2, 24): {("sha3_256", 0): 27, ("sha3_256", 16): 38, ("blake2b", 0): 24, ("blake2b", 15): 29},
    (2, 1): {("sha3_256", 0): 10, ("sha3_256", 16): 4, ("blake2b", 0): 8, ("blake2b", 15): 13},
    (3, 24): {("sha3_256", 0): 33, ("sha3_256", 16): 37, ("blake2b", 0): 26, ("blake2b", 15): None},
    (0, 1): {("sha3_256", 0): 13, ("sha3_256", 16): 12, ("blake2b", 0): 8, ("blake2b", 15): 7},
}


def sdig_rows(fid, lo, hi):
    """n_rows in [lo, hi] at SHA3 residue 0 and 16 and BLAKE2b residue 0 (and 15 where the field reaches it)"""
    L = DR.LIMBS[fid]
    out = {}
    for name, fn, wanted in (("sha3_256", DR.sha3_residue, (0, 16)), ("blake2b", DR.blake2b_residue, (0, 15))):
        for res in wanted:
            out[(name, res)] = next((r for r in range(lo, hi + 1) if fn(L, r) == res), None)
    return out


@pytest.mark.parametrize("digest", DR.DIGEST_NAMES)
@pytest.mark.parametrize("fid,lo,hi", [(2, 24, 60), (2, 1, 23), (3, 24, 60), (0, 1, 23)])
def test_block_edges_brakedown(oracle, fid, lo, hi, digest):
    """the position-major commitment (>= 24 rows: the leaf kernels read canonical values at stride n_rows) and the row-major one
    below, at a whole padding block / an exactly full block and at the last-word residue"""
    O = oracle
    n_per_row = 40
    oenc = O.Encoding.sdig_from_dims(fid, n_per_row, 0, 3, DR.SDIG_CODE)
    _, _, n_cols = oenc.get_dims(n_per_row)
    from lcpc_amd import SdigEncoding
    enc = SdigEncoding.new_from_dims(fid, n_per_row, n_cols, 3, DR.SDIG_CODE, digest=digest)
    rows = sdig_rows(fid, lo, hi)
    assert rows == SDIG_EDGE_ROWS[(fid, lo)]               # derived; the table pins what the derivation must keep reaching
    assert all(n is None or (n >= 24) == (lo >= 24) for n in rows.values())
    done = set()
    for (name, res), n_rows in sorted(rows.items(), key=str):
        if n_rows is None or (digest != "blake3" and name != digest):
            continue
        coeffs = DR.edge_elems(O, fid, n_rows * n_per_row - 3, 200 + n_rows)
        rc = DR.RefCase(O, oenc, coeffs, digest)
        assert rc.n_rows == n_rows and rc.n_cols & (rc.n_cols - 1)          # leaf slots beyond n_cols: Output<D>::default()
        check_case(O, rc, enc, "%s sdig ft%d %s residue %d n_rows %d" % (digest, fid, name, res, n_rows))
        done.add((name, res))
    assert done == {k for k, v in SDIG_EDGE_ROWS[(fid, lo)].items() if v is not None and (digest == "blake3" or k[0] == digest)}


@pytest.mark.parametrize("digest", DR.DIGEST_NAMES)
@pytest.mark.parametrize("fid", [0, 1, 2, 3])
@pytest.mark.parametrize("n_per_row,n_cols", [(1, 2), (1, 4), (3, 4), (7, 8), (2, 16)])
def test_tiny_shapes(oracle, fid, n_per_row, n_cols, digest):
    """tests/test_gpu_edges.py::test_tiny_shapes under every digest"""
    O = oracle
    oenc = O.Encoding.ligero_from_dims(fid, n_per_row, n_cols)
    enc = DR.make_enc("ligero", fid, 0, digest, dims=(n_per_row, n_cols))
    for n in (1, n_per_row, n_per_row + 1, 5 * n_per_row - (1 if n_per_row > 1 else 0)):
        rc = DR.RefCase(O, oenc, O.random_elems(fid, n, n + n_cols), digest)
        check_case(O, rc, enc, "%s ft%d %dx%d n %d" % (digest, fid, n_per_row, n_cols, n))


@pytest.mark.parametrize("digest", DR.DIGEST_NAMES)
@pytest.mark.parametrize("fid", [0, 1, 2, 3])
def test_refill_with_other_row_counts(oracle, fid, digest):
    """one LcCommit refilled under one encoder with more rows, then fewer: a stale leaf slot or tree level would show in `hashes`"""
    O = oracle
    n_per_row, n_cols = 96, 256
    oenc = O.Encoding.ligero_from_dims(fid, n_per_row, n_cols)
    enc = DR.make_enc("ligero", fid, 0, digest, dims=(n_per_row, n_cols))
    c = LcCommit(enc)
    for n_rows in (5, 33, 2, 33, 1):
        rc = DR.RefCase(O, oenc, DR.edge_elems(O, fid, n_rows * n_per_row - 1, 300 + n_rows), digest)
        LcCommit.commit(rc.coeffs, enc, into=c)
        assert c.n_rows == n_rows and np.array_equal(c.hashes(), rc.hashes()) and c.get_root() == rc.root
        pf = c.prove(rc.outer, enc, DR.mk_tr(Transcript, rc.root, rc.nco)).to_bytes()
        assert pf == rc.proof


@pytest.mark.parametrize("digest", DR.DIGEST_NAMES)
@pytest.mark.parametrize("fid", [1, 2, 3])
def test_from_parts_n_cols_not_a_multiple_of_64(oracle, fid, digest):
    O, n_per_row, n_rows = oracle, 40, 6
    oenc = O.Encoding.sdig_from_dims(fid, n_per_row, 0, 3, DR.SDIG_CODE)
    _, _, n_cols = oenc.get_dims(n_per_row)
    assert n_cols % 64
    from lcpc_amd import SdigEncoding
    enc = SdigEncoding.new_from_dims(fid, n_per_row, n_cols, 3, DR.SDIG_CODE, digest=digest)
    rc = DR.RefCase(O, oenc, DR.edge_elems(O, fid, n_rows * n_per_row, 7), digest)
    c = LcCommit.from_parts(enc, rc.oc.comm(), rc.oc.coeffs(), n_rows)
    assert np.array_equal(c.hashes(), rc.hashes()) and c.get_root() == rc.root
    pf = c.prove(rc.outer, enc, DR.mk_tr(Transcript, rc.root, rc.nco)).to_bytes()
    assert pf == rc.proof

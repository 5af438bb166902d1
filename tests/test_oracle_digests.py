"""The digest-generic reference (oracle/pyref.py with its `digest` parameter, the bincode proof parser and verify_bytes) before it
is trusted for SHA3-256 and BLAKE2b: with BLAKE3 it must be the C oracle bit for bit -- the `hashes` array, the proof bytes and
the verdict on every mutated proof of the verifier sweep -- and with the two hashlib digests it must agree with the second
statement of the tree (tests/sha3_ref.py, tests/blake2b_ref.py), round-trip its own proofs through the parser, and reproduce the
committed fixtures of tests/golden/digest_cases.json.  CPU only."""
import importlib.util
import os

import numpy as np
import pytest

import digest_ref as DR
import pyref as P
from common import load_golden, mk_transcript



def ref_case(O, shape, digest, seed=5):
    kind, fid, n, dims = shape
    return DR.RefCase(O, DR.make_oenc(O, kind, fid, n, 1, dims), DR.edge_elems(O, fid, n, seed + fid), digest)


@pytest.mark.parametrize("shape", DR.SWEEP_SHAPES, ids=DR.SWEEP_IDS)
def test_blake3_parameter_is_the_c_oracle(oracle, shape):
    O = oracle
    rc = ref_case(O, shape, "blake3")
    # the tree, with pyref's own BLAKE3 as well as the C one behind the same parameter
    assert np.array_equal(rc.hashes(), rc.oc.hashes()) and rc.root == rc.oc.get_root()
    if rc.n_cols <= 256:
        pure = DR.pyref_commit(O, rc.fid, rc.oc, P.BLAKE3)
        assert pure.hashes == rc.c.hashes
    # the proof bytes
    opf, ocols = rc.oc.prove(rc.outer, rc.oenc, mk_transcript(O.Transcript, rc.root, rc.nco))
    assert rc.proof == opf and list(ocols) == rc.cols
    assert len(opf) == P.proof_size(rc.F, rc.n_rows, rc.n_per_row, rc.n_cols, rc.nco, rc.oenc.get_n_degree_tests())
    # parse -> serialise is the identity
    assert P.ser_proof(rc.F, P.deser_proof(rc.F, opf)) == opf
    # the verdict on the verifier sweep's blobs: the same error, in the same order of checks, as lo_verify
    cases = DR.mutation_cases(opf, rc.L, rc.n_per_row, rc.n_rows, 1000 + rc.fid, 32, rc.n_cols)
    cases += DR.digest_cases(opf, rc.L, rc.n_per_row, rc.n_rows, rc.n_cols, 32, rc.nco)
    cases += [("whole", opf), ("trailing byte", opf + b"\0"), ("13 trailing bytes", opf + bytes(13))]
    for name, blob in cases:
        orc, oev = O.verify(rc.oenc, rc.root, rc.outer, rc.inner, blob, mk_transcript(O.Transcript, rc.root, rc.nco))
        got = rc.verdict(blob)
        if orc == 0:
            assert got == rc.eval and np.array_equal(oev, rc.eval_limbs()), name
            assert name in ("whole", "trailing byte", "13 trailing bytes"), name
        else:
            assert isinstance(got, str) and DR.VERR[got] == orc, (name, got, orc)
    # a wrong root and the two wrong tensor lengths
    bad_root = rc.root[:-1] + bytes([rc.root[-1] ^ 1])
    assert rc.verdict(opf, root=bad_root) == "ColumnPath"
    assert O.verify(rc.oenc, bad_root, rc.outer, rc.inner, opf, mk_transcript(O.Transcript, rc.root, rc.nco))[0] == DR.VERR["ColumnPath"]
    tr = DR.mk_tr(P.Transcript, rc.root, rc.nco)
    assert P.verify_bytes(rc.F, rc.D, rc.root, rc.outer_i + [1], rc.inner_i, opf, rc.enc, tr) == "OuterTensor"
    assert P.verify_bytes(rc.F, rc.D, rc.root, rc.outer_i, rc.inner_i[:-1] + [1, 1], opf, rc.enc, tr) == "InnerTensor"


@pytest.mark.parametrize("digest", ["sha3_256", "blake2b"])
@pytest.mark.parametrize("shape", DR.SWEEP_SHAPES, ids=DR.SWEEP_IDS)
def test_hashlib_digests_tree_roundtrip_and_sweep(oracle, shape, digest):
    O = oracle
    rc = ref_case(O, shape, digest)
    T, dl = DR.tree_ref(digest), DR.DLEN[digest]
    want = T.tree(T.leaves(O, rc.fid, rc.oc.comm(), rc.n_rows, rc.n_cols))
    assert rc.c.hashes == want and len(rc.root) == dl
    assert len(rc.proof) == P.proof_size(rc.F, rc.n_rows, rc.n_per_row, rc.n_cols, rc.nco, rc.oenc.get_n_degree_tests(), dl)
    pf = P.deser_proof(rc.F, rc.proof, dl)
    assert P.ser_proof(rc.F, pf) == rc.proof and pf.n_unreduced == 0
    np2 = (len(want) + 1) // 2
    for (col, path), cn in list(zip(pf.columns, rc.cols))[:16]:
        assert path == T.path(want, np2, cn) and T.fold(want[cn], cn, path) == rc.root
    assert rc.verdict(rc.proof) == rc.eval == rc.verdict(rc.proof + b"\0")
    # the proof means nothing under another digest: entries of the wrong length, or a path that does not fold to the root
    for other in DR.DIGEST_NAMES:
        if other != digest:
            want_err = "Malformed" if DR.DLEN[other] != dl else "ColumnPath"
            assert rc.verdict(rc.proof, digest=DR.ref_digest(other, O)) == want_err, other
    bad_root = rc.root[:-1] + bytes([rc.root[-1] ^ 1])
    assert rc.verdict(rc.proof, root=bad_root) == "ColumnPath"
    # the sweep the GPU tests run against the library: the reference rejects every case
    cases = DR.mutation_cases(rc.proof, rc.L, rc.n_per_row, rc.n_rows, 1000 + rc.fid, dl, rc.n_cols)
    cases += DR.digest_cases(rc.proof, rc.L, rc.n_per_row, rc.n_rows, rc.n_cols, dl, rc.nco)
    for name, blob in cases:
        assert isinstance(rc.verdict(blob), str), name
    by_name = dict((n, rc.verdict(b)) for n, b in cases[-8:])
    assert by_name["col0 digest second half"] == by_name["col0 digest last byte"] == "ColumnPath"
    assert by_name["col0 entry length %d" % (96 - dl)] == by_name["col0 last entry length %d" % (96 - dl)] == "Malformed"


@pytest.mark.parametrize("digest", DR.DIGEST_NAMES)
@pytest.mark.parametrize("shape", DR.SWEEP_SHAPES, ids=DR.SWEEP_IDS)
def test_sweep_cases_with_unreduced_limbs_stay_under_a_third(oracle, shape, digest):
    """the library refuses a limb vector >= p as malformed where the reference computes mod p; the sweeps
    allow that difference for at most a third of their cases.  Which cases can fall under it is a property of the bytes: count
    them here, for the very proofs the GPU sweep mutates."""
    rc = ref_case(oracle, shape, digest)
    dl = DR.DLEN[digest]
    cases = DR.mutation_cases(rc.proof, rc.L, rc.n_per_row, rc.n_rows, 1000 + rc.fid, dl, rc.n_cols)
    cases += DR.digest_cases(rc.proof, rc.L, rc.n_per_row, rc.n_rows, rc.n_cols, dl, rc.nco)
    n = DR.count_unreduced(rc.F, cases, dl)
    assert 1 <= n <= len(cases) // 3, (n, len(cases))          # at least the crafted "p_eval[0] >= p"


def test_parser_refuses_what_bincode_refuses(oracle):
    rc = ref_case(oracle, DR.SWEEP_SHAPES[3], "blake2b")
    F, pf = rc.F, rc.proof
    o = DR.proof_layout(pf, rc.L, rc.n_per_row, rc.n_rows, rc.n_cols, 64)
    P.deser_proof(F, pf, 64)
    for dl in (32, 63, 65, 0):
        with pytest.raises(P.MalformedProof):
            P.deser_proof(F, pf, dl)
    for cut in (0, 7, 15, 16, o["nd"] + 3, o["ncol"] + 7, o["dig0"], o["dig0"] + 63, len(pf) - 1):
        with pytest.raises(P.MalformedProof):
            P.deser_proof(F, pf[:cut], 64)
    for pos in (8, o["nd"], o["ncol"], o["col0"], o["plen0"]):   # a count of 2^56 and more at every length prefix
        b = bytearray(pf)
        b[pos + 7] = 1
        with pytest.raises(P.MalformedProof):
            P.deser_proof(F, bytes(b), 64)
    b = bytearray(pf)
    b[o["ncol"]] ^= 1
    with pytest.raises(P.VerifierError):
        P.deser_proof(F, bytes(b), 64, rc.nco)


def test_published_proof_sizes_with_the_digest_length():
    """proof_size(dl = 32) is the formula the 36 published sizes pin (tests/test_oracle_vs_pyref.py); a 64-byte digest adds 32
    bytes per path entry and nothing else"""
    for F in P.FIELDS:
        for lg in (10, 12):
            nr, npr, nc = P.LigeroEncoding.get_dims_len(F, 1 << lg)
            enc = P.LigeroEncoding(F, npr, nc)
            a = P.proof_size(F, nr, npr, nc, enc.get_n_col_opens(), enc.get_n_degree_tests())
            assert a == P.proof_size(F, nr, npr, nc, enc.get_n_col_opens(), enc.get_n_degree_tests(), 32)
            b = P.proof_size(F, nr, npr, nc, enc.get_n_col_opens(), enc.get_n_degree_tests(), 64)
            assert b - a == 32 * enc.get_n_col_opens() * P.log2_ceil(nc)


def test_digest_cases_golden_regenerates():
    here = os.path.dirname(os.path.abspath(__file__))
    spec = importlib.util.spec_from_file_location("make_golden", os.path.join(here, "golden", "make_golden.py"))
    mg = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mg)
    want = load_golden("digest_cases.json")
    got = mg.digest_cases()
    assert [c["name"] for c in got] == [c["name"] for c in want]
    for g, w in zip(got, want):
        assert g == w, w["name"]
    assert {c["digest"] for c in want} == set(DR.DIGEST_NAMES) and {c["field"] for c in want} == {0, 1, 2, 3}
    assert {c["enc"]["kind"] for c in want} == {"ligero", "sdig"}
    assert any(c["n_cols"] & (c["n_cols"] - 1) for c in want) and any(c["n_coeffs"] % c["n_per_row"] for c in want)

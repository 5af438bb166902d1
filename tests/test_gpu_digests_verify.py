"""lcpc_verify and the commitment's serde under every digest, on bytes they must not trust: the mutated proofs of
tests/test_gpu_verify_mutations.py with their offsets computed from the digest length, the mutations that only exist because
digests have a length (tests/digest_ref.py digest_cases), a wrong root, a proof of one digest handed to an encoder of another --
never an accept, and the VerifierError the digest-generic reference (oracle/pyref.py verify_bytes) reports for the same bytes,
except where the library is stricter by design (limbs >= p -> VERR_MALFORMED).  And the committed
fixtures of tests/golden/digest_cases.json end to end."""
import hashlib
import io
import random

import numpy as np
import pytest

import digest_ref as DR
import lcpc_amd
from common import golden_coeffs, load_golden
from lcpc_amd import LcCommit, LcEvalProof, LcpcError, LigeroEncoding, SdigEncoding, Transcript

pytestmark = pytest.mark.gpu



def lib_verdict(enc, rc, blob, root=None):
    """lcpc_status of the library's verify (0 and the evaluation on an accept)"""
    try:
        ev = LcEvalProof.from_bytes(blob, enc.L).verify(rc.root if root is None else root, rc.outer, rc.inner, enc,
                                                        DR.mk_tr(Transcript, rc.root, rc.nco))
        return 0, ev
    except LcpcError as e:
        return e.code, None


@pytest.mark.parametrize("digest", DR.DIGEST_NAMES)
@pytest.mark.parametrize("shape", DR.SWEEP_SHAPES, ids=DR.SWEEP_IDS)
def test_mutated_proofs_same_verdict_as_reference(oracle, shape, digest):
    O = oracle
    kind, fid, n, dims = shape
    dl = DR.DLEN[digest]
    rc = DR.RefCase(O, DR.make_oenc(O, kind, fid, n, 1, dims), DR.edge_elems(O, fid, n, 5 + fid), digest)
    enc = DR.make_enc(kind, fid, n, digest, 1, dims)
    c = LcCommit.commit(rc.coeffs, enc)
    assert c.get_root() == rc.root
    pf = c.prove(rc.outer, enc, DR.mk_tr(Transcript, rc.root, rc.nco)).to_bytes()
    assert pf == rc.proof                                  # so the blobs below are the ones the CPU tests counted and judged
    code, ev = lib_verdict(enc, rc, pf)
    assert code == 0 and np.array_equal(ev, rc.eval_limbs()) and rc.verdict(pf) == rc.eval
    cases = DR.mutation_cases(pf, rc.L, rc.n_per_row, rc.n_rows, 1000 + fid, dl, rc.n_cols)
    cases += DR.digest_cases(pf, rc.L, rc.n_per_row, rc.n_rows, rc.n_cols, dl, rc.nco)
    assert DR.count_unreduced(rc.F, cases, dl) <= len(cases) // 3
    n_strict = 0
    for name, blob in cases:
        code, _ = lib_verdict(enc, rc, blob)
        want = rc.verdict(blob)
        assert code != 0, name                             # never accepts a mutated proof
        assert isinstance(want, str), name                 # nor does the reference
        if code == lcpc_amd.VERR_MALFORMED and DR.VERR[want] != code:
            n_strict += 1                                  # stricter on purpose: unreduced limbs
            continue
        assert code == DR.VERR[want], (name, code, want)
    assert n_strict <= len(cases) // 3
    # a root that differs in its last byte
    bad_root = rc.root[:-1] + bytes([rc.root[-1] ^ 1])
    assert lib_verdict(enc, rc, pf, bad_root)[0] == lcpc_amd.VERR_COLUMN_PATH == DR.VERR[rc.verdict(pf, root=bad_root)]
    # the proof handed to an encoder of each other digest
    for other in DR.DIGEST_NAMES:
        if other == digest:
            continue
        eo = DR.make_enc(kind, fid, n, other, 1, dims)
        root_o = (rc.root + bytes(64))[:DR.DLEN[other]]
        code, _ = lib_verdict(eo, rc, pf, root_o)
        want = rc.verdict(pf, root=root_o, digest=DR.ref_digest(other, O))
        assert code != 0 and code == DR.VERR[want], (other, code, want)
        assert want == ("Malformed" if DR.DLEN[other] != dl else "ColumnPath")
    # the untouched proof still verifies (no state left behind by the failures); trailing bytes are ignored
    for blob in (pf, pf + b"\0", pf + bytes(13)):
        code, ev = lib_verdict(enc, rc, blob)
        assert code == 0 and np.array_equal(ev, rc.eval_limbs())


def golden_enc(case, cls_l=LigeroEncoding, cls_s=SdigEncoding):
    e, fid, d = case["enc"], case["field"], case["digest"]
    if e["kind"] == "ligero":
        if "length" in e:
            return cls_l.new(fid, e["length"], rho=tuple(e["rho"]), digest=d)
        return cls_l.new_from_dims(fid, e["n_per_row"], e["n_cols"], rho=tuple(e["rho"]), digest=d)
    return cls_s.new(fid, e["length"], e["seed"], e["code"], digest=d)


@pytest.mark.parametrize("case", load_golden("digest_cases.json"), ids=lambda c: c["name"])
def test_digest_goldens_end_to_end(oracle, case):
    """commit -> root, serde bytes, proof bytes, verify's evaluation: the fixtures pyref + hashlib wrote"""
    O, fid = oracle, case["field"]
    enc = golden_enc(case)
    c = LcCommit.commit(golden_coeffs(O, case), enc)
    assert (c.n_rows, c.n_per_row, c.n_cols) == (case["n_rows"], case["n_per_row"], case["n_cols"])
    root = c.get_root()
    assert root.hex() == case["root"] and len(root) == case["digest_len"]
    hs = c.hashes()
    assert hs[0].tobytes().hex() == case["leaf0"] and hashlib.sha256(hs.tobytes()).hexdigest() == case["hashes_sha256"]
    buf = io.BytesIO()
    c.to_bincode(buf)
    assert len(buf.getvalue()) == case["commit_bincode_len"] == c.bincode_size()
    assert hashlib.sha256(buf.getvalue()).hexdigest() == case["commit_bincode_sha256"]
    back = LcCommit.from_bincode(enc, io.BytesIO(buf.getvalue()))
    assert back.get_root() == root and np.array_equal(back.hashes(), hs)
    import pyref as P
    F, nco = P.FIELDS[fid], case["n_col_opens"]
    x = int(case["eval_point"], 16)
    inner = O.to_mont(fid, [pow(x, i, F.p) for i in range(c.n_per_row)])
    xr = pow(x, c.n_per_row, F.p)
    outer = O.to_mont(fid, [pow(xr, i, F.p) for i in range(c.n_rows)])
    pf = back.prove(outer, enc, DR.mk_tr(Transcript, root, nco))
    blob = pf.to_bytes()
    assert len(blob) == case["proof_len"] and hashlib.sha256(blob).hexdigest() == case["proof_sha256"]
    assert [int(v) for v in pf.cols_opened[:8]] == case["cols_opened_head"]
    ev = LcEvalProof.from_bytes(blob, enc.L).verify(root, outer, inner, enc, DR.mk_tr(Transcript, root, nco))
    assert O.to_canon_ints(fid, ev[None, :])[0] == int(case["eval"], 16)


@pytest.mark.parametrize("digest", DR.DIGEST_NAMES)
def test_commit_bincode_bad_streams_and_sweep(oracle, digest):
    """tests/test_gpu_commit_serde.py's bad streams and its mutation sweep with the offsets of a dl-byte digest: the reader
    refuses, or -- a flip inside `coeffs`, which no digest covers -- accepts with the same root"""
    O, fid, n = oracle, 1, 3000
    dl = DR.DLEN[digest]
    enc = LigeroEncoding.new(fid, n, digest=digest)
    c = LcCommit.commit(DR.edge_elems(O, fid, n, 15), enc)
    root = c.get_root()
    buf = io.BytesIO()
    c.to_bincode(buf)
    good = buf.getvalue()
    nr, npr, nc, F = c.n_rows, c.n_per_row, c.n_cols, 16
    coeffs_lo = 8 + nr * nc * F + 8
    coeffs_hi = coeffs_lo + nr * npr * F
    off_hashes = coeffs_hi + 24
    assert len(good) == off_hashes + 8 + c.n_hashes * (8 + dl)

    def status(b):
        with pytest.raises(LcpcError) as e:
            LcCommit.from_bincode(enc, io.BytesIO(bytes(b)))
        return e.value.code

    assert status(good[:-1]) == lcpc_amd.ERR_ARG
    for pos in (8 + 40, len(good) - 1, len(good) - dl, off_hashes + 8 + 8 + dl - 1, off_hashes + 8 + (8 + dl) * nc + 8 + dl // 2):
        bad = bytearray(good)
        bad[pos] ^= 1                                     # a comm element; the root's last and first byte; leaf 0's last byte; a filler slot
        assert status(bad) == lcpc_amd.ERR_COMMIT, pos
    for slot in (0, c.n_hashes - 1):                      # a digest announced with the other length
        bad = bytearray(good)
        q = off_hashes + 8 + slot * (8 + dl)
        bad[q:q + 8] = (96 - dl).to_bytes(8, "little")
        assert status(bad) in (lcpc_amd.ERR_COMMIT, lcpc_amd.ERR_ARG), slot
    rnd = random.Random(7)
    refused = 0
    for i in range(60):
        bad = bytearray(good)
        if i % 6 == 5:
            bad = bad[:rnd.randrange(len(bad))]
        else:
            pos = rnd.randrange(len(bad))
            bad[pos] ^= 1 << rnd.randrange(8)
        try:
            d = LcCommit.from_bincode(enc, io.BytesIO(bytes(bad)))
        except LcpcError as e:
            assert e.code in (lcpc_amd.ERR_ARG, lcpc_amd.ERR_COMMIT), e.code
            refused += 1
            continue
        assert len(bad) == len(good) and coeffs_lo <= pos < coeffs_hi, "a mutated stream outside coeffs was accepted (byte %d)" % pos
        assert d.get_root() == root
    assert refused >= 40

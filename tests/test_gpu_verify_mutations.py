"""The verifier on proofs it must not trust: random mutations of valid bincode proofs (bit flips in polynomials, column
values, path digests and length fields, truncations).  lcpc_verify (LcEvalProof::verify, lcpc-2d/src/lib.rs:832-952)
must neither crash nor accept, and must report the VerifierError the oracle's restatement of the reference reports for the
same bytes -- except where it is deliberately stricter: a limb vector >= p is refused as malformed,
where the reference computes on it mod p and fails later (or, for a column entry, not at all if the residue matches)."""
import pytest

import lcpc_amd
from common import mk_transcript, powers
from digest_ref import mutation_cases
from lcpc_amd import LcCommit, LcEvalProof, LigeroEncoding, SdigEncoding, Transcript

pytestmark = pytest.mark.gpu


def _setup(O, kind, fid, n, seed):
    coeffs = O.random_elems(fid, n, seed)
    if kind == "ligero":
        enc, oenc = LigeroEncoding.new(fid, n), O.Encoding.ligero(fid, n)
    else:
        enc, oenc = SdigEncoding.new(fid, n, 1), O.Encoding.sdig(fid, n, 1)
    c = LcCommit.commit(coeffs, enc)
    import pyref as P
    x = 0x1234567 % P.FIELDS[fid].p
    inner = powers(O, fid, x, c.n_per_row)
    outer = powers(O, fid, x, c.n_rows, c.n_per_row)
    root = c.get_root()
    nco = enc.get_n_col_opens()
    pf = c.prove(outer, enc, mk_transcript(Transcript, root, nco)).to_bytes()
    return enc, oenc, root, nco, inner, outer, bytes(pf), c


def _both(O, enc, oenc, root, nco, inner, outer, blob):
    try:                                                  # (deserialisation errors surface as VERR_MALFORMED too)
        LcEvalProof.from_bytes(blob, enc.L).verify(root, outer, inner, enc, mk_transcript(Transcript, root, nco))
        rc = 0
    except lcpc_amd.LcpcError as e:
        rc = e.code
    orc, _ = O.verify(oenc, root, outer, inner, blob, mk_transcript(O.Transcript, root, nco))
    return rc, orc


@pytest.mark.parametrize("kind,fid,n", [("ligero", 3, 1 << 12), ("ligero", 1, 1 << 11), ("sdig", 3, 1 << 11), ("ligero", 0, 1 << 10)])
def test_mutated_proofs_same_verdict_as_oracle(oracle, kind, fid, n):
    O = oracle
    enc, oenc, root, nco, inner, outer, pf, c = _setup(O, kind, fid, n, 5 + fid)
    assert _both(O, enc, oenc, root, nco, inner, outer, pf) == (0, 0)
    # the case list is shared with the sweeps under the other digests (tests/digest_ref.py: same generator, same draws)
    cases = mutation_cases(pf, enc.L, c.n_per_row, c.n_rows, 1000 + fid, 32, c.n_cols)
    assert len(cases) == 56
    n_strict = 0
    for name, blob in cases:
        rc, orc = _both(O, enc, oenc, root, nco, inner, outer, blob)
        assert rc != 0, name                              # never accepts a mutated proof
        assert orc != 0, name
        if rc == lcpc_amd.VERR_MALFORMED and orc != rc:
            n_strict += 1                                 # stricter on purpose: unreduced limbs (see the module docstring)
            continue
        assert rc == orc, (name, rc, orc)
    assert n_strict <= len(cases) // 3
    # and the untouched proof still verifies afterwards (no state left behind by the failures); trailing bytes are ignored,
    # as by bincode::deserialize (bincode 1.3's top-level functions allow them)
    assert _both(O, enc, oenc, root, nco, inner, outer, pf) == (0, 0)
    assert _both(O, enc, oenc, root, nco, inner, outer, pf + b"\0") == (0, 0)
    assert _both(O, enc, oenc, root, nco, inner, outer, pf + bytes(13)) == (0, 0)

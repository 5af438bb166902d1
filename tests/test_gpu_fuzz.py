"""Seeded random sweep of commit shapes against the oracle: field x rate x length for Ligero (every pass plan the
planner can produce up to 2^18 columns, all four fields (the specialised two-pass kernels K1s / K1n and the general kernel), ragged last rows, 1..600 rows), field x code x length for Brakedown.  Each
case checks comm, coeffs, every digest of the tree and one collapse; a few also run prove and compare proof bytes.
The *_digests functions draw the digest (BLAKE3, SHA3-256, BLAKE2b) per case from generators of the same kind, with seeds of their
own: the tree from tests/sha3_ref.py / tests/blake2b_ref.py (BLAKE3: the oracle), and on the small cases proof bytes and verify's
evaluation from the digest-generic reference (tests/digest_ref.py)."""
import random

import numpy as np
import pytest

from common import mk_transcript
from lcpc_amd import LcCommit, LigeroEncoding, SdigEncoding, Transcript

pytestmark = pytest.mark.gpu


def _check(O, c, oc, fid, enc, oenc, rnd, do_prove):
    assert (c.n_rows, c.n_per_row, c.n_cols) == (oc.n_rows, oc.n_per_row, oc.n_cols)
    assert (c.comm() == oc.comm()).all()
    assert (c.coeffs() == oc.coeffs()).all()
    assert (c.hashes() == oc.hashes()).all()
    t = O.random_elems(fid, c.n_rows, rnd.randrange(1 << 30))
    assert (c.eval_outer(t) == oc.collapse(t)).all()
    if do_prove:
        root = c.get_root()
        pf = c.prove(t, enc, mk_transcript(Transcript, root, enc.get_n_col_opens()))
        opf, _ = oc.prove(t, oenc, mk_transcript(O.Transcript, root, enc.get_n_col_opens()))
        assert pf.to_bytes() == opf


@pytest.mark.parametrize("seed", range(8))
def test_fuzz_ligero(oracle, seed):
    O = oracle
    rnd = random.Random(1000 + seed)
    for i in range(20):
        fid = rnd.choice([0, 1, 2, 3, 3, 3])
        rho = rnd.choice([(1, 2), (1, 2), (1, 4), (3, 4), (38, 39)])
        log_n = rnd.randrange(1, 19)
        n_cols = 1 << log_n
        n_per_row = max(1, min(n_cols - 1, n_cols * rho[0] // rho[1] - rnd.choice([0, 0, 1, 3])))
        max_rows = max(1, min(600, (1 << 19) // n_cols))
        n_rows = rnd.randrange(1, max_rows + 1)
        n = n_rows * n_per_row - rnd.randrange(0, n_per_row)
        enc = LigeroEncoding.new_from_dims(fid, n_per_row, n_cols, rho)
        oenc = O.Encoding.ligero_from_dims(fid, n_per_row, n_cols, rho)
        coeffs = O.random_elems(fid, n, rnd.randrange(1 << 30))
        c = LcCommit.commit(coeffs, enc)
        oc = O.Commit.commit(coeffs, oenc, n_threads=4)
        _check(O, c, oc, fid, enc, oenc, rnd, do_prove=(i % 4 == 0))


@pytest.mark.parametrize("seed", range(4))
def test_fuzz_brakedown(oracle, seed):
    O = oracle
    rnd = random.Random(2000 + seed)
    for i in range(6):
        fid = rnd.choice([0, 1, 2, 3, 3])
        code = rnd.randrange(1, 7)
        n_per_row = rnd.randrange(60, 3000)
        n_rows = rnd.choice([1, 2, 7, 15, 16, 17, 23, 24, 25, 40, 64, 65, 90, 130])
        n = n_rows * n_per_row - rnd.randrange(0, n_per_row)
        mseed = rnd.randrange(1 << 40)
        oenc = O.Encoding.sdig_from_dims(fid, n_per_row, 0, mseed, code)
        _, _, n_cols = oenc.get_dims(n_per_row)
        enc = SdigEncoding.new_from_dims(fid, n_per_row, n_cols, mseed, code)
        coeffs = O.random_elems(fid, n, rnd.randrange(1 << 30))
        c = LcCommit.commit(coeffs, enc)
        oc = O.Commit.commit(coeffs, oenc, n_threads=4)
        _check(O, c, oc, fid, enc, oenc, rnd, do_prove=(i == 0))


# ---- the digest drawn per case ----------------------------------------------------------------------------------------------------
def _check_digest(O, c, oc, fid, enc, oenc, coeffs, digest, small):
    import digest_ref as DR
    assert enc.digest == digest and (c.n_rows, c.n_per_row, c.n_cols) == (oc.n_rows, oc.n_per_row, oc.n_cols)
    assert (c.comm() == oc.comm()).all() and (c.coeffs() == oc.coeffs()).all()
    T = DR.tree_ref(digest)
    if T is None:
        want = oc.hashes()
    else:
        want = np.frombuffer(b"".join(T.tree(T.leaves(O, fid, oc.comm(), oc.n_rows, oc.n_cols))), np.uint8).reshape(-1, DR.DLEN[digest])
    got = c.hashes()
    assert got.shape == want.shape
    bad = np.nonzero((got != want).any(axis=1))[0]
    assert bad.size == 0, (digest, fid, c.n_rows, c.n_cols, bad[:8])
    assert c.get_root() == want[-1].tobytes()
    if small:
        DR.check_case(DR.RefCase(O, oenc, coeffs, digest), enc, "%s ft%d %dx%d" % (digest, fid, c.n_rows, c.n_cols), commit=c)
    return small


@pytest.mark.parametrize("seed", range(6))
def test_fuzz_ligero_digests(oracle, seed):
    import digest_ref as DR
    O = oracle
    rnd = random.Random(3000 + seed)
    n_small, seen = 0, set()
    for i in range(12):
        digest = DR.DIGEST_NAMES[(i + seed) % 3] if i < 3 else rnd.choice(DR.DIGEST_NAMES)      # every digest in every seed
        fid = rnd.choice([0, 1, 2, 3, 3])
        rho = rnd.choice([(1, 2), (1, 2), (1, 4), (3, 4), (38, 39)])
        log_n = rnd.randrange(1, 9) if i % 3 == 0 else rnd.randrange(1, 17)                     # every third case small enough to prove
        n_cols = 1 << log_n
        n_per_row = max(1, min(n_cols - 1, n_cols * rho[0] // rho[1] - rnd.choice([0, 0, 1, 3])))
        max_rows = max(1, min(48 if i % 3 == 0 else 300, (1 << (13 if i % 3 == 0 else 18)) // n_cols))
        n_rows = rnd.randrange(1, max_rows + 1)
        n = n_rows * n_per_row - rnd.randrange(0, n_per_row)
        enc = LigeroEncoding.new_from_dims(fid, n_per_row, n_cols, rho, digest=digest)
        oenc = O.Encoding.ligero_from_dims(fid, n_per_row, n_cols, rho)
        coeffs = O.random_elems(fid, n, rnd.randrange(1 << 30))
        c = LcCommit.commit(coeffs, enc)
        oc = O.Commit.commit(coeffs, oenc, n_threads=4)
        n_small += _check_digest(O, c, oc, fid, enc, oenc, coeffs, digest, small=(i % 3 == 0))
        seen.add(digest)
    assert n_small == 4 and seen == set(DR.DIGEST_NAMES)


@pytest.mark.parametrize("seed", range(3))
def test_fuzz_brakedown_digests(oracle, seed):
    import digest_ref as DR
    O = oracle
    rnd = random.Random(4000 + seed)
    seen = set()
    for i in range(6):
        digest = DR.DIGEST_NAMES[(i + seed) % 3]
        fid = rnd.choice([0, 1, 2, 3, 3])
        small = i < 3                                                                            # one proof per digest and seed
        code = 6 if small else rnd.randrange(1, 7)            # (SdigCode6: the fewest openings for the bignum prover)
        n_per_row = rnd.randrange(30, 120) if small else rnd.randrange(60, 3000)
        n_rows = rnd.choice([1, 2, 7, 23, 24, 25] if small else [1, 2, 7, 15, 16, 17, 23, 24, 25, 40, 64, 65, 90, 130])
        n = n_rows * n_per_row - rnd.randrange(0, n_per_row)
        mseed = rnd.randrange(1 << 40)
        oenc = O.Encoding.sdig_from_dims(fid, n_per_row, 0, mseed, code)
        _, _, n_cols = oenc.get_dims(n_per_row)
        enc = SdigEncoding.new_from_dims(fid, n_per_row, n_cols, mseed, code, digest=digest)
        coeffs = O.random_elems(fid, n, rnd.randrange(1 << 30))
        c = LcCommit.commit(coeffs, enc)
        oc = O.Commit.commit(coeffs, oenc, n_threads=4)
        _check_digest(O, c, oc, fid, enc, oenc, coeffs, digest, small)
        seen.add(digest)
    assert seen == set(DR.DIGEST_NAMES)

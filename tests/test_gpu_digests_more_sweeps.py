"""Keccak-256 and SHA-256 under the cross-cutting suites BLAKE2b runs in -- the counterpart, for digest_more.NEW_DIGESTS, of what
the fixed list digest_ref.DIGEST_NAMES reaches in tests/test_gpu_fuzz.py (the *_digests legs), tests/test_gpu_digests_paths.py,
tests/test_gpu_digests_edges.py (tiny shapes, refill, from_parts), tests/test_gpu_digests_verify.py (the commitment's serde on
bytes it must not trust) and tests/test_gpu_blake2b.py (rate 1/4).  Same generators, same shapes, seeds of their own; the tree
reference is digest_more.hashes_ref, proofs and verdicts come from the digest-generic reference (digest_ref.RefCase)."""
import io
import json
import os
import random
import subprocess
import sys

import numpy as np
import pytest

import digest_more as DM
import digest_ref as DR
import lcpc_amd
from common import FIRST_TWO_PASS, ntt_plan
from lcpc_amd import LcCommit, LcpcError, LigeroEncoding, SdigEncoding, Transcript

pytestmark = pytest.mark.gpu

NEW = DM.NEW_DIGESTS
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _check_digest(O, c, oc, fid, enc, oenc, coeffs, digest, small):
    assert enc.digest == digest and (c.n_rows, c.n_per_row, c.n_cols) == (oc.n_rows, oc.n_per_row, oc.n_cols)
    assert (c.comm() == oc.comm()).all() and (c.coeffs() == oc.coeffs()).all()
    want = DM.hashes_ref(digest, O, fid, oc.comm(), oc.n_rows, oc.n_cols)
    got = c.hashes()
    assert got.shape == want.shape
    bad = np.nonzero((got != want).any(axis=1))[0]
    assert bad.size == 0, (digest, fid, c.n_rows, c.n_cols, bad[:8])
    assert c.get_root() == want[-1].tobytes()
    if small:
        DR.check_case(DR.RefCase(O, oenc, coeffs, digest), enc, "%s ft%d %dx%d" % (digest, fid, c.n_rows, c.n_cols), commit=c)
    return small


# ---- tests/test_gpu_fuzz.py: the digest drawn per case ------------------------------------------------------------------------------

@pytest.mark.parametrize("seed", range(6))
def test_fuzz_ligero_digests(oracle, seed):
    O = oracle
    rnd = random.Random(5000 + seed)
    n_small, seen, rates = 0, set(), set()
    for i in range(12):
        digest = NEW[(i + seed) % 2] if i < 4 else rnd.choice(NEW)                               # both digests in every seed
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
        rates.add(rho)
    assert n_small == 4 and seen == set(NEW) and len(rates) >= 2


@pytest.mark.parametrize("seed", range(3))
def test_fuzz_brakedown_digests(oracle, seed):
    O = oracle
    rnd = random.Random(6000 + seed)
    seen = set()
    for i in range(6):
        digest = NEW[(i + seed) % 2]
        fid = rnd.choice([0, 1, 2, 3, 3])
        small = i < 2                                                                            # one proof per digest and seed
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
    assert seen == set(NEW)


# ---- tests/test_gpu_blake2b.py: rate 1/4 ------------------------------------------------------------------------------------------

@pytest.mark.parametrize("digest", NEW)
@pytest.mark.parametrize("fid,log_n", [(1, 20), (3, 18)])
def test_hashes_ligero_rate_quarter(oracle, fid, log_n, digest):
    n = 1 << log_n
    enc = LigeroEncoding.new(fid, n, rho=(1, 4), digest=digest)
    c = LcCommit.commit(DR.edge_elems(oracle, fid, n, 3), enc)
    want = DM.hashes_ref(digest, oracle, fid, c.comm(), c.n_rows, c.n_cols)
    assert np.array_equal(c.hashes(), want) and c.get_root() == want[-1].tobytes()


# ---- tests/test_gpu_digests_paths.py: behind the row-NTT switches ------------------------------------------------------------------

N_ROWS = 3
SWITCHES = {"default": {}, "general": {"LCPC_NTT_GENERAL": "1"}, "mid0": {"LCPC_NTT_MID_MAX_MB": "0"}, "mid1": {"LCPC_NTT_MID_MAX_MB": "1"}}

CHILD = r"""
import json, sys
sys.path[:0] = [%r, %r, %r]
import oracle_lib as O
import digest_ref as DR
import digest_more as DM
out = []
for fid, log_n in %r:
    n_cols = 1 << log_n
    oenc = O.Encoding.ligero_from_dims(fid, n_cols // 2, n_cols)
    coeffs = DR.edge_elems(O, fid, %d * (n_cols // 2) - 5, 40 + fid)
    for digest in DM.NEW_DIGESTS:
        enc = DR.make_enc("ligero", fid, 0, digest, dims=(n_cols // 2, n_cols))
        rc = DR.RefCase(O, oenc, coeffs, digest)
        DR.check_case(rc, enc, "%%s ft%%d 2^%%d" %% (digest, fid, log_n))
        out.append([fid, digest])
print("DONE " + json.dumps(out))
"""


def plan_facts(fid, name):
    log_n = FIRST_TWO_PASS[fid]
    general = name == "general"
    mid_mb = {"mid0": 0, "mid1": 1}.get(name)
    plan = ntt_plan(fid, log_n, general, mid_mb, N_ROWS)
    return DR.leaf_canon_in(fid, "ligero", log_n, N_ROWS, general), bool(plan[0]["mid"]), plan[0]["kernel"]


@pytest.mark.parametrize("name", list(SWITCHES))
def test_digests_behind_ntt_switches(name):
    """one Ligero shape per field under each switch, both digests, in a fresh child process with a time limit: under
    LCPC_NTT_GENERAL comm stays in Montgomery form for Ft63 / Ft127 / Ft191, the only way Ligero runs the <NL, false> leaf kernels"""
    shapes = [(fid, FIRST_TWO_PASS[fid]) for fid in range(4)]
    env = {k: v for k, v in os.environ.items() if k not in ("LCPC_NTT_GENERAL", "LCPC_NTT_MID_MAX_MB")}
    env.update(SWITCHES[name])
    code = CHILD % (ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "oracle"), shapes, N_ROWS)
    r = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    done = json.loads(r.stdout.split("DONE ", 1)[1])
    assert sorted(map(tuple, done)) == sorted((fid, d) for fid in range(4) for d in NEW)
    for fid in range(4):
        canon, mid, kernel = plan_facts(fid, name)
        assert kernel == ("general" if name == "general" else "K1s" if fid == 3 else "K1n")
        assert canon == (fid == 3 or name != "general")


def test_switch_matrix_reaches_both_leaf_instantiations():
    reach = {(fid, plan_facts(fid, name)[0]) for fid in range(4) for name in SWITCHES}
    assert reach == {(0, True), (0, False), (1, True), (1, False), (2, True), (2, False), (3, True)}


# ---- tests/test_gpu_digests_edges.py: tiny shapes, refill, from_parts --------------------------------------------------------------

@pytest.mark.parametrize("digest", NEW)
@pytest.mark.parametrize("fid", [0, 1, 2, 3])
@pytest.mark.parametrize("n_per_row,n_cols", [(1, 2), (1, 4), (3, 4), (7, 8), (2, 16)])
def test_tiny_shapes(oracle, fid, n_per_row, n_cols, digest):
    O = oracle
    oenc = O.Encoding.ligero_from_dims(fid, n_per_row, n_cols)
    enc = DR.make_enc("ligero", fid, 0, digest, dims=(n_per_row, n_cols))
    for n in (1, n_per_row, n_per_row + 1, 5 * n_per_row - (1 if n_per_row > 1 else 0)):
        rc = DR.RefCase(O, oenc, O.random_elems(fid, n, n + n_cols), digest)
        DR.check_case(rc, enc, "%s ft%d %dx%d n %d" % (digest, fid, n_per_row, n_cols, n))


# n_rows of the refills: more rows, then fewer, through every padding case the field reaches (SHA-256 residue (4 + L n_rows) mod 8:
# 7 = one more block, 0 = a block of padding alone, 6 / others = the same block; Keccak-256 (4 + L n_rows) mod 17: 0 and 16)
REFILL_ROWS = {0: (5, 33, 3, 4, 2, 12, 13, 1), 1: (5, 33, 2, 1, 15, 6, 1), 2: (5, 33, 1, 4, 6, 10, 1), 3: (5, 33, 1, 16, 3, 2, 1)}


@pytest.mark.parametrize("digest", NEW)
@pytest.mark.parametrize("fid", [0, 1, 2, 3])
def test_refill_with_other_row_counts(oracle, fid, digest):
    """one LcCommit refilled under one encoder with other row counts: a stale leaf slot, tree level or padding block would show"""
    O, L = oracle, DR.LIMBS[fid]
    n_per_row, n_cols = 96, 256
    oenc = O.Encoding.ligero_from_dims(fid, n_per_row, n_cols)
    enc = DR.make_enc("ligero", fid, 0, digest, dims=(n_per_row, n_cols))
    c = LcCommit(enc)
    res = set()
    for n_rows in REFILL_ROWS[fid]:
        rc = DR.RefCase(O, oenc, DR.edge_elems(O, fid, n_rows * n_per_row - 1, 300 + n_rows), digest)
        LcCommit.commit(rc.coeffs, enc, into=c)
        assert c.n_rows == n_rows and np.array_equal(c.hashes(), rc.hashes()) and c.get_root() == rc.root
        pf = c.prove(rc.outer, enc, DR.mk_tr(Transcript, rc.root, rc.nco)).to_bytes()
        assert pf == rc.proof
        res.add(DM.sha256_residue(L, n_rows) if digest == "sha256" else DR.sha3_residue(L, n_rows))
    if digest == "sha256":
        assert res >= {1: {0, 6, 7}, 2: {0, 6}, 3: {0, 6, 7}, 4: {0}}[L]
    else:
        assert res >= {0, 16}


@pytest.mark.parametrize("digest", NEW)
@pytest.mark.parametrize("fid", [1, 2, 3])
def test_from_parts_n_cols_not_a_multiple_of_64(oracle, fid, digest):
    O, n_per_row, n_rows = oracle, 40, 6
    oenc = O.Encoding.sdig_from_dims(fid, n_per_row, 0, 3, DR.SDIG_CODE)
    _, _, n_cols = oenc.get_dims(n_per_row)
    assert n_cols % 64
    enc = SdigEncoding.new_from_dims(fid, n_per_row, n_cols, 3, DR.SDIG_CODE, digest=digest)
    rc = DR.RefCase(O, oenc, DR.edge_elems(O, fid, n_rows * n_per_row, 7), digest)
    c = LcCommit.from_parts(enc, rc.oc.comm(), rc.oc.coeffs(), n_rows)
    assert np.array_equal(c.hashes(), rc.hashes()) and c.get_root() == rc.root
    pf = c.prove(rc.outer, enc, DR.mk_tr(Transcript, rc.root, rc.nco)).to_bytes()
    assert pf == rc.proof


# ---- tests/test_gpu_digests_verify.py: the commitment's serde on bytes it must not trust -------------------------------------------

@pytest.mark.parametrize("digest", NEW)
def test_commit_bincode_bad_streams_and_sweep(oracle, digest):
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

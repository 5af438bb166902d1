"""What the digest-generic tests share (tests/test_oracle_digests.py on the CPU, tests/test_gpu_digests_*.py on the MI355X): the
reference of LcCommit<D, E> for D = BLAKE3, SHA3-256 and BLAKE2b-512 -- oracle/pyref.py with its digest parameter, fed with the C
oracle's encoded rows so that it stays fast at a few thousand coefficients -- the list of mutated proofs every verifier sweep
uses, and the block-edge arithmetic of the two new leaf messages."""
import random
import struct

import numpy as np

import pyref as P
from common import mk_transcript

DIGEST_NAMES = ["blake3", "sha3_256", "blake2b"]
DLEN = {"blake3": 32, "sha3_256": 32, "blake2b": 64}
LIMBS = {0: 1, 1: 2, 2: 3, 3: 4}
# VerifierError (lcpc-2d/src/lib.rs:139-166) -> lcpc_status (include/lcpc_hip.h), "Malformed" = bytes bincode refuses
VERR = {"NumColOpens": -32, "ColumnPath": -33, "ColumnEval": -34, "ColumnDegree": -35, "OuterTensor": -36, "InnerTensor": -37,
        "EncodingDims": -38, "Encode": -39, "Malformed": -40}


def ref_digest(name, O=None):
    """pyref's D.  With the C oracle at hand BLAKE3 runs on its lo_blake3 (pinned to the same upstream vectors as pyref.blake3 in
    tests/test_oracle_kats.py): the pure-Python compression is the one slow part of a BLAKE3 tree."""
    if name == "blake3" and O is not None:
        return P.Digest("blake3", 32, O.blake3)
    return P.DIGESTS[name]


def tree_ref(name):
    """the second, independent statement of the tree: tests/sha3_ref.py / tests/blake2b_ref.py (None for BLAKE3: the C oracle)"""
    if name == "sha3_256":
        import sha3_ref
        return sha3_ref
    if name == "blake2b":
        import blake2b_ref
        return blake2b_ref
    return None


def edge_elems(O, fid, n, seed):
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


# ---- the reference over the C oracle's encoder ---------------------------------------------------------------------------------

class OracleEnc:
    """pyref's encoder interface (LcEncoding, lcpc-2d/src/lib.rs:74-104) on the C oracle's encoder: the code is the same for every
    digest and is pinned against pyref's own in tests/test_oracle_vs_pyref.py; what differs per digest is hashed by pyref."""
    LABEL_DT, LABEL_PR, LABEL_PE, LABEL_CO = b"$l//DT", b"$l//PR", b"$l//PE", b"$l//CO"

    def __init__(self, O, oenc):
        self.O, self.oenc, self.fid = O, oenc, oenc.fid
        _, self.n_per_row, self.n_cols = oenc.get_dims(1)

    def get_dims(self, length):
        return self.oenc.get_dims(length)

    def dims_ok(self, n_per_row, n_cols):
        return self.oenc.dims_ok(n_per_row, n_cols)

    def get_n_col_opens(self):
        return self.oenc.get_n_col_opens()

    def get_n_degree_tests(self):
        return self.oenc.get_n_degree_tests()

    def encode(self, row):
        return self.O.to_canon_ints(self.fid, self.oenc.encode(self.O.to_mont(self.fid, row)))


def pyref_commit(O, fid, oc, digest):
    """pyref's LcCommit<D, E> of an oracle commitment: its comm and coeffs as canonical ints, merkleized by pyref under D"""
    F = P.FIELDS[fid]
    c = P.LcCommit(O.to_canon_ints(fid, oc.comm()), O.to_canon_ints(fid, oc.coeffs()), oc.n_rows, oc.n_cols, oc.n_per_row, None)
    P.merkleize(F, c, digest)
    return c


mk_tr = mk_transcript


class RefCase:
    """one commitment under one digest, proved by the reference: .coeffs (Montgomery limbs), .oenc / .oc (C oracle, BLAKE3), .enc
    (OracleEnc), .c (pyref commitment under D; the transcript is the C oracle's merlin, pinned with pyref's to the same vectors in
    tests/test_oracle_kats.py -- neither depends on D), .root, .outer / .inner (limbs) with .outer_i / .inner_i (ints), .proof (the
    reference prover's bincode bytes), .cols (the opened columns), .eval (int)"""

    def __init__(self, O, oenc, coeffs, digest_name, x=0x1234567):
        fid = oenc.fid
        self.O, self.fid, self.F, self.L = O, fid, P.FIELDS[fid], LIMBS[fid]
        self.name, self.D, self.dl = digest_name, ref_digest(digest_name, O), DLEN[digest_name]
        self.coeffs, self.oenc = coeffs, oenc
        self.oc = O.Commit.commit(coeffs, oenc, n_threads=4)
        self.enc = OracleEnc(O, oenc)
        self.c = pyref_commit(O, fid, self.oc, self.D)
        self.n_rows, self.n_per_row, self.n_cols = self.oc.n_rows, self.oc.n_per_row, self.oc.n_cols
        self.root, self.nco = self.c.get_root(), oenc.get_n_col_opens()
        p = self.F.p
        x %= p
        self.inner_i = [pow(x, i, p) for i in range(self.n_per_row)]
        xr = pow(x, self.n_per_row, p)
        self.outer_i = [pow(xr, i, p) for i in range(self.n_rows)]
        self.inner, self.outer = O.to_mont(fid, self.inner_i), O.to_mont(fid, self.outer_i)
        pf, self.cols = P.prove(self.F, self.c, self.outer_i, self.enc, mk_tr(O.Transcript, self.root, self.nco))
        self.proof = P.ser_proof(self.F, pf)
        self.eval = sum(a * b for a, b in zip(self.inner_i, pf.p_eval)) % p

    def hashes(self):
        return np.frombuffer(b"".join(self.c.hashes), np.uint8).reshape(-1, self.dl)

    def verdict(self, blob, root=None, digest=None):
        """the reference's answer to these bytes: the evaluation (int) or the error's name"""
        root = self.root if root is None else root     # (the transcript is the prover's whatever root the verifier is handed)
        return P.verify_bytes(self.F, digest or self.D, root, self.outer_i, self.inner_i, blob, self.enc,
                              mk_tr(self.O.Transcript, self.root, self.nco))

    def eval_limbs(self):
        return self.O.to_mont(self.fid, [self.eval])[0]


SDIG_CODE = 6      # SdigCode6: the fewest column openings of the six codes (3755), which is what a bignum verifier pays for


def make_oenc(O, kind, fid, n, seed=1, dims=None):
    """("ligero", n) / ("sdig", n, seed) as the encoder constructors pick the shape, or ("ligero", dims=(n_per_row, n_cols))"""
    if dims is not None:
        return O.Encoding.ligero_from_dims(fid, dims[0], dims[1])
    return O.Encoding.ligero(fid, n) if kind == "ligero" else O.Encoding.sdig(fid, n, seed, SDIG_CODE)


def make_enc(kind, fid, n, digest, seed=1, dims=None):
    """the library's encoder of the same shape (GPU tests only)"""
    from lcpc_amd import LigeroEncoding, SdigEncoding
    if dims is not None:
        return LigeroEncoding.new_from_dims(fid, dims[0], dims[1], digest=digest)
    return LigeroEncoding.new(fid, n, digest=digest) if kind == "ligero" else SdigEncoding.new(fid, n, seed, SDIG_CODE, digest=digest)


# ---- mutated proofs ------------------------------------------------------------------------------------------------------------

# the shapes of the verifier sweep under every digest: (kind, fid, n_coeffs, dims); the last is n_cols = 2 (path_len = 1), 3 rows
SWEEP_SHAPES = [("ligero", 3, 1 << 12, None), ("ligero", 2, 1 << 11, None), ("sdig", 1, 1 << 9, None), ("ligero", 0, 3, (1, 2))]
SWEEP_IDS = ["ligero-ft255", "ligero-ft191", "sdig-ft127", "ligero-ft63-2cols"]


def check_case(rc, enc, label, commit=None):
    """the library (GPU tests only) against the reference case rc: commit (or the commitment handed in), the whole `hashes`
    array, proof bytes == the reference prover's, verify accepts with the reference's evaluation"""
    from lcpc_amd import LcCommit, LcEvalProof, Transcript
    c = LcCommit.commit(rc.coeffs, enc) if commit is None else commit
    assert (c.n_rows, c.n_per_row, c.n_cols) == (rc.n_rows, rc.n_per_row, rc.n_cols), label
    assert np.array_equal(c.comm(), rc.oc.comm()), label
    got, want = c.hashes(), rc.hashes()
    assert got.shape == want.shape, label
    bad = np.nonzero((got != want).any(axis=1))[0]
    assert bad.size == 0, "%s: hash slots differ from the reference: %s" % (label, bad[:8])
    assert c.get_root() == rc.root, label
    pf = c.prove(rc.outer, enc, mk_tr(Transcript, rc.root, rc.nco)).to_bytes()
    assert pf == rc.proof, label
    ev = LcEvalProof.from_bytes(pf, enc.L).verify(rc.root, rc.outer, rc.inner, enc, mk_tr(Transcript, rc.root, rc.nco))
    assert np.array_equal(ev, rc.eval_limbs()), label
    assert rc.verdict(pf) == rc.eval, label
    return c



def proof_layout(pf, L, n_per_row, n_rows, n_cols, dl):
    """offsets into a bincode proof (lib.rs:550-609): n_cols, len, p_eval, n_deg, (len, p_random)*, n_columns,
    (len, col, path_len, (dl, digest)*)*"""
    F = 8 * L
    o = dict(F=F, eval=16, nd=16 + n_per_row * F)
    o["n_deg"] = struct.unpack_from("<Q", pf, o["nd"])[0]
    o["rand"] = o["nd"] + 16
    o["ncol"] = o["nd"] + 8 + o["n_deg"] * (8 + n_per_row * F)
    o["col0"] = o["ncol"] + 8
    o["path_len"] = max(0, (n_cols - 1).bit_length())
    o["col_bytes"] = 8 + n_rows * F + 8 + o["path_len"] * (8 + dl)
    o["plen0"] = o["col0"] + 8 + n_rows * F
    o["dig0"] = o["plen0"] + 16
    return o


def mutation_cases(pf, L, n_per_row, n_rows, seed, dl=32, n_cols=None):
    """(name, bytes) of the mutated proofs of one valid proof `pf`: two bit flips at every field of the wire layout, 24 anywhere,
    truncations, and a limb vector >= p in p_eval.  With dl = 32 this is the list tests/test_gpu_verify_mutations.py has always
    drawn (same generator, same order of draws)."""
    o = proof_layout(pf, L, n_per_row, n_rows, n_cols or 2, dl)
    F = o["F"]
    rnd = random.Random(seed)
    spots = {
        "n_cols": 0, "p_eval len": 8, "p_eval": o["eval"] + rnd.randrange(n_per_row * F), "n_deg": o["nd"],
        "p_random len": o["nd"] + 8, "p_random": o["rand"] + rnd.randrange(n_per_row * F), "n_columns": o["ncol"],
        "col0 len": o["col0"], "col0 value": o["col0"] + 8 + rnd.randrange(n_rows * F),
        "col0 path len": o["plen0"], "col0 digest len": o["plen0"] + 8,
        "col0 digest": o["dig0"] + rnd.randrange(dl), "last byte": len(pf) - 1,
    }
    cases = []
    for name, pos in spots.items():
        for bit in (0, rnd.randrange(8)):
            b = bytearray(pf)
            b[pos] ^= 1 << bit
            cases.append((name + " bit %d" % bit, bytes(b)))
    for _ in range(24):                                   # anywhere
        b = bytearray(pf)
        pos = rnd.randrange(len(pf))
        b[pos] ^= 1 << rnd.randrange(8)
        cases.append(("byte %d" % pos, bytes(b)))
    cases += [("truncated", pf[:-1]), ("truncated 8", pf[:-8]), ("half", pf[:len(pf) // 2]), ("header only", pf[:16]), ("empty", b"")]
    # a limb vector >= p in p_eval: all ones in the top limb of element 0
    b = bytearray(pf)
    b[o["eval"] + F - 8:o["eval"] + F] = b"\xff" * 8
    cases.append(("p_eval[0] >= p", bytes(b)))
    return cases


def digest_cases(pf, L, n_per_row, n_rows, n_cols, dl, n_open):
    """the mutations that depend on the digest's size: a flip in the second half of a path entry (bytes 32.. of a 64-byte one), a
    path entry announced with the other digests' length, one path entry more or fewer, a flip in the last entry of the last
    column, and two columns' values exchanged"""
    o = proof_layout(pf, L, n_per_row, n_rows, n_cols, dl)
    F = o["F"]
    cases = []

    def put(name, pos, data):
        b = bytearray(pf)
        b[pos:pos + len(data)] = data
        cases.append((name, bytes(b)))

    def flip(name, pos, mask):
        put(name, pos, bytes([pf[pos] ^ mask]))

    flip("col0 digest second half", o["dig0"] + dl // 2 + dl // 4 + 1, 0x10)
    flip("col0 digest last byte", o["dig0"] + dl - 1, 0x80)
    flip("last column last digest byte %d" % (dl // 2), len(pf) - dl // 2, 0x01)
    put("col0 entry length %d" % (96 - dl), o["plen0"] + 8, struct.pack("<Q", 96 - dl))
    last = o["plen0"] + 8 + (o["path_len"] - 1) * (8 + dl)
    put("col0 last entry length %d" % (96 - dl), last, struct.pack("<Q", 96 - dl))
    put("col0 path_len + 1", o["plen0"], struct.pack("<Q", o["path_len"] + 1))
    put("col0 path_len - 1", o["plen0"], struct.pack("<Q", o["path_len"] - 1))
    v0 = pf[o["col0"] + 8:o["col0"] + 8 + n_rows * F]
    for k in range(1, n_open):                           # the first column that holds other values (the draw may repeat a column)
        q = o["col0"] + k * o["col_bytes"] + 8
        vk = pf[q:q + n_rows * F]
        if vk != v0:
            b = bytearray(pf)
            b[o["col0"] + 8:o["col0"] + 8 + n_rows * F] = vk
            b[q:q + n_rows * F] = v0
            cases.append(("columns 0 and %d exchange their values" % k, bytes(b)))
            break
    return cases                                         # (n_cols = 2 at rate 1/2: both columns hold the row's one coefficient)


def count_unreduced(F, cases, dl):
    """how many of the blobs parse and hold a limb vector >= p: the cases where the library is stricter than the reference by
    design (VERR_MALFORMED) -- decided from the bytes alone"""
    n = 0
    for _, blob in cases:
        try:
            n += P.deser_proof(F, blob, dl).n_unreduced > 0
        except (P.MalformedProof, P.VerifierError):
            pass
    return n


# ---- block edges of the leaf messages ------------------------------------------------------------------------------------------

def sha3_residue(L, n_rows):
    """64-bit words of the SHA3-256 leaf message (4 + L n_rows) left in the last 17-word block: 0 = a whole padding block, 16 = one
    word left, 0x06 and 0x80 in the same word"""
    return (4 + L * n_rows) % 17


def blake2b_residue(L, n_rows):
    """words of the BLAKE2b leaf message (8 + L n_rows) in the last 16-word block: 0 = exactly full, no extra block"""
    return (8 + L * n_rows) % 16


SHA3_RESIDUES = (0, 1, 8, 15, 16)       # 8: a mid value
BLAKE2B_RESIDUES = (0, 1, 15)


def edge_rows(fid, lo=1, hi=70):
    """{(digest, residue): n_rows}: for every residue the block-edge test claims, the smallest n_rows in [lo, hi] that reaches it
    (None where the field cannot: L n_rows is a multiple of L, so an even L never gives an odd BLAKE2b residue, and L = 4 only
    residues = 0 mod 4)"""
    L = LIMBS[fid]
    out = {}
    for name, fn, wanted in (("sha3_256", sha3_residue, SHA3_RESIDUES), ("blake2b", blake2b_residue, BLAKE2B_RESIDUES)):
        for res in wanted:
            out[(name, res)] = next((r for r in range(lo, hi + 1) if fn(L, r) == res), None)
    return out


def leaf_canon_in(fid, kind, log_n_cols, n_rows, general=False):
    """which <NL, CANON> instantiation of the leaf kernels a commit runs (lcpc_amd/csrc/commit.cpp LeafArgs::canon_in): Brakedown
    hashes canonical values from 24 rows on (the position-major commitment) and Montgomery form below; a Ligero context keeps comm
    canonical for Ft255 always, and for the other fields when it runs the limb plan (K1n: two or three passes, not under
    LCPC_NTT_GENERAL) -- the plan as tests/common.py restates it"""
    from common import ntt_plan
    if kind == "sdig":
        return n_rows >= 24
    return fid == 3 or ntt_plan(fid, log_n_cols, general)[0]["kernel"] != "general"

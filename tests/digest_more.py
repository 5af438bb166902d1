"""Keccak-256 and SHA-256 for the digest-generic tests: the two references as pyref.Digest objects in this module's own DIGESTS
table.  When this module is imported, digest_ref.ref_digest learns to look the two names up here and digest_ref.DLEN their
length, so that digest_ref.RefCase / check_case / mutation_cases / digest_cases serve them unchanged.  pyref.DIGESTS itself is
NOT touched: tests/golden/make_golden.py iterates it and tests/test_oracle_digests.py regenerates the committed fixtures from
it in the same session (digest_ref.DIGEST_NAMES is a fixed list too: the existing parametrised tests do not grow).

  * SHA-256: hashlib.sha256.
  * Keccak-256 = Keccak[512](M || 01, 256): hashlib has SHA3-256 only (padding byte 0x06), so the sponge is written here on
    pyref's Keccak-f[1600] (keccak256).  It is pinned by the two published vectors below and by differing from SHA3-256.  Pure
    Python costs about 0.2 ms per permutation, so the registered digest runs the same sponge on the C oracle's lo_keccak_f1600 when
    that library is at hand (as digest_ref.ref_digest does for BLAKE3); tests/test_host_digests_more.py holds the two and the
    batched numpy form (keccak256_many: one sponge per row of an array, for whole trees at 2^24) to each other.

The block-edge arithmetic of the two leaf messages is at the end."""
import functools
import hashlib

import numpy as np

import digest_ref as DR
import pyref as P

NEW_DIGESTS = ["keccak256", "sha256"]
RATE = 136
KAT = {b"": "c5d2460186f7233c927e7db2dcc703c0e500b653ca82273b7bfad8045d85a470",
       b"abc": "4e03657aea45a94fc7d47ba826c8d667c0d1e6e33a64a036ec44f58fa12d6c45"}


def _sponge(data, perm, dom):
    data = bytes(data)
    p = bytearray(data) + bytearray(RATE - len(data) % RATE)
    p[len(data)] ^= dom
    p[-1] ^= 0x80
    st = bytearray(200)
    for o in range(0, len(p), RATE):
        blk = int.from_bytes(p[o:o + RATE], "little") ^ int.from_bytes(st[:RATE], "little")
        st[:RATE] = blk.to_bytes(RATE, "little")
        st = perm(st)
    return bytes(st[:32])


def keccak256(data):
    """Keccak[512](M || 01, 256) on pyref's Keccak-f: the reference"""
    return _sponge(data, P.keccak_f1600, 0x01)


def sha3_256_sponge(data):
    """the same sponge with FIPS 202's domain byte: must be hashlib.sha3_256 (checks the sponge itself against a library)"""
    return _sponge(data, P.keccak_f1600, 0x06)


def _oracle_perm():
    import ctypes

    import oracle_lib as O
    f = O.lib().lo_keccak_f1600

    def perm(st):
        buf = (ctypes.c_uint8 * 200).from_buffer(st)
        f(ctypes.cast(buf, ctypes.c_void_p))
        return st
    return perm


@functools.lru_cache(maxsize=1 << 17)
def keccak256_fast(data):
    """keccak256 with the permutation in the C oracle (pinned to pyref's in tests/test_host_digests_more.py); memoised: a
    mutation sweep folds the same paths for every blob"""
    global _PERM
    if _PERM is None:
        _PERM = _oracle_perm()
    return _sponge(data, _PERM, 0x01)


_PERM = None

_ROT = np.array([[0, 36, 3, 41, 18], [1, 44, 10, 45, 2], [62, 6, 43, 15, 61], [28, 55, 25, 21, 56], [27, 20, 39, 8, 14]])


def _rol(x, n):
    n = int(n) % 64
    return x if n == 0 else (x << np.uint64(n)) | (x >> np.uint64(64 - n))


def _keccak_f_many(A):
    """Keccak-f[1600] on every row of A[n][25] (uint64, lane (x, y) at x + 5 y), in place"""
    for rc in P._KRC:
        C = [A[:, x] ^ A[:, x + 5] ^ A[:, x + 10] ^ A[:, x + 15] ^ A[:, x + 20] for x in range(5)]
        D = [C[(x - 1) % 5] ^ _rol(C[(x + 1) % 5], 1) for x in range(5)]
        B = [None] * 25
        for x in range(5):
            for y in range(5):
                B[y + 5 * ((2 * x + 3 * y) % 5)] = _rol(A[:, x + 5 * y] ^ D[x], _ROT[x][y])
        for y in range(5):
            for x in range(5):
                A[:, x + 5 * y] = B[x + 5 * y] ^ (~B[(x + 1) % 5 + 5 * y] & B[(x + 2) % 5 + 5 * y])
        A[:, 0] ^= np.uint64(rc)
    return A


def keccak256_many(msgs):
    """Keccak-256 of every row of msgs[n][length] (uint8, one length): [n][32] uint8.  Many rows go to a few threads in slices
    (numpy releases the interpreter lock inside its loops)."""
    msgs = np.ascontiguousarray(msgs, np.uint8)
    n, ln = msgs.shape
    if n > 8192:
        from concurrent.futures import ThreadPoolExecutor
        step = max(4096, (n + 15) // 16)
        with ThreadPoolExecutor(8) as ex:
            return np.concatenate(list(ex.map(keccak256_many, [msgs[i:i + step] for i in range(0, n, step)])))
    total = (ln // RATE + 1) * RATE
    p = np.zeros((n, total), np.uint8)
    p[:, :ln] = msgs
    p[:, ln] ^= 0x01
    p[:, -1] ^= 0x80
    lanes = p.view("<u8").reshape(n, total // RATE, 17)
    A = np.zeros((n, 25), np.uint64)
    for b in range(total // RATE):
        A[:, :17] ^= lanes[:, b]
        _keccak_f_many(A)
    return np.ascontiguousarray(A[:, :4]).view(np.uint8).reshape(n, 32)


def sha256(data):
    return hashlib.sha256(bytes(data)).digest()


DIGESTS = {}
_ref_digest_before = DR.ref_digest


def _ref_digest(name, O=None):
    return DIGESTS[name] if name in DIGESTS else _ref_digest_before(name, O)


def register(fast=True):
    """DIGESTS holds the two references; digest_ref.ref_digest / digest_ref.DLEN learn the two names (both are only ever indexed
    by name)"""
    DIGESTS["sha256"] = P.Digest("sha256", 32, sha256)
    fn = keccak256
    if fast:
        keccak256_fast(b"")    # (loads, and if need be builds, the C oracle: a failure there is an error, not a reason to go slow)
        fn = keccak256_fast
    DIGESTS["keccak256"] = P.Digest("keccak256", 32, fn)
    DR.DLEN.update(keccak256=32, sha256=32)
    DR.ref_digest = _ref_digest


register()


# ---- whole trees in bulk -------------------------------------------------------------------------------------------------------

def many(name, msgs):
    """D of every row of msgs[n][length] -> [n][32] uint8"""
    msgs = np.ascontiguousarray(msgs, np.uint8)
    if name == "keccak256":
        return keccak256_many(msgs)
    return np.frombuffer(b"".join(hashlib.sha256(r.tobytes()).digest() for r in msgs), np.uint8).reshape(len(msgs), 32)


def hashes_ref(name, oracle, fid, comm, n_rows, n_cols):
    """the flat `hashes` array [2 np2 - 1][32] of a row-major comm (n_rows * n_cols, L) in Montgomery form"""
    import sha3_ref
    rep = sha3_ref.repr_bytes(oracle, fid, comm).reshape(n_rows, n_cols, -1).transpose(1, 0, 2).reshape(n_cols, -1)
    msgs = np.zeros((n_cols, 32 + rep.shape[1]), np.uint8)
    msgs[:, 32:] = rep
    np2 = 1
    while np2 < n_cols:
        np2 *= 2
    level = np.zeros((np2, 32), np.uint8)
    level[:n_cols] = many(name, msgs)
    out = [level]
    while len(level) > 1:
        level = many(name, level.reshape(len(level) // 2, 64))
        out.append(level)
    return np.concatenate(out)


def fold(name, leaf, col, sibs):
    """verify_column_path (lib.rs:955-982) under D"""
    D = DIGESTS[name]
    h = leaf
    for s in sibs:
        h = D(h + s) if col % 2 == 0 else D(s + h)
        col //= 2
    return h


# ---- block edges of the two leaf messages --------------------------------------------------------------------------------------

def sha256_residue(L, n_rows):
    """64-bit words of the SHA-256 leaf message (4 + L n_rows) in the block that holds its end: 0 = a block of padding alone,
    7 = 0x80 in the last word and the length in one more block, 6 = 0x80 and the length side by side"""
    return (4 + L * n_rows) % 8


SHA256_RESIDUES = (0, 1, 6, 7)


def edge_rows(fid, lo=1, hi=70):
    """{(digest, residue): n_rows}: the smallest n_rows in [lo, hi] that reaches each residue the block-edge tests claim, None where
    the field cannot (4 + L n_rows mod 8: L = 2 reaches even residues only, L = 4 only 0 and 4).  Keccak-256 has SHA3-256's
    message and rate, so its residues are digest_ref.SHA3_RESIDUES."""
    L = DR.LIMBS[fid]
    out = {}
    for name, fn, wanted in (("sha256", sha256_residue, SHA256_RESIDUES), ("keccak256", DR.sha3_residue, DR.SHA3_RESIDUES)):
        for res in wanted:
            out[(name, res)] = next((r for r in range(lo, hi + 1) if fn(L, r) == res), None)
    return out

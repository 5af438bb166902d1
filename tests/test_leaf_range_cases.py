"""The references and the case tables of tests/test_gpu_leaf_range.py -- the resumable column hash of SHA3-256 / Keccak-256 / SHA-256 /
BLAKE2b (launch_*_leaves_range of lcpc_amd/csrc/kernels.h) called directly through tests/lr_harness.py -- with the checks that need no
GPU: that the row counts reach every block-edge residue the one-shot digest suites name, that the batched Keccak-256 reference is the
sponge of tests/digest_more.py, that the harness is a library of its own and refuses every bad index before it touches the device.  No
GPU is needed, but the built tree is.

The leaf message of a column is P zero bytes (32; BLAKE2b: 64) and then every row's element as its canonical value in 8 L little-endian
bytes.  The reference of every digest is hashlib (Keccak-256: the sponge of digest_more on the same bytes), never a kernel."""
import functools
import hashlib
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
import common as CM  # noqa: E402
import digest_more as DM  # noqa: E402
import digest_ref as DR  # noqa: E402
import lr_harness as H  # noqa: E402
import test_k3_cases as K  # noqa: E402

DIGESTS = ("sha3_256", "keccak256", "sha256", "blake2b")
FIDS = (0, 1, 2, 3)
N_COLS = (1, 255, 256, 257)          # one partial workgroup, one short of full, full, full plus one lane
MAX_COLS = max(N_COLS)
GROUP = {"sha3_256": 17, "keccak256": 17, "sha256": 8, "blake2b": 16}      # rows after which the word -> (row, limb) map repeats
SENTINEL = 0xA5C3F00D
GUARD = 64                             # sentinel words on either side of the state and of the digests


def max_rows(digest):
    """three groups and two rows of a fourth"""
    return 3 * GROUP[digest] + 2


def n_blocks(digest, fid, n_rows):
    """blocks of the leaf message with its padding (sha3.hip, sha256.hip, blake2b.hip restated)"""
    P, W = H.SHAPE[digest][:2]
    w = P + CM.FIELD_L[fid] * n_rows
    if digest == "blake2b":
        return (w + 15) // 16
    if digest == "sha256":
        return w // 8 + 1 + (1 if w % 8 == 7 else 0)
    return w // 17 + 1


def last_row_of(digest, fid, n_rows, blk_end):
    """the last row that blocks [0, blk_end) hold a byte of (None: the zero prefix only)"""
    P, W = H.SHAPE[digest][:2]
    if W * blk_end <= P:
        return None
    return min(n_rows - 1, (W * blk_end - P - 1) // CM.FIELD_L[fid])


def blocks_ready(digest, fid, n_rows, r1):
    """commit.cpp's rule: the blocks all of whose rows are < r1"""
    P, W = H.SHAPE[digest][:2]
    return n_blocks(digest, fid, n_rows) if r1 >= n_rows else min(n_blocks(digest, fid, n_rows), (P + CM.FIELD_L[fid] * r1) // W)


@functools.lru_cache(maxsize=None)
def case_index(fid, n_rows):
    """pool indices (n_rows, MAX_COLS) of tests/test_k3_cases.py's operand pool; a launch of n_cols columns reads the first n_cols"""
    return K.case_index(fid, n_rows, MAX_COLS, 7)


def messages(digest, fid, n_rows):
    """(MAX_COLS, P + 8 L n_rows) uint8: every column's leaf message"""
    idx = case_index(fid, n_rows)
    P = 8 * H.SHAPE[digest][0]
    body = np.ascontiguousarray(K.pool(fid)[0][idx].transpose(1, 0, 2)).reshape(MAX_COLS, -1)
    out = np.zeros((MAX_COLS, P + body.shape[1] * 4), np.uint8)
    out[:, P:] = body.view(np.uint8)
    return out


def comm_of(fid, n_rows, n_cols, canon):
    """row-major comm (n_rows, n_cols, L) uint64: canonical values, or the stored (Montgomery) form"""
    return np.ascontiguousarray(K.pool(fid)[2 if canon else 1][case_index(fid, n_rows)[:, :n_cols]])


def keccak256_ragged(msgs):
    """Keccak-256 of a list of (n_i, len_i) uint8 arrays -> list of (n_i, 32): digest_more's batched permutation with every message of
    every length in one sponge, lanes sorted by block count so that block b runs on a prefix of them"""
    RATE = DM.RATE
    nb = [m.shape[1] // RATE + 1 for m in msgs]
    order = sorted(range(len(msgs)), key=lambda i: -nb[i])
    total = sum(m.shape[0] for m in msgs)
    lanes = np.zeros((total, max(nb), 17), np.uint64)
    count = np.zeros(max(nb) + 1, np.int64)          # count[b]: lanes with more than b blocks
    at, where = 0, {}
    for i in order:
        m = msgs[i]
        p = np.zeros((m.shape[0], nb[i] * RATE), np.uint8)
        p[:, :m.shape[1]] = m
        p[:, m.shape[1]] ^= 0x01
        p[:, -1] ^= 0x80
        lanes[at:at + m.shape[0], :nb[i]] = p.view("<u8").reshape(m.shape[0], nb[i], 17)
        where[i] = (at, at + m.shape[0])
        at += m.shape[0]
        count[:nb[i]] = at
    A = np.zeros((total, 25), np.uint64)
    for b in range(max(nb)):
        v = A[:count[b]]
        v[:, :17] ^= lanes[:count[b], b]
        DM._keccak_f_many(v)
    dig = np.ascontiguousarray(A[:, :4]).view(np.uint8).reshape(total, 32)
    return [dig[where[i][0]:where[i][1]] for i in range(len(msgs))]


def _hashlib_many(fn, msgs):
    return np.frombuffer(b"".join(fn(r.tobytes()).digest() for r in msgs), np.uint8).reshape(len(msgs), -1)


@functools.lru_cache(maxsize=None)
def ref_digests(digest, fid):
    """{n_rows: (MAX_COLS, digest words) uint32} for n_rows = 1 .. max_rows(digest): computed once, never written to"""
    rows = range(1, max_rows(digest) + 1)
    msgs = [messages(digest, fid, r) for r in rows]
    if digest == "keccak256":
        digs = keccak256_ragged(msgs)
    else:
        fn = {"sha3_256": hashlib.sha3_256, "sha256": hashlib.sha256, "blake2b": hashlib.blake2b}[digest]
        digs = [_hashlib_many(fn, m) for m in msgs]
    out = {}
    for r, d in zip(rows, digs):
        a = np.ascontiguousarray(d).view("<u4").astype(np.uint32)
        a.setflags(write=False)
        out[r] = a
    return out


def three_way(nb, seed):
    """a sample of three-range splits (a, b): [0, a), [a, b), [b, nb) -- always one with a one-block middle range"""
    if nb < 3:
        return []
    g = np.random.default_rng([nb, seed])
    a = int(g.integers(1, nb - 1))
    out = {(a, a + 1)}
    if nb > 3:
        x, y = sorted(int(v) for v in g.choice(np.arange(1, nb), 2, replace=False))
        out.add((x, y))
    return sorted(out)


# ---- CPU checks ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fid", FIDS)
def test_row_counts_reach_every_block_edge(fid):
    """every residue the one-shot block-edge tests name (digest_ref / digest_more edge_rows) that the field can reach at all lies inside
    1 .. max_rows: the 0x80 / length block that is padding alone for SHA-256, the last message byte as the last byte of a rate block for
    the sponges, the exactly full final block of BLAKE2b"""
    L = CM.FIELD_L[fid]
    for digest, fn, wanted in (("sha3_256", DR.sha3_residue, DR.SHA3_RESIDUES), ("keccak256", DR.sha3_residue, DR.SHA3_RESIDUES),
                               ("sha256", DM.sha256_residue, DM.SHA256_RESIDUES), ("blake2b", DR.blake2b_residue, DR.BLAKE2B_RESIDUES)):
        have = {fn(L, r) for r in range(1, max_rows(digest) + 1)}
        reachable = {fn(L, r) for r in range(1, 2000)}
        assert set(wanted) & reachable <= have, (digest, fid)
    if fid in (0, 2):
        r = 3 if fid == 0 else 1                    # SHA-256, 4 + L r = 7 mod 8: the length takes a block of padding alone
        assert DM.sha256_residue(L, r) == 7 and n_blocks("sha256", fid, r) == (4 + L * r) // 8 + 2
    assert any(DR.blake2b_residue(L, r) == 0 for r in range(1, max_rows("blake2b") + 1))
    assert any(DR.sha3_residue(L, r) == 0 for r in range(1, max_rows("sha3_256") + 1))
    # more than one block at most row counts, and at least three somewhere: every split kind exists
    for digest in DIGESTS:
        assert max(n_blocks(digest, fid, r) for r in range(1, max_rows(digest) + 1)) >= 4


def test_block_rules_match_the_library_and_hashlib():
    """n_blocks is what the harness (kernels.h) counts, and the message of n_blocks blocks is what the padding rules make of it"""
    for digest in DIGESTS:
        P, W = H.SHAPE[digest][:2]
        for fid in FIDS:
            for r in range(1, max_rows(digest) + 1):
                nb = n_blocks(digest, fid, r)
                assert H.leaf_blocks(digest, fid, r) == nb
                nbytes = 8 * (P + CM.FIELD_L[fid] * r)
                pad = {"sha3_256": nbytes // 136 + 1, "keccak256": nbytes // 136 + 1, "sha256": (nbytes + 9 + 63) // 64,
                       "blake2b": max(1, -(-nbytes // 128))}[digest]
                assert nb == pad
                assert blocks_ready(digest, fid, r, r) == nb and blocks_ready(digest, fid, r, 0) == 0
                for r1 in range(1, r):
                    b = blocks_ready(digest, fid, r, r1)
                    last = last_row_of(digest, fid, r, b)
                    assert last is None or last < r1
    assert int(H.lib().lrh_leaf_blocks(9, 2, 5)) == 0 and int(H.lib().lrh_leaf_blocks(0, 3, 5)) == 0


def test_keccak_reference_is_the_sponge():
    """keccak256_ragged on mixed lengths == digest_more.keccak256 (pinned to the published vectors there), and the same batching with
    SHA3's domain byte would be hashlib's: the lanes, the padding and the prefix-of-lanes loop are right"""
    g = np.random.default_rng(5)
    msgs = [g.integers(0, 256, (n, ln), dtype=np.uint8) for n, ln in ((3, 135), (2, 136), (1, 137), (2, 32), (4, 272), (1, 407), (2, 408))]
    got = keccak256_ragged(msgs)
    for m, d in zip(msgs, got):
        for row, dig in zip(m, d):
            assert dig.tobytes() == DM.keccak256(row.tobytes())
    assert DM.sha3_256_sponge(msgs[0][0].tobytes()) == hashlib.sha3_256(msgs[0][0].tobytes()).digest()


def test_lr_harness_is_a_separate_library():
    """lib/liblcpc_lr_harness.so (tests/native/lr_harness.cpp, a further artefact of the Makefile's `all`): lrh_* only, linked against
    the product, of which the product carries no trace"""
    import test_abi
    test_abi._harness_is_a_separate_library("lr_harness", "lrh_", "tests/native/lr_harness.cpp", "LRH_OUT")


def test_makefile_builds_the_harness_from_a_clean_tree():
    """a clean checkout has no lib/: `make -n` from there lists the harness link among the steps of `all`, behind the product's"""
    import subprocess
    out = subprocess.run(["make", "-n", "-B", "-C", os.path.join(ROOT, "lcpc_amd", "csrc"), "all"], capture_output=True, text=True, check=True).stdout
    lines = [l for l in out.splitlines() if "-o ../lib/" in l and "-shared" in l]
    names = [l.split("-o ../lib/")[1].split()[0] for l in lines]
    assert "liblcpc_lr_harness.so" in names and names.index("liblcpc_hip.so") < names.index("liblcpc_lr_harness.so")
    assert "lr_harness.cpp" in lines[names.index("liblcpc_lr_harness.so")] and "-llcpc_hip" in lines[names.index("liblcpc_lr_harness.so")]


def test_harness_refuses_bad_ranges_before_the_device():
    """tests/native/lr_harness.cpp checks every index the kernel will form before it touches the device: each of these returns BadArgs on
    a machine with no GPU, where any device call would fail with another error"""
    digest, fid, n_rows, n_cols = "sha3_256", 0, 40, 8            # 44 words: 3 blocks; block 0 holds rows 0 .. 12, block 1 rows 13 .. 29
    sw, dw = H.SHAPE[digest][2:]
    comm = np.zeros((n_rows * n_cols, 1), np.uint64)
    state, out = np.zeros(sw * n_cols, np.uint32), np.zeros(dw * n_cols, np.uint32)

    def bad(digest=digest, fid=fid, comm=comm, rs=n_cols, cs=1, n_cols=n_cols, n_rows=n_rows, b0=0, b1=1, state=state, so=0, out=out, oo=0):
        with pytest.raises(H.BadArgs):
            H.leaf_range(digest, fid, comm, rs, cs, n_cols, n_rows, b0, b1, False, state, so, out, oo)
    bad(b0=2, b1=1)                                   # a range that runs backwards
    bad(b0=0, b1=4)                                   # .. past the last block
    bad(b0=3, b1=4)
    bad(comm=comm[:13 * n_cols - 1])                  # block 0 needs row 12, all of it
    bad(comm=comm[:13 * n_cols], b0=1, b1=2)          # block 1 needs row 29
    bad(comm=comm[:30 * n_cols - 1], b0=1, b1=2)
    bad(comm=comm[:n_rows * n_cols - 1], b0=2, b1=3)  # the last block needs the last row
    bad(comm=comm[:n_rows * n_cols - 1], rs=1, cs=n_rows, b0=2, b1=3)       # .. position-major too
    bad(n_cols=0)
    bad(n_rows=0)
    bad(n_cols=9)                                     # a ninth column: comm, state and out are too short
    bad(state=state[:-1])
    bad(out=out[:-1])
    bad(state=np.zeros(sw * n_cols + 2, np.uint32), so=1)       # a 64-bit state at an odd word
    bad(state=np.zeros(sw * n_cols + 2, np.uint32), so=4)       # .. ending past the buffer
    bad(out=np.zeros(dw * n_cols + 8, np.uint32), oo=2)         # digests off their 16-byte alignment
    bad(out=np.zeros(dw * n_cols + 8, np.uint32), oo=12)
    bad(digest="blake2b", out=out)                              # 16-word digests into a buffer of 8-word ones
    bad(rs=1 << 29)
    with pytest.raises(KeyError):
        H.leaf_range("blake3", fid, comm, n_cols, 1, n_cols, n_rows, 0, 1, False, state, 0, out, 0)
    assert H.lib().lrh_leaf_range(7, 2, comm.ctypes.data, comm.shape[0], n_cols, 1, n_cols, n_rows, 0, 1, 0, state.ctypes.data, state.size, 0,
                                  out.ctypes.data, out.size, 0) == -1
    assert H.lib().lrh_leaf_range(0, 5, comm.ctypes.data, comm.shape[0], n_cols, 1, n_cols, n_rows, 0, 1, 0, state.ctypes.data, state.size, 0,
                                  out.ctypes.data, out.size, 0) == -1
    assert not state.any() and not out.any()

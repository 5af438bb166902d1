"""The references and the case tables of tests/test_gpu_k3_kernels.py -- the BLAKE3 column-hash (K3), Merkle-tree (K4) and path-gather
kernels called directly through tests/k3_harness.py -- with the checks that need no GPU: that the tables reach every block and chunk edge
of the leaf message, every kernel-selection axis (kernels.hip / commit.cpp restated in tests/common.py) and every width of the tree, that
the references are BLAKE3 (oracle/pyref.py, pinned to the official vectors by tests/test_oracle_kats.py) and the reference's Merkle
tree, and that the harness refuses every bad index before it touches the device.  No GPU is needed, but the built tree is:
test_harness_refuses_* loads lcpc_amd/lib/liblcpc_k3_harness.so.

The leaf message of a column is 32 zero bytes and then every row's element as its canonical value in F = 8 L little-endian bytes:
32 + F n_rows bytes, hashed in 1024-byte chunks of 64-byte blocks.  A stored element is x 2^(64 L) mod p; a canon_in buffer holds x.

The references run oracle/pyref.py's b3_compress on numpy uint64 arrays -- one lane per column; its arithmetic is masked to 32 bits and
takes an array where it takes an int -- with the flags and the chunk loop of b3_chunk_cv and the parent rule of b3_parent, and every
case is checked against pyref's own blake3() of the message bytes below."""
import functools
import os
import random
import re
import sys
from collections import namedtuple

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
import common as CM  # noqa: E402
import pyref as P  # noqa: E402

FT = {0: "ft63", 1: "ft127", 2: "ft191", 3: "ft255"}
FIDS = (0, 1, 2, 3)
NLW = CM.NTT_NL                                               # 32-bit words per element
SENTINEL = 0xA5C3F00D
TREE_FLAGS = P.CHUNK_START | P.CHUNK_END | P.ROOT              # a tree node is BLAKE3 of the 64 bytes left || right


# ---- references ----------------------------------------------------------------------------------------------------------------------
def _lanes(a):
    """(n, 8 or 16) uint32 -> list of per-word uint64 lane arrays"""
    return [a[:, i].astype(np.uint64) for i in range(a.shape[1])]


def _unlanes(ws, n):
    return np.stack([np.broadcast_to(np.asarray(w, np.uint64), (n,)) for w in ws], axis=1).astype(np.uint32)


def ref_chunk_cvs(words, msg_len, chunks, n_chunks_total):
    """words (n_cols, >= ceil(msg_len / 4)) uint32: the message words of every column, zero past the message.  -> (len(chunks), n_cols, 8):
    the chaining value of each chunk (b3_chunk_cv's loop; one chunk in all: the ROOT digest).  A lane is a (chunk, column) pair -- the
    chunk counter, block length and flags are per-lane arrays -- and the loop runs over the up to 16 blocks of a chunk"""
    chunks = np.asarray(list(chunks), np.int64)
    n, K = words.shape[0], len(chunks)
    wp = np.zeros((n, 256 * n_chunks_total), np.uint32)
    wp[:, :min(words.shape[1], wp.shape[1])] = words[:, :wp.shape[1]]
    assert not words[:, wp.shape[1]:].any() and n_chunks_total == max(1, -(-msg_len // 1024))
    w3 = wp.reshape(n, n_chunks_total, 256)[:, chunks].transpose(1, 0, 2)                  # (K, n, 256)
    clen = np.minimum(1024, msg_len - 1024 * chunks)
    nblocks = -(-clen // 64)
    cv = np.tile(np.array(P.B3_IV, np.uint32), (K, n, 1))
    for b in range(16):
        act = np.nonzero(nblocks > b)[0]
        if not len(act):
            break
        last = nblocks[act] == b + 1
        flags = (P.CHUNK_START if b == 0 else 0) | np.where(last, P.CHUNK_END | (P.ROOT if n_chunks_total == 1 else 0), 0)
        lane = lambda v: np.repeat(np.asarray(v, np.uint64), n)
        out = P.b3_compress(_lanes(cv[act].reshape(-1, 8)), _lanes(w3[act, :, 16 * b:16 * b + 16].reshape(-1, 16)), lane(chunks[act]),
                            lane(np.minimum(64, clen[act] - 64 * b)), lane(flags))
        cv[act] = _unlanes(out, len(act) * n).reshape(len(act), n, 8)
    return cv


def ref_parent(l, r, is_root):
    """b3_parent on (n, 8) arrays"""
    return _unlanes(P.b3_parent(_lanes(l), _lanes(r), is_root), l.shape[0])


def ref_subtree(cvs, lo, hi, is_root):
    """the BLAKE3 subtree over chunk CVs cvs[lo:hi] ((n_chunks, n, 8)): pyref._b3_subtree's split at the largest power of two below the count"""
    if hi - lo == 1:
        return cvs[lo]
    left = 1 << ((hi - lo - 1).bit_length() - 1)
    return ref_parent(ref_subtree(cvs, lo, lo + left, False), ref_subtree(cvs, lo + left, hi, False), is_root)


def ref_fold_nodes(node_cvs, node_logs, is_root):
    """the incremental (stack) rule of the BLAKE3 paper, generalised to aligned subtrees: after pushing a node of 2^l chunks merge while bit l,
    l + 1, .. of the running chunk count is clear; at the end fold the stack from the top, ROOT on the last parent"""
    stack, total = [], 0
    for j, (cv, l) in enumerate(zip(node_cvs, node_logs)):
        if j == len(node_cvs) - 1:
            break
        total += 1 << l
        t = total >> l
        while t & 1 == 0:
            cv = ref_parent(stack.pop(), cv, False)
            t >>= 1
        stack.append(cv)
    cv = node_cvs[-1]
    while stack:
        left = stack.pop()
        cv = ref_parent(left, cv, is_root and not stack)
    return cv


def ref_node(a, b):
    """one tree level: (n, 8), (n, 8) -> (n, 8) BLAKE3(left || right)"""
    return _unlanes(P.b3_compress(list(P.B3_IV), _lanes(a) + _lanes(b), 0, 64, TREE_FLAGS), a.shape[0])


def ref_tree(hashes, np2, levels_done=0):
    """fill the levels above `levels_done` of a flat (2 np2 - 1, 8) hashes array in place (lib.rs merkle_tree layout: level j + 1 behind level j)"""
    off, w = 0, np2
    for lvl in range(np2.bit_length() - 1):
        if lvl >= levels_done:
            hashes[off + w:off + w + w // 2] = ref_node(hashes[off:off + w:2], hashes[off + 1:off + w:2])
        off, w = off + w, w // 2
    return hashes


def ref_paths(hashes, np2, path_len, cols):
    """open_column's sibling digests: level l's node (col >> l) ^ 1"""
    out = np.zeros((len(cols), path_len, 8), np.uint32)
    for k, c in enumerate(cols):
        off, w = 0, np2
        for lvl in range(path_len):
            out[k, lvl] = hashes[off + ((int(c) >> lvl) ^ 1)]
            off, w = off + w, w // 2
    return out


# ---- operands ------------------------------------------------------------------------------------------------------------------------
N_SPECIAL, POOL = 16, 1024


@functools.lru_cache(maxsize=None)
def pool(fid):
    """POOL distinct elements as (canonical (POOL, NL) uint32 words, stored (POOL, L) uint64 limbs, canonical (POOL, L) uint64 limbs, ints).
    The first N_SPECIAL are the extremes of both forms -- 0, 1, 2, p - 1, p - 2, R mod p (stored 1 ..), and the elements whose STORED form
    is p - 1, p - 2, 1, has all-ones low words (the inputs of fe_canon / fe_canon_r29 are stored forms) or a lone top bit -- the rest random"""
    F, L, nl = P.FIELDS[fid], CM.FIELD_L[fid], NLW[fid]
    p, rng = F.p, random.Random(0xB3 + fid)
    low_ones = (1 << (32 * (nl - 1))) - 1
    top = p >> (32 * (nl - 1))
    stored_special = [p - 1, p - 2, 1, 2, (rng.randrange(top) << (32 * (nl - 1))) | low_ones, ((top - 1) << (32 * (nl - 1))) | low_ones,
                      low_ones, 1 << (p.bit_length() - 2), (1 << (p.bit_length() - 1)) - 1, (1 << 32) - 1]
    xs = [0, 1, p - 1, p - 2, (p - 1) // 2, (p + 1) // 2] + [F.from_mont(s) for s in stored_special]
    assert len(xs) == N_SPECIAL and all(s < p for s in stored_special)
    xs = list(dict.fromkeys(xs))                               # (Ft63: some of the stored extremes coincide; random ones fill up)
    seen = set(xs)
    while len(xs) < POOL:
        x = rng.randrange(p)
        if x not in seen:
            seen.add(x)
            xs.append(x)
    assert len(set(xs)) == POOL
    canon_bytes = b"".join(F.to_repr(x) for x in xs)
    canon_words = np.frombuffer(canon_bytes, "<u4").reshape(POOL, nl).copy()
    canon_limbs = np.frombuffer(canon_bytes, "<u8").reshape(POOL, L).copy()
    stored = CM.to_limbs([F.to_mont(x) for x in xs], L).reshape(POOL, L)
    return canon_words, stored, canon_limbs, xs


def case_index(fid, n_rows, n_cols, seed):
    """(n_rows, n_cols) pool indices: a quarter extremes, the rest anything; column c carries its own number in its first rows (one row:
    c itself; else base-POOL digits in rows 0 and 1), so no two columns of a case are the same message"""
    g = np.random.default_rng([fid, n_rows, n_cols, seed])
    idx = np.where(g.random((n_rows, n_cols)) < 0.25, g.integers(0, N_SPECIAL, (n_rows, n_cols)), g.integers(0, POOL, (n_rows, n_cols)))
    c = np.arange(n_cols)
    assert n_cols <= (POOL if n_rows == 1 else POOL * POOL)
    idx[0] = c % POOL
    if n_rows > 1:
        idx[1] = c // POOL
    return idx


def message_words(fid, idx):
    """(n_cols, 8 + NL n_rows) uint32: every column's leaf message"""
    n_rows, n_cols = idx.shape
    w = pool(fid)[0][idx]                                          # (n_rows, n_cols, NL)
    out = np.zeros((n_cols, 8 + NLW[fid] * n_rows), np.uint32)
    out[:, 8:] = w.transpose(1, 0, 2).reshape(n_cols, -1)
    return out


def comm_buffer(fid, idx, row_base, n_local, layout, canon):
    """the rows [row_base, row_base + n_local) of the case as the flat comm a launch reads: -> (comm (elems, L) uint64, row_stride, col_stride).
    layout "row": row-major (n_cols, 1); "pos": position-major (1, n_local)"""
    vals = pool(fid)[2 if canon else 1][idx[row_base:row_base + n_local]]                 # (n_local, n_cols, L)
    L = CM.FIELD_L[fid]
    if layout == "row":
        return np.ascontiguousarray(vals).reshape(-1, L), idx.shape[1], 1
    return np.ascontiguousarray(vals.transpose(1, 0, 2)).reshape(-1, L), 1, n_local


def rows_of_chunks(fid, n_rows, begin, count):
    """[first, last] rows whose bytes overlap chunks [begin, begin + count) of the leaf message (None: only the zero prefix)"""
    eb = 8 * CM.FIELD_L[fid]
    b0, b1 = 1024 * begin, min(CM.leaf_len(fid, n_rows), 1024 * (begin + count))
    if b1 <= 32:
        return None
    return max(0, b0 - 32) // eb, (b1 - 32 - 1) // eb


# ---- row counts, derived ---------------------------------------------------------------------------------------------------------------
CHUNK_COUNTS = (1, 2, 3, 4, 5, 7, 8, 9, 16, 17, 33)
LAST_NBLOCKS = (1, 2, 3, 15, 16)
MAX_ROWS = 4200


def _first(fid, pred, lo=1):
    return next((n for n in range(lo, MAX_ROWS) if pred(n)), None)


def exact_chunk_fill_rows(fid):
    """n_rows whose message is exactly 1 .. 5 full chunks"""
    return [n for n in range(1, MAX_ROWS) if CM.leaf_len(fid, n) % 1024 == 0 and CM.leaf_n_chunks(fid, n) <= 5]


def short_last_chunk_rows(fid):
    """{n_rows: bytes in the last chunk}: for every size up to one element that the field can leave there, the first row count of two or
    more chunks that does"""
    F = 8 * CM.FIELD_L[fid]
    out = {}
    for b in range(8, F + 1, 8):
        n = _first(fid, lambda n: CM.leaf_n_chunks(fid, n) >= 2 and CM.leaf_last(fid, n)[0] == b)
        if n is not None:
            out[n] = b
    return out


def exact_block_fill_rows(fid):
    """{(n_chunks, nblocks of the last chunk): n_rows} where the message ends exactly on a block boundary, for 1 .. 3 chunks"""
    out = {}
    for nc in (1, 2, 3):
        for nb in LAST_NBLOCKS:
            n = _first(fid, lambda n: CM.leaf_n_chunks(fid, n) == nc and CM.leaf_last(fid, n)[1:] == (nb, 64))
            if n is not None:
                out[(nc, nb)] = n
    return out


def first_rows_of_chunk_count(fid):
    return {c: _first(fid, lambda n: CM.leaf_n_chunks(fid, n) == c) for c in CHUNK_COUNTS}


@functools.lru_cache(maxsize=None)
def row_table(fid):
    rows = set()
    for n in exact_chunk_fill_rows(fid):
        rows |= {n, n + 1}
    rows |= set(short_last_chunk_rows(fid))
    for n in exact_block_fill_rows(fid).values():
        rows |= {n - 1, n, n + 1}
    rows |= set(first_rows_of_chunk_count(fid).values())
    rows.discard(0)
    return sorted(rows)


# ---- leaf cases ------------------------------------------------------------------------------------------------------------------------
# split: the chunk ranges (begin, count) of the split-range launches, a partition of the message; the whole-message launch always runs too
LeafCase = namedtuple("LeafCase", "fid n_rows n_cols canon layout split")
SMALL_COLS = (70, 257, 1, 64, 100, 300)                    # not multiples of 64 / 256 but one; 257 and 300: a second 256-lane workgroup
BIG_COLS = 2100                                             # x 33 chunks > 65536 (one lane per column), x 1 .. 31 chunks <= 65536 (QUAD)


def _splits(nc, i):
    if nc == 1:
        return ((0, 1),)
    if nc == 2:
        return ((0, 1), (1, 1))
    if i % 2:
        return ((0, nc // 2), (nc // 2, nc - nc // 2))
    return ((0, 1), (1, nc - 2), (nc - 1, 1))


@functools.lru_cache(maxsize=None)
def leaf_cases(fid):
    out = []
    for i, n in enumerate(row_table(fid)):
        nc = CM.leaf_n_chunks(fid, n)
        out.append(LeafCase(fid, n, SMALL_COLS[i % len(SMALL_COLS)], bool(i & 1), "pos" if i & 2 else "row", _splits(nc, i >> 2)))
    # one lane per column: 33 chunks on BIG_COLS columns, both CANON values; the ranges (0, 1) and (5, 15) are QUAD launches beside
    # one-lane neighbours, (1, 4) and (20, 13) start and end mid-message
    n33 = first_rows_of_chunk_count(fid)[33]
    for canon, layout, split in ((False, "row", ((0, 1), (1, 32))), (True, "pos", ((0, 5), (5, 15), (20, 13)))):
        out.append(LeafCase(fid, n33, BIG_COLS, canon, layout, split))
    return out


def leaf_case_id(c):
    return "%s-r%d-c%d-%s-%s-%s" % (FT[c.fid], c.n_rows, c.n_cols, "canon" if c.canon else "stored", c.layout,
                                    "+".join("%d.%d" % s for s in c.split))


def launch_rows(c, begin, count, whole):
    """(row_base, n_rows_local) of a launch: the whole-message launch holds every row; a range launch the rows of its chunks and one
    more on either side where the message has one (so row_base > 0 for a range that starts mid-message)"""
    if whole:
        return 0, c.n_rows
    r = rows_of_chunks(c.fid, c.n_rows, begin, count)
    if r is None:
        return 0, 1
    lo, hi = max(0, r[0] - 1), min(c.n_rows - 1, r[1] + 1)
    return lo, hi - lo + 1


# ---- finish cases ----------------------------------------------------------------------------------------------------------------------
def aligned_decompositions(lo, hi):
    """every way to tile chunks [lo, hi) with nodes of 2^l chunks that start at multiples of their size: lists of logs"""
    if lo == hi:
        return [[]]
    out, l = [], 0
    while lo % (1 << l) == 0 and lo + (1 << l) <= hi:
        out += [[l] + rest for rest in aligned_decompositions(lo + (1 << l), hi)]
        l += 1
    return out


def sampled_decomposition(lo, hi, rng):
    logs, at = [], lo
    while at < hi:
        ls = [l for l in range(12) if at % (1 << l) == 0 and at + (1 << l) <= hi]
        logs.append(rng.choice(ls))
        at += 1 << logs[-1]
    return logs


def finish_node_cases():
    """(n_chunks, logs): every aligned decomposition for counts <= 9, four seeded ones for each count beyond"""
    rng = random.Random(33)
    out = []
    for c in CHUNK_COUNTS:
        if c <= 9:
            out += [(c, d) for d in aligned_decompositions(0, c)]
        else:
            out += [(c, sampled_decomposition(0, c, rng)) for _ in range(4)]
    return out


PREMERGE_RANGES = ((0, 1), (3, 1), (0, 2), (6, 2), (4, 4), (8, 8), (16, 16), (32, 32))      # (chunk0, 2^k chunks): aligned subtrees


# ---- tree cases ------------------------------------------------------------------------------------------------------------------------
TREE_NP2 = tuple(1 << k for k in range(1, 21))                # levels_done = 0
FUSED_NP2 = tuple(1 << k for k in range(7, 17))               # levels_done = 6: what leaf_tree_supported allows (128 .. 65536)
PATH_NP2 = (2, 4, 512, 1024, 1 << 17)

# leaf_tree_supported's borders: (n_cols, np2, chunk_begin, n_chunks_local, n_chunks_total)
LEAF_TREE_PROBES = [(64, 64, 0, 1, 1), (128, 128, 0, 1, 1), (128, 128, 0, 2, 2), (192, 256, 0, 1, 1), (192, 192, 0, 1, 1), (129, 256, 0, 1, 1),
                    (256, 512, 0, 1, 1), (256, 256, 0, 1, 1), (65536, 65536, 0, 1, 1), (65536, 65536, 0, 2, 2), (32768, 32768, 0, 2, 2),
                    (32832, 65536, 0, 2, 2), (65600, 131072, 0, 1, 1), (131072, 131072, 0, 1, 1), (256, 256, 0, 3, 3), (256, 256, 1, 1, 2),
                    (256, 256, 0, 1, 2), (256, 256, 1, 2, 2), (320, 512, 0, 1, 1), (200, 256, 0, 1, 1)]

# leaf_tree launches: (fid, n_rows, n_cols, canon, layout).  One and two chunks for every field and both CANON values; Ft191 with the
# element that straddles the chunk boundary (43 rows: row 41 holds bytes 1016 .. 1040); a full first chunk and a short second one
def leaf_tree_cases():
    out = []
    for fid in FIDS:
        full = exact_chunk_fill_rows(fid)[0] if fid != 2 else None
        one = full if full is not None else first_rows_of_chunk_count(fid)[2] - 1
        two = sorted(short_last_chunk_rows(fid))[0]
        for i, (n, n_cols) in enumerate(((one, 128), (two, 256), (one // 2, 512), (two + 7, 128))):
            for canon in (False, True):
                out.append((fid, n, n_cols, canon, "pos" if (i + canon) & 1 else "row"))
    return out


# ---- batch cases (lcpc_amd/csrc/kernels.hip's BATCH forms, tests/test_gpu_k3_batch.py) ---------------------------------------------------------
# A batched buffer holds member i in the first words of row i of an (n_batch, stride) word array.  A gap is what a stride adds to one
# member rounded up to 4 words (kernels.h: strides are multiples of 4 words); None: more than a member
BATCH_SIZES = (1, 2, 3, 7)
BATCH_COLS = (1, 63, 64, 65, 255, 257, 300)                 # the last workgroup partly filled: 64 columns (QUAD), 256 (one lane each)
BATCH_CHUNKS = (1, 2, 3, 5)
BATCH_GAPS = ((0, 0), (4, 4), (None, None), (0, 12), (8, 0))          # (comm, out): tight, 4 words, above a member, unequal
BatchLeafCase = namedtuple("BatchLeafCase", "fid n_rows n_cols canon layout split n_batch comm_gap out_gap")


def batch_stride(member_words, gap):
    m = -(-member_words // 4) * 4
    return m + (m + 8 if gap is None else gap)


def batch_index(fid, n_rows, n_cols, n_batch, seed):
    """(n_batch, n_rows, n_cols) pool indices, every member its own table: a quarter extremes, the rest anything, and (up to POOL columns
    and members) row 0 of member m is column number + 3 m mod POOL -- the columns of a member differ, and so does column c of any two;
    a batch of more members carries the member number in base POOL in its first two columns, so that whole members differ"""
    g = np.random.default_rng([fid, n_rows, n_cols, n_batch, seed])
    shape = (n_batch, n_rows, n_cols)
    idx = np.where(g.random(shape) < 0.25, g.integers(0, N_SPECIAL, shape), g.integers(0, POOL, shape))
    if n_cols <= POOL and n_batch <= POOL:
        idx[:, 0] = (np.arange(n_cols)[None, :] + 3 * np.arange(n_batch)[:, None]) % POOL
    elif n_batch > POOL:
        assert n_cols >= 2 and n_batch <= POOL * POOL
        idx[:, 0, 0], idx[:, 0, 1] = np.arange(n_batch) % POOL, np.arange(n_batch) // POOL
    return idx


def batch_message_words(fid, idx):
    """(n_batch * n_cols, 8 + NL n_rows): message_words of every member, member-major"""
    n_batch, n_rows, n_cols = idx.shape
    return message_words(fid, idx.transpose(1, 0, 2).reshape(n_rows, n_batch * n_cols))


def batch_comm_buffer(fid, idx, row_base, n_local, layout, canon):
    """comm_buffer for every member: -> ((n_batch, elems, L) uint64, row_stride, col_stride)"""
    vals = pool(fid)[2 if canon else 1][idx[:, row_base:row_base + n_local]]              # (n_batch, n_local, n_cols, L)
    n_batch, L = idx.shape[0], CM.FIELD_L[fid]
    if layout == "row":
        return np.ascontiguousarray(vals).reshape(n_batch, -1, L), idx.shape[2], 1
    return np.ascontiguousarray(vals.transpose(0, 2, 1, 3)).reshape(n_batch, -1, L), 1, n_local


@functools.lru_cache(maxsize=None)
def batch_leaf_cases():
    """the four-lanes-per-column form: every column count with every field, the other axes cycling at periods that do not divide"""
    out = []
    for fid in FIDS:
        first = first_rows_of_chunk_count(fid)
        for i, n_cols in enumerate(BATCH_COLS):
            k = len(BATCH_COLS) * fid + i
            nc = BATCH_CHUNKS[(i + fid) % 4]
            gap = BATCH_GAPS[k % 5]
            out.append(BatchLeafCase(fid, first[nc] + i % 3, n_cols, bool((i + fid) & 1), "pos" if (k // 2) & 1 else "row", _splits(nc, k // 3),
                                     BATCH_SIZES[(k + k // 4) % 4], gap[0], gap[1]))
    return out


BORDER_COLS = 257                                            # 255 members: 65535 pairs; 256 members: 65792


@functools.lru_cache(maxsize=None)
def batch_lane_cases():
    """either side of launch_leaf_chunks_nl's 65536 (column, chunk) pairs of a whole batch: exactly that many and one member more; every
    leaf_chunk_kernel<NL, CANON, false, true> just above it on a column count that fills no workgroup; three chunks on one shape in both
    forms; a batch whose range launch (1, 2) is one lane per column as well"""
    one = ((0, 1),)
    out = [BatchLeafCase(0, 1, 256, False, "row", one, 256, 0, 0), BatchLeafCase(0, 1, 256, False, "row", one, 257, 0, 0)]
    for fid in FIDS:
        for canon in (False, True):
            out.append(BatchLeafCase(fid, 1 + fid, BORDER_COLS, canon, "pos" if canon else "row", one, 256, 4 if canon else 0, 0))
    out.append(BatchLeafCase(1, 1, BORDER_COLS, True, "row", one, 255, 0, 0))
    three = first_rows_of_chunk_count(2)[3]
    out += [BatchLeafCase(2, three, 300, False, "row", ((0, 1), (1, 2)), n, 0, 0) for n in (72, 73)]
    out.append(BatchLeafCase(3, first_rows_of_chunk_count(3)[3], BORDER_COLS, True, "pos", ((0, 1), (1, 2)), 128, 0, 4))
    return out


GRID_LIMIT_LEAF = BatchLeafCase(0, 1, 4, False, "row", ((0, 1),), CM.K3B_MAX_BATCH, 0, 0)


def batch_case_id(c):
    gap = lambda g: "m" if g is None else str(g)
    return "%s-b%d-g%s.%s" % (leaf_case_id(c), c.n_batch, gap(c.comm_gap), gap(c.out_gap))


TREE_BATCH = (1, 2, 5)


@functools.lru_cache(maxsize=None)
def tree_batch_cases():
    """(np2, levels_done, n_batch, gap): every width from either starting level; all of TREE_BATCH where the width handed to the launcher is
    256 .. 2048 (either side of lw <= 9: one 1024-thread launch, or 256-thread launches first), one of them elsewhere, two members above
    2^16 leaves (2^19: three launches over two members) and one at 2^20, where the reference of a second would take the test's time"""
    out = []
    for ld, widths in ((0, TREE_NP2), (6, FUSED_NP2)):
        for k, np2 in enumerate(widths):
            if np2 > 1 << 16:
                nbs = (2,) if np2 < 1 << 20 else (1,)
            elif 256 <= np2 >> ld <= 2048:
                nbs = TREE_BATCH
            else:
                nbs = (TREE_BATCH[k % 3],)
            for j, nb in enumerate(nbs):
                out.append((np2, ld, nb, (0, 4, None)[(k + j) % 3] if np2 <= 1 << 16 else (0, 4)[k % 2]))
    return out


LEAF_TREE_BATCH = (1, 3, 5)


def leaf_tree_batch_cases():
    """leaf_tree_cases() with (n_batch, comm gap, hashes gap) cycling"""
    return [c + (LEAF_TREE_BATCH[i % 3],) + BATCH_GAPS[i % 5] for i, c in enumerate(leaf_tree_cases())]


def finish_stack_slots(n_chunks):
    """the slots of cvs that leaf_finish_kernel's stack stores to (the rule of ref_fold_nodes on single chunks); the others are only read"""
    depth, written = 0, set()
    for j in range(n_chunks - 1):
        t = j + 1
        while t & 1 == 0:
            depth -= 1
            t >>= 1
        written.add(depth)
        depth += 1
    return written


PLACE_BIG = 4096 * 256 + 257                                 # batch_place_kernel's grid is capped at 4096 workgroups: a second trip of its loop


def place_cases():
    """(n_batch, src_stride, n_valid, dst_stride)"""
    out = []
    for i, ds in enumerate((1, 255, 256, 257)):
        for j, nv in enumerate(sorted({0, 1, ds - 1, ds})):
            for loose in (False, True):
                out.append(((1, 3)[(i + j + loose) % 2], nv + 3 if loose else nv, nv, ds))
    out.append((2, PLACE_BIG + 2, PLACE_BIG - 1, PLACE_BIG))
    out.append((CM.K3B_MAX_BATCH, 5, 3, 4))
    return out


# =========================================================================================================================================
# checks
# =========================================================================================================================================
ISSUE_EXACT = {0: [124, 252], 1: [62, 126], 2: [84, 212], 3: [31, 63, 95]}
ISSUE_SHORT = {0: {125: 8}, 1: {63: 16}, 2: {42: 16, 85: 24, 127: 8}, 3: {32: 32}}
ISSUE_FIRST33 = {0: (125, 4093), 1: (63, 2047), 2: (42, 1365), 3: (32, 1024)}


@pytest.mark.parametrize("fid", FIDS)
def test_row_tables_are_derived_and_reach_every_edge(fid):
    F = 8 * CM.FIELD_L[fid]
    ex = exact_chunk_fill_rows(fid)
    assert set(ISSUE_EXACT[fid]) <= set(ex) and all((32 + F * n) % 1024 == 0 for n in ex)
    if fid == 2:
        assert ex == [84, 212]                                   # 1024 k - 32 is a multiple of 24 for k = 2, 5 only
    assert short_last_chunk_rows(fid) == ISSUE_SHORT[fid]
    first = first_rows_of_chunk_count(fid)
    assert (first[2], first[33]) == ISSUE_FIRST33[fid] and first[1] == 1
    rows = row_table(fid)
    assert all(n in rows and n + 1 in rows for n in ex) and all(n in rows for n in ISSUE_SHORT[fid]) and all(n in rows for n in first.values())
    # exact last-block fill and both neighbours, at every block count of the last chunk the pipelined loop distinguishes
    mod, res = {0: (8, 4), 1: (4, 2), 2: (8, 4), 3: (2, 1)}[fid]
    eb = exact_block_fill_rows(fid)
    assert {nb for _, nb in eb} == set(LAST_NBLOCKS)
    for n in eb.values():
        assert n % mod == res and CM.leaf_len(fid, n) % 64 == 0 and {n - 1, n, n + 1} - {0} <= set(rows)
    assert all((CM.leaf_len(fid, n) % 64 == 0) == (n % mod == res) for n in range(1, 300))
    assert {CM.leaf_last(fid, n)[1] for n in rows} >= set(LAST_NBLOCKS)
    assert {CM.leaf_n_chunks(fid, n) for n in rows} >= set(CHUNK_COUNTS)
    # last-block sizes: full, one element, and (Ft63) the 8-byte last chunk
    lb = {CM.leaf_last(fid, n)[2] for n in rows}
    assert 64 in lb and min(lb) == {0: 8, 1: 16, 2: 8, 3: 32}[fid]
    # odd and even block counts of a chunk, 1 and 16
    assert {CM.leaf_last(fid, n)[1] % 2 for n in rows} == {0, 1}
    if fid == 2:
        # all three block phases, and a chunk boundary inside an element (row 41 of >= 43 rows: bytes 1016 .. 1040)
        assert CM.leaf_block_phases(2, [0]) == {0, 2, 4} and [(16 * b - 8) % 6 for b in range(3)] == [4, 2, 0]
        assert any(CM.leaf_n_chunks(2, n) >= 3 for n in rows)
        assert (32 + 24 * 41) < 1024 < (32 + 24 * 42) and any(n >= 43 for n in rows)
    else:
        assert CM.leaf_block_phases(fid, range(40)) == {0}


@pytest.mark.parametrize("fid", FIDS)
def test_leaf_cases_reach_every_selection_axis(fid):
    cases = leaf_cases(fid)
    assert [c.n_rows for c in cases[:len(row_table(fid))]] == row_table(fid)
    launches = []                                               # (quad, canon, layout, row_base, n_chunks_total, begin, count)
    for c in cases:
        nc = CM.leaf_n_chunks(fid, c.n_rows)
        assert sum(k for _, k in c.split) == nc and all(c.split[i][0] + c.split[i][1] == c.split[i + 1][0] for i in range(len(c.split) - 1))
        assert c.split[0][0] == 0
        for whole, (b, k) in [(True, (0, nc))] + [(False, s) for s in c.split]:
            launches.append((CM.leaf_quad(c.n_cols, k), c.canon, c.layout, launch_rows(c, b, k, whole)[0], nc, b, k))
    ax = lambda i: {l[i] for l in launches}
    assert ax(0) == {True, False} and ax(1) == {True, False} and ax(2) == {"row", "pos"}
    assert 0 in ax(3) and max(ax(3)) > 0
    assert 1 in ax(4) and max(ax(4)) == 33
    for quad in (True, False):
        for canon in (True, False):                             # every instantiation leaf_chunk_kernel<NL, CANON, QUAD>, on many chunks
            assert any(l[0] == quad and l[1] == canon and l[4] > 1 for l in launches)
    mid = [l for l in launches if l[5] > 0 and l[5] + l[6] < l[4]]          # starts and ends mid-message
    assert mid and any(l[6] == 1 for l in launches if l[5] > 0) and any(l[3] > 0 for l in mid)
    # a case whose neighbouring ranges differ in QUAD
    assert any(len({CM.leaf_quad(c.n_cols, k) for _, k in c.split}) == 2 for c in cases)
    assert {c.n_cols % 64 != 0 for c in cases} == {True, False} and any(c.n_cols % 256 for c in cases) and any(c.n_cols > 256 for c in cases)


def _fn_body(src, head):
    """the text of the function whose definition starts with `head`, up to its closing brace at column 0"""
    i = src.index(head)
    return src[i:src.index("\n}\n", i)]


def test_selection_rules_match_the_sources():
    """the numbers tests/common.py restates are the ones in kernels.hip"""
    src = open(os.path.join(ROOT, "lcpc_amd", "csrc", "kernels.hip")).read()
    # one rule for single and batched commits: launch_leaf_chunks calls it with n_batch = 1
    assert [int(v) for v in re.findall(r"const bool quad = \(u64\)a\.n_cols \* a\.n_chunks_local \* n_batch <= (\d+);", src)] == [CM.K3_QUAD_MAX]
    assert "hipError_t launch_leaf_chunks(int nl, const LeafArgs& a, hipStream_t st) { return launch_leaf_chunks_t<false>(nl, a, 1, 0, 0, st); }" in src
    assert int(re.search(r"constexpr u32 SLICE = (\d+);", _fn_body(src, "static hipError_t launch_leaf_chunks_t(")).group(1)) == CM.K3_SLICE
    m = re.search(r"bool leaf_tree_supported\(const LeafArgs& a, u64 np2\) \{\s*return (.*?);\s*\}", src, re.S).group(1)
    assert re.sub(r"\s+", " ", m) == ("a.n_chunks_total <= 2 && a.n_chunks_local == a.n_chunks_total && a.chunk_begin == 0 && np2 == a.n_cols && "
                                      "a.n_cols >= 128 && (a.n_cols & 63) == 0 && a.n_cols * a.n_chunks_total <= 65536")
    assert "if (lw <= 9) {" in src and "const u32 lsub = 9;" in src and "constexpr u32 NQ = BS / 4;" in src
    assert src.count("if (n_out > NQ) {") == 2


def test_tree_cases_reach_every_width_and_branch():
    assert TREE_NP2 == tuple(2 ** k for k in range(1, 21)) and FUSED_NP2 == (128, 256, 512, 1024, 2048, 4096, 8192, 16384, 32768, 65536)
    seen = set()
    for np2, ld in [(n, 0) for n in TREE_NP2] + [(n, 6) for n in FUSED_NP2]:
        ls = CM.merkle_launches(np2, ld)
        assert ls[-1][0] == 1024 and ls[-1][1] == 1 and all(bs == 256 and lsub == 9 for bs, _, lsub, _ in ls[:-1])
        assert sum(l[2] for l in ls) + ld == np2.bit_length() - 1
        seen |= {(bs, br) for bs, _, _, brs in ls for br in brs}
        seen |= {("wg", nwg) for bs, nwg, _, _ in ls if bs == 256}
    # n_out against BS / 4: the 256-thread kernel folds 512 nodes (levels of 256 and 128 parents on lanes, 64 .. 1 on quads); the one
    # 1024-thread workgroup is only ever given <= 512 nodes, so its levels have <= 256 = BS / 4 parents: its lane side has no caller
    assert seen - {s for s in seen if s[0] == "wg"} == {(256, "lane"), (256, "quad"), (1024, "quad")}
    assert min(s[1] for s in seen if s[0] == "wg") == 2 and ("wg", 2048) in seen          # two .. 2048 workgroups of 512 nodes
    assert len(CM.merkle_launches(1 << 20)) == 3 and len(CM.merkle_launches(1 << 19)) == 3 and len(CM.merkle_launches(1 << 18)) == 2
    assert {CM.merkle_launches(n, 0)[-1][2] for n in TREE_NP2} == set(range(1, 10))        # every lsub of the last workgroup
    want = {p: CM.leaf_tree_supported(*p) for p in LEAF_TREE_PROBES}
    assert sum(want.values()) >= 6 and sum(not v for v in want.values()) >= 10
    # each clause of the rule decides at least one probe alone
    flip = lambda p, i, v: CM.leaf_tree_supported(*(p[:i] + (v,) + p[i + 1:]))
    assert want[(128, 128, 0, 1, 1)] and not want[(64, 64, 0, 1, 1)] and not want[(192, 256, 0, 1, 1)] and want[(192, 192, 0, 1, 1)]
    assert not want[(129, 256, 0, 1, 1)] and want[(65536, 65536, 0, 1, 1)] and not want[(65536, 65536, 0, 2, 2)] and want[(32768, 32768, 0, 2, 2)]
    assert not want[(131072, 131072, 0, 1, 1)] and not want[(256, 256, 0, 3, 3)] and not want[(256, 256, 1, 1, 2)] and not want[(256, 256, 0, 1, 2)]
    assert flip((256, 256, 0, 3, 3), 3, 2) is False and flip((256, 256, 1, 1, 2), 2, 0) is False
    for fid, n, n_cols, canon, layout in leaf_tree_cases():
        assert n_cols & (n_cols - 1) == 0                       # the tree is over np2 == n_cols leaves: a power of two
        assert CM.leaf_tree_supported(n_cols, n_cols, 0, CM.leaf_n_chunks(fid, n), CM.leaf_n_chunks(fid, n)), (fid, n, n_cols)
    lt = leaf_tree_cases()
    for fid in FIDS:
        mine = [c for c in lt if c[0] == fid]
        assert {(CM.leaf_n_chunks(fid, c[1]), c[3]) for c in mine} == {(1, False), (1, True), (2, False), (2, True)}
        assert {c[4] for c in mine} == {"row", "pos"}
    assert any(c[0] == 2 and c[1] >= 43 for c in lt)                                   # Ft191's straddling element
    assert any(CM.leaf_last(c[0], c[1])[0] <= 8 * CM.FIELD_L[c[0]] and CM.leaf_n_chunks(c[0], c[1]) == 2 for c in lt)   # short second chunk


def test_finish_cases():
    cases = finish_node_cases()
    assert {c for c, _ in cases} == set(CHUNK_COUNTS)
    for c, logs in cases:
        at = 0
        for l in logs:
            assert at % (1 << l) == 0
            at += 1 << l
        assert at == c
    count = lambda c: sum(1 for k, _ in cases if k == c)
    assert [count(c) for c in (1, 2, 3, 4, 5, 7, 8, 9)] == [1, 2, 2, 5, 5, 10, 26, 26]      # f(2^k) = 1 + f(2^(k-1))^2; f(a + b) = f(a) f(b)
    assert any(len(logs) == 1 and c > 1 for c, logs in cases)                                # a single node that is the whole message
    assert all(n & (n - 1) == 0 and c0 % n == 0 for c0, n in PREMERGE_RANGES)


@pytest.mark.parametrize("fid", FIDS)
def test_operand_pool(fid):
    cw, stored, cl, xs = pool(fid)
    F = P.FIELDS[fid]
    p, L = F.p, F.L
    assert {0, 1, p - 1} <= set(xs[:N_SPECIAL])
    st = [sum(int(stored[i, j]) << (64 * j) for j in range(L)) for i in range(POOL)]
    assert all(s == x * (1 << (64 * L)) % p for s, x in zip(st, xs))                       # stored = x 2^(64 L) mod p
    assert p - 1 in st[:N_SPECIAL] and 1 in st[:N_SPECIAL]
    low = (1 << (32 * (NLW[fid] - 1))) - 1
    assert sum(1 for s in st[:N_SPECIAL] if s & low == low) >= 3                           # all-ones low words in the STORED form
    assert all(cw[i].tobytes() == F.to_repr(xs[i]) == cl[i].tobytes() for i in range(POOL))
    idx = case_index(fid, 5, 300, 1)
    assert len({tuple(col) for col in idx.T}) == 300 and (idx < N_SPECIAL).mean() > 0.2
    assert len({tuple(col) for col in case_index(fid, 1, 70, 1).T}) == 70
    words = message_words(fid, case_index(fid, 3, 4, 1))
    assert words[2].tobytes() == b"\0" * 32 + b"".join(F.to_repr(xs[i]) for i in case_index(fid, 3, 4, 1)[:, 2])


CPU_COLS = 3          # the references are checked on a few columns of every case: the arithmetic is per lane


@pytest.mark.parametrize("fid", FIDS)
def test_reference_cvs_fold_to_blake3(fid):
    """per case: the stack fold of the reference chunk CVs is pyref.blake3 of the message; so is the tree split, and (sampled) every aligned
    node decomposition folded by the stack rule.  One chunk: the reference 'CV' is the digest itself."""
    rng = random.Random(fid)
    seen_rows = set()
    for c in leaf_cases(fid):
        if c.n_rows in seen_rows:
            continue
        seen_rows.add(c.n_rows)
        idx = case_index(fid, c.n_rows, CPU_COLS, 7)
        words = message_words(fid, idx)
        nc, mlen = CM.leaf_n_chunks(fid, c.n_rows), CM.leaf_len(fid, c.n_rows)
        cvs = ref_chunk_cvs(words, mlen, range(nc), nc)
        check = (0,) if nc > 9 else range(CPU_COLS)
        want = {k: np.frombuffer(P.blake3(words[k].tobytes()[:mlen]), "<u4") for k in check}
        got = cvs[0] if nc == 1 else ref_fold_nodes(list(cvs), [0] * nc, True)
        tree = ref_subtree(cvs, 0, nc, True)
        decomp = sampled_decomposition(0, nc, rng)
        at, nodes = 0, []
        for l in decomp:
            nodes.append(ref_subtree(cvs, at, at + (1 << l), False))
            at += 1 << l
        folded = nodes[0] if nc == 1 else ref_fold_nodes(nodes, decomp, True) if len(nodes) > 1 else None
        for k in check:
            assert np.array_equal(got[k], want[k]) and np.array_equal(tree[k], want[k]), (fid, c.n_rows, k)
            assert folded is None or np.array_equal(folded[k], want[k]), (fid, c.n_rows, decomp)
        if nc > 1:                                              # a chunk CV is pyref's
            for ch in (0, nc - 1):
                assert list(cvs[ch, 0]) == P.b3_chunk_cv(words[0].tobytes()[:mlen][1024 * ch:1024 * ch + 1024], ch, False)


def test_every_decomposition_folds_to_the_same_root():
    g = np.random.default_rng(5)
    for c in (1, 2, 3, 4, 5, 7, 8, 9):
        cvs = g.integers(0, 1 << 32, (c, 2, 8), dtype=np.uint64).astype(np.uint32)
        want = ref_subtree(cvs, 0, c, True)
        for _, logs in [x for x in finish_node_cases() if x[0] == c]:
            at, nodes = 0, []
            for l in logs:
                nodes.append(ref_subtree(cvs, at, at + (1 << l), False))
                at += 1 << l
            if len(nodes) > 1:
                assert np.array_equal(ref_fold_nodes(nodes, logs, True), want), (c, logs)


def test_reference_tree_is_the_merkle_tree(oracle):
    """ref_tree / ref_paths against pyref.merkleize and the C oracle's hashes and opened paths on one small commitment"""
    O = oracle
    fid, n_per_row, n_cols = 1, 6, 16
    F = P.FIELDS[fid]
    oenc = O.Encoding.ligero_from_dims(fid, n_per_row, n_cols)
    oc = O.Commit.commit(O.random_elems(fid, 3 * n_per_row, 3), oenc)
    h = np.ascontiguousarray(oc.hashes()).view(np.uint32).reshape(-1, 8)
    mine = np.zeros_like(h)
    mine[:n_cols] = h[:n_cols]
    assert np.array_equal(ref_tree(mine, n_cols), h)
    comm = [F.from_mont(F.from_limbs(l)) for l in np.asarray(oc.comm()).reshape(-1, F.L)]
    pc = P.LcCommit(comm, None, 3, n_cols, n_per_row, None)
    P.merkleize(F, pc)
    assert b"".join(pc.hashes) == h.tobytes()
    part = h.copy()
    part[n_cols + n_cols // 2:] = 0
    assert np.array_equal(ref_tree(part, n_cols, 1), h)          # levels_done: the levels below are taken as given
    for col in (0, 5, 15):
        _, path = oc.open_column(col)
        assert np.array_equal(ref_paths(h, n_cols, 4, [col])[0].tobytes(), np.asarray(path).tobytes())
    a = np.arange(16, dtype=np.uint32).reshape(2, 8)
    assert ref_node(a[:1], a[1:])[0].tobytes() == P.blake3(a.tobytes())


# ---- the harness refuses what it has not checked ---------------------------------------------------------------------------------------
def _leaf(H, fid=0, n_rows=300, n_cols=8, begin=0, count=None, row_base=0, n_local=None, total=None, comm_elems=None, layout="row"):
    nc = CM.leaf_n_chunks(fid, n_rows) if total is None else total
    n_local = n_rows if n_local is None else n_local
    comm = np.zeros((n_local * n_cols if comm_elems is None else comm_elems, CM.FIELD_L[fid]), np.uint64)
    rs, cs = (n_cols, 1) if layout == "row" else (1, n_local)
    return H.Leaf(fid, comm, rs, cs, n_cols, row_base, n_local, n_rows, begin, nc if count is None else count, nc, False)


def test_harness_refuses_bad_indices_before_the_device():
    """tests/native/k3_harness.cpp checks every index a kernel will form before it touches the device (a kernel that writes out of bounds can
    take the machine down): each of these returns BadArgs on a machine with no GPU, where any device call would fail with another error"""
    import k3_harness as H
    bad = lambda fn, *a: pytest.raises(H.BadArgs, fn, *a) and None
    out = lambda leaf, slots=None: np.zeros((leaf.n_chunks_local if slots is None else slots, leaf.n_cols, 8), np.uint32)
    # Ft63, 300 rows: 2432 bytes = 3 chunks; chunk 1 holds rows 124 .. 251, chunk 2 rows 252 .. 299
    for leaf in (_leaf(H, total=2), _leaf(H, total=4),                      # n_chunks_total is not the message's
                 _leaf(H, begin=2, count=2), _leaf(H, count=0),             # range past the message; empty
                 _leaf(H, begin=1, count=1, row_base=125, n_local=175),     # chunk 1 needs row 124
                 _leaf(H, begin=1, count=1, row_base=124, n_local=127),     # .. and row 251
                 _leaf(H, begin=0, count=1, row_base=1, n_local=299),       # chunk 0 needs row 0
                 _leaf(H, comm_elems=300 * 8 - 1), _leaf(H, comm_elems=300 * 8 - 1, layout="pos"),      # the last element lies outside comm
                 _leaf(H, row_base=-1, n_local=301), _leaf(H, n_cols=0)):
        bad(H.leaf_chunks, leaf, out(leaf, max(1, leaf.n_chunks_local)))
    ok = _leaf(H, begin=1, count=1, row_base=124, n_local=128)
    bad(H.leaf_chunks, ok, out(ok, 3), 3)                                   # output slot past the buffer
    bad(H.leaf_tree, _leaf(H, n_cols=128, comm_elems=128 * 300 - 1), np.zeros((255, 8), np.uint32), 128)
    bad(H.leaf_tree, _leaf(H, n_cols=128, total=2), np.zeros((255, 8), np.uint32), 128)
    with pytest.raises(AssertionError):
        H.leaf_tree(_leaf(H, n_cols=128), np.zeros((200, 8), np.uint32), 128)          # hashes shorter than 2 np2 - 1
    bad(H.leaf_tree, _leaf(H, n_cols=96), np.zeros((2 * 96 - 1, 8), np.uint32), 96)    # np2 is no power of two
    cvs, dig = np.zeros((3, 5, 8), np.uint32), np.zeros((5, 8), np.uint32)
    bad(H.leaf_finish, cvs, dig[:4])                                        # fewer digest slots than columns
    u = lambda *v: np.array(v, np.uint32)
    for slot, log, n_nodes, chunk0, n_chunks, root in ((u(0, 1, 3), u(0, 0, 0), 3, 0, 3, True),          # slot >= n_slots
                                                       (u(0, 1, 1), u(0, 0, 0), 3, 0, 3, True),          # a slot twice
                                                       (u(0, 1), u(0, 1), 2, 0, 3, True),                # node of 2 chunks at chunk 1
                                                       (u(0, 1), u(1, 0), 2, 0, 4, True),                # nodes cover 3 chunks, not 4
                                                       (u(0, 1), u(1, 1), 2, 0, 3, True),                # .. 4, not 3
                                                       (u(0, 1), u(0, 0), 2, 2, 2, True),                # root of a range that is not the message
                                                       (u(0, 1, 2), u(0, 0, 0), 3, 3, 3, False),         # pre-merge of 3 chunks: no subtree
                                                       (u(0, 1), u(0, 0), 2, 1, 2, False),               # .. of an unaligned pair
                                                       (u(0,), u(40,), 1, 0, 1, True)):
        bad(H.leaf_finish_nodes, cvs, slot, log, n_nodes, chunk0, n_chunks, dig, root)
    bad(H.leaf_finish_nodes, cvs, None, None, 4, 0, 4, dig, True)            # more nodes than slots
    h = lambda np2: np.zeros((2 * np2 - 1, 8), np.uint32)
    bad(H.merkle_tree_from, h(128), 128, 7)                                  # levels_done leaves nothing to do ..
    bad(H.merkle_tree_from, h(128), 128, 8)                                  # .. or is taller than the tree
    bad(H.merkle_tree_from, h(2), 2, 1)
    bad(H.merkle_tree_from, np.zeros((5, 8), np.uint32), 3, 0)               # np2 is no power of two
    bad(H.merkle_tree_from, np.zeros((1, 8), np.uint32), 1, 0)
    cols = lambda *v: np.array(v, np.uint64)
    bad(H.gather_paths, h(8), 8, 3, cols(0, 8), np.zeros((2, 3, 8), np.uint32))          # cols < np2
    bad(H.gather_paths, h(8), 8, 4, cols(0), np.zeros((1, 4, 8), np.uint32))             # a path taller than the tree
    bad(H.gather_paths, h(8), 8, 0, cols(0), np.zeros((1, 0, 8), np.uint32))
    # the pure rule needs no device either, and is the restated one on every probe
    for p in LEAF_TREE_PROBES:
        assert H.leaf_tree_supported(*p) == CM.leaf_tree_supported(*p), p


# ---- the batch tables ------------------------------------------------------------------------------------------------------------------
def _batch_launches(c):
    """(quad, begin, count, row_base) of the whole-message launch and the range launches of a batch case"""
    nc = CM.leaf_n_chunks(c.fid, c.n_rows)
    return [(CM.leaf_quad_batch(c.n_cols, k, c.n_batch), b, k, launch_rows(c, b, k, whole)[0])
            for whole, (b, k) in [(True, (0, nc))] + [(False, s) for s in c.split]]


def test_batch_selection_rule_matches_the_source():
    src = open(os.path.join(ROOT, "lcpc_amd", "csrc", "kernels.hip")).read()
    assert [int(v) for v in re.findall(r"const bool quad = \(u64\)a\.n_cols \* a\.n_chunks_local \* n_batch <= (\d+);", src)] == [CM.K3B_QUAD_MAX]

    # each of the five batch launchers reaches a refusal of n_batch > 65535: its own, or that of the implementation it shares with the
    # single launcher (NAME_t<true>)
    assert CM.K3B_MAX_BATCH == 65535
    for entry in ("launch_leaf_chunks_batch", "launch_leaf_tree_batch", "launch_leaf_finish_batch", "launch_merkle_tree_from_batch",
                  "launch_batch_place"):
        b = _fn_body(src, "hipError_t %s(" % entry)
        shared = re.search(r"return (\w+_t)<true>\(", b)
        assert b.count("n_batch > 65535") == 1 if shared is None else _fn_body(src, "static hipError_t %s(" % shared.group(1)).count("n_batch > 65535") == 1, entry
    assert src.count("if (lw <= 9) {") == 1 and "blocks < 4096 ? blocks : 4096" in src
    assert CM.leaf_quad_batch(256, 1, 256) and not CM.leaf_quad_batch(256, 1, 257) and CM.leaf_quad_batch(2048, 3, 1) == CM.leaf_quad(2048, 3)


def test_batch_leaf_cases_reach_every_axis():
    cases = batch_leaf_cases()
    nc = lambda c: CM.leaf_n_chunks(c.fid, c.n_rows)
    assert all(all(l[0] for l in _batch_launches(c)) for c in cases)                   # the quad form throughout
    assert {(c.fid, c.n_cols) for c in cases} == {(f, n) for f in FIDS for n in BATCH_COLS}
    assert {(c.fid, c.canon) for c in cases} == {(f, b) for f in FIDS for b in (False, True)}
    assert {c.n_batch for c in cases} == set(BATCH_SIZES) and {nc(c) for c in cases} == set(BATCH_CHUNKS)
    assert {(c.comm_gap, c.out_gap) for c in cases} == set(BATCH_GAPS) and {c.layout for c in cases} == {"row", "pos"}
    for fid in (1, 2):                                                                  # many chunks for the fields named for it
        assert any(c.fid == fid and nc(c) >= 3 for c in cases)
    assert (32 + 24 * 41) < 1024 < (32 + 24 * 42) and any(c.fid == 2 and c.n_rows >= 43 for c in cases)      # Ft191's straddling element
    many = [c for c in cases if c.n_batch > 1]
    # a partly filled last workgroup in a batch of several, at tight strides (its idle lanes would land in the next member)
    assert any(c.n_cols % 64 and (c.comm_gap, c.out_gap) == (0, 0) for c in many)
    # the two strides differ from each other wherever there is a second member (comm and out members differ), and the gaps differ in some
    for c in many:
        L, slots = CM.FIELD_L[c.fid], nc(c) + 2
        assert batch_stride(2 * L * c.n_rows * c.n_cols, c.comm_gap) != batch_stride(slots * c.n_cols * 8, c.out_gap)
    assert any(c.comm_gap != c.out_gap for c in many)
    ranges = [(c, l) for c in cases for l in _batch_launches(c)[1:]]
    assert any(l[1] > 0 and l[1] + l[2] < nc(c) and c.n_batch > 1 for c, l in ranges)   # starts and ends mid-message
    assert any(l[3] > 0 and c.n_batch > 1 and c.layout == lay for c, l in ranges for lay in ("row", "pos"))     # row_base > 0
    for c in cases:
        assert sum(k for _, k in c.split) == nc(c) and c.split[0][0] == 0
        assert all(c.split[i][0] + c.split[i][1] == c.split[i + 1][0] for i in range(len(c.split) - 1))


def test_batch_lane_cases_sit_on_the_border():
    cases = batch_lane_cases()
    pairs = lambda c: c.n_cols * CM.leaf_n_chunks(c.fid, c.n_rows) * c.n_batch
    assert pairs(cases[0]) == CM.K3B_QUAD_MAX and pairs(cases[1]) == CM.K3B_QUAD_MAX + 256 and cases[1].n_batch == cases[0].n_batch + 1
    assert (cases[0].n_cols, cases[0].n_rows, cases[0].n_batch) == (256, 1, 256)
    whole = {c: _batch_launches(c)[0][0] for c in cases}
    assert whole[cases[0]] and not whole[cases[1]]
    lane = [c for c in cases if not whole[c]]
    assert {(c.fid, c.canon) for c in lane if c.n_cols % 256} == {(f, b) for f in FIDS for b in (False, True)}
    assert any(whole[c] and c.n_cols % 256 and pairs(c) == CM.K3B_QUAD_MAX - 1 for c in cases)
    three = [c for c in cases if CM.leaf_n_chunks(c.fid, c.n_rows) == 3]
    assert any(a._replace(n_batch=0) == b._replace(n_batch=0) and whole[a] and not whole[b] for a in three for b in three)
    assert any(not l[0] and l[1] > 0 for c in cases for l in _batch_launches(c)[1:])    # a lane-per-column launch of a range that starts mid-message
    g = GRID_LIMIT_LEAF
    assert (g.fid, g.n_rows, g.n_cols, g.n_batch) == (0, 1, 4, 65535) and not _batch_launches(g)[0][0]


def test_batch_members_differ():
    """no test that tiles one member can pass: column c of any two members differs (whole members, where the batch outnumbers the pool)"""
    for c in batch_leaf_cases() + batch_lane_cases() + [GRID_LIMIT_LEAF]:
        idx = batch_index(c.fid, c.n_rows, c.n_cols, c.n_batch, 1)
        if c.n_batch <= POOL:
            per_col = idx.transpose(2, 0, 1)                                            # (n_cols, n_batch, n_rows)
            assert all(len(np.unique(m, axis=0)) == c.n_batch for m in per_col[:: max(1, c.n_cols // 7)]), c
            assert all(len(np.unique(m.T, axis=0)) == c.n_cols for m in idx[:: max(1, c.n_batch // 5)]), c
        else:
            assert len(np.unique(idx.reshape(c.n_batch, -1), axis=0)) == c.n_batch, c
    for fid, n_rows, n_cols, canon, layout, n_batch, _, _ in leaf_tree_batch_cases():
        idx = batch_index(fid, n_rows, n_cols, n_batch, 2)
        assert len(np.unique(idx[:, :, 5], axis=0)) == n_batch
    # the member-major references are the single ones on each member
    idx = batch_index(2, 45, 5, 3, 1)
    words = batch_message_words(2, idx)
    for m in range(3):
        assert np.array_equal(words[5 * m:5 * m + 5], message_words(2, idx[m]))
        for layout in ("row", "pos"):
            got, rs, cs = batch_comm_buffer(2, idx, 3, 40, layout, False)
            one, rs1, cs1 = comm_buffer(2, idx[m], 3, 40, layout, False)
            assert np.array_equal(got[m], one) and (rs, cs) == (rs1, cs1)


def test_tree_finish_and_place_batch_tables():
    tc = tree_batch_cases()
    assert {(n, ld) for n, ld, _, _ in tc} == {(n, 0) for n in TREE_NP2} | {(n, 6) for n in FUSED_NP2}
    for ld in (0, 6):
        for first_bs in (1024, 256):                            # every batch size on either side of lw <= 9, from either starting level
            assert {nb for n, l, nb, _ in tc if l == ld and CM.merkle_launches(n, l)[0][0] == first_bs and n <= 1 << 16} >= set(TREE_BATCH)
        assert {g for _, l, nb, g in tc if l == ld and nb > 1} == {0, 4, None}
    assert any(nb > 1 and len(CM.merkle_launches(n, l)) == 3 for n, l, nb, _ in tc)
    lt = leaf_tree_batch_cases()
    assert {c[5] for c in lt} == set(LEAF_TREE_BATCH) and {c[6:] for c in lt if c[5] > 1} == set(BATCH_GAPS)
    assert {(CM.leaf_n_chunks(c[0], c[1]), c[5] > 1) for c in lt} == {(1, False), (1, True), (2, False), (2, True)}
    assert finish_stack_slots(1) == set() and finish_stack_slots(2) == {0} and finish_stack_slots(5) == {0, 1} and finish_stack_slots(8) == {0, 1, 2}
    assert all(max(finish_stack_slots(n), default=-1) < n - 1 for n in CHUNK_COUNTS if n > 1)    # the last chunk's slot is only read
    pc = place_cases()
    assert {ds for _, _, _, ds in pc} == {1, 255, 256, 257, PLACE_BIG, 4} and {nb for nb, _, _, _ in pc} == {1, 2, 3, 65535}
    for ds in (1, 255, 256, 257):
        mine = [c for c in pc if c[3] == ds]
        assert {c[2] for c in mine} == {0, 1, ds - 1, ds} and {c[1] == c[2] for c in mine} == {True, False}
        assert {c[0] for c in mine} == {1, 3} or ds == 1
    assert {c[0] for c in pc if c[3] == 1} == {1, 3}
    assert all(nv <= ss and nv <= ds for _, ss, nv, ds in pc)
    assert -(-PLACE_BIG // 256) > 4096 and (65535, 5, 3, 4) in pc and (2, PLACE_BIG + 2, PLACE_BIG - 1, PLACE_BIG) in pc


def test_harness_refuses_bad_batches_before_the_device():
    """the batch entry points of tests/native/k3_harness.cpp: what test_harness_refuses_bad_indices_before_the_device checks per member, and
    a member count outside 1 .. 65535, a stride below one member and a stride that is no multiple of 4 words"""
    import k3_harness as H
    bad = lambda fn, *a: pytest.raises(H.BadArgs, fn, *a) and None
    w = lambda n_batch, stride: np.zeros((n_batch, stride), np.uint32)

    def lb(n_batch=2, comm_stride=None, **kw):
        leaf = _leaf(H, **kw)
        return H.LeafBatch(leaf, w(n_batch, 2 * leaf.comm.size if comm_stride is None else comm_stride))

    # Ft63, 300 rows x 8 columns: a comm member is 4800 words, an out member of 3 slots 192, a hashes member of 128 leaves 2040
    for b, out in ((lb(0), w(0, 192)), (lb(65536, 4800), w(65536, 192)), (lb(comm_stride=4796), w(2, 192)), (lb(comm_stride=4802), w(2, 192)),
                   (lb(), w(2, 188)), (lb(), w(2, 194)), (lb(total=2), w(2, 192)), (lb(begin=2, count=2), w(2, 192)),
                   (lb(begin=1, count=1, row_base=125, n_local=175), w(2, 192)), (lb(comm_elems=300 * 8 - 1, comm_stride=4800), w(2, 192)),
                   (lb(n_cols=0, comm_stride=8), w(2, 192))):
        bad(H.leaf_chunks_batch, b, out, 3)
    bad(H.leaf_chunks_batch, lb(begin=1, count=1, row_base=124, n_local=128), w(2, 192), 3, 3)      # output slot past the member
    t = dict(n_cols=128)
    for b, hashes in ((lb(0, **t), w(0, 2040)), (lb(65536, 8, n_rows=1, **t), w(65536, 2040)), (lb(comm_stride=76796, **t), w(2, 2040)),
                      (lb(comm_stride=76802, **t), w(2, 2040)), (lb(**t), w(2, 2036)), (lb(**t), w(2, 2042)), (lb(total=2, **t), w(2, 2040)),
                      (lb(comm_elems=128 * 300 - 1, comm_stride=76800, **t), w(2, 2040))):
        bad(H.leaf_tree_batch, b, hashes, 128)
    bad(H.leaf_tree_batch, lb(n_cols=96), w(2, 191 * 8), 96)                 # np2 is no power of two
    bad(H.leaf_tree_batch, lb(**t), w(2, 2040), 128, 1)                     # the launcher may be told n_batch, 0 or more than 65535 only
    bad(H.leaf_tree_batch, lb(**t), w(2, 2040), 128, 65535)
    fin = lambda n_batch=2, cs=3 * 5 * 8, ds=5 * 8, dig_cols=5: (w(n_batch, cs), 3, 5, w(n_batch, ds), dig_cols)
    for a in (fin(0), fin(65536), fin(cs=116), fin(cs=122), fin(ds=36), fin(ds=42), fin(dig_cols=4), fin(ds=40, dig_cols=6)):
        bad(H.leaf_finish_batch, *a)
    root = lambda n: np.zeros((n + 1, 8), np.uint32)
    for hashes, np2, ld, r in ((w(0, 2040), 128, 0, None), (w(65536, 24), 2, 0, None), (w(2, 2036), 128, 0, None), (w(2, 2042), 128, 0, None),
                               (w(2, 2040), 128, 7, root(2)), (w(2, 40), 3, 0, None), (w(2, 8), 1, 0, None), (w(2, 24), 2, 1, root(2))):
        bad(H.merkle_tree_from_batch, hashes, np2, ld, r)
    u = lambda n_batch, stride: np.zeros((n_batch, stride), np.uint64)
    d = lambda n: np.zeros(n, np.uint64)
    for src, nv, dst, ds in ((u(0, 4), 4, d(8), 4), (u(65536, 1), 1, d(65536), 1), (u(2, 4), 5, d(16), 8),      # n_valid > src_stride
                             (u(2, 8), 5, d(16), 4), (u(2, 4), 4, d(7), 4), (u(2, 4), 0, d(8), 0)):               # .. > dst_stride; dst too short
        bad(H.batch_place, src, nv, dst, ds)

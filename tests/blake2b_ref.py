"""Python reference of LcCommit<Blake2b, E>'s digests (lcpc-2d/src/lib.rs:690-785, 955-982) on hashlib's BLAKE2b-512 (RFC 7693).

leaf[c] = BLAKE2b(0^64 || to_repr(comm[0][c]) || ... || to_repr(comm[n_rows - 1][c])); node = BLAKE2b(left || right);
hashes = the np2 leaf slots (slots n_cols .. np2 are 64 zero bytes) followed by every level of the tree, root last.
Output<Blake2b>::default() -- the leaf prefix and the padding slots -- is 64 zero bytes."""
import hashlib

import numpy as np

from sha3_ref import repr_bytes  # noqa: F401  (the oracle's bulk to_repr, shared)

DLEN = 64
ZERO = b"\0" * DLEN


def b2(b):
    return hashlib.blake2b(b).digest()


def leaf_from_ints(F, col_canon):
    """one leaf from canonical python ints, with pyref's Field.to_repr"""
    return b2(ZERO + b"".join(F.to_repr(v) for v in col_canon))


def leaves(oracle, fid, comm, n_rows, n_cols):
    """leaf digests of a row-major comm (n_rows * n_cols, L) in Montgomery form"""
    rep = repr_bytes(oracle, fid, comm).reshape(n_rows, n_cols, -1).transpose(1, 0, 2).reshape(n_cols, -1)
    rep = np.ascontiguousarray(rep)
    return [b2(ZERO + rep[c].tobytes()) for c in range(n_cols)]


def tree(leaf_digests):
    """the flat `hashes` array (2 np2 - 1 digests) over the leaves"""
    n = len(leaf_digests)
    np2 = 1
    while np2 < n:
        np2 *= 2
    level = list(leaf_digests) + [ZERO] * (np2 - n)
    out = list(level)
    while len(level) > 1:
        level = [b2(level[2 * i] + level[2 * i + 1]) for i in range(len(level) // 2)]
        out += level
    return out


def path(hashes, np2, col):
    """the sibling digests of column `col` from the leaves up (open_column, lib.rs:788-825)"""
    out, base, width = [], 0, np2
    while width > 1:
        out.append(hashes[base + (col ^ 1)])
        base += width
        width //= 2
        col //= 2
    return out


def fold(leaf, col, sibs):
    """verify_column_path (lib.rs:955-982) with BLAKE2b"""
    h = leaf
    for s in sibs:
        h = b2(h + s) if col % 2 == 0 else b2(s + h)
        col //= 2
    return h


def exact_last_block(L, n_rows):
    """True when the leaf message (8 + L n_rows words) fills its last 128-byte block exactly (L n_rows = 8 mod 16)"""
    return (8 + L * n_rows) % 16 == 0

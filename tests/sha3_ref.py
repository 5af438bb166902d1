"""Python reference of LcCommit<Sha3_256, E>'s digests (lcpc-2d/src/lib.rs:690-785, 955-982) on hashlib's FIPS 202 SHA3-256.

leaf[c] = SHA3-256(0^32 || to_repr(comm[0][c]) || ... || to_repr(comm[n_rows - 1][c])); node = SHA3-256(left || right);
hashes = the np2 leaf slots (slots n_cols .. np2 zero) followed by every level of the tree, root last."""
import hashlib

import numpy as np


def sha3(b):
    return hashlib.sha3_256(b).digest()


def leaf_from_ints(F, col_canon):
    """one leaf from canonical python ints, with pyref's Field.to_repr"""
    return sha3(b"\0" * 32 + b"".join(F.to_repr(v) for v in col_canon))


def repr_bytes(oracle, fid, mont):
    """(n, L) Montgomery limbs -> (n, 8 L) uint8 to_repr bytes, in bulk (the oracle's PrimeField::to_repr)"""
    mont = np.ascontiguousarray(mont, np.uint64)
    L = oracle.limbs(fid)
    n = mont.size // L
    out = np.zeros(n * 8 * L, np.uint8)
    oracle.lib().lo_f_to_repr(fid, oracle.ptr(mont), oracle.ptr(out), n)
    return out.reshape(n, 8 * L)


def leaves(oracle, fid, comm, n_rows, n_cols):
    """leaf digests of a row-major comm (n_rows * n_cols, L) in Montgomery form"""
    rep = repr_bytes(oracle, fid, comm).reshape(n_rows, n_cols, -1).transpose(1, 0, 2).reshape(n_cols, -1)
    rep = np.ascontiguousarray(rep)
    z = b"\0" * 32
    return [sha3(z + rep[c].tobytes()) for c in range(n_cols)]


def tree(leaf_digests):
    """the flat `hashes` array (2 np2 - 1 digests) over the leaves"""
    n = len(leaf_digests)
    np2 = 1
    while np2 < n:
        np2 *= 2
    level = list(leaf_digests) + [b"\0" * 32] * (np2 - n)
    out = list(level)
    while len(level) > 1:
        level = [sha3(level[2 * i] + level[2 * i + 1]) for i in range(len(level) // 2)]
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
    """verify_column_path (lib.rs:955-982) with SHA3-256"""
    h = leaf
    for s in sibs:
        h = sha3(h + s) if col % 2 == 0 else sha3(s + h)
        col //= 2
    return h

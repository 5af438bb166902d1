"""ctypes side of tests/native/k8_harness.cpp (lcpc_amd/lib/liblcpc_k8_harness.so, built by lcpc_amd/csrc/Makefile): the Merkle path
folds of the batched verify and the column check (K8b, launch_fold_paths_b3 / launch_chain_fold_paths of lcpc_amd/csrc/kernels.h) on
operands a test builds, and the case builder with its expectations: hashlib for SHA3-256, SHA-256 and BLAKE2b-512, and the Keccak-256
and BLAKE3 references of the digest suites (tests/digest_ref.py ref_digest).  Errors as in tests/harness_kit.py."""
import ctypes as C
import random

import numpy as np

import digest_more  # noqa: F401  (teaches digest_ref.ref_digest Keccak-256 and SHA-256)
import digest_ref as DR
import harness_kit as K
from harness_kit import BadArgs, HipError, check as _check, ptr as _ptr  # noqa: F401

LIB_PATH = K.lib_path("k8")
HIP_SUCCESS, HIP_ERROR_INVALID_VALUE = 0, 1
PATH_BIT = 4
DIGESTS = ["blake3", "sha3_256", "keccak256", "sha256", "blake2b"]      # the harness's digest numbers
LAYOUTS = ["level", "column"]
POISON = 0xA5

_vp, _u64, _u32, _i32 = C.c_void_p, C.c_uint64, C.c_uint32, C.c_int
SYMBOLS = {
    "k8h_device_count": [],
    "k8h_fold_paths": [_i32, _vp, _u64, _u64, _vp, _vp, _u64, _u64, _u64, _u64, _vp, _vp, _u64, _u64, _u32, _u32, _u32],
    "k8h_refusal": [_i32, _u32, _u32, _u32, _u32],
}


def lib():
    return K.load("k8", SYMBOLS)


# ---- the reference -------------------------------------------------------------------------------------------------------------

_digest, _nodes, _trees = {}, {}, {}


def digest(name):
    """the reference D of `name` (BLAKE3 on the C oracle when it is built, as the digest suites run it)"""
    if name not in _digest:
        try:
            import oracle_lib as O
            O.lib()
        except Exception:
            O = None
        _digest[name] = DR.ref_digest(name, O)
    return _digest[name]


def node(name, left, right):
    """D(left || right), remembered: the lanes of a case fold the same tree again and again"""
    key = (name, left, right)
    if key not in _nodes:
        _nodes[key] = digest(name)(left + right)
    return _nodes[key]


def fold(name, leaf, col, sibs):
    """verify_column_path (lib.rs:955-982): the digest the path leads to"""
    h = leaf
    for s in sibs:
        h = node(name, h, s) if col % 2 == 0 else node(name, s, h)
        col >>= 1
    return h


def tree(name, leaves):
    """the flat `hashes` array (2 np2 - 1 digests) over the leaves, the slots behind the last leaf zero (merkleize, lib.rs:690-704)"""
    np2 = 1
    while np2 < len(leaves):
        np2 *= 2
    hashes = list(leaves) + [bytes(len(leaves[0]))] * (np2 - len(leaves))
    ins, width = 0, np2
    while width > 1:
        hashes += [node(name, hashes[ins + 2 * i], hashes[ins + 2 * i + 1]) for i in range(width // 2)]
        ins, width = ins + width, width // 2
    return hashes, np2


def path(hashes, np2, col):
    """the sibling digests of column `col` from the leaves up (open_column, lib.rs:788-825)"""
    out, base, width = [], 0, np2
    while width > 1:
        out.append(hashes[base + (col ^ 1)])
        base, width, col = base + width, width // 2, col >> 1
    return out


def random_tree(name, depth, seed):
    """a tree over 2^depth random leaf digests, built once per (digest, depth, seed)"""
    key = (name, depth, seed)
    if key not in _trees:
        rng = random.Random("%s/%d/%d" % key)
        dl = DR.DLEN[name]
        _trees[key] = tree(name, [rng.getrandbits(8 * dl).to_bytes(dl, "little") for _ in range(1 << depth)])
    return _trees[key]


def column_numbers(depth, n_open):
    """0, 2^depth - 1, alternating bits both ways, a number drawn twice, and random ones"""
    top = (1 << depth) - 1
    alt = int("01" * 32, 2) & top
    fixed = [0, top, alt, top ^ alt, top // 3, top // 3]
    rng = random.Random(depth * 1000 + n_open)
    out = (fixed + [rng.randrange(top + 1) for _ in range(n_open)])[:n_open]
    if n_open >= 2:
        out[-1] = out[0] if n_open < 5 else out[4]           # one number drawn twice, whatever n_open cut off
    return out


class Case:
    """One launch of K8b.  Member m has a tree of 2^depth random leaves; its opened column k is the leaf drawn[m][k] with that leaf's
    path, so a number drawn twice opens the same leaf twice, as in a proof.  layout: "level" = siblings [lvl][column] (the batched
    verify), "column" = [column][lvl] (the open-columns layout).  gap: words of poison behind every member's leaves, siblings and status
    words (a multiple of 4).  Faults are planted into the operands; expected() folds what is there."""

    def __init__(self, name, depth, drawn, layout="level", gap=0, seed=1):
        assert layout in LAYOUTS and gap % 4 == 0
        self.name, self.depth, self.layout, self.gap = name, depth, layout, gap
        self.dl = DR.DLEN[name]
        self.drawn = [list(d) for d in drawn]
        self.n_batch, self.n_open = len(self.drawn), len(self.drawn[0])
        assert all(len(d) == self.n_open and all(0 <= cn < (1 << depth) for cn in d) for d in self.drawn)
        self.leaves, self.sibs, self.roots = [], [], []
        for m in range(self.n_batch):
            hashes, np2 = random_tree(name, depth, seed * 100 + m)
            self.leaves.append([hashes[cn] for cn in self.drawn[m]])
            self.sibs.append([path(hashes, np2, cn) for cn in self.drawn[m]])
            self.roots.append(hashes[-1])

    # ---- faults: each must set the path bit of exactly the lanes it reaches ----
    @staticmethod
    def _flip(b, bit):
        x = bytearray(b)
        x[(bit // 8) % len(x)] ^= 1 << (bit % 8)
        return bytes(x)

    def flip_sibling(self, m, k, lvl, bit=0):
        self.sibs[m][k][lvl] = self._flip(self.sibs[m][k][lvl], bit)

    def flip_leaf(self, m, k, bit=0):
        self.leaves[m][k] = self._flip(self.leaves[m][k], bit)

    def flip_root(self, m, bit=0):
        self.roots[m] = self._flip(self.roots[m], bit)

    def swap_siblings(self, m, k, a, b):
        s = self.sibs[m][k]
        s[a], s[b] = s[b], s[a]

    def expected(self):
        """status bits K8b sets, [m][k], by the reference digest"""
        out = np.zeros((self.n_batch, self.n_open), np.uint32)
        for m in range(self.n_batch):
            for k, cn in enumerate(self.drawn[m]):
                if fold(self.name, self.leaves[m][k], cn, self.sibs[m][k]) != self.roots[m]:
                    out[m, k] = PATH_BIT
        return out

    def strides(self):
        """(leaves, sib_member, sib_col, sib_lvl, status) in 32-bit words"""
        dw = self.dl // 4
        sib_col, sib_lvl = (dw, self.n_open * dw) if self.layout == "level" else (self.depth * dw, dw)
        return self.n_open * dw + self.gap, self.n_open * self.depth * dw + self.gap, sib_col, sib_lvl, self.n_open + self.gap

    def arrays(self, prefill=0):
        """(leaves (n_batch, stride) u32, drawn (n_batch, n_open) u64, sibs (n_batch, stride) u32, roots (n_batch, DW) u32,
        status (n_batch, stride) u32); everything no lane owns is poison"""
        dw = self.dl // 4
        ls, sm, sc, sl, ss = self.strides()
        poison = np.uint32(POISON * 0x01010101)
        leaves = np.full((self.n_batch, ls), poison, np.uint32)
        sibs = np.full((self.n_batch, max(sm, 4)), poison, np.uint32)
        status = np.full((self.n_batch, ss), poison, np.uint32)
        w = lambda b: np.frombuffer(b, np.uint32)
        prefill = np.broadcast_to(np.asarray(prefill, np.uint32), (self.n_batch, self.n_open))
        for m in range(self.n_batch):
            for k in range(self.n_open):
                leaves[m, k * dw:(k + 1) * dw] = w(self.leaves[m][k])
                for lvl in range(self.depth):
                    o = k * sc + lvl * sl
                    sibs[m, o:o + dw] = w(self.sibs[m][k][lvl])
            status[m, :self.n_open] = prefill[m]
        roots = np.stack([w(r) for r in self.roots]).astype(np.uint32)
        return leaves, np.array(self.drawn, np.uint64).reshape(self.n_batch, self.n_open), sibs, roots, status

    def run(self, prefill=0):
        """K8b on the device: the status words (n_batch, n_open) uint32 after the launch; prefill: a number or an (n_batch, n_open)
        array they hold before it.  The poison behind every member's status words must come back untouched"""
        leaves, drawn, sibs, roots, status = self.arrays(prefill)
        ls, sm, sc, sl, ss = self.strides()
        before = status.copy()
        _check("k8h_fold_paths", lib().k8h_fold_paths(DIGESTS.index(self.name), _ptr(leaves), leaves.size, ls, _ptr(drawn), _ptr(sibs), sibs.size,
                                                      sibs.shape[1], sc, sl, _ptr(roots), _ptr(status), status.size, ss, self.n_open,
                                                      self.depth, self.n_batch))
        assert np.array_equal(status[:, self.n_open:], before[:, self.n_open:]), "status words no lane owns were written"
        return status[:, :self.n_open].copy()


def refusal(name, n_batch, n_open, depth, null_mask=0):
    """the hipError_t of the launcher on a job it must settle before any launch (null or never-read buffers; no device is touched);
    BadArgs when the job is one a correct launcher would launch.  null_mask: bit 0 leaves, 1 drawn, 2 sibs, 3 roots, 4 status"""
    rc = lib().k8h_refusal(DIGESTS.index(name), n_batch, n_open, depth, null_mask)
    if rc == -1:
        raise BadArgs("k8h_refusal")
    return rc

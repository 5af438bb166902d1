"""ctypes side of tests/native/k5_harness.cpp (lcpc_amd/lib/liblcpc_k5_harness.so, built by lcpc_amd/csrc/Makefile): the prover's kernels
(K5 / K6 of lcpc_amd/csrc/kernels.h: collapse in both forms, to_r29, the split sum, to_mont / to_canon, the column and path gathers in
both forms, assemble_columns) on operands a test builds, and the case builders with their Python-int expectations.  Elements cross as
uint64 arrays of stored (Montgomery) limbs, last axis L.  Errors as in tests/harness_kit.py.

Every builder lays its inputs out with POISON (all-ones limbs, not a reduced element) in every gap and its outputs pre-filled with
SENTINEL, and gives the whole expected output array: what the kernel must write, and SENTINEL everywhere else.  The members of a batch
carry distinct data and sit in memory in an order unlike their batch order, so a wrong member offset shows.  `fault` makes an
expectation wrong in a named way ("swap": members 0 and 1 exchanged; "no_j0": the collapse reads column j - j0; "no_slice": the second
slice of a column gather reads the first slice's column numbers); tests/test_k5_cases.py holds every batched case to changing under it."""
import ctypes as C
import random
from operator import mul

import numpy as np

from common import FIELD_L, field_p, maxc, maxt, to_int, to_limbs  # noqa: F401
import harness_kit as K
from harness_kit import BadArgs, HipError, check as _check, ptr as _ptr  # noqa: F401
from k2_harness import NL  # noqa: F401

LIB_PATH = K.lib_path("k5")
HIP_SUCCESS, HIP_ERROR_INVALID_VALUE = 0, 1
POISON = (1 << 64) - 1                  # all-ones limbs in every gap of an input: must never be read
SENTINEL = 0x5A5A5A5A5A5A5A5A           # what every output holds before the launch
SLICE = 32768                           # launch_gather_columns(_batch): opened columns per launch
GAP = 3                                 # elements (digests) of poison in front of every member

_vp, _u64, _u32, _i32 = C.c_void_p, C.c_uint64, C.c_uint32, C.c_int
SYMBOLS = {
    "k5h_device_count": [],
    "k5h_collapse": [_i32, _vp, _u64, _vp, _vp, _vp, _u64, _u64, _u64, _u32, _u32, _u64, _u64, _u64, _u32, _i32, _i32],
    "k5h_to_r29": [_vp, _u64, _vp, _u64],
    "k5h_field_sum": [_i32, _vp, _u64, _u32, _u64, _u32, _i32],
    "k5h_convert": [_i32, _i32, _vp, _u64, _vp, _vp, _u64, _i32],
    "k5h_gather_columns": [_i32, _vp, _u64, _vp, _vp, _vp, _vp, _u64, _u64, _vp, _u32, _vp, _vp, _u64, _u32, _i32],
    "k5h_gather_paths": [_vp, _u64, _vp, _u64, _u32, _vp, _u32, _vp, _u64, _u32, _u32, _i32],
    "k5h_assemble_columns": [_i32, _vp, _u64, _vp, _u32, _u32, _u64, _vp, _u64],
    "k5h_refuse_collapse": [_i32, _u64, _u32, _u32, _u64, _u64, _i32, _u32, _i32],
    "k5h_refuse_field_sum": [_i32, _u32, _u64, _i32, _u32],
    "k5h_refuse_gather_columns": [_i32, _u64, _u32, _i32, _u32],
    "k5h_refuse_gather_paths": [_u32, _u32, _u32, _i32, _u32],
    "k5h_refuse_convert": [_i32, _i32, _u64],
    "k5h_refuse_assemble_columns": [_i32, _u32, _u64],
}


def lib():
    return K.load("k5", SYMBOLS)


def pack(vals, L):
    """to_limbs for many values: python ints -> (n, L) uint64 limbs"""
    vals = list(vals)
    if not vals:
        return np.zeros((0, L), np.uint64)
    return np.frombuffer(b"".join(v.to_bytes(8 * L, "little") for v in vals), np.uint64).reshape(-1, L).copy()


def mont_r(fid):
    return 1 << (64 * FIELD_L[fid])


def r2_limbs(fid):
    return to_limbs([mont_r(fid) ** 2 % field_p(fid)], FIELD_L[fid])


def positions(n):
    """memory position of member m: a permutation unlike the batch order for n >= 2"""
    pos = [(2 * m + 1) % n for m in range(n)] if n % 2 else [n - 1 - m for m in range(n)]
    assert sorted(pos) == list(range(n))
    return pos


def _swapped(m, fault):
    return {0: 1, 1: 0}.get(m, m) if fault == "swap" else m


def _distinct(blocks):
    """the members' data differ pairwise"""
    keys = [repr(b) for b in blocks]
    assert len(set(keys)) == len(keys)


# ---- K5 / K5b: collapse -------------------------------------------------------------------------------------------------------------
class CollapseData:
    """coefficients [member][row][column], two tensors [member][tensor][row] as stored integers, and the exact dot products.
    Rows: MAXC, p - 1 where r % 7 == 4, uniformly random where r % 4 == (m + 2) % 4 and at r == m % n_rows (so every member has one).
    Tensor entries: MAXT, p - 1 where r % 3 == 1, random where r % 5 == (m + t + 1) % 5."""

    def __init__(self, fid, n_rows, n_per_row, n_members=1, seed=1):
        self.fid, self.L, self.p = fid, FIELD_L[fid], field_p(fid)
        self.n_rows, self.n_per_row, self.n_members = n_rows, n_per_row, n_members
        rng, p = random.Random(seed * 1000003 + fid), self.p
        self.coeffs, self.tensors = [], []
        for m in range(n_members):
            rows = []
            for r in range(n_rows):
                if r == m % n_rows or r % 4 == (m + 2) % 4:
                    rows.append([rng.randrange(p) for _ in range(n_per_row)])
                else:
                    rows.append([p - 1 if r % 7 == 4 else maxc(fid)] * n_per_row)
            self.coeffs.append(rows)
            self.tensors.append([[rng.randrange(p) if r % 5 == (m + t + 1) % 5 else p - 1 if r % 3 == 1 else maxt(fid) for r in range(n_rows)]
                                 for t in range(2)])
        _distinct(self.coeffs)
        _distinct(self.tensors)
        self._cols = [list(zip(*rows)) for rows in self.coeffs]        # [member][column] -> the column's rows
        self._dots, self._packed = {}, {}

    def packed(self, m):
        """member m's coefficients as (n_rows * n_per_row, L) limbs"""
        if m not in self._packed:
            self._packed[m] = pack((v for row in self.coeffs[m] for v in row), self.L)
        return self._packed[m]

    def dots(self, m_coeffs, m_tensors, t, r0, r1):
        """[j] -> sum_{r0 <= r < r1} t_r c_rj / R mod p on the stored values: what a split holding those rows must write"""
        key = (m_coeffs, m_tensors, t, r0, r1)
        if key not in self._dots:
            rinv = pow(mont_r(self.fid), -1, self.p)
            tv = self.tensors[m_tensors][t][r0:r1]
            self._dots[key] = [sum(map(mul, tv, col[r0:r1])) * rinv % self.p for col in self._cols[m_coeffs]]
        return self._dots[key]


class CollapseCase:
    """One launch of K5 (n_batch None: the single form) or K5b.  j0, j1, out_stride go to the launcher as given (0: its defaults)."""

    def __init__(self, data, n_tensors, n_splits, n_batch=None, j0=0, j1=0, out_stride=0, limb=None, tail=5):
        self.d, self.fid, self.L = data, data.fid, data.L
        self.batch, self.n_batch = n_batch is not None, n_batch or 1
        assert self.n_batch == data.n_members
        self.n_tensors, self.n_splits, self.j0, self.j1, self.out_stride = n_tensors, n_splits, j0, j1, out_stride
        self.limb = (self.fid == 3) if limb is None else limb
        self.ej0, self.ej1 = (j0, j1) if j1 else (0, data.n_per_row)
        self.es = out_stride or data.n_per_row
        self.len = self.ej1 - self.ej0
        self.pos = positions(self.n_batch)
        self.block = data.n_rows * data.n_per_row
        self.off = [GAP + q * (self.block + GAP) for q in self.pos]
        self.coeffs_elems = self.n_batch * (self.block + GAP) + GAP
        self.out_elems = self.n_batch * n_splits * n_tensors * self.es + tail

    def splits(self):
        """[(r0, r1)] per split; r0 >= r1: the split holds no row"""
        n_rows = self.d.n_rows
        per = -(-n_rows // self.n_splits)
        return [(min(z * per, n_rows), min(z * per + per, n_rows)) for z in range(self.n_splits)]

    def expected(self, fault=None):
        """the whole out array: (out_elems, L) uint64"""
        out = np.full((self.out_elems, self.L), SENTINEL, np.uint64)
        shift = self.ej0 if fault == "no_j0" else 0
        for m in range(self.n_batch):
            for z, (r0, r1) in enumerate(self.splits()):
                for t in range(self.n_tensors):
                    row = self.d.dots(_swapped(m, fault), m, t, r0, r1) if r0 < r1 else [0] * self.d.n_per_row
                    at = ((m * self.n_splits + z) * self.n_tensors + t) * self.es
                    out[at:at + self.len] = pack(row[self.ej0 - shift:self.ej1 - shift], self.L)
        return out

    def arrays(self):
        """(coeffs (coeffs_elems, L), coeff_off (n_batch,), tensors (n_batch, n_tensors, n_rows, L)) uint64"""
        coeffs = np.full((self.coeffs_elems, self.L), POISON, np.uint64)
        for m in range(self.n_batch):
            coeffs[self.off[m]:self.off[m] + self.block] = self.d.packed(m)
        tensors = np.stack([np.stack([pack(self.d.tensors[m][t], self.L) for t in range(self.n_tensors)]) for m in range(self.n_batch)])
        return coeffs, np.array(self.off, np.uint64), tensors

    def run(self):
        coeffs, off, tensors = self.arrays()
        out = np.full((self.out_elems, self.L), SENTINEL, np.uint64)
        _check("k5h_collapse", lib().k5h_collapse(NL[self.fid], _ptr(coeffs), self.coeffs_elems, _ptr(off), _ptr(tensors), _ptr(out), self.out_elems,
                                                  self.d.n_rows, self.d.n_per_row, self.n_tensors, self.n_splits, self.j0, self.j1,
                                                  self.out_stride, self.n_batch, int(self.batch), int(self.limb)))
        return out


N_PER_ROW = 300                                   # one ragged 256-lane block
RANGES = [(0, 0, 0), (37, 293, 300), (37, 293, 0), (37, 293, 256)]      # (j0, j1, out_stride): defaults; a range at the row stride, given
#                                                                         and by default; the same range packed (out_stride == len)
ROWS_PER_SPLIT = {0: [7, 8, 9], 1: [7, 8, 9], 2: [7, 8, 9], 3: [6, 7, 8, 9, 60, 61, 121]}


def rows_for(rows_per, n_splits):
    """a row count whose ceil(n_rows / n_splits) is rows_per, the last split one row short when there is more than one"""
    n = rows_per * n_splits - (n_splits > 1)
    assert -(-n // n_splits) == rows_per
    return n


def collapse_single_shapes(fid, n_splits):
    """(n_rows, n_splits) of the single-form tests: 64 splits meet 61 rows (one row each, three with none)"""
    return [(61, 64)] if n_splits == 64 else [(rows_for(rp, n_splits), n_splits) for rp in ROWS_PER_SPLIT[fid]]


def collapse_batch_shapes(fid):
    """(n_rows, n_splits, n_batch) of the batch-form tests"""
    s = [(rows_for(7, 1), 1, 1), (rows_for(8, 2), 2, 3), (rows_for(9, 3), 3, 5), (61, 64, 3)]
    if fid == 3:
        s += [(rows_for(6, 3), 3, 3), (rows_for(60, 2), 2, 3), (rows_for(61, 1), 1, 5), (rows_for(121, 2), 2, 3)]
    return s


def collapse_views(data, n_splits, n_batch=None):
    """every launch the tests make on one set of operands: 1 and 2 tensors, every column range; Ft255 with and without the limb form"""
    return [CollapseCase(data, nt, n_splits, n_batch, j0, j1, st, limb)
            for nt in (1, 2) for j0, j1, st in RANGES for limb in ((True, False) if data.fid == 3 else (False,))]


# ---- to_r29, to_mont, to_canon --------------------------------------------------------------------------------------------------------
def r29_expected(vals, n_entries):
    """(n_entries, 12) uint32: nine 29-bit limbs of 32 t mod p and three zero words per value, SENTINEL behind them"""
    p = field_p(3)
    out = np.full((n_entries, 12), SENTINEL & 0xFFFFFFFF, np.uint32)
    for i, t in enumerate(vals):
        x = 32 * t % p
        out[i] = [(x >> (29 * k)) & ((1 << 29) - 1) for k in range(9)] + [0, 0, 0]
    return out


def to_r29(vals, tail=3):
    inp = pack(vals, 4)
    out = np.full((len(vals) + tail, 12), SENTINEL & 0xFFFFFFFF, np.uint32)
    _check("k5h_to_r29", lib().k5h_to_r29(_ptr(inp), len(vals), _ptr(out), len(out)))
    return out


def convert_expected(fid, vals, to_mont, tail=3):
    p, R = field_p(fid), mont_r(fid)
    f = R if to_mont else pow(R, -1, p)
    return np.concatenate([pack([v * f % p for v in vals], FIELD_L[fid]), np.full((tail, FIELD_L[fid]), SENTINEL, np.uint64)])


def convert(fid, vals, to_mont, in_place, tail=3):
    L = FIELD_L[fid]
    inp = pack(vals, L)
    out = np.full((len(vals) + tail, L), SENTINEL, np.uint64)
    if in_place:
        out[:len(vals)] = inp
    r2 = r2_limbs(fid)
    _check("k5h_convert", lib().k5h_convert(NL[fid], int(to_mont), None if in_place else _ptr(inp), len(vals), _ptr(r2) if to_mont else None,
                                            _ptr(out), len(out), int(in_place)))
    return out


# ---- the split sum ----------------------------------------------------------------------------------------------------------------------
class SumCase:
    """parts [member][part][element]; fill "max": every part p - 1 (a batch member m keeps its part m % n_parts random, so that
    members differ); "random".  The buffer: the parts, the sums right behind them, `tail` more elements."""

    def __init__(self, fid, n_parts, n_elems, n_batch=None, fill="random", seed=1, tail=4):
        self.fid, self.L, self.p = fid, FIELD_L[fid], field_p(fid)
        self.batch, self.n_batch, self.n_parts, self.n_elems, self.tail = n_batch is not None, n_batch or 1, n_parts, n_elems, tail
        rng, p = random.Random(seed), self.p
        self.parts = [[[rng.randrange(p) if fill == "random" or (self.batch and q == m % n_parts) else p - 1 for _ in range(n_elems)]
                       for q in range(n_parts)] for m in range(self.n_batch)]
        _distinct(self.parts)
        self.n_in = self.n_batch * n_parts * n_elems
        self.buf_elems = self.n_in + self.n_batch * n_elems + tail

    def buffer(self):
        buf = np.full((self.buf_elems, self.L), SENTINEL, np.uint64)
        buf[:self.n_in] = pack((v for mem in self.parts for part in mem for v in part), self.L)
        return buf

    def expected(self, fault=None):
        buf = self.buffer()
        sums = [sum(col) % self.p for m in range(self.n_batch) for col in zip(*self.parts[_swapped(m, fault)])]
        buf[self.n_in:self.n_in + len(sums)] = pack(sums, self.L)
        return buf

    def run(self):
        buf = self.buffer()
        _check("k5h_field_sum", lib().k5h_field_sum(NL[self.fid], _ptr(buf), self.buf_elems, self.n_parts, self.n_elems, self.n_batch, int(self.batch)))
        return buf


# ---- K6 / K6b: the column gather --------------------------------------------------------------------------------------------------------
class GatherCase:
    """comm[member][row][column] random stored integers; layouts[m] "row" (row-major: strides n_cols, 1) or "pos" (position-major: 1,
    n_rows); canon[m]: the member's values are canonical and come out multiplied by R; cols[m] its opened column numbers."""

    def __init__(self, fid, n_rows, n_cols, cols, layouts, canon, batch=True, seed=1, tail=4):
        self.fid, self.L, self.p = fid, FIELD_L[fid], field_p(fid)
        self.n_rows, self.n_cols, self.cols, self.layouts, self.canon, self.batch, self.tail = n_rows, n_cols, cols, layouts, canon, batch, tail
        self.n_batch, self.n_open = len(cols), len(cols[0])
        assert all(len(c) == self.n_open for c in cols) and len(layouts) == len(canon) == self.n_batch and (batch or self.n_batch == 1)
        rng = random.Random(seed)
        self.comm = [[[rng.randrange(self.p) for _ in range(n_cols)] for _ in range(n_rows)] for _ in range(self.n_batch)]
        _distinct(self.comm)
        self.pos = positions(self.n_batch)
        self.block = n_rows * n_cols
        self.off = [GAP + q * (self.block + GAP) for q in self.pos]
        self.comm_elems = self.n_batch * (self.block + GAP) + GAP
        self.vals_elems = self.n_batch * self.n_open * n_rows + tail

    def strides(self, m):
        return (self.n_cols, 1) if self.layouts[m] == "row" else (1, self.n_rows)

    def arrays(self):
        comm = np.full((self.comm_elems, self.L), POISON, np.uint64)
        for m in range(self.n_batch):
            a = pack((v for row in self.comm[m] for v in row), self.L).reshape(self.n_rows, self.n_cols, self.L)
            if self.layouts[m] == "pos":
                a = a.transpose(1, 0, 2)
            comm[self.off[m]:self.off[m] + self.block] = a.reshape(self.block, self.L)
        rs = np.array([self.strides(m)[0] for m in range(self.n_batch)], np.uint64)
        cs = np.array([self.strides(m)[1] for m in range(self.n_batch)], np.uint64)
        return (comm, np.array(self.off, np.uint64), rs, cs, np.array(self.canon, np.uint32),
                np.array(self.cols, np.uint64).reshape(self.n_batch, self.n_open))

    def expected(self, fault=None):
        """the whole vals array, (vals_elems, L): vals[m][k][r] = comm_m[r][cols[m][k]]"""
        R, p = mont_r(self.fid), self.p
        out = np.full((self.vals_elems, self.L), SENTINEL, np.uint64)
        for m in range(self.n_batch):
            s = _swapped(m, fault)
            f = R if self.canon[s] else 1
            a = pack((v * f % p for row in self.comm[s] for v in row), self.L).reshape(self.n_rows, self.n_cols, self.L)
            ks = [c if fault != "no_slice" or k < SLICE else self.cols[m][k - SLICE] for k, c in enumerate(self.cols[m])]
            at = m * self.n_open * self.n_rows
            out[at:at + self.n_open * self.n_rows] = a[:, ks].transpose(1, 0, 2).reshape(-1, self.L)
        return out

    def run(self):
        comm, off, rs, cs, canon, cols = self.arrays()
        vals = np.full((self.vals_elems, self.L), SENTINEL, np.uint64)
        r2 = r2_limbs(self.fid) if any(self.canon) else None
        _check("k5h_gather_columns", lib().k5h_gather_columns(NL[self.fid], _ptr(comm), self.comm_elems, _ptr(off), _ptr(rs), _ptr(cs), _ptr(canon),
                                                              self.n_rows, self.n_cols, _ptr(cols), self.n_open, _ptr(r2), _ptr(vals),
                                                              self.vals_elems, self.n_batch, int(self.batch)))
        return vals


def col_list(n_open, n_cols, m=0):
    """n_open column numbers that hold 0, n_cols - 1 and duplicates where there is room, differ from member to member, and differ
    between the slices: entry k + SLICE is never entry k (members 0 .. n_cols - 2)"""
    out = [(5 * k + 3 * m) % n_cols for k in range(min(n_open, SLICE))]
    for k, v in enumerate([0, n_cols - 1, n_cols - 1, 0][:max(0, n_open - 1)]):
        out[k + 1] = v
    for k in range(SLICE, n_open):
        out.append((out[k - SLICE] + 1 + m) % n_cols)
    return out


def gather_batch_cases(fid):
    """{id: factory} of the batch-form gather cases: row counts 1, 255, 257; the grid-stride loop behind 64 row blocks; mixed members;
    the second slice"""
    mixed_l, mixed_c = ["row", "pos", "row", "pos", "pos"], [False, True, True, False, True]
    cases = {}
    for n_rows in (1, 255, 257):
        for nb in (1, 3, 5):
            cases["rows%d-batch%d-mixed" % (n_rows, nb)] = (
                lambda n_rows=n_rows, nb=nb: GatherCase(fid, n_rows, 6, [col_list(7, 6, m) for m in range(nb)], mixed_l[:nb], mixed_c[:nb], seed=n_rows + nb))
    cases["rows257-batch3-row-major-montgomery"] = lambda: GatherCase(fid, 257, 6, [col_list(7, 6, m) for m in range(3)], ["row"] * 3, [False] * 3, seed=2)
    cases["rows257-batch3-position-major-canonical"] = lambda: GatherCase(fid, 257, 6, [col_list(7, 6, m) for m in range(3)], ["pos"] * 3, [True] * 3, seed=3)
    cases["rows16641-batch3-grid-stride"] = lambda: GatherCase(fid, 16384 + 257, 3, [[2, 0], [1, 1], [0, 2]], ["pos", "row", "pos"], [True, False, False], seed=4)
    cases["two-slices-batch2"] = lambda: GatherCase(fid, 2, 7, [col_list(SLICE + 3, 7, m) for m in range(2)], ["row", "pos"], [True, False], seed=5)
    return cases


# ---- the path gather ----------------------------------------------------------------------------------------------------------------------
class PathsCase:
    """hashes[member]: 2 np2 - 1 random digests of dw words; paths[m][k][lvl] = the sibling of column cols[m][k]'s ancestor at level lvl"""

    def __init__(self, dw, np2, path_len, cols, batch=True, seed=1, tail=2):
        self.dw, self.np2, self.path_len, self.cols, self.batch = dw, np2, path_len, cols, batch
        self.n_batch, self.n_open = len(cols), len(cols[0])
        assert all(len(c) == self.n_open for c in cols) and (batch or self.n_batch == 1)
        self.n_dig = 2 * np2 - 1
        self.hashes = [np.random.RandomState(seed * 100 + m).randint(0, 1 << 32, (self.n_dig, dw), np.uint64).astype(np.uint32)
                       for m in range(self.n_batch)]
        _distinct([h.tobytes() for h in self.hashes])
        self.pos = positions(self.n_batch)
        self.off = [GAP + q * (self.n_dig + GAP) for q in self.pos]
        self.hashes_digests = self.n_batch * (self.n_dig + GAP) + GAP
        self.paths_digests = self.n_batch * self.n_open * path_len + tail

    def arrays(self):
        h = np.full((self.hashes_digests, self.dw), POISON & 0xFFFFFFFF, np.uint32)
        for m in range(self.n_batch):
            h[self.off[m]:self.off[m] + self.n_dig] = self.hashes[m]
        return h, np.array(self.off, np.uint64), np.array(self.cols, np.uint64).reshape(self.n_batch, self.n_open)

    def expected(self, fault=None):
        out = np.full((self.paths_digests, self.dw), SENTINEL & 0xFFFFFFFF, np.uint32)
        base = [sum(self.np2 >> i for i in range(lvl)) for lvl in range(self.path_len)]       # first node of level lvl
        for m in range(self.n_batch):
            src = self.hashes[_swapped(m, fault)]
            for k, c in enumerate(self.cols[m]):
                for lvl in range(self.path_len):
                    out[(m * self.n_open + k) * self.path_len + lvl] = src[base[lvl] + ((c >> lvl) ^ 1)]
        return out

    def run(self):
        h, off, cols = self.arrays()
        paths = np.full((self.paths_digests, self.dw), SENTINEL & 0xFFFFFFFF, np.uint32)
        _check("k5h_gather_paths", lib().k5h_gather_paths(_ptr(h), self.hashes_digests, _ptr(off), self.np2, self.path_len, _ptr(cols), self.n_open,
                                                          _ptr(paths), self.paths_digests, self.dw, self.n_batch, int(self.batch)))
        return paths


def path_cols(n_open, np2, m):
    """first, last and three more leaves, another choice for every member"""
    return [0, np2 - 1, (np2 // 2 + m) % np2, (3 * m + 1) % np2, (np2 // 3 + 2 * m) % np2][:n_open] if n_open > 1 else [(np2 - 1 - m) % np2]


def paths_batch_cases(dw):
    cases = {}
    for np2 in (2, 64, 4096):
        depth = np2.bit_length() - 1
        for path_len in (depth, depth - 1):
            for nb in (1, 3):
                for n_open in (1, 5):
                    cases["np2_%d-len%d-batch%d-open%d" % (np2, path_len, nb, n_open)] = (
                        lambda np2=np2, path_len=path_len, nb=nb, n_open=n_open: PathsCase(
                            dw, np2, path_len, [path_cols(n_open, np2, m) for m in range(nb)], seed=np2 + nb))
    return cases


# ---- assemble_columns -------------------------------------------------------------------------------------------------------------------------
class AssembleCase:
    """rank g's block holds its rows rb[g] .. rb[g + 1] of the n opened columns as [k][row]; out[k][r] over all rows.  slack: words of
    poison behind the largest rank's data in every block"""

    def __init__(self, fid, rb, n, slack=6, seed=1, tail=3):
        self.fid, self.L, self.p = fid, FIELD_L[fid], field_p(fid)
        self.rb, self.G, self.n, self.n_rows, self.tail = list(rb), len(rb) - 1, n, rb[-1], tail
        rng = random.Random(seed)
        self.data = [[[rng.randrange(self.p) for _ in range(rb[g + 1] - rb[g])] for _ in range(n)] for g in range(self.G)]
        self.block_words = max(n * (rb[g + 1] - rb[g]) for g in range(self.G)) * 2 * self.L + slack
        assert self.block_words % 2 == 0
        self.out_elems = n * self.n_rows + tail

    def recv(self):
        r = np.full((self.G, self.block_words // 2), POISON, np.uint64)
        for g in range(self.G):
            flat = pack((v for col in self.data[g] for v in col), self.L).reshape(-1)
            r[g, :len(flat)] = flat
        return r

    def expected(self):
        out = np.full((self.out_elems, self.L), SENTINEL, np.uint64)
        out[:self.n * self.n_rows] = pack((v for k in range(self.n) for g in range(self.G) for v in self.data[g][k]), self.L)
        return out

    def run(self):
        recv, rb = self.recv(), np.array(self.rb, np.uint64)
        out = np.full((self.out_elems, self.L), SENTINEL, np.uint64)
        _check("k5h_assemble_columns", lib().k5h_assemble_columns(NL[self.fid], _ptr(recv), self.block_words, _ptr(rb), self.G, self.n, self.n_rows,
                                                                  _ptr(out), self.out_elems))
        return out


# ---- the launchers' own refusals (null buffers; no device is touched).  BadArgs: the job is one a correct launcher would launch -------------
def _refusal(name, *args):
    rc = getattr(lib(), name)(*args)
    if rc == -1:
        raise BadArgs(name)
    return rc


def refuse_collapse(nl, n_per_row=300, n_tensors=1, n_splits=1, j0=0, j1=0, n_batch=None, limb=False):
    return _refusal("k5h_refuse_collapse", nl, n_per_row, n_tensors, n_splits, j0, j1, int(n_batch is not None), n_batch or 0, int(limb))


def refuse_field_sum(nl, n_parts, n_elems, n_batch=None):
    return _refusal("k5h_refuse_field_sum", nl, n_parts, n_elems, int(n_batch is not None), n_batch or 0)


def refuse_gather_columns(nl, n_rows, n_open, n_batch=None):
    return _refusal("k5h_refuse_gather_columns", nl, n_rows, n_open, int(n_batch is not None), n_batch or 0)


def refuse_gather_paths(digest_words, path_len, n_open, n_batch=None):
    return _refusal("k5h_refuse_gather_paths", digest_words, path_len, n_open, int(n_batch is not None), n_batch or 0)


def refuse_convert(nl, which, n):
    """which: "canon", "mont" or "r29" """
    return _refusal("k5h_refuse_convert", nl, {"canon": 0, "mont": 1, "r29": 2}[which], n)


def refuse_assemble_columns(nl, n, n_rows):
    return _refusal("k5h_refuse_assemble_columns", nl, n, n_rows)

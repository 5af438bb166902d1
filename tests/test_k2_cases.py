"""The case tables of tests/test_gpu_k2_kernels.py -- the Brakedown (K2) kernels called directly, on matrices and operands built here --
with the checks that need no GPU: that the tables reach every kernel instantiation and every term count the lazy-reduction bounds are
about (through launch_spmm_t's selection and spmv_kernel's lazy switch restated on thresholds READ from kernels.hip), that the
extreme operands are extreme in the limb model of test_lazy_bounds.py, and that the Python-int reference the GPU tests trust is the C
oracle's Brakedown encode on real generated matrices.  No GPU is needed, but the built tree is: test_harness_refuses_.. loads
lcpc_amd/lib/liblcpc_k2_harness.so (and with it the product library and the HIP runtime) to see it refuse bad indices before any
device call; tests/k2_harness.py says how to build it when it is missing.

Arithmetic, on STORED limbs (Montgomery form, R = 2^(64 L)): out = sum_k v_k x_col(k) / R mod p for the matrices, whichever path
multiplies (Wide<NL>: REDC by R; limb paths: the value is pre-scaled to v R' / R and the REDC is by R'), and Horner
out_k = sum_j in_j (k + 1)^j mod p for the Reed-Solomon base case (the point k + 1 is a plain integer, the stored form carries over)."""
import functools
import os
import random
import sys
from collections import namedtuple
from operator import mul

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import common as CM  # noqa: E402
import test_lazy_bounds as LB  # noqa: E402

BASE = [0, 1, 5, 6, 7, 59, 60, 61, 119, 120, 121, 181]        # terms per lane / slice: normalise (6), REDC chunk (60) and Wide (8) edges
VPATS = ("ext", "pm1", "alt", "rnd")                          # matrix-value pattern of an output
XPATS = ("ext", "pm1", "alt", "rnd", "ext/rnd", "words")      # operand pattern of a row (row r: XPATS[r % 6])
FT = {0: "ft63", 1: "ft127", 2: "ft191", 3: "ft255"}

# path: "spmv" (launch_spmv, row-major) or "spmm" (launch_spmm_t, position-major); limb: the limb form of the values is built and passed
# (False: vals29 = nullptr); alt: outputs go to out_alt
Case = namedtuple("Case", "path fid m n_rows limb n_in in_off out_off alt")


def _case(path, fid, m, n_rows, limb=None, n_in=509, in_off=3, gap=2, alt=False):
    limb = fid != 0 if limb is None else limb
    return Case(path, fid, m, n_rows, limb, n_in, in_off, in_off + n_in + gap, alt)


# Position-major: every row count of {24, 63, 64, 65, 101, 112, 113, 128, 130, 257}; m sits ON the selection thresholds (8192 is the
# first m of spmm_t_kernel, 8191 / 2049 the ends of sliced<2>, 2048 / 257 of sliced<4>, 256 the first of sliced<8>).
# Ft255 at m = 8192: n_rows % 64 = 1, 37, 48 run the packed-tail kernel beside spmm_t_kernel (65: one whole group + a tail of 1),
# 0 and 49 do not; 130 rows: the second 128-row workgroup has a wave with no row.
SPMM_CASES = [
    _case("spmm", 3, 8192, 65), _case("spmm", 3, 8192, 101, alt=True), _case("spmm", 3, 8192, 112), _case("spmm", 3, 8192, 64),
    _case("spmm", 3, 8192, 113), _case("spmm", 3, 8192, 128, in_off=0, gap=0), _case("spmm", 3, 8192, 24),
    _case("spmm", 0, 8192, 101), _case("spmm", 1, 8192, 65), _case("spmm", 1, 8192, 24, limb=False),
    _case("spmm", 2, 8192, 113), _case("spmm", 2, 8192, 63, limb=False, alt=True),
    _case("spmm", 3, 8191, 24), _case("spmm", 3, 2049, 130), _case("spmm", 0, 2049, 65), _case("spmm", 1, 2049, 63),
    _case("spmm", 2, 2049, 64, alt=True), _case("spmm", 1, 2049, 24, limb=False),
    _case("spmm", 3, 2048, 63), _case("spmm", 3, 257, 257, alt=True), _case("spmm", 0, 257, 130), _case("spmm", 1, 257, 128),
    _case("spmm", 2, 257, 101), _case("spmm", 2, 257, 24, limb=False), _case("spmm", 1, 2048, 24, limb=False),
    _case("spmm", 2, 2049, 24, limb=False),
    _case("spmm", 3, 256, 130), _case("spmm", 3, 100, 24, alt=True), _case("spmm", 0, 256, 257), _case("spmm", 1, 256, 130),
    _case("spmm", 2, 100, 257), _case("spmm", 1, 100, 64, limb=False), _case("spmm", 2, 256, 112, limb=False),
]
# Row-major: 1 and 23 rows.  Ft255 with the limb form: outputs of up to 60 * 8 = 480 terms stay lazy, longer ones take Wide<8>;
# without it every output takes Wide<8>.  The other fields have Wide<NL> only here.
SPMV_CASES = [
    _case("spmv", 3, 120, 1), _case("spmv", 3, 120, 23, alt=True), _case("spmv", 3, 120, 23, limb=False),
    _case("spmv", 0, 120, 23), _case("spmv", 0, 120, 1, alt=True), _case("spmv", 1, 120, 23, limb=False), _case("spmv", 2, 120, 23, limb=False),
    _case("spmv", 1, 120, 1, limb=False, in_off=0, gap=0),
]
CASES = SPMM_CASES + SPMV_CASES


def case_id(c):
    return "%s-%s-m%d-r%d%s%s%s" % (c.path, FT[c.fid], c.m, c.n_rows, "" if c.limb or c.fid == 0 else "-nolimb", "-alt" if c.alt else "",
                                    "-off0" if c.in_off == 0 else "")


# ---- which kernel, which arithmetic (kernels.hip launch_spmm_t / spmv_kernel / spmm_t_terms, restated) ---------------------------------
def select(c, th=None):
    """{kernel name: slices per output} for a case: the kernels its launch runs"""
    th = th or LB.k2_thresholds()
    nl = 2 * CM.FIELD_L[c.fid]
    if c.path == "spmv":
        assert c.n_rows < th["t_min_rows"]
        return {"spmv_kernel<%d,%d>" % (nl, th["spmv_sl"]): th["spmv_sl"]}
    assert c.n_rows >= th["t_min_rows"]
    assert c.fid != 3 or c.limb                                   # (the launcher refuses Ft255 without the limb form)
    if c.m >= th["opw_min_m"]:
        tail = c.n_rows % th["rows_per_group"]
        out = {}
        packed = c.fid == 3 and c.limb and 0 < tail <= th["tail_max"]
        if c.n_rows - (tail if packed else 0):
            out["spmm_t_kernel<%d,%d>" % (nl, th["opw"])] = 1
        if packed:
            out["spmm_t_tail_kernel"] = 1
        return out
    sl = th["sliced_sl"][-1]
    for above, s in zip(th["sliced_above"], th["sliced_sl"]):
        if c.m > above:
            sl = s
            break
    return {"spmm_t_sliced_kernel<%d,%d>" % (nl, sl): sl}


def arithmetic(c, length, th=None):
    """the accumulator an output of `length` terms goes through: "lazy29" (Ft255 limbs), "ln" (Ft127 / Ft191 limbs) or "wide" """
    th = th or LB.k2_thresholds()
    if c.path == "spmv":
        return "lazy29" if c.fid == 3 and c.limb and length <= th["spmv_lazy_terms"] * th["spmv_sl"] else "wide"
    return "wide" if not c.limb else "lazy29" if c.fid == 3 else "ln"


def lane_counts(c, length, th=None):
    """terms per lane / slice of an output of `length` terms, for every kernel of the case"""
    th = th or LB.k2_thresholds()
    out = {}
    for kern, sl in select(c, th).items():
        if c.path == "spmv":
            out[kern] = [len(range(s, length, sl)) for s in range(sl)]          # lane s: terms s, s + SL, ..
        else:
            out[kern] = [length * (s + 1) // sl - length * s // sl for s in range(sl)]
    return out


# ---- the matrices ----------------------------------------------------------------------------------------------------------------------
def special_lengths(c, th=None):
    th = th or LB.k2_thresholds()
    sl = max(select(c, th).values())
    if c.path == "spmv":
        lazy = th["spmv_lazy_terms"]
        # every lane at each BASE count; one lane more / fewer than the rest; the last lazy length, the first Wide<8> one; 8 * 6 +- 1
        return sorted({sl * b for b in BASE} | set(range(1, sl)) | {sl * lazy, sl * lazy + 1, sl * 6 - 1, sl * 6 + 1, sl * 59 + 1, sl * 61 - 1})
    if sl == 1:
        return list(BASE)
    return sorted({sl * b for b in BASE} | set(range(1, sl)) | {sl * 60 + 1, sl * 61 - 1, sl * 6 + 1, sl * 6 - 1})


def build_structure(c):
    """(rowptr, colidx, vpat) of the case's matrix, deterministic: every special length twice (values "ext", and one of the other
    patterns in turn) or once where m is small, spread over the outputs; an empty output first, last and in the middle; the rest 1 .. 3
    (m > 2048) or 1 .. 7 terms with the value patterns in turn.  Columns are random, except that term 0 of every fourth output hits
    input 0 and its last term input n_in - 1, and that every third output of >= 2 terms repeats its first column."""
    rnd = random.Random("%s %d %d" % (c.path, c.fid, c.m))
    sp = special_lengths(c)
    reps = 2 if c.m >= 2 * len(sp) + 3 else 1
    assert c.m >= reps * len(sp) + 3
    want = [(ln, "ext" if rep == 0 else VPATS[1 + i % 3]) for i, ln in enumerate(sp) for rep in range(reps) if ln]
    # every length that gives a lane / slice more than one REDC chunk also with "pm1" values: p - 1 on both sides is what makes the
    # REDC input largest (81 terms of (p - 1)^2 are the first count whose Ft255 REDC output passes 2p: test_broken_cadences_..)
    sl = max(select(c).values())
    want += [(ln, "pm1") for ln in sp if ln // sl > 60 and (ln, "pm1") not in want]
    assert c.m >= len(want) + 3
    length, vpat = [None] * c.m, [None] * c.m
    for o in (0, c.m // 2, c.m - 1):
        length[o], vpat[o] = 0, "ext"
    free = [o for o in range(c.m) if length[o] is None]
    step = len(free) // len(want)
    for i, (ln, vp) in enumerate(want):
        o = free[i * step + (step // 2 if step > 1 else 0)]
        length[o], vpat[o] = ln, vp
    hi = 3 if c.m > 2048 else 7
    for o in range(c.m):
        if length[o] is None:
            length[o], vpat[o] = rnd.randint(1, hi), VPATS[o % 4]
    rowptr = np.zeros(c.m + 1, np.int64)
    rowptr[1:] = np.cumsum(length)
    colidx = [rnd.randrange(c.n_in) for _ in range(int(rowptr[-1]))]
    for o in range(c.m):
        k0, k1 = int(rowptr[o]), int(rowptr[o + 1])
        if k1 - k0 and o % 4 == 1:
            colidx[k0], colidx[k1 - 1] = 0, c.n_in - 1
        if k1 - k0 >= 2 and o % 3 == 2:
            colidx[k0 + 1] = colidx[k0]
    return rowptr, np.array(colidx, np.int64), vpat


@functools.lru_cache(maxsize=None)
def extremes(fid, arith):
    """(gathered operand, stored matrix value) whose multiplied forms are largest for an accumulator"""
    if arith == "wide":                                         # Wide<NL>: every 32-bit word but the top one all ones, both sides
        w = CM.maximal_limbs(fid, 32, 2 * CM.FIELD_L[fid] - 1)
        return w, w
    return CM.ln_maxx(fid), CM.ln_maxv(fid)


def stored_of_multiplied(fid, vl):
    """the stored matrix value that the limb paths multiply as vl: they multiply v R' / R mod p (tests/common.py ln_maxv)"""
    p = CM.field_p(fid)
    N, W = CM.LN_SHAPE[fid]
    return vl * pow(2, 64 * CM.FIELD_L[fid], p) * pow(2, -N * W, p) % p


def multiplied_of_stored(fid, v):
    p = CM.field_p(fid)
    N, W = CM.LN_SHAPE[fid]
    return v * pow(2, N * W, p) * pow(2, -64 * CM.FIELD_L[fid], p) % p


def build_values(c, rowptr, vpat):
    """the stored matrix values as Python ints, by each output's pattern and the arithmetic its length selects.  "ext" and "pm1" are
    about what is MULTIPLIED: on the limb paths the stored value is the one whose R'-form is the extreme / is p - 1, on Wide<NL> the
    stored value itself is"""
    p = CM.field_p(c.fid)
    rnd = random.Random("v %s" % (c,))
    th = LB.k2_thresholds()
    vals = []
    for o in range(c.m):
        n = int(rowptr[o + 1] - rowptr[o])
        ar = arithmetic(c, n, th)
        ext = extremes(c.fid, ar)[1]
        pm1 = p - 1 if ar == "wide" else stored_of_multiplied(c.fid, p - 1)
        vals += {"ext": lambda: [ext] * n, "pm1": lambda: [pm1] * n, "alt": lambda: [ext if k & 1 else 0 for k in range(n)],
                 "rnd": lambda: [rnd.randrange(p) for _ in range(n)]}[vpat[o]]()
    return vals


def build_rows(c):
    """X[pos][row]: the operands as Python ints.  Row r follows XPATS[r % 6]; the constant and alternating patterns carry one entry of their own
    (r + 1 at a position that moves with r), so that no two rows are equal and a result in the wrong row shows."""
    p = CM.field_p(c.fid)
    rnd = random.Random("x %s" % (c,))
    limb_ext = extremes(c.fid, "ln" if c.limb and c.fid != 0 else "wide")[0]
    word_ext = extremes(c.fid, "wide")[0]
    rows = []
    for r in range(c.n_rows):
        pat = XPATS[r % 6]
        if pat in ("ext", "pm1", "words"):
            x = [{"ext": limb_ext, "pm1": p - 1, "words": word_ext}[pat]] * c.n_in
            x[(7 * r + 1) % c.n_in] = r + 1
        elif pat == "alt":
            x = [limb_ext if (i + r // 6) & 1 else 0 for i in range(c.n_in)]
            x[(7 * r + 1) % c.n_in] = r + 1
        elif pat == "rnd":
            x = [rnd.randrange(p) for _ in range(c.n_in)]
        else:
            x = [limb_ext if i % 3 else rnd.randrange(p) for i in range(c.n_in)]
        rows.append(x)
    assert len({tuple(x) for x in rows}) == c.n_rows
    return [list(col) for col in zip(*rows)]


# ---- the reference ------------------------------------------------------------------------------------------------------------------------
def ref_matvec(fid, rowptr, colidx, vals, X):
    """out[o][row] = sum_k vals[k] X[colidx[k]][row] / R mod p over k in [rowptr[o], rowptr[o + 1]), Python ints (stored limbs in and out)"""
    p = CM.field_p(fid)
    rinv = pow(1 << (64 * CM.FIELD_L[fid]), -1, p)
    n_rows = len(X[0])
    out = []
    for o in range(len(rowptr) - 1):
        k0, k1 = int(rowptr[o]), int(rowptr[o + 1])
        if k0 == k1:
            out.append([0] * n_rows)
            continue
        vs = vals[k0:k1]
        out.append([sum(map(mul, vs, xs)) * rinv % p for xs in zip(*[X[j] for j in colidx[k0:k1]])])
    return out


def ref_rs(fid, inp, n_out):
    """out[k][row] = sum_j inp[j][row] (k + 1)^j mod p by Horner, Python ints"""
    p = CM.field_p(fid)
    out = []
    for k in range(n_out):
        acc = [0] * len(inp[0]) if inp else []
        for j in range(len(inp) - 1, -1, -1):
            acc = [(a * (k + 1) + b) % p for a, b in zip(acc, inp[j])]
        out.append(acc)
    return out


def ints_to_elems(vals, L):
    """flat list of Python ints -> (n, L) uint64 limbs"""
    return np.frombuffer(b"".join(v.to_bytes(8 * L, "little") for v in vals), np.uint64).reshape(-1, L).copy()


def elems_to_ints(a):
    L = a.shape[-1]
    b = np.ascontiguousarray(a).tobytes()
    return [int.from_bytes(b[i:i + 8 * L], "little") for i in range(0, len(b), 8 * L)]


# ---- self-checks -------------------------------------------------------------------------------------------------------------------------
def test_case_ids_are_unique_and_cover_the_row_counts():
    ids = [case_id(c) for c in CASES]
    assert len(set(ids)) == len(ids)
    assert {c.n_rows for c in SPMV_CASES} == {1, 23}
    assert {c.n_rows for c in SPMM_CASES} == {24, 63, 64, 65, 101, 112, 113, 128, 130, 257}
    for c in CASES:
        assert c.out_off >= c.in_off + c.n_in
    assert any(c.in_off == 0 for c in SPMM_CASES) and any(c.in_off == 0 for c in SPMV_CASES)
    assert any(c.in_off and c.out_off > c.in_off + c.n_in for c in CASES)
    for path in ("spmm", "spmv"):
        assert {c.alt for c in CASES if c.path == path} == {False, True}


def test_selection_restated_on_the_thresholds_in_the_source():
    th = LB.k2_thresholds()
    assert th["sliced_above"] == sorted(th["sliced_above"], reverse=True) and th["opw_min_m"] > th["sliced_above"][0]
    assert len(th["sliced_sl"]) == len(th["sliced_above"]) + 1
    mk = lambda fid, m, r, limb=None: select(_case("spmm", fid, m, r, limb), th)
    # on both sides of every threshold
    assert mk(3, th["opw_min_m"], 64) == {"spmm_t_kernel<8,4>": 1} and mk(3, th["opw_min_m"] - 1, 64) == {"spmm_t_sliced_kernel<8,2>": 2}
    assert mk(0, th["sliced_above"][0] + 1, 64) == {"spmm_t_sliced_kernel<2,2>": 2} and mk(0, th["sliced_above"][0], 64) == {"spmm_t_sliced_kernel<2,4>": 4}
    assert mk(1, th["sliced_above"][1] + 1, 64) == {"spmm_t_sliced_kernel<4,4>": 4} and mk(1, th["sliced_above"][1], 64) == {"spmm_t_sliced_kernel<4,8>": 8}
    assert mk(3, 8192, 64 + th["tail_max"]) == {"spmm_t_kernel<8,4>": 1, "spmm_t_tail_kernel": 1}
    assert mk(3, 8192, 64 + th["tail_max"] + 1) == {"spmm_t_kernel<8,4>": 1}
    assert mk(3, 8192, th["tail_max"]) == {"spmm_t_tail_kernel": 1}                 # fewer than 64 rows: the tail kernel alone
    assert mk(2, 8192, 65) == {"spmm_t_kernel<6,4>": 1} and mk(0, 8192, 65) == {"spmm_t_kernel<2,4>": 1}


def _reached():
    """{kernel: {arithmetic: set of per-lane term counts}}, {kernel: set of output lengths}, {kernel: set of n_rows % 64}"""
    th = LB.k2_thresholds()
    counts, lengths, tails = {}, {}, {}
    for c in CASES:
        rowptr, _, _ = build_structure(c)
        for ln in set(np.diff(rowptr).tolist()):
            for kern, per in lane_counts(c, ln, th).items():
                counts.setdefault(kern, {}).setdefault(arithmetic(c, ln, th), set()).update(per)
                lengths.setdefault(kern, set()).add(ln)
        for kern in select(c, th):
            tails.setdefault(kern, set()).add(c.n_rows % 64)
    return counts, lengths, tails


def test_tables_reach_every_instantiation_and_every_boundary():
    counts, lengths, tails = _reached()
    full = set(BASE)
    limb_arith = {2: None, 4: "ln", 6: "ln", 8: "lazy29"}
    for nl in (2, 4, 6, 8):
        for kern in ["spmm_t_kernel<%d,4>" % nl] + ["spmm_t_sliced_kernel<%d,%d>" % (nl, s) for s in (2, 4, 8)]:
            assert kern in counts, kern
            if limb_arith[nl]:
                assert full <= counts[kern].get(limb_arith[nl], set()), (kern, "limb path")
            if nl != 8:                                        # Wide<2|4|6> in spmm_t_terms (Ft255 has the limb path only)
                assert full <= counts[kern].get("wide", set()), (kern, "Wide")
            else:
                assert "wide" not in counts[kern]
        for s in (2, 4, 8):
            got = lengths["spmm_t_sliced_kernel<%d,%d>" % (nl, s)]
            assert set(range(s)) | {s * 60, s * 60 + 1, s * 61 - 1} <= got, (nl, s)     # empty slices; the chunk edge inside the slices
        kern = "spmv_kernel<%d,8>" % nl
        assert full <= counts[kern]["wide"], kern
        assert {8 * 6 - 1, 8 * 6 + 1, 480, 481} <= lengths[kern]
    assert {b for b in BASE if b <= 60} <= counts["spmv_kernel<8,8>"]["lazy29"] and max(counts["spmv_kernel<8,8>"]["lazy29"]) == 60
    assert full <= counts["spmm_t_tail_kernel"]["lazy29"]
    assert {1, 37, 48} <= tails["spmm_t_tail_kernel"]
    no_tail = {c.n_rows % 64 for c in CASES if c.path == "spmm" and c.fid == 3 and list(select(c)) == ["spmm_t_kernel<8,4>"]}
    assert {0, 49} <= no_tail
    assert all("spmm_t_tail_kernel" not in select(c) for c in CASES if c.fid != 3)
    # the spmv lazy switch from both sides, in one launch
    th = LB.k2_thresholds()
    c = SPMV_CASES[0]
    assert arithmetic(c, 480, th) == "lazy29" and arithmetic(c, 481, th) == "wide" and c.fid == 3 and c.limb


@pytest.mark.parametrize("c", CASES, ids=case_id)
def test_matrix_structure(c):
    rowptr, colidx, vpat = build_structure(c)
    ln = np.diff(rowptr)
    assert len(rowptr) == c.m + 1 and rowptr[0] == 0 and (ln >= 0).all() and len(colidx) == rowptr[-1]
    assert ln[0] == 0 and ln[-1] == 0 and ln[c.m // 2] == 0                         # empty output first, last, in the middle
    assert colidx.min() == 0 and colidx.max() == c.n_in - 1                         # first and last input position
    assert any(ln[o] >= 2 and colidx[rowptr[o]] == colidx[rowptr[o] + 1] for o in range(c.m))      # a column repeated in one output
    assert set(special_lengths(c)) <= set(ln.tolist())
    for s in special_lengths(c):                                                    # every special length with all-extreme values
        if s:
            assert any(ln[o] == s and vpat[o] == "ext" for o in range(c.m)), s
    assert set(vpat) == set(VPATS)
    if c.n_rows >= 6:
        assert {XPATS[r % 6] for r in range(c.n_rows)} == set(XPATS)


@pytest.mark.parametrize("fid", [1, 2, 3])
def test_extremes_are_extreme_in_the_limb_model(fid):
    """ln_maxx / ln_maxv: every limb below the top one of the multiplied forms is 2^W - 1 and the top limbs are the largest that
    leaves them so; and 60 such terms at the kernels' cadence put the accumulator AT the proven maximum: the columns that take
    products of low limbs only hold exactly their bound before the first normalise, and the largest column value of the whole
    schedule is within 2^-10 of the bound's (the bound lets the top limb be floor((p - 1) / 2^(W (N - 1))), these have one less)."""
    a = LB.ln_acc(fid)
    p, N, W = a.p, a.N, a.W
    x, v = CM.ln_maxx(fid), CM.ln_maxv(fid)
    assert x < p and v < p
    vl = v * pow(2, N * W, p) * pow(2, -64 * CM.FIELD_L[fid], p) % p                # what launch_ntt_lns_roots / to_r29_kernel make of v
    top = (p >> (W * (N - 1))) - 1
    assert a.limbs(x) == a.limbs(vl) == [a.M] * (N - 1) + [top]
    assert x == a.maximal() and a.limbs(p - 1)[-1] == top + 1
    norm, terms = 6, 60
    assert LB.lazy29_cadences()["spmm_t_terms (lazy29)"] == ([6], [60, 60])
    cols, peak, first = [0] * (2 * N), 0, None
    xl = a.limbs(x)
    for t in range(1, terms + 1):
        for i in range(N):
            for j in range(N):
                cols[i + j] += xl[i] * xl[j]
        assert max(cols) < 1 << 64
        peak = max(peak, max(cols))
        if t == norm:
            first = list(cols)
        if t % norm == 0:
            a._norm(cols)
            peak = max(peak, max(cols))
    lm = a.max_limbs()
    per_term = [sum(lm[i] * lm[k - i] for i in range(N) if 0 <= k - i < N) for k in range(2 * N)]
    assert first[:N - 1] == [norm * per_term[k] for k in range(N - 1)]
    bound, _ = a.column_bounds(norm, terms)
    assert peak <= bound and bound - peak <= bound >> 10, (peak.bit_length(), bound.bit_length())
    want = terms * x * vl * pow(a.R, -1, p) % p
    assert a.replay([x] * terms, [vl] * terms, norm, terms) == want
    if fid == 3:                                                # Ft255 has no room: normalising every 9 terms (8 is the derived limit) wraps a column
        assert a.replay([x] * 60, [vl] * 60, 9, 60) != want


def _csr_from_csc(mat):
    """oracle CSC (rows, cols, colptr, rowidx, vals) -> CSR by output"""
    m, n_in, colptr, rowidx, vals = mat
    cols = np.repeat(np.arange(n_in), np.diff(colptr.astype(np.int64)))
    order = np.argsort(rowidx.astype(np.int64), kind="stable")
    rowptr = np.zeros(m + 1, np.int64)
    rowptr[1:] = np.cumsum(np.bincount(rowidx.astype(np.int64), minlength=m))
    return rowptr, cols[order], elems_to_ints(vals[order]) if len(order) else []


@pytest.mark.parametrize("fid", [0, 1, 2, 3])
def test_reference_is_the_oracle_encode(oracle, fid):
    """ref_matvec and ref_rs, chained the way encode.rs does (precodes down, R-S base case, postcodes up), give the C oracle's
    whole codeword on a real generated code -- every level's matrix, two rows at once -- so the GPU tests compare with a reference
    that was itself checked"""
    O = oracle
    n_per_row = 3000
    oenc = O.Encoding.sdig_from_dims(fid, n_per_row, 0, 21, 3)
    n_cols = oenc.get_dims(n_per_row)[2]
    mats = oenc.sdig_matrices()
    assert len(mats) >= 3
    L = CM.FIELD_L[fid]
    msg = O.random_elems(fid, 2 * n_per_row, 9).reshape(2, n_per_row, L)
    want = []
    for r in range(2):
        row = np.zeros((n_cols, L), np.uint64)
        row[:n_per_row] = msg[r]
        want.append(elems_to_ints(oenc.encode(row)))
    X = [[0, 0] for _ in range(n_cols)]
    for r in range(2):
        for i, v in enumerate(elems_to_ints(msg[r])):
            X[i][r] = v
    pre = [_csr_from_csc(a) + (a[0], a[1]) for a, _ in mats]
    post = [_csr_from_csc(b) + (b[0], b[1]) for _, b in mats]
    in_start = 0
    for rowptr, colidx, vals, m, n in pre[:-1]:
        X[in_start + n:in_start + n + m] = ref_matvec(fid, rowptr, colidx, vals, X[in_start:in_start + n])
        in_start += n
    rowptr, colidx, vals, m, n = pre[-1]
    in_end = in_start + n
    base = ref_matvec(fid, rowptr, colidx, vals, X[in_start:in_end])
    out_end = in_end + post[-1][4]
    X[in_end:out_end] = ref_rs(fid, base, out_end - in_end)
    in_start, out_start = in_end + m, out_end
    for (_, _, _, pm, _), (rowptr, colidx, vals, mm, nn) in zip(reversed(pre), reversed(post)):
        in_start -= pm
        assert nn == out_start - in_start
        X[out_start:out_start + mm] = ref_matvec(fid, rowptr, colidx, vals, X[in_start:out_start])
        out_start += mm
    assert out_start == n_cols
    for r in range(2):
        assert [x[r] for x in X] == want[r]


def test_int_limb_conversions():
    for fid in range(4):
        p, L = CM.field_p(fid), CM.FIELD_L[fid]
        vals = [0, 1, p - 1, CM.maxc(fid), (1 << 64) % p]
        a = ints_to_elems(vals, L)
        assert (a == CM.to_limbs(vals, L)).all() and elems_to_ints(a) == vals


def test_harness_refuses_indices_outside_its_buffers():
    """tests/native/k2_harness.cpp checks every index a kernel will form before it touches the device (a kernel that writes out of bounds
    can take the machine down with it): a column beyond the inputs, a rowptr that is not monotone or does not end at nnz, outputs
    beyond the buffer or over the inputs, a limb form for Ft63, a transpose source shorter than its rows.  No GPU is needed to refuse."""
    import k2_harness as H
    c = _case("spmm", 1, 300, 24)
    rowptr, colidx, _ = build_structure(c)
    vals = np.zeros((len(colidx), 2), np.uint64)
    t = np.zeros((c.out_off + c.m, c.n_rows, 2), np.uint64)
    mat = np.zeros((3, c.out_off + c.m, 2), np.uint64)

    def refused(fn, *a, **k):
        with pytest.raises(H.BadArgs):
            fn(*a, **k)

    bad_col = colidx.copy()
    bad_col[len(bad_col) // 2] = c.n_in
    bad_ptr = rowptr.copy()
    bad_ptr[5], bad_ptr[6] = rowptr[6], rowptr[5] - 1
    short = rowptr.copy()
    short[-1] -= 1
    for rp, ci in ((rowptr, bad_col), (bad_ptr, colidx), (short, colidx)):
        refused(H.spmm_t, 1, t, c.n_in, c.in_off, c.out_off, H.Csr(1, rp, ci, vals), True)
        refused(H.spmv, 1, mat, c.n_in, c.in_off, c.out_off, H.Csr(1, rp, ci, vals), False)
    ok = H.Csr(1, rowptr, colidx, vals)
    refused(H.spmm_t, 1, t, c.n_in, c.in_off, c.out_off + 1, ok, True)              # the last output beyond T
    refused(H.spmm_t, 1, t, c.n_in, c.in_off, c.in_off + 1, ok, True)               # outputs over the inputs
    refused(H.spmm_t, 1, t, t.shape[0], c.in_off, c.out_off, ok, True)              # inputs beyond T
    refused(H.spmv, 1, mat, c.n_in, c.in_off, c.out_off + 1, ok, False)
    refused(H.spmv, 1, mat, c.n_in, c.in_off, 0, ok, False, np.zeros((3, c.m - 1, 2), np.uint64))   # out_alt rows shorter than m
    refused(H.spmm_t, 0, np.zeros((t.shape[0], 24, 1), np.uint64), c.n_in, c.in_off, c.out_off,
            H.Csr(0, rowptr, colidx, np.zeros((len(colidx), 1), np.uint64)), True)  # Ft63 has no limb form
    refused(H.sdig_rs_t, 1, np.zeros((4, 24, 2), np.uint64), np.zeros((10, 24, 2), np.uint64), 3, 8)
    refused(H.sdig_rs, 1, np.zeros((2, 4, 2), np.uint64), 4, np.zeros((2, 10, 2), np.uint64), 3, 8)
    refused(H.transpose_to_t, 1, np.zeros((99, 2), np.uint64), 10, 10, 10, np.zeros((10, 10, 2), np.uint64))
    refused(H.transpose_from_t, 1, np.zeros((10, 4, 2), np.uint64), np.zeros((4, 9, 2), np.uint64))
    refused(H.pad_rows, 1, np.zeros((2, 8, 2), np.uint64), np.zeros((2, 7, 2), np.uint64), 8)


def _slices(c, rowptr, o, th):
    """[(k0, k1)] term ranges of output o's slices in the case's position-major kernel"""
    sl = max(select(c, th).values())
    k0, ln = int(rowptr[o]), int(rowptr[o + 1] - rowptr[o])
    return [(k0 + ln * s // sl, k0 + ln * (s + 1) // sl) for s in range(sl)]


FT255_SPMM_M = sorted({c.m for c in SPMM_CASES if c.fid == 3})


@pytest.mark.parametrize("m", FT255_SPMM_M)
def test_broken_cadences_give_wrong_outputs_on_these_tables(m):
    """The tables are not vacuous for the two bounds of the Ft255 limb path: the kernels' schedule replayed in the limb model
    (test_lazy_bounds.LimbAcc.replay: u64 wrap-around, one subtraction after REDC) on THIS case's matrix, rows and slice split gives
    every output right at (normalise 6, chunk 60), and gives wrong outputs with a normalise every 9 terms (on "ext" values x "ext" rows:
    a column wraps) and with REDC chunks of 81 terms (on "pm1" values x "pm1" rows: 81 (p - 1)^2 puts the REDC output past 2p; the
    limb-extreme operands, slightly smaller, do not).  Replayed: the outputs of more than one chunk per slice with "ext" / "pm1" values,
    their first and last slice, one "ext" and one "pm1" row."""
    c = next(c for c in SPMM_CASES if c.fid == 3 and c.m == m)
    th = LB.k2_thresholds()
    a = LB.lazy29()
    rowptr, colidx, vpat = build_structure(c)
    vals = build_values(c, rowptr, vpat)
    X = build_rows(c)
    sl = max(select(c, th).values())
    rinv = pow(a.R, -1, a.p)
    outs = [o for o in range(c.m) if vpat[o] in ("ext", "pm1") and (rowptr[o + 1] - rowptr[o]) // sl > 60]
    assert {vpat[o] for o in outs} == {"ext", "pm1"}
    wrong = {"norm9": set(), "chunk81": set()}
    for o in outs:
        for k0, k1 in {_slices(c, rowptr, o, th)[0], _slices(c, rowptr, o, th)[-1]}:
            vl = [multiplied_of_stored(3, v) for v in vals[k0:k1]]
            for r in (0, 1):
                assert XPATS[r] == ("ext", "pm1")[r]
                xs = [X[j][r] for j in colidx[k0:k1]]
                want = sum(map(mul, xs, vl)) * rinv % a.p
                assert a.replay(xs, vl, 6, 60) == want
                for name, (norm, terms) in (("norm9", (9, 60)), ("chunk81", (6, 81))):
                    try:
                        bad = a.replay(xs, vl, norm, terms) != want
                    except AssertionError:                     # the model's "chunk result not reduced": the kernel would store >= p
                        bad = True
                    if bad:
                        wrong[name].add((vpat[o], XPATS[r]))
    assert ("ext", "ext") in wrong["norm9"], wrong
    assert ("pm1", "pm1") in wrong["chunk81"], wrong


# ---- a message whose pre[0] outputs are chosen: the deep levels of the real encode at extremes (test_gpu_k2_kernels) ----------------------
def solve_message(fid, pre0, targets):
    """messages x (stored ints, one list of n_in per target) with pre[0] x = target on stored limbs, i.e. sum_k v_k x_col(k) = target_o R
    mod p for every output o: Gauss-Jordan elimination over F_p on the first columns of pre[0] that give it full row rank (the other
    message entries stay zero).  pre0 = (rowptr, colidx, vals, m, n_in) by output; targets: lists of m stored ints."""
    p = CM.field_p(fid)
    rowptr, colidx, vals, m, n_in = pre0
    R = pow(2, 64 * CM.FIELD_L[fid], p)
    n_use = min(n_in, m + m // 2 + 16)
    nt = len(targets)
    A = [[0] * n_use + [t[o] * R % p for t in targets] for o in range(m)]
    for o in range(m):
        for k in range(int(rowptr[o]), int(rowptr[o + 1])):
            if colidx[k] < n_use:
                A[o][int(colidx[k])] = (A[o][int(colidx[k])] + vals[k]) % p
    pivots, row = [], 0
    for col in range(n_use):
        piv = next((r for r in range(row, m) if A[r][col]), None)
        if piv is None:
            continue
        A[row], A[piv] = A[piv], A[row]
        inv = pow(A[row][col], -1, p)
        A[row] = [a * inv % p for a in A[row]]
        for r in range(m):
            f = A[r][col]
            if f and r != row:
                pr = A[row]
                A[r] = [(a - f * b) % p for a, b in zip(A[r], pr)]
        pivots.append(col)
        row += 1
        if row == m:
            break
    assert row == m, "pre[0] has no full row rank on its first %d columns" % n_use
    out = []
    for t in range(nt):
        x = [0] * n_in
        for r, col in enumerate(pivots):
            x[col] = A[r][n_use + t]
        out.append(x)
    return out


DEEP_N_PER_ROW = 1000          # pre[0]: 178 x 1000 (Gauss-Jordan on 178 x ~280 in Python ints), pre[1]: 32 x 178, pre[2]: 6 x 32


def deep_level_case(oracle, fid):
    """(oracle encoder, n_cols, pre matrices by output, targets, messages): messages whose pre[0] outputs -- the operands pre[1] gathers --
    are all ln_maxx (limb-extreme), all p - 1, and 0 / ln_maxx alternating"""
    oenc = oracle.Encoding.sdig_from_dims(fid, DEEP_N_PER_ROW, 0, 21, 3)
    n_cols = oenc.get_dims(DEEP_N_PER_ROW)[2]
    pre = [_csr_from_csc(a) + (a[0], a[1]) for a, _ in oenc.sdig_matrices()]
    assert len(pre) >= 3 and pre[0][4] == DEEP_N_PER_ROW
    p, m = CM.field_p(fid), pre[0][3]
    ext = CM.ln_maxx(fid) if fid else CM.maxc(fid)
    targets = [[ext] * m, [p - 1] * m, [ext if o & 1 else 0 for o in range(m)]]
    return oenc, n_cols, pre, targets, solve_message(fid, pre[0], targets)


@pytest.mark.parametrize("fid", [1, 3])
def test_solved_messages_put_the_targets_on_pre0(oracle, fid):
    """the solve is right in the reference AND in the oracle's encode: codeword positions [n, n + m0) hold the targets"""
    oenc, n_cols, pre, targets, msgs = deep_level_case(oracle, fid)
    L, m = CM.FIELD_L[fid], pre[0][3]
    got = ref_matvec(fid, pre[0][0], pre[0][1], pre[0][2], [list(col) for col in zip(*msgs)])
    assert [list(col) for col in zip(*got)] == targets
    for x, t in zip(msgs, targets):
        row = np.zeros((n_cols, L), np.uint64)
        row[:DEEP_N_PER_ROW] = ints_to_elems(x, L)
        assert elems_to_ints(oenc.encode(row)[DEEP_N_PER_ROW:DEEP_N_PER_ROW + m]) == t

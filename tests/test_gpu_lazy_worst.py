"""GPU tests of the lazy-reduction dot products at their worst operands (tests/test_lazy_bounds.py proves the bounds on CPU).

Operands are chosen by their stored Montgomery limbs, so that what the kernel multiplies is maximal:
  * coefficients: MAXC, the largest value < p whose low limbs are all ones -- eight 29-bit limbs for Ft255 (collapse29_kernel's
    ln::from_packed split), all but the top 32-bit word for Ft63 / Ft127 / Ft191 (collapse_kernel's Wide<NL> words) -- and p - 1;
  * tensors: for Ft255 the value whose 2^261 form (to_r29_kernel: t * 2^5 mod p) is MAXC, i.e. MAXC / 32 mod p; for the other fields
    MAXC itself;
  * a sprinkle of random rows / entries between the extremes, so that a wrong row order or a wrong batch boundary shows too.
The collapse reference is Python-int arithmetic (sum_r t_r c_rj / R mod p on the stored limbs, R = 2^(64 L)), not the C oracle."""
import random

import numpy as np
import pytest

import lcpc_amd
from common import (field_p, maxc, maxt, mk_transcript, ntt_case_id, ntt_case_stages, ntt_maxlimb, ntt_root, ntt_worst_cases,
                    stage_input_rows, to_int, to_limbs)
from lcpc_amd import LcCommit, LigeroEncoding, SdigEncoding, Transcript

pytestmark = pytest.mark.gpu


def _p(fid):
    return field_p(fid)


def _L(fid):
    return lcpc_amd.FIELD_LIMBS[fid]


def coeff_rows(O, fid, n_rows, n_per_row, seed):
    """(n_rows, n_per_row, L): MAXC rows, with rows of p - 1 (r % 7 == 4) and uniformly random rows (r % 16 == 9)"""
    L, p = _L(fid), _p(fid)
    out = np.empty((n_rows, n_per_row, L), np.uint64)
    out[:] = to_limbs([maxc(fid)], L)[0]
    out[4::7] = to_limbs([p - 1], L)[0]
    rnd = [r for r in range(n_rows) if r % 16 == 9]
    if rnd:
        out[rnd] = O.random_elems(fid, len(rnd) * n_per_row, seed).reshape(len(rnd), n_per_row, L)
    return out


def tensor(O, fid, n_rows, seed, kind=0):
    """kind 0: MAXT with p - 1 (r % 13 == 3) and random entries (r % 11 == 5); kind 1: p - 1 with MAXT every 5th, random every 9th"""
    L, p = _L(fid), _p(fid)
    rnd = O.random_elems(fid, n_rows, seed)
    vals = []
    for r in range(n_rows):
        if kind == 0:
            v = p - 1 if r % 13 == 3 else None if r % 11 == 5 else maxt(fid)
        else:
            v = maxt(fid) if r % 5 == 2 else None if r % 9 == 4 else p - 1
        vals.append(to_int(rnd[r]) if v is None else v)
    return to_limbs(vals, L)


def collapse_ref(fid, coeffs, t, cols):
    """Python ints: sum_r t_r c_rj / R mod p, for the columns `cols` (stored limbs in, stored limbs out)"""
    p, L = _p(fid), _L(fid)
    rinv = pow(1 << (64 * L), -1, p)
    ti = [to_int(x) for x in t]
    out = []
    for j in cols:
        col = coeffs[:, j]
        cache = {}
        s = 0
        for r in range(coeffs.shape[0]):
            key = col[r].tobytes()
            c = cache.get(key)
            if c is None:
                c = cache[key] = to_int(col[r])
            s += ti[r] * c
        out.append(s * rinv % p)
    return out


def collapse_splits(n_rows, n_per_row):
    """commit.cpp collapse_splits, restated: the whole-polynomial collapse splits its rows so that the grid has >= ~2k workgroups
    while every split keeps >= 16 rows (powers of two, at most 64)"""
    col_blocks = (n_per_row + 255) // 256
    s = 1
    while s < 64 and col_blocks * s < 2048 and n_rows // (s * 2) >= 16:
        s *= 2
    return s


# (n_rows, n_per_row).  Narrow rows let the split count climb to 64; rows per split = ceil(n_rows / splits) crosses the normalise
# cadence (6 terms) at 5..13 rows (one split) and the REDC chunk (60 rows) only when a split holds more than 60 rows, i.e. at
# 64 splits from 3 840 rows on: 64 x {59, 60, 61, 120, 121, 256} rows below.
COLLAPSE_SHAPES = [(1, 256), (5, 300), (6, 256), (7, 300), (12, 256), (13, 300), (59, 256), (60, 300), (61, 256), (119, 300),
                   (120, 256), (121, 300), (128, 256), (256, 300), (512, 256), (1024, 300), (2047, 256),
                   (64 * 59, 256), (64 * 60, 256), (64 * 61 - 3, 256), (64 * 120, 256), (64 * 121 - 40, 256), (64 * 256, 256)]


def _shape_id(s):
    n_rows, npr = s
    sp = collapse_splits(n_rows, npr)
    return "%dx%d-splits%d-rows_per_split%d" % (n_rows, npr, sp, -(-n_rows // sp))


def test_collapse_shapes_reach_every_split_count():
    """the split count is a power of two in [1, 64]; the shapes below take each of the seven values, and rows per split cross 6, 60
    and 120 (the normalise and REDC cadences of collapse29_kernel) and reach 256"""
    splits = {collapse_splits(r, n) for r, n in COLLAPSE_SHAPES}
    assert splits == {1, 2, 4, 8, 16, 32, 64}
    per = {-(-r // collapse_splits(r, n)) for r, n in COLLAPSE_SHAPES}
    assert {5, 6, 7, 12, 13, 59, 60, 61, 120, 121, 256} <= per


@pytest.mark.parametrize("fid", [3, 0, 1, 2])
@pytest.mark.parametrize("shape", COLLAPSE_SHAPES, ids=_shape_id)
def test_eval_outer_worst_operands(oracle, fid, shape):
    """eval_outer (lcpc_collapse -> collapse_run): Ft255 runs collapse29_kernel<NT> (ln::lazy_mac, normalise every 6 rows, one
    ln::lazy_reduce per <= 60 rows: REDC input < 60 p^2, output < 2p), the other fields collapse_kernel<NL, NT> (Wide<NL>, reduced every 8
    rows); with more than one split, field_sum_kernel adds the per-split partials.  NT = 1 (one tensor) and NT = 2 (a stack of two),
    MAXC / p - 1 / random coefficient rows against MAXT / p - 1 / random tensor entries, against Python ints at sampled columns
    (the first and last of each 256-column block, the ragged block's last, random ones)."""
    O = oracle
    n_rows, npr = shape
    L = _L(fid)
    coeffs = coeff_rows(O, fid, n_rows, npr, 1000 + n_rows)
    n_cols = 1 << (2 * npr - 1).bit_length()          # (Ligero: a power of two, >= 2 n_per_row)
    enc = LigeroEncoding.new_from_dims(fid, npr, n_cols)
    c = LcCommit.from_parts(enc, np.zeros((n_rows * n_cols, L), np.uint64), coeffs.reshape(-1, L), n_rows)
    assert c.n_rows == n_rows and c.n_per_row == npr
    t1 = tensor(O, fid, n_rows, 7, 0)
    t2 = tensor(O, fid, n_rows, 8, 1)
    rnd = random.Random(n_rows * 7 + fid)
    cols = sorted({0, npr - 1, 255 % npr, min(256, npr - 1)} | {rnd.randrange(npr) for _ in range(6)})
    one = c.eval_outer(t1)
    both = c.eval_outer(np.stack([t1, t2]))
    ref1 = collapse_ref(fid, coeffs, t1, cols)
    ref2 = collapse_ref(fid, coeffs, t2, cols)
    for k, j in enumerate(cols):
        assert to_int(one[j]) == ref1[k], ("NT=1", j)
        assert to_int(both[0, j]) == ref1[k], ("NT=2 first", j)
        assert to_int(both[1, j]) == ref2[k], ("NT=2 second", j)
    if not any(r % 16 == 9 for r in range(n_rows)):
        # no random row: every column holds the same extremes, so every output equals the sampled ones
        assert (one == one[0]).all() and (both == both[:, :1]).all()


PROVE_SHAPES = [(3, 1024, 256), (3, 64 * 61 - 3, 256), (0, 1024, 256), (1, 300, 512), (2, 2047, 256)]


@pytest.mark.parametrize("fid,n_rows,npr", PROVE_SHAPES,
                         ids=["ft%d-%s" % (f, _shape_id((r, n))) for f, r, n in PROVE_SHAPES])
def test_prove_worst_operands(oracle, fid, n_rows, npr):
    """LcCommit::prove on an extreme commitment (MAXC / p - 1 / random rows; outer tensor MAXT / p - 1 / random): p_eval and p_random
    are collapse outputs (collapse29_kernel for Ft255, collapse_kernel otherwise; the split count is in the id), pinned inside the wire format by the
    oracle prover's bytes; p_eval also against Python ints at sampled columns."""
    O = oracle
    L = _L(fid)
    coeffs = coeff_rows(O, fid, n_rows, npr, 2000 + n_rows).reshape(-1, L)
    enc = LigeroEncoding.new_from_dims(fid, npr, 2 * npr)
    oenc = O.Encoding.ligero_from_dims(fid, npr, 2 * npr)
    c = LcCommit.commit(coeffs, enc)
    oc = O.Commit.commit(coeffs, oenc, n_threads=8)
    root = c.get_root()
    assert root == oc.get_root()
    outer = tensor(O, fid, n_rows, 9, 0)
    nco = enc.get_n_col_opens()
    pf = c.prove(outer, enc, mk_transcript(Transcript, root, nco))
    opf, _ = oc.prove(outer, oenc, mk_transcript(O.Transcript, root, nco))
    assert pf.to_bytes() == opf
    pe = c.eval_outer(outer)
    cols = [0, 1, npr // 2, npr - 1]
    assert [to_int(pe[j]) for j in cols] == collapse_ref(fid, coeffs.reshape(n_rows, npr, L), outer, cols)


@pytest.mark.parametrize("fid,n_per_row,n_cols,n_rows", [(3, 36864, 131072, 17), (1, 40000, 131072, 9)], ids=lambda v: str(v))
def test_prove_long_polynomial_worst_operands(oracle, fid, n_per_row, n_cols, n_rows):
    """the sliced collapse (commit.cpp collapse_range with len < n_per_row: prove fetches p_random in two column ranges, the cut at
    n_per_row / 8 rounded up to 256), one tensor, rows split further than the whole-polynomial launch; extreme rows on both sides of
    the cut (every row is constant across columns except the random ones): proof bytes == the oracle prover's."""
    O = oracle
    L = _L(fid)
    n = n_rows * n_per_row - 1234
    coeffs = coeff_rows(O, fid, n_rows, n_per_row, 3000).reshape(-1, L)[:n]
    enc = LigeroEncoding.new_from_dims(fid, n_per_row, n_cols)
    oenc = O.Encoding.ligero_from_dims(fid, n_per_row, n_cols)
    c = LcCommit.commit(coeffs, enc)
    oc = O.Commit.commit(coeffs, oenc, n_threads=8)
    root = c.get_root()
    assert root == oc.get_root()
    nco = enc.get_n_col_opens()
    for kind in (0, 1):
        outer = tensor(O, fid, n_rows, 10 + kind, kind)
        pf = c.prove(outer, enc, mk_transcript(Transcript, root, nco))
        opf, _ = oc.prove(outer, oenc, mk_transcript(O.Transcript, root, nco))
        assert pf.to_bytes() == opf, kind


def sdig_rows(O, fid, n_rows, n_per_row, n):
    """Brakedown message rows: MAXC (r % 3 == 0; for Ft255 the lazy29 limb split, for Ft63 the Wide words), p - 1 (r % 3 == 1),
    random (r % 3 == 2); n coefficients in all (a ragged last row when n < n_rows * n_per_row)"""
    rows = np.empty((n_rows, n_per_row, _L(fid)), np.uint64)
    rows[0::3] = to_limbs([maxc(fid)], _L(fid))[0]
    rows[1::3] = to_limbs([_p(fid) - 1], _L(fid))[0]
    k = len(range(2, n_rows, 3))
    if k:
        rows[2::3] = O.random_elems(fid, k * n_per_row, 41).reshape(k, n_per_row, -1)
    return rows.reshape(-1, _L(fid))[:n]


# Which kernel applies the first precode matrix (pre[0], the only level whose input is the message, i.e. the extreme rows; it writes
# codeword positions [n_per_row, n_per_row + m)) -- kernels.hip launch_spmv / launch_spmm_t: fewer than 24 rows take spmv_kernel (lane =
# output, 8 lanes per output; Ft255: the lazy29 branch, since no output of these codes has more than 60 * 8 terms -- checked below, so
# spmv_kernel's Wide<8> fallback cannot be reached through the API; Ft63: Wide<2>).  From 24 rows on the position-major kernels: m >= 8192
# outputs spmm_t_kernel<NL, 4>, plus spmm_t_tail_kernel for Ft255 when 1 <= n_rows % 64 <= 48; m in (2048, 8192) spmm_t_sliced_kernel<NL, 2>,
# (256, 2048] <NL, 4>.  The id names the kernel, and the test asserts the m that selects it.
SDIG_SHAPES = [
    (3, 3000, 12, "spmv-lazy29"), (0, 3000, 12, "spmv-wide2"),
    (3, 50000, 64, "spmm4-64rows"), (3, 50000, 101, "spmm4-tail37"), (3, 50000, 72, "spmm4-tail8"),
    (3, 20000, 30, "sliced2"), (3, 2500, 30, "sliced4"), (0, 50000, 101, "spmm4-wide2"), (0, 2500, 30, "sliced4-wide2"),
]


def _pre0_terms(oenc):
    """pre[0] as (m, [(input positions, values as ints)] per output) from the oracle's CSC matrices"""
    pre, _ = oenc.sdig_matrices()[0]
    m, n_in, colptr, rowidx, vals = pre
    cols = np.repeat(np.arange(n_in), np.diff(colptr.astype(np.int64)))
    return m, cols, rowidx.astype(np.int64), vals


@pytest.mark.parametrize("fid,n_per_row,n_rows,path", SDIG_SHAPES, ids=[s[3] + "-ft%d" % s[0] for s in SDIG_SHAPES])
def test_brakedown_worst_operands(oracle, fid, n_per_row, n_rows, path):
    """Brakedown encode with message rows of MAXC and of p - 1 (every product of pre[0]'s dot products has its gathered operand at
    its largest) between random rows, ragged last row.  Ft255: lazy29 in spmv_kernel / spmm_t_terms / spmm_t_tail_kernel (normalise every
    6 terms, REDC per <= 60); Ft63: Wide<2> in batches of 8.  The whole comm and the whole hashes array against the oracle, and sampled
    pre[0] outputs of the extreme rows against a Python-int mat-vec of the oracle's matrix (sum_k v_k x_col(k) / R mod p)."""
    O = oracle
    oenc = O.Encoding.sdig_from_dims(fid, n_per_row, 0, 21, 3)
    _, _, n_cols = oenc.get_dims(n_per_row)
    assert len(oenc.sdig_matrices()) > 1                      # pre[0]'s outputs are stored in the codeword
    m, cols, outs, vals = _pre0_terms(oenc)
    if path.startswith("spmv"):
        assert n_rows < 24
        assert np.bincount(outs, minlength=m).max() <= 60 * 8  # lazy29 branch for every output (Ft255)
    elif path.startswith("spmm4"):
        assert n_rows >= 24 and m >= 8192
        tail = n_rows % 64
        assert ("tail" in path) == (fid == 3 and 1 <= tail <= 48) and (path.endswith("tail%d" % tail) or "tail" not in path)
    else:
        assert n_rows >= 24 and m < 8192
        assert (2048 < m) == (path.startswith("sliced2")) and m > 256
    n = n_per_row * n_rows - 5
    coeffs = sdig_rows(O, fid, n_rows, n_per_row, n)
    enc = SdigEncoding.new_from_dims(fid, n_per_row, n_cols, 21, 3)
    c = LcCommit.commit(coeffs, enc)
    oc = O.Commit.commit(coeffs, oenc, n_threads=8)
    assert (c.comm() == oc.comm()).all()
    assert (c.hashes() == oc.hashes()).all() and c.get_root() == oc.get_root()
    p, L = _p(fid), _L(fid)
    rinv = pow(1 << (64 * L), -1, p)
    rnd = random.Random(n_rows + fid)
    for r in (0, 1):                                          # a MAXC row and a p - 1 row
        x = to_int(coeffs[r * n_per_row])                     # (constant rows)
        got = c.comm(r, 1)
        for o in [0, m - 1] + [rnd.randrange(m) for _ in range(6)]:
            sel = outs == o
            want = sum(to_int(v) for v in vals[sel]) * x * rinv % p
            assert to_int(got[n_per_row + o]) == want, (r, o)


# ---- the row NTT with extremes entering every DIF stage --------------------------------------------------------------------------------
def _ntt_patterns(fid):
    p = _p(fid)
    return {"p-1": [p - 1], "0/p-1": [0, p - 1], "maxlimb": [ntt_maxlimb(fid)]}


def _ntt_stage_batches(fid, log_n, log_rate, stages, max_bytes=512 << 20):
    """(tags, rows) batches of the stage-input rows, pattern by pattern, stage by stage; no batch's codewords exceed max_bytes"""
    L, n = _L(fid), 1 << log_n
    per = max(1, max_bytes // (n * L * 8))
    tags, buf = [], []
    for name, pat in _ntt_patterns(fid).items():
        rows = stage_input_rows(fid, log_n, stages, pat, log_rate)
        for s, row in zip(stages, rows):
            tags.append((name, s))
            buf.append(row)
            if len(buf) == per:
                yield tags, np.stack(buf)
                tags, buf = [], []
        del rows
    if buf:
        yield tags, np.stack(buf)


def _ints(row):
    b, L = row.tobytes(), row.shape[-1]
    return [int.from_bytes(b[8 * L * i:8 * L * (i + 1)], "little") for i in range(row.shape[0])]


NTT_CASES = ntt_worst_cases()


@pytest.mark.parametrize("fid,log_n,log_rate,general,mid_mb", NTT_CASES, ids=[ntt_case_id(*c) for c in NTT_CASES])
def test_ntt_extremes_at_every_stage(oracle, fid, log_n, log_rate, general, mid_mb):
    """Rows built so that the values entering DIF stage s (oracle/lcpc_oracle.c fft_io_L: natural in, bit-reversed out,
    w = ROOT^(2^(S - log n)); restated in tests/common.py dif_stage) are a pattern P -- all p - 1, alternating 0 / p - 1, or the element
    with every low limb of the NTT's limb form at 2^W - 1.  A rate-2^-r row (x, 0, ..., 0) keeps its free prefix x through stages
    0 .. r - 1, and from stage r on that prefix never meets the rest of the row (tests/common.py stage_input_rows), so P holds on
    the first n / 2^r inputs of stage s: every stage up to 2^20 columns, including the pass boundaries and the register-fed last
    round; above (three-pass plans, the forced general kernel at 2^21) stage 0, the last two and each pass boundary with its
    neighbours (tests/common.py ntt_case_stages).  The shapes (tests/common.py ntt_worst_cases; the id names the instantiation:
    first-pass stages S, three-pass plan, K1s's limb intermediate and LCPC_NTT_MID_MAX_MB, blk0_gone of the canonical-output last
    pass) take every first-pass template of ntt_l9s.hip (K1s, Ft255) and ntt_lns.hip (K1n, Ft63 / Ft127 / Ft191), both last-pass
    variants, the three-pass plans, the one-pass general plan, and the general kernel of kernels.hip (LCPC_NTT_GENERAL=1);
    tests/test_lazy_bounds.py::test_ntt_worst_cases_reach_every_instantiation checks that.  Rows go in batches of at most 512 MiB
    of codewords (a ragged row count: one row per stage).  Every row through encode (Montgomery output) against the oracle's
    encoding of it, and commit (canonical-output path: comm, hashes, root) against the oracle's commit; sampled columns of two rows
    against the definition sum_i c_i w^(i bitrev(j)) mod p in Python ints."""
    import os
    O = oracle
    p, L, n = _p(fid), _L(fid), 1 << log_n
    npr = n >> log_rate
    rho = (1, 1 << log_rate)
    what = ntt_case_id(fid, log_n, log_rate, general, mid_mb)
    stages = ntt_case_stages(fid, log_n, general)
    env = {"LCPC_NTT_GENERAL": "1"} if general else {}
    if mid_mb is not None:
        env["LCPC_NTT_MID_MAX_MB"] = str(mid_mb)
    os.environ.update(env)
    try:
        enc = LigeroEncoding.new_from_dims(fid, npr, n, rho=rho)
    finally:
        for k in env:
            os.environ.pop(k, None)
    oenc = O.Encoding.ligero_from_dims(fid, npr, n, rho=rho)
    probe = {("maxlimb", stages[-1]), ("p-1", stages[len(stages) // 2])}
    kept = {}
    for tags, rows in _ntt_stage_batches(fid, log_n, log_rate, stages):
        nb = len(tags)
        msg = rows.reshape(-1, L)
        oc = O.Commit.commit(msg, oenc, n_threads=16)
        want = oc.comm().reshape(nb, n, L)
        padded = np.zeros((nb, n, L), np.uint64)
        padded[:, :npr] = rows
        got = enc.encode(padded).reshape(nb, n, L)
        del padded
        for i in range(nb):
            assert (got[i] == want[i]).all(), (what, "encode", tags[i])
        for i, t in enumerate(tags):
            if t in probe:
                kept[t] = (_ints(rows[i]), got[i].copy())
        del got
        c = LcCommit.commit(msg, enc)
        assert (c.comm().reshape(nb, n, L) == want).all(), (what, "commit", tags)
        assert (c.hashes() == oc.hashes()).all() and c.get_root() == oc.get_root(), (what, "hashes", tags)
        del c, oc, want
    # the definition, independent of the oracle and of pyref
    w = ntt_root(fid, log_n)
    rnd = random.Random(log_n * 10 + fid)
    cols = [0, 1, n - 1] + [rnd.randrange(n) for _ in range(13 if log_n <= 16 else 1)]
    for t, (x, out) in sorted(kept.items()):
        for j in cols:
            wj = pow(w, int(format(j, "0%db" % log_n)[::-1], 2), p)
            acc = 0
            for v in reversed(x):
                acc = (acc * wj + v) % p
            assert to_int(out[j]) == acc, (what, t, j)

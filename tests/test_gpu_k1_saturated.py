"""The pass kernels of the Ligero row NTT (K1) on a FULL device.  tests/test_gpu_k1_passes.py holds every instantiation to the exact model
of tests/k1_pass_model.py, but with 1 or 3 rows: at most a few thousand workgroups, and at the small shapes 2 .. 6 of them on 256 CUs.  A
missing or misplaced barrier between two LDS rounds gives wrong values only when the waves of a workgroup drift apart, and they drift
least on an idle CU.  Here every launch has SAT_TILES = 2 x CUs x 8 workgroups (k1_pass_model.sat_tiles; the CU count is read from the
device): 8 is the most 256-thread workgroups a CU can hold, so every CU is full and every slot is refilled at least once whatever the
real residency is -- CUs shared by several workgroups, a workgroup starting in the LDS another has just left, waves of different
workgroups competing for issue under mem_phase, and the XCD-aware workgroup-to-(tile, row) mappings at hundreds to thousands of rows.

The model does not grow.  A three-row reference run is held to the model exactly as in test_gpu_k1_passes.py (its run_step, with every
check of that module), and its bytes are kept; the saturating launch of the same step then has R rows, row r being row r % 3 of the
reference run, and must give row r % 3's bytes.  R is the smallest odd row count that 3 does not divide with R x tiles_per_row >=
SAT_TILES (k1_pass_model.sat_rows), which keeps q % n_rows and q / n_rows off the powers of two and off the period of the pattern.
The three rows: uniform residues; p - 1 throughout; 0 / p - 1 alternating with common.ntt_maxlimb in every fourth element.

Per step and variant (limb / packed intermediate for K1s, Montgomery / canonical output where the step has a converting table):
  1. every dst row, mid record and copy_dst row on [0, n_valid) equals its reference row byte for byte (a mismatch names the row, tile
     and element of the first difference and counts the rows that differ);
  2. canaries intact, the gaps between strided rows and copy_dst beyond n_valid untouched, a first pass that writes mid leaves dst alone
     and a last pass that reads it leaves it alone;
  3. the same launch once more gives the same bytes;
  4. the steps the product runs in place (after the first, without mid) give the same bytes in place.
First-pass fills at R rows: n_valid = n / 2 with a source stride of n_valid + 3, copy_dst, and n_src_total cutting the LAST row in its
middle; that row is held to the last row of a three-row run with the same cut.

Cases: every k1_pass_model.plan_cases() entry up to 2^20 columns (three-pass rows are 2048 workgroups each already, and their sub-row
passes are the 2^20 kernels), Ft255 forced general at 2^19 (l9<11>), and the Montgomery-word Ft255 kernel at 2^10 and 2^11.  The
general kernel counts its own tile, so ntt_pass_kernel runs in its BS = 256 form throughout (asserted).  Every launch stays below
1 GiB of device memory (tests/test_k1_pass_cases.py).

Commits (test_commit_at_a_saturating_row_count): the default plan of every field at 2^5, 2^10 and from its first two-pass size to
2^20 columns, rate 1/2, R rows with a ragged last one, against the oracle's commit on comm, coeffs, hashes and root, and enc.encode of
the same rows -- the product's own batching, in-place second pass and streams.  Ft255 up to 2^15 columns also under
LCPC_NTT_MID_MAX_MB = 1024 (the whole job one batch of the limb intermediate; so is the default's 6144 at these sizes: a saturating
job holds 4 Mi elements x 36 bytes = 144 MiB) and = 48 (four batches: 144 MiB / 48 MiB rounded up to whole rows).

Wall time per case, measured on an MI355X (256 CUs: SAT_TILES = 4096, R = 5 .. 4097; pytest --durations, two runs on two machines).
With all four variants at every size the slowest K1s case, K1s-2^20-split, took 9.7 s and 14.8 s (2^19: 5.4 / 10.7 s, 2^18: 3.0 s),
so from 2^16 columns on a K1s case runs two of them (_variants): 4.7 s at 2^20, 2.9 s at 2^19, 1.0 .. 2.6 s below.  2^11 .. 2^15
columns, all four variants: 1.1 .. 3.3 s.  The slowest
K1n case is K1n-ft191-2^20 with 1.6 s, the slowest general-kernel case general-ft255-2^19 with 1.6 s; a fills case at most 1.2 s, a
commit at most 0.7 s."""
import numpy as np
import pytest

import common as CM
import k1_pass_model as M
import k1p_harness as H
import test_gpu_k1_passes as P
from test_gpu_k1_passes import ctxs  # noqa: F401  (the fixture: one context at a time)

pytestmark = pytest.mark.gpu
SAT_CASES = M.sat_plan_cases()
GAP = P.GAP
SEED = 91


_CUS = []


def _cus():
    """compute units of the device, read once"""
    if not _CUS:
        import torch
        _CUS.append(int(torch.cuda.get_device_properties(0).multi_processor_count))
    return _CUS[0]


def _three_rows(O, fid, n, seed):
    """(3, n, L): uniform residues; p - 1; 0 / p - 1 alternating with the all-ones-limbs element in every fourth place"""
    L, p = CM.FIELD_L[fid], CM.field_p(fid)
    rows = np.empty((3, n, L), np.uint64)
    rows[0] = O.random_elems(fid, n, seed)
    rows[1] = np.tile(CM.to_limbs([p - 1], L), (n, 1))
    rows[2] = np.tile(CM.to_limbs([0, p - 1, 0, CM.ntt_maxlimb(fid)], L), (n // 4, 1))
    return rows


def _job(O, fid, rows, n_valid, stride, seed, order=(0, 1, 2)):
    """a job's source of three rows at `stride`: rows[order[r]][:n_valid] at r * stride, uniform residues between them"""
    L = CM.FIELD_L[fid]
    src = O.random_elems(fid, 3 * stride, seed).reshape(3, stride, L).copy()
    for r in range(3):
        src[r, :n_valid] = rows[order[r], :n_valid]
    return src.reshape(-1, L)


def _tile_words(words3, R):
    """(3, W) -> (R, W): row r is row r % 3"""
    return words3[np.arange(R) % 3]


def _source(rec, inp, R, ln, NL):
    """the source of the saturating launch of the step `rec` records, whose three-row run read `inp`"""
    if rec["step"] == 0:
        stride = rec["src_stride"]
        rows3 = M.limbs_to_words(inp[:3 * stride]).reshape(3, stride * NL)
        need = min(rec["n_src_total"], (R - 1) * stride + rec["n_valid"])
        return _tile_words(rows3, R).reshape(-1)[:need * NL]
    if rec["reads_mid"]:
        return _tile_words(M.mid_encode(inp).reshape(3, ln * 9), R).reshape(-1)
    stride = rec["src_stride"]
    buf = np.full((R, stride, NL), P.JUNK, np.uint32)
    buf[:, :ln] = _tile_words(M.limbs_to_words(inp).reshape(3, ln * NL), R).reshape(R, ln, NL)
    return buf.reshape(-1)[:((R - 1) * stride + ln) * NL]


def _elem_of_word(w, NL):
    return w // NL


def _elem_of_mid_word(w, NL=None):
    """the element a word of a row's limb records belongs to: [tile][limbs 0-3 x 1024 | limbs 4-7 x 1024 | limb 8 x 1024]"""
    tile, off = divmod(w, 9 * M.TILE)
    return tile * M.TILE + ((off % (4 * M.TILE)) // 4 if off < 8 * M.TILE else off - 8 * M.TILE)


def _same_rows(got, ref, what, name, elem_of=_elem_of_word, NL=1, last=None):
    """got (R, W) against ref (3, W): row r equals ref[r % 3] -- the last row equals `last` where that is given"""
    body = got if last is None else got[:-1]
    n_bad, first = 0, None
    for j in range(3):
        d = body[j::3] != ref[j]
        if d.any():
            rows = np.nonzero(d.any(axis=1))[0]
            n_bad += len(rows)
            r = int(rows[0]) * 3 + j
            if first is None or r < first[0]:
                first = (r, int(np.nonzero(d[rows[0]])[0][0]))
    if last is not None and (got[-1] != last).any():
        n_bad += 1
        if first is None:
            first = (len(got) - 1, int(np.nonzero(got[-1] != last)[0][0]))
    if first is not None:
        e = elem_of(first[1], NL)
        raise AssertionError(tuple(what) + ("%s: %d of %d rows differ from their reference row; first: row %d tile %d element %d" % (
            name, n_bad, len(got), first[0], e >> 10, e),))


def _dst_rows(buf, n_rows, stride, ln, NL):
    b = buf.body.reshape(n_rows, stride, NL)
    return b[:, :ln].reshape(n_rows, ln * NL), b[:, ln:]


def saturate(cx, rec, inp, R, what, last=None):
    """the launch `rec` records, with R rows in place of three, held to the bytes rec's launch gave.  last: the record of a three-row
    run whose LAST row is the reference of this launch's last row (the n_src_total cut)"""
    i, NL = rec["step"], cx.NL
    ln = 1 << cx.steps[i].log_n
    assert cx.steps[i].log_n == cx.log_n                 # (no sub-row passes up to 2^20 columns)
    what = tuple(what) + ("step %d" % i, "rows %d" % R, "flags %d" % rec["flags"])
    ss, ds, nv = rec["src_stride"], rec["dst_stride"], rec["n_valid"]
    src = _source(rec, inp, R, ln, NL)
    kw = dict(n_rows=R, src_stride=ss, dst_stride=ds, n_valid=nv if i == 0 else None, n_src_total=rec["n_src_total"])
    dst, mid, cp = cx.run_step(i, src, flags=rec["flags"], **kw)

    def ref_of(name, f):
        return f(rec[name]), (None if last is None else f(last[name])[2])

    assert dst.canaries_intact(), what + ("dst canaries",)
    if rec["writes_mid"]:
        assert dst.untouched(), what + ("a first pass that writes mid wrote dst",)
        assert mid.canaries_intact(), what + ("mid canaries",)
        ref, lst = ref_of("mid", lambda b: b.body.reshape(3, ln * 9))
        _same_rows(mid.body.reshape(R, ln * 9), ref, what, "mid", _elem_of_mid_word, last=lst)
    else:
        rows, gaps = _dst_rows(dst, R, ds, ln, NL)
        ref, lst = ref_of("dst", lambda b: _dst_rows(b, 3, ds, ln, NL)[0])
        _same_rows(rows, ref, what, "dst", NL=NL, last=lst)
        assert (gaps == H.CANARY).all(), what + ("gap written",)
        if rec["reads_mid"]:
            assert mid.canaries_intact() and (mid.body == src).all(), what + ("the last pass wrote mid",)
    if cp is not None:
        assert cp.canaries_intact(), what + ("copy_dst canaries",)
        body = cp.body.reshape(R, ss, NL)
        ref, lst = ref_of("copy", lambda b: np.ascontiguousarray(b.body.reshape(3, ss, NL)[:, :nv]).reshape(3, nv * NL))
        _same_rows(np.ascontiguousarray(body[:, :nv]).reshape(R, nv * NL), ref, what, "copy_dst", NL=NL, last=lst)
        assert (body[:, nv:] == H.CANARY).all(), what + ("copy_dst written past n_valid",)
    # ---- once more: the same bytes
    again = cx.run_step(i, src, flags=rec["flags"], **kw)
    for a, b, name in zip((dst, mid, cp), again, ("dst", "mid", "copy_dst")):
        assert (a is None and b is None) or (a.all == b.all).all(), what + ("%s differs between two runs of one launch" % name,)
    del again
    # ---- in place, where the product runs in place
    if i > 0 and not rec["reads_mid"]:
        assert ss == ds
        z, _, _ = cx.run_step(i, src, flags=rec["flags"] | H.F_INPLACE, **kw)
        assert z.canaries_intact(), what + ("in place: dst canaries",)
        zrows, zgaps = _dst_rows(z, R, ds, ln, NL)
        assert (zrows == rows).all(), what + ("in place and out of place differ", int((zrows != rows).any(axis=1).sum()))
        assert (zgaps[:-1] == P.JUNK).all() and (zgaps[-1] == H.CANARY).all(), what + ("in place: gap written",)


def _variants(cx):
    """(limb intermediate, canonical output): both intermediates for a K1s two-pass plan, both outputs where the plan converts.  From
    2^16 columns on, where the three-row model runs are the cost of a case (four variants: 14 s at 2^20 columns), a K1s plan keeps two
    of the four: the packed intermediate with canonical output (what a commit runs there) and the limb one with Montgomery output"""
    mids = (False, True) if P._has_mid(cx) else (False,)
    canons = (False, True) if cx.steps[0].can_canon else (False,)
    if cx.log_n >= P.BIG and len(mids) == 2 and len(canons) == 2:
        return [(False, True), (True, False)]
    return [(m, c) for m in mids for c in canons]


@pytest.mark.parametrize("case", SAT_CASES, ids=[c[0] for c in SAT_CASES])
def test_every_step_on_a_full_device(oracle, ctxs, case):  # noqa: F811
    O = oracle
    cid, fid, k, env, general = case
    cx = P._plan(ctxs, case)
    n = 1 << k
    R = M.sat_rows(M.sat_tiles_per_row(fid, k, general), _cus())
    assert R % 2 == 1 and R % 3 and R * M.sat_tiles_per_row(fid, k, general) >= M.sat_tiles(_cus())
    for st in cx.steps:
        if st.kind == "general":                         # more than 256 tiles: never the one-row block size
            assert ", 1024>" not in M.general_instantiation(fid, st.log_tile, st.s, st.log_tj, R, k), st
            assert R << (k - st.s - st.log_tj) >= M.sat_tiles(_cus()), st
    rows = _three_rows(O, fid, n, SEED + k)
    job = _job(O, fid, rows, n, n, SEED)
    for mid, canonical in _variants(cx):
        what = (cid, "mid %d" % mid, "canon %d" % canonical)
        x = job
        for i in range(len(cx.steps)):
            rec = {}
            kw = dict(n_valid=n, src_stride=n, copy=True) if i == 0 else {}
            y = P.run_step(O, ctxs, cx, i, x, 3, canonical, mid=mid, gap=0 if mid else GAP, what=what, keep=rec, **kw)
            saturate(cx, rec, x, R, what)
            x = y


@pytest.mark.parametrize("case", SAT_CASES, ids=[c[0] for c in SAT_CASES])
def test_first_pass_fills_on_a_full_device(oracle, ctxs, case):  # noqa: F811
    """rate 1/2 (the zero-padded first round), rows further apart than they are long, copy_dst, and the source ending in the middle
    of the last row"""
    O = oracle
    cid, fid, k, env, general = case
    cx = P._plan(ctxs, case)
    n = 1 << k
    R = M.sat_rows(M.sat_tiles_per_row(fid, k, general), _cus())
    nv, stride = n // 2, n // 2 + 3
    rows = _three_rows(O, fid, n, SEED + k)
    canonical = cx.steps[0].can_canon
    c_last = (R - 1) % 3                                  # the reference row the saturating run's last row repeats
    order = tuple((j + c_last - 2) % 3 for j in range(3))
    assert order[2] == c_last
    for mid in ((False, True) if P._has_mid(cx) and k < P.BIG else (False,)):
        what = (cid, "fills", "mid %d" % mid)
        whole, cut = {}, {}
        job = _job(O, fid, rows, nv, stride, SEED)
        kw = dict(mid=mid, gap=0 if mid else GAP, n_valid=nv, src_stride=stride, copy=True)
        P.run_step(O, ctxs, cx, 0, job, 3, canonical, what=what, keep=whole, **kw)
        P.run_step(O, ctxs, cx, 0, _job(O, fid, rows, nv, stride, SEED, order), 3, canonical, n_src_total=2 * stride + nv // 2,
                   what=what + ("cut",), keep=cut, **kw)
        saturate(cx, whole, job, R, what)
        sat = dict(whole, n_src_total=(R - 1) * stride + nv // 2)
        saturate(cx, sat, job, R, what + ("cut",), last=cut)


# ---- the Montgomery-word Ft255 kernel --------------------------------------------------------------------------------------------------------
def _general(cx, src, lt, t0, s, ltj, n_rows, flags):
    return cx.run_general(src, lt, t0, s, ltj, n_rows=n_rows, flags=flags)[0]


@pytest.mark.parametrize("k", M.MONTWORD_SIZES)
def test_montgomery_word_kernel_on_a_full_device(oracle, ctxs, k):  # noqa: F811
    """ntt_pass_kernel<8, 10 / 11, 256> (qp29 == null): the passes of test_montgomery_word_ft255_kernel, three rows against the model
    and R rows against the three"""
    O = oracle
    cx = ctxs.get(3, k, {})
    n, L, NL = 1 << k, 4, 8
    x0 = _three_rows(O, 3, n, SEED + k)
    for passes in M.sat_montword_splits(k):
        x = x0
        for lt, t0, s, ltj in passes:
            what = ("montword", k, lt, t0, s, ltj)
            R = M.sat_rows(max(1, n >> lt), _cus())
            assert M.general_instantiation(3, lt, s, ltj, R, k, montword=True) == "ntt_pass_kernel<8, %d, 256>" % lt
            ref = _general(cx, M.limbs_to_words(x), lt, t0, s, ltj, 3, H.F_MONTWORD)
            assert ref.canaries_intact(), what
            y = M.words_to_limbs(ref.body, L).reshape(3, n, L)
            assert (y == M.model_dif(O, 3, x, k, t0, s)).all(), what
            src = _tile_words(M.limbs_to_words(x).reshape(3, n * NL), R).reshape(-1)
            got = _general(cx, src, lt, t0, s, ltj, R, H.F_MONTWORD)
            assert got.canaries_intact(), what
            _same_rows(got.body.reshape(R, n * NL), ref.body.reshape(3, n * NL), what, "dst", NL=NL)
            again = _general(cx, src, lt, t0, s, ltj, R, H.F_MONTWORD)
            assert (again.all == got.all).all(), what + ("two runs of one launch differ",)
            if t0 > 0:                                   # (the product runs the passes after the first in place)
                z = _general(cx, src, lt, t0, s, ltj, R, H.F_MONTWORD | H.F_INPLACE)
                assert (z.all == got.all).all(), what + ("in place and out of place differ",)
            x = y


# ---- whole commits at a saturating row count ---------------------------------------------------------------------------------------------------
COMMITS = [(fid, k, None) for fid, k in M.sat_commit_cases()] + [(3, k, mb) for k in range(11, 16) for mb in (1024, 48)]


@pytest.mark.parametrize("fid,k,mid_mb", COMMITS, ids=["ft%d-2^%d-%s" % (CM.FIELD_BITS[f], k, "default" if mb is None else "mid%d" % mb)
                                                       for f, k, mb in COMMITS])
def test_commit_at_a_saturating_row_count(oracle, fid, k, mid_mb):
    from lcpc_amd import LcCommit
    O = oracle
    n, L = 1 << k, CM.FIELD_L[fid]
    npr = n // 2
    R = M.sat_rows(M.sat_tiles_per_row(fid, k, False), _cus())
    n_coeffs = (R - 1) * npr + npr // 2 + 1               # a ragged last row
    coeffs = O.random_elems(fid, n_coeffs, SEED + 7 * k + fid)
    oc = O.Commit.commit(coeffs, O.Encoding.ligero_from_dims(fid, npr, n), n_threads=8)
    want = oc.comm()
    enc = P._product(fid, {}, npr, n, mid_mb)
    if mid_mb is not None:                               # what the cap is there for: one batch, or several
        rb = CM.ntt_mid_rows(fid, k, 2, R, mid_mb)
        assert (rb == R) if mid_mb == 1024 else (0 < rb and -(-R // rb) >= 3), (R, rb)
    c = LcCommit.commit(coeffs, enc)
    what = (fid, k, mid_mb, R)
    assert c.get_n_rows() == R, what
    assert (c.comm() == want).all(), what + ("comm",)
    assert (c.coeffs() == oc.coeffs()).all(), what + ("coeffs",)
    assert (c.hashes() == oc.hashes()).all() and c.get_root() == oc.get_root(), what + ("root",)
    rows = np.zeros((R, n, L), np.uint64)
    padded = np.zeros((R * npr, L), np.uint64)
    padded[:n_coeffs] = coeffs
    rows[:, :npr] = padded.reshape(R, npr, L)
    assert (enc.encode(rows.reshape(-1, L)) == want).all(), what + ("encode",)

"""The pass kernels of the Ligero row NTT (K1), ONE launch at a time, against the exact model of tests/k1_pass_model.py: the general kernel
(kernels.hip launch_ntt_pass), K1s (ntt_l9s.hip launch_ntt_pass_l9s) and K1n (ntt_lns.hip launch_ntt_pass_lns), through
tests/native/k1p_harness.cpp, which fills NttPassArgs the way ctx.cpp encode_rows_device does.  The whole-commit tests compare the last
pass's output with the oracle; here every pass's own output is compared, in every element, with no tolerance:

  1. the decoded dst / mid is congruent mod p to the model, in the representation the rule names for that element (value x R, or the
     value itself under canonical output: k1_pass_model.mont_mask_after);
  2. the stored form is within the producer's documented range: K1s first passes below p + 2^239, K1n first passes below p + 64 B, the
     general kernel and every last pass fully reduced; mid records normalised with |value| < 4p (pure / coset form: 12.04p);
  3. canaries and the gaps between strided rows are untouched; copy_dst equals the source on [0, n_valid) of every row, is zero where
     the flat index is >= n_src_total and untouched elsewhere; a first pass that writes mid leaves dst alone;
  4. in place and out of place give the same bytes (the steps the product runs in place);
  5. all steps chained through the harness give the bytes of enc.encode (Montgomery output) and of LcCommit.commit(...).comm() and
     .coeffs() (canonical output, copy_dst) for the same rows.

Cases (k1_pass_model.plan_cases; tests/test_k1_pass_cases.py asserts that they reach every instantiation): K1s at 2^11 .. 2^20 columns
under the DIF and the pure / coset form with both multipliers, each with the limb intermediate and with the packed one; K1n for Ft63 /
Ft127 / Ft191 from their first two-pass size to 2^20; the three-pass plans at 2^21 and 2^22 for all four fields; the general kernel at
each field's largest one-pass, first two-pass and first three-pass size, Ft127 at 2^20 with one row (ntt_pass_kernel<4, 12, 1024>) and
Ft63 at 2^12 with 1 and 300 rows (BS = 1024 and 256); the Montgomery-word Ft255 kernel (qp29 == null) at 2^10 and 2^11; and free
splits of the general kernel at 2^12 .. 2^14 columns.  One row and three rows (three rows with gaps between the rows); one row only from
2^21 columns on.  Rows, not shapes, are what keeps a case to a few seconds (BIG = 2^16 columns): from there on the three-row run of a
context is made once -- strided, without the limb intermediate -- and the variants (Montgomery / canonical output, limb / packed
intermediate, the fills, the consumer-side inputs) run on one row; at 2^22 columns the two sub-row passes, which are the kernels and
the shapes of 2^21, get the chain alone.

Fills (first passes): n_valid in {1, n/4, n/4 + 1, n/2, n/2 + 1, n - 1, n}; n_src_total cutting the last row in its first element, in
the middle and one element before its end.  Inputs: uniform residues; p - 1, alternating 0 / p - 1 and common.ntt_maxlimb placed as THIS
pass's input; for the passes that read an intermediate, the top of the producer's range (p + 2^239 - 1, p + 64 B - 1), p - 1, p, p + 1,
and mid records of value +-(4p - 1) (coset pass: +-(12.04p - 1)) and with every low limb at 2^29 - 1 beside the largest and smallest
top limb.

Free splits: every (t0, s, log_tj) with s + log_tj <= log_tile on a tile no longer than the row, for each field at the tile sizes
plan_passes uses for it.  Any (t0, s) chains with (0, t0) and (t0 + s, ..) to a whole transform, and the model of a split is the
stages [t0, t0 + s) of the transform the CPU tests hold to lo_fft_io.  They reach (test_k1_pass_cases.py
test_free_splits_reach_the_paths_of_the_general_kernel): s odd, s even and s = 1; lb < log_tj (a tile that spans several blocks of the
pass); the trivial last two stages in a radix-4 round (s even, t0 + s = log_n) and the trivial last stage in the radix-2 tail (s odd).

Instantiations of launch_ntt_pass that nothing but this harness reaches: ntt_pass_kernel<8, 10, 256> and <8, 11, 256> (no context leaves
qp29 null for Ft255).  ntt_pass_kernel<4, 12, 1024> runs otherwise only for Ft127 forced general at 2^20 with one row."""
import os

import numpy as np
import pytest

import common as CM
import k1_pass_model as M
import k1p_harness as H

pytestmark = pytest.mark.gpu
PLAN_CASES = M.plan_cases()
GAP = 5                                                  # elements between strided rows
BIG = 16                                                 # log2 columns from which the variants of a context run on one row
JUNK = 0xEEEEEEEE                                        # what a source holds where no pass may read


class Env:
    """one context at a time (a 2^22-column context holds gigabytes of tables), with its restated plan and the coset twist"""

    def __init__(self):
        self.key, self.cx, self.twist = None, None, None

    def get(self, fid, k, env):
        key = (fid, k, tuple(sorted(env.items())))
        if key != self.key:
            self.close()
            self.cx, self.key, self.twist = H.Ctx(fid, (1 << k) // 2, 1 << k, env=env), key, None
        return self.cx

    def close(self):
        if self.cx:
            self.cx.close()
        self.key, self.cx = None, None


@pytest.fixture(scope="module")
def ctxs():
    e = Env()
    yield e
    e.close()


def _plan(ctxs, case):
    """the context of a case; the plan it got is the plan the case asked for, field by field"""
    _, fid, k, env, general = case
    cx = ctxs.get(fid, k, env)
    rs = M.restated_steps(fid, k, general, env.get("LCPC_NTT_FORM"))
    assert len(cx.steps) == len(rs), (cx.steps, rs)
    for a, b in zip(cx.steps, rs):
        for f in M.RStep.FIELDS:
            if f == "log_tile" and b.kind != "general":
                continue
            if f == "first" and b.kind == "general":
                continue
            assert getattr(a, f) == getattr(b, f), (f, a, b)
    M.check_plan_fields(fid, k, cx.steps)
    for st in cx.steps:                                  # the multiplier and the pack classes the switches ask for (ctx.cpp build_limb_plan)
        if st.kind == "general":
            assert st.n_classes == 0 and st.mul2 == 0, st
            continue
        nf, mul, s0 = st.form == 1, env.get("LCPC_NTT_MUL"), cx.steps[0].s
        has = st.s == 10 if not st.first else st.s not in (2, 7, 9)               # kernels.h ntt_l9s_mul2_supported
        want = nf and has and (mul == "split" or (mul is None and (s0 == 8 if st.first else s0 >= 6)))
        assert st.mul2 == int(want), (st, env)
        assert st.n_classes == (1 << (st.log_n - 10) if st.first != nf else 1), st
    if ctxs.twist is None and cx.steps[-1].kind == "K1s" and cx.steps[-1].form == 1:
        import oracle_lib as O
        ctxs.twist = M.twist_table(O, fid, k)
    return cx


def _has_mid(cx):
    return len(cx.steps) == 2 and cx.steps[0].kind == "K1s"


def _rows_of(buf, n_sub, stride, ln, NL):
    """body of a dst / copy buffer -> (the rows (n_sub, ln, NL) uint32, the gaps)"""
    b = buf.body.reshape(n_sub, stride, NL)
    return b[:, :ln], b[:, ln:]


def run_step(O, ctxs, cx, i, inp, n_rows, canonical, mid=False, gap=0, n_valid=None, n_src_total=H.UNLIMITED, src_stride=None, copy=False,
             inplace=False, what=(), keep=None):
    """launch step i on `inp` and hold everything it wrote to the model.  inp: step 0: the job's source, (elements, L) uint64; later
    steps: (n_rows, n, L) stored values below the producer's bound, or (n_rows, n, 9) int32 limb records if the step reads mid.
    -> the step's output in the form the next step reads (stored limbs, or limb records).  keep: a dict that receives the launch as it
    was made -- the source words, the strides, n_valid, n_src_total, the flags -- and the three buffers as they came back"""
    fid, k, L, NL = cx.fid, cx.log_n, CM.FIELD_L[cx.fid], cx.NL
    p, n = CM.field_p(fid), 1 << k
    st, last = cx.steps[i], i + 1 == len(cx.steps)
    ln = 1 << st.log_n
    n_sub = n_rows << (k - st.log_n)
    what = tuple(what) + ("step %d" % i, "rows %d" % n_rows, "canon %d" % canonical, "mid %d" % mid, "gap %d" % gap)
    reads_mid, writes_mid = mid and i > 0, mid and i == 0
    flags = (H.F_CANON if canonical else 0) | (H.F_MID if mid else 0) | (H.F_COPY if copy else 0) | (H.F_INPLACE if inplace else 0)
    dst_stride = ln + gap
    # ---- the source words, and the stored residues the pass reads
    if i == 0:
        n_valid = ln if n_valid is None else n_valid
        src_stride = n_valid if src_stride is None else src_stride
        need = min(n_src_total, (n_rows - 1) * src_stride + n_valid)
        src_words = M.limbs_to_words(inp[:need])
        read = M.padded_source(inp, n_rows, n, src_stride, n_valid, n_src_total, L)
        res = read
        s_stride = src_stride
    elif reads_mid:
        src_words = M.mid_encode(inp)
        res, norm, rng = M.mid_values(inp, p, M.mid_bound(p, st.form))
        assert norm.all() and rng.all(), what
        res = res.reshape(n_rows, n, L)
        s_stride = ln
    else:
        s_stride = dst_stride if inplace or gap else ln
        buf = np.full(((n_sub - 1) * s_stride + ln, NL), JUNK, np.uint32)
        sub = M.limbs_to_words(inp).reshape(n_sub, ln, NL)
        for r in range(n_sub):
            buf[r * s_stride:r * s_stride + ln] = sub[r]
        src_words = buf.reshape(-1)
        flat = inp.reshape(-1, L)
        assert not M.ge_const(flat, 2 * p).any()
        res = M.reduce_once(flat, p).reshape(n_rows, n, L)
    dst, midb, cp = cx.run_step(i, src_words, n_rows=n_rows, src_stride=s_stride, dst_stride=dst_stride, n_valid=n_valid if i == 0 else None,
                                n_src_total=n_src_total, flags=flags)
    if keep is not None:
        keep.update(step=i, src_words=src_words, src_stride=s_stride, dst_stride=dst_stride, n_valid=n_valid if i == 0 else ln,
                    n_src_total=n_src_total, flags=flags, dst=dst, mid=midb, copy=cp, reads_mid=reads_mid, writes_mid=writes_mid)
    # ---- the model
    m_in = M.mont_mask_after(fid, k, cx.steps, i - 1, canonical)
    m_out = M.mont_mask_after(fid, k, cx.steps, i, canonical)
    y = M.model_step(O, fid, st, M.stored_to_mont(O, fid, res, m_in), ctxs.twist)
    want = M.mont_to_stored(O, fid, y, m_out)
    # ---- what the pass stored
    assert dst.canaries_intact(), what + ("dst canaries",)
    if writes_mid:
        assert dst.untouched(), what + ("a first pass that writes mid wrote dst",)
        assert midb.canaries_intact(), what + ("mid canaries",)
        limbs = M.mid_decode(midb.body, n_rows, k)
        got, norm, rng = M.mid_values(limbs, p, M.mid_bound(p, st.form))
        assert norm.all(), what + ("mid limbs not normalised", int((~norm).sum()))
        assert rng.all(), what + ("|mid value| >= %s" % ("12.04p" if st.form else "4p"), int((~rng).sum()))
        out = limbs
    else:
        rows, gaps = _rows_of(dst, n_sub, dst_stride, ln, NL)
        if inplace:                                      # (the source's own gaps; nothing was uploaded behind the last row)
            assert (gaps[:-1] == JUNK).all() and (gaps[-1] == H.CANARY).all(), what + ("gap written",)
        else:
            assert (gaps == H.CANARY).all(), what + ("gap written",)
        stored = M.words_to_limbs(np.ascontiguousarray(rows), L)
        bound = M.store_bound(fid, st.kind, last)
        over = M.ge_const(stored, bound)
        assert not over.any(), what + ("stored value outside [0, %#x)" % bound, int(over.sum()), int(np.nonzero(over)[0][0]))
        got = stored if bound == p else M.reduce_once(stored, p)
        out = stored.reshape(n_rows, n, L)
        if reads_mid:
            assert midb.canaries_intact() and (midb.body == src_words).all(), what + ("the last pass wrote mid",)
    bad = (got.reshape(n_rows, n, L) != want).any(axis=2)
    if bad.any():
        r, g = (int(v[0]) for v in np.nonzero(bad))
        raise AssertionError(what + ("%d wrong residues; first: row %d element %d (tile %d), stored as %s" % (
            int(bad.sum()), r, g, g >> 10, "value x R" if m_out[g] else "value"),))
    # ---- copy_dst: the loads on [0, n_valid), nothing else
    if copy:
        body = cp.body.reshape(n_rows, s_stride, NL)
        assert cp.canaries_intact(), what + ("copy_dst canaries",)
        assert (M.words_to_limbs(np.ascontiguousarray(body[:, :n_valid]), L).reshape(n_rows, n_valid, L) == read[:, :n_valid]).all(), what + ("copy_dst",)
        assert (body[:, n_valid:] == H.CANARY).all(), what + ("copy_dst written past n_valid",)
    return out


def chain(O, ctxs, cx, src, n_rows, canonical, mid, gap=0, n_valid=None, src_stride=None, copy=False, inplace_too=False, what=()):
    """every step of the plan, each fed what the step before stored -> the last step's stored limbs (n_rows, n, L)"""
    x = src
    for i in range(len(cx.steps)):
        kw = dict(n_valid=n_valid, src_stride=src_stride, copy=copy) if i == 0 else {}
        y = run_step(O, ctxs, cx, i, x, n_rows, canonical, mid=mid, gap=0 if mid else gap, what=what, **kw)
        if inplace_too and i > 0 and not mid:
            z = run_step(O, ctxs, cx, i, x, n_rows, canonical, gap=gap, inplace=True, what=tuple(what) + ("in place",))
            assert (z == y).all(), tuple(what) + ("step %d: in place and out of place differ" % i,)
        x = y
    return x


def _product(fid, env, n_per_row, n_cols, mid_mb):
    """an encoder of the product under the case's switches"""
    from lcpc_amd import LigeroEncoding
    e = dict(env)
    if mid_mb is not None:
        e["LCPC_NTT_MID_MAX_MB"] = str(mid_mb)
    saved = {k: os.environ.pop(k) for k in H.SWITCHES if k in os.environ}
    os.environ.update(e)
    try:
        return LigeroEncoding.new_from_dims(fid, n_per_row, n_cols, rho=(1, 2))
    finally:
        for k in e:
            del os.environ[k]
        os.environ.update(saved)


@pytest.mark.parametrize("case", PLAN_CASES, ids=[c[0] for c in PLAN_CASES])
def test_every_step_and_their_chain(oracle, ctxs, case):
    """uniform residues at rate 1/2 with copy_dst: each step against the model (checks 1 - 3), in place against out of place (4), and the
    chain against the product (5)"""
    from lcpc_amd import LcCommit
    O = oracle
    cid, fid, k, env, general = case
    cx = _plan(ctxs, case)
    n, L = 1 << k, CM.FIELD_L[fid]
    npr = n // 2
    rows_list = M.GENERAL_EXTRA_ROWS.get((fid, k), [1] if (fid, k) == (1, 20) else M.case_rows(k)) if general else M.case_rows(k)
    can_canon = cx.steps[0].can_canon
    for n_rows in rows_list:
        coeffs = O.random_elems(fid, n_rows * npr, 31 + k + n_rows)
        for mid in ((False, True) if _has_mid(cx) else (False,)):
            enc = _product(fid, env, npr, n, (64 if mid else 0) if _has_mid(cx) else None)
            variants = [(False, 0), (True, 0)] if can_canon else [(False, 0)]
            if n_rows == 3:                              # the strided run; from BIG on it is the only three-row run
                variants = [(can_canon, GAP)] if k >= BIG else variants + [(can_canon, GAP)]
            if n_rows == 3 and k >= BIG and mid:
                continue
            for canonical, gap in variants:
                what = (cid, "chain")
                out = chain(O, ctxs, cx, coeffs, n_rows, canonical, mid, gap=gap, n_valid=npr, copy=True, inplace_too=gap == 0 and not canonical,
                            what=what)
                if gap:
                    continue
                if canonical:
                    c = LcCommit.commit(coeffs, enc)
                    assert (M.from_canon(O, fid, out).reshape(-1, L) == c.comm()).all(), what + ("comm", n_rows, mid)
                    assert (c.coeffs() == coeffs).all()
                else:
                    full = np.zeros((n_rows, n, L), np.uint64)
                    full[:, :npr] = coeffs.reshape(n_rows, npr, L)
                    assert (enc.encode(full.reshape(-1, L)) == out.reshape(-1, L)).all(), what + ("encode", n_rows, mid)


@pytest.mark.parametrize("case", PLAN_CASES, ids=[c[0] for c in PLAN_CASES])
def test_first_pass_fills(oracle, ctxs, case):
    """n_valid at the boundaries of the first round's three forms (rate <= 1/4, rate <= 1/2, general) and n_src_total cutting the last
    row, with copy_dst and a source stride larger than n_valid"""
    O = oracle
    cid, fid, k, env, general = case
    cx = _plan(ctxs, case)
    n = 1 << k
    n_rows = 1 if k >= BIG else 3
    canonical = cx.steps[0].can_canon
    src = O.random_elems(fid, n_rows * (n + 3), 17 + k)
    mids = (False, True) if _has_mid(cx) and k < BIG else (False,)
    for j, nv in enumerate((1, n // 4, n // 4 + 1, n // 2, n // 2 + 1, n - 1, n)):
        stride = nv + (3 if n_rows > 1 else 0)
        for mid in mids:
            run_step(O, ctxs, cx, 0, src, n_rows, canonical and j % 2 == 0, mid=mid, n_valid=nv, src_stride=stride, copy=True, what=(cid, "n_valid %d" % nv))
    for nv in ((n // 2, n) if k < BIG else (n // 2,)):
        stride = nv + (3 if n_rows > 1 else 0)
        first = (n_rows - 1) * stride                    # flat index of the last row's first element
        for cut in (first, first + nv // 2, first + nv - 1):
            run_step(O, ctxs, cx, 0, src, n_rows, canonical, n_valid=nv, src_stride=stride, n_src_total=cut, copy=True,
                     what=(cid, "n_valid %d n_src_total %d" % (nv, cut)))


def _patterns(fid, n, L):
    """three rows: p - 1, alternating 0 / p - 1, the element whose low limbs are all ones"""
    p = CM.field_p(fid)
    rows = np.empty((3, n, L), np.uint64)
    for r, pat in enumerate(([p - 1], [0, p - 1], [CM.ntt_maxlimb(fid)])):
        rows[r] = np.tile(CM.to_limbs(pat, L), (n // len(pat), 1))
    return rows


def _mid_records(vals, n):
    return np.tile(np.array([M.mid_limbs_of(v) for v in vals], np.int64).astype(np.int32), (n // len(vals), 1))


@pytest.mark.parametrize("case", PLAN_CASES, ids=[c[0] for c in PLAN_CASES])
def test_crafted_and_consumer_side_inputs(oracle, ctxs, case):
    """the crafted patterns as THIS pass's input, and -- for the passes that read an intermediate -- the edges of what the producer may
    store, which a last pass never sees through a commit"""
    O = oracle
    cid, fid, k, env, general = case
    cx = _plan(ctxs, case)
    n, L, p = 1 << k, CM.FIELD_L[fid], CM.field_p(fid)
    one_row = k >= 21
    pats = _patterns(fid, n, L)
    canons = [cx.steps[0].can_canon] if k >= BIG else sorted({False, cx.steps[0].can_canon})
    for i, st in enumerate(cx.steps):
        if k >= 22 and i > 0 and st.kind != "general":     # (the sub-row passes of 2^21, same kernels and shapes)
            break
        mids = (False, True) if _has_mid(cx) and (k < BIG or i > 0) else (False,)
        for canonical in canons:
            for mid in mids:
                reads_mid = mid and i > 0
                what = (cid, "crafted")
                if reads_mid:
                    rec = np.stack([_mid_records([v], n) for v in (p - 1, CM.ntt_maxlimb(fid), 0)])
                    rec[2, 1::2] = _mid_records([p - 1], n)[1::2]
                    run_step(O, ctxs, cx, i, rec, 3, canonical, mid=True, what=what)
                elif i == 0:
                    for r in ([0, 1, 2] if one_row else [None]):
                        src = pats[r] if one_row else pats.reshape(-1, L)
                        run_step(O, ctxs, cx, 0, src, 1 if one_row else 3, canonical, mid=mid, what=what)
                else:
                    for r in ([0, 1, 2] if one_row else [None]):
                        run_step(O, ctxs, cx, i, pats[r:r + 1] if one_row else pats, 1 if one_row else 3, canonical, what=what)
        if i == 0:
            continue
        # ---- consumer side: what the step before may store
        prev = cx.steps[i - 1]
        bound = M.store_bound(fid, prev.kind, False)
        canonical = cx.steps[0].can_canon
        if bound > p:
            edge = [bound - 1, p - 1, p, p + 1, 0, bound - 2, 1, p - 2]
            rows = np.empty((1 if k >= BIG else 3, n, L), np.uint64)
            rows[0] = np.tile(CM.to_limbs(edge, L), (n // len(edge), 1))
            if len(rows) == 3:
                rows[1] = np.tile(CM.to_limbs([bound - 1], L), (n, 1))
                lift = np.tile(CM.to_limbs([bound - p, 0, 0], L), (n // 2, 1))[:n]       # every third one lifted to [bound - p, bound)
                rows[2] = _add_small(O.random_elems(fid, n, 5 + k), lift)
            run_step(O, ctxs, cx, i, rows, len(rows), canonical, what=(cid, "producer's range"))
        if _has_mid(cx):
            # +-(4p - 1) -- the coset pass: +-(12.04p - 1), what the pure pass may store (k1_pass_model.mid_bound) --; every low limb at
            # 2^29 - 1 under the largest and the smallest top limb; every low limb zero likewise
            B = M.mid_bound(p, st.form)
            P4, ones = B - 1, (1 << 232) - 1
            hi, lo = (P4 - ones) >> 232, -((P4 + ones) >> 232)
            vals = [P4, -P4, (hi << 232) + ones, (lo << 232) + ones, (P4 >> 232) << 232, -((P4 >> 232) << 232), 0, ones]
            if st.form:
                vals[6:8] = [4 * p - 1, -(4 * p - 1)]
            assert all(abs(v) < B for v in vals) and ((hi + 1) << 232) + ones >= B and ((lo - 1) << 232) + ones <= -B
            rec = np.stack([_mid_records(vals, n), _mid_records([P4], n), _mid_records([-P4], n)][:1 if k >= BIG else 3])
            run_step(O, ctxs, cx, i, rec, len(rec), canonical, mid=True, what=(cid, "mid at the edge of invariant I"))


def _add_small(a, b):
    """a + b on (n, L) uint64 limbs with carries (no overflow of the top limb)"""
    out = a.copy()
    carry = np.zeros(len(a), np.uint64)
    for i in range(a.shape[1]):
        s = a[:, i] + b[:, i]
        c1 = s < a[:, i]
        s2 = s + carry
        c2 = s2 < s
        out[:, i] = s2
        carry = (c1 | c2).astype(np.uint64)
    return out


# ---- the general kernel on free splits, and the Montgomery-word Ft255 kernel ---------------------------------------------------------------
FREE = [(fid, k, lt) for fid in range(4) for k in M.FREE_SPLIT_SIZES for lt in M.free_tiles(fid)]


def _general_run(O, cx, x, log_tile, t0, s, ltj, flags, what):
    """launch_ntt_pass on stored Montgomery limbs x (1, n, L), whole row -> stored limbs, held to the model"""
    fid, k, L = cx.fid, cx.log_n, CM.FIELD_L[cx.fid]
    p, n = CM.field_p(fid), 1 << k
    dst, _ = cx.run_general(M.limbs_to_words(x), log_tile, t0, s, ltj, flags=flags)
    assert dst.canaries_intact(), what
    got = M.words_to_limbs(dst.body, L)
    assert not M.ge_const(got, p).any(), what + ("not fully reduced",)
    return got.reshape(1, n, L)


@pytest.mark.parametrize("fid,k,lt", FREE, ids=["ft%d-2^%d-lt%d" % (CM.FIELD_BITS[f], k, lt) for f, k, lt in FREE])
def test_general_kernel_free_splits(oracle, ctxs, fid, k, lt):
    """every split launch_ntt_pass accepts; Ft255 (the lazy-limb kernel) with canonical output, where the stages before t0 decide what is
    still in Montgomery form at the input and mont_prefix what the final pass reduces"""
    O = oracle
    cx = ctxs.get(fid, k, {"LCPC_NTT_GENERAL": "1"})
    n, L = 1 << k, CM.FIELD_L[fid]
    x0 = O.random_elems(fid, n, 40 + k).reshape(1, n, L)
    before = {0: x0}                                     # the row after stages [0, t0)
    for t in range(1, k):
        before[t] = M.model_dif(O, fid, before[t - 1], k, t - 1, 1)
    canonical = fid == 3
    blk = np.arange(n)
    for t0, s, ltj in M.free_splits(k, lt):
        what = ("free split", fid, k, lt, t0, s, ltj)
        m_in = blk < (n >> t0) if canonical else np.ones(n, bool)
        m_out = (blk < (n >> (t0 + s))) & (t0 + s < k) if canonical else np.ones(n, bool)
        src = M.mont_to_stored(O, fid, before[t0], m_in)
        got = _general_run(O, cx, src, lt, t0, s, ltj, H.F_CANON if canonical else 0, what)
        want = M.mont_to_stored(O, fid, M.model_dif(O, fid, before[t0], k, t0, s), m_out)
        bad = (got != want).any(axis=2)
        assert not bad.any(), what + (int(bad.sum()), int(np.nonzero(bad[0])[0][0]))


@pytest.mark.parametrize("k", M.MONTWORD_SIZES)
def test_montgomery_word_ft255_kernel(oracle, ctxs, k):
    """ntt_pass_kernel<8, 10 / 11, 256>, the Ft255 kernel behind qp29 == null: whole transforms in one pass and in two"""
    O = oracle
    cx = ctxs.get(3, k, {})
    n = 1 << k
    x = O.random_elems(3, n, 50 + k).reshape(1, n, 4)
    want = x.copy()
    assert O.lib().lo_fft_io(3, O.ptr(want[0]), k) == 0
    splits = [[(lt, 0, k, 0)] for lt in (10, 11) if k <= lt] + [[(lt, 0, 1, lt - 1), (lt, 1, k - 1, 0)] for lt in (10, 11) if k - 1 <= lt <= k]
    for passes in splits:
        y = x
        for lt, t0, s, ltj in passes:
            what = ("montword", k, lt, t0, s, ltj)
            z = _general_run(O, cx, y, lt, t0, s, ltj, H.F_MONTWORD, what)
            assert (z == M.model_dif(O, 3, y, k, t0, s)).all(), what
            y = z
        assert (y == want).all(), ("montword", k, passes)


# ---- the launchers' refusals -----------------------------------------------------------------------------------------------------------------
REFUSALS = [(0, 0, 12, {}), (0, 3, 13, {"LCPC_NTT_GENERAL": "1"}), (1, 3, 13, {}), (2, 3, 13, {}), (2, 3, 21, {}), (3, 3, 21, {}),
            (4, 3, 12, {"LCPC_NTT_FORM": "coset"}), (4, 3, 17, {}), (4, 3, 19, {}), (5, 1, 13, {}), (5, 0, 13, {})]


@pytest.mark.parametrize("which,fid,k,env", REFUSALS, ids=["%d-ft%d-2^%d" % (w, CM.FIELD_BITS[f], k) for w, f, k, _ in REFUSALS])
def test_launchers_refuse_what_they_document(ctxs, which, fid, k, env):
    """hipErrorInvalidValue, and not a word of dst or copy_dst written"""
    cx = ctxs.get(fid, k, env)
    err, intact = cx.refused(which)
    assert err == H.HIP_ERROR_INVALID_VALUE, (H.REFUSALS[which], err)
    assert intact, H.REFUSALS[which]


def test_harness_refuses_before_the_device():
    """the harness's own checks: sizes that are not exact, flags a step does not have, strides shorter than a row"""
    with H.Ctx(3, 1 << 11, 1 << 12) as cx:
        n, NL = 1 << 12, 8
        src = np.zeros(n * NL, np.uint32)
        for kw in (dict(n_rows=0), dict(dst_stride=n - 1), dict(n_valid=n + 1), dict(flags=H.F_INPLACE), dict(flags=32), dict(src_stride=n // 2),
                   dict(n_rows=2)):
            with pytest.raises(H.BadArgs):
                cx.run_step(0, src, **kw)
        for kw in (dict(flags=H.F_COPY), dict(n_valid=n // 2), dict(n_src_total=5), dict(flags=H.F_INPLACE, dst_stride=n + 1)):
            with pytest.raises(H.BadArgs):
                cx.run_step(1, src, **kw)
        with pytest.raises(H.BadArgs):
            cx.run_step(2, src)
        with pytest.raises(H.BadArgs):
            cx.run_step(1, src, flags=H.F_MID)           # (the source must then be the 9-word records)
        for a in ((10, 0, 6, 5), (12, 0, 12, 0), (9, 0, 9, 0), (10, 5, 8, 0), (10, 0, 0, 0)):
            with pytest.raises(H.BadArgs):
                cx.run_general(src, *a)
        with pytest.raises(H.BadArgs):
            cx.run_general(src, 10, 0, 10, 0, flags=H.F_CANON | H.F_MONTWORD)
        for w in (3, 4, 5, 6):
            with pytest.raises(H.BadArgs):
                cx.refused(w)
    with H.Ctx(0, 1 << 12, 1 << 13) as cx:
        with pytest.raises(H.BadArgs):
            cx.run_step(0, np.zeros((1 << 13) * 2, np.uint32), flags=H.F_MID)
        with pytest.raises(H.BadArgs):
            cx.run_general(np.zeros((1 << 13) * 2, np.uint32), 12, 0, 12, 0, flags=H.F_MONTWORD)

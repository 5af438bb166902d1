"""Range proofs for the lazy (unreduced) dot-product accumulators, as Python integers.  CPU only.

Every fast dot product on the device skips reductions, and each skip rests on a range argument:
  * ln::lazy_mac / lazy_normalize / lazy_reduce (field_ln.h) for Ft255 (LnField<FT255>: 9 limbs of 29 bits, R' = 2^261), called by
    collapse29_kernel (eval_outer / prove), spmv_kernel's lazy branch, spmm_t_terms and spmm_t_tail_kernel (Brakedown SpMM), all with
    a normalise every 6 terms and one REDC per <= 60 terms ("lazy29" below);
  * the same templates for Ft127 / Ft191 (5 / 7 limbs of 29 bits), the Brakedown SpMM of those fields, at the same cadence ("ln");
  * Wide<NL> (field_dev.h wide_mac / wide_reduce, carry-propagating 32-bit words), collapse_kernel and the non-lazy SpMV / SpMM,
    in batches of 8.
Each accumulator is modelled column by column with upper bounds at the exact schedule its callers run (which limbs each operand can
have, the normalise cadence, what normalize leaves in each column, the unmasked top column, the terms per reduction), and the
cadences are read out of the kernel sources, so that changing one fails here until its proof is updated.  The schedule is also
replayed on concrete worst-case operands with the 64-bit wrap-around of the hardware, against the true dot product mod p.

Operand ranges: stored elements are < p (include/lcpc_hip.h: elements always cross as fully reduced Montgomery limbs); a tensor or
matrix value for lazy29 is t * 2^5 mod p (to_r29_kernel: five modular doublings of a value < p), for ln the R'-form v R' mod p
(launch_ntt_lns_roots, fully reduced): every operand of the limb dot products is an integer in [0, p)."""
import os
import re
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
import pyref as P  # noqa: E402

CSRC = os.path.join(ROOT, "lcpc_amd", "csrc")
M64 = (1 << 64) - 1


def _src(name):
    return open(os.path.join(CSRC, name)).read()


def _body(text, head):
    """the text of the function whose definition starts with `head`, up to its closing brace at column 0"""
    i = text.index(head)
    return text[i:text.index("\n}\n", i)]


def _ints(pattern, text):
    """the integer constants matched by the group (\\d+) of `pattern`; a constant may be written `1u << 20`"""
    pattern = pattern.replace(r"(\d+)", r"(\d+)u?(?: << (\d+))?")
    return [int(a) << int(b or 0) for a, b in re.findall(pattern, text)]


# ---- the cadences in the sources -------------------------------------------------------------------------------------------------
def lazy29_cadences():
    """(normalise every, terms per REDC) of every lazy29 / ln caller, read from kernels.hip; each caller must state one value"""
    k = _src("kernels.hip")
    out = {}
    b = _body(k, "__global__ void __launch_bounds__(256) collapse29_kernel(")
    out["collapse29_kernel"] = (_ints(r"\+\+since == (\d+)", b), _ints(r"rb \+= (\d+)", b) + _ints(r"rb \+ (\d+) < r1", b))
    b = _body(k, "__global__ void __launch_bounds__(256) spmv_kernel(")
    # lane sl of an SL-lane group takes every SL-th term: a row of <= T * SL terms gives a lane <= T terms
    out["spmv_kernel"] = (_ints(r"\+\+since == (\d+)", b), _ints(r"k1 - k0 <= (\d+) \* SL", b))
    b = _body(k, "__device__ __forceinline__ Fe<NL> spmm_t_terms(")
    lz = b[:b.index("} else {")]
    out["spmm_t_terms (lazy29)"] = (_ints(r"\+\+since == (\d+)", lz), _ints(r"kb \+= (\d+)", lz) + _ints(r"kb \+ (\d+) < k1", lz))
    ln = b[b.index("ln::LazyN<FT> acc"):b.index("if (!done)")]
    lnh = b[b.index("LnField<NL == 4"):b.index("if (!done)")]
    out["spmm_t_terms (ln)"] = (_ints(r"\+\+since == (\d+)", ln), _ints(r"kb \+= (\d+)", lnh) + _ints(r"kb \+ (\d+) < k1", lnh))
    b = _body(k, "__global__ void __launch_bounds__(256) spmm_t_tail_kernel(")
    out["spmm_t_tail_kernel"] = (_ints(r"\+\+since == (\d+)", b), _ints(r"ib \+= (\d+)", b) + _ints(r"ib \+ (\d+) < maxlen", b))
    return out


def wide_batches():
    k = _src("kernels.hip")
    out = {}
    b = _body(k, "__global__ void __launch_bounds__(256) collapse_kernel(")
    out["collapse_kernel"] = _ints(r"constexpr int BATCH = (\d+);", b)
    b = _body(k, "__global__ void __launch_bounds__(256) spmv_kernel(")
    out["spmv_kernel (Wide)"] = _ints(r"constexpr u32 BATCH = (\d+);", b)
    b = _body(k, "__device__ __forceinline__ Fe<NL> spmm_t_terms(")
    wd = b[b.index("if (!done)"):]
    out["spmm_t_terms (Wide)"] = _ints(r"kb \+= (\d+)", wd) + _ints(r"kb \+ (\d+) < k1", wd)
    return out


def k2_thresholds():
    """what decides which Brakedown (K2) kernel runs and where its lazy path ends, read from kernels.hip / internal.h: launch_spmm_t's
    selection by the number of outputs m (spmm_t_kernel<NL, OPW> from `opw_min_m`; below it spmm_t_sliced_kernel<NL, SL> with SL by
    falling m: m > above[i] takes sliced_sl[i], the rest the last one), the longest last row group the packed-tail kernel takes, the
    lanes per output of spmv_kernel and the terms per lane up to which it stays lazy, and the row count from which the host takes
    the position-major path.  tests/test_k2_cases.py restates the selection on these, so a changed threshold fails there instead of
    silently moving a case to another kernel."""
    k = _src("kernels.hip")
    b = _body(k, "hipError_t launch_spmm_t(int nl")
    one = lambda pat, text: (lambda v: v[0] if len(v) == 1 else pytest.fail("%s: %s" % (pat, v)))(_ints(pat, text))
    out = dict(opw_min_m=one(r"a\.m >= (\d+)\)", b), sliced_above=_ints(r"a\.m > (\d+)\)", b),
               sliced_sl=_ints(r"spmm_t_sliced_kernel<NLV, (\d+)>", b), opw=one(r"spmm_t_kernel<NLV, (\d+)>", b),
               tail_max=one(r"tail <= (\d+)\)", b), rows_per_group=one(r"a\.n_rows & (\d+)\)", b) + 1)
    assert "nl == 8 && a.vals29 != nullptr && tail != 0 && tail <= " in b            # the tail kernel: Ft255 limb path only
    # the batch launcher selects through the same body (the overload that takes the batch rows), each batch form beside its single form
    assert _ints(r"spmm_t_sliced_kernel<NLV, (\d+), true>", b) == out["sliced_sl"] and _ints(r"spmm_t_kernel<NLV, (\d+), true>", b) == [out["opw"]]
    bb = _body(k, "hipError_t launch_spmm_t_batch(int nl")
    assert "return launch_spmm_t(nl, a, st, &b);" in bb and "hipLaunchKernelGGL" not in bb
    b = _body(k, "hipError_t launch_spmv(int nl")
    out["spmv_sl"] = one(r"constexpr int SL = (\d+);", b)
    b = _body(k, "__global__ void __launch_bounds__(256) spmv_kernel(")
    out["spmv_lazy_terms"] = one(r"k1 - k0 <= (\d+) \* SL", b)
    assert "lazy = a.vals29 != nullptr && k1 - k0 <= " in b and "if constexpr (NL == 8) {" in b
    out["t_min_rows"] = one(r"constexpr uint64_t SDIG_T_MIN_ROWS = (\d+);", _src("internal.h"))
    return out


def ln_params():
    """{fid: (N, W, NL)} from field_ln.h's LnField specialisations"""
    t = _src("field_ln.h")
    out = {}
    for name, fid in (("FT63", 0), ("FT127", 1), ("FT191", 2), ("FT255", 3)):
        m = re.search(r"struct LnField<%s> \{\s*static constexpr int FID = %s, N = (\d+), W = (\d+), NL = (\d+)" % (name, name), t)
        out[fid] = tuple(int(v) for v in m.groups())
    return out


# ---- the accumulators --------------------------------------------------------------------------------------------------------------
class LimbAcc:
    """ln::lazy_* (Ft255: N = 9, W = 29, NL = 8): 2N u64 columns, acc[i + j] += x_i v_j, normalize carries columns 0..2N-2 up
    (the top column 2N-1 takes no products and is never masked), reduce = normalize + a column-wise REDC by R' = 2^(N W) with
    quotient digits m_k = -acc mod 2^W (p == 1 mod 2^W), whose N result limbs are masked to W bits and packed into NL words."""

    def __init__(self, fid, N, W, NL):
        self.p, self.N, self.W, self.NL = P.FIELDS[fid].p, N, W, NL
        self.R = 1 << (N * W)
        self.M = (1 << W) - 1
        self.plimb = [(self.p >> (W * k)) & self.M for k in range(N)]
        assert self.p % (1 << W) == 1 and self.plimb[0] == 1       # the negate-and-mask quotient digit
        assert self.p < 1 << (N * W)

    def limbs(self, v):
        """the split of an element < p: N - 1 limbs of W bits, the top limb takes every bit from W (N - 1) up"""
        return [(v >> (self.W * k)) & self.M for k in range(self.N - 1)] + [v >> (self.W * (self.N - 1))]

    def max_limbs(self):
        """limb-wise maxima over [0, p): W-bit low limbs, a top limb of at most (p - 1) >> W (N - 1) (23 bits for Ft255)"""
        return [self.M] * (self.N - 1) + [(self.p - 1) >> (self.W * (self.N - 1))]

    def maximal(self):
        """the largest element whose low N - 1 limbs are all 2^W - 1"""
        s = self.W * (self.N - 1)
        return ((self.p >> s) << s) - 1

    def column_bounds(self, norm_every, n_terms):
        """worst column values over one REDC chunk of n_terms terms of (x < p) * (v < p), normalised every norm_every terms.
        Returns (largest column value ever held, the column bounds REDC starts from)."""
        N, W, M = self.N, self.W, self.M
        lm = self.max_limbs()
        per_term = [sum(lm[i] * lm[k - i] for i in range(N) if 0 <= k - i < N) for k in range(2 * N)]
        c = [0] * (2 * N)
        peak = 0

        def normalize():
            nonlocal peak
            for k in range(2 * N - 1):
                c[k + 1] += c[k] >> W          # monotone: the bound of the carry is the carry of the bound
                c[k] = min(c[k], M)
                peak = max(peak, c[k + 1])

        since = 0
        for _ in range(n_terms):
            for k in range(2 * N):
                c[k] += per_term[k]
            peak = max(peak, max(c))
            since += 1
            if since == norm_every:
                normalize()
                since = 0
        normalize()                            # lazy_reduce's own first step
        return peak, c

    def redc_acc_peak(self, cols):
        """the largest value of REDC's single u64 accumulator, from column bounds (quotient digits <= 2^W - 1)"""
        N, W, M = self.N, self.W, self.M
        acc, peak = 0, 0
        for k in range(2 * N):
            acc += cols[k] + sum(M * self.plimb[k - i] for i in range(N) if i < k and 1 <= k - i < N)
            if k < N:
                acc += M
            peak = max(peak, acc)
            acc >>= W
        return peak

    def redc_out_max(self, n_terms):
        """(largest REDC input, largest REDC output) for n_terms products of values < p: (V + m p) / R' with m < R'"""
        v = n_terms * (self.p - 1) ** 2
        return v, (v + (self.R - 1) * self.p) // self.R

    def max_safe(self, norm_every_max=64, terms_max=4096):
        """the largest normalise cadence (at the derived term count) and the largest term count per REDC for which every column
        stays < 2^64, the REDC accumulator stays < 2^64 and the REDC output stays < 2p"""
        t = 1
        while t < terms_max and self.redc_out_max(t + 1)[1] < 2 * self.p:
            t += 1
        s = 1
        while s < norm_every_max and self._fits(s + 1, t):
            s += 1
        return s, t

    def _fits(self, s, t):
        peak, cols = self.column_bounds(s, t)
        return peak < 1 << 64 and self.redc_acc_peak(cols) < 1 << 64

    # concrete replay with the hardware's wrap-around
    def replay(self, xs, vs, norm_every, terms):
        """sum_k xs[k] vs[k] / R' mod p, computed the way the kernels do: chunks of `terms` terms, each accumulated in 2N
        wrapping u64 columns with a normalise every `norm_every` terms, REDC'd with wrapping u64 arithmetic, masked, packed into
        NL 32-bit words (bits above are lost), reduced once, and the chunk results added mod p (fe_add of values < p)."""
        N, W, M = self.N, self.W, self.M
        total = 0
        for c0 in range(0, len(xs), terms):
            c = [0] * (2 * N)
            since = 0
            for x, v in zip(xs[c0:c0 + terms], vs[c0:c0 + terms]):
                xl, vl = self.limbs(x), self.limbs(v)
                for i in range(N):
                    for j in range(N):
                        c[i + j] = (c[i + j] + xl[i] * vl[j]) & M64
                since += 1
                if since == norm_every:
                    self._norm(c)
                    since = 0
            self._norm(c)
            acc, m, r = 0, [0] * N, [0] * N
            for k in range(2 * N):
                acc = (acc + c[k]) & M64
                for i in range(N):
                    j = k - i
                    if i < k and 1 <= j < N:
                        acc = (acc + m[i] * self.plimb[j]) & M64
                if k < N:
                    m[k] = (-(acc & 0xFFFFFFFF)) & M
                    acc = (acc + m[k]) & M64
                else:
                    r[k - N] = acc & M
                acc >>= W
            t = sum(l << (W * k) for k, l in enumerate(r)) & ((1 << (32 * self.NL)) - 1)
            if t >= self.p:
                t = (t - self.p) & ((1 << (32 * self.NL)) - 1)
            assert t < self.p, "chunk result not reduced: fe_add would take it as an element"
            total = (total + t) % self.p
        return total

    def _norm(self, c):
        for k in range(2 * self.N - 1):
            c[k + 1] = (c[k + 1] + (c[k] >> self.W)) & M64
            c[k] &= self.M


def lazy29():
    return ln_acc(3)


def ln_acc(fid):
    N, W, NL = ln_params()[fid]
    return LimbAcc(fid, N, W, NL)


LIMB_ACCS = {"lazy29 (Ft255)": lazy29, "ln (Ft127)": lambda: ln_acc(1), "ln (Ft191)": lambda: ln_acc(2)}

# derived limits (max_safe): (largest normalise cadence at the largest REDC chunk, largest REDC chunk; 4096 = "at least").  The REDC
# chunk is bound by "output < 2p": T (p - 1)^2 + (R' - 1) p < 2 p R', i.e. 80 terms for Ft255 (the comment's 64 p^2 is a round
# number below it).  The normalise cadence is bound by the middle columns, which take N - 2 products of two full limbs and two with
# the short top limb per term, plus what normalize leaves behind and the carry from below: 8 terms for lazy29 (field_ln.h's
# comment counts 6), and far more for Ft127, whose 12-bit top limb makes the columns short.
DERIVED = {"lazy29 (Ft255)": (8, 80), "ln (Ft127)": (16, 4096), "ln (Ft191)": (10, 4096)}


def test_cadences_are_read_from_the_sources():
    cad = lazy29_cadences()
    for name, (norm, terms) in cad.items():
        assert norm and terms, name
        assert len(set(norm)) == 1 and len(set(terms)) == 1, (name, norm, terms)
    assert {n: (v[0][0], v[1][0]) for n, v in cad.items()} == {
        "collapse29_kernel": (6, 60), "spmv_kernel": (6, 60), "spmm_t_terms (lazy29)": (6, 60), "spmm_t_terms (ln)": (6, 60),
        "spmm_t_tail_kernel": (6, 60)}
    wb = wide_batches()
    assert all(len(set(v)) == 1 for v in wb.values()) and {n: v[0] for n, v in wb.items()} == {
        "collapse_kernel": 8, "spmv_kernel (Wide)": 8, "spmm_t_terms (Wide)": 8}
    assert ln_params() == {0: (3, 26, 2), 1: (5, 29, 4), 2: (7, 29, 6), 3: (9, 29, 8)}
    assert k2_thresholds() == dict(opw_min_m=8192, sliced_above=[2048, 256], sliced_sl=[2, 4, 8], opw=4, tail_max=48, rows_per_group=64,
                                   spmv_sl=8, spmv_lazy_terms=60, t_min_rows=24)


@pytest.mark.parametrize("name", list(LIMB_ACCS))
def test_limb_accumulator_bounds_at_source_cadence(name):
    """columns < 2^64 throughout, REDC input < 64 p^2 (Ft255, field_ln.h lazy_reduce) / < p R' (ln), REDC accumulator < 2^64,
    REDC output < 2p and inside NL words, at the cadence of every caller in kernels.hip"""
    a = LIMB_ACCS[name]()
    callers = {n: (v[0][0], v[1][0]) for n, v in lazy29_cadences().items() if ("(ln)" in n) == name.startswith("ln")}
    assert callers
    for caller, (norm, terms) in callers.items():
        peak, cols = a.column_bounds(norm, terms)
        assert peak < 1 << 64, (caller, peak.bit_length())
        assert cols[2 * a.N - 1] < 1 << 64
        assert a.redc_acc_peak(cols) < 1 << 64, caller
        v, out = a.redc_out_max(terms)
        if name.startswith("lazy29"):
            assert v < 64 * a.p ** 2, caller
        assert v < a.p * a.R, caller
        assert out < 2 * a.p <= 1 << (32 * a.NL), caller
        # the comments' arithmetic: 6 terms of <= N products of two full limbs
        assert norm * a.N * (a.M ** 2) < 1 << 64


@pytest.mark.parametrize("name", list(LIMB_ACCS))
def test_limb_accumulator_derived_limits(name):
    """the largest safe cadence, derived; the sources' cadence does not exceed it"""
    a = LIMB_ACCS[name]()
    s, t = a.max_safe()
    assert (s, t) == DERIVED[name]
    # one step past each limit breaks the bound it is limited by
    assert a.redc_out_max(t + 1)[1] >= 2 * a.p or t == 4096
    assert not a._fits(s + 1, t) or s == 64
    for caller, (norm, terms) in lazy29_cadences().items():
        if ("(ln)" in caller) == name.startswith("ln"):
            assert norm[0] <= s and terms[0] <= t, caller
            assert a._fits(norm[0], terms[0])


def _worst_operands(a, kind):
    """x: coefficient elements, v: tensor / matrix values in the form the kernel multiplies (both < p)"""
    big = a.maximal()
    assert big < a.p and all(l == a.M for l in a.limbs(big)[:-1])
    return {"maximal limbs": big, "p - 1": a.p - 1}[kind]


@pytest.mark.parametrize("name", list(LIMB_ACCS))
@pytest.mark.parametrize("kind", ["maximal limbs", "p - 1", "mixed"])
def test_limb_accumulator_replay(name, kind):
    """the kernels' schedule on concrete worst-case operands, with u64 wrap-around: the true dot product mod p, at 1, 6, 7, 59, 60,
    61, 120 and 121 terms (normalise and REDC boundaries)"""
    import random
    a = LIMB_ACCS[name]()
    rnd = random.Random(hash(name) & 0xFFFF)
    norm, terms = 6, 60
    for n in (1, 6, 7, 59, 60, 61, 120, 121):
        if kind == "mixed":
            pool = [_worst_operands(a, "maximal limbs"), a.p - 1]
            xs = [rnd.choice(pool) if rnd.random() < 0.8 else rnd.randrange(a.p) for _ in range(n)]
            vs = [rnd.choice(pool) if rnd.random() < 0.8 else rnd.randrange(a.p) for _ in range(n)]
        else:
            xs = vs = [_worst_operands(a, kind)] * n
        want = sum(x * v for x, v in zip(xs, vs)) * pow(a.R, -1, a.p) % a.p
        assert a.replay(xs, vs, norm, terms) == want, n


def test_lazy29_replay_catches_wrong_cadences():
    """the replay is not vacuous: past the derived limits the worst operands give a wrong value (a middle column wraps at 2^64 with
    a normalise every 12 terms; the REDC output passes 2p with one REDC per 256 terms)"""
    a = lazy29()
    x = _worst_operands(a, "maximal limbs")
    want = lambda n: n * x * x * pow(a.R, -1, a.p) % a.p
    assert a.replay([x] * 60, [x] * 60, 12, 60) != want(60)
    assert a.replay([x] * 256, [x] * 256, 6, 1 << 20) != want(256)
    assert a.replay([x] * 256, [x] * 256, 6, 60) == want(256)


# ---- Wide<NL> -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fid", [0, 1, 2, 3])
def test_wide_accumulator_bounds(fid):
    """wide_mac is exact (carries propagate into 2 NL + 1 words), so a batch of B products < p^2 must fit 2 NL + 1 words; wide_reduce
    REDCs the low 2 NL words and keeps the result as (top word : NL words), then subtracts p while it is >= p: the result must fit
    NL + 1 words (top is a u32).  The batch of 8 of collapse_kernel / spmv_kernel / spmm_t_terms, and the derived largest batch."""
    p = P.FIELDS[fid].p
    NL = {0: 2, 1: 4, 2: 6, 3: 8}[fid]
    R = 1 << (32 * NL)

    def ok(b):
        v = b * (p - 1) ** 2
        out = (v + (R - 1) * p) // R
        return v < 1 << (32 * (2 * NL + 1)) and out < 1 << (32 * (NL + 1))

    for caller, batches in wide_batches().items():
        batch = batches[0]
        assert ok(batch), caller
        out = (batch * (p - 1) ** 2 + (R - 1) * p) // R
        assert out // p <= 8, caller                 # at most 8 trips of the subtraction loop
    lo, hi = 8, 1 << 40                              # largest safe batch: binary search
    while lo < hi:
        mid = (lo + hi + 1) // 2
        lo, hi = (mid, hi) if ok(mid) else (lo, mid - 1)
    assert lo >= 1 << 30                             # the loop's bound, not the words, limits it; 8 is far inside


# ---- the stage construction of test_gpu_lazy_worst.test_ntt_extremes_at_every_stage ----------------------------------------------------
@pytest.mark.parametrize("fid", [0, 3])
def test_dif_stage_restatement_and_stage_inputs(fid):
    """tests/common.py dif_stage, all stages in order, is the oracle's row NTT (lo_fft_io) and pyref.fft_io at 2^12; and
    row_with_stage_input gives a row whose values entering stage s are the pattern on the first half, for every s"""
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    import common as CM
    import oracle_lib as O
    log_n, p = 12, CM.field_p(fid)
    n, w = 1 << log_n, CM.ntt_root(fid, log_n)
    L = CM.FIELD_L[fid]
    import random
    rnd = random.Random(5)
    x = [rnd.randrange(p) for _ in range(n // 2)] + [0] * (n // 2)
    full = list(x)
    for k in range(log_n):
        CM.dif_stage(full, k, w, p)
    assert full == P.fft_io(P.FIELDS[fid], list(x))
    arr = CM.to_limbs(x, L)
    O.lib().lo_fft_io(fid, O.ptr(arr), log_n)
    assert [CM.to_int(v) for v in arr] == full
    back = list(full)
    for k in range(log_n - 1, -1, -1):
        CM.dif_stage(back, k, w, p, inverse=True)
    assert back == x
    for pat in ([p - 1], [0, p - 1], [CM.ntt_maxlimb(fid)]):
        for s in range(log_n):
            row = CM.row_with_stage_input(fid, log_n, s, pat) + [0] * (n // 2)
            for k in range(s):
                CM.dif_stage(row, k, w, p)
            assert all(row[i] == pat[i % len(pat)] for i in range(n // 2)), s


@pytest.mark.parametrize("fid", [0, 1, 2, 3])
@pytest.mark.parametrize("log_n", [10, 11, 12])
def test_stage_input_builder(fid, log_n):
    """tests/common.py stage_input_rows (one oracle lo_dif_stage call per stage over all rows) equals row_with_stage_input at rate
    1/2 for every stage and pattern; at rates 1/2 and 1/4 the forward stages 0 .. s-1 of its row (free prefix, zeros after) put
    the pattern on the free prefix"""
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    import common as CM
    p, n, L = CM.field_p(fid), 1 << log_n, CM.FIELD_L[fid]
    w = CM.ntt_root(fid, log_n)
    for pat in ([p - 1], [0, p - 1], [CM.ntt_maxlimb(fid)]):
        for log_rate in (1, 2):
            m = n >> log_rate
            rows = CM.stage_input_rows(fid, log_n, range(log_n), pat, log_rate)
            assert rows.shape == (log_n, m, L)
            for s in range(log_n):
                x = [CM.to_int(v) for v in rows[s]]
                if log_rate == 1:
                    assert x == CM.row_with_stage_input(fid, log_n, s, pat), (pat, s)
                row = x + [0] * (n - m)
                for k in range(s):
                    CM.dif_stage(row, k, w, p)
                assert all(row[i] == pat[i % len(pat)] for i in range(m)), (pat, log_rate, s)


@pytest.mark.parametrize("fid", [0, 1, 2, 3])
def test_dif_stages_compose_to_the_oracle_ntt(fid):
    """lo_dif_stage over stages 0 .. log n - 1 is lo_fft_io at 2^16 (a random row and two rows at once), and the inverse stages
    in reverse order give the row back"""
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    import oracle_lib as O
    import numpy as np
    log_n, n = 16, 1 << 16
    x = O.random_elems(fid, 2 * n, 77 + fid)
    want = x.copy()
    for r in range(2):
        O.lib().lo_fft_io(fid, O.ptr(want[r * n:]), log_n)
    y = x.copy()
    for k in range(log_n):
        assert O.lib().lo_dif_stage(fid, O.ptr(y), 2 * n, log_n, k, 0, 4) == 0
    assert (y == want).all()
    for k in range(log_n - 1, -1, -1):
        assert O.lib().lo_dif_stage(fid, O.ptr(y), 2 * n, log_n, k, 1, 4) == 0
    assert (y == x).all()
    assert O.lib().lo_dif_stage(fid, O.ptr(y), n // 2 + 1, log_n, 1, 0, 1) != 0     # not whole blocks


def test_ntt_worst_cases_reach_every_instantiation():
    """the shape matrix of test_gpu_lazy_worst.test_ntt_extremes_at_every_stage, through the restated plan choice (tests/common.py
    ntt_plan: ctx.cpp plan_passes, build_limb_plan, ntt_mid_rows, kernels.h *_supported), launches every first-pass template
    S = 1 .. 10 of K1s (limb intermediate on and off) and of K1n (Ft63, Ft127, Ft191), both last-pass variants (blk0_gone, and the
    limb intermediate for K1s), the three-pass first passes S = 1, 2 of every field and each field's one-pass general plan"""
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    import common as CM
    cases = CM.ntt_worst_cases()
    ids = [CM.ntt_case_id(*c) for c in cases]
    assert len(set(ids)) == len(ids)
    assert [c for c in cases if c[2] == 1 and c[4] is None and (c[0], c[1], c[3]) in CM.NTT_LEGACY] == \
        [(f, k, 1, g, None) for f, k, g in CM.NTT_LEGACY]
    reached = set()
    for fid, log_n, log_rate, general, mid_mb in cases:
        reached |= CM.ntt_instantiations(fid, CM.ntt_plan(fid, log_n, general, mid_mb), log_n)
    missing = sorted(CM.ntt_required_instantiations() - reached)
    assert not missing, "not reached: %s" % missing


def test_ntt_plan_restatement():
    """spot values of the restated plan choice: FIRST_TWO_PASS matches plan_passes, K1s at 2^19 / 2^20 keeps two passes on
    1024-element tiles (the general kernel takes 2048), the limb intermediate is on by default only up to 2^15 and LCPC_NTT_MID_MAX_MB=64 batches
    rows from 2^17 on, blk0_gone from a first pass of 8 stages (not for Ft63), three passes of s0, 10, 10 stages from 2^21"""
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    import common as CM
    for fid, k0 in CM.FIRST_TWO_PASS.items():
        assert len(CM.general_passes(fid, k0 - 1)) == 1 and len(CM.general_passes(fid, k0)) == 2
    assert CM.general_passes(3, 20) == [(0, 10, 0, 10), (10, 10, 0, 10)] and CM.general_passes(3, 20, True) == [(0, 9, 2, 11), (9, 11, 0, 11)]
    assert [CM.ntt_plan(3, k)[0]["mid"] > 0 for k in (15, 16)] == [True, False]
    assert CM.ntt_mid_rows(3, 16, 2, 16, 64) == 16 and CM.ntt_mid_rows(3, 17, 2, 17, 64) == 9 and CM.ntt_mid_rows(3, 18, 2, 18, 64) == 6 and CM.ntt_mid_rows(3, 20, 2, 3, 64) == 1
    assert CM.ntt_mid_rows(3, 13, 2, 5, 0) == 0
    for fid in range(4):
        assert [p["blk0_gone"] for p in CM.ntt_plan(fid, 17)] == [False, False]
        assert [p["blk0_gone"] for p in CM.ntt_plan(fid, 18)] == [False, fid != 0]
        assert [(p["t0"], p["s"], p["first"]) for p in CM.ntt_plan(fid, 22)] == [(0, 2, True), (2, 10, True), (12, 10, False)]

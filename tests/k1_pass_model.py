"""An exact model of ONE pass of the Ligero row NTT (K1), for tests/test_k1_pass_cases.py (CPU) and tests/test_gpu_k1_passes.py, which
launch the pass kernels one at a time through tests/native/k1p_harness.cpp.  No tolerances anywhere: residues are compared as integers.

What a pass computes.  Stored (Montgomery) residues transform like the values, the twiddles being plain residues, so every model
works on the limbs as they are stored:
  * DIF passes (the general kernel, K1n, K1s in the DIF form): stages [t0, t0 + s) of the (sub-)row, one at a time, through the oracle's
    lo_dif_stage -- the call tests/common.py stage_input_rows builds its rows with.  The last two passes of a three-pass plan run on
    sub-rows of 2^20 elements, back to back.
  * K1s pure first pass: a 2^S-point DIF on every column b (elements b + 1024 i), no twist.  K1s coset last pass: tile t (it holds the
    frequencies k1 = rev_S(t)) multiplies its element b by w^(k1 b) and runs a 1024-point DIF.  These two are tests/ntt_coset_rules.py's
    run_pure and run_coset; up to 2^12 columns the models are ALSO computed by those two and by common.dif_stage in Python integers.

How a pass stores it (the representation rule, mont_mask_after).  With Montgomery output every stored residue is value x R.  With
canonical output (a.roots29c) the conversion rides on the twiddle multiplies, so after t stages exactly "block 0", the elements
[0, n / 2^t) of a row that never met a multiplier, are still value x R and everything else is the value itself:
  * the general lazy-limb kernel (kernels.hip ntt_pass_l9_kernel, Ft255) leaves block 0 after each pass and reduces the prefix the trivial
    last stages leave (mont_prefix = 4, or 2 after a radix-2 tail) at the final pass's store;
  * K1s / K1n first passes (ntt_l9s.hip, ntt_lns.hip) leave block 0 = [0, n >> S) -- unless the pass has a uniform round (Shape::RU:
    S >= 8, and ln::has_mul_u: not Ft63), whose predecessor converts the pure sum too: then nothing is left and the next pass is told
    so (blk0_gone).  The last pass (S = 10) has such a round for Ft127 / Ft191 / Ft255; Ft63 reduces its 4-element prefix at the store;
  * a three-pass plan's first pass (S = 1, 2) leaves block 0 = [0, 2^20) = sub-row 0 of each row, which is what canon_row_mask selects
    for the two sub-row passes; the middle pass (S = 10) leaves nothing (Ft63: the first 1024 elements);
  * K1s pure first pass: round RC converts its pure sum as well (S = 1, 3: the radix-2 round, S = 2: the I-only round), so nothing is
    left and the coset pass always runs with blk0_gone.
The rule is checked against the plan's own fields (blk0_gone, mont_prefix, canon_row_mask) in check_plan_fields.

Stored forms.  The general kernel stores fully reduced values after every pass; a K1s first pass stores packed values in
[0, p + 2^239), a K1n first pass in [0, p + 64 B) with B = 2^(W (N - 1)); every last pass is fully reduced.  K1s's limb intermediate
`mid` holds 9 signed 29-bit limbs per element, normalised (limbs 0 .. 7 in [0, 2^29)), with |value| < 4p in the DIF form and < 12.04p
in the pure / coset form (mid_bound), per row as the successor's tiles: [tile of 1024 elements][limbs 0-3 x 1024 | limbs 4-7 x 1024 |
limb 8 x 1024] (ntt_l9s.hip)."""
import numpy as np

import common as CM
import ntt_coset_rules as NR

M64 = (1 << 64) - 1
TILE = 1024
N_THREADS = 16


# ---- numpy integers of K 64-bit words, (n, K) uint64 little-endian ---------------------------------------------------------------------
def _const(v, K):
    assert 0 <= v < 1 << (64 * K)
    return [np.array([(v >> (64 * i)) & M64], np.uint64) for i in range(K)]


def ge_const(a, v):
    """a >= v, per row"""
    K = a.shape[1]
    if v >= 1 << (64 * K):
        return np.zeros(len(a), bool)
    c = _const(v, K)
    ge, open_ = np.ones(len(a), bool), np.ones(len(a), bool)
    for i in range(K - 1, -1, -1):
        gt, lt = a[:, i] > c[i], a[:, i] < c[i]
        ge = np.where(open_ & lt, False, ge)
        open_ &= ~(gt | lt)
    return ge


def sub_const_where(a, v, mask):
    """a - v in the rows of mask (which must hold a >= v), a elsewhere"""
    K = a.shape[1]
    c = _const(v, K)
    out = a.copy()
    borrow = np.zeros(len(a), np.uint64)
    for i in range(K):
        x = a[:, i]
        d = x - c[i]
        d2 = d - borrow
        nb = (x < c[i]) | (d < borrow)
        out[:, i] = np.where(mask, d2, x)
        borrow = nb.astype(np.uint64)
    return out


def reduce_once(a, p):
    """a mod p for a < 2p"""
    return sub_const_where(a, p, ge_const(a, p))


def to_ints(a):
    return [sum(int(x) << (64 * i) for i, x in enumerate(r)) for r in a]


def words_to_limbs(words, L):
    """(n x 2L) uint32 words -> (n, L) uint64"""
    return np.ascontiguousarray(words, np.uint32).reshape(-1, 2 * L).view(np.uint64)


def limbs_to_words(limbs):
    return np.ascontiguousarray(limbs, np.uint64).view(np.uint32).reshape(-1)


# ---- the limb intermediate ----------------------------------------------------------------------------------------------------------
def mid_decode(words, n_rows, log_n):
    """the records of n_rows rows of 2^log_n elements -> (n_rows, n, 9) int32 limbs in element order"""
    t = np.ascontiguousarray(words, np.uint32).reshape(n_rows, (1 << log_n) // TILE, 9 * TILE)
    lo = t[:, :, :4 * TILE].reshape(n_rows, -1, TILE, 4)
    hi = t[:, :, 4 * TILE:8 * TILE].reshape(n_rows, -1, TILE, 4)
    top = t[:, :, 8 * TILE:].reshape(n_rows, -1, TILE, 1)
    return np.concatenate([lo, hi, top], axis=3).reshape(n_rows, 1 << log_n, 9).view(np.int32)


def mid_encode(limbs):
    """(n_rows, n, 9) int32 limbs -> the records, flat uint32"""
    n_rows, n = limbs.shape[:2]
    t = np.ascontiguousarray(limbs, np.int32).view(np.uint32).reshape(n_rows, n // TILE, TILE, 9)
    out = np.empty((n_rows, n // TILE, 9 * TILE), np.uint32)
    out[:, :, :4 * TILE] = t[:, :, :, 0:4].reshape(n_rows, -1, 4 * TILE)
    out[:, :, 4 * TILE:8 * TILE] = t[:, :, :, 4:8].reshape(n_rows, -1, 4 * TILE)
    out[:, :, 8 * TILE:] = t[:, :, :, 8]
    return out.reshape(-1)


def mid_limbs_of(v):
    """the normalised limbs of a signed integer: limbs 0 .. 7 in [0, 2^29), the top limb floor(v / 2^232)"""
    low = v & ((1 << 232) - 1)
    return [(low >> (29 * i)) & ((1 << 29) - 1) for i in range(8)] + [v >> 232]


def mid_value_int(limbs):
    """one record's value, in Python integers"""
    return sum(int(x) << (29 * i) for i, x in enumerate(limbs))


def mid_bound(p, form):
    """the exclusive bound on |value| of a mid record, as an integer.  DIF form: 4p, invariant I (every slot is a clamped sum, a product
    or a normalised sum of two products).  Pure form: 12.04p -- the I-only round that ends the pure pass clamps c0 only and stores c1, c2,
    c3 normalised as they come out of the butterfly (|c1| < 10.8p, 12.04p behind an ln::mul2 round; |c2|, |c3| < 8.72p); the coset pass
    is built for exactly that (ntt_l9s.hip: round 0 clamps x0 and multiplies x1 .. x3, normalised with |value| < 12.1p, by ln::mul_u)"""
    return (1204 * p + 99) // 100 if form else 4 * p


def mid_values(limbs, p, bound=None):
    """(n, 9) int32 limbs -> (residues mod p as (n, 4) uint64, normalised per record, |value| < bound per record; bound: 4p unless
    given, at most 16p).  Vectorised: 16p is added limb by limb, the carries are propagated, and the non-negative result below 32p is
    packed into five words and reduced"""
    bound = 4 * p if bound is None else bound
    assert 0 < bound <= 16 * p
    l = limbs.reshape(-1, 9).astype(np.int64)
    mask = (1 << 29) - 1
    norm = ((l[:, :8] >= 0) & (l[:, :8] <= mask)).all(axis=1)
    t = l + np.array(mid_limbs_of(16 * p), np.int64)
    for i in range(8):
        t[:, i + 1] += t[:, i] >> 29
        t[:, i] &= mask
    nonneg = t[:, 8] >= 0
    t[:, 8] = np.where(nonneg, t[:, 8], 0)
    u = t.astype(np.uint64)
    w = np.zeros((len(u), 5), np.uint64)
    for i in range(9):
        word, sh = (29 * i) // 64, (29 * i) % 64
        w[:, word] |= u[:, i] << np.uint64(sh)
        if sh + 29 > 64 or i == 8:
            w[:, word + 1] |= u[:, i] >> np.uint64(64 - sh)
    in_range = nonneg & ge_const(w, 16 * p - bound + 1) & ~ge_const(w, 16 * p + bound)
    for m in (16, 8, 4, 2, 1):
        w = sub_const_where(w, m * p, ge_const(w, m * p))
    return np.ascontiguousarray(w[:, :4]), norm, in_range


# ---- the plan, restated ---------------------------------------------------------------------------------------------------------------
class RStep:
    """one step of a plan as ctx.cpp plans it (plan_passes, build_limb_plan), with the attribute names of k1p_harness.Step"""
    FIELDS = ("kind", "first", "log_n", "t0", "s", "log_tj", "log_tile", "form", "mont_prefix", "blk0_gone", "canon_row_mask")

    def __init__(self, **kw):
        for f in self.FIELDS:
            setattr(self, f, kw[f])

    def __repr__(self):
        return "RStep(%s)" % ", ".join("%s=%r" % (f, getattr(self, f)) for f in self.FIELDS)


def restated_steps(fid, log_n, general=False, form=None):
    """form: LCPC_NTT_FORM ("dif", "coset" or None = unset)"""
    k = log_n
    gp = CM.general_passes(fid, k, general)
    plan = CM.ntt_plan(fid, k, general)
    if plan[0]["kernel"] == "general":
        return [RStep(kind="general", first=False, log_n=k, t0=t0, s=s, log_tj=ltj, log_tile=lt, form=0, blk0_gone=0, canon_row_mask=0,
                      mont_prefix=(4 if s % 2 == 0 else 2) if t0 + s == k else 0) for t0, s, ltj, lt in gp]
    n_pass, s0 = len(plan), plan[0]["s"]
    nf = fid == 3 and n_pass == 2 and (form == "coset" or (form is None and s0 >= 6))
    out = []
    for i, p in enumerate(plan):
        sub, last = n_pass == 3 and i > 0, i + 1 == n_pass
        ln = 20 if sub else k
        out.append(RStep(kind=p["kernel"], first=not last, log_n=ln, t0=ln - 10 if last else 0, s=p["s"], log_tj=10 - p["s"], log_tile=0,
                         form=int(nf), mont_prefix=4 if last and fid == 0 else 0, blk0_gone=int(p["blk0_gone"] or (nf and last)),
                         canon_row_mask=(1 << (k - 20)) - 1 if sub else 0))
    return out


def stages_done(steps, i):
    """row stages finished after step i"""
    return sum(st.s for st in steps[:i + 1])


def mont_mask_after(fid, log_n, steps, i, canonical):
    """(n,) bool: the elements of a row whose stored residue is value x R after step i (i = -1: the job's source)"""
    n = 1 << log_n
    m = np.zeros(n, bool)
    if not canonical or i < 0:
        m[:] = True
        return m
    st, last = steps[i], i + 1 == len(steps)
    blk0 = n >> stages_done(steps, i)
    if last or st.form == 1:
        return m
    if st.kind != "general" and fid != 0 and st.s >= 8:          # a uniform round: the round before it converts the pure sum
        return m
    m[:blk0] = True
    return m


def check_plan_fields(fid, log_n, steps):
    """the plan's own statements about what is left in Montgomery form, held to mont_mask_after"""
    for i, st in enumerate(steps):
        before = mont_mask_after(fid, log_n, steps, i - 1, True)
        last = i + 1 == len(steps)
        if st.kind != "general" and i > 0:
            assert bool(st.blk0_gone) == (fid != 0 and not before.any()), (i, st)
            # the never-multiplied elements a sub-row pass may meet lie in the sub-rows canon_row_mask selects
            per = 1 << st.log_n
            assert st.canon_row_mask == (1 << (log_n - st.log_n)) - 1 and int(before.sum()) <= per, (i, st)
        else:
            assert st.blk0_gone == 0 and st.canon_row_mask == 0
        # what the last pass's own multiplies cannot reach is reduced at the store
        if last and (st.kind == "general" or fid == 0):
            assert st.mont_prefix == (2 if st.kind == "general" and st.s % 2 else 4), (i, st)
        else:
            assert st.mont_prefix == 0, (i, st)
    assert not mont_mask_after(fid, log_n, steps, len(steps) - 1, True).any()
    assert mont_mask_after(fid, log_n, steps, len(steps) - 1, False).all()


def store_bound(fid, kind, is_last):
    """the exclusive bound of a pass's stored packed values"""
    p = CM.field_p(fid)
    if kind == "general" or is_last:
        return p
    if kind == "K1s":
        return p + (1 << 239)
    N, W = CM.LN_SHAPE[fid]
    return p + (64 << (W * (N - 1)))


# ---- one pass on stored limbs, through the oracle ---------------------------------------------------------------------------------------
def _stage(O, fid, x, log_n, t):
    assert O.lib().lo_dif_stage(fid, O.ptr(x), x.size // x.shape[-1], log_n, t, 0, N_THREADS) == 0


def model_dif(O, fid, x, log_n, t0, s):
    """stages [t0, t0 + s) of the 2^log_n-point DIF on every consecutive run of 2^log_n elements of x (..., L)"""
    y = np.ascontiguousarray(x).copy()
    for t in range(t0, t0 + s):
        _stage(O, fid, y, log_n, t)
    return y


def model_pure(O, fid, x, log_n):
    """x: (rows, n, L).  A 2^S-point DIF on every column of 1024-element stride"""
    rows, n, L = x.shape
    S = log_n - 10
    y = np.ascontiguousarray(x.reshape(rows, 1 << S, TILE, L).transpose(0, 2, 1, 3))
    for t in range(S):
        _stage(O, fid, y, S, t)
    return np.ascontiguousarray(y.transpose(0, 2, 1, 3)).reshape(rows, n, L)


def twist_table(O, fid, log_n):
    """(n, L): element (t << 10) + b holds w^(rev_S(t) b), Montgomery form"""
    n, S, L = 1 << log_n, log_n - 10, CM.FIELD_L[fid]
    half = np.zeros((n // 2, L), np.uint64)
    assert O.lib().lo_roots_table(fid, log_n, O.ptr(half)) == 0
    neg = np.zeros_like(half)
    O.lib().lo_f_sub(fid, O.ptr(np.zeros_like(half)), O.ptr(half), O.ptr(neg), n // 2)
    full = np.concatenate([half, neg])                              # w^i, i < n
    k1 = np.array([NR.brev(t, S) for t in range(1 << S)], np.uint64)
    e = (k1[:, None] * np.arange(TILE, dtype=np.uint64)[None, :]) & np.uint64(n - 1)
    return np.ascontiguousarray(full[e.reshape(-1)])


def model_coset(O, fid, x, log_n, twist=None):
    rows, n, L = x.shape
    tw = twist_table(O, fid, log_n) if twist is None else twist
    y = np.empty_like(x)
    for r in range(rows):
        _elementwise(O.lib().lo_f_mul, fid, y[r], np.ascontiguousarray(x[r]), tw)
    for t in range(10):
        _stage(O, fid, y, 10, t)
    return y


def model_step(O, fid, st, x, twist=None):
    """step st on x (rows, n, L), the whole rows of the context; a sub-row step sees them as rows << (log_n - st.log_n) sub-rows"""
    if st.kind == "K1s" and st.form == 1:
        return model_pure(O, fid, x, st.log_n) if st.first else model_coset(O, fid, x, st.log_n, twist)
    return model_dif(O, fid, x, st.log_n, st.t0, st.s)


def model_step_ints(fid, st, row):
    """the same on ONE row of Python integers (up to 2^12 columns: two-pass and one-pass plans only)"""
    p, k = CM.field_p(fid), st.log_n
    assert len(row) == 1 << k and k <= 12
    w = CM.ntt_root(fid, k)
    x = list(row)
    if st.kind == "K1s" and st.form == 1:
        fourth = pow(w, (1 << k) // 4, p)
        return (NR.run_pure if st.first else NR.run_coset)(x, k, 10, w, p, fourth)
    for t in range(st.t0, st.t0 + st.s):
        CM.dif_stage(x, t, w, p)
    return x


def _elementwise(fn, fid, out, *ins):
    """an elementwise call of the oracle, fn(fid, ins..., out, count), over N_THREADS slices of (elements, L) arrays (ctypes releases the GIL)"""
    import ctypes as C
    from concurrent.futures import ThreadPoolExecutor
    L = out.shape[-1]
    n = out.size // L
    step = -(-n // N_THREADS)
    if n < 1 << 14:
        fn(fid, *[C.c_void_p(a.ctypes.data) for a in ins], C.c_void_p(out.ctypes.data), n)
        return out

    def part(lo):
        cnt = min(step, n - lo)
        fn(fid, *[C.c_void_p(a.ctypes.data + lo * L * 8) for a in ins], C.c_void_p(out.ctypes.data + lo * L * 8), cnt)
    with ThreadPoolExecutor(N_THREADS) as ex:
        list(ex.map(part, range(0, n, step)))
    return out


def to_repr(O, fid, x):
    return _elementwise(O.lib().lo_f_to_repr, fid, np.empty_like(x), np.ascontiguousarray(x))


def from_canon(O, fid, x):
    return _elementwise(O.lib().lo_f_from_canon, fid, np.empty_like(x), np.ascontiguousarray(x))


def stored_to_mont(O, fid, res, mask):
    """reduced stored residues (rows, n, L) -> the Montgomery limbs the models work on: canonical elements (mask False) times R"""
    if mask.all():
        return res
    return np.where(mask[None, :, None], res, from_canon(O, fid, res))


def mont_to_stored(O, fid, y, mask):
    if mask.all():
        return y
    return np.where(mask[None, :, None], y, to_repr(O, fid, y))


def padded_source(src, n_rows, n, src_stride, n_valid, n_src_total, L):
    """what a first pass reads: element g of row r is src[r * src_stride + g] if g < n_valid and the flat index < n_src_total, else 0.
    src: (elements, L) -- at least the elements that may be read"""
    out = np.zeros((n_rows, n, L), np.uint64)
    for r in range(n_rows):
        hi = min(n_valid, max(0, min(n_src_total, len(src)) - r * src_stride))
        out[r, :hi] = src[r * src_stride:r * src_stride + hi]
    return out


# ---- the case list -----------------------------------------------------------------------------------------------------------------------
def k1s_plans(log_n):
    """the (LCPC_NTT_FORM, LCPC_NTT_MUL) plans of tests/test_gpu_ntt_reg_store.py plans() -- its LCPC_NTT_MID_MAX_MB settings are the
    limb intermediate forced on (64) and off (0), which every K1s case here runs both of -- and, from 2^16 columns on, where the default
    form is the coset one, the DIF form as well (the only way to a DIF first pass with S >= 6 on two-pass rows)"""
    import test_gpu_ntt_reg_store as RS
    seen, out = set(), []
    for env in RS.plans(log_n):
        e = {k: v for k, v in env.items() if k != "LCPC_NTT_MID_MAX_MB"}
        key = tuple(sorted(e.items()))
        if key not in seen:
            seen.add(key)
            out.append(e)
    if log_n >= 16:
        out.append({"LCPC_NTT_FORM": "dif"})
    return out


def plan_cases():
    """(id, fid, log_n, env, general): every context whose whole plan is run step by step"""
    out = []
    for k in range(11, 21):
        for env in k1s_plans(k):
            tag = "-".join(v for _, v in sorted(env.items())) or "default"
            out.append(("K1s-2^%d-%s" % (k, tag), 3, k, env, False))
    for fid in (0, 1, 2):
        for k in range(CM.FIRST_TWO_PASS[fid], 21):
            out.append(("K1n-ft%d-2^%d" % (CM.FIELD_BITS[fid], k), fid, k, {}, False))
    for fid in (3, 0, 1, 2):
        for k in (21, 22):
            out.append(("3pass-ft%d-2^%d" % (CM.FIELD_BITS[fid], k), fid, k, {}, False))
    for fid in (3, 0, 1, 2):
        sizes = [max(k for k in range(1, 27) if len(CM.general_passes(fid, k, True)) == 1)]
        sizes += [min(k for k in range(1, 27) if len(CM.general_passes(fid, k, True)) == np_) for np_ in (2, 3)]
        if fid == 1:
            sizes.append(20)                                        # ntt_pass_kernel<4, 12, 1024> with one row
        for k in sizes:
            out.append(("general-ft%d-2^%d" % (CM.FIELD_BITS[fid], k), fid, k, {"LCPC_NTT_GENERAL": "1"}, True))
    return out


def case_rows(log_n):
    """one row and three rows; from 2^21 columns on one row only"""
    return [1] if log_n >= 21 else [1, 3]


def general_instantiation(fid, log_tile, s, log_tj, n_rows, log_n, montword=False):
    """the kernel launch_ntt_pass picks (kernels.hip launch_ntt_pass, launch_ntt_pass_t)"""
    nl = CM.NTT_NL[fid]
    if nl == 8 and not montword:
        return "l9<%d>" % log_tile
    tiles = n_rows << (log_n - s - log_tj)
    bs = 1024 if log_tile >= 12 and tiles <= 256 and s + log_tj >= 12 else 256
    return "ntt_pass_kernel<%d, %d, %d>" % (nl, log_tile, bs)


GENERAL_EXTRA_ROWS = {(0, 12): [1, 300]}                            # Ft63 at 2^12: BS = 1024 with one row, BS = 256 with 300
MONTWORD_SIZES = (10, 11)                                           # the Montgomery-word Ft255 kernel behind qp29 == null
FREE_SPLIT_SIZES = (12, 13, 14)
# the general-kernel instantiations the case list must reach besides common.ntt_required_instantiations()
GENERAL_REQUIRED = {"ntt_pass_kernel<4, 12, 1024>", "ntt_pass_kernel<2, 12, 1024>", "ntt_pass_kernel<2, 12, 256>", "ntt_pass_kernel<8, 10, 256>",
                    "ntt_pass_kernel<8, 11, 256>", "l9<10>", "l9<11>"}


# ---- the saturating runs of tests/test_gpu_k1_saturated.py ---------------------------------------------------------------------------------
SAT_WG_PER_CU = 8                                                   # 32 wave slots per CU / 4 waves: the most 256-thread workgroups a CU holds
SAT_NOMINAL_CUS = 256                                               # the MI355X; the GPU module reads the real count from the device
SAT_MAX_BYTES = 1 << 30                                             # device memory of one launch, all its buffers
SAT_MAX_LOG_N = 20                                                  # (one row of a three-pass plan is 2048 workgroups already)


def sat_tiles(cus):
    """workgroups per launch that fill every CU to the bound and refill every slot at least once"""
    return 2 * cus * SAT_WG_PER_CU


def sat_rows(tiles_per_row, cus):
    """the smallest row count that is odd, no multiple of 3 and reaches sat_tiles: q % n_rows and q / n_rows of the XCD-aware mappings
    then stay off the powers of two, and off the period of the three reference rows"""
    r = -(-sat_tiles(cus) // tiles_per_row)
    while r % 2 == 0 or r % 3 == 0:
        r += 1
    return r


def sat_plan_cases():
    """the contexts of plan_cases() that get a saturating run: all but the three-pass ones; and Ft255 forced general at 2^19 columns,
    the lazy-limb kernel on 2^11-element tiles (l9<11>), which plan_cases() has at 2^21 columns only"""
    return [c for c in plan_cases() if c[2] <= SAT_MAX_LOG_N] + [("general-ft255-2^19", 3, 19, {"LCPC_NTT_GENERAL": "1"}, True)]


def sat_tiles_per_row(fid, log_n, general):
    """workgroups per row, counted in the kernel's own tile: 1024 elements for K1s / K1n, 2^log_tile for the general kernel (whose passes
    launch n >> (s + log_tj) >= n >> log_tile workgroups per row)"""
    plan = CM.ntt_plan(fid, log_n, general)
    if plan[0]["kernel"] != "general":
        return (1 << log_n) >> 10
    return max(1, (1 << log_n) >> max(lt for _, _, _, lt in CM.general_passes(fid, log_n, general)))


def sat_montword_splits(log_n):
    """the passes test_montgomery_word_ft255_kernel runs, as lists of (log_tile, t0, s, log_tj)"""
    k = log_n
    return [[(lt, 0, k, 0)] for lt in (10, 11) if k <= lt] + [[(lt, 0, 1, lt - 1), (lt, 1, k - 1, 0)] for lt in (10, 11) if k - 1 <= lt <= k]


def sat_case_bytes(fid, log_n, general, rows, gap=0, src_extra=0):
    """the most device memory one launch of a saturating case holds: source, dst and copy_dst of rows x (n + gap) packed elements (the
    source and copy_dst with src_extra more per row), and the limb intermediate (36 bytes per element) where the plan has one"""
    n, eb = 1 << log_n, 8 * CM.FIELD_L[fid]
    has_mid = fid == 3 and not general
    return rows * ((n + gap) * eb + 2 * (n + src_extra) * eb + (n * 36 if has_mid else 0))


def sat_reached_instantiations(cus=SAT_NOMINAL_CUS):
    """every kernel instantiation the saturating runs launch, by the names of reached_instantiations()"""
    names = set()
    for _, fid, k, env, general in sat_plan_cases():
        rows = sat_rows(sat_tiles_per_row(fid, k, general), cus)
        for mb in ((0, 64) if fid == 3 and not general else (None,)):
            names |= CM.ntt_instantiations(fid, CM.ntt_plan(fid, k, general, mb, n_rows=rows), k)
        if general:
            for t0, s, ltj, lt in CM.general_passes(fid, k, True):
                names.add(general_instantiation(fid, lt, s, ltj, rows, k))
    for k in MONTWORD_SIZES:
        for passes in sat_montword_splits(k):
            for lt, t0, s, ltj in passes:
                names.add(general_instantiation(3, lt, s, ltj, sat_rows(max(1, (1 << k) >> lt), cus), k, montword=True))
    return names


def sat_required_instantiations():
    """what the saturating runs must reach: the names of common.ntt_required_instantiations() and GENERAL_REQUIRED that exist up to
    2^SAT_MAX_LOG_N columns -- no three-pass first pass -- with the block size the row count selects: a saturating launch has more than
    256 tiles, so every ntt_pass_kernel<NL, 12, 1024> becomes <NL, 12, 256>"""
    req = {x for x in CM.ntt_required_instantiations() if not x.startswith("3pass-")}
    for fid in (0, 1, 2):                                           # K1n first passes shorter than the first two-pass size's: three-pass plans only
        req -= {"K1n-ft%d-first-S%d" % (CM.FIELD_BITS[fid], s) for s in range(1, CM.FIRST_TWO_PASS[fid] - 10)}
    return req | {x.replace(", 1024>", ", 256>") for x in GENERAL_REQUIRED}


# what the saturating runs reach besides: the names the two lists above have no word for (Ft63's last pass, which has no uniform round
# and so one form only; the multi-pass plans of the general kernel; its 2^11 tile for Ft127 and its 2^10 tile for Ft191)
SAT_ALSO = {"K1n-ft63-last-blk0kept", "general-ft63", "general-ft127", "general-ft191", "general-ft255", "ntt_pass_kernel<4, 11, 256>",
            "ntt_pass_kernel<6, 10, 256>"}


def sat_commit_cases():
    """(fid, log_n) of the commits at a saturating row count: the default plan of every field from its first two-pass size to
    2^SAT_MAX_LOG_N columns, and the one-pass sizes 2^5 and 2^10"""
    return [(fid, k) for fid in range(4) for k in [5, 10] + list(range(CM.FIRST_TWO_PASS[fid], SAT_MAX_LOG_N + 1))]


def free_tiles(fid):
    """the tile sizes plan_passes uses for the field: its small and its big one"""
    nl = CM.NTT_NL[fid]
    return (10, 11) if nl >= 6 else ((11, 12) if nl == 4 else (12,))


def free_splits(log_n, log_tile):
    """every (t0, s, log_tj) launch_ntt_pass accepts at this size: s + log_tj <= log_tile, and a tile is no longer than the row.  Any
    (t0, s) chains with (0, t0) and (t0 + s, ...) to a whole transform"""
    return [(t0, s, ltj) for t0 in range(log_n) for s in range(1, min(log_tile, log_n - t0) + 1)
            for ltj in range(0, log_tile - s + 1) if s + ltj <= log_n]


def free_split_features(log_n, t0, s, ltj):
    """which of the general kernel's paths a split takes"""
    f = {"s=1" if s == 1 else ("s odd" if s % 2 else "s even")}
    if log_n - t0 - s < ltj:
        f.add("lb < log_tj")
    if t0 + s == log_n:
        f.add("trivial last stages in a radix-4 round" if s % 2 == 0 else "trivial last stage in the radix-2 tail")
    return f


def reached_instantiations():
    """every kernel instantiation the case list of tests/test_gpu_k1_passes.py launches, by the names of common.ntt_instantiations and
    general_instantiation"""
    names = set()
    for _, fid, k, env, general in plan_cases():
        mids = (0, 64) if fid == 3 and not general and k <= 20 else (None,)
        for mb in mids:
            plan = CM.ntt_plan(fid, k, general, mb, n_rows=1)
            names |= CM.ntt_instantiations(fid, plan, k)
        if general:
            for rows in GENERAL_EXTRA_ROWS.get((fid, k), case_rows(k) if (fid, k) != (1, 20) else [1]):
                for t0, s, ltj, lt in CM.general_passes(fid, k, True):
                    names.add(general_instantiation(fid, lt, s, ltj, rows, k))
    for k in MONTWORD_SIZES:
        for lt in (10, 11):
            if k <= lt:
                names.add(general_instantiation(3, lt, k, 0, 1, k, montword=True))
    for fid in range(4):
        for k in FREE_SPLIT_SIZES:
            for lt in free_tiles(fid):
                for t0, s, ltj in free_splits(k, lt):
                    names.add(general_instantiation(fid, lt, s, ltj, 1, k))
    return names

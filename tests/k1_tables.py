"""The contracts of the tables the Ligero row NTT (K1) reads, as exact Python-integer models and checkers.  No GPU here: the checkers
take arrays (what tests/k1_harness.py copies out of a real context, or what the models below build) and return a list of findings, so
tests/test_k1_table_checks.py can show on the CPU that each of them bites; tests/test_gpu_k1_tables.py holds the product's tables to them.

Who relies on what (lcpc_amd/csrc/field_ln.h):
  ln::mul      its twiddle normalised, in [0, p)                          d_rootsl, d_rootslc, every lane-varying pack entry
  ln::mul2     both entries of its pair normalised, in [0, p)             the split packs: b0 = e 2^-116, b1 = e 2^29
  ln::mul_u    the N shifted multiples balanced(w 2^(W j) mod p)          d_wq_w and the packs' tables at u_off
  ln::clamp    (i - 24) p as normalised signed limbs                      d_qpl
  fe_mul       w^i R mod p, fully reduced                                 d_roots

w is the root of unity of order n = 2^log_n of the (sub-)transform a pass works on, R = 2^(32 NL), R' = 2^(N W).  The index rules of
the pure / coset form are those of tests/ntt_coset_rules.py; the rule of the DIF / K1n packs (ntt_lns.hip ntt_lns_pack_kernel,
ntt_lns_upack_kernel) is restated below (dif_*), and at LBT = 0 it must be ntt_coset_rules' pure rule."""
import numpy as np

import common as CM
import ntt_coset_rules as NR
from test_fe_cases import clamp_table, fld, shifted_multiples  # noqa: F401

MAX_FINDINGS = 8           # per check: the first few are what a failure message needs


class LazyTable(NR.Table):
    """ntt_coset_rules.Table without the n / 2 stored powers: w^ix for ix < n / 2, past that the negated entry"""

    def __init__(self, w, k, p):
        self.p, self.half, self.w, self.memo = p, 1 << (k - 1) if k else 1, w, {}

    def __call__(self, ix):
        assert 0 <= ix < 2 * self.half
        if ix not in self.memo:
            self.memo[ix] = pow(self.w, ix, self.p) if ix < self.half else self.p - pow(self.w, ix - self.half, self.p)
        return self.memo[ix]


class PassDesc:
    """what the checkers need of one pass of a plan (k1_harness.Pass has the same names)"""

    def __init__(self, kind, first, log_n, t0, s, form=0, mul2=0, n_classes=None):
        self.kind, self.first, self.log_n, self.t0, self.s, self.form, self.mul2 = kind, bool(first), log_n, t0, s, form, mul2
        self.n_classes = classes_of(self) if n_classes is None else n_classes


def classes_of(d):
    """ctx.cpp build_limb_plan: a DIF first pass and a coset last pass have one class per tile position"""
    return 1 << (d.log_n - 10) if d.first != bool(d.form) else 1


def has_mul_u(F):
    return F.N >= 5


def u_slot(F):
    return (F.N * F.N + 31) & ~31


# ---- what a pack holds (ntt_ln_dev.h Shape / PureShape / coset_sets; the pack kernels' skips) ---------------------------------------------
def pass_lbt(d):
    return 10 - d.s if d.first and not d.form else 0


def pass_slots(F, d):
    """-> (lane-varying slots [(round_off index, variants of one table, positions)], shifted-multiples tables [(round, position, v)])"""
    if d.form and not d.first:
        return [(r, 3, 4 ** r) for r in (2, 3, 4)], [(r, m, v) for r in (0, 1) for m in range(4 ** r) for v in range(3)]
    S, LBT, u0, nr4 = d.s, pass_lbt(d), d.s & 1, d.s // 2
    slots = [(0, 2, 1 << (S - 1 + LBT))] if u0 else []
    for r in range(nr4):
        if d.t0 + u0 + 2 * r + 2 != d.log_n:                 # (stages k-2, k-1: one wave-uniform twiddle, not packed)
            slots.append((u0 + r, 6, 1 << (S - u0 - 2 * r - 2 + LBT)))
    utabs = []
    if d.form:
        if nr4 >= 3:
            utabs = [(0, jl0, v) for jl0 in range(4) for v in range(3)]
    elif has_mul_u(F) and nr4 >= 4:
        for ru in range(nr4 - 3):
            if d.t0 + u0 + 2 * (3 + ru) + 2 != d.log_n:
                utabs += [(ru, jl0, v) for jl0 in range(4) for v in range(3)]
    return slots, utabs


def pack_heads(F, d, classes):
    """(class, slot, variant, jl) of every record k1h_pack_entries returns for these classes, in its order"""
    nb = 2 if d.mul2 else 1
    out = []
    for c in classes:
        for slot, nv, period in pass_slots(F, d)[0]:
            a = np.empty((nb * nv * period, 4), np.uint32)
            a[:, 0], a[:, 1] = c, slot
            a[:, 2] = np.repeat(np.arange(nb * nv), period)
            a[:, 3] = np.tile(np.arange(period), nb * nv)
            out.append(a)
    return np.concatenate(out) if out else np.zeros((0, 4), np.uint32)


def uniform_heads(F, d, classes):
    return np.array([(c, r, m, v) for c in classes for r, m, v in pass_slots(F, d)[1]], np.uint32).reshape(-1, 4)


# ---- which power of w a slot holds -------------------------------------------------------------------------------------------------------
def dif_r2_exp(d, cls, jl):
    """ntt_lns_pack_kernel, the radix-2 slot: (g1 & gm) << t0, g1 the row index of the pair's first element"""
    LBT = pass_lbt(d)
    lb = d.log_n - d.s if d.first else 0
    lo = cls << LBT if d.first else 0
    g1 = ((jl >> LBT) << lb) | lo | (jl & ((1 << LBT) - 1))
    return (g1 & ((1 << (d.log_n - d.t0 - 1)) - 1)) << d.t0


def _dif_g0(d, cls, r, jl):
    LBT, u0 = pass_lbt(d), d.s & 1
    hb = d.s - (u0 + 2 * r) - 1
    lb = d.log_n - d.s if d.first else 0
    lo = cls << LBT if d.first else 0
    return (NR.quad_index(jl >> LBT, hb) << lb) | lo | (jl & ((1 << LBT) - 1)), hb, lb


def dif_r4_exps(d, cls, r, jl):
    """radix-4 slot r, position jl: (w0, w3, w2) = w^ex, w^(3 ex), w^(2 ex), ex = (g0 & gm0) << t"""
    t = d.t0 + (d.s & 1) + 2 * r
    g0, _, _ = _dif_g0(d, cls, r, jl)
    ex = (g0 & ((1 << (d.log_n - t - 1)) - 1)) << t
    return ex, 3 * ex, 2 * ex


def dif_u_exp(d, cls, ru, jl0, v):
    """ntt_lns_upack_kernel: uniform round ru (radix-4 round 3 + ru), position jl0 < 4: w0, w1 = I w0, w2"""
    r = 3 + ru
    u0 = d.s & 1
    t = d.t0 + u0 + 2 * r
    period = 1 << (d.s - u0 - 2 * r - 2 + pass_lbt(d))
    g0, hb, lb = _dif_g0(d, cls, r, jl0 & (period - 1))
    g1 = g0 + (1 << (hb - 1 + lb))
    gm0 = (1 << (d.log_n - t - 1)) - 1
    return ((g0 & gm0) << t, (g1 & gm0) << t, (g0 & (gm0 >> 1)) << (t + 1))[v]


def entry_exp(d, cls, slot, v, jl):
    """(index into the n-entry table of tab_entry_neg, converting?) of lane-varying entry (slot, v, jl) of class cls; v < NV"""
    k, S = d.log_n, d.s
    if d.form and not d.first:
        return (v + 1) * NR.coset_exp(k, 10, cls, slot, jl), False
    u0 = S & 1
    if u0 and slot == 0:
        return (NR.pure_r2_exp(k, 10, jl) if d.form else dif_r2_exp(d, cls, jl)), v == 1
    r = slot - u0
    ex = NR.pure_r4_exps(k, 10, S, r, jl) if d.form else dif_r4_exps(d, cls, r, jl)
    return ex[v % 3], v >= 3


def uniform_exp(d, cls, rnd, pos, v):
    if d.form and not d.first:
        return (v + 1) * NR.coset_exp(d.log_n, 10, cls, rnd, pos)
    if d.form:
        return NR.pure_u_exps(d.log_n, 10, d.s, pos)[v]
    return dif_u_exp(d, cls, rnd, pos, v)


# ---- values ------------------------------------------------------------------------------------------------------------------------------
def limb_value(F, limbs):
    """the value of N unsigned limbs of W bits"""
    return sum(int(x) << (F.W * k) for k, x in enumerate(limbs))


def signed_value(F, limbs):
    """the value of N limbs of which the top one is a two's-complement word"""
    top = int(limbs[F.N - 1])
    return sum(int(x) << (F.W * k) for k, x in enumerate(limbs[:F.N - 1])) + ((top - (1 << 32) if top >> 31 else top) << (F.W * (F.N - 1)))


def to_limbs(F, v):
    return [(v >> (F.W * k)) & F.M for k in range(F.N)]


def packed_value(words):
    return int.from_bytes(np.ascontiguousarray(words, "<u4").tobytes(), "little")


def is_member(F, x, log_n):
    """x^n == 1 (mod p), n = 2^log_n: the multiplicative group is cyclic, so x is a power of the root w of order n"""
    x %= F.p
    for _ in range(log_n):
        x = x * x % F.p
    return x == 1


def scales(F):
    """(plain, converting): R', R' R^-1 mod p -- for Ft255 2^261 and 2^5"""
    return F.Rl % F.p, F.Rl * F.Rinv % F.p


class _Findings(list):
    def __init__(self):
        list.__init__(self)
        self.dropped = 0

    def add(self, text):
        if len(self) < MAX_FINDINGS:
            self.append(text)
        else:
            self.dropped += 1


def _below(arr, const):
    """rows of unsigned words (least significant first) that are < const, const given as words of the same width"""
    lt = np.zeros(len(arr), bool)
    eq = np.ones(len(arr), bool)
    for k in range(arr.shape[1] - 1, -1, -1):
        lt |= eq & (arr[:, k] < const[k])
        eq &= arr[:, k] == const[k]
    return lt


def _first(mask):
    return [int(i) for i in np.flatnonzero(mask)[:MAX_FINDINGS]]


# ---- checkers: the twiddle, clamp and fourth-root tables ------------------------------------------------------------------------------------
def check_roots(F, w, arr, idx, first=0, name="d_roots"):
    """d_roots[i] == w^i R mod p, fully reduced.  arr: entries [first, first + len) as NL packed words; every entry must be < p, the
    entries idx (absolute) are compared exactly"""
    out = _Findings()
    pw = np.array([(F.p >> (32 * k)) & 0xFFFFFFFF for k in range(F.NL)], np.uint32)
    for i in _first(~_below(arr, pw)):
        out.add("%s[%d]: not below p" % (name, first + i))
    for i in idx:
        got, want = packed_value(arr[i - first]), pow(w, i, F.p) * F.R % F.p
        if got != want:
            out.add("%s[%d]: %#x, expected w^%d R mod p = %#x%s" % (name, i, got, i, want, " (same residue)" if (got - want) % F.p == 0 else ""))
    return out


def check_limb_repr(F, arr, first=0, name="d_rootsl"):
    """every entry of a limb-form table: limbs < 2^W, value < p, words N .. STRIDE zero"""
    out = _Findings()
    for i, k in zip(*(a[:MAX_FINDINGS] for a in np.nonzero(arr[:, :F.N] > F.M))):
        out.add("%s[%d]: limb %d = %#x is not below 2^%d" % (name, first + i, k, arr[i, k], F.W))
    for i, k in zip(*(a[:MAX_FINDINGS] for a in np.nonzero(arr[:, F.N:]))):
        out.add("%s[%d]: pad word %d = %#x is not zero" % (name, first + i, F.N + k, arr[i, F.N + k]))
    pl = np.array(to_limbs(F, F.p), np.uint32)
    for i in _first(~_below(arr[:, :F.N], pl) & ~(arr[:, :F.N] > F.M).any(axis=1)):
        out.add("%s[%d]: value is not below p" % (name, first + i))
    return out


def check_limb_table(F, w, arr, idx, conv, first=0, name="d_rootsl", step=1):
    """a limb-form twiddle table: the representation of every entry, and entry i == the limbs of w^(i step) c mod p for i in idx
    (absolute; c = R', or with conv R' R^-1)"""
    out = check_limb_repr(F, arr, first, name)
    c = scales(F)[1 if conv else 0]
    for i in idx:
        want = pow(w, i * step, F.p) * c % F.p
        got = limb_value(F, arr[i - first, :F.N])
        if got != want or [int(x) for x in arr[i - first, :F.N]] != to_limbs(F, want):
            out.add("%s[%d]: limbs %s, expected those of w^%d c mod p = %#x%s" % (name, i, [hex(int(x)) for x in arr[i - first, :F.N]], i * step, want,
                                                                              " (same residue)" if (got - want) % F.p == 0 else ""))
    return out


def check_subtable(sub, full, s0, name="d_rootsls"):
    """three-pass plans: sub[i] == full[i << s0], every word of every entry"""
    out = _Findings()
    want = full[::1 << s0][:len(sub)]
    if want.shape != sub.shape:
        out.add("%s: %s entries, the full table has %s at stride 2^%d" % (name, sub.shape, want.shape, s0))
        return out
    for i, k in zip(*(a[:MAX_FINDINGS] for a in np.nonzero(sub != want))):
        out.add("%s[%d] word %d: %#x, expected %#x (entry %d of the full table)" % (name, i, k, sub[i, k], want[i, k], i << s0))
    return out


def check_clamp(F, arr, name="d_qpl"):
    """d_qpl == (i - 24) p as normalised signed limbs, all 64 x STRIDE words"""
    out = _Findings()
    want = clamp_table(F)
    if arr.shape != want.shape:
        out.add("%s: shape %s, expected %s" % (name, arr.shape, want.shape))
        return out
    for i, k in zip(*(a[:MAX_FINDINGS] for a in np.nonzero(arr != want))):
        out.add("%s[%d] (q = %d) word %d: %#x, expected %#x" % (name, i, i - 24, k, arr[i, k], want[i, k]))
    return out


def fourth_root(F):
    """w^(n/4) for every n: ROOT_OF_UNITY^(2^(S - 2))"""
    return CM.ntt_root(F.fid, 2)


def check_wq(F, arr, name="d_wq_w"):
    """d_wq_w[:N N] == shifted_multiples(F, I), the rest of its 96 words zero"""
    out = _Findings()
    arr = np.asarray(arr).reshape(-1)
    want = np.zeros(96, np.uint32)
    want[:F.N * F.N] = shifted_multiples(F, fourth_root(F))
    if arr.shape != want.shape:
        out.add("%s: %d words, expected 96" % (name, arr.size))
        return out
    for t in _first(arr != want):
        out.add("%s word %d%s: %#x, expected %#x" % (name, t, " (limb %d of W_%d)" % (t // F.N, t % F.N) if t < F.N * F.N else " (pad)", arr[t], want[t]))
    return out


# ---- checkers: the packs -----------------------------------------------------------------------------------------------------------------
def _where(d, rec):
    return "pass(first=%d s=%d form=%d) class %d slot %d variant %d jl %d" % (d.first, d.s, d.form, rec[0], rec[1], rec[2], rec[3])


def check_pack_entries(F, d, recs, classes, w, exact=True):
    """the lane-varying entries of a pass (k1h_pack_entries records) for `classes`.  Every entry: the records are the ones the pass
    shape names; limbs < 2^W; 0 < value < p; membership ((e / c)^n == 1 for the variant's scale c); with exact, the value named by the
    index rule.  A split pack (d.mul2): variant v < NV is b0 == e 2^-116, NV + v is b1 == e 2^29 of the entry e the rule names."""
    out = _Findings()
    heads = pack_heads(F, d, classes)
    if heads.shape != recs[:, :4].shape or (heads != recs[:, :4]).any():
        out.add("pass(first=%d s=%d form=%d): the records are not those of the pass shape (%d records, expected %d)" % (d.first, d.s, d.form, len(recs), len(heads)))
        return out
    for i, k in zip(*(a[:MAX_FINDINGS] for a in np.nonzero(recs[:, 4:] > F.M))):
        out.add("%s: limb %d = %#x is not below 2^%d" % (_where(d, recs[i]), k, recs[i, 4 + k], F.W))
    tab = LazyTable(w, d.log_n, F.p)
    nv_of = {slot: nv for slot, nv, _ in pass_slots(F, d)[0]}
    c_plain, c_conv = scales(F)
    inv = {False: pow(c_plain, -1, F.p), True: pow(c_conv, -1, F.p)}
    k0, k1 = pow(2, -116, F.p), pow(2, 29, F.p)
    kinv = (1, pow(k0, -1, F.p), pow(k1, -1, F.p))
    member = {}
    lim = recs[:, 4:].tolist()
    for i, (cls, slot, v, jl) in enumerate(recs[:, :4].tolist()):
        nv = nv_of[slot]
        half = 0 if not d.mul2 else (1 if v < nv else 2)     # 0: the entry itself; 1: b0; 2: b1
        ix, conv = entry_exp(d, cls, slot, v % nv, jl)
        got = sum(x << (F.W * k) for k, x in enumerate(lim[i]))
        if not 0 < got < F.p:
            out.add("%s: value %#x is not in (0, p)" % (_where(d, recs[i]), got))
        key = (got, conv, half)
        if key not in member:
            member[key] = is_member(F, got * kinv[half] * inv[conv], d.log_n)
        if not member[key]:
            out.add("%s: (entry / scale)^n != 1 -- not a power of w in this variant's form" % _where(d, recs[i]))
        if exact:
            e = tab(ix) * (c_conv if conv else c_plain) % F.p
            want = (e, e * k0 % F.p, e * k1 % F.p)[half]
            if got != want:
                out.add("%s: %#x, expected %s of w^%d (table index %d) = %#x%s" % (
                    _where(d, recs[i]), got, ("the entry", "b0 = e 2^-116", "b1 = e 2^29")[half], ix, ix, want,
                    " (same residue)" if (got - want) % F.p == 0 else (" (the negated value)" if (got + want) % F.p == 0 else "")))
    return out


def check_uniform(F, d, recs, classes, w, exact=True):
    """the shifted-multiples tables of a pass (k1h_uniform records): words N^2 .. U_SLOT zero; the N multiples V_j with limbs 0 .. N-2
    in [0, 2^W) and a signed top limb, -(p-1)/2 <= V_j <= (p-1)/2, V_j == V_0 2^(W j) (mod p), V_0^n == 1; with exact, the table equals
    shifted_multiples(F, w^ix) word for word at the index the rule names"""
    out = _Findings()
    heads = uniform_heads(F, d, classes)
    if heads.shape != recs[:, :4].shape or (heads != recs[:, :4]).any():
        out.add("pass(first=%d s=%d form=%d): the tables are not those of the pass shape (%d, expected %d)" % (d.first, d.s, d.form, len(recs), len(heads)))
        return out
    N, NN = F.N, F.N * F.N
    tab = LazyTable(w, d.log_n, F.p)
    hi = (F.p - 1) // 2
    for i, (cls, rnd, pos, v) in enumerate(recs[:, :4].tolist()):
        words = recs[i, 4:]
        where = "pass(first=%d s=%d form=%d) class %d round %d position %d v %d" % (d.first, d.s, d.form, cls, rnd, pos, v)
        for t in _first(words[NN:] != 0):
            out.add("%s: pad word %d = %#x is not zero" % (where, NN + t, words[NN + t]))
        V = []
        for j in range(N):
            limbs = [int(words[N * k + j]) for k in range(N)]
            for k in range(N - 1):
                if limbs[k] > F.M:
                    out.add("%s: limb %d of W_%d = %#x is not below 2^%d" % (where, k, j, limbs[k], F.W))
            V.append(signed_value(F, limbs))
            if not -hi <= V[j] <= hi:
                out.add("%s: W_%d = %d is outside the balanced range (%+.3f p)" % (where, j, V[j], V[j] / F.p))
            if (V[j] - (V[0] << (F.W * j))) % F.p:
                out.add("%s: W_%d is not W_0 2^(%d) mod p" % (where, j, F.W * j))
        if not is_member(F, V[0], d.log_n):
            out.add("%s: W_0^n != 1 -- not a power of w" % where)
        if exact:
            ix = uniform_exp(d, cls, rnd, pos, v)
            want = shifted_multiples(F, tab(ix))
            for t in range(NN):
                if int(words[t]) != want[t]:
                    out.add("%s word %d (limb %d of W_%d): %#x, expected %#x of w^%d" % (where, t, t // N, t % N, words[t], want[t], ix))
                    break
    return out


# ---- models: the arrays a correct builder leaves (for the tests of the checkers, and as a second statement of the layout) ------------------
def model_roots(F, w, n):
    return np.array([[(pow(w, i, F.p) * F.R % F.p >> (32 * k)) & 0xFFFFFFFF for k in range(F.NL)] for i in range(n)], np.uint32)


def model_limb_table(F, w, n, conv):
    c = scales(F)[1 if conv else 0]
    t = np.zeros((n, F.STRIDE), np.uint32)
    for i in range(n):
        t[i, :F.N] = to_limbs(F, pow(w, i, F.p) * c % F.p)
    return t


def model_wq(F):
    t = np.zeros(96, np.uint32)
    t[:F.N * F.N] = shifted_multiples(F, fourth_root(F))
    return t


def model_pack_entries(F, d, classes, w, table=None):
    """the records of k1h_pack_entries for a correct pack; table: the n-entry twiddle table (default: LazyTable)"""
    tab = table or LazyTable(w, d.log_n, F.p)
    heads = pack_heads(F, d, classes)
    nv_of = {slot: nv for slot, nv, _ in pass_slots(F, d)[0]}
    c_plain, c_conv = scales(F)
    k0, k1 = pow(2, -116, F.p), pow(2, 29, F.p)
    recs = np.zeros((len(heads), 4 + F.N), np.uint32)
    recs[:, :4] = heads
    for i, (cls, slot, v, jl) in enumerate(heads.tolist()):
        nv = nv_of[slot]
        ix, conv = entry_exp(d, cls, slot, v % nv, jl)
        e = tab(ix) * (c_conv if conv else c_plain) % F.p
        if d.mul2:
            e = e * (k0 if v < nv else k1) % F.p
        recs[i, 4:] = to_limbs(F, e)
    return recs


def model_uniform(F, d, classes, w):
    tab = LazyTable(w, d.log_n, F.p)
    heads = uniform_heads(F, d, classes)
    recs = np.zeros((len(heads), 4 + u_slot(F)), np.uint32)
    recs[:, :4] = heads
    for i, (cls, rnd, pos, v) in enumerate(heads.tolist()):
        recs[i, 4:4 + F.N * F.N] = shifted_multiples(F, tab(uniform_exp(d, cls, rnd, pos, v)))
    return recs


# ---- what a test samples -----------------------------------------------------------------------------------------------------------------
def sample_classes(n_classes, seed):
    """every class of a pass with at most 16; else class 0, 1, the last, the one with alternating bits, and 12 seeded ones"""
    import random
    if n_classes <= 16:
        return list(range(n_classes))
    alt = int("01" * 16, 2) & (n_classes - 1)
    fixed = [0, 1, n_classes - 1, alt]
    rng = random.Random("k1 classes %s" % (seed,))
    rest = [c for c in rng.sample(range(n_classes), 16) if c not in fixed][:12]
    return fixed + rest


def sample_indices(n_entries, log_n, seed, full_to=14):
    """every entry of a table up to 2^full_to columns; above, i in {0, 1, 2, n/4 - 1, n/4, n/2 - 1} and 4096 seeded indices"""
    import random
    if log_n <= full_to:
        return list(range(n_entries))
    n = 1 << log_n
    fixed = [i for i in (0, 1, 2, n // 4 - 1, n // 4, n // 2 - 1) if 0 <= i < n_entries]
    rng = random.Random("k1 indices %s" % (seed,))
    return sorted(set(fixed + [rng.randrange(n_entries) for _ in range(4096)]))

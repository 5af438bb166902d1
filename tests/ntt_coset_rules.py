"""The index rules of K1s's pure / coset form (lcpc_amd/csrc/ntt_l9s.hip, NttPassArgs.form == 1), restated in plain Python: which
power of the row's root w each pack slot holds (lcpc_amd/csrc/ntt_lns.hip: ntt_lns_pack_kernel at LBT = 0, l9s_pure_upack_kernel,
coset_exp / l9s_coset_pack_kernel / l9s_coset_upack_kernel) and which slot a quad of the pass kernel reads.  `lt` is log2 of the
tile (10 in the kernels; the model test shrinks it), k = log2 n_cols, S = k - lt the first pass's stage count.

A transform on top of these rules (run) is what tests/test_ntt_coset_model.py holds to the direct DFT."""


def brev(x, bits):
    return int(format(x, "0%db" % bits)[::-1], 2) if bits else 0


class Table:
    """the twiddle table as the device holds it: w^i for i < n / 2; past that the negated entry (ntt_lns.hip tab_entry_neg)"""

    def __init__(self, w, k, p):
        self.p, self.half = p, 1 << (k - 1)
        self.t = [1] * self.half
        for i in range(1, self.half):
            self.t[i] = self.t[i - 1] * w % p

    def __call__(self, ix):
        assert 0 <= ix < 2 * self.half
        return self.t[ix] if ix < self.half else self.p - self.t[ix - self.half]


# ---- pure first pass: a 2^S-point DIF per column, element stride 2^lt ----------------------------------------------------------------
def pure_shape(S):
    """(U0, NR4, sets per radix-4 round, RU, RC) -- ntt_ln_dev.h PureShape"""
    u0, nr4 = S & 1, S // 2
    sets = [1 << (S - u0 - 2 * r - 2) for r in range(nr4)]
    ru = nr4 - 2 if nr4 >= 3 else -1
    rc = nr4 - 3 if nr4 >= 3 else (0 if nr4 == 2 else -1)
    return u0, nr4, sets, ru, rc


def pure_r2_exp(k, lt, i):
    """radix-2 slot, pair index i < 2^(S-1): (g1 & gm) << t0 with g1 = i << lb, lb = lt, t0 = 0"""
    return ((i << lt) & ((1 << (k - 1)) - 1))


def pure_r4_exps(k, lt, S, r, jl):
    """radix-4 slot r, position jl < sets(r): (w0, w3, w2) = w^ex, w^(3 ex), w^(2 ex), ex = (g0 & gm0) << u, g0 = jl << lt"""
    u = (S & 1) + 2 * r
    ex = ((jl << lt) & ((1 << (k - u - 1)) - 1)) << u
    return ex, 3 * ex, 2 * ex


def pure_u_exps(k, lt, S, jl0):
    """the uniform round's tables for position jl0 < 4: (w0, w1 = I w0, w2) -- l9s_pure_upack_kernel"""
    u0, nr4, _, ru, _ = pure_shape(S)
    u = u0 + 2 * ru
    hb = S - u - 1
    gm0 = (1 << (k - u - 1)) - 1
    g0 = jl0 << lt
    g1 = g0 + (1 << (hb - 1 + lt))
    return (g0 & gm0) << u, (g1 & gm0) << u, (g0 & (gm0 >> 1)) << (u + 1)


def quad_index(j, hb):
    """first element of quad j of a round whose quarter distance is 2^(hb - 1) (the kernels' i0; coset pass: e0)"""
    return ((j >> (hb - 1)) << (hb + 1)) | (j & ((1 << (hb - 1)) - 1))


# ---- coset last pass --------------------------------------------------------------------------------------------------------------------
def coset_exp(k, lt, cls, r, m):
    """round r, sub-block m < 4^r of tile class cls: E with w1 = w^E, w2 = w^(2 E), w3 = w^(3 E) -- ntt_lns.hip coset_exp"""
    S = k - lt
    k1 = brev(cls, S)
    return (k1 + (brev(m, 2 * r) << S)) << (lt - 2 - 2 * r)


def run_pure(x, k, lt, w, p, fourth):
    """the pure first pass alone on a row x of n = 2^k residues, in place: a 2^S-point DIF on every column b (elements b + (i << lt))"""
    S, T = k - lt, 1 << lt
    tab = Table(w, k, p)
    u0, nr4, sets, ru, _ = pure_shape(S)
    for b in range(T):                                   # column b: elements b + (i << lt)
        def at(i):
            return b + (i << lt)
        if u0:
            half = 1 << (S - 1)
            for i in range(half):
                a, c = x[at(i)], x[at(i + half)]
                x[at(i)], x[at(i + half)] = (a + c) % p, (a - c) * tab(pure_r2_exp(k, lt, i)) % p
        for r in range(nr4):
            hb = S - u0 - 2 * r - 1
            d = 1 << (hb - 1)
            for j in range(1 << (S - 2)):
                i0 = quad_index(j, hb)
                x0, x1, x2, x3 = (x[at(i0 + c * d)] for c in range(4))
                jl = j & (sets[r] - 1)
                if sets[r] == 1:                         # the I-only round
                    b2, t = x0 - x2, (x1 - x3) * fourth
                    c = [x0 + x2 + x1 + x3, x0 + x2 - x1 - x3, b2 + t, b2 - t]
                elif r == ru:                            # the uniform round: four multiplies by the tables of position j mod 4
                    e0, e1, e2 = pure_u_exps(k, lt, S, jl)
                    b2, b3 = (x0 - x2) * tab(e0), (x1 - x3) * tab(e1)
                    c = [x0 + x2 + x1 + x3, (x0 + x2 - x1 - x3) * tab(e2), b2 + b3, (b2 - b3) * tab(e2)]
                else:
                    e0, e3, e2 = pure_r4_exps(k, lt, S, r, jl)
                    t, f = (x1 - x3) * fourth, x0 - x2
                    c = [x0 + x2 + x1 + x3, (x0 + x2 - x1 - x3) * tab(e2), (f + t) * tab(e0), (f - t) * tab(e3)]
                for cc in range(4):
                    x[at(i0 + cc * d)] = c[cc] % p
    return x


def run_coset(x, k, lt, w, p, fourth):
    """the coset-form last pass alone, in place on what run_pure left: tile t evaluates its 2^lt coefficients on w^rev_S(t) <w_{2^lt}>"""
    S, T = k - lt, 1 << lt
    tab = Table(w, k, p)
    for tile in range(1 << S):                           # tile: the contiguous elements (tile << lt) + e
        base = tile << lt
        for r in range(lt // 2):
            hb = lt - 1 - 2 * r
            d = 1 << (hb - 1)
            for q in range(T // 4):
                m = q >> (hb - 1)
                e0 = base + quad_index(q, hb)
                E = coset_exp(k, lt, tile, r, m)
                x0 = x[e0]
                p1, p2, p3 = x[e0 + d] * tab(E) % p, x[e0 + 2 * d] * tab(2 * E) % p, x[e0 + 3 * d] * tab(3 * E) % p
                t = (p1 - p3) * fourth
                x[e0], x[e0 + d], x[e0 + 2 * d], x[e0 + 3 * d] = ((x0 + p2 + p1 + p3) % p, (x0 + p2 - p1 - p3) % p,
                                                                   (x0 - p2 + t) % p, (x0 - p2 - t) % p)
    return x


def run(x, k, lt, w, p, fourth):
    """the two passes on a row x of n = 2^k residues, in place; fourth = w^(n/4).  Returns x (the reference's order: bit-reversed)."""
    return run_coset(run_pure(x, k, lt, w, p, fourth), k, lt, w, p, fourth)

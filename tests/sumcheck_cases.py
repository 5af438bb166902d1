"""Shared by tests/test_sumcheck_abi.py, tests/test_k18_cases.py, tests/test_gpu_k18_kernels.py and tests/test_gpu_sumcheck.py: the
operand sets, the term lists and the Python bignum model of include/lcpc_hip_sumcheck.h -- the binding of a variable, the round
sums of a composition and the interpolation of the round polynomial from its values at 0 .. d, on canonical Python ints mod p -- and
the ctypes calls of the host entry points with canaries around their outputs.  Everything is exact."""
import ctypes as C

import numpy as np

from lcpc_amd import _lib

import fft_cases as FC

FIELDS = FC.FIELDS
CANARY = FC.CANARY
ERR_ARG = FC.ERR_ARG
vp = FC.vp
ORDERS = ("low", "high")
PAD = 8                                              # canary elements in front of and behind an output
SETS = ("random", "max", "zeros", "equal_halves", "descending", "wrap")
# name -> (tables, terms); a term is (coefficient or None, table indices).  A coefficient is a canonical int, -1 standing for p - 1
# and "rnd" for a random one (terms_of fills them in)
TERM_LISTS = {
    "a": (1, [(None, [0])]),
    "ab": (2, [(None, [0, 1])]),
    "abc": (3, [(None, [0, 1, 2])]),
    "abcd": (4, [(None, [0, 1, 2, 3])]),
    "aa": (1, [(None, [0, 0])]),
    "eq_ab_minus_c": (4, [(1, [0, 1, 2]), (-1, [0, 3])]),
    "full": (8, [("rnd", [0, 1, 2, 3]), ("rnd", [4, 5]), ("rnd", [6, 7, 0]), ("rnd", [7])]),
}


def terms_of(fid, name):
    """(n_tables, terms) of a TERM_LISTS entry with the coefficients as canonical ints (or None)"""
    F = FC.field(fid)
    rnd = FC.rng("sumcheck-coeff", fid, name)
    n_tables, terms = TERM_LISTS[name]
    return n_tables, [(None if c is None else F.p - 1 if c == -1 else rnd.randrange(F.p) if c == "rnd" else c, list(idx)) for c, idx in terms]


def degree(terms):
    return max(len(idx) for _, idx in terms)


def places(order, i, h):
    """where (lo, hi) of pair i stand in a table of 2 h elements"""
    return (2 * i, 2 * i + 1) if order == "low" else (i, i + h)


def tables(fid, name, order, n_tables, n, *key):
    """n_tables tables of n canonical ints.  "random" has 0, 1 and p - 1 planted; "max": all p - 1; "equal_halves": hi == lo in every
    pair (a zero slope); "descending": lo > hi in every pair (every hi - lo wraps); "wrap": table 0 is all p - 1 and the others all 1,
    so every product that holds table 0 an odd number of times is p - 1 at every t and every step of its sum wraps around p"""
    F = FC.field(fid)
    rnd = FC.rng("sumcheck", fid, name, order, n_tables, n, *key)
    h = n // 2
    out = []
    for j in range(n_tables):
        if name == "max":
            t = [F.p - 1] * n
        elif name == "zeros":
            t = [0] * n
        elif name == "wrap":
            t = [F.p - 1 if j == 0 else 1] * n
        else:
            t = [rnd.randrange(F.p) for _ in range(n)]
            if name == "random" and n >= 8:
                for v in (0, 1, F.p - 1):
                    t[rnd.randrange(n)] = v
            for i in range(h):
                lo, hi = places(order, i, h)
                if name == "equal_halves":
                    t[hi] = t[lo]
                elif name == "descending":
                    a, b = rnd.randrange(F.p), rnd.randrange(F.p)
                    while a == b:
                        b = rnd.randrange(F.p)
                    t[lo], t[hi] = max(a, b), min(a, b)
        out.append(t)
    return out


def bind_ref(fid, order, table, r):
    """out[i] = lo_i + r (hi_i - lo_i)"""
    F = FC.field(fid)
    h = len(table) // 2
    out = []
    for i in range(h):
        lo, hi = places(order, i, h)
        out.append((table[lo] + r * (table[hi] - table[lo])) % F.p)
    return out


def round_ref(fid, order, tabs, terms):
    """evals[t] = sum_i sum_m c_m prod_k ext(tabs[idx_mk], i, t), t = 0 .. d"""
    F = FC.field(fid)
    h, d = len(tabs[0]) // 2, degree(terms)
    evals = [0] * (d + 1)
    for c, idx in terms:
        c = 1 if c is None else c
        for i in range(h):
            lo, hi = places(order, i, h)
            for t in range(d + 1):
                prod = c
                for k in idx:
                    prod = prod * (tabs[k][lo] + t * (tabs[k][hi] - tabs[k][lo])) % F.p
                evals[t] += prod
    return [e % F.p for e in evals]


def composition_sum(fid, tabs, terms):
    """sum over the whole tables of sum_m c_m prod_k tabs[idx_mk][x]"""
    F = FC.field(fid)
    s = 0
    for c, idx in terms:
        for x in range(len(tabs[0])):
            prod = 1 if c is None else c
            for k in idx:
                prod = prod * tabs[k][x] % F.p
            s += prod
    return s % F.p


def interpolate(fid, evals, x):
    """g(x) of the polynomial of degree <= d with g(t) = evals[t], t = 0 .. d (Lagrange)"""
    F = FC.field(fid)
    s = 0
    for t, e in enumerate(evals):
        num = den = 1
        for u in range(len(evals)):
            if u != t:
                num = num * (x - u) % F.p
                den = den * (t - u) % F.p
        s += e * num * pow(den, F.p - 2, F.p)
    return s % F.p


def bitrev_table(table):
    v = len(table).bit_length() - 1
    return [table[FC.rev(i, v)] for i in range(len(table))]


def elem(fid, v):
    """one element: the L Montgomery limbs of a canonical int (None stays None)"""
    return None if v is None else FC.mont(fid, [v])[0].copy()


def c_terms(fid, terms):
    """(lcpcm_term array, n_terms, coefficients as (n_terms, L) limbs or None, d); a None among given coefficients stands for one"""
    arr = (_lib.LcpcmTerm * len(terms))()
    for m, (_, idx) in enumerate(terms):
        arr[m].n_factors = len(idx)
        for k, t in enumerate(idx):
            arr[m].table[k] = t
    cs = None
    if any(c is not None for c, _ in terms):
        cs = FC.mont(fid, [1 if c is None else c for c, _ in terms])
    return arr, len(terms), cs, (degree(terms) if terms else 0)


def wrapper_terms(fid, terms):
    """the terms as lcpc_amd's wrappers take them: (limbs or None, indices), every coefficient given or none"""
    if all(c is None for c, _ in terms):
        return [(None, idx) for _, idx in terms]
    return [(elem(fid, 1 if c is None else c), idx) for c, idx in terms]


def host_bind(fid, order, tab, r, out=None, n=None, expect=0):
    """lcpcm_bind with canaries around the output (unless `out` is given: the in-place call).  order by name or number; r: limbs"""
    L = tab.shape[-1]
    n = tab.shape[0] if n is None else n
    h = max(min(n, tab.shape[0]) // 2, 1)
    o = _lib.SUMCHECK_ORDERS[order] if isinstance(order, str) else order
    buf = np.full((PAD + h + PAD, L), CANARY, np.uint64) if out is None else None
    dst = buf[PAD:PAD + h] if out is None else out
    rc = _lib.lib().lcpcm_bind(fid, o, vp(tab), vp(dst), n, vp(r))
    assert rc == expect, rc
    if buf is not None:
        assert (buf[:PAD] == CANARY).all() and (buf[PAD + h:] == CANARY).all(), "elements around the output were written"
        if expect:
            assert (buf == CANARY).all(), "an output was written on an error"
    return dst[:h]


def host_round(fid, order, tabs, terms, n=None, expect=0, carr=None):
    """lcpcm_round with canaries around evals.  tabs: a list of (n, L) limbs; terms: (canonical coefficient or None, indices), or
    carr = (array, n_terms, coefficient limbs, d) as c_terms returns"""
    L = tabs[0].shape[-1]
    n = tabs[0].shape[0] if n is None else n
    o = _lib.SUMCHECK_ORDERS[order] if isinstance(order, str) else order
    arr, n_terms, cs, d = c_terms(fid, terms) if carr is None else carr
    ptrs = (C.c_void_p * len(tabs))(*[t.ctypes.data for t in tabs])
    buf = np.full((PAD + 5 + PAD, L), CANARY, np.uint64)
    rc = _lib.lib().lcpcm_round(fid, o, ptrs, len(tabs), arr, n_terms, vp(cs), n, vp(buf[PAD:]))
    assert rc == expect, rc
    if expect:
        assert (buf == CANARY).all(), "evals were written on an error"
        return None
    assert (buf[:PAD] == CANARY).all() and (buf[PAD + d + 1:] == CANARY).all(), "elements around evals were written"
    return buf[PAD:PAD + d + 1].copy()


REFUSAL_N = 1 << 12


def refusal_buffer_bytes(lib, h, L):
    """the bytes of each of the buffers device_refusals takes"""
    return REFUSAL_N * 8 * L + lib.lcpcm_round_work_bytes(h, REFUSAL_N, 4) + 64 * 8 * L


def device_refusals(lib, h, fid, buffers):
    """every refusal of the three device calls that takes a context: each is settled before any HIP call.  buffers: six device
    addresses of refusal_buffer_bytes each, aligned, which no refused call reads or writes -- they are real so that every pointer
    handed over, offsets included, stays inside an allocation"""
    F = FC.field(fid)
    L, n = F.L, REFUSAL_N
    eb = 8 * L
    wb = lib.lcpcm_round_work_bytes
    need = wb(h, n, 2)
    assert need > 0 and need % eb == 0
    assert wb(None, n, 1) == 0 and wb(h, 0, 1) == 0 and wb(h, 1, 1) == 0 and wb(h, 3, 1) == 0 and wb(h, n, 0) == 0 and wb(h, n, 5) == 0 and wb(h, 1 << 39, 1) == 0
    last = 0
    for k in range(1, 39):
        assert wb(h, 1 << k, 1) >= max(last, eb) and wb(h, 1 << k, 4) == 4 * wb(h, 1 << k, 1), k
        last = wb(h, 1 << k, 1)
    A, B, OA, OB, EV, WORK = buffers
    at = lambda p, off: p + off
    r = elem(fid, 5)
    big = np.full(L, 0xFFFFFFFFFFFFFFFF, np.uint64)
    terms2 = [(None, [0, 1]), (None, [1])]
    arr, n_terms, _, _ = c_terms(fid, terms2)
    cs = FC.mont(fid, [3, 4])
    bad_cs = cs.copy()
    bad_cs[1] = big

    def ptrs(v):
        return None if v is None else (C.c_void_p * max(len(v), 1))(*v)

    def bind(order=1, i=(A, B), o=(OA, OB), nt=2, n_=n, r_=r, ctx=h):
        return lib.lcpcm_bind_device(ctx, order, ptrs(i), ptrs(o), nt, n_, vp(r_), None)

    def rnd(order=1, i=(A, B), nt=2, t=arr, ntm=n_terms, c=cs, n_=n, ev=EV, work=WORK, bytes_=need, ctx=h):
        return lib.lcpcm_round_device(ctx, order, ptrs(i), nt, t, ntm, vp(c), n_, ev, work, bytes_, None)

    def fused(order=1, i=(A, B), o=(OA, OB), nt=2, t=arr, ntm=n_terms, c=cs, n_=n, r_=r, ev=EV, work=WORK, bytes_=need, ctx=h):
        return lib.lcpcm_bind_round_device(ctx, order, ptrs(i), ptrs(o), nt, t, ntm, vp(c), n_, vp(r_), ev, work, bytes_, None)

    for f in (bind, rnd, fused):
        assert f(ctx=None) == ERR_ARG and f(order=2) == ERR_ARG
        assert f(n_=0) == ERR_ARG and f(n_=1) == ERR_ARG and f(n_=n - 1) == ERR_ARG and f(n_=3 * n // 4) == ERR_ARG and f(n_=1 << 39) == ERR_ARG
        assert f(nt=0) == ERR_ARG and f(nt=9, i=(A,) * 9) == ERR_ARG
        assert f(i=None) == ERR_ARG and f(i=(A, None)) == ERR_ARG and f(i=(A, at(B, 4))) == ERR_ARG
    assert fused(n_=2) == ERR_ARG
    for f in (bind, fused):
        assert f(o=None) == ERR_ARG and f(o=(OA, None)) == ERR_ARG and f(o=(at(OA, 4), OB)) == ERR_ARG
        assert f(r_=None) == ERR_ARG and f(r_=big) == ERR_ARG
        # the overlap rules: low first takes no overlap at all, high first a table's own input as its output and nothing else
        assert f(order=0, o=(A, OB)) == ERR_ARG and f(order=0, o=(OA, B)) == ERR_ARG and f(order=0, o=(A, B)) == ERR_ARG
        assert f(order=1, o=(B, OB)) == ERR_ARG and f(order=1, o=(B, A)) == ERR_ARG                    # another table's input
        assert f(order=1, i=(A, A), o=(A, OB)) == ERR_ARG                                             # in place on an input listed twice
        for order in (0, 1):
            assert f(order=order, o=(at(A, eb), OB)) == ERR_ARG and f(order=order, o=(at(A, n * eb - eb), OB)) == ERR_ARG     # partial
            assert f(order=order, i=(at(OA, eb), B)) == ERR_ARG and f(order=order, o=(at(A, n // 2 * eb), OB)) == ERR_ARG     # the upper half
            assert f(order=order, o=(OA, OA)) == ERR_ARG and f(order=order, o=(OA, at(OA, n // 2 * eb - eb))) == ERR_ARG     # outputs meet
    for f in (rnd, fused):
        assert f(t=None) == ERR_ARG and f(ntm=0) == ERR_ARG and f(ntm=5) == ERR_ARG
        for nf, idx in ((0, 0), (5, 0), (2, 2)):                                                     # n_factors, a table index
            bad = (_lib.LcpcmTerm * 2)()
            bad[0].n_factors, bad[1].n_factors = 1, nf
            bad[1].table[1] = idx
            assert f(t=bad) == ERR_ARG
        assert f(c=bad_cs) == ERR_ARG
        assert f(ev=None) == ERR_ARG and f(ev=at(EV, 4)) == ERR_ARG and f(work=None) == ERR_ARG and f(work=at(WORK, 4)) == ERR_ARG
        assert f(bytes_=0) == ERR_ARG and f(bytes_=eb - 1) == ERR_ARG
        assert f(ev=at(A, eb)) == ERR_ARG and f(ev=at(B, n * eb - eb)) == ERR_ARG and f(work=at(A, n * eb - eb)) == ERR_ARG and f(work=B) == ERR_ARG
        last_work = (need if f is rnd else wb(h, n // 2, 2)) - eb          # (the fused round runs over n / 4 pairs: a shorter workspace)
        assert f(ev=WORK) == ERR_ARG and f(work=at(EV, 2 * eb)) == ERR_ARG and f(ev=at(WORK, last_work)) == ERR_ARG
    assert rnd(bytes_=need - 1) == ERR_ARG and fused(bytes_=wb(h, n // 2, 2) - 1) == ERR_ARG             # (the fused round runs over n / 4 pairs)
    assert wb(h, n // 2, 2) < need
    assert fused(ev=at(OA, eb)) == ERR_ARG and fused(work=at(OB, n // 2 * eb - eb)) == ERR_ARG and fused(o=(OA, EV)) == ERR_ARG

"""The domain extension (include/lcpc_hip_domain.h) on the device, through the C ABI and the Python wrappers: the device forms against
the host forms (themselves held to bignum by tests/test_domain_abi.py), the shift tables' cache, the low-degree extension, the commit
from values on a coset against lcpc_commit_device on the interpolated coefficients, and the values of a commitment.  All comparisons
are for equality."""
import ctypes as C
import functools

import numpy as np
import pytest

import lcpc_amd
from lcpc_amd import LcCommit, LcpcError, LigeroEncoding, SdigEncoding, Transcript, _lib

import domain_cases as DC
import fft_cases as FC
import oracle_lib as O
from common import mk_transcript

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

DEV = "cuda:0"
CANARY = DC.CANARY
ERR_ARG, ERR_STATE = DC.ERR_ARG, DC.ERR_STATE
LOG_NS = (0, 1, 9, 10, 11, 13)


def to_dev(a):
    return torch.from_numpy(np.ascontiguousarray(a).view(np.int64)).to(DEV)


def to_host(t):
    return t.cpu().numpy().view(np.uint64)


def dptr(t, off=0):
    return C.c_void_p(t.data_ptr() + off)


@functools.lru_cache(maxsize=None)
def enc_of(fid):
    return LigeroEncoding.new_from_dims(fid, 64, 128)


def sdig_enc(fid, n_per_row, digest="blake3"):
    _, _, n_cols = O.Encoding.sdig_from_dims(fid, n_per_row, 0, 3, 3).get_dims(n_per_row)
    return SdigEncoding.new_from_dims(fid, n_per_row, n_cols, 3, 3, digest=digest)


def gen(fid):
    return lcpc_amd.generator(fid)


def canaried(rows, L):
    buf = torch.full((rows + 16, L), CANARY, dtype=torch.int64, device=DEV)
    torch.cuda.synchronize()
    return buf


def inner(buf):
    got = to_host(buf)
    assert (got[:8] == CANARY).all() and (got[-8:] == CANARY).all(), "elements around the output were written"
    return got[8:-8]


# ---- the device forms against the host forms ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fid", DC.FIELDS)
def test_coset_device_equals_host(fid):
    """every form, out of place and in place, two vectors, on a stream of its own, the generator and a random shift"""
    enc, L = enc_of(fid), O.limbs(fid)
    st = torch.cuda.Stream(device=DEV)
    for log_n in LOG_NS:
        n = 1 << log_n
        x = np.stack([FC.mont(fid, FC.random_vector(fid, log_n, "ddev", v)) for v in range(2)])
        d_x = to_dev(x)
        for name in ("gen", "random"):
            sl = DC.shift_limbs(fid, DC.shifts(fid, "ddev", log_n)[name])
            for form in DC.FORMS:
                want = np.stack([DC.host_coset_fft(fid, form, sl, x[v], log_n) for v in range(2)])
                buf = canaried(2 * n, L)
                out = buf[8:8 + 2 * n].view(2, n, L)
                assert enc.coset_fft(d_x, sl, form, out=out, stream=st.cuda_stream) is out
                inp = d_x.clone()
                torch.cuda.synchronize()
                assert enc.coset_fft(inp, sl, form, out=inp, stream=st.cuda_stream) is inp
                st.synchronize()
                assert np.array_equal(inner(buf).reshape(2, n, L), want), (form, log_n, name)
                assert np.array_equal(to_host(inp), want), (form, log_n, name, "in place")
                assert np.array_equal(to_host(d_x), x)


@pytest.mark.parametrize("fid", DC.FIELDS)
def test_extend_device_equals_host(fid):
    enc, L = enc_of(fid), O.limbs(fid)
    for log_n in LOG_NS:
        n = 1 << log_n
        for nc in sorted({n, max(1, n - 1), n // 2 + 1}):
            if DC.ceil_log2(nc) != log_n:
                continue
            c = np.stack([FC.mont(fid, FC.random_vector(fid, log_n, "dext", v)) for v in range(2)])
            d_c = to_dev(c)
            sl = DC.shift_limbs(fid, DC.shifts(fid, "dext", nc)["random"])
            for b in (0, 1, 3) if log_n < 13 else (0, 2):
                log_m = log_n + b
                for order in DC.ORDERS:
                    want = np.stack([DC.host_extend(fid, sl, c[v], nc, log_m, order) for v in range(2)])
                    buf = canaried(2 << log_m, L)
                    out = buf[8:8 + (2 << log_m)].view(2, 1 << log_m, L)
                    assert enc.extend(d_c, sl, log_m, order, n_coeffs=nc, out=out) is out
                    torch.cuda.synchronize()
                    assert np.array_equal(inner(buf).reshape(2, 1 << log_m, L), want), (nc, log_m, order)
            assert np.array_equal(to_host(d_c), c)


def test_shift_table_cache():
    """more keys in a row than the cache holds, then the first again: every table is built (and rebuilt) right"""
    fid = 3
    F = FC.field(fid)
    enc = LigeroEncoding.new_from_dims(fid, 64, 128)        # a context of its own: an empty cache
    rnd = FC.rng("cache")
    keys = [(rnd.randrange(2, F.p), log_n) for log_n in (9, 10, 11, 9, 12, 10, 11, 12, 13, 8)]
    xs = {log_n: FC.mont(fid, FC.random_vector(fid, log_n, "cache")) for _, log_n in keys}
    for s, log_n in keys + keys[:1] + keys[::-1]:
        sl = DC.shift_limbs(fid, s)
        for form in ("fft_io", "ifft_oi"):
            got = to_host(enc.coset_fft(to_dev(xs[log_n]), sl, form))
            assert np.array_equal(got, DC.host_coset_fft(fid, form, sl, xs[log_n], log_n)), (log_n, form)


@pytest.mark.parametrize("fid", (3, 0))
def test_twiddle_and_shift_caches_interleaved(fid):
    """plain and coset transforms alternated on one fresh encoder, six sizes in both directions: twelve twiddle keys through four
    entries and twelve shift keys through eight, on the stamp the two caches share; then the first keys again.  Every result is the
    host form's"""
    L = O.limbs(fid)
    enc = LigeroEncoding.new_from_dims(fid, 64, 128)        # a context of its own: two empty caches
    sl = DC.shift_limbs(fid, FC.rng("caches", fid).randrange(2, FC.field(fid).p))
    log_ns = (1, 2, 3, 4, 5, 6)
    xs = {log_n: FC.mont(fid, FC.random_vector(fid, log_n, "caches")) for log_n in log_ns}
    keys = [(log_n, form) for log_n in log_ns for form in ("fft_io", "ifft_oi")]
    for log_n, form in keys + keys[:3]:
        d_x = to_dev(xs[log_n])
        got = to_host(enc.fft(d_x, form))
        assert np.array_equal(got, FC.host_fft(fid, form, xs[log_n], log_n)), (log_n, form, "plain")
        got = to_host(enc.coset_fft(d_x, sl, form))
        assert np.array_equal(got, DC.host_coset_fft(fid, form, sl, xs[log_n], log_n)), (log_n, form, "coset")
        assert got.shape == (1 << log_n, L)


# ---- the low-degree extension ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fid", DC.FIELDS)
def test_lde(fid):
    F = FC.field(fid)
    enc, L, log_n = enc_of(fid), O.limbs(fid), 8
    n = 1 << log_n
    coeffs = [FC.random_vector(fid, log_n, "lde", v) for v in range(2)]
    sh = DC.shifts(fid, "lde")
    for log_m in (8, 9, 11):
        b = log_m - log_n
        for s_in, s_out in ((None, 1), (None, sh["gen"]), (sh["gen"], sh["random"]), (sh["random"], 1)):
            for in_order, out_order in (("natural", "natural"), ("bitrev", "bitrev"), ("natural", "bitrev")):
                vals = [DC.coset_dft(fid, c, s_in or 1) for c in coeffs]
                x = np.stack([FC.mont(fid, FC.permute(v, log_n) if in_order == "bitrev" else v) for v in vals])
                want = np.stack([FC.mont(fid, DC.extend_fast(fid, c, s_out, log_m, out_order)) for c in coeffs])
                d_x = to_dev(x)
                si = None if s_in is None else DC.shift_limbs(fid, s_in)
                out, work = enc.lde(d_x, log_m, DC.shift_limbs(fid, s_out), shift_in=si, in_order=in_order, out_order=out_order)
                assert np.array_equal(to_host(out), want), (log_m, s_in, s_out, in_order, out_order)
                assert np.array_equal(to_host(work), np.stack([FC.mont(fid, c) for c in coeffs]))       # the coefficients
                assert np.array_equal(to_host(d_x), x)
                if s_in is None and s_out == 1 and in_order == out_order == "natural":
                    assert torch.equal(out[:, ::1 << b], d_x)      # H_n lies in H_m: independent of any transform reference
                out2, work2 = enc.lde(d_x, log_m, DC.shift_limbs(fid, s_out), shift_in=si, in_order=in_order, out_order=out_order, work=d_x)
                assert work2 is d_x and torch.equal(out2, out) and torch.equal(d_x, work)               # work_dev == in_dev
    # refusals: nothing is written
    lib = _lib.lib()
    g = gen(fid)
    d_x = to_dev(FC.mont(fid, coeffs[0]))
    buf = canaried(4 * n, L)
    keep = to_host(d_x).copy()
    eb = 8 * L
    f = lambda *a: lib.lcpcd_lde_device(enc._h, *a)
    o, w = dptr(buf, 8 * eb), dptr(buf, (8 + 2 * n) * eb)
    assert f(0, None, dptr(d_x), log_n, FC.vp(g), log_n + 1, 0, o, dptr(buf, (8 + 2 * n - 1) * eb), 1, None) == ERR_ARG       # work meets out
    assert f(0, None, dptr(d_x), log_n, FC.vp(g), log_n + 1, 0, o, o, 1, None) == ERR_ARG
    assert f(0, None, dptr(buf, (8 + n) * eb), log_n, FC.vp(g), log_n + 1, 0, o, w, 1, None) == ERR_ARG                      # in meets out
    assert f(0, None, dptr(buf, (8 + 2 * n + 1) * eb), log_n, FC.vp(g), log_n + 1, 0, o, w, 1, None) == ERR_ARG              # in meets work, unequal
    assert f(0, None, dptr(d_x), log_n, FC.vp(g), log_n - 1, 0, o, w, 1, None) == ERR_ARG                                    # log_m < log_n
    assert f(2, None, dptr(d_x), log_n, FC.vp(g), log_n, 0, o, w, 1, None) == ERR_ARG and f(0, None, dptr(d_x), log_n, FC.vp(g), log_n, 2, o, w, 1, None) == ERR_ARG
    assert f(0, FC.vp(np.zeros(L, np.uint64)), dptr(d_x), log_n, FC.vp(g), log_n, 0, o, w, 1, None) == ERR_ARG
    assert f(0, None, dptr(d_x), log_n, None, log_n, 0, o, w, 1, None) == ERR_ARG
    assert f(0, None, dptr(d_x), log_n, FC.vp(g), log_n, 0, o, w, 0, None) == ERR_ARG
    assert f(0, None, dptr(d_x), 0, FC.vp(g), 16, 0, o, w, 1, None) == ERR_ARG                                               # 2^16 blocks
    assert f(0, None, dptr(d_x), log_n, FC.vp(g), 33, 0, o, w, 1, None) == ERR_ARG
    assert f(0, None, None, log_n, FC.vp(g), log_n, 0, o, w, 1, None) == ERR_ARG
    torch.cuda.synchronize()
    assert (to_host(buf) == CANARY).all() and np.array_equal(to_host(d_x), keep)


def test_device_refusals():
    """every error is settled before any launch: the outputs keep their canaries"""
    fid, log_n = 3, 6
    F = FC.field(fid)
    lib, enc, n = _lib.lib(), enc_of(fid), 1 << log_n
    g, zero = gen(fid), np.zeros(F.L, np.uint64)
    big = O.ints_to_limbs([F.p], F.L)[0]
    d_x = to_dev(FC.mont(fid, FC.random_vector(fid, log_n, "drefuse")))
    d_o = torch.full((4 * n, F.L), CANARY, dtype=torch.int64, device=DEV)
    torch.cuda.synchronize()
    f = lambda form, s, i, o, ln, nv: lib.lcpcd_coset_fft_device(enc._h, form, FC.vp(s), i, o, ln, nv, None)
    for s in (zero, big, None):
        assert f(1, s, dptr(d_x), dptr(d_o), log_n, 1) == ERR_ARG
    assert lib.lcpcd_coset_fft_device(None, 1, FC.vp(g), dptr(d_x), dptr(d_o), log_n, 1, None) == ERR_ARG
    assert f(6, g, dptr(d_x), dptr(d_o), log_n, 1) == ERR_ARG
    assert f(1, g, None, dptr(d_o), log_n, 1) == ERR_ARG and f(1, g, dptr(d_x), None, log_n, 1) == ERR_ARG
    assert f(1, g, dptr(d_x, 8), dptr(d_o), log_n - 1, 1) == ERR_ARG and f(1, g, dptr(d_x), dptr(d_o, 8), log_n, 1) == ERR_ARG
    assert f(1, g, dptr(d_x), dptr(d_o), 33, 1) == ERR_ARG and f(1, g, dptr(d_x), dptr(d_o), F.S + 1, 1) == ERR_ARG
    assert f(1, g, dptr(d_x), dptr(d_o), log_n, 0) == ERR_ARG and f(1, g, dptr(d_x), dptr(d_o), log_n, 65536) == ERR_ARG
    assert f(1, g, dptr(d_x), dptr(d_o), 32, 128) == ERR_ARG
    assert f(1, g, dptr(d_o), dptr(d_o, 32), log_n, 1) == ERR_ARG and f(1, g, dptr(d_o, 32 * (n - 1)), dptr(d_o), log_n, 1) == ERR_ARG
    x = lambda s, c, nc, lm, order, o, nv: lib.lcpcd_extend_device(enc._h, FC.vp(s), c, nc, lm, order, o, nv, None)
    for s in (zero, big, None):
        assert x(s, dptr(d_x), n, log_n + 1, 0, dptr(d_o), 1) == ERR_ARG
    assert x(g, None, n, log_n + 1, 0, dptr(d_o), 1) == ERR_ARG and x(g, dptr(d_x), n, log_n + 1, 0, None, 1) == ERR_ARG
    assert x(g, dptr(d_x), n, log_n + 1, 2, dptr(d_o), 1) == ERR_ARG
    assert x(g, dptr(d_x), 0, log_n + 1, 0, dptr(d_o), 1) == ERR_ARG and x(g, dptr(d_x), n + 1, log_n, 0, dptr(d_o), 1) == ERR_ARG
    assert x(g, dptr(d_x), n, log_n + 1, 0, dptr(d_o), 0) == ERR_ARG
    assert x(g, dptr(d_x), n, log_n + 16, 0, dptr(d_o), 1) == ERR_ARG                           # 2^16 blocks
    assert x(g, dptr(d_x), 1 << 31, 32, 0, dptr(d_o), 128) == ERR_ARG                          # 2^39 elements
    assert x(g, dptr(d_x), n, 33, 0, dptr(d_o), 1) == ERR_ARG
    assert x(g, dptr(d_x, 8), n, log_n + 1, 0, dptr(d_o), 1) == ERR_ARG and x(g, dptr(d_x), n, log_n + 1, 0, dptr(d_o, 8), 1) == ERR_ARG
    assert x(g, dptr(d_o, 32 * (2 * n - 1)), n, log_n + 1, 0, dptr(d_o), 1) == ERR_ARG            # overlap, in == out included
    assert x(g, dptr(d_o), n, log_n + 1, 0, dptr(d_o), 1) == ERR_ARG
    torch.cuda.synchronize()
    assert (to_host(d_o) == CANARY).all()
    assert x(g, dptr(d_x), n, log_n + 1, 1, dptr(d_o), 1) == 0
    torch.cuda.synchronize()
    assert np.array_equal(to_host(d_o)[:2 * n], DC.host_extend(fid, g, to_host(d_x), n, log_n + 1, "bitrev")) and (to_host(d_o)[2 * n:] == CANARY).all()


# ---- commit from values on a coset ---------------------------------------------------------------------------------------------------------
def same_commitment(a, b):
    assert (a.n_rows, a.n_per_row, a.n_cols, a.n_hashes) == (b.n_rows, b.n_per_row, b.n_cols, b.n_hashes)
    assert a.get_root() == b.get_root()
    assert (a.hashes() == b.hashes()).all()
    assert (a.coeffs() == b.coeffs()).all()
    assert (a.comm() == b.comm()).all()


def commit_coset_matrix(fid, enc, log_ns):
    F = FC.field(fid)
    ref, cm = LcCommit(enc), LcCommit(enc)
    for log_n in log_ns:
        n = 1 << log_n
        coeffs = FC.random_vector(fid, log_n, "cevals")
        s = DC.shifts(fid, "cevals", log_n)["gen" if log_n == log_ns[0] else "random"]
        sl = DC.shift_limbs(fid, s)
        evals = DC.coset_dft(fid, coeffs, s)             # evals[i] = p(s w^i)
        d_c = to_dev(FC.mont(fid, coeffs))
        want = LcCommit.commit_device(d_c.data_ptr(), n, enc, into=ref)
        for order in DC.ORDERS:
            e = FC.mont(fid, evals if order == "natural" else FC.permute(evals, log_n))
            d_e = to_dev(e)
            for src in (d_e, e):
                got = LcCommit.commit_coset_evals(src, sl, enc, order=order, into=cm)
                same_commitment(got, want)
                assert (got.coeffs()[:n] == FC.mont(fid, coeffs)).all() and (got.coeffs()[n:] == 0).all()
            assert np.array_equal(to_host(d_e), e)      # the caller's buffer is only read
        x = FC.rng("cpt", fid, log_n).randrange(F.p)
        outer, inner_t = enc.tensors(FC.mont(fid, [x]), got.n_rows)
        root = got.get_root()
        pf = got.prove(outer, enc, mk_transcript(Transcript, root, enc.get_n_col_opens()))
        ev = pf.verify(root, outer, inner_t, enc, mk_transcript(Transcript, root, enc.get_n_col_opens()))
        assert FC.canon(fid, ev) == [sum(c * pow(x, k, F.p) for k, c in enumerate(coeffs)) % F.p]


@pytest.mark.parametrize("fid", (1, 3))
def test_commit_coset_evals_ligero(fid):
    commit_coset_matrix(fid, enc_of(fid), (12, 10))


@pytest.mark.parametrize("fid", (1, 3))
def test_commit_coset_evals_brakedown(fid):
    commit_coset_matrix(fid, sdig_enc(fid, 40), (12, 10))


def test_commit_coset_evals_sha3():
    commit_coset_matrix(3, LigeroEncoding.new_from_dims(3, 64, 128, digest="sha3_256"), (12, 10))
    commit_coset_matrix(1, sdig_enc(1, 40, "sha3_256"), (10,))


# ---- the values of a commitment -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ("ligero", "brakedown"))
@pytest.mark.parametrize("fid", (1, 3))
def test_commit_values(fid, kind):
    """against lcpcd_extend on lcpc_get_coeffs, and at four sampled points against lcpce_eval in the powers basis; 300 coefficients
    under 64 per row pad to 320, under 40 per row to 320 as well: not a power of two"""
    F = FC.field(fid)
    enc = enc_of(fid) if kind == "ligero" else sdig_enc(fid, 40)
    for n in (300, 1 << 10):
        cm = LcCommit.commit(O.random_elems(fid, n, 9), enc)
        padded = cm.n_rows * cm.n_per_row
        assert padded >= n and (n != 300 or padded & (padded - 1))
        coeffs = cm.coeffs()
        base = DC.ceil_log2(padded)
        for log_m in (base, base + 2):
            for order in DC.ORDERS:
                s = DC.shifts(fid, "vals", n, log_m)["gen" if order == "natural" else "random"]
                sl = DC.shift_limbs(fid, s)
                got = cm.values(sl, log_m, order)
                torch.cuda.synchronize()
                assert np.array_equal(to_host(got), DC.host_extend(fid, sl, coeffs, padded, log_m, order)), (n, log_m, order)
                ks = [0, 1, (1 << log_m) - 1, FC.rng("vk", n, log_m).randrange(1 << log_m)]
                pts = FC.mont(fid, [s * pow(FC.root(fid, log_m), k, F.p) % F.p for k in ks])
                at = [FC.rev(k, log_m) if order == "bitrev" else k for k in ks]
                assert np.array_equal(to_host(got)[at], cm.eval(pts, basis="powers")), (n, log_m, order)
        assert np.array_equal(cm.coeffs(), coeffs)
        buf = canaried(1 << (base - 1), F.L)
        with pytest.raises(LcpcError) as err:
            cm.values(gen(fid), base - 1, out=buf[8:8 + (1 << (base - 1))])      # fewer points than coefficients
        assert err.value.code == lcpc_amd.ERR_ARG
        torch.cuda.synchronize()
        assert (to_host(buf) == CANARY).all()


def test_commit_values_state_and_arguments():
    fid, log_n = 3, 7
    F = FC.field(fid)
    lib, enc = _lib.lib(), enc_of(fid)
    g = gen(fid)
    d_o = torch.full((1 << (log_n + 1), F.L), CANARY, dtype=torch.int64, device=DEV)
    torch.cuda.synchronize()
    v = lambda h, s, lm, order, o: lib.lcpcd_commit_values_device(h, FC.vp(s), lm, order, o, None)
    em = LcCommit(enc)
    assert v(em._h, g, log_n, 0, dptr(d_o)) == ERR_STATE                                          # an empty object
    senc = LigeroEncoding.new(fid, 1 << 12, shard=(0, 2))
    scm = LcCommit(senc)
    assert v(scm._h, g, log_n, 0, dptr(d_o)) == ERR_STATE                                         # a sharded encoder
    e = FC.mont(fid, FC.random_vector(fid, log_n, "vstate"))
    assert lib.lcpcd_commit_coset_evals_device(scm._h, 0, FC.vp(g), dptr(to_dev(e)), log_n, None, None) == ERR_STATE
    assert lib.lcpcd_commit_coset_evals(scm._h, 0, FC.vp(g), FC.vp(e), log_n, None) == ERR_STATE
    cm = LcCommit.commit_coset_evals(e, g, enc)
    root, coeffs = cm.get_root(), cm.coeffs().copy()
    bad = e.copy()
    bad[3] = O.ints_to_limbs([F.p], F.L)[0]
    zero = np.zeros(F.L, np.uint64)
    d_e = to_dev(e)
    calls = (lambda: v(cm._h, zero, log_n, 0, dptr(d_o)), lambda: v(cm._h, None, log_n, 0, dptr(d_o)), lambda: v(cm._h, bad[3], log_n, 0, dptr(d_o)),
             lambda: v(cm._h, g, log_n, 2, dptr(d_o)), lambda: v(cm._h, g, log_n, 0, None), lambda: v(cm._h, g, log_n, 0, dptr(d_o, 8)),
             lambda: v(cm._h, g, 33, 0, dptr(d_o)), lambda: v(cm._h, g, log_n - 1, 0, dptr(d_o)), lambda: v(None, g, log_n, 0, dptr(d_o)),
             lambda: lib.lcpcd_commit_coset_evals_device(cm._h, 0, FC.vp(zero), dptr(d_e), log_n, None, None),
             lambda: lib.lcpcd_commit_coset_evals_device(cm._h, 0, None, dptr(d_e), log_n, None, None),
             lambda: lib.lcpcd_commit_coset_evals_device(cm._h, 2, FC.vp(g), dptr(d_e), log_n, None, None),
             lambda: lib.lcpcd_commit_coset_evals_device(cm._h, 0, FC.vp(g), None, log_n, None, None),
             lambda: lib.lcpcd_commit_coset_evals_device(cm._h, 0, FC.vp(g), dptr(d_e, 8), log_n - 1, None, None),
             lambda: lib.lcpcd_commit_coset_evals_device(cm._h, 0, FC.vp(g), dptr(d_e), 33, None, None),
             lambda: lib.lcpcd_commit_coset_evals(cm._h, 0, FC.vp(bad[3]), FC.vp(e), log_n, None),
             lambda: lib.lcpcd_commit_coset_evals(cm._h, 1, FC.vp(g), FC.vp(bad), log_n, None),
             lambda: lib.lcpcd_commit_coset_evals(cm._h, 0, FC.vp(g), None, log_n, None))
    for k, call in enumerate(calls):
        assert call() == ERR_ARG, k
        assert cm.get_root() == root and (cm.coeffs() == coeffs).all()
    torch.cuda.synchronize()
    assert (to_host(d_o) == CANARY).all()
    got = cm.values(g, log_n + 1, out=d_o)
    torch.cuda.synchronize()
    assert np.array_equal(to_host(got), DC.host_extend(fid, g, coeffs, 1 << log_n, log_n + 1, "natural"))
    assert np.array_equal(to_host(got)[::2], DC.host_coset_fft(fid, "fft_ii", g, coeffs, log_n)) and cm.get_root() == root

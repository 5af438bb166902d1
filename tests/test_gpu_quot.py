"""The quotient extension (include/lcpc_hip_quot.h) on the device, through the C ABI and the Python wrappers: the device forms against
the host forms (themselves held to bignum by tests/test_quot_abi.py), the two chains the extension exists for -- division by the
vanishing polynomial between an extension and a coset inverse, and the opening quotient of a commitment committed to again -- against
bignum polynomial arithmetic, and the refusals.  All comparisons are for equality."""
import ctypes as C
import functools

import numpy as np
import pytest

import lcpc_amd
from lcpc_amd import LcCommit, LcpcError, LigeroEncoding, SdigEncoding, _lib

import domain_cases as DC
import fft_cases as FC
import oracle_lib as O
import quot_cases as QC

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

DEV = "cuda:0"
CANARY = QC.CANARY
ERR_ARG = QC.ERR_ARG
TILE = 4096


def to_dev(a):
    return torch.from_numpy(np.ascontiguousarray(a).view(np.int64)).to(DEV)


def to_host(t):
    return t.cpu().numpy().view(np.uint64)


def dptr(t, off=0):
    return C.c_void_p(t.data_ptr() + off)


@functools.lru_cache(maxsize=None)
def enc_of(fid):
    return LigeroEncoding.new_from_dims(fid, 64, 128)


def sdig_enc(fid, n_per_row):
    _, _, n_cols = O.Encoding.sdig_from_dims(fid, n_per_row, 0, 3, 3).get_dims(n_per_row)
    return SdigEncoding.new_from_dims(fid, n_per_row, n_cols, 3, 3)


def canaried(rows, L):
    buf = torch.full((rows + 16, L), CANARY, dtype=torch.int64, device=DEV)
    torch.cuda.synchronize()
    return buf


def inner(buf):
    got = to_host(buf)
    assert (got[:8] == CANARY).all() and (got[-8:] == CANARY).all(), "elements around the output were written"
    return got[8:-8]


# ---- the device forms against the host forms ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fid", QC.FIELDS)
def test_inverse_and_pointwise_device_equal_host(fid):
    """one tile, a ragged one and several; (n, L) and (n_vecs, n, L); out of place between canaries, out == a and out == b"""
    enc, L = enc_of(fid), O.limbs(fid)
    for n in (100, TILE, 3 * TILE + 17):
        b = FC.mont(fid, QC.operands(fid, "edge_zeros", n, TILE, TILE // 8, "dev"))
        a = FC.mont(fid, QC.operands(fid, "random", n, TILE, TILE // 8, "dev"))
        d_a, d_b = to_dev(a), to_dev(b)
        buf = canaried(n, L)
        out = buf[8:8 + n]
        assert enc.batch_inverse(d_b, out=out) is out
        torch.cuda.synchronize()
        want = QC.host_inverse(fid, b)
        assert np.array_equal(inner(buf), want), n
        inp = d_b.clone()
        assert enc.batch_inverse(inp, out=inp) is inp and np.array_equal(to_host(inp), want)
        for op in QC.OPS:
            want = QC.host_pointwise(fid, op, a, b)
            buf = canaried(n, L)
            enc.pointwise(op, d_a, d_b, out=buf[8:8 + n])
            assert np.array_equal(inner(buf), want), (n, op)
            ia, ib = d_a.clone(), d_b.clone()
            assert enc.pointwise(op, ia, d_b, out=ia) is ia and enc.pointwise(op, d_a, ib, out=ib) is ib
            assert np.array_equal(to_host(ia), want) and np.array_equal(to_host(ib), want), (n, op, "in place")
        assert np.array_equal(to_host(d_a), a) and np.array_equal(to_host(d_b), b)
    x = FC.mont(fid, QC.operands(fid, "random", 3 * 64, TILE, TILE // 8, "vecs")).reshape(3, 64, L)
    got = to_host(enc.batch_inverse(to_dev(x)))
    assert got.shape == x.shape and np.array_equal(got.reshape(-1, L), QC.host_inverse(fid, x.reshape(-1, L)))


@pytest.mark.parametrize("fid", QC.FIELDS)
def test_divide_device_equals_host(fid):
    """one point to four tiles, one vector and three with three different y, both orders, on a stream of its own -- and a dependent
    call behind it on the same stream"""
    F = FC.field(fid)
    enc, L = enc_of(fid), F.L
    st = torch.cuda.Stream(device=DEV)
    for log_m in (0, 5, 12, 14):
        m = 1 << log_m
        sh = QC.coset_shifts(fid, log_m, "dev")
        for n_vecs in (1, 3):
            v = np.stack([FC.mont(fid, FC.random_vector(fid, log_m, "qdev", i)) for i in range(n_vecs)])
            d_v = to_dev(v)
            y = FC.mont(fid, [FC.rng("qdevy", fid, log_m, i).randrange(F.p) for i in range(n_vecs)])
            d_y = to_dev(y)
            torch.cuda.synchronize()
            for order in QC.ORDERS:
                for s, sl in ((1, None), (sh["random"], DC.shift_limbs(fid, sh["random"]))):
                    zl = DC.shift_limbs(fid, QC.off_domain(fid, s, log_m, "dev"))
                    want = np.stack([QC.host_divide_linear(fid, sl, order, v[i], log_m, zl, y[i]) for i in range(n_vecs)])
                    buf = canaried(n_vecs * m, L)
                    out = buf[8:8 + n_vecs * m].view(n_vecs, m, L)
                    assert enc.divide_linear(d_v, sl, zl, d_y, order, out=out, stream=st.cuda_stream) is out
                    nxt = enc.batch_inverse(out, stream=st.cuda_stream)          # reads what the call before it wrote
                    st.synchronize()
                    assert np.array_equal(inner(buf).reshape(n_vecs, m, L), want), (log_m, n_vecs, order, s)
                    assert np.array_equal(to_host(nxt).reshape(-1, L), QC.host_inverse(fid, want.reshape(-1, L)))
                    inp = d_v.clone()
                    torch.cuda.synchronize()
                    assert enc.divide_linear(inp, sl, zl, d_y, order, out=inp) is inp and np.array_equal(to_host(inp), want)
                sl = DC.shift_limbs(fid, sh["gen"])
                for log_n in sorted({0, log_m // 2, log_m}):
                    want = np.stack([QC.host_divide_vanishing(fid, sl, order, v[i], log_m, log_n) for i in range(n_vecs)])
                    buf = canaried(n_vecs * m, L)
                    out = buf[8:8 + n_vecs * m].view(n_vecs, m, L)
                    enc.divide_vanishing(d_v, sl, log_n, order, out=out, stream=st.cuda_stream)
                    st.synchronize()
                    assert np.array_equal(inner(buf).reshape(n_vecs, m, L), want), (log_m, log_n, n_vecs, order)
                    inp = d_v.clone()
                    torch.cuda.synchronize()
                    assert np.array_equal(to_host(enc.divide_vanishing(inp, sl, log_n, order, out=inp)), want)
            assert np.array_equal(to_host(d_v), v) and np.array_equal(to_host(d_y), y)


# ---- the two chains ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("log_n,log_m", ((4, 6), (10, 12)))
@pytest.mark.parametrize("fid", (0, 3))
def test_vanishing_round_trip(fid, log_n, log_m):
    """f = q (X^n - 1) for a random q of degree < m - n: extend f to g H_m, divide by X^n - 1 there, interpolate: q, then n zeros"""
    F = FC.field(fid)
    enc, g = enc_of(fid), lcpc_amd.generator(fid)
    n, m = 1 << log_n, 1 << log_m
    rnd = FC.rng("vrt", fid, log_n, log_m)
    q = [rnd.randrange(F.p) for _ in range(m - n)]
    f = [0] * m
    for i, c in enumerate(q):
        f[i + n] = (f[i + n] + c) % F.p
        f[i] = (f[i] - c) % F.p
    for order, inv in (("natural", "ifft_ii"), ("bitrev", "ifft_oi")):
        vals = enc.extend(to_dev(FC.mont(fid, f)), g, log_m, order)
        quot = enc.divide_vanishing(vals, g, log_n, order, out=vals)
        coeffs = to_host(enc.coset_fft(quot, g, inv))
        assert np.array_equal(coeffs, FC.mont(fid, q + [0] * n)), order


def opening_round_trip(fid, enc):
    F = FC.field(fid)
    log_c = 12
    nc = 1 << log_c
    g = lcpc_amd.generator(fid)
    coeffs = FC.random_vector(fid, log_c, "open")
    d_c = to_dev(FC.mont(fid, coeffs))
    cm = LcCommit.commit_device(d_c.data_ptr(), nc, enc)
    z = QC.off_domain(fid, DC.GENERATORS[fid], log_c + 1, "open")
    zl = DC.shift_limbs(fid, z)
    y = cm.eval(to_dev(zl.reshape(1, -1)))                                 # p(z), left on the device
    q, r = QC.synthetic_division(fid, coeffs, z)
    assert FC.canon(fid, to_host(y)) == [r]
    vals = cm.values(g, log_c + 1)
    quot = enc.divide_linear(vals, g, zl, y)
    got = to_host(enc.coset_fft(quot, g, "ifft_ii"))
    assert len(q) == nc - 1
    assert np.array_equal(got[:nc - 1], FC.mont(fid, q)) and (got[nc - 1:] == 0).all() and got[nc - 1:].shape[0] == nc + 1
    qc = LcCommit.commit_coset_evals(quot, g, enc)
    d_q = to_dev(FC.mont(fid, q + [0] * (nc + 1)))
    want = LcCommit.commit_device(d_q.data_ptr(), 2 * nc, enc)
    assert qc.get_root() == want.get_root() and (qc.hashes() == want.hashes()).all()


@pytest.mark.parametrize("fid", (1, 3))
def test_opening_round_trip_ligero(fid):
    opening_round_trip(fid, enc_of(fid))


@pytest.mark.parametrize("fid", (1, 3))
def test_opening_round_trip_brakedown(fid):
    opening_round_trip(fid, sdig_enc(fid, 40))


# ---- refusals: nothing is written -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fid", QC.FIELDS)
def test_device_refusals_write_nothing(fid):
    F = FC.field(fid)
    enc, L, log_m = enc_of(fid), F.L, 6
    m = 1 << log_m
    eb = 8 * L
    lib = _lib.lib()
    g, one, zero = lcpc_amd.generator(fid), DC.shift_limbs(fid, 1), np.zeros(L, np.uint64)
    big = np.full(L, 0xFFFFFFFFFFFFFFFF, np.uint64)
    w = FC.root(fid, log_m)
    z_ok = DC.shift_limbs(fid, QC.off_domain(fid, DC.GENERATORS[fid], log_m))
    z_on = DC.shift_limbs(fid, DC.GENERATORS[fid] * pow(w, 5, F.p) % F.p)
    v = FC.mont(fid, FC.random_vector(fid, log_m, "qrefd"))
    d_v, d_y = to_dev(np.concatenate([v, v])), to_dev(FC.mont(fid, [3, 4]))
    buf = canaried(2 * m, L)
    o = dptr(buf, 8 * eb)
    vp = FC.vp
    inv = lambda i, out, n: lib.lcpcq_batch_inverse_device(enc._h, i, out, n, None)
    pw = lambda op, a, b, out, n: lib.lcpcq_pointwise_device(enc._h, op, a, b, out, n, None)
    lin = lambda s, order, i, lm, nv, z, y, out: lib.lcpcq_divide_linear_device(enc._h, vp(s), order, i, lm, nv, vp(z), y, out, None)
    van = lambda s, order, i, lm, ln, nv, out: lib.lcpcq_divide_vanishing_device(enc._h, vp(s), order, i, lm, ln, nv, out, None)
    calls = (
        lambda: lib.lcpcq_batch_inverse_device(None, dptr(d_v), o, m, None),
        lambda: inv(None, o, m), lambda: inv(dptr(d_v), None, m), lambda: inv(dptr(d_v), o, 0), lambda: inv(dptr(d_v), o, 1 << 39),
        lambda: inv(dptr(d_v, 4), o, m), lambda: inv(dptr(d_v), dptr(buf, 8 * eb + 4), m),
        lambda: inv(o, dptr(buf, 9 * eb), m), lambda: inv(dptr(buf, 9 * eb), o, m),                          # partial overlap
        lambda: pw(4, dptr(d_v), dptr(d_v), o, m), lambda: pw(0, None, dptr(d_v), o, m), lambda: pw(0, dptr(d_v), None, o, m),
        lambda: pw(3, dptr(d_v), dptr(d_v), None, m), lambda: pw(2, dptr(d_v), dptr(d_v), o, 0),
        lambda: pw(1, dptr(d_v, 4), dptr(d_v), o, m), lambda: pw(1, dptr(d_v), dptr(d_v, 4), o, m),
        lambda: pw(3, dptr(d_v), dptr(buf, 9 * eb), o, m), lambda: pw(3, dptr(buf, 9 * eb), dptr(d_v), o, m),
        lambda: lin(g, 0, dptr(d_v), log_m, 1, z_on, dptr(d_y), o),                                          # z = shift w^5
        lambda: lin(None, 0, dptr(d_v), log_m, 1, DC.shift_limbs(fid, pow(w, 5, F.p)), dptr(d_y), o),
        lambda: lin(zero, 0, dptr(d_v), log_m, 1, z_ok, dptr(d_y), o), lambda: lin(big, 0, dptr(d_v), log_m, 1, z_ok, dptr(d_y), o),
        lambda: lin(g, 0, dptr(d_v), log_m, 1, big, dptr(d_y), o), lambda: lin(g, 0, dptr(d_v), log_m, 1, None, dptr(d_y), o),
        lambda: lin(g, 0, dptr(d_v), log_m, 1, z_ok, None, o), lambda: lin(g, 2, dptr(d_v), log_m, 1, z_ok, dptr(d_y), o),
        lambda: lin(g, 0, dptr(d_v), log_m, 0, z_ok, dptr(d_y), o), lambda: lin(g, 0, dptr(d_v), log_m, 65536, z_ok, dptr(d_y), o),
        lambda: lin(g, 0, dptr(d_v), 33, 1, z_ok, dptr(d_y), o), lambda: lin(g, 0, dptr(d_v), 32, 128, z_ok, dptr(d_y), o),
        lambda: lin(g, 0, None, log_m, 1, z_ok, dptr(d_y), o), lambda: lin(g, 0, dptr(d_v), log_m, 1, z_ok, dptr(d_y), None),
        lambda: lin(g, 0, dptr(d_v, 4), log_m, 1, z_ok, dptr(d_y), o), lambda: lin(g, 0, dptr(d_v), log_m, 1, z_ok, dptr(d_y, 4), o),
        lambda: lin(g, 0, dptr(buf, 9 * eb), log_m, 1, z_ok, dptr(d_y), o),
        lambda: lin(g, 0, dptr(d_v), log_m, 1, z_ok, dptr(buf, 10 * eb), o),                                  # y inside the output
        lambda: van(one, 0, dptr(d_v), log_m, 2, 1, o), lambda: van(None, 0, dptr(d_v), log_m, 2, 1, o),
        lambda: van(DC.shift_limbs(fid, w), 0, dptr(d_v), log_m, 2, 1, o), lambda: van(zero, 0, dptr(d_v), log_m, 2, 1, o),
        lambda: van(big, 0, dptr(d_v), log_m, 2, 1, o), lambda: van(g, 0, dptr(d_v), log_m, log_m + 1, 1, o),
        lambda: van(g, 2, dptr(d_v), log_m, 2, 1, o), lambda: van(g, 0, dptr(d_v), log_m, 2, 0, o),
        lambda: van(g, 0, dptr(d_v), 33, 2, 1, o), lambda: van(g, 0, dptr(d_v), 32, 2, 128, o),
        lambda: van(g, 0, None, log_m, 2, 1, o), lambda: van(g, 0, dptr(d_v), log_m, 2, 1, None),
        lambda: van(g, 0, dptr(d_v, 4), log_m, 2, 1, o), lambda: van(g, 0, dptr(buf, 9 * eb), log_m, 2, 1, o),
    )
    for i, call in enumerate(calls):
        assert call() == ERR_ARG, i
    torch.cuda.synchronize()
    assert (to_host(buf) == CANARY).all()
    with pytest.raises(LcpcError) as err:
        enc.divide_vanishing(d_v[:m], one, 2, out=buf[8:8 + m])
    assert err.value.code == lcpc_amd.ERR_ARG
    with pytest.raises(ValueError):
        enc.pointwise("pow", d_v, d_v)
    with pytest.raises(ValueError):
        enc.divide_linear(d_v[:m], g, z_ok, d_y.cpu())
    torch.cuda.synchronize()
    assert (to_host(buf) == CANARY).all()
    assert lin(g, 1, dptr(d_v), log_m, 2, z_ok, dptr(d_y), o) == 0 and van(g, 1, o, log_m, 2, 2, o) == 0      # the same jobs, accepted
    torch.cuda.synchronize()
    assert (to_host(buf)[:8] == CANARY).all() and (to_host(buf)[-8:] == CANARY).all()

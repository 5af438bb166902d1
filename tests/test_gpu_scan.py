"""The scan extension (include/lcpc_hip_scan.h) on the device, through the C ABI and the Python wrappers: the device forms against the
host forms (themselves held to bignum by tests/test_scan_abi.py), calls chained through their totals, the ratio form against its
composition, and the two accumulators the extension exists for -- the grand product of a permutation argument and the running sum of
a log-derivative lookup, checked step by step on the device and committed to -- and the refusals.  All comparisons are for equality."""
import functools

import numpy as np
import pytest

import lcpc_amd
from lcpc_amd import LcCommit, LcpcError, LigeroEncoding, _lib

import fft_cases as FC
import k17_harness as K17
import scan_cases as SC

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

DEV = "cuda:0"
CANARY = SC.CANARY
ERR_ARG = SC.ERR_ARG


def to_dev(a):
    return torch.from_numpy(np.ascontiguousarray(a).view(np.int64)).to(DEV)


def to_host(t):
    return t.cpu().numpy().view(np.uint64)


@functools.lru_cache(maxsize=None)
def enc_of(fid):
    return LigeroEncoding.new_from_dims(fid, 64, 128)


def tile(fid):
    return K17.tile(2 * FC.field(fid).L)


def canaried(rows, L):
    buf = torch.full((rows + 16, L), CANARY, dtype=torch.int64, device=DEV)
    torch.cuda.synchronize()
    return buf


def inner(buf):
    got = to_host(buf)
    assert (got[:8] == CANARY).all() and (got[-8:] == CANARY).all(), "elements around the output were written"
    return got[8:-8]


def host_vectors(fid, op, mode, x, inits):
    """lcpcs_scan vector by vector: ((n_vecs, n, L) outputs, (n_vecs, L) totals)"""
    res = [SC.host_scan(fid, op, mode, x[v], None if inits is None else inits[v]) for v in range(x.shape[0])]
    return np.stack([r[0] for r in res]), np.stack([r[1] for r in res])


# ---- the device forms against the host forms ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fid", SC.FIELDS)
def test_scan_device_equals_host(fid):
    """a part of a tile, one tile, three and a ragged fourth; (n, L) and (3, n, L); with and without init and total; out of place
    between canaries and in place"""
    F = FC.field(fid)
    enc, L, T = enc_of(fid), F.L, tile(fid)
    for n in (100, T, 3 * T + 17):
        x = np.stack([FC.mont(fid, SC.operands(fid, "nonzero", n, T, 8, "dev", v)) for v in range(3)])
        inits = FC.mont(fid, [FC.rng("dev-init", fid, n, v).randrange(1, F.p) for v in range(3)])
        d_x, d_i = to_dev(x), to_dev(inits)
        for op in SC.OPS:
            for mode in SC.MODES:
                excl = mode == "exclusive"
                for vecs in (1, 3):
                    d_src = d_x[0] if vecs == 1 else d_x
                    for with_ends in (False, True):
                        want, wtot = host_vectors(fid, op, mode, x[:vecs], inits[:vecs] if with_ends else None)
                        buf, tot = canaried(vecs * n, L), canaried(vecs, L)
                        out = buf[8:8 + vecs * n].view(d_src.shape)
                        if with_ends:
                            res = enc.scan(d_src, op, excl, init=d_i[:vecs], out=out, total=tot[8:8 + vecs])
                            assert res[0] is out
                        else:
                            assert enc.scan(d_src, op, excl, out=out) is out
                        tag = (n, op, mode, vecs, with_ends)
                        assert np.array_equal(inner(buf).reshape(vecs, n, L), want), tag
                        assert np.array_equal(inner(tot), wtot) if with_ends else (to_host(tot) == CANARY).all(), tag
                        inp = d_src.clone()
                        assert enc.scan(inp, op, excl, init=d_i[:vecs] if with_ends else None, out=inp) is inp
                        assert np.array_equal(to_host(inp).reshape(vecs, n, L), want), (tag, "in place")
        assert np.array_equal(to_host(d_x), x) and np.array_equal(to_host(d_i), inits)
    fresh, total = enc.scan(d_x, "sum", total=torch.empty((3, L), dtype=torch.int64, device=DEV))    # a new output tensor
    want, wtot = host_vectors(fid, "sum", "inclusive", x, None)
    assert np.array_equal(to_host(fresh), want) and np.array_equal(to_host(total), wtot)


def test_more_tiles_than_one_level_of_totals():
    """n = (M + 1) T + 5: the tile totals no longer fit one tile, so their scan takes the three phases itself (five launches).  Ft63
    only, whose elements are the smallest (134 MB); the host form is the reference"""
    fid = 0
    F = FC.field(fid)
    enc, T, M = enc_of(fid), tile(fid), K17.mid_chunk(2)
    n = (M + 1) * T + 5
    assert n * 8 < 1 << 30
    x = np.random.default_rng(17).integers(1, F.p, size=(n, 1), dtype=np.uint64)      # (any value below p is a Montgomery form)
    init = FC.mont(fid, [12345])
    d_x, d_i = to_dev(x), to_dev(init)
    for op, mode in (("product", "exclusive"), ("sum", "inclusive")):
        want, wtot = SC.host_scan(fid, op, mode, x, init[0])
        tot = torch.empty((1, 1), dtype=torch.int64, device=DEV)
        got = enc.scan(d_x, op, mode == "exclusive", init=d_i, total=tot)[0]
        assert np.array_equal(to_host(tot)[0], wtot), (op, mode)
        assert np.array_equal(to_host(got), want), (op, mode)
        del got


@pytest.mark.parametrize("fid", SC.FIELDS)
def test_chained_calls_and_streams(fid):
    """two calls through total_dev -> init_dev on one stream equal one call over the whole; a scan on a stream of its own with a
    dependent pointwise behind it"""
    F = FC.field(fid)
    enc, L, T = enc_of(fid), F.L, tile(fid)
    n, cut = 2 * T + 100, T + 37
    x = FC.mont(fid, SC.operands(fid, "nonzero", n, T, 8, "chain"))
    d_x = to_dev(x)
    st = torch.cuda.Stream(device=DEV)
    torch.cuda.synchronize()
    for op in SC.OPS:
        for mode in SC.MODES:
            excl = mode == "exclusive"
            want, wtot = SC.host_scan(fid, op, mode, x)
            out = torch.empty_like(d_x)
            mid, end = (torch.empty((1, L), dtype=torch.int64, device=DEV) for _ in range(2))
            torch.cuda.synchronize()
            enc.scan(d_x[:cut], op, excl, out=out[:cut], total=mid, stream=st.cuda_stream)
            enc.scan(d_x[cut:], op, excl, init=mid, out=out[cut:], total=end, stream=st.cuda_stream)
            nxt = enc.pointwise("mul", out, out, stream=st.cuda_stream)          # reads what the calls before it wrote
            st.synchronize()
            assert np.array_equal(to_host(out), want) and np.array_equal(to_host(end)[0], wtot), (op, mode)
            assert np.array_equal(to_host(nxt), lcpc_amd.pointwise(fid, "mul", want, want)), (op, mode, "dependent call")


@pytest.mark.parametrize("fid", SC.FIELDS)
def test_scan_ratio_device(fid):
    """against pointwise(DIV) followed by the scan, against the host form and against bignum, zeros among the denominators; out == num
    and out == den"""
    F = FC.field(fid)
    enc, L, T = enc_of(fid), F.L, tile(fid)
    n = T + 300
    num = SC.operands(fid, "nonzero", n, T, 8, "rnum")
    den = SC.operands(fid, "nonzero", n, T, 8, "rden")
    c = FC.rng("rinit", fid).randrange(1, F.p)
    for name, dd in (("alive", den), ("zeros", [0 if k in (0, 77, T - 1, T, n - 1) else v for k, v in enumerate(den)])):
        nm, dm, cm = FC.mont(fid, num), FC.mont(fid, dd), FC.mont(fid, [c])
        d_n, d_d, d_c = to_dev(nm), to_dev(dm), to_dev(cm)
        terms = SC.ratio_terms(fid, num, dd)
        for op in SC.OPS:
            for mode in SC.MODES:
                excl = mode == "exclusive"
                ref, rtot = SC.scan_ref(fid, op, mode, terms, c)
                want, wtot = FC.mont(fid, ref), FC.mont(fid, [rtot])
                host, htot = SC.host_scan_ratio(fid, op, mode, nm, dm, cm[0])
                assert np.array_equal(host, want) and np.array_equal(htot, wtot[0])
                buf, tot = canaried(n, L), canaried(1, L)
                enc.scan_ratio(d_n, d_d, op, excl, init=d_c, out=buf[8:8 + n], total=tot[8:9])
                assert np.array_equal(inner(buf), want) and np.array_equal(inner(tot), wtot), (name, op, mode)
                comp = enc.scan(enc.pointwise("div", d_n, d_d), op, excl, init=d_c)
                assert np.array_equal(to_host(comp), want), (name, op, mode, "composition")
                on, od = d_n.clone(), d_d.clone()
                assert enc.scan_ratio(on, d_d, op, excl, init=d_c, out=on) is on and enc.scan_ratio(d_n, od, op, excl, init=d_c, out=od) is od
                assert np.array_equal(to_host(on), want) and np.array_equal(to_host(od), want), (name, op, mode, "in place")
        assert np.array_equal(to_host(d_n), nm) and np.array_equal(to_host(d_d), dm)


# ---- the accumulators ----------------------------------------------------------------------------------------------------------------
def interpolation_value(fid, vals, x):
    """p(x) for the p of degree < n with p(w^i) = vals[i]: (x^n - 1) / n * sum_i vals[i] w^i / (x - w^i)"""
    F = FC.field(fid)
    n = len(vals)
    w = FC.root(fid, n.bit_length() - 1)
    acc, wi = 0, 1
    for v in vals:
        acc = (acc + v * wi % F.p * pow((x - wi) % F.p, F.p - 2, F.p)) % F.p
        wi = wi * w % F.p
    return (pow(x, n, F.p) - 1) * pow(n, F.p - 2, F.p) % F.p * acc % F.p


def committed_value_matches(fid, enc, z_dev, z_vals):
    """the composition the extension exists for: the column goes through LcCommit.commit_evals, and the committed polynomial takes the
    value of the bignum interpolation at a random point"""
    F = FC.field(fid)
    x = FC.rng("acc-x", fid).randrange(2, F.p)
    cm = LcCommit.commit_evals(z_dev, enc)
    assert FC.canon(fid, cm.eval(FC.mont(fid, [x]))) == [interpolation_value(fid, z_vals, x)]


@pytest.mark.parametrize("fid", (3, 1))
def test_permutation_accumulator(fid):
    """a column a that is constant on the cycles of a random permutation sigma: prod (a[k] + beta k + gamma) / (a[k] + beta sigma(k)
    + gamma) = 1.  z = scan_ratio(product, exclusive): total == 1, z[k + 1] den[k] == z[k] num[k] at every k (on the device), and z is
    committed to.  One changed value of a in the denominators: total != 1"""
    F = FC.field(fid)
    enc, L, n = enc_of(fid), F.L, 1 << 12
    rnd = FC.rng("perm", fid)
    sigma = list(range(n))
    rnd.shuffle(sigma)
    a, seen = [0] * n, [False] * n
    for k in range(n):                                   # one value per cycle of sigma
        if not seen[k]:
            v, j = rnd.randrange(F.p), k
            while not seen[j]:
                seen[j], a[j] = True, v
                j = sigma[j]
    beta, gamma = rnd.randrange(1, F.p), rnd.randrange(F.p)
    num = [(a[k] + beta * k + gamma) % F.p for k in range(n)]
    den = [(a[k] + beta * sigma[k] + gamma) % F.p for k in range(n)]
    assert all(den)
    d_num, d_den = to_dev(FC.mont(fid, num)), to_dev(FC.mont(fid, den))
    total = torch.empty((1, L), dtype=torch.int64, device=DEV)
    z, _ = enc.scan_ratio(d_num, d_den, "product", exclusive=True, total=total)
    assert FC.canon(fid, to_host(total)) == [1]
    lhs = enc.pointwise("mul", z[1:], d_den[:-1])
    rhs = enc.pointwise("mul", z[:-1], d_num[:-1])
    assert torch.equal(lhs, rhs)
    zc = FC.canon(fid, to_host(z))
    assert zc[0] == 1 and zc[n - 1] * num[n - 1] % F.p == den[n - 1]             # the last step closes the cycle: z[n] = total = 1
    assert zc == SC.scan_ref(fid, "product", "exclusive", SC.ratio_terms(fid, num, den))[0]
    committed_value_matches(fid, enc, z, zc)
    bad = list(den)
    j = n // 3
    bad[j] = (a[j] + 1 + beta * sigma[j] + gamma) % F.p                            # a'[j] = a[j] + 1
    enc.scan_ratio(d_num, to_dev(FC.mont(fid, bad)), "product", exclusive=True, total=total)
    assert FC.canon(fid, to_host(total)) != [1]


@pytest.mark.parametrize("fid", (3, 1))
def test_log_derivative_sum(fid):
    """a lookup of 2^11 witness values in a table of 2^11 entries: sum_i 1 / (beta - f[i]) - sum_k m[k] / (beta - t[k]) = 0 with m the
    multiplicities.  s = scan_ratio(sum, exclusive) over the 2^12 terms: total == 0, (s[k + 1] - s[k]) den[k] == num[k] at every k
    (on the device), and s is committed to.  A witness value outside the table: total != 0"""
    F = FC.field(fid)
    enc, L, h = enc_of(fid), F.L, 1 << 11
    rnd = FC.rng("logup", fid)
    table = rnd.sample(range(1, 1 << 40), h)
    f = [table[rnd.randrange(h // 4)] for _ in range(h)]                          # (repeated entries: multiplicities above one)
    mult = {t: 0 for t in table}
    for v in f:
        mult[v] += 1
    beta = rnd.randrange(1 << 41, F.p)
    num = [1] * h + [(-mult[t]) % F.p for t in table]
    den = [(beta - v) % F.p for v in f] + [(beta - t) % F.p for t in table]
    d_num, d_den = to_dev(FC.mont(fid, num)), to_dev(FC.mont(fid, den))
    total = torch.empty((1, L), dtype=torch.int64, device=DEV)
    s, _ = enc.scan_ratio(d_num, d_den, "sum", exclusive=True, total=total)
    assert FC.canon(fid, to_host(total)) == [0]
    step = enc.pointwise("mul", enc.pointwise("sub", s[1:], s[:-1]), d_den[:-1])
    assert torch.equal(step, d_num[:-1])
    sc = FC.canon(fid, to_host(s))
    assert sc[0] == 0 and (0 - sc[-1]) * den[-1] % F.p == num[-1]                   # the last step returns to zero
    committed_value_matches(fid, enc, s, sc)
    bad = list(den)
    bad[5] = (beta - (1 << 40) - 7) % F.p                                          # a witness value no table entry equals
    enc.scan_ratio(d_num, to_dev(FC.mont(fid, bad)), "sum", exclusive=True, total=total)
    assert FC.canon(fid, to_host(total)) != [0]


# ---- refusals: nothing is written -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fid", SC.FIELDS)
def test_device_refusals_write_nothing(fid):
    F = FC.field(fid)
    enc, L = enc_of(fid), F.L
    lib = _lib.lib()
    size = SC.refusal_buffer_bytes(lib, enc._h, L)
    bufs = [torch.full((size // 8,), CANARY, dtype=torch.int64, device=DEV) for _ in range(6)]
    torch.cuda.synchronize()
    SC.device_refusals(lib, enc._h, L, [b.data_ptr() for b in bufs])
    x = bufs[0][:64 * L].view(64, L)
    with pytest.raises(ValueError):
        enc.scan(x, "max")
    with pytest.raises(ValueError):
        enc.scan(x, "sum", init=bufs[1][:2 * L].view(2, L))                        # one element per vector
    with pytest.raises(ValueError):
        enc.scan(x, "sum", total=bufs[1][:L].view(1, L).cpu())
    with pytest.raises(ValueError):
        enc.scan_ratio(x, bufs[1][:32 * L].view(32, L), "product")
    with pytest.raises(LcpcError) as err:
        enc.scan(x, "sum", init=x[3:4], out=bufs[2][:64 * L].view(64, L))          # init inside the input
    assert err.value.code == lcpc_amd.ERR_ARG
    torch.cuda.synchronize()
    for b in bufs:
        assert bool((b == CANARY).all())

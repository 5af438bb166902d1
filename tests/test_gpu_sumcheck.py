"""The sumcheck extension (include/lcpc_hip_sumcheck.h) on the device, through the C ABI and the Python wrappers: the device forms
against the host forms (themselves held to bignum by tests/test_sumcheck_abi.py), every refusal, and what the extension exists for --
a whole sumcheck over a committed multilinear polynomial that ends in an opening of the commitment at the bound point.  All
comparisons are for equality."""
import functools

import numpy as np
import pytest

import lcpc_amd
from lcpc_amd import LcCommit, LcpcError, LigeroEncoding, SdigEncoding, Transcript, _lib

import fft_cases as FC
import oracle_lib as O
import sumcheck_cases as MC
from common import mk_transcript

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

DEV = "cuda:0"
CANARY = MC.CANARY
ERR_ARG = MC.ERR_ARG


def to_dev(a):
    return torch.from_numpy(np.ascontiguousarray(a).view(np.int64)).to(DEV)


def to_host(t):
    return t.cpu().numpy().view(np.uint64)


@functools.lru_cache(maxsize=None)
def enc_of(fid):
    return LigeroEncoding.new_from_dims(fid, 64, 128)


def canaried(rows, L):
    buf = torch.full((rows + 16, L), CANARY, dtype=torch.int64, device=DEV)
    torch.cuda.synchronize()
    return buf


def inner(buf):
    got = to_host(buf)
    assert (got[:8] == CANARY).all() and (got[-8:] == CANARY).all(), "elements around the output were written"
    return got[8:-8]


# ---- the device forms against the host forms ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("order", MC.ORDERS)
@pytest.mark.parametrize("fid", MC.FIELDS)
def test_device_equals_host(fid, order):
    """bind, round and the fused call at n = 2^10 (two workgroups) and 2^13 (sixteen): new outputs, outputs between canaries, and in
    place under the high order; on torch's stream and on a stream of the caller's"""
    F = FC.field(fid)
    enc, L = enc_of(fid), F.L
    side = torch.cuda.Stream()
    for n in (1 << 10, 1 << 13):
        rng = np.random.default_rng(n + fid)
        tabs = rng.integers(0, 1 << 64, size=(8, n, L), dtype=np.uint64)
        tabs[:, :, L - 1] = rng.integers(0, F.p >> (64 * (L - 1)), size=(8, n), dtype=np.uint64)      # (any value below p is a Montgomery form)
        d_tabs = [to_dev(t) for t in tabs]
        r = MC.elem(fid, FC.rng("gpu-sumcheck-r", fid, order, n).randrange(F.p))
        want_bound = [MC.host_bind(fid, order, t, r).copy() for t in tabs]
        got = enc.sumcheck_bind(d_tabs, r, order)
        assert len(got) == 8 and all(np.array_equal(to_host(g), w) for g, w in zip(got, want_bound))
        bufs = [canaried(n // 2, L) for _ in range(2)]
        outs = [b[8:8 + n // 2] for b in bufs]
        res = enc.sumcheck_bind(d_tabs[:2], r, order, out=outs)
        assert res[0] is outs[0] and all(np.array_equal(inner(b), w) for b, w in zip(bufs, want_bound))
        for tname in ("ab", "eq_ab_minus_c", "full"):
            n_tables, terms = MC.terms_of(fid, tname)
            wterms = MC.wrapper_terms(fid, terms)
            d = MC.degree(terms)
            want = MC.host_round(fid, order, list(tabs[:n_tables]), terms)
            assert np.array_equal(to_host(enc.sumcheck_round(d_tabs[:n_tables], wterms, order)), want), (n, tname)
            ev = canaried(d + 1, L)
            with torch.cuda.stream(side):
                side.wait_stream(torch.cuda.current_stream())
                assert enc.sumcheck_round(d_tabs[:n_tables], wterms, order, evals=ev[8:8 + d + 1], stream=side.cuda_stream) is not None
            side.synchronize()
            assert np.array_equal(inner(ev), want), (n, tname, "stream")
            # the fused call: the bind's stores and the round of the bound tables
            want2 = MC.host_round(fid, order, want_bound[:n_tables], terms)
            bound, evals = enc.sumcheck_bind_round(d_tabs[:n_tables], wterms, r, order)
            assert all(np.array_equal(to_host(b), w) for b, w in zip(bound, want_bound)) and np.array_equal(to_host(evals), want2), (n, tname)
            two = enc.sumcheck_round(enc.sumcheck_bind(d_tabs[:n_tables], r, order), wterms, order)
            assert np.array_equal(to_host(two), to_host(evals)), (n, tname, "the two calls")
            if order == "high":
                io = [t.clone() for t in d_tabs[:n_tables]]
                bound, evals = enc.sumcheck_bind_round(io, wterms, r, order, out=io)
                assert all(b.data_ptr() == t.data_ptr() and b.shape[0] == n // 2 for b, t in zip(bound, io))
                assert all(np.array_equal(to_host(b), w) for b, w in zip(bound, want_bound)) and np.array_equal(to_host(evals), want2)
                assert all(np.array_equal(to_host(t)[n // 2:], s[n // 2:]) for t, s in zip(io, tabs)), "in place, the upper half was written"
        if order == "high":
            io = [t.clone() for t in d_tabs]
            bound = enc.sumcheck_bind(io, r, order, out=io)
            assert all(np.array_equal(to_host(b), w) for b, w in zip(bound, want_bound))
        else:
            with pytest.raises(LcpcError):
                enc.sumcheck_bind(d_tabs[:1], r, order, out=d_tabs[:1])
        assert all(np.array_equal(to_host(t), s) for t, s in zip(d_tabs, tabs)), "an input was written"


# ---- refusals: nothing is written -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fid", MC.FIELDS)
def test_device_refusals_write_nothing(fid):
    F = FC.field(fid)
    enc, L = enc_of(fid), F.L
    lib = _lib.lib()
    size = MC.refusal_buffer_bytes(lib, enc._h, L)
    bufs = [torch.full((size // 8,), CANARY, dtype=torch.int64, device=DEV) for _ in range(6)]
    torch.cuda.synchronize()
    MC.device_refusals(lib, enc._h, fid, [b.data_ptr() for b in bufs])
    x = bufs[0][:64 * L].view(64, L)
    with pytest.raises(ValueError):
        enc.sumcheck_bind([x], MC.elem(fid, 3), "middle")
    with pytest.raises(ValueError):
        enc.sumcheck_round([x, x[:32]], [(None, [0, 1])])
    with pytest.raises(ValueError):
        enc.sumcheck_round([x], [(None, [0]), (MC.elem(fid, 3), [0])])
    with pytest.raises(ValueError):
        enc.sumcheck_bind_round([x], [(None, [0])], MC.elem(fid, 3), "high", out=[x, x])
    with pytest.raises(LcpcError):
        enc.sumcheck_round([x], [(None, [1])])                           # a table index beyond the tables
    torch.cuda.synchronize()
    assert all((to_host(b) == CANARY).all() for b in bufs)


# ---- a whole sumcheck, and the opening it ends in ---------------------------------------------------------------------------------------
def challenge(tr, fid, evals):
    """the round's evaluations go into the transcript, r comes out of it"""
    tr.append_message(b"sumcheck round", to_host(evals).tobytes())
    return int.from_bytes(tr.challenge_bytes(b"sumcheck r", 64), "little") % FC.field(fid).p


@pytest.mark.parametrize("order", MC.ORDERS)
@pytest.mark.parametrize("kind", ("ligero", "brakedown"))
@pytest.mark.parametrize("fid", (0, 3))
def test_whole_sumcheck_ends_in_an_opening(fid, kind, order):
    """sum_x f(x) g(x) = claim over v = 12 variables, f the committed tensor: round 0 by enc.sumcheck_round, every further round by
    enc.sumcheck_bind_round with the challenge before it, the last challenge by enc.sumcheck_bind.  The verifier's checks hold round by
    round, the last bound value of f is LcCommit.eval at the bound point, and verify accepts the opening there"""
    F = FC.field(fid)
    v, L = 12, F.L
    n = 1 << v
    enc = LigeroEncoding.new_ml(fid, v) if kind == "ligero" else SdigEncoding.new_ml(fid, v, 5)
    f_l, g_l = O.random_elems(fid, n, 70 + fid), O.random_elems(fid, n, 80 + fid)
    d_f, d_g = to_dev(f_l), to_dev(g_l)
    cm = LcCommit.commit_device(d_f.data_ptr(), n, enc)
    terms = [(None, [0, 1])]
    claim = sum(a * b for a, b in zip(FC.canon(fid, f_l), FC.canon(fid, g_l))) % F.p
    tr = Transcript(b"sumcheck test")
    tr.append_message(b"polycommit", bytes(cm.get_root()))
    tabs = [d_f.clone(), d_g.clone()] if order == "high" else [d_f, d_g]
    evals = enc.sumcheck_round(tabs, terms, order)
    rs = []
    for k in range(v):
        g = FC.canon(fid, to_host(evals))
        assert (g[0] + g[1]) % F.p == claim, k                           # the verifier's check of round k
        r = challenge(tr, fid, evals)
        rs.append(r)
        claim = MC.interpolate(fid, g, r)
        if k + 1 < v:
            assert tabs[0].shape[0] == n >> k
            tabs, evals = enc.sumcheck_bind_round(tabs, terms, MC.elem(fid, r), order, out=tabs if order == "high" else None)
        else:
            tabs = enc.sumcheck_bind(tabs, MC.elem(fid, r), order, out=tabs if order == "high" else None)
    assert tabs[0].shape[0] == 1
    f_end, g_end = to_host(tabs[0])[:1], to_host(tabs[1])[:1]
    assert FC.canon(fid, f_end)[0] * FC.canon(fid, g_end)[0] % F.p == claim      # the last check: the composition at the bound point
    assert np.array_equal(to_host(d_f), f_l) and np.array_equal(to_host(d_g), g_l)
    # the bound point in the variable order of include/lcpc_hip_eval.h, and the opening of the commitment there
    z = rs if order == "low" else rs[::-1]
    pt = FC.mont(fid, z)
    assert np.array_equal(cm.eval(pt.reshape(1, v, L), basis="ml_lagrange"), f_end)
    assert np.array_equal(to_host(cm.eval(to_dev(pt).view(1, v, L), basis="ml_lagrange")), f_end)
    outer, inner_t = enc.tensors(pt, cm.n_rows, basis="ml_lagrange")
    root = cm.get_root()
    pf = cm.prove(outer, enc, mk_transcript(Transcript, root, enc.get_n_col_opens()))
    ev = pf.verify(root, outer, inner_t, enc, mk_transcript(Transcript, root, enc.get_n_col_opens()))
    assert np.array_equal(ev.reshape(1, L), f_end)
    # and g, which the verifier holds itself: the host form ends in the same value
    t = g_l
    for r in rs:
        t = lcpc_amd.sumcheck_bind(fid, t, MC.elem(fid, r), order)
    assert np.array_equal(t, g_end)

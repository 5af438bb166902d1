"""The evaluation extension (include/lcpc_hip_eval.h) on the device: the tensor kernels K10 against the host call, the dot product K11
against bignum, and the value of committed polynomials -- univariate and multilinear, Ligero and Brakedown -- against bignum and
against what verify returns for a proof made with the same point's tensors.  Every comparison is equality of limbs."""
import ctypes as C
import threading

import numpy as np
import pytest

import lcpc_amd
from lcpc_amd import LcCommit, LcpcError, LigeroEncoding, SdigEncoding, Transcript, _lib

import eval_cases as EC
import ints_cases as IC
import oracle_lib as O
from common import mk_transcript

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

DEV = "cuda:0"
CANARY = EC.CANARY
vp = EC.vp
ERR_ARG, ERR_STATE = lcpc_amd.ERR_ARG, lcpc_amd.ERR_STATE


def to_dev(a):
    return torch.from_numpy(np.ascontiguousarray(a, np.uint64).view(np.int64)).to(DEV)


def dptr(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def canaried(n_elems, L):
    """n_elems elements of canary words with 64 more words behind them"""
    return torch.full((n_elems * L + 64,), int(CANARY), dtype=torch.int64, device=DEV)


def read(t, n_elems, L):
    out = t.cpu().numpy().view(np.uint64)
    assert (out[n_elems * L:] == CANARY).all(), "canaries behind the output"
    return out[:n_elems * L].reshape(n_elems, L)


@pytest.fixture(scope="module")
def small_encs():
    return {fid: LigeroEncoding.new_from_dims(fid, 64, 128) for fid in EC.FIELDS}


# ---- K10 ------------------------------------------------------------------------------------------------------------------------
TENSOR_SHAPES = {"powers": ((1, 1), (257, 1), (130, 96), (5000, 1 << 20)),
                 "ml_monomial": ((1, 1), (8, 1), (64, 32), (1, 512)), "ml_lagrange": ((1, 1), (8, 1), (64, 32), (1, 512))}


@pytest.mark.parametrize("fid", EC.FIELDS)
@pytest.mark.parametrize("basis", EC.BASES)
def test_tensors_device_equals_host(small_encs, fid, basis):
    enc, L = small_encs[fid], O.limbs(fid)
    p = IC.modulus(fid)
    for n_rows, n_per_row in TENSOR_SHAPES[basis]:
        n_pt = EC.n_point(basis, n_rows, n_per_row)
        rnd = EC.rng("k10", fid, basis, n_rows, n_per_row)
        pts = [EC.random_point(basis, fid, n_rows, n_per_row, rnd) for _ in range(3)]
        if basis == "powers":
            pts[1] = [p - 1]
        want = [EC.host_tensors(fid, basis, EC.mont(fid, pt) if pt else None, n_pt, n_rows, n_per_row) for pt in pts]
        for n_points in (1, 3):
            flat = [z for pt in pts[:n_points] for z in pt]
            d_pts = to_dev(EC.mont(fid, flat)) if flat else None
            d_outer, d_inner = canaried(n_points * n_rows, L), canaried(n_points * n_per_row, L)
            rc = _lib.lib().lcpce_tensors_device(enc._h, _lib.EVAL_BASES[basis], dptr(d_pts), n_pt, n_points, n_rows, n_per_row, dptr(d_outer),
                                                 dptr(d_inner), None)
            assert rc == 0
            torch.cuda.synchronize()
            outer = read(d_outer, n_points * n_rows, L).reshape(n_points, n_rows, L)
            inner = read(d_inner, n_points * n_per_row, L).reshape(n_points, n_per_row, L)
            for t in range(n_points):
                assert np.array_equal(outer[t], want[t][0]) and np.array_equal(inner[t], want[t][1]), (n_rows, n_per_row, n_points, t)
        # one tensor alone: the other is neither needed nor written
        d_pts = to_dev(EC.mont(fid, pts[0])) if pts[0] else None
        d_inner = canaried(n_per_row, L)
        assert _lib.lib().lcpce_tensors_device(enc._h, _lib.EVAL_BASES[basis], dptr(d_pts), n_pt, 1, n_rows, n_per_row, None, dptr(d_inner), None) == 0
        torch.cuda.synchronize()
        assert np.array_equal(read(d_inner, n_per_row, L), want[0][1])


# ---- K11 ------------------------------------------------------------------------------------------------------------------------
# (from 4096 elements on K11 cuts a pair into chunks and adds their sums in a second launch: the sizes around that, and a ragged last chunk)
DOT_N = (1, 63, 64, 65, 255, 256, 257, 1000, 8192, 4095, 4096, 4099, 6151)


@pytest.mark.parametrize("fid", EC.FIELDS)
@pytest.mark.parametrize("operands", ("max", "random"))
def test_dot_device_against_bignum(small_encs, fid, operands):
    enc, L = small_encs[fid], O.limbs(fid)
    p = IC.modulus(fid)
    n_max = 3 * max(DOT_N)
    if operands == "max":
        a = b = [p - 1] * n_max
        a_l = b_l = np.tile(EC.mont(fid, [p - 1]), (n_max, 1))
    else:
        rnd = EC.rng("k11", fid)
        a, b = [rnd.randrange(p) for _ in range(n_max)], [rnd.randrange(p) for _ in range(n_max)]
        a_l, b_l = EC.mont(fid, a), EC.mont(fid, b)
    d_a, d_b = to_dev(a_l), to_dev(b_l)
    for n in DOT_N:
        for n_pairs in (1, 3):
            for b_stride in (0, n):
                want = [sum(a[t * n + i] * b[t * b_stride + i] for i in range(n)) % p for t in range(n_pairs)]
                d_out = canaried(n_pairs, L)
                assert _lib.lib().lcpce_dot_device(enc._h, dptr(d_a), n, dptr(d_b), b_stride, n, n_pairs, dptr(d_out), None) == 0
                torch.cuda.synchronize()
                assert np.array_equal(read(d_out, n_pairs, L), EC.mont(fid, want)), (n, n_pairs, b_stride)


# ---- evaluation -------------------------------------------------------------------------------------------------------------------
def horner(coeffs, x, p):
    acc = 0
    for c in reversed(coeffs):
        acc = (acc * x + c) % p
    return acc


def three_entry_points(cm, basis, n_pt, pts_l):
    """lcpce_eval, lcpce_eval_device and lcpce_eval_tensors_device (tensors by lcpce_tensors_device) for pts_l (n_points, n_pt, L)"""
    enc, L = cm.enc, cm.enc.L
    n_points = pts_l.shape[0]
    b = _lib.EVAL_BASES[basis]
    lib = _lib.lib()
    host = np.full((n_points + 1, L), CANARY, np.uint64)
    assert lib.lcpce_eval(cm._h, b, vp(pts_l), n_pt, n_points, vp(host)) == 0
    assert (host[n_points] == CANARY).all()
    d_pts = to_dev(pts_l)
    d_ev = canaried(n_points, L)
    assert lib.lcpce_eval_device(cm._h, b, dptr(d_pts), n_pt, n_points, None, dptr(d_ev)) == 0
    d_outer, d_inner = canaried(n_points * cm.n_rows, L), canaried(n_points * cm.n_per_row, L)
    assert lib.lcpce_tensors_device(enc._h, b, dptr(d_pts), n_pt, n_points, cm.n_rows, cm.n_per_row, dptr(d_outer), dptr(d_inner), None) == 0
    d_ev2 = canaried(n_points, L)
    assert lib.lcpce_eval_tensors_device(cm._h, dptr(d_outer), dptr(d_inner), n_points, None, dptr(d_ev2)) == 0
    torch.cuda.synchronize()
    return host[:n_points], read(d_ev, n_points, L), read(d_ev2, n_points, L)


def round_trip(cm, basis, pt_l, claimed):
    """prove with the point's outer tensor, verify with both: verify's evaluation is the claimed limbs"""
    enc = cm.enc
    outer, inner = enc.tensors(pt_l, cm.n_rows, basis=basis)
    root = cm.get_root()
    pf = cm.prove(outer, enc, mk_transcript(Transcript, root, enc.get_n_col_opens()))
    ev = pf.verify(root, outer, inner, enc, mk_transcript(Transcript, root, enc.get_n_col_opens()))
    assert np.array_equal(ev.reshape(-1), np.asarray(claimed).reshape(-1))


def make_enc(kind, fid, n):
    """"ligero-rows": 64 coefficients per row, so that the same sizes make 16, 64 and 16 rows (the encoders' own choice is 1 to 8)"""
    if kind == "ligero-rows":
        return LigeroEncoding.new_from_dims(fid, 64, 128)
    return LigeroEncoding.new(fid, n) if kind == "ligero" else SdigEncoding.new(fid, n, 7)


@pytest.mark.parametrize("fid", EC.FIELDS)
@pytest.mark.parametrize("kind", ("ligero", "brakedown", "ligero-rows"))
def test_univariate_evaluation(fid, kind):
    p, L = IC.modulus(fid), O.limbs(fid)
    for n in (1 << 10, 1 << 12, 1000) + ((64 * 37 + 5,) if kind == "ligero-rows" else ()):
        enc = make_enc(kind, fid, n)
        coeffs_l = O.random_elems(fid, n, 40 + fid)
        cm = LcCommit.commit(coeffs_l, enc)
        assert cm.n_rows * cm.n_per_row >= n
        if n == 1000 and kind != "brakedown":
            assert cm.n_rows * cm.n_per_row > n        # a ragged last row: its tail counts as zeros
        if n == 64 * 37 + 5:
            assert cm.n_rows == 38                     # a row count that is no power of two
        coeffs = EC.canon(fid, coeffs_l)
        rnd = EC.rng("uni", fid, kind, n)
        xs = [rnd.randrange(p) for _ in range(3)] + [p - 1, 0]
        want = EC.mont(fid, [horner(coeffs, x, p) for x in xs])
        pts_l = EC.mont(fid, xs).reshape(5, 1, L)
        for n_points in (1, 2, 3, 5):
            for got in three_entry_points(cm, "powers", 1, pts_l[:n_points]):
                assert np.array_equal(got, want[:n_points]), (n, n_points)
        round_trip(cm, "powers", pts_l[0], want[0])


@pytest.mark.parametrize("fid", EC.FIELDS)
@pytest.mark.parametrize("kind", ("ligero", "brakedown"))
def test_multilinear_evaluation(fid, kind):
    p, L = IC.modulus(fid), O.limbs(fid)
    for n_vars in (10, 12):
        enc = LigeroEncoding.new_ml(fid, n_vars) if kind == "ligero" else SdigEncoding.new_ml(fid, n_vars, 5)
        n = 1 << n_vars
        coeffs_l = O.random_elems(fid, n, 50 + fid)
        cm = LcCommit.commit(coeffs_l, enc)
        assert cm.n_rows * cm.n_per_row == n
        coeffs = EC.canon(fid, coeffs_l)
        for basis in EC.ML_BASES:
            rnd = EC.rng("ml", fid, kind, n_vars, basis)
            pts = [EC.random_point(basis, fid, cm.n_rows, cm.n_per_row, rnd) for _ in range(2)] + [[rnd.randrange(p) for _ in range(n_vars)]]
            want = EC.mont(fid, [EC.eval_ref(basis, fid, coeffs, pt, cm.n_rows, cm.n_per_row) for pt in pts])
            pts_l = EC.mont(fid, [z for pt in pts for z in pt]).reshape(3, n_vars, L)
            for n_points in (1, 3):
                for got in three_entry_points(cm, basis, n_vars, pts_l[:n_points]):
                    assert np.array_equal(got, want[:n_points]), (n_vars, basis, n_points)
            round_trip(cm, basis, pts_l[2], want[2])
        # the Lagrange basis at the Boolean point of index e: coefficient e itself
        idx = [e for e in (0, 1, cm.n_per_row, n - 1) if e < n]       # (a one-row commitment has no coefficient n_per_row)
        pts_l = EC.mont(fid, [(e >> k) & 1 for e in idx for k in range(n_vars)]).reshape(len(idx), n_vars, L)
        for got in three_entry_points(cm, "ml_lagrange", n_vars, pts_l):
            assert np.array_equal(got, coeffs_l[idx])


def test_concurrent_evaluations_beside_a_prove():
    fid, n = 3, 1 << 12
    enc = LigeroEncoding.new(fid, n)
    cm = LcCommit.commit(O.random_elems(fid, n, 9), enc)
    pts = [O.random_elems(fid, 3, 60 + t) for t in range(2)]
    outer, _ = enc.tensors(pts[0][0], cm.n_rows)
    root = cm.get_root()
    serial = [cm.eval(pt) for pt in pts]
    serial_pf = cm.prove(outer, enc, mk_transcript(Transcript, root, enc.get_n_col_opens())).to_bytes()
    got, errs = {}, []

    def evaluator(t):
        try:
            got[t] = [cm.eval(pts[t]) for _ in range(8)]
        except Exception as e:      # noqa: BLE001 -- reported below
            errs.append(e)

    def prover():
        try:
            got["pf"] = [cm.prove(outer, enc, mk_transcript(Transcript, root, enc.get_n_col_opens())).to_bytes() for _ in range(4)]
        except Exception as e:      # noqa: BLE001
            errs.append(e)

    threads = [threading.Thread(target=evaluator, args=(0,)), threading.Thread(target=evaluator, args=(1,)), threading.Thread(target=prover)]
    for th in threads:
        th.start()
    for th in threads:
        th.join()
    assert not errs, errs
    for t in range(2):
        assert all(np.array_equal(g, serial[t]) for g in got[t])
    assert all(pf == serial_pf for pf in got["pf"])


def test_states_and_shapes():
    fid, L = 3, 4
    lib = _lib.lib()
    enc = LigeroEncoding.new(fid, 1000)
    x = EC.mont(fid, [7])
    d_x = to_dev(x)
    out = np.full((2, L), CANARY, np.uint64)
    d_out = canaried(1, L)
    d_big = canaried(4096, L)
    # nothing committed
    cm = LcCommit(enc)
    assert lib.lcpce_eval(cm._h, 0, vp(x), 1, 1, vp(out)) == ERR_STATE
    assert lib.lcpce_eval_device(cm._h, 0, dptr(d_x), 1, 1, None, dptr(d_out)) == ERR_STATE
    assert lib.lcpce_eval_tensors_device(cm._h, dptr(d_big), dptr(d_big), 1, None, dptr(d_out)) == ERR_STATE
    # a sharded encoder
    senc = LigeroEncoding.new(fid, 1 << 12, shard=(0, 2))
    scm = LcCommit(senc)
    assert lib.lcpce_eval(scm._h, 0, vp(x), 1, 1, vp(out)) == ERR_STATE
    assert lib.lcpce_eval_device(scm._h, 0, dptr(d_x), 1, 1, None, dptr(d_out)) == ERR_STATE
    assert lib.lcpce_eval_tensors_device(scm._h, dptr(d_big), dptr(d_big), 1, None, dptr(d_out)) == ERR_STATE
    # a committed object: arguments
    cm = LcCommit.commit(O.random_elems(fid, 1000, 3), enc)
    n_rows, n_per_row = cm.n_rows, cm.n_per_row
    assert n_rows * n_per_row > 1000 and n_per_row & (n_per_row - 1) == 0
    # a multilinear basis wants both dimensions to be powers of two, and one variable per bit: the encoder's own 1000-coefficient
    # commit (whatever rows it chose), and one of 5 rows of 64
    cm5 = LcCommit.commit(O.random_elems(fid, 300, 3), LigeroEncoding.new_from_dims(fid, 64, 128))
    assert (cm5.n_rows, cm5.n_per_row) == (5, 64)
    for c in (cm, cm5):
        nv = (c.n_rows * c.n_per_row - 1).bit_length()
        z = EC.mont(fid, [3] * (nv + 1))
        ok = c.n_rows & (c.n_rows - 1) == 0
        assert ok == (c is cm)
        for basis in (1, 2):
            for n_pt in (nv - 1, nv, nv + 1):
                want = 0 if ok and n_pt == nv else ERR_ARG
                assert lib.lcpce_eval(c._h, basis, vp(z), n_pt, 1, vp(out if want else np.zeros((1, L), np.uint64))) == want
                assert lib.lcpce_eval_device(c._h, basis, dptr(to_dev(z)), n_pt, 1, None, dptr(d_out if want else canaried(1, L))) == want
    assert lib.lcpce_eval(cm._h, 3, vp(x), 1, 1, vp(out)) == ERR_ARG                   # unknown basis
    assert lib.lcpce_eval(cm._h, 0, vp(x), 2, 1, vp(out)) == ERR_ARG                   # powers takes one element
    assert lib.lcpce_eval(cm._h, 0, vp(x), 1, 0, vp(out)) == ERR_ARG                   # n_points
    assert lib.lcpce_eval(cm._h, 0, vp(x), 1, 65536, vp(out)) == ERR_ARG
    assert lib.lcpce_eval(cm._h, 0, None, 1, 1, vp(out)) == ERR_ARG
    assert lib.lcpce_eval(cm._h, 0, vp(x), 1, 1, None) == ERR_ARG
    assert lib.lcpce_eval(cm._h, 0, vp(O.ints_to_limbs([IC.modulus(fid)], L)), 1, 1, vp(out)) == ERR_ARG     # a point >= p
    assert lib.lcpce_eval_device(cm._h, 0, dptr(d_x), 1, 0, None, dptr(d_out)) == ERR_ARG
    assert lib.lcpce_eval_device(cm._h, 0, dptr(d_x), 1, 65536, None, dptr(d_out)) == ERR_ARG
    assert lib.lcpce_eval_device(cm._h, 0, C.c_void_p(d_big.data_ptr() + 8), 1, 1, None, dptr(d_out)) == ERR_ARG      # misaligned
    assert lib.lcpce_eval_device(cm._h, 0, dptr(d_x), 1, 1, None, C.c_void_p(d_big.data_ptr() + 8)) == ERR_ARG
    assert lib.lcpce_eval_tensors_device(cm._h, C.c_void_p(d_big.data_ptr() + 8), dptr(d_big), 1, None, dptr(d_out)) == ERR_ARG
    assert lib.lcpce_eval_tensors_device(cm._h, dptr(d_big), dptr(d_big), 0, None, dptr(d_out)) == ERR_ARG
    assert lib.lcpce_tensors_device(enc._h, 0, C.c_void_p(d_big.data_ptr() + 8), 1, 1, 4, 4, dptr(d_big), None, None) == ERR_ARG
    assert lib.lcpce_tensors_device(enc._h, 0, dptr(d_x), 1, 1, 4, 4, None, None, None) == ERR_ARG
    assert lib.lcpce_tensors_device(enc._h, 1, dptr(d_big), 4, 1, 4, 6, dptr(d_big), None, None) == ERR_ARG
    assert lib.lcpce_dot_device(enc._h, dptr(d_big), 0, dptr(d_big), 0, 0, 1, dptr(d_out), None) == ERR_ARG
    assert lib.lcpce_dot_device(enc._h, dptr(d_big), 0, dptr(d_big), 0, 4, 65536, dptr(d_out), None) == ERR_ARG
    assert lib.lcpce_dot_device(enc._h, dptr(d_big), 0, C.c_void_p(d_big.data_ptr() + 8), 0, 4, 1, dptr(d_out), None) == ERR_ARG
    torch.cuda.synchronize()
    assert (out == CANARY).all() and (read(d_out, 1, L) == CANARY).all() and (read(d_big, 4096, L) == CANARY).all()
    # and a good call after the refusals
    coeffs = EC.canon(fid, cm.coeffs())
    assert np.array_equal(cm.eval(x), EC.mont(fid, [horner(coeffs, 7, IC.modulus(fid))]))


def test_python_eval_numpy_and_torch():
    fid = 1
    enc = LigeroEncoding.new_ml(fid, 10)
    cm = LcCommit.commit(O.random_elems(fid, 1 << 10, 4), enc)
    xs = O.random_elems(fid, 3, 5)
    ev = cm.eval(xs)
    assert ev.shape == (3, enc.L) and np.array_equal(cm.eval(xs[0]), ev[:1])
    ev_t = cm.eval(to_dev(xs))
    assert torch.is_tensor(ev_t) and np.array_equal(ev_t.cpu().numpy().view(np.uint64), ev)
    outers, inners = zip(*(enc.tensors(x, cm.n_rows) for x in xs))
    assert np.array_equal(cm.eval_tensors(np.stack(outers), np.stack(inners)), ev)
    assert np.array_equal(cm.eval_tensors(to_dev(np.stack(outers)), to_dev(np.stack(inners))).cpu().numpy().view(np.uint64), ev)
    # the polynomial collapsed with the outer tensor, dotted with the inner one by the caller, is the same element
    p = IC.modulus(fid)
    poly = EC.canon(fid, cm.eval_outer(outers[0]))
    assert EC.mont(fid, [sum(a * b for a, b in zip(poly, EC.canon(fid, inners[0]))) % p]).tolist() == ev[:1].tolist()
    for basis in EC.ML_BASES:
        zs = O.random_elems(fid, 2 * 10, 6).reshape(2, 10, enc.L)
        ev = cm.eval(zs, basis=basis)
        assert ev.shape == (2, enc.L)
        assert np.array_equal(cm.eval(to_dev(zs), basis=basis).cpu().numpy().view(np.uint64), ev)
        o, i = enc.tensors(zs[1], cm.n_rows, basis=basis)
        assert np.array_equal(cm.eval_tensors(o, i), ev[1:])
    o, i = lcpc_amd.tensors(fid, xs[0], cm.n_rows, cm.n_per_row)
    assert np.array_equal(o, outers[0]) and np.array_equal(i, inners[0])

"""The transform extension (include/lcpc_hip_fft.h) on the device, through the C ABI and the Python wrappers: the device transform
against the host form and the oracle's fft_io, the inverse forms by round trip and by five-term bignum sums, the tie to the Ligero
encoder, the reference's own collapse-and-interpolate test, and the commit from evaluations against lcpc_commit_device on the
interpolated coefficients.  All comparisons are for equality."""
import ctypes as C
import functools

import numpy as np
import pytest

import lcpc_amd
from lcpc_amd import LcCommit, LcpcError, LigeroEncoding, SdigEncoding, Transcript, _lib

import fft_cases as FC
import oracle_lib as O
from common import mk_transcript

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

DEV = "cuda:0"
CANARY = FC.CANARY
ERR_ARG, ERR_STATE = FC.ERR_ARG, FC.ERR_STATE
BIG = (20, 21)          # the largest two-pass size and the first three-pass size of the product's plan (checked below)


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


@functools.lru_cache(maxsize=None)
def big_case(fid, log_n):
    """(x, fft_io(x)) by the oracle at a large size, computed once and only read: (n, L) Montgomery limbs"""
    x = O.random_elems(fid, 1 << log_n, 40 + log_n)
    X = x.copy()
    assert O.lib().lo_fft_io(fid, O.ptr(X), log_n) == 0
    return x, X


# ---- the device transform -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fid", FC.FIELDS)
def test_device_equals_host(fid):
    """log_n 0 .. 12, every form, out of place and in place, two vectors, on a stream of its own: canaries around the output stand
    and the input of an out-of-place call is unchanged"""
    enc, L = enc_of(fid), O.limbs(fid)
    st = torch.cuda.Stream(device=DEV)
    for log_n in range(0, 13):
        n = 1 << log_n
        x = np.stack([FC.mont(fid, FC.random_vector(fid, log_n, "dev", v)) for v in range(2)])
        d_x = to_dev(x)
        torch.cuda.synchronize()
        for form in FC.FORMS:
            want = np.stack([FC.host_fft(fid, form, x[v], log_n) for v in range(2)])
            buf = torch.full((2 * n + 16, L), CANARY, dtype=torch.int64, device=DEV)
            torch.cuda.synchronize()
            out = buf[8:8 + 2 * n].view(2, n, L)
            assert enc.fft(d_x, form, out=out, stream=st.cuda_stream) is out
            inp = d_x.clone()
            torch.cuda.synchronize()
            assert enc.fft(inp, form, out=inp, stream=st.cuda_stream) is inp
            st.synchronize()
            got = to_host(buf)
            assert (got[:8] == CANARY).all() and (got[-8:] == CANARY).all()
            assert np.array_equal(got[8:-8].reshape(2, n, L), want), (form, log_n)
            assert np.array_equal(to_host(inp), want), (form, log_n, "in place")
            assert np.array_equal(to_host(d_x), x)
    # the tables of the first sizes left the cache long ago: they are built again
    x = FC.mont(fid, FC.random_vector(fid, 3, "again"))
    assert np.array_equal(to_host(enc.fft(to_dev(x), "ifft_io")), FC.host_fft(fid, "ifft_io", x, 3))


def test_the_plan_boundaries():
    import k12_harness as K12
    top = K12.max_log_tile()
    assert len(K12.plan(BIG[0], top)) == 2 and len(K12.plan(BIG[0] + 1, top)) == 3 and BIG[1] == BIG[0] + 1


@pytest.mark.parametrize("log_n", BIG)
@pytest.mark.parametrize("fid", (0, 3))
def test_large_forward_is_the_oracles(fid, log_n):
    x, X = big_case(fid, log_n)
    enc = enc_of(fid)
    d_x = to_dev(x)
    assert np.array_equal(to_host(enc.fft(d_x, "fft_io")), X)


@pytest.mark.parametrize("log_n", BIG)
@pytest.mark.parametrize("fid", (0, 3))
def test_large_inverse_round_trips(fid, log_n):
    """the inverse forms undo the forward ones; fft_io itself is the oracle's (above)"""
    x, X = big_case(fid, log_n)
    enc = enc_of(fid)
    d_x, d_X = to_dev(x), to_dev(X)
    assert torch.equal(enc.fft(d_X, "ifft_oi"), d_x)
    nat = enc.fft(d_x, "fft_ii")
    assert torch.equal(enc.fft(nat, "ifft_ii"), d_x)
    x_rev = enc.fft(nat, "ifft_io")                              # x[j] at rev(j)
    assert torch.equal(enc.fft(x_rev, "fft_oi"), nat) and torch.equal(enc.fft(x_rev, "fft_oi", out=x_rev), nat)
    assert torch.equal(enc.fft(enc.fft(d_x, "ifft_io"), "fft_oi"), d_x)


@pytest.mark.parametrize("log_n", BIG)
@pytest.mark.parametrize("fid", (0, 3))
def test_large_inverse_five_term_sums(fid, log_n):
    """independent of any forward code: five non-zero X[k], at 0, 1, n / 2, n - 1 and a random place; every output is
    n^-1 sum_k X[k] w^(-jk), and 4096 sampled outputs are compared with bignum"""
    F = FC.field(fid)
    n = 1 << log_n
    rnd = FC.rng("five", fid, log_n)
    ks = [0, 1, n // 2, n - 1, rnd.randrange(2, n // 2)]
    vals = [rnd.randrange(1, F.p) for _ in ks]
    vals[1] = F.p - 1
    winv = pow(FC.root(fid, log_n), -1, F.p)
    ninv = pow(n, -1, F.p)
    js = sorted({0, 1, n // 2, n - 1} | {rnd.randrange(n) for _ in range(4092)})
    want = FC.mont(fid, [ninv * sum(v * pow(winv, j * k % n, F.p) for k, v in zip(ks, vals)) % F.p for j in js])
    enc = enc_of(fid)
    rv = lambda i: FC.rev(i, log_n)
    for form in ("ifft_ii", "ifft_io", "ifft_oi"):
        X = torch.zeros((n, F.L), dtype=torch.int64, device=DEV)
        at = [rv(k) if form[-2] == "o" else k for k in ks]
        X[at] = to_dev(FC.mont(fid, vals))
        got = enc.fft(X, form)
        idx = [rv(j) if form[-1] == "o" else j for j in js]
        assert np.array_equal(to_host(got[idx]), want), form


# ---- the encoder's transform ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fid", FC.FIELDS)
def test_encoder_tie(fid):
    """every row of a Ligero commitment matrix is FFT_IO of its coefficient row, zero-padded to n_cols: the new transform against
    the oracle-pinned encoder and its root"""
    for enc, n in ((enc_of(fid), 300), (LigeroEncoding.new(fid, 1 << 12), (1 << 12) - 7)):
        cm = LcCommit.commit(O.random_elems(fid, n, 5), enc)
        rows = np.zeros((cm.n_rows, cm.n_cols, enc.L), np.uint64)
        rows[:, :cm.n_per_row] = cm.coeffs().reshape(cm.n_rows, cm.n_per_row, enc.L)
        got = enc.fft(to_dev(rows), "fft_io")
        assert np.array_equal(to_host(got).reshape(cm.n_rows, cm.n_cols, enc.L), cm.comm().reshape(cm.n_rows, cm.n_cols, enc.L))
        assert np.array_equal(FC.host_fft(fid, "fft_io", rows[-1], cm.n_cols.bit_length() - 1), cm.comm(cm.n_rows - 1, 1))      # (and the host form)


@pytest.mark.parametrize("fid", FC.FIELDS)
def test_collapsed_codeword_interpolates_to_the_collapsed_polynomial(fid):
    """lcpc-2d's own commit test, restated: collapse the rows of comm with the outer tensor of a point, IFFT_OI on the device, the
    elements from n_per_row on are zero, and the dot product with the inner tensor is the polynomial's value at the point"""
    F = FC.field(fid)
    for enc, n in ((enc_of(fid), 300), (LigeroEncoding.new(fid, 1 << 12), 1 << 12)):
        cm = LcCommit.commit(O.random_elems(fid, n, 6), enc)
        x = FC.rng("collapse", fid, n).randrange(F.p)
        outer, inner = enc.tensors(FC.mont(fid, [x]), cm.n_rows)
        o, i = FC.canon(fid, outer), FC.canon(fid, inner)
        comm = FC.canon(fid, cm.comm())
        nc = cm.n_cols
        collapsed = [sum(o[r] * comm[r * nc + c] for r in range(cm.n_rows)) % F.p for c in range(nc)]
        poly = to_host(enc.fft(to_dev(FC.mont(fid, collapsed)), "ifft_oi"))
        assert (poly[cm.n_per_row:] == 0).all()
        p = FC.canon(fid, poly[:cm.n_per_row])
        assert FC.mont(fid, [sum(a * b for a, b in zip(p, i)) % F.p]).tolist() == cm.eval(FC.mont(fid, [x])).tolist()


# ---- commit from evaluations ---------------------------------------------------------------------------------------------------------
def same_commitment(a, b):
    assert (a.n_rows, a.n_per_row, a.n_cols, a.n_hashes) == (b.n_rows, b.n_per_row, b.n_cols, b.n_hashes)
    assert a.get_root() == b.get_root()
    assert (a.hashes() == b.hashes()).all()
    assert (a.coeffs() == b.coeffs()).all()
    assert (a.comm() == b.comm()).all()


def commit_evals_matrix(fid, enc, log_ns):
    F = FC.field(fid)
    ref, cm = LcCommit(enc), LcCommit(enc)           # refilled: a smaller commit finds the buffers of a larger one
    for log_n in log_ns:
        n = 1 << log_n
        coeffs = FC.random_vector(fid, log_n, "evals")
        evals = FC.dft(fid, coeffs)                  # evals[i] = p(w^i)
        d_c = to_dev(FC.mont(fid, coeffs))
        want = LcCommit.commit_device(d_c.data_ptr(), n, enc, into=ref)
        for order in ("natural", "bitrev"):
            e = FC.mont(fid, evals if order == "natural" else FC.permute(evals, log_n))
            d_e = to_dev(e)
            for src in (d_e, e):
                got = LcCommit.commit_evals(src, enc, order=order, into=cm)
                same_commitment(got, want)
                assert (got.coeffs()[:n] == FC.mont(fid, coeffs)).all() and (got.coeffs()[n:] == 0).all()
            assert np.array_equal(to_host(d_e), e)  # the caller's buffer is only read
        # a proof from the object verifies, and the polynomial takes the committed values on the subgroup
        x = FC.rng("pt", fid, log_n).randrange(F.p)
        outer, inner = enc.tensors(FC.mont(fid, [x]), got.n_rows)
        root = got.get_root()
        pf = got.prove(outer, enc, mk_transcript(Transcript, root, enc.get_n_col_opens()))
        ev = pf.verify(root, outer, inner, enc, mk_transcript(Transcript, root, enc.get_n_col_opens()))
        assert FC.canon(fid, ev) == [sum(c * pow(x, k, F.p) for k, c in enumerate(coeffs)) % F.p]
        w = FC.root(fid, log_n)
        idx = sorted({0, n - 1, n // 2} | {FC.rng("i", log_n, k).randrange(n) for k in range(5)})
        assert np.array_equal(got.eval(FC.mont(fid, [pow(w, i, F.p) for i in idx])), FC.mont(fid, [evals[i] for i in idx]))


@pytest.mark.parametrize("fid", FC.FIELDS)
def test_commit_evals_ligero(fid):
    commit_evals_matrix(fid, enc_of(fid), (12, 0, 7))


@pytest.mark.parametrize("fid", (1, 3))
def test_commit_evals_brakedown(fid):
    commit_evals_matrix(fid, sdig_enc(fid, 40), (12, 0, 7))          # 103 rows: the position-major branch; 1 and 4 rows: row-major


@pytest.mark.parametrize("digest", ("sha256", "blake2b"))
def test_commit_evals_chained_digests(digest):
    commit_evals_matrix(3, LigeroEncoding.new_from_dims(3, 64, 128, digest=digest), (12, 0, 7))
    commit_evals_matrix(3, sdig_enc(3, 40, digest), (12, 7))


def test_async_commit_evals_then_prove():
    """commit_evals(sync=False) on a stream of its own followed at once by prove: the bytes of the synchronous run"""
    fid, log_n = 3, 12
    enc = enc_of(fid)
    e = FC.mont(fid, FC.random_vector(fid, log_n, "async"))
    outer = O.random_elems(fid, (1 << log_n) // 64, 2)
    proofs = []
    for sync in (True, False):
        st = torch.cuda.Stream(device=DEV)
        d = to_dev(e)
        torch.cuda.synchronize()
        cm = LcCommit.commit_evals(d, enc, stream=st.cuda_stream, sync=sync)
        assert (cm._coeffs_ref is None) == sync
        proofs.append(cm.prove(outer, enc, Transcript(b"evals")).to_bytes())
    assert proofs[0] == proofs[1]


def test_failing_calls_leave_a_commitment_as_it_was():
    fid, log_n = 3, 7
    F = FC.field(fid)
    lib = _lib.lib()
    enc = enc_of(fid)
    e = FC.mont(fid, FC.random_vector(fid, log_n, "fail"))
    d_e = to_dev(e)
    cm = LcCommit.commit_evals(d_e, enc)
    root, coeffs = cm.get_root(), cm.coeffs().copy()
    outer = O.random_elems(fid, cm.n_rows, 2)
    pf = cm.prove(outer, enc, Transcript(b"x")).to_bytes()
    bad = e.copy()
    bad[5] = O.ints_to_limbs([F.p], F.L)[0]
    calls = (lambda h: lib.lcpcf_commit_evals_device(h, 0, dptr(d_e), F.S + 1, None, None),
             lambda h: lib.lcpcf_commit_evals_device(h, 0, dptr(d_e), 33, None, None),
             lambda h: lib.lcpcf_commit_evals_device(h, 2, dptr(d_e), log_n, None, None),
             lambda h: lib.lcpcf_commit_evals_device(h, 0, None, log_n, None, None),
             lambda h: lib.lcpcf_commit_evals_device(h, 0, dptr(d_e, 8), log_n - 1, None, None),
             lambda h: lib.lcpcf_commit_evals(h, 0, FC.vp(e), F.S + 1, None),
             lambda h: lib.lcpcf_commit_evals(h, 2, FC.vp(e), log_n, None),
             lambda h: lib.lcpcf_commit_evals(h, 0, None, log_n, None),
             lambda h: lib.lcpcf_commit_evals(h, 1, FC.vp(bad), log_n, None))
    for k, call in enumerate(calls):
        assert call(cm._h) == ERR_ARG, k
        assert cm.get_root() == root and (cm.coeffs() == coeffs).all()
        assert cm.prove(outer, enc, Transcript(b"x")).to_bytes() == pf
    # a sharded encoder: as lcpc_commit_device
    senc = LigeroEncoding.new(fid, 1 << 12, shard=(0, 2))
    scm = LcCommit(senc)
    assert lib.lcpc_commit_device(scm._h, dptr(d_e), 1 << log_n, None, 0, None) == ERR_STATE
    assert lib.lcpcf_commit_evals_device(scm._h, 0, dptr(d_e), log_n, None, None) == ERR_STATE
    assert lib.lcpcf_commit_evals(scm._h, 0, FC.vp(e), log_n, None) == ERR_STATE
    # an empty object stays empty
    em = LcCommit(enc)
    assert lib.lcpcf_commit_evals_device(em._h, 0, dptr(d_e), 33, None, None) == ERR_ARG
    with pytest.raises(LcpcError) as err:
        em.prove(outer, enc, Transcript(b"x"))
    assert err.value.code == lcpc_amd.ERR_STATE


def test_device_transform_refusals():
    """every error is settled before any launch: the output keeps its canaries"""
    fid, log_n = 3, 6
    F = FC.field(fid)
    lib = _lib.lib()
    enc = enc_of(fid)
    n = 1 << log_n
    d_x = to_dev(FC.mont(fid, FC.random_vector(fid, log_n, "refuse")))
    d_o = torch.full((2 * n, F.L), CANARY, dtype=torch.int64, device=DEV)
    torch.cuda.synchronize()
    f = lib.lcpcf_fft_device
    assert f(None, 1, dptr(d_x), dptr(d_o), log_n, 1, None) == ERR_ARG
    assert f(enc._h, 6, dptr(d_x), dptr(d_o), log_n, 1, None) == ERR_ARG
    assert f(enc._h, 1, None, dptr(d_o), log_n, 1, None) == ERR_ARG and f(enc._h, 1, dptr(d_x), None, log_n, 1, None) == ERR_ARG
    assert f(enc._h, 1, dptr(d_x, 8), dptr(d_o), log_n - 1, 1, None) == ERR_ARG             # misaligned (Ft255: 16 bytes)
    assert f(enc._h, 1, dptr(d_x), dptr(d_o, 8), log_n, 1, None) == ERR_ARG
    assert f(enc._h, 1, dptr(d_x), dptr(d_o), 33, 1, None) == ERR_ARG and f(enc._h, 1, dptr(d_x), dptr(d_o), F.S + 1, 1, None) == ERR_ARG
    assert f(enc._h, 1, dptr(d_x), dptr(d_o), log_n, 0, None) == ERR_ARG and f(enc._h, 1, dptr(d_x), dptr(d_o), log_n, 65536, None) == ERR_ARG
    assert f(enc._h, 1, dptr(d_x), dptr(d_o), 32, 128, None) == ERR_ARG                     # 2^39 elements
    assert f(enc._h, 1, dptr(d_o), dptr(d_o, 32), log_n, 1, None) == ERR_ARG                # overlap without being equal
    assert f(enc._h, 1, dptr(d_o, 32 * (n - 1)), dptr(d_o), log_n, 1, None) == ERR_ARG
    torch.cuda.synchronize()
    assert (to_host(d_o) == CANARY).all()
    assert f(enc._h, 1, dptr(d_o), dptr(d_o, 32 * n), log_n, 1, None) == 0                  # adjacent ranges do not overlap
    assert f(enc._h, 1, dptr(d_x), dptr(d_o), log_n, 1, None) == 0
    torch.cuda.synchronize()
    # Ft63 and Ft191 elements need 8-byte alignment only
    e0 = enc_of(0)
    x0 = to_dev(FC.mont(0, FC.random_vector(0, 3, "a8")))
    buf = torch.zeros((9, 1), dtype=torch.int64, device=DEV)
    assert f(e0._h, 1, dptr(x0), dptr(buf, 8), 3, 1, None) == 0
    torch.cuda.synchronize()
    assert np.array_equal(to_host(buf)[1:], FC.host_fft(0, "fft_io", to_host(x0), 3))

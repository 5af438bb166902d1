"""Concurrent prove and verify on ONE commitment and ONE encoder (include/lcpc_hip.h "Threads").

LcCommit::prove takes &self and LcEvalProof::verify takes &E (lcpc-2d/src/lib.rs:304-311, 518-527): a Rayon caller proves many
points of one commitment, or verifies many proofs under one encoder, at once.  The library runs such calls side by side, each in
a working set of its own; every call must return exactly the bytes and status it returns alone, a refill of the object must wait
for the readers in flight, and callers beyond the pool's eight sets must wait, not fail."""
import statistics
import threading
import time

import numpy as np
import pytest

from common import mk_transcript
from lcpc_amd import LcCommit, LcEvalProof, LcpcError, LigeroEncoding, SdigEncoding, Transcript

pytestmark = pytest.mark.gpu


def run_threads(fn, args):
    """fn(*a) on one thread per entry of args, started together; returns the exceptions raised"""
    errs, start = [], threading.Barrier(len(args))

    def body(a):
        try:
            start.wait()
            fn(*a)
        except Exception as ex:      # pragma: no cover
            errs.append(repr(ex))

    th = [threading.Thread(target=body, args=(a,)) for a in args]
    for t in th:
        t.start()
    for t in th:
        t.join(600)
    assert not any(t.is_alive() for t in th), "a thread did not finish"
    return errs


def random_elems_fast(L, n, seed):
    """n reduced elements of Ft255 (p > 2^254): random limbs, the top one below 2^60"""
    a = np.random.default_rng(seed).integers(0, 2 ** 64 - 1, (n, L), dtype=np.uint64, endpoint=True)
    a[:, L - 1] &= np.uint64((1 << 60) - 1)
    return a


def verify_rc(pf_bytes, root, outer, inner, enc, nco):
    try:
        ev = LcEvalProof.from_bytes(pf_bytes, enc.L).verify(root, outer, inner, enc, mk_transcript(Transcript, root, nco))
        return 0, bytes(ev.tobytes())
    except LcpcError as e:
        return e.code, None


# ---- 1. bytes under concurrency --------------------------------------------------------------------------------------------
def _setup(O, kind):
    """(enc, commitment, oracle encoder + commitment or None, field id)"""
    if kind == "ligero_ft255":
        fid, n_per_row, n_cols, n_rows = 3, 32768, 65536, 24
        enc, oenc = LigeroEncoding.new_from_dims(fid, n_per_row, n_cols), O.Encoding.ligero_from_dims(fid, n_per_row, n_cols)
        coeffs = O.random_elems(fid, n_rows * n_per_row - 7, 91)
    elif kind == "sdig_ft127":
        fid, n = 1, 1 << 16
        enc, oenc = SdigEncoding.new(fid, n, 7), O.Encoding.sdig(fid, n, 7)
        coeffs = O.random_elems(fid, n, 92)
    else:                            # SHA3-256 / BLAKE2b digest: the library's serial prove / verify is the reference
        fid, n = 3, 1 << 16           # (test_gpu_sha3.py, test_gpu_blake2b.py and test_gpu_digests_*.py check it)
        enc, oenc = LigeroEncoding.new(fid, n, digest="blake2b" if kind.startswith("blake2b") else "sha3_256"), None
        coeffs = O.random_elems(fid, n, 93)
    c = LcCommit.commit(coeffs, enc)
    oc = O.Commit.commit(coeffs, oenc, n_threads=8) if oenc else None
    if oc is not None:
        assert c.get_root() == oc.get_root()
    return enc, c, oenc, oc, fid


@pytest.mark.parametrize("kind", ["ligero_ft255", "sdig_ft127", "sha3_ligero_ft255", "blake2b_ligero_ft255"])
def test_concurrent_prove_verify_bytes(oracle, kind):
    O = oracle
    enc, c, oenc, oc, fid = _setup(O, kind)
    root, nco = c.get_root(), enc.get_n_col_opens()
    T, R = 8, 3
    outers = [[O.random_elems(fid, c.n_rows, 1000 + 10 * k + r) for r in range(R)] for k in range(T)]
    inners = [[O.random_elems(fid, c.n_per_row, 2000 + 10 * k + r) for r in range(R)] for k in range(T)]
    if oc is not None:
        want = [[oc.prove(outers[k][r], oenc, mk_transcript(O.Transcript, root, nco))[0] for r in range(R)] for k in range(T)]
    else:
        want = [[c.prove(outers[k][r], enc, mk_transcript(Transcript, root, nco)).to_bytes() for r in range(R)] for k in range(T)]
    got = [[None] * R for _ in range(T)]

    def prove(k):
        for r in range(R):
            got[k][r] = c.prove(outers[k][r], enc, mk_transcript(Transcript, root, nco)).to_bytes()

    assert not run_threads(prove, [(k,) for k in range(T)])
    for k in range(T):
        for r in range(R):
            assert got[k][r] == want[k][r], (k, r)

    # every proof verified at once under the one encoder: the evaluation the oracle's verifier returns
    if oc is not None:
        want_ev = []
        for k in range(T):
            row = []
            for r in range(R):
                orc, oev = O.verify(oenc, root, outers[k][r], inners[k][r], want[k][r], mk_transcript(O.Transcript, root, nco))
                assert orc == 0
                row.append(bytes(oev.tobytes()))
            want_ev.append(row)
    else:
        want_ev = [[verify_rc(want[k][r], root, outers[k][r], inners[k][r], enc, nco)[1] for r in range(R)] for k in range(T)]
    got_ev = [[None] * R for _ in range(T)]

    def verify(k):
        for r in range(R):
            rc, ev = verify_rc(got[k][r], root, outers[k][r], inners[k][r], enc, nco)
            assert rc == 0, rc
            got_ev[k][r] = ev

    assert not run_threads(verify, [(k,) for k in range(T)])
    assert got_ev == want_ev

    # mutated proofs, verified at once: the same VerifierError codes as one at a time
    base = bytearray(want[0][0])
    hdr = 16
    muts = []
    rng = np.random.default_rng(7)
    for i in range(16):
        b = bytearray(base)
        if i == 0:
            b = b[: len(b) // 2]                                   # truncated
        elif i == 1:
            b[0] ^= 1                                              # n_cols
        else:
            pos = int(rng.integers(hdr, len(b)))
            b[pos] ^= 1 << int(rng.integers(0, 8))
        muts.append(bytes(b))
    outer, inner = outers[0][0], inners[0][0]
    serial = [verify_rc(m, root, outer, inner, enc, nco)[0] for m in muts]
    conc = [None] * len(muts)

    def verify_mut(k):
        for i in range(k, len(muts), T):
            conc[i] = verify_rc(muts[i], root, outer, inner, enc, nco)[0]

    assert not run_threads(verify_mut, [(k,) for k in range(T)])
    assert conc == serial
    assert all(rc != 0 for rc in serial)


# ---- 2. overlap --------------------------------------------------------------------------------------------------------------
def test_concurrent_proves_and_verifies_overlap():
    """2^24 Ft255 Ligero: a prove is almost all host transcript (serial STROBE), so four proves of one commitment at once take
    about as long as one -- they used to queue up behind a whole-call lock (about 4x).  The same for four verifies under one
    encoder.  2x leaves room for a noisy host on both sides."""
    fid, n, L = 3, 1 << 24, 4
    enc = LigeroEncoding.new(fid, n)
    c = LcCommit.commit(random_elems_fast(L, n, 5), enc)
    root, nco = c.get_root(), enc.get_n_col_opens()
    outers = [random_elems_fast(L, c.n_rows, 10 + k) for k in range(4)]
    inner = random_elems_fast(L, c.n_per_row, 20)

    def one_prove(k):
        return c.prove(outers[k], enc, mk_transcript(Transcript, root, nco))

    pfs = [one_prove(k) for k in range(4)]            # (warm: working sets, proof buffers)
    t_single = []
    for _ in range(5):
        t0 = time.perf_counter()
        one_prove(0)
        t_single.append(time.perf_counter() - t0)
    single = statistics.median(t_single)
    assert single >= 0.003, "the overlap test needs a prove of >= 3 ms, got %.2f ms" % (single * 1e3)
    walls = []
    for _ in range(2):
        t0 = time.perf_counter()
        assert not run_threads(one_prove, [(k,) for k in range(4)])
        walls.append(time.perf_counter() - t0)
    wall = min(walls)
    assert wall <= 2.0 * single, "4 proves at once: %.2f ms, one: %.2f ms" % (wall * 1e3, single * 1e3)

    blobs = [p.to_bytes() for p in pfs]

    def one_verify(k):
        LcEvalProof.from_bytes(blobs[k], L).verify(root, outers[k], inner, enc, mk_transcript(Transcript, root, nco))

    for k in range(4):
        one_verify(k)
    t_single = []
    for _ in range(5):
        t0 = time.perf_counter()
        one_verify(0)
        t_single.append(time.perf_counter() - t0)
    single_v = statistics.median(t_single)
    walls = []
    for _ in range(2):
        t0 = time.perf_counter()
        assert not run_threads(one_verify, [(k,) for k in range(4)])
        walls.append(time.perf_counter() - t0)
    wall_v = min(walls)
    assert wall_v <= 2.0 * single_v, "4 verifies at once: %.2f ms, one: %.2f ms" % (wall_v * 1e3, single_v * 1e3)


# ---- 3. a refill waits for the readers in flight -----------------------------------------------------------------------------
def test_refill_waits_for_readers(oracle):
    import torch
    O, fid, n = oracle, 3, 1 << 16
    enc = LigeroEncoding.new(fid, n)
    nco = enc.get_n_col_opens()
    srcs = [O.random_elems(fid, n, 501), O.random_elems(fid, n, 502)]
    dev = [torch.from_numpy(s.view(np.int64).copy()).cuda() for s in srcs]
    torch.cuda.synchronize()
    # the references: one commitment per source, proved alone.  The transcript leaves the root out, so that a proof's bytes
    # depend only on which commitment the object held while it was proved
    ref = [LcCommit.commit(s, enc) for s in srcs]
    roots = [r.get_root() for r in ref]
    assert roots[0] != roots[1]
    outer = O.random_elems(fid, ref[0].n_rows, 503)
    inner = O.random_elems(fid, ref[0].n_per_row, 504)

    def tr():
        t = Transcript(b"refill test")
        t.append_message(b"ncols", int(nco).to_bytes(8, "big"))
        return t

    want = [r.prove(outer, enc, tr()).to_bytes() for r in ref]
    c = LcCommit.commit_device(dev[0].data_ptr(), n, enc)
    assert c.get_root() == roots[0]
    got = []
    done = threading.Event()

    def prover():
        try:
            for _ in range(40):
                got.append(c.prove(outer, enc, tr()).to_bytes())
        finally:
            done.set()

    def refiller():
        k = 1
        while not done.is_set():
            LcCommit.commit_device(dev[k].data_ptr(), n, enc, into=c)
            k ^= 1

    assert not run_threads(lambda f: f(), [(prover,), (refiller,)])
    assert len(got) == 40
    seen = set()
    for pf in got:
        assert pf in want, "a proof matches neither commitment"
        i = want.index(pf)
        seen.add(i)
        ev = LcEvalProof.from_bytes(pf, enc.L).verify(roots[i], outer, inner, enc, tr())
        assert ev is not None
    assert seen, seen


# ---- 4. callers beyond the pool wait -----------------------------------------------------------------------------------------
def test_twelve_callers_one_commitment(oracle):
    O, fid, n = oracle, 3, 1 << 16
    enc, oenc = LigeroEncoding.new(fid, n), O.Encoding.ligero(fid, n)
    coeffs = O.random_elems(fid, n, 601)
    c, oc = LcCommit.commit(coeffs, enc), O.Commit.commit(coeffs, oenc, n_threads=8)
    root, nco = c.get_root(), enc.get_n_col_opens()
    assert root == oc.get_root()
    T = 12
    outers = [O.random_elems(fid, c.n_rows, 610 + k) for k in range(T)]
    inner = O.random_elems(fid, c.n_per_row, 630)
    want = [oc.prove(outers[k], oenc, mk_transcript(O.Transcript, root, nco))[0] for k in range(T)]
    got = [None] * T

    def prove(k):
        for _ in range(2):
            got[k] = c.prove(outers[k], enc, mk_transcript(Transcript, root, nco)).to_bytes()

    assert not run_threads(prove, [(k,) for k in range(T)])
    assert got == want
    evs = [None] * T

    def verify(k):
        evs[k] = verify_rc(got[k], root, outers[k], inner, enc, nco)

    assert not run_threads(verify, [(k,) for k in range(T)])
    for k in range(T):
        orc, oev = O.verify(oenc, root, outers[k], inner, want[k], mk_transcript(O.Transcript, root, nco))
        assert evs[k] == (orc, bytes(oev.tobytes()))

    # collapse and open from twelve threads beside each other: the serial results
    cols = np.arange(0, c.n_cols, max(1, c.n_cols // 37), dtype=np.uint64)[:37]
    want_poly = [c.eval_outer(outers[k]) for k in range(T)]
    want_open = c.open_columns(cols)
    res = [None] * T

    def read(k):
        res[k] = (c.eval_outer(outers[k]), c.open_columns(cols))

    assert not run_threads(read, [(k,) for k in range(T)])
    for k in range(T):
        assert np.array_equal(res[k][0], want_poly[k])
        assert np.array_equal(res[k][1][0], want_open[0]) and np.array_equal(res[k][1][1], want_open[1])

"""Commit from plain integers (include/lcpc_hip_ints.h) on the device: the widening kernel K9 directly, the two commit entry points
against lcpc_commit_device on the bignum reference limbs, plain integers end to end, ordering and errors."""
import ctypes as C
import random

import numpy as np
import pytest

import lcpc_amd
from lcpc_amd import LcCommit, LcpcError, LigeroEncoding, SdigEncoding, Transcript, _lib

import ints_cases as IC
import oracle_lib as O
from common import mk_transcript

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

DEV = "cuda:0"
CANARY = 0x5A5A5A5A5A5A5A5A
SIZES = (1, 2, 3, 63, 64, 65, 255, 256, 257, 1023, 4099)


def vp(a):
    return a.ctypes.data_as(C.c_void_p)


def to_dev(a):
    """a numpy integer array -> a device tensor of the same bytes (unsigned storage travels as the signed dtype of its width)"""
    signed = {np.dtype(np.uint32): np.int32, np.dtype(np.uint64): np.int64}.get(a.dtype)
    return torch.from_numpy(a.view(signed) if signed else a).to(DEV)


def values_with_edges(kind, fid, n, seed):
    """n values of `kind`: random, with E(kind) cycled over the first, the last and the block-boundary positions (a block is 256 lanes)"""
    vals = IC.random_values(kind, fid, n, seed)
    E = IC.edges(kind, fid)
    pos = list(range(min(n, len(E)))) + list(range(max(0, n - len(E)), n))
    for b in range(256, n, 256):
        pos += [b - 1, b]
    for k, i in enumerate(pos):
        vals[i] = E[k % len(E)]
    return vals


def host_from_ints(fid, kind, arr, n):
    out = np.zeros((n, O.limbs(fid)), np.uint64)
    assert _lib.lib().lcpci_from_ints(fid, _lib.INTS_KINDS[kind], vp(arr), n, vp(out)) == 0
    return out


def device_from_ints(enc, kind, arr, n, off=0):
    """lcpci_from_ints_device on arr[off:], the input `off` elements into its allocation; the output followed by canaries"""
    L = enc.L
    d_in = to_dev(arr)
    d_out = torch.full((n * L + 64,), CANARY, dtype=torch.int64, device=DEV)
    esz = arr.dtype.itemsize * (L if kind == "wide" else 1)
    rc = _lib.lib().lcpci_from_ints_device(enc._h, _lib.INTS_KINDS[kind], C.c_void_p(d_in.data_ptr() + off * esz), n,
                                           C.c_void_p(d_out.data_ptr()), None)
    assert rc == 0
    torch.cuda.synchronize()
    out = d_out.cpu().numpy().view(np.uint64)
    assert (out[n * L:] == CANARY).all(), "canaries behind the output"
    return out[:n * L].reshape(n, L)


@pytest.fixture(scope="module")
def small_encs():
    return {fid: LigeroEncoding.new_from_dims(fid, 64, 128) for fid in IC.FIELDS}


@pytest.mark.parametrize("fid", IC.FIELDS)
@pytest.mark.parametrize("kind", IC.KINDS)
def test_kernel_against_host(small_encs, fid, kind):
    enc, L = small_encs[fid], O.limbs(fid)
    for n in SIZES:
        vals = values_with_edges(kind, fid, n, 100 * n + fid)
        arr = IC.pack(kind, vals, L)
        want = host_from_ints(fid, kind, arr, n)
        if n == 257:
            assert (want == IC.reference(fid, vals)).all()                # (the host call is tied to bignum in test_ints_abi.py)
        assert (device_from_ints(enc, kind, arr, n) == want).all(), n
    # the input 1, 2, 3 elements into its allocation: only the element's own alignment is asked for
    n = 257
    vals = values_with_edges(kind, fid, n + 3, 5)
    arr = IC.pack(kind, vals, L)
    for off in (1, 2, 3):
        want = host_from_ints(fid, kind, arr[off:], n)
        assert (device_from_ints(enc, kind, arr, n, off) == want).all(), off


# ---- commits --------------------------------------------------------------------------------------------------------------------
def sdig_enc(fid, n_per_row, digest="blake3"):
    _, _, n_cols = O.Encoding.sdig_from_dims(fid, n_per_row, 0, 3, 3).get_dims(n_per_row)
    return SdigEncoding.new_from_dims(fid, n_per_row, n_cols, 3, 3, digest=digest)


ENCODERS = {
    "ligero": lambda fid, digest: LigeroEncoding.new_from_dims(fid, 64, 128, digest=digest),
    "brakedown-rows": lambda fid, digest: sdig_enc(fid, 256, digest),           # 4 / 16 rows: row-major commitment
    "brakedown-t": lambda fid, digest: sdig_enc(fid, 40, digest),               # 26 / 103 rows: the position-major branch
}


def same_commitment(a, b):
    assert (a.n_rows, a.n_per_row, a.n_cols, a.n_hashes) == (b.n_rows, b.n_per_row, b.n_cols, b.n_hashes)
    assert a.get_root() == b.get_root()
    assert (a.hashes() == b.hashes()).all()
    assert (a.coeffs() == b.coeffs()).all()
    assert (a.comm() == b.comm()).all()


def reference_commit(enc, fid, vals, into=None):
    """lcpc_commit_device from the bignum reference limbs of vals"""
    ref = torch.from_numpy(IC.reference(fid, vals).view(np.int64)).to(DEV)
    return LcCommit.commit_device(ref.data_ptr(), len(vals), enc, into=into)


def device_commit_matrix(fid, digest):
    for name, make in ENCODERS.items():
        enc = make(fid, digest)
        ref = LcCommit(enc)
        for kind in ("i32", "u64", "wide"):
            cm = LcCommit(enc)                         # refilled: every commit after the first finds the buffers of a larger one
            for n in ((1 << 12) - 5, 1 << 10, (1 << 10) - 3):
                if name == "brakedown-t":
                    assert -(-n // enc.n_per_row) >= 24
                elif name == "brakedown-rows":
                    assert -(-n // enc.n_per_row) < 24
                vals = values_with_edges(kind, fid, n, n + fid)
                got = LcCommit.commit_ints(to_dev(IC.pack(kind, vals, enc.L)), enc, kind=kind, into=cm)
                same_commitment(got, reference_commit(enc, fid, vals, into=ref))
                assert (got.coeffs()[n:] == 0).all()   # the ragged tail, behind a larger earlier fill


@pytest.mark.parametrize("fid", IC.FIELDS)
def test_device_commit(fid):
    device_commit_matrix(fid, "blake3")


@pytest.mark.parametrize("digest", ("sha256", "blake2b"))
def test_device_commit_chained_digests(digest):
    device_commit_matrix(3, digest)


@pytest.mark.parametrize("pinned", (False, True), ids=("pageable", "pinned"))
def test_host_commit_small(pinned):
    n = (1 << 12) - 5
    for fid in IC.FIELDS:
        for name in ("ligero", "brakedown-t"):
            enc = ENCODERS[name](fid, "blake3")
            for kind in ("i32", "u64", "wide"):
                vals = values_with_edges(kind, fid, n, 3 + fid)
                arr = IC.pack(kind, vals, enc.L)
                if pinned:
                    keep = to_dev(arr).cpu().pin_memory()
                    assert keep.is_pinned()
                    arr = keep.numpy().view(arr.dtype)
                same_commitment(LcCommit.commit_ints(arr, enc, kind=kind), reference_commit(enc, fid, vals))


@pytest.mark.parametrize("digest", ("blake3", "sha256"))
def test_host_commit_row_batches(digest):
    fid, n = 3, (1 << 21) + 12345
    enc = LigeroEncoding.new(fid, n, digest=digest)
    n_rows, n_per_row, n_cols = enc.get_dims(n)
    assert n_rows >= 16 and n * 32 >= 64 << 20            # the row-batch path, not the small one
    rnd = np.random.default_rng(11)
    arr = rnd.integers(0, 1 << 32, n, dtype=np.uint32)    # pageable
    E = np.array(IC.edges("u32", fid), np.uint32)
    arr[:E.size] = E
    arr[-E.size:] = E
    got = LcCommit.commit_ints(arr, enc)
    d_in = to_dev(arr)
    d_ref = torch.empty((n, enc.L), dtype=torch.int64, device=DEV)
    assert _lib.lib().lcpci_from_ints_device(enc._h, _lib.INTS_KINDS["u32"], C.c_void_p(d_in.data_ptr()), n, C.c_void_p(d_ref.data_ptr()), None) == 0
    torch.cuda.synchronize()
    ref = LcCommit.commit_device(d_ref.data_ptr(), n, enc)
    assert (got.n_rows, got.n_per_row, got.n_cols) == (n_rows, n_per_row, n_cols) == (ref.n_rows, ref.n_per_row, ref.n_cols)
    assert got.get_root() == ref.get_root()
    assert (got.hashes() == ref.hashes()).all()
    rows = sorted({0, n_rows - 1, n_rows // 16, n_rows // 16 + 1} | set(int(r) for r in rnd.integers(0, n_rows, 12)))
    for r in rows:                                        # 16 rows x 256 columns: 4096 entries of each matrix
        cc = rnd.integers(0, n_per_row, 256)
        assert (got.coeffs(r, 1)[cc] == ref.coeffs(r, 1)[cc]).all()
        cm = rnd.integers(0, n_cols, 256)
        assert (got.comm(r, 1)[cm] == ref.comm(r, 1)[cm]).all()
    tail = got.coeffs(n_rows - 1, 1)
    assert (tail[n - (n_rows - 1) * n_per_row:] == 0).all()
    assert (tail[:n - (n_rows - 1) * n_per_row] == d_ref[(n_rows - 1) * n_per_row:].cpu().numpy().view(np.uint64)).all()


@pytest.mark.parametrize("fid,brakedown", ((1, False), (3, True)), ids=("ft127-ligero", "ft255-brakedown"))
def test_plain_integers_end_to_end(fid, brakedown):
    """commit, prove and verify with nothing but integers on the caller's side"""
    n = 1 << 10
    p = IC.modulus(fid)
    enc = sdig_enc(fid, 40) if brakedown else LigeroEncoding.new(fid, n)
    rnd = random.Random(77)
    coeffs = [rnd.randint(-(1 << 63), (1 << 63) - 1) for _ in range(n)]
    coeffs[:3] = [-(1 << 63), -1, (1 << 63) - 1]
    cm = LcCommit.commit_ints(np.array(coeffs, np.int64), enc)
    x = rnd.randrange(p)
    inner = enc.from_ints([pow(x, j, p) for j in range(cm.n_per_row)])
    outer = enc.from_ints([pow(x, r * cm.n_per_row, p) for r in range(cm.n_rows)])
    root = cm.get_root()
    pf = cm.prove(outer, enc, mk_transcript(Transcript, root, enc.get_n_col_opens()))
    ev = pf.verify(root, outer, inner, enc, mk_transcript(Transcript, root, enc.get_n_col_opens()))
    assert enc.to_ints(ev) == [sum(c * pow(x, i, p) for i, c in enumerate(coeffs)) % p]
    # Python ints of any size and sign
    big = [0, -1, p, -p, 3 * p + 5, -(1 << 300), 1 << 300]
    assert enc.to_ints(enc.from_ints(big)) == [v % p for v in big]


def test_async_commit_then_prove():
    """commit_ints(sync=False) followed at once by prove: the bytes of the synchronous run"""
    fid, n = 3, (1 << 12) - 5
    enc = LigeroEncoding.new_from_dims(fid, 64, 128)
    vals = values_with_edges("i64", fid, n, 9)
    outer = O.random_elems(fid, -(-n // 64), 2)
    proofs = []
    for sync in (True, False):
        st = torch.cuda.Stream(device=DEV)
        d = to_dev(IC.pack("i64", vals, enc.L))
        torch.cuda.synchronize()                      # the upload ran on another stream than `st`
        cm = LcCommit.commit_ints(d, enc, stream=st.cuda_stream, sync=sync)
        assert (cm._coeffs_ref is None) == sync
        proofs.append(cm.prove(outer, enc, Transcript(b"ints")).to_bytes())
    assert proofs[0] == proofs[1]


def test_errors_leave_the_object_uncommitted():
    fid, n = 0, 1 << 10
    enc = LigeroEncoding.new_from_dims(fid, 64, 128)
    arr = np.arange(n, dtype=np.uint32)
    d = to_dev(arr)
    outer = O.random_elems(fid, n // 64, 2)
    L = _lib.lib()
    for call in (lambda h: L.lcpci_commit_ints(h, 5, vp(arr), n, None), lambda h: L.lcpci_commit_ints(h, 0, vp(arr), 0, None),
                 lambda h: L.lcpci_commit_ints(h, 0, None, n, None),
                 lambda h: L.lcpci_commit_ints_device(h, 5, C.c_void_p(d.data_ptr()), n, None, None),
                 lambda h: L.lcpci_commit_ints_device(h, 0, C.c_void_p(d.data_ptr()), 0, None, None),
                 lambda h: L.lcpci_commit_ints_device(h, 0, None, n, None, None)):
        cm = LcCommit(enc)
        assert call(cm._h) == lcpc_amd.ERR_ARG
        with pytest.raises(LcpcError) as e:
            cm.prove(outer, enc, Transcript(b"x"))
        assert e.value.code == lcpc_amd.ERR_STATE
    out = torch.zeros((n, 1), dtype=torch.int64, device=DEV)
    assert L.lcpci_from_ints_device(enc._h, 5, C.c_void_p(d.data_ptr()), n, C.c_void_p(out.data_ptr()), None) == lcpc_amd.ERR_ARG
    assert L.lcpci_from_ints_device(enc._h, 0, C.c_void_p(d.data_ptr()), 0, C.c_void_p(out.data_ptr()), None) == lcpc_amd.ERR_ARG
    assert L.lcpci_from_ints_device(enc._h, 2, C.c_void_p(d.data_ptr() + 4), 8, C.c_void_p(out.data_ptr()), None) == lcpc_amd.ERR_ARG
    # a good commit after the refusals
    assert LcCommit.commit_ints(arr, enc).get_root() == LcCommit.commit_ints(d, enc, kind="u32").get_root()

"""lcpc_amd.check_columns (lcpcp_check_columns, include/lcpc_hip_columns.h): columns opened outside a proof, checked against a root on
the device -- the leaf digests by the batch column-hash kernels, the folds by K8b on the column-major layout open_columns returns.
The second opinion is the same fold in Python with the reference digests (tests/digest_ref.py ref_digest)."""
import random

import numpy as np
import pytest

import digest_more  # noqa: F401  (Keccak-256 and SHA-256 for ref_digest)
import digest_ref as DR
import sha3_ref
from lcpc_amd import ERR_COLUMN_NUMBER, LcCommit, LcpcError, LigeroEncoding, _lib, check_columns
from test_gpu_prove_batch import FT255_61, elems, sdig

pytestmark = pytest.mark.gpu

DIGESTS = ["blake3", "sha3_256", "keccak256", "sha256", "blake2b"]
SHAPES = {"ft255_128cols_" + d: (lambda O, d=d: FT255_61(digest=d)) for d in DIGESTS}
SHAPES["ft127_2^12"] = lambda O: (LigeroEncoding.new(1, 1 << 12), 1 << 12)
SHAPES["sdig_ft63"] = lambda O: (sdig(O, 0), 3 * 900)                          # n_cols is no power of two
_OPENED = {}


class Opened:
    """a commitment and 303 of its columns, opened: 0, n_cols - 1, one number twice, 300 random ones (more than one 256-lane block)"""

    def __init__(self, enc, n_coeffs, digest):
        self.enc, self.digest = enc, digest
        self.cm = LcCommit.commit(elems(enc, n_coeffs, 31), enc)
        self.root = self.cm.get_root()
        rng = random.Random(n_coeffs)
        self.cols = np.array([0, enc.n_cols - 1, 5] + [rng.randrange(enc.n_cols) for _ in range(300)], np.uint64)
        self.cols[7] = self.cols[2]
        self.vals, self.paths = self.cm.open_columns(self.cols)
        self.n = self.cols.size


def opened(oracle, shape):
    if shape not in _OPENED:
        enc, n = SHAPES[shape](oracle)
        digest = shape.split("cols_")[1] if "cols_" in shape else "blake3"
        _OPENED[shape] = Opened(enc, n, digest)
    return _OPENED[shape]


def host_check(O, o, root, vals, paths):
    """verify_column_path (lib.rs:955-982) in Python: the leaf digest of the canonical column bytes, folded up the path"""
    D = DR.ref_digest(o.digest, O)
    dl = o.enc.digest_len
    rep = sha3_ref.repr_bytes(O, o.enc.field, vals.reshape(-1, o.enc.L)).reshape(o.n, -1)
    out = np.zeros(o.n, bool)
    for k in range(o.n):
        h, cc = D(bytes(dl) + rep[k].tobytes()), int(o.cols[k])
        for lvl in range(paths.shape[1]):
            s = paths[k, lvl].tobytes()
            h = D(h + s) if cc % 2 == 0 else D(s + h)
            cc >>= 1
        out[k] = h == bytes(root)
    return out


@pytest.mark.parametrize("shape", sorted(SHAPES))
def test_round_trip_and_faults(oracle, shape):
    o = opened(oracle, shape)
    if shape == "sdig_ft63":
        assert o.enc.n_cols & (o.enc.n_cols - 1)
    assert o.paths.shape == (o.n, max(0, (o.enc.n_cols - 1).bit_length()), o.enc.digest_len)
    ok = check_columns(o.enc, o.root, o.cols, o.vals, o.paths)
    assert ok.dtype == bool and ok.shape == (o.n,) and ok.all()
    # one value limb flipped: that column alone (the other opening of the same number keeps its own copy)
    vals = o.vals.copy()
    vals[7, o.vals.shape[1] - 1, 0] ^= np.uint64(4)
    ok = check_columns(o.enc, o.root, o.cols, vals, o.paths)
    assert np.flatnonzero(~ok).tolist() == [7]
    # one path byte flipped, in the first and in the second 256-lane block, at the bottom and at the top of the path
    paths = o.paths.copy()
    paths[1, 0, 0] ^= 1
    paths[300, -1, -1] ^= 0x80
    ok = check_columns(o.enc, o.root, o.cols, o.vals, paths)
    assert np.flatnonzero(~ok).tolist() == [1, 300]
    # a wrong root: nothing folds to it
    wrong = bytearray(o.root)
    wrong[3] ^= 1
    assert not check_columns(o.enc, bytes(wrong), o.cols, o.vals, o.paths).any()
    # a limb >= p: no honest opening has one; that column is answered 0 and the call succeeds
    vals = o.vals.copy()
    vals[256, 0, :] = np.uint64((1 << 64) - 1)
    ok = check_columns(o.enc, o.root, o.cols, vals, o.paths)
    assert np.flatnonzero(~ok).tolist() == [256]


@pytest.mark.parametrize("shape", sorted(SHAPES))
def test_agrees_with_the_host_fold(oracle, shape):
    """honest and tampered openings mixed: the same verdicts as the reference digests in Python"""
    o = opened(oracle, shape)
    vals, paths = o.vals.copy(), o.paths.copy()
    rng = random.Random(5)
    for k in rng.sample(range(o.n), 20):
        if k % 2:
            vals[k, rng.randrange(vals.shape[1]), 0] ^= np.uint64(1 << rng.randrange(40))
        else:
            paths[k, rng.randrange(paths.shape[1]), rng.randrange(paths.shape[2])] ^= 1 << rng.randrange(8)
    want = host_check(oracle, o, o.root, vals, paths)
    got = check_columns(o.enc, o.root, o.cols, vals, paths)
    assert np.array_equal(got, want) and 15 <= int((~got).sum()) <= 20
    assert host_check(oracle, o, o.root, o.vals, o.paths).all()


def test_column_number_out_of_range(oracle):
    o = opened(oracle, "ft255_128cols_blake3")
    cols = o.cols.copy()
    cols[o.n - 1] = o.enc.n_cols
    out = np.full(o.n, 7, np.uint8)
    with pytest.raises(LcpcError) as e:
        check_columns(o.enc, o.root, cols, o.vals, o.paths, out=out)
    assert e.value.code == ERR_COLUMN_NUMBER and (out == 7).all()                 # nothing was judged
    assert check_columns(o.enc, o.root, o.cols, o.vals, o.paths, out=out) is out and (out == 1).all()
    assert check_columns(o.enc, o.root, o.cols[:0], o.vals[:0], o.paths[:0]).shape == (0,)


def test_more_columns_than_one_slice(oracle):
    """the values of one slice fit the 64 MiB arena budget: enough openings of a 61-row Ft255 column for two slices, a fault in each"""
    o = opened(oracle, "ft255_128cols_blake3")
    per_col = o.vals.shape[1] * 8 * o.enc.L + 12 + o.enc.digest_len
    per_slice = _lib.VERIFY_ARENA_BUDGET // per_col
    n = per_slice + 700
    idx = np.arange(n) % o.n
    cols, vals, paths = o.cols[idx], o.vals[idx], o.paths[idx].copy()
    paths[per_slice - 1, 2, 9] ^= 1
    paths[per_slice, 0, 0] ^= 1
    paths[n - 1, -1, 31] ^= 1
    ok = check_columns(o.enc, o.root, cols, vals, paths)
    assert np.flatnonzero(~ok).tolist() == [per_slice - 1, per_slice, n - 1]

"""K1s global addressing (lcpc_amd/csrc/ntt_l9s.hip "Global addresses", ntt_ln_dev.h ubase / lane_at / pack_get_u): every global access
of a pass is a 64-bit wave-uniform base in scalar registers plus an unsigned 32-bit byte offset per lane -- the tile load, the coeffs
copy, the twiddle packs, the limb intermediate and the stores.  A wrong base or a wrapped offset reads or writes another element, so
every case is held to the oracle bit for bit through the public path: comm, hashes and root of a commit (and the coeffs it keeps).

Cases (Ft255):
  * 2^16 and 2^18 columns, the default plan (pure first pass S = 6 / 8, coset last pass, ln::mul2), 1, 3 and 5 rows: the XCD-aware
    workgroup order with row counts that are no power of two, so row and tile bases of every kind occur;
  * 2^12 .. 2^15 columns with LCPC_NTT_FORM=coset: the same helpers at S = 2 .. 5, with the limb intermediate (the default there: the
    first pass's plane store, the last pass's tile copy) and with the packed one (LCPC_NTT_MID_MAX_MB=0);
  * 2^11 columns on the DIF form (S = 1: the radix-2 round's pack, one pack class per tile);
  * a ragged n_per_row (odd, no multiple of a tile: the first pass's last columns are partly zero) with a ragged last row (the flat
    vector ends inside it);
  * the coeffs copy (copy_dst) and its absence: commit_device in copy and in borrow mode;
  * a source pointer 3 elements into its allocation (32-byte, not 128-byte aligned).
The base beyond 4 GiB is tests/test_gpu_fullsize.py's."""
import os

import numpy as np
import pytest

from lcpc_amd import LcCommit, LigeroEncoding

pytestmark = pytest.mark.gpu
FID = 3
SWITCHES = ("LCPC_NTT_MUL", "LCPC_NTT_FORM", "LCPC_NTT_MID_MAX_MB")


def _enc(env, n_per_row, n_cols):
    saved = {k: os.environ.pop(k, None) for k in SWITCHES}
    os.environ.update(env)                               # (switches are read once, when an encoder is created)
    try:
        return LigeroEncoding.new_from_dims(FID, n_per_row, n_cols)
    finally:
        for k in SWITCHES:
            os.environ.pop(k, None)
            if saved[k] is not None:
                os.environ[k] = saved[k]


def _oracle(O, coeffs, n_per_row, n_cols):
    oc = O.Commit.commit(coeffs, O.Encoding.ligero_from_dims(FID, n_per_row, n_cols), n_threads=16)
    return oc.comm().copy(), oc.hashes().copy(), oc.get_root()      # (comm / hashes are views of the oracle commit's own memory)


def _same(c, want, what):
    comm, hashes, root = want
    assert (c.comm() == comm).all(), (what, "comm")
    assert (c.hashes() == hashes).all(), (what, "hashes")
    assert c.get_root() == root, (what, "root")


@pytest.mark.parametrize("n_rows", [1, 3, 5])
@pytest.mark.parametrize("log_n", [16, 18])
def test_default_plan(oracle, log_n, n_rows):
    n_cols = 1 << log_n
    coeffs = oracle.random_elems(FID, n_rows * (n_cols // 2), 1000 + log_n * 7 + n_rows)
    want = _oracle(oracle, coeffs, n_cols // 2, n_cols)
    _same(LcCommit.commit(coeffs, _enc({}, n_cols // 2, n_cols)), want, (log_n, n_rows))


@pytest.mark.parametrize("log_n", [12, 13, 14, 15])
def test_coset_form_small(oracle, log_n):
    n_cols, n_rows = 1 << log_n, 3
    coeffs = oracle.random_elems(FID, n_rows * (n_cols // 2), 2000 + log_n)
    want = _oracle(oracle, coeffs, n_cols // 2, n_cols)
    for env in ({"LCPC_NTT_FORM": "coset"}, {"LCPC_NTT_FORM": "coset", "LCPC_NTT_MID_MAX_MB": "0"},
                {"LCPC_NTT_FORM": "coset", "LCPC_NTT_MUL": "split", "LCPC_NTT_MID_MAX_MB": "0"}):
        _same(LcCommit.commit(coeffs, _enc(env, n_cols // 2, n_cols)), want, (log_n, env))


def test_dif_form_2k(oracle):
    n_cols, n_rows = 1 << 11, 3
    coeffs = oracle.random_elems(FID, n_rows * (n_cols // 2), 3000)
    want = _oracle(oracle, coeffs, n_cols // 2, n_cols)
    for env in ({"LCPC_NTT_FORM": "dif"}, {"LCPC_NTT_FORM": "dif", "LCPC_NTT_MID_MAX_MB": "0"}):
        _same(LcCommit.commit(coeffs, _enc(env, n_cols // 2, n_cols)), want, env)


@pytest.mark.parametrize("log_n", [13, 16])
def test_ragged_rows(oracle, log_n):
    """n_per_row odd and a little under half the columns; the vector ends 123 elements into its third row"""
    n_cols = 1 << log_n
    n_per_row = n_cols // 2 - 1000 + 7
    coeffs = oracle.random_elems(FID, 2 * n_per_row + 123, 4000 + log_n)
    want = _oracle(oracle, coeffs, n_per_row, n_cols)
    c = LcCommit.commit(coeffs, _enc({}, n_per_row, n_cols))
    assert c.n_rows == 3
    _same(c, want, (log_n, "ragged"))
    kept = c.coeffs()                                    # the padded copy the first pass wrote beside its loads
    assert (kept[:len(coeffs)] == coeffs).all() and not kept[len(coeffs):].any()


@pytest.fixture(scope="module")
def device_case(oracle):
    n_cols, n_rows = 1 << 16, 3
    coeffs = oracle.random_elems(FID, n_rows * (n_cols // 2), 5000)
    return n_cols, coeffs, _oracle(oracle, coeffs, n_cols // 2, n_cols)


@pytest.mark.parametrize("borrow", [False, True])
@pytest.mark.parametrize("offset", [0, 3])
def test_device_source_copy_and_borrow(device_case, borrow, offset):
    """copy mode: the first pass writes LcCommit.coeffs while it loads (copy_dst); borrow mode: it does not, and the commitment reads the
    caller's buffer.  offset: the source starts that many elements into its allocation"""
    import torch
    n_cols, coeffs, want = device_case
    n = coeffs.shape[0]
    buf = torch.zeros((n + offset, 4), dtype=torch.int64, device="cuda")
    buf[offset:] = torch.from_numpy(np.ascontiguousarray(coeffs).view(np.int64)).cuda()
    enc = _enc({}, n_cols // 2, n_cols)
    c = LcCommit.commit_device(buf.data_ptr() + offset * 32, n, enc, torch.cuda.current_stream().cuda_stream, borrow=borrow)
    _same(c, want, (borrow, offset))
    assert (c.coeffs() == coeffs).all()
    assert (buf[offset:].cpu().numpy().view(np.uint64) == coeffs).all()      # (the source is read, never written)

"""lcpc_commit from host memory on its row-batch branch under SHA3-256 / Keccak-256 / SHA-256 / BLAKE2b: the column hash runs behind
every batch there (commit.cpp, launch_*_leaves_range), and every byte of the commitment has to stay what lcpc_commit_device -- the
one-shot kernels, pinned to hashlib by the digest suites -- makes of the same coefficients: the whole `hashes` array, the root, the
proof.  Inputs are the smallest that take the branch (a Ligero encoder, 64 MiB of coefficients, >= 16 rows), with dimensions chosen so
that a batch is 5 rows (no multiple of a digest's 17-, 16- or 8-row group: batches end inside blocks), the last batch is shorter than
the others and the last row is ragged."""
import os
import sys
import threading

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import common as CM  # noqa: E402
from lcpc_amd import LcCommit, LigeroEncoding, Transcript  # noqa: E402

pytestmark = pytest.mark.gpu
DIGESTS = ("sha3_256", "keccak256", "sha256", "blake2b")
# fid -> (coefficients in 64 MiB, n_per_row, n_cols): 67 rows = 13 batches of 5 and one of 2
SHAPES = {3: (1 << 21, 31301, 1 << 16), 0: (1 << 23, 125204, 1 << 18)}


def _lengths(fid):
    n0, npr, _ = SHAPES[fid]
    return n0, n0 + 5 * npr + 123, n0 + 100         # 67 rows; then a refill with 73 (larger), then one with 68 (smaller), all ragged


@pytest.fixture(scope="module")
def sources():
    """fid -> (pageable (n, L) uint64, the same in pinned memory, the same on the device): drawn once, never written to"""
    out = {}
    for fid in SHAPES:
        L = CM.FIELD_L[fid]
        host = np.random.default_rng([9, fid]).integers(0, 1 << 62, (max(_lengths(fid)), L), dtype=np.uint64)
        pinned = torch.from_numpy(host.view(np.int64)).pin_memory()
        out[fid] = (host, pinned.numpy().view(np.uint64), pinned.cuda(), pinned)
    yield out
    out.clear()
    torch.cuda.empty_cache()


def _same(host_c, dev_c, enc, prove):
    assert (host_c.n_rows, host_c.n_cols, host_c.n_per_row) == (dev_c.n_rows, dev_c.n_cols, dev_c.n_per_row)
    assert host_c.get_root() == dev_c.get_root()
    assert np.array_equal(host_c.hashes(), dev_c.hashes())
    if prove:
        outer = np.random.default_rng(host_c.n_rows).integers(0, 1 << 62, (host_c.n_rows, enc.L), dtype=np.uint64)
        a = host_c.prove(outer, enc, Transcript(b"host batches")).to_bytes()
        b = dev_c.prove(outer, enc, Transcript(b"host batches")).to_bytes()
        assert a == b


@pytest.mark.parametrize("fid", sorted(SHAPES))
@pytest.mark.parametrize("digest", DIGESTS)
def test_host_commit_equals_device_commit(digest, fid, sources):
    """pageable and pinned sources at exactly 64 MiB, then the same object refilled with a larger and with a smaller input (a chaining
    state left over from the fill before would show), each against lcpc_commit_device of the same coefficients"""
    n0, npr, n_cols = SHAPES[fid]
    host, pinned, dev, _ = sources[fid]
    enc = LigeroEncoding.new_from_dims(fid, npr, n_cols, digest=digest)
    assert n0 * 8 * enc.L == 64 << 20
    ch, cd = LcCommit(enc), LcCommit(enc)
    for i, (n, src) in enumerate(((n0, host), (n0, pinned), (_lengths(fid)[1], pinned), (_lengths(fid)[2], host))):
        LcCommit.commit(src[:n], enc, into=ch)
        LcCommit.commit_device(dev.data_ptr(), n, enc, into=cd)
        rows = -(-n // npr)
        assert ch.n_rows == rows >= 16 and rows % (-(-rows // 16)) and n % npr and -(-rows // 16) == 5
        _same(ch, cd, enc, prove=i in (0, 3))


@pytest.mark.parametrize("digest", DIGESTS)
def test_concurrent_refills_under_two_digests(digest, sources):
    """one object is refilled from host memory while a second thread refills another object under another digest's encoder: each has
    its own chaining state, streams and events, and both end as the device commit of their last input"""
    fid = 3
    n0, npr, n_cols = SHAPES[fid]
    host, pinned, dev, _ = sources[fid]
    other = DIGESTS[(DIGESTS.index(digest) + 1) % len(DIGESTS)]
    enc_a = LigeroEncoding.new_from_dims(fid, npr, n_cols, digest=digest)
    enc_b = LigeroEncoding.new_from_dims(fid, npr, n_cols, digest=other)
    a, b = LcCommit.commit(host[:n0], enc_a), LcCommit.commit(pinned[:n0], enc_b)
    la, lb = _lengths(fid)[1:], _lengths(fid)[:0:-1]
    err = []

    def refill(obj, enc, lens, src):
        try:
            for n in lens:
                LcCommit.commit(src[:n], enc, into=obj)
        except Exception as e:          # reported by the main thread
            err.append(e)
    t = threading.Thread(target=refill, args=(b, enc_b, lb, host))
    t.start()
    refill(a, enc_a, la, pinned)
    t.join()
    assert not err, err
    _same(a, LcCommit.commit_device(dev.data_ptr(), la[-1], enc_a), enc_a, prove=False)
    _same(b, LcCommit.commit_device(dev.data_ptr(), lb[-1], enc_b), enc_b, prove=False)

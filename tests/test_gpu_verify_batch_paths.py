"""lcpcv_verify_batch folds the Merkle paths on the device (K8b; include/lcpc_hip_verify.h "path folds"): every verdict is still the single
verify's of that member alone.  Shapes and helpers are those of tests/test_gpu_prove_batch.py and tests/test_gpu_verify_batch.py; a
shape's honest batch is made once and shared by the tests that tamper with copies of its bytes."""
import os
import re
import struct
import subprocess
import sys

import numpy as np
import pytest

from lcpc_amd import VERR_COLUMN_DEGREE, VERR_COLUMN_EVAL, VERR_COLUMN_PATH, _lib, verify_batch
from test_gpu_prove_batch import FT255_61, SHAPES, member_transcript, sdig
from test_gpu_verify_batch import Batch, check_batch, single

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DIGESTS = ["blake3", "sha3_256", "keccak256", "sha256", "blake2b"]
PATH_SHAPES = {"ft255_61rows_" + d: (lambda d=d: FT255_61(digest=d)) for d in DIGESTS}
PATH_SHAPES["ft63_8rows"] = SHAPES["ft63_8rows"]
_BATCHES = {}


def batch(shape):
    if shape not in _BATCHES:
        enc, n = PATH_SHAPES[shape]()
        _BATCHES[shape] = Batch(enc, n)
    return _BATCHES[shape]


def with_member_1(b, p):
    return [b.proofs[0], bytes(p), b.proofs[2]]


@pytest.mark.parametrize("where", ["level0", "top", "leaf"])
@pytest.mark.parametrize("shape", sorted(PATH_SHAPES))
def test_tampered_path_fails_its_member_alone(shape, where):
    """a flipped byte in a path's first entry, in its last entry, and in a column value (another leaf digest): the member gets what the
    single verify gives it, the others pass"""
    b = batch(shape)
    assert b.path_len >= 2
    p = bytearray(b.proofs[1])
    if where == "level0":
        p[b.path_off(4, 0) + b.dl - 1] ^= 0x80
    elif where == "top":
        p[b.path_off(b.n_open - 1, b.path_len - 1)] ^= 0x01
    else:
        p[b.value_off(6, b.n_rows - 1) + 1] ^= 0x02
    _, status, _ = check_batch(b, proofs=with_member_1(b, p))
    assert status[0] == 0 and status[2] == 0
    if where == "leaf":
        assert status[1] in (VERR_COLUMN_DEGREE, VERR_COLUMN_EVAL, VERR_COLUMN_PATH)
    else:
        assert status[1] == VERR_COLUMN_PATH


@pytest.mark.parametrize("shape", ["ft255_61rows_blake3", "ft255_61rows_blake2b", "ft63_8rows"])
def test_precedence_and_first_column(shape):
    """a column that fails the value check and carries a bad path keeps the value code; a bad path in an earlier column decides"""
    b = batch(shape)
    p = bytearray(b.proofs[1])
    p[b.value_off(7, 1)] ^= 1
    p[b.path_off(7, 1) + 3] ^= 1
    _, status, _ = check_batch(b, proofs=with_member_1(b, p))
    assert status[1] in (VERR_COLUMN_DEGREE, VERR_COLUMN_EVAL) and status[0] == status[2] == 0
    p[b.path_off(2, 0)] ^= 1
    check_batch(b, proofs=with_member_1(b, p), want_codes=[0, VERR_COLUMN_PATH, 0])


@pytest.mark.parametrize("shape", ["ft255_61rows_sha256", "ft255_61rows_blake2b", "ft63_8rows"])
def test_wrong_root(shape):
    b = batch(shape)
    check_batch(b, roots=[b.roots[0], b.roots[2], b.roots[2]], want_codes=[0, VERR_COLUMN_PATH, 0])


def reencode_path(b, proof, k, delta):
    """column k's path with one entry fewer (delta = -1) or one more, a copy of its last (delta = +1); the length field follows, so the
    bytes still parse"""
    start = b.head + k * b.col_bytes
    plen_off = start + 8 + b.n_rows * b.F
    ents = plen_off + 8
    end = start + b.col_bytes
    we = 8 + b.dl
    assert struct.unpack_from("<Q", proof, plen_off)[0] == b.path_len and end - ents == b.path_len * we
    body = proof[ents:end - we] if delta < 0 else proof[ents:end] + proof[end - we:end]
    return proof[:plen_off] + struct.pack("<Q", b.path_len + delta) + body + proof[end:]


@pytest.mark.parametrize("delta", [-1, 1])
@pytest.mark.parametrize("shape", ["ft255_61rows_blake3", "ft255_61rows_sha3_256", "ft63_8rows"])
def test_irregular_path_lengths(shape, delta):
    """the parser takes any entry count; such a column is folded on the host, as many levels as it has entries: the single verify's code"""
    b = batch(shape)
    for k in (0, 3, b.n_open - 1):
        p = reencode_path(b, b.proofs[1], k, delta)
        assert len(p) == len(b.proofs[1]) + delta * (8 + b.dl)
        _, status, _ = check_batch(b, proofs=with_member_1(b, p))
        assert status[0] == 0 and status[2] == 0 and status[1] == VERR_COLUMN_PATH
    # a short path beside a bad value in an earlier column: the earlier column decides
    p = bytearray(reencode_path(b, b.proofs[1], 5, delta))
    p[b.value_off(1, 0)] ^= 1
    _, status, _ = check_batch(b, proofs=with_member_1(b, p))
    assert status[1] in (VERR_COLUMN_DEGREE, VERR_COLUMN_EVAL)


def test_path_budget_crossing(oracle):
    """Brakedown over Ft63, 900 coefficients, 1 row, code 3: thousands of openings of an 11-level path, about 2.3 MB of siblings per
    member, so that 32 members cross the 64 MiB path budget inside ONE group: the first floor(budget / P) fold on the device, the rest
    of the group on the host"""
    enc = sdig(oracle, 0)
    n_rows, n_batch = 1, 32
    b = Batch(enc, n_rows * 900, n_batch=n_batch, seed=83)
    assert b.n_rows == n_rows
    F, D, nt, n_open = 8 * enc.L, enc.digest_len, enc.get_n_degree_tests() + 1, enc.get_n_col_opens()
    path_len = max(0, (enc.n_cols - 1).bit_length())
    P = n_open * path_len * D
    even = lambda x: x + (x & 1) if enc.L % 2 else x
    arena = 2 * nt * enc.n_per_row * F + nt * n_rows * F + n_open * (8 + 4 + D) + even(n_open * n_rows) * F      # the header's A
    on_device = max(1, _lib.VERIFY_PATH_BUDGET // P)
    print("n_open %d path_len %d P %d A %d: %d of %d members fold on the device" % (n_open, path_len, P, arena, on_device, n_batch))
    assert n_batch * P > _lib.VERIFY_PATH_BUDGET and 1 < on_device < n_batch - 1          # the batch crosses the path budget
    assert n_batch * arena <= _lib.VERIFY_ARENA_BUDGET                                       # in one group
    proofs = list(b.proofs)
    tampered = (on_device - 2, on_device + 1)                                                # one on each side of the boundary
    for i, k in zip(tampered, (n_open - 1, 17)):
        p = bytearray(proofs[i])
        p[b.path_off(k, path_len // 2) + 7] ^= 0x10
        proofs[i] = bytes(p)
    trs = [member_transcript(i) for i in range(n_batch)]
    evals, status, stats = verify_batch(enc, b.roots, b.outer, b.inner, proofs, trs, return_stats=True)
    assert stats.groups == 1 and stats.host_syncs == 2
    for i in sorted({0, on_device - 1, on_device, n_batch - 1} | set(tampered)):
        code, ev = single(enc, b.roots[i], b.outer, b.inner, proofs[i], member_transcript(i))
        assert status[i] == code and code == (VERR_COLUMN_PATH if i in tampered else 0), i
        if code == 0:
            assert np.array_equal(evals[i], ev), i
    assert not np.delete(status, tampered).any()


CHILD = """
import sys
import numpy as np
from test_gpu_verify_batch import Batch, ALL_SHAPES
from test_gpu_prove_batch import member_transcript
from lcpc_amd import verify_batch
enc, n = ALL_SHAPES["ft255_61rows"]()
b = Batch(enc, n)
evals, status = verify_batch(enc, b.roots, b.outer, b.inner, b.proofs, [member_transcript(i) for i in range(3)])
assert not status.any()
print("n_open", b.n_open)
"""


def test_debug_line_counts_the_folds():
    """LCPC_DEBUG_TIMING is read when the encoder is created: a fresh process.  An honest batch folds every column on the device"""
    env = dict(os.environ, LCPC_DEBUG_TIMING="1")
    env["PYTHONPATH"] = os.pathsep.join([ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "oracle"), env.get("PYTHONPATH", "")])
    r = subprocess.run([sys.executable, "-c", CHILD], env=env, cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    n_open = int(re.search(r"n_open (\d+)", r.stdout).group(1))
    lines = re.findall(r"\[lcpcv_verify_batch\].*?(\d+) columns folded on the device, (\d+) on the host", r.stderr)
    assert lines, r.stderr[-2000:]
    assert [(int(a), int(c)) for a, c in lines] == [(3 * n_open, 0)] * len(lines)


def test_path_budget_is_the_headers():
    assert _lib.VERIFY_PATH_BUDGET == 64 << 20

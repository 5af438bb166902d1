"""lcpcv_verify_batch (include/lcpc_hip_verify.h): every proof of a batch checked in one lockstep pipeline.

The reference for every verdict is the existing single path: lcpc_verify of member i alone on a clone of its transcript (itself pinned
to the oracle by tests/test_gpu_parity.py and the digest suites).  status[i] must be its return code, evals[i] its evaluation, and the
transcript must end in the same state.  Proofs are made with commit_batch + prove_batch at the shapes of
tests/test_gpu_prove_batch.py; a shape's honest batch is made once and shared by the tests that tamper with copies of its bytes."""
import ctypes as C
import threading

import numpy as np
import pytest

from lcpc_amd import (ERR_ARG, ERR_STATE, VERR_COLUMN_DEGREE, VERR_COLUMN_EVAL, VERR_COLUMN_PATH, VERR_MALFORMED, VERR_OUTER_TENSOR,
                      LcEvalProof, LcpcError, _lib, prove_batch, verify_batch)
from test_gpu_prove_batch import FT255_61, SHAPES, batch_of, elems, ligero, member_transcript, sdig

pytestmark = pytest.mark.gpu

HOST_SYNCS_PER_GROUP = 2           # the header: one event wait behind the row encode, one stream synchronisation at the end

ALL_SHAPES = dict(SHAPES)
ALL_SHAPES["ft255_61rows_sha3_256"] = lambda: FT255_61(digest="sha3_256")
ALL_SHAPES["ft255_61rows_keccak256"] = lambda: FT255_61(digest="keccak256")
ALL_SHAPES["ft63_8rows_sha256"] = lambda: (ligero(0, 32, 64, digest="sha256"), 8 * 32)       # a chained digest over a non-Ft255 field


class Batch:
    """an honest batch: encoder, roots, the shared tensors, proof bytes, and what the single verify says about each member"""

    def __init__(self, enc, n_coeffs, n_batch=3, seed=71):
        self.enc, self.n = enc, n_batch
        self.cms = batch_of(enc, n_batch, n_coeffs, seed)
        self.n_rows = self.cms[0].n_rows
        self.outer = elems(enc, self.n_rows, seed + 1)
        self.inner = elems(enc, enc.n_per_row, seed + 2)
        self.roots = [cm.get_root() for cm in self.cms]
        pfs = prove_batch(self.cms, self.outer, [member_transcript(i) for i in range(n_batch)])
        self.proofs = [p.to_bytes() for p in pfs]
        self.cols_opened = [p.cols_opened for p in pfs]
        # the wire layout (lib.rs:550-609): where the columns start, the bytes of one, and the bytes of one polynomial
        F, dl = 8 * enc.L, enc.digest_len
        self.F, self.dl = F, dl
        self.pb = enc.n_per_row * F
        self.n_deg, self.n_open = enc.get_n_degree_tests(), enc.get_n_col_opens()
        self.path_len = max(0, (enc.n_cols - 1).bit_length())
        self.head = 8 + (8 + self.pb) + 8 + self.n_deg * (8 + self.pb) + 8
        self.col_bytes = 8 + self.n_rows * F + 8 + self.path_len * (8 + dl)
        assert len(self.proofs[0]) == self.head + self.n_open * self.col_bytes

    def value_off(self, k, r):
        return self.head + k * self.col_bytes + 8 + r * self.F

    def path_off(self, k, lvl):
        return self.head + k * self.col_bytes + 8 + self.n_rows * self.F + 8 + lvl * (8 + self.dl) + 8


_BATCHES = {}


def batch(shape):
    if shape not in _BATCHES:
        enc, n = ALL_SHAPES[shape]()
        _BATCHES[shape] = Batch(enc, n)
    return _BATCHES[shape]


def single(enc, root, outer, inner, proof, tr):
    """the single path: (status, evaluation or None)"""
    try:
        return 0, LcEvalProof(bytes(proof), enc.L).verify(root, outer, inner, enc, tr)
    except LcpcError as e:
        return e.code, None


def check_verify(enc, roots, outers, inners, proofs, shared=True, want_codes=None):
    """verify_batch against the single verifies of the same members; outers / inners: per member (shared: all the same, passed once)"""
    n = len(proofs)
    trs = [member_transcript(i) for i in range(n)]
    ref = [t.clone() for t in trs]
    want = [single(enc, roots[i], outers[i], inners[i], proofs[i], ref[i]) for i in range(n)]
    o = outers[0] if shared else np.stack(outers)
    inn = inners[0] if shared else np.stack(inners)
    evals, status, stats = verify_batch(enc, roots, o, inn, proofs, trs, return_stats=True)
    assert status.tolist() == [w[0] for w in want], (status.tolist(), [w[0] for w in want])
    if want_codes is not None:
        assert status.tolist() == list(want_codes)
    for i in range(n):
        if want[i][0] == 0:
            assert np.array_equal(evals[i], want[i][1]), i
            assert trs[i].challenge_bytes(b"after", 32) == ref[i].challenge_bytes(b"after", 32), i
        else:
            assert not evals[i].any(), i                 # left alone
    return evals, status, stats


def check_batch(b, proofs=None, roots=None, want_codes=None):
    proofs = b.proofs if proofs is None else proofs
    return check_verify(b.enc, b.roots if roots is None else roots, [b.outer] * len(proofs), [b.inner] * len(proofs), proofs,
                        want_codes=want_codes)


@pytest.mark.parametrize("shape", sorted(ALL_SHAPES))
def test_honest_batch(shape):
    b = batch(shape)
    if shape == "ft63_8rows":
        assert b.n_deg > 1                                # several degree-test rows per member
    _, status, stats = check_batch(b, want_codes=[0, 0, 0])
    assert stats.groups == 1 and stats.host_syncs == HOST_SYNCS_PER_GROUP
    assert stats.encode_launches > 0 and stats.hash_launches > 0 and stats.check_launches > 0


@pytest.mark.parametrize("fid", [0, 3])
@pytest.mark.parametrize("n_rows", [8, 24])
def test_honest_batch_brakedown(oracle, fid, n_rows):
    """thousands of opened columns.  The row encode of the batch: Ft255, 3 members -- 3 (n_deg + 1) < 24 stacked polynomials, the
    row-major kernels; Ft63, 8 members -- 24 or more, the position-major kernels"""
    enc = sdig(oracle, fid)
    n_batch = 8 if fid == 0 else 3
    b = Batch(enc, n_rows * 900, n_batch=n_batch, seed=81)
    assert b.n_rows == n_rows and (n_batch * (b.n_deg + 1) >= 24) == (fid == 0)
    check_batch(b, want_codes=[0] * n_batch)
    # one flipped column value in the middle member: that member alone fails
    bad = bytearray(b.proofs[1])
    bad[b.value_off(b.n_open - 1, n_rows - 1)] ^= 1
    _, status, _ = check_batch(b, proofs=[b.proofs[0], bytes(bad)] + b.proofs[2:])
    assert status[1] in (VERR_COLUMN_DEGREE, VERR_COLUMN_EVAL) and not status[0] and not status[2]


def _tampered(b, kind):
    """(proofs, roots, the code the tampered member 1 must get, or None where only the single path decides)"""
    proofs, roots = list(b.proofs), list(b.roots)
    p = bytearray(proofs[1])
    code = None
    if kind == "column_value":                           # a flipped limb bit in an opened column (still < p)
        p[b.value_off(3, 2)] ^= 1
    elif kind == "column_limb_ge_p":
        off = b.value_off(4, 1)
        p[off:off + b.F] = b"\xff" * b.F
        code = VERR_MALFORMED
    elif kind == "path_digest":
        p[b.path_off(2, b.path_len - 1) + 5] ^= 0x40
        code = VERR_COLUMN_PATH
    elif kind == "wrong_root":
        roots[1] = roots[0]
        code = VERR_COLUMN_PATH
    elif kind == "p_eval":
        p[16 + 3 * b.F] ^= 1                              # (absorbed before the columns are drawn: other columns are checked than were opened)
    elif kind == "truncated":
        p = p[:len(p) - 9]
        code = VERR_MALFORMED
    elif kind == "other_n_rows":
        other = Batch(b.enc, (b.n_rows + 1) * b.enc.n_per_row, n_batch=1, seed=91)
        p = bytearray(other.proofs[0])
        code = VERR_OUTER_TENSOR
    elif kind == "other_digest":                         # the same polynomial committed and opened under another 32-byte digest
        enc2 = ligero(b.enc.field, b.enc.n_per_row, b.enc.n_cols, digest="sha3_256")
        cm = b.cms[1]
        from lcpc_amd import LcCommit
        cm2 = LcCommit.commit(cm.coeffs(), enc2)
        p = bytearray(cm2.prove(b.outer, enc2, member_transcript(1)).to_bytes())
        code = VERR_COLUMN_PATH
    else:
        raise AssertionError(kind)
    proofs[1] = bytes(p)
    return proofs, roots, code


KINDS = ["column_value", "column_limb_ge_p", "path_digest", "wrong_root", "p_eval", "truncated", "other_n_rows", "other_digest"]


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("shape", ["ft255_61rows", "ft63_8rows"])
def test_mixed_batch(shape, kind):
    """one tampered member between honest ones: every status is the single verify's, the honest members' evaluations are intact"""
    b = batch(shape)
    proofs, roots, code = _tampered(b, kind)
    _, status, _ = check_batch(b, proofs=proofs, roots=roots)
    assert status[0] == 0 and status[2] == 0 and status[1] != 0
    if code is not None:
        assert status[1] == code
    else:
        assert status[1] in (VERR_COLUMN_DEGREE, VERR_COLUMN_EVAL, VERR_COLUMN_PATH)


def test_proof_at_an_odd_address():
    b = batch("ft255_61rows")
    buf = np.zeros(len(b.proofs[1]) + 1, np.uint8)
    buf[1:] = np.frombuffer(b.proofs[1], np.uint8)
    odd = buf[1:]
    assert odd.ctypes.data % 2 == 1
    check_batch(b, proofs=[b.proofs[0], odd, b.proofs[2]], want_codes=[0, 0, 0])


def test_precedence():
    """the first failing column decides, and within a column degree > eval > path"""
    b = batch("ft255_61rows")
    p = bytearray(b.proofs[1])
    p[b.path_off(5, 0)] ^= 1                              # a bad path in column 5
    p[b.value_off(9, 0)] ^= 1                             # a bad value in column 9
    check_batch(b, proofs=[b.proofs[0], bytes(p), b.proofs[2]], want_codes=[0, VERR_COLUMN_PATH, 0])
    q = bytearray(b.proofs[2])
    q[b.value_off(7, 1)] ^= 1                             # a bad value and a bad path in the same column
    q[b.path_off(7, 1)] ^= 1
    _, status, _ = check_batch(b, proofs=[b.proofs[0], b.proofs[1], bytes(q)])
    assert status[2] in (VERR_COLUMN_DEGREE, VERR_COLUMN_EVAL) and status[0] == status[1] == 0


def _raw(enc, roots, outer, n_outer, o_stride, inner, n_inner, i_stride, proofs, trs):
    """the C entry point itself, with tensor strides a caller chooses: (rc, evals, status)"""
    n = len(proofs)
    rootb = np.frombuffer(b"".join(roots), np.uint8).copy()
    bufs = [np.frombuffer(p, np.uint8) for p in proofs]
    pp = (C.c_void_p * n)(*[x.ctypes.data for x in bufs])
    plen = (C.c_uint64 * n)(*[x.size for x in bufs])
    th = (C.c_void_p * n)(*[t._h for t in trs])
    evals, status = np.zeros((n, enc.L), np.uint64), np.full(n, 99, np.int32)
    vp = lambda a: a.ctypes.data_as(C.c_void_p)
    rc = _lib.lib().lcpcv_verify_batch(enc._h, n, vp(rootb), vp(outer), n_outer, o_stride, vp(inner), n_inner, i_stride, pp, plen, th,
                                       vp(evals), vp(status), None)
    return rc, evals, status


def test_tensors_shared_per_member_and_strided():
    b = batch("ft255_61rows")
    shared = check_batch(b)[0]
    per_member = check_verify(b.enc, b.roots, [b.outer] * 3, [b.inner] * 3, b.proofs, shared=False)[0]
    assert np.array_equal(shared, per_member)
    # per-member tensors at a stride larger than their length, all-ones limbs (no reduced element) between them
    L, nr, npr = b.enc.L, b.n_rows, b.enc.n_per_row
    outer = np.full((3, nr + 5, L), (1 << 64) - 1, np.uint64)
    inner = np.full((3, npr + 3, L), (1 << 64) - 1, np.uint64)
    outer[:, :nr], inner[:, :npr] = b.outer, b.inner
    rc, evals, status = _raw(b.enc, b.roots, outer, nr, nr + 5, inner, npr, npr + 3, b.proofs, [member_transcript(i) for i in range(3)])
    assert rc == 0 and status.tolist() == [0, 0, 0] and np.array_equal(evals, shared)
    # a member whose OWN outer tensor is another one fails alone (its eval row no longer matches)
    outer[1, :nr] = elems(b.enc, nr, 93)
    rc, evals, status = _raw(b.enc, b.roots, outer, nr, nr + 5, inner, npr, npr + 3, b.proofs, [member_transcript(i) for i in range(3)])
    assert rc == 0 and status.tolist() == [0, VERR_COLUMN_EVAL, 0] and np.array_equal(evals[0], shared[0]) and not evals[1].any()
    # tensor lengths that fit no member's proof: every member gets the single path's code, the call itself succeeds
    rc, _, status = _raw(b.enc, b.roots, outer, nr - 1, nr + 5, inner, npr, npr + 3, b.proofs, [member_transcript(i) for i in range(3)])
    assert rc == 0 and status.tolist() == [VERR_OUTER_TENSOR] * 3
    rc, _, status = _raw(b.enc, b.roots, outer, 0, 0, inner, npr, npr + 3, b.proofs, [member_transcript(i) for i in range(3)])
    assert rc == 0 and status.tolist() == [VERR_OUTER_TENSOR] * 3          # an outer tensor of no rows: judged by the single verify


@pytest.mark.parametrize("shape", ["ft255_61rows", "ft63_8rows"])
def test_launches_do_not_grow_with_the_batch(shape):
    enc, n = SHAPES[shape]()
    stats = []
    for n_batch in (2, 16):
        b = Batch(enc, n, n_batch=n_batch, seed=58)
        stats.append(check_batch(b, want_codes=[0] * n_batch)[2])
    a, c = stats
    assert a.groups == c.groups == 1
    assert (a.encode_launches, a.hash_launches, a.check_launches, a.host_syncs) == (c.encode_launches, c.hash_launches, c.check_launches, c.host_syncs)
    assert a.encode_launches > 0 and a.hash_launches > 0 and a.check_launches > 0
    assert a.host_syncs == HOST_SYNCS_PER_GROUP


def test_groups():
    """Ft255 8192 x 16384, 8 rows: about 1.1 MiB of pinned arena per member, so 96 members cross the 64 MiB budget"""
    enc = ligero(3, 8192, 16384)
    n_rows, n_batch = 8, 96
    b = Batch(enc, n_rows * 8192, n_batch=n_batch, seed=60)
    F, D, nt, n_open = 8 * enc.L, enc.digest_len, enc.get_n_degree_tests() + 1, enc.get_n_col_opens()
    even = lambda x: x + (x & 1) if enc.L % 2 else x
    arena = 2 * nt * enc.n_per_row * F + nt * n_rows * F + n_open * (8 + 4 + D) + even(n_open * n_rows) * F      # the header's A
    per_group = max(1, _lib.VERIFY_ARENA_BUDGET // arena)
    want_groups = -(-n_batch // per_group)
    assert want_groups == 2
    trs = [member_transcript(i) for i in range(n_batch)]
    evals, status, stats = verify_batch(enc, b.roots, b.outer, b.inner, b.proofs, trs, return_stats=True)
    assert stats.groups == want_groups and stats.host_syncs == HOST_SYNCS_PER_GROUP * want_groups
    assert not status.any()
    for i in (0, per_group - 1, per_group, n_batch - 1):          # both sides of the group boundary against the single path
        code, ev = single(enc, b.roots[i], b.outer, b.inner, b.proofs[i], member_transcript(i))
        assert code == 0 and np.array_equal(evals[i], ev), i


def test_concurrent_with_single_verifies():
    """two threads each run batch verifies under one encoder while a third loops the single verify: all verdicts as alone"""
    b = batch("ft255_61rows")
    bad, _, _ = _tampered(b, "column_value")
    want = [single(b.enc, b.roots[i], b.outer, b.inner, b.proofs[i], member_transcript(i)) for i in range(3)]
    bad_codes = [single(b.enc, b.roots[i], b.outer, b.inner, bad[i], member_transcript(i))[0] for i in range(3)]
    assert bad_codes[0] == bad_codes[2] == 0 and bad_codes[1] in (VERR_COLUMN_DEGREE, VERR_COLUMN_EVAL)
    errs, start = [], threading.Barrier(3)

    def run_batch(proofs, codes):
        for _ in range(6):
            evals, status = verify_batch(b.enc, b.roots, b.outer, b.inner, proofs, [member_transcript(i) for i in range(3)])
            assert status.tolist() == codes
            for i in range(3):
                assert codes[i] or np.array_equal(evals[i], want[i][1])

    def run_single():
        for k in range(12):
            i = k % 3
            assert single(b.enc, b.roots[i], b.outer, b.inner, b.proofs[i], member_transcript(i))[0] == 0

    def run(fn, *a):
        try:
            start.wait()
            fn(*a)
        except BaseException as ex:      # pragma: no cover
            errs.append(repr(ex))

    th = [threading.Thread(target=run, args=(run_batch, b.proofs, [0, 0, 0])),
          threading.Thread(target=run, args=(run_batch, bad, bad_codes)),
          threading.Thread(target=run, args=(run_single,))]
    for x in th:
        x.start()
    for x in th:
        x.join(120)
    assert not any(x.is_alive() for x in th), "a thread did not finish"
    assert not errs, errs


def test_call_errors():
    b = batch("ft255_61rows")
    trs = [member_transcript(i) for i in range(3)]
    with pytest.raises(LcpcError) as e:
        verify_batch(b.enc, b.roots, b.outer, b.inner, b.proofs, [trs[0], trs[1], trs[1]])       # a transcript listed twice
    assert e.value.code == ERR_ARG
    sh = ligero(3, 64, 128, shard=(0, 2))                                                          # a sharded encoder
    rc, _, status = _raw(sh, b.roots, b.outer, b.n_rows, 0, b.inner, b.enc.n_per_row, 0, b.proofs, trs)
    assert rc == ERR_STATE and status.tolist() == [ERR_STATE] * 3
    with pytest.raises(LcpcError) as e:
        verify_batch(sh, b.roots, b.outer, b.inner, b.proofs, trs)
    assert e.value.code == ERR_STATE
    check_batch(b, want_codes=[0, 0, 0])                                                           # and the encoder still verifies

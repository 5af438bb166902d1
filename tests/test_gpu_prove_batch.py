"""lcpcx_prove_batch (include/lcpc_hip_batch.h): every member of a batch opened in one lockstep pipeline.

The reference is the existing single path: member i proved alone with lcpc_prove on a clone of its transcript (itself pinned to the
oracle by tests/test_gpu_parity.py and friends).  Every batch proof must equal it byte for byte, with the same opened columns and the
same transcript state afterwards, and must verify.  Inputs come from random_coeffs_device (Field::random: the top of the field
occurs).  Shapes are the smallest at which each path of the batch kernels (kernels.hip K5b / K6b) exists; the row splits of the
collapse are those of the single collapse (doubled while a split keeps >= 16 rows)."""
import ctypes as C
import random
import threading

import numpy as np
import pytest
import torch

from lcpc_amd import (ERR_ARG, ERR_OUTER_TENSOR, ERR_STATE, LcCommit, LcpcError, LigeroEncoding, SdigEncoding, Transcript, _lib,
                      commit_batch, prove_batch)

pytestmark = pytest.mark.gpu


def polys(enc, n_batch, n_coeffs, seed, stride=None):
    """[n_batch, stride * L] int64 on the device: polynomial i in the first n_coeffs elements of row i, poison behind it"""
    stride = n_coeffs if stride is None else stride
    t = enc.random_coeffs_device(n_batch * stride, seed=seed).reshape(n_batch, stride * enc.L)
    if stride > n_coeffs:
        t[:, n_coeffs * enc.L:] = -1          # all-ones limbs: not a reduced element; must never be read
    torch.cuda.synchronize()
    return t


def ligero(fid, n_per_row, n_cols, **kw):
    return LigeroEncoding.new_from_dims(fid, n_per_row, n_cols, **kw)


_SDIG = {}


def sdig(O, fid, n_per_row=900, seed=5):
    """Brakedown at 900 coefficients per row, as tests/test_gpu_commit_batch_brakedown.py: n_cols from the oracle's get_dims"""
    if fid not in _SDIG:
        _, _, n_cols = O.Encoding.sdig_from_dims(fid, n_per_row, 0, seed).get_dims(n_per_row)
        _SDIG[fid] = SdigEncoding.new_from_dims(fid, n_per_row, n_cols, seed)
    return _SDIG[fid]


def elems(enc, n, seed):
    """n reduced random elements on the host, (n, L) uint64"""
    t = enc.random_coeffs_device(n, seed=seed)
    torch.cuda.synchronize()
    return t.cpu().numpy().view(np.uint64).reshape(n, enc.L).copy()


def member_transcript(i):
    """one transcript per member, each with a message of its own: the members' challenges differ"""
    tr = Transcript(b"prove batch test")
    tr.append_message(b"member", int(i).to_bytes(8, "big"))
    return tr


def check_prove(enc, cms, outers, shared=None, verify=True):
    """prove_batch over cms against the single proves; outers[i] = member i's tensor; shared: pass this ONE tensor instead"""
    n = len(cms)
    trs = [member_transcript(i) for i in range(n)]
    ref = [t.clone() for t in trs]
    want = [cms[i].prove(outers[i], enc, ref[i]) for i in range(n)]
    got, stats = prove_batch(cms, shared if shared is not None else np.stack(outers), trs, return_stats=True)
    assert len(got) == n
    for i in range(n):
        assert got[i].to_bytes() == want[i].to_bytes(), i
        assert np.array_equal(got[i].cols_opened, want[i].cols_opened), i
        assert trs[i].challenge_bytes(b"after", 32) == ref[i].challenge_bytes(b"after", 32), i
    if verify:
        inner = elems(enc, cms[0].n_per_row, 77)
        for i in range(n):
            got[i].verify(cms[i].get_root(), outers[i], inner, enc, member_transcript(i))
    return got, stats


def batch_of(enc, n_batch, n_coeffs, seed):
    t = polys(enc, n_batch, n_coeffs, seed)
    return commit_batch(enc, t, n_coeffs=n_coeffs)


def FT255_61(**kw):
    return ligero(3, 64, 128, **kw), 61 * 64


SHAPES = {
    # one split, a partly filled 256-lane workgroup, path_len 6; several degree tests
    "ft63_8rows": lambda: (ligero(0, 32, 64), 8 * 32),
    # collapse29: one row past a 60-row lazy block, two uneven row splits (31 + 30), canonical comm (the R^2 multiply)
    "ft255_61rows": FT255_61,
    "ft255_64rows": lambda: (ligero(3, 64, 128), 64 * 64),                        # four splits
    "ft191_100rows": lambda: (ligero(2, 64, 128), 100 * 64),                      # the generic kernel, NL = 6
    "ft127_2^12": lambda: (LigeroEncoding.new(1, 1 << 12), 1 << 12),              # NL = 4
    "ft255_2colblocks": lambda: (ligero(3, 512, 1024), 8 * 512),                  # two column blocks
    "ft255_61rows_blake2b": lambda: FT255_61(digest="blake2b"),                   # 16-word path entries
    "ft255_61rows_sha256": lambda: FT255_61(digest="sha256"),
}


@pytest.mark.parametrize("shape", sorted(SHAPES))
def test_bytes_equal_single_proves(shape):
    enc, n = SHAPES[shape]()
    if shape == "ft63_8rows":
        assert enc.get_n_degree_tests() > 1          # the multi-round loop and the stashed p_eval run
        assert max(0, (enc.n_cols - 1).bit_length()) == 6
    cms = batch_of(enc, 3, n, 41)
    outer = elems(enc, cms[0].n_rows, 42)
    check_prove(enc, cms, [outer] * 3, shared=outer)


@pytest.mark.parametrize("fid", [0, 3])
@pytest.mark.parametrize("n_rows", [7, 37])
def test_bytes_equal_single_proves_brakedown(oracle, fid, n_rows):
    """n_rows < 24: row-major members; n_rows >= 24: position-major members (column stride n_rows, the R^2 multiply)"""
    enc = sdig(oracle, fid)
    cms = batch_of(enc, 3, n_rows * 900, 43)
    assert cms[0].n_rows == n_rows and (cms[0].n_rows >= 24) == (n_rows == 37)      # the regime, by n_rows
    outer = elems(enc, n_rows, 44)
    check_prove(enc, cms, [outer] * 3, shared=outer)


@pytest.mark.parametrize("n_batch", [1, 2, 3, 7, 64])
def test_batch_sizes(n_batch):
    enc, n = FT255_61()
    cms = batch_of(enc, n_batch, n, 45)
    outer = elems(enc, 61, 46)
    check_prove(enc, cms, [outer] * n_batch, shared=outer, verify=n_batch <= 7)


def test_members_of_any_origin(oracle):
    enc, n = FT255_61()
    t = polys(enc, 3, n, 47)
    members = list(commit_batch(enc, t))
    t1 = polys(enc, 1, n, 48)
    members.append(LcCommit.commit_device(t1[0].data_ptr(), n, enc))
    members.append(LcCommit.commit(elems(enc, n, 49), enc))
    tb = polys(enc, 2, n, 50, stride=n + 64)
    members += commit_batch(enc, tb, n_coeffs=n, borrow=True)
    random.Random(5).shuffle(members)
    outer = elems(enc, 61, 51)
    check_prove(enc, members, [outer] * len(members), shared=outer)
    # Brakedown, position-major: slab members next to a single commit
    senc, rows = sdig(oracle, 3), 37
    ts = polys(senc, 2, rows * 900, 52)
    one = polys(senc, 1, rows * 900, 53)
    sm = list(commit_batch(senc, ts))
    sm.insert(1, LcCommit.commit_device(one[0].data_ptr(), rows * 900, senc))
    assert all(m.n_rows == rows >= 24 for m in sm)
    souter = elems(senc, rows, 54)
    check_prove(senc, sm, [souter] * 3, shared=souter, verify=False)


def test_shared_and_per_member_outer_tensors():
    enc, n = FT255_61()
    cms = batch_of(enc, 4, n, 55)
    outer = elems(enc, 61, 56)
    shared, _ = check_prove(enc, cms, [outer] * 4, shared=outer, verify=False)
    explicit, _ = check_prove(enc, cms, [outer] * 4, verify=False)             # the same tensor, (n_batch, n_rows, L)
    assert [p.to_bytes() for p in shared] == [p.to_bytes() for p in explicit]
    distinct = list(elems(enc, 4 * 61, 57).reshape(4, 61, enc.L))
    got, _ = check_prove(enc, cms, distinct)
    assert len({p.to_bytes() for p in got}) == 4


@pytest.mark.parametrize("shape", ["ft255_61rows", "ft63_8rows"])
def test_launches_do_not_grow_with_the_batch(shape):
    enc, n = SHAPES[shape]()
    stats = []
    for n_batch in (2, 16):
        cms = batch_of(enc, n_batch, n, 58)
        outer = elems(enc, cms[0].n_rows, 59)
        stats.append(check_prove(enc, cms, [outer] * n_batch, shared=outer, verify=False)[1])
    a, b = stats
    assert a.groups == b.groups == 1
    assert (a.collapse_launches, a.open_launches, a.host_syncs) == (b.collapse_launches, b.open_launches, b.host_syncs)
    assert a.collapse_launches > 0 and a.open_launches > 0
    assert a.host_syncs == enc.get_n_degree_tests() + 1      # one per degree-test round, one for the open


def test_groups():
    """Ft255 8192 x 16384, 8 rows: about 1 MiB of pinned arena per member, so 96 members cross the 64 MiB budget"""
    enc = ligero(3, 8192, 16384)
    n_rows, n_batch = 8, 96
    cms = batch_of(enc, n_batch, n_rows * 8192, 60)
    F, D = 8 * enc.L, enc.digest_len
    path_len = (enc.n_cols - 1).bit_length()
    arena = (2 * n_rows + 4 * enc.n_per_row) * F + enc.get_n_col_opens() * (8 + n_rows * F + path_len * D)     # the header's A
    per_group = max(1, _lib.PROVE_ARENA_BUDGET // arena)
    want_groups = -(-n_batch // per_group)
    assert want_groups == 2
    outer = elems(enc, n_rows, 61)
    _, stats = check_prove(enc, cms, [outer] * n_batch, shared=outer, verify=False)
    assert stats.groups == want_groups


def _raw(cms, n_batch, outer, n_outer, stride, trs, proofs="own", lens="own"):
    """the C entry point itself; returns (status, the proofs array)"""
    n = max(len(cms) if cms is not None else 0, len(trs) if trs is not None else 0, 1)
    ca = (C.c_void_p * n)(*cms) if cms is not None else None
    ta = (C.c_void_p * n)(*trs) if trs is not None else None
    pp = (C.c_void_p * n)(*([1] * n)) if proofs == "own" else None       # a sentinel: a failing call must store NULL over it
    pl = (C.c_uint64 * n)() if lens == "own" else None
    rc = _lib.lib().lcpcx_prove_batch(ca, n_batch, outer.ctypes.data_as(C.c_void_p) if outer is not None else None, n_outer, stride, ta,
                                      pp, pl, None, None)
    return rc, pp


def test_errors():
    enc, other_enc = ligero(3, 64, 128), ligero(3, 64, 128)
    n = 61 * 64
    a, b = batch_of(enc, 2, n, 62)
    short = batch_of(enc, 1, 8 * 64, 63)[0]              # another n_rows
    foreign = batch_of(other_enc, 1, n, 64)[0]           # another encoder
    empty = LcCommit(enc)                                # never committed
    outer = elems(enc, 61, 65)
    want = [m.prove(outer, enc, member_transcript(i)).to_bytes() for i, m in enumerate((a, b))]
    t0, t1 = member_transcript(0), member_transcript(1)
    A, B, T0, T1 = a._h, b._h, t0._h, t1._h
    cases = [
        (ERR_ARG, dict(cms=None, n_batch=2)),
        (ERR_ARG, dict(cms=[A, None])),
        (ERR_ARG, dict(trs=None)),
        (ERR_ARG, dict(trs=[T0, None])),
        (ERR_ARG, dict(outer=None)),
        (ERR_ARG, dict(proofs=None)),
        (ERR_ARG, dict(lens=None)),
        (ERR_ARG, dict(n_batch=0)),
        (ERR_ARG, dict(n_batch=65536)),
        (ERR_ARG, dict(cms=[A, A])),                     # a member listed twice
        (ERR_ARG, dict(trs=[T0, T0])),                   # a transcript listed twice
        (ERR_ARG, dict(cms=[A, foreign._h])),            # members of two encoders
        (ERR_ARG, dict(cms=[A, short._h])),              # members of different n_rows
        (ERR_ARG, dict(stride=60)),                      # 0 < outer_stride < n_outer
        (ERR_STATE, dict(cms=[A, empty._h])),            # an uncommitted member
        (ERR_OUTER_TENSOR, dict(n_outer=60)),
        (ERR_OUTER_TENSOR, dict(n_outer=62)),
    ]
    for code, kw in cases:
        args = dict(cms=[A, B], n_batch=2, outer=outer, n_outer=61, stride=0, trs=[T0, T1], proofs="own", lens="own")
        args.update(kw)
        if args["n_outer"] > 61:
            args["outer"] = np.concatenate([outer, outer])
        rc, pp = _raw(**args)
        assert rc == code, (kw, rc)
        if pp is not None and 0 < args["n_batch"] <= 65535:
            assert all(pp[i] is None for i in range(2)), kw          # every proofs[i] is NULL
    sh = ligero(3, 64, 128, shard=(0, 2))
    x, y = LcCommit(sh), LcCommit(sh)
    rc, pp = _raw([x._h, y._h], 2, outer, 61, 0, [T0, T1])
    assert rc == ERR_STATE and pp[0] is None and pp[1] is None      # a sharded encoder
    with pytest.raises(LcpcError) as e:
        prove_batch([a, b], outer[:60], [t0, t1])                    # the wrapper passes the status on
    assert e.value.code == ERR_OUTER_TENSOR
    # the members still prove alone, and together, with the right bytes
    assert [m.prove(outer, enc, member_transcript(i)).to_bytes() for i, m in enumerate((a, b))] == want
    assert [p.to_bytes() for p in prove_batch([a, b], outer, [member_transcript(0), member_transcript(1)])] == want




def test_concurrent_with_single_proves_and_refill():
    """two threads run overlapping batch proves while a third proves a shared member alone: all bytes as alone.  A refill of
    member 3 -- a member of the second thread's batch -- is issued meanwhile: it waits for the batch in flight and completes; each
    batch proof of member 3 is that of the commitment it held before or after, and a prove after it matches the new commitment"""
    enc, n = FT255_61()
    cms = commit_batch(enc, polys(enc, 4, n, 66))
    fresh = polys(enc, 1, n, 67)
    outer = elems(enc, 61, 68)
    alone = [cms[i].prove(outer, enc, member_transcript(i)).to_bytes() for i in range(4)]
    refilled = LcCommit.commit_device(fresh[0].data_ptr(), n, enc)
    refilled_root = refilled.get_root()
    refilled_proof = refilled.prove(outer, enc, member_transcript(3)).to_bytes()
    assert refilled_proof != alone[3]
    errs, start = [], threading.Barrier(4)

    def batch(idx):
        for _ in range(6):
            got = prove_batch([cms[i] for i in idx], outer, [member_transcript(i) for i in idx])
            for i, p in zip(idx, got):
                assert p.to_bytes() in ((alone[3], refilled_proof) if i == 3 else (alone[i],)), i

    def single():
        for _ in range(12):
            assert cms[2].prove(outer, enc, member_transcript(2)).to_bytes() == alone[2]

    def refill():
        LcCommit.commit_device(fresh[0].data_ptr(), n, enc, into=cms[3])

    def run(fn, *a):
        try:
            start.wait()
            fn(*a)
        except BaseException as ex:      # pragma: no cover
            errs.append(repr(ex))

    th = [threading.Thread(target=run, args=(batch, [0, 1, 2])), threading.Thread(target=run, args=(batch, [2, 3, 1])),
          threading.Thread(target=run, args=(single,)), threading.Thread(target=run, args=(refill,))]
    for x in th:
        x.start()
    for x in th:
        x.join(120)
    assert not any(x.is_alive() for x in th), "a thread did not finish"
    assert not errs, errs
    assert cms[3].get_root() == refilled_root
    got = prove_batch([cms[3], cms[0]], outer, [member_transcript(3), member_transcript(0)])
    assert got[0].to_bytes() == refilled_proof and got[1].to_bytes() == alone[0]

"""What tests/test_gpu_k2_batch.py rests on that needs no GPU (the built tree is needed: lcpc_amd/lib/liblcpc_k2b_harness.so): the batch
launchers of the position-major Brakedown kernels settle what they must BEFORE any launch -- n_batch == 0 or > 65535, more batch rows
than their grid's second dimension carries, Ft255 without the limb form, empty work -- the harness refuses indices outside its buffers
before it touches the device, and it is a library of its own beside the product."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import k2_harness as H  # noqa: E402
import k2b_harness as B  # noqa: E402
import test_k2_cases as K  # noqa: E402


def test_launchers_settle_bad_and_empty_jobs_before_any_launch():
    """null buffers throughout: a launcher that launched any of these would fault, and none touches the device"""
    for which, per_block in ((B.TRANSPOSE, 32), (B.SPMM, 128), (B.SDIG_RS, 128)):
        for fid in range(4):
            assert B.refusal(which, fid, 0, 37) == B.HIP_ERROR_INVALID_VALUE                 # n_batch == 0
            assert B.refusal(which, fid, 65536, 1) == B.HIP_ERROR_INVALID_VALUE              # beyond a grid dimension's members
            assert B.refusal(which, fid, 0, 37, work=0) == B.HIP_ERROR_INVALID_VALUE         # (checked before the emptiness)
            limit = 65535 * per_block
            # one batch row too many, as few members of many rows and as many members of few
            assert B.refusal(which, fid, 3, limit // 3 + 1) == B.HIP_ERROR_INVALID_VALUE
            assert B.refusal(which, fid, 65535, per_block + 1) == B.HIP_ERROR_INVALID_VALUE
            assert B.refusal(which, fid, 5, 37, work=0) == B.HIP_SUCCESS                     # no outputs / no valid positions
            assert B.refusal(which, fid, 5, 0) == B.HIP_SUCCESS                              # no rows
            with pytest.raises(B.BadArgs):                                                   # a job the launcher would launch: the harness's own refusal
                B.refusal(which, fid, 5, 37)
            with pytest.raises(B.BadArgs):                                                   # exactly the limit is such a job
                B.refusal(which, fid, 65535, per_block)
    assert B.refusal(B.SPMM, 3, 5, 37, limb=False) == B.HIP_ERROR_INVALID_VALUE              # Ft255 has the limb path only
    assert B.refusal(B.SPMM, 3, 5, 37, work=0, limb=False) == B.HIP_ERROR_INVALID_VALUE
    with pytest.raises(B.BadArgs):
        B.refusal(B.SPMM, 1, 5, 37, limb=False)                                              # Ft127 without it is the Wide<4> path: a real job


def test_harness_refuses_indices_outside_its_buffers():
    c = K._case("spmm", 1, 300, 24, in_off=0)
    rowptr, colidx, _ = K.build_structure(c)
    vals = np.zeros((len(colidx), 2), np.uint64)
    n_pos, n_rows = c.out_off + c.m, c.n_rows
    t = np.zeros((3, n_pos * n_rows + 2, 2), np.uint64)
    ok = H.Csr(1, rowptr, colidx, vals)

    def refused(fn, *a, **k):
        with pytest.raises(B.BadArgs):
            fn(*a, **k)

    bad_col = colidx.copy()
    bad_col[len(bad_col) // 2] = c.n_in
    short = rowptr.copy()
    short[-1] -= 1
    refused(B.spmm_t, 1, t, n_pos, n_rows, c.n_in, 0, c.out_off, H.Csr(1, rowptr, bad_col, vals), True)
    refused(B.spmm_t, 1, t, n_pos, n_rows, c.n_in, 0, c.out_off, H.Csr(1, short, colidx, vals), True)
    refused(B.spmm_t, 1, t, n_pos, n_rows, c.n_in, 0, c.out_off + 1, ok, True)               # the last output beyond a member's T
    refused(B.spmm_t, 1, t, n_pos, n_rows, c.n_in, 0, 1, ok, True)                           # outputs over the inputs
    refused(B.spmm_t, 1, t, n_pos + 1, n_rows, c.n_in, 0, c.out_off, ok, True)               # a member larger than the stride
    refused(B.spmm_t, 1, t, n_pos, n_rows, c.n_in, 0, c.out_off, ok, True, np.zeros((3, c.m * n_rows - 2, 2), np.uint64))   # out_alt too
    refused(B.spmm_t, 0, np.zeros((3, n_pos * n_rows + 2, 1), np.uint64), n_pos, n_rows, c.n_in, 0, c.out_off,
            H.Csr(0, rowptr, colidx, np.zeros((len(colidx), 1), np.uint64)), True)           # Ft63 has no limb form
    refused(B.spmm_t, 0, np.zeros((3, n_pos * n_rows + 1, 1), np.uint64), n_pos, n_rows, c.n_in, 0, c.out_off,
            H.Csr(0, rowptr, colidx, np.zeros((len(colidx), 1), np.uint64)), False)          # a stride that is no multiple of 16 bytes
    refused(B.sdig_rs_t, 1, np.zeros((2, 4 * 24, 2), np.uint64), 4, np.zeros((2, 10 * 24, 2), np.uint64), 10, 24, 3, 8)
    refused(B.sdig_rs_t, 1, np.zeros((2, 4 * 24 - 2, 2), np.uint64), 4, np.zeros((2, 12 * 24, 2), np.uint64), 12, 24, 3, 8)
    # the stacked source one element short of the last member's last row
    refused(B.transpose_to_t, 1, np.zeros((3 * 24 * 10 - 1, 2), np.uint64), 10, 10, 24, np.zeros((3, 10 * 24, 2), np.uint64))
    refused(B.transpose_to_t, 1, np.zeros((3 * 24 * 10, 2), np.uint64), 10, 10, 24, np.zeros((3, 10 * 24 - 2, 2), np.uint64))


def test_k2b_harness_is_a_separate_library():
    """lib/liblcpc_k2b_harness.so exports the k2bh_* entry points of tests/k2b_harness.py and nothing of the product, which it links
    against and which carries no trace of it (tests/test_abi.py holds the other harnesses to the same)"""
    from lcpc_amd import _lib
    assert os.path.dirname(B.LIB_PATH) == os.path.dirname(_lib.LIB_PATH) and os.path.exists(B.LIB_PATH)
    defined = [l.split() for l in subprocess.check_output(["nm", "-D", "--defined-only", B.LIB_PATH], text=True).splitlines()]
    funcs = sorted(l[-1] for l in defined if l[-2] in "TtWw")
    assert funcs == sorted(B.SYMBOLS) and all(f.startswith("k2bh_") for f in funcs)
    assert not any("lcpc" in l[-1] for l in defined)
    needed = re.findall(r"NEEDED.*\[(.*?)\]", subprocess.run(["readelf", "-d", B.LIB_PATH], capture_output=True, text=True).stdout)
    assert "liblcpc_hip.so" in needed
    assert b"k2bh_" not in open(_lib.LIB_PATH, "rb").read()
    from test_abi import make_builds
    assert make_builds("k2b_harness", "tests/native/k2b_harness.cpp") == (True, True)

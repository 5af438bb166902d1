"""ctypes side of tests/native/k17_harness.cpp (lcpc_amd/lib/liblcpc_k17_harness.so, built by lcpc_amd/csrc/Makefile): the scan
launcher (K17, launch_scan of lcpc_amd/csrc/kernels.h) with canaries around the output, the totals and the workspace, K17b alone on
a caller's tile totals, and the launcher's refusals.  Errors as in tests/harness_kit.py."""
import ctypes as C

import numpy as np

import fft_cases as FC
import harness_kit as K
from harness_kit import BadArgs, HipError, check as _check, ptr as _ptr  # noqa: F401

LIB_PATH = K.lib_path("k17")
HIP_SUCCESS, HIP_ERROR_INVALID_VALUE = 0, 1
CANARY, PAD = K.CANARY, K.PAD                      # the canary elements around an output: harness_kit.padded
OPS = {"sum": 0, "product": 1}
MODES = {"inclusive": 0, "exclusive": 1}

_vp, _u64, _u32, _i32 = C.c_void_p, C.c_uint64, C.c_uint32, C.c_int
SYMBOLS = {
    "k17h_device_count": (_i32, []),
    "k17h_cu_count": (_i32, []),
    "k17h_tile": (_u32, [_i32]),
    "k17h_lane_elems": (_u32, [_i32]),
    "k17h_mid_chunk": (_u32, [_i32]),
    "k17h_work_elems": (_u64, [_i32, _u64, _u32]),
    "k17h_scan": (_i32, [_i32, _i32, _i32, _vp, _u64, _u32, _vp, _u64, _u64, _i32, _vp, _vp, _u64, _u64, _vp, _vp, _u64, _u64, _vp]),
    "k17h_scan_totals": (_i32, [_i32, _i32, _vp, _u64, _u32, _vp, _u64, _u64, _vp, _vp, _u64, _u64, _vp, _vp, _u64, _u64]),
    "k17h_scan_refusal": (_i32, [_i32, _i32, _i32, _u64, _u32, _u32, _u32, _i32, _i32]),
}


def lib():
    return K.load("k17", SYMBOLS)


def tile(nl):
    """the elements of a workgroup's tile"""
    return lib().k17h_tile(nl)


def lane_elems(nl):
    """the consecutive elements a lane holds"""
    return lib().k17h_lane_elems(nl)


def mid_chunk(nl):
    """the tile totals K17b takes per recursion level"""
    return lib().k17h_mid_chunk(nl)


def work_elems(nl, n, n_vecs=1):
    return lib().k17h_work_elems(nl, n, n_vecs)


def run_scan(fid, op, mode, x, init=None, in_place=False, totals_only=False):
    """launch_scan on the device.  x: (n, L) or (n_vecs, n, L) limbs; init: (n_vecs, L) limbs or None.  totals_only: through
    k17h_scan_totals, K17b alone (exclusive, in place).  Returns (out of x's shape, (n_vecs, L) totals, kernels launched); the
    canaries around the output, the totals and the workspace must come back untouched, and so must an out-of-place input"""
    F = FC.field(fid)
    nl = 2 * F.L
    x = np.ascontiguousarray(x, np.uint64)
    v = x.reshape(-1, x.shape[-2], F.L)
    n_vecs, n = v.shape[0], v.shape[1]
    keep = v.copy()
    one = FC.mont(fid, [1])
    ini = None if init is None else np.ascontiguousarray(init, np.uint64).reshape(n_vecs, F.L)
    buf = K.padded(n_vecs * n, F.L)
    tot = K.padded(n_vecs, F.L)
    work = K.padded(work_elems(nl, n, n_vecs), F.L)
    launches = C.c_uint32(0)
    off = PAD * nl
    if totals_only:
        _check("k17h_scan_totals", lib().k17h_scan_totals(nl, OPS[op], _ptr(v), n, n_vecs, _ptr(buf), buf.size * 2, off, None if ini is None else _ptr(ini),
                                                         _ptr(tot), tot.size * 2, off, _ptr(one), _ptr(work), work.size * 2, off))
    else:
        _check("k17h_scan", lib().k17h_scan(nl, OPS[op], MODES[mode], _ptr(v), n, n_vecs, _ptr(buf), buf.size * 2, off, int(in_place),
                                           None if ini is None else _ptr(ini), _ptr(tot), tot.size * 2, off, _ptr(one), _ptr(work),
                                           work.size * 2, off, C.byref(launches)))
    out, totals = K.inner(buf), K.inner(tot, "the totals")
    K.inner(work, "the workspace")
    assert (v == keep).all(), "the input was written"
    return out.reshape(x.shape).copy(), totals.copy(), launches.value


def scan_refusal(nl, op, mode, n, n_vecs=1, null_mask=0, misalign=0, overlap=0, short_work=0):
    """the hipError_t of launch_scan on a job it must settle before any launch (never-read buffers; no device is touched); BadArgs
    when the job is one a correct launcher would launch.  bits: 0 in, 1 out, 2 work, 3 init, 4 total, 5 one; overlap: 1 out one
    element behind in, 2 init in the output, 3 total in the input, 4 work on the output's last element, 5 init is total"""
    rc = lib().k17h_scan_refusal(nl, OPS.get(op, op), MODES.get(mode, mode), n, n_vecs, null_mask, misalign, overlap, short_work)
    if rc == -1:
        raise BadArgs("k17h_scan_refusal")
    return rc

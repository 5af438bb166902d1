"""ctypes side of tests/native/k18_harness.cpp (lcpc_amd/lib/liblcpc_k18_harness.so, built by lcpc_amd/csrc/Makefile): the sumcheck
launchers (K18 / K19 of lcpc_amd/csrc/kernels.h) with a max_groups of the caller's choice, canaries around every output, the evals
and the workspace, and the launchers' refusals.  Errors as in tests/harness_kit.py."""
import ctypes as C

import numpy as np

import fft_cases as FC
import sumcheck_cases as MC
import harness_kit as K
from harness_kit import BadArgs, HipError, check as _check, ptr as _ptr  # noqa: F401

LIB_PATH = K.lib_path("k18")
HIP_SUCCESS, HIP_ERROR_INVALID_VALUE = 0, 1
CANARY, PAD = K.CANARY, K.PAD                      # the canary elements around an output: harness_kit.padded
ORDERS = {"low": 0, "high": 1}
MODES = {"bind": 0, "round": 1, "fused": 2}

_vp, _u64, _u32, _i32 = C.c_void_p, C.c_uint64, C.c_uint32, C.c_int
SYMBOLS = {
    "k18h_device_count": (_i32, []),
    "k18h_cu_count": (_i32, []),
    "k18h_tile_pairs": (_u32, [_i32]),
    "k18h_default_groups": (_u32, []),
    "k18h_work_elems": (_u64, [_u64, _u32, _u32]),
    "k18h_run": (_i32, [_i32, _i32, _i32, _vp, _u64, _u32, _vp, _u64, _u64, _i32, _vp, _u32, _vp, _vp, _vp, _vp, _u64, _u64, _vp, _u64, _u64, _u32, _vp]),
    "k18h_refusal": (_i32, [_i32, _i32, _i32, _u64, _u32, _vp, _u32, _u32, _u32, _i32, _i32, _u32]),
}


def lib():
    return K.load("k18", SYMBOLS)


def tile_pairs(nl):
    """P: the pairs a workgroup takes per stride of its loop"""
    return lib().k18h_tile_pairs(nl)


def default_groups():
    """the max_groups the product passes"""
    return lib().k18h_default_groups()


def work_elems(pairs, n_terms, max_groups):
    return lib().k18h_work_elems(pairs, n_terms, max_groups)


def term_words(terms):
    """(coefficient, indices) terms -> the (n_terms, 5) uint32 records the launchers take"""
    t = np.zeros((max(len(terms), 1), 5), np.uint32)
    for m, (_, idx) in enumerate(terms):
        t[m, 0] = len(idx)
        t[m, 1:1 + len(idx)] = idx
    return t


def run(mode, fid, order, tabs, terms=None, r=None, max_groups=None, in_place=False):
    """one launcher on the device.  tabs: (n_tables, n, L) limbs; terms: (canonical coefficient or None, indices); r: a canonical int.
    Returns (bound tables (n_tables, n / 2, L) or None, evals (d + 1, L) or None, kernels launched).  The canaries around every
    output, the evals and the workspace must come back untouched, and so must an out-of-place input and, in place, the upper half"""
    F = FC.field(fid)
    nl = 2 * F.L
    tabs = np.ascontiguousarray(tabs, np.uint64)
    n_tables, n = tabs.shape[0], tabs.shape[1]
    keep = tabs.copy()
    bind, rnd = mode != "round", mode != "bind"
    max_groups = default_groups() if max_groups is None else max_groups
    one = FC.mont(fid, [1])
    rl = None if r is None else FC.mont(fid, [r])
    d = MC.degree(terms) if rnd else 0
    cs = None
    if rnd and any(c is not None for c, _ in terms):
        cs = FC.mont(fid, [1 if c is None else c for c, _ in terms])
    tw = term_words(terms) if rnd else None
    span = n if in_place else n // 2
    slot = PAD + span + PAD
    out = np.full((n_tables, slot, F.L), CANARY, np.uint64)
    ev = K.padded(5, F.L)
    pairs = n // 4 if mode == "fused" else n // 2
    need = work_elems(pairs, len(terms), max_groups) if rnd else 0
    work = K.padded(need, F.L)
    launches = C.c_uint32(0)
    off = PAD * nl
    _check("k18h_run", lib().k18h_run(MODES[mode], nl, ORDERS[order], _ptr(tabs), n, n_tables, _ptr(out), slot * nl, off, int(in_place),
                                     None if tw is None else _ptr(tw), len(terms) if rnd else 0, None if cs is None else _ptr(cs), _ptr(one),
                                     None if rl is None else _ptr(rl), _ptr(ev), ev.size * 2, off, _ptr(work), work.size * 2, off, max_groups,
                                     C.byref(launches)))
    assert (tabs == keep).all(), "an input was written"
    K.inner(work, "the workspace")
    bound = evals = None
    if bind:
        assert (out[:, :PAD] == CANARY).all() and (out[:, PAD + span:] == CANARY).all(), "elements around an output were written"
        if in_place:
            assert (out[:, PAD + n // 2:PAD + n] == keep[:, n // 2:]).all(), "in place, the upper half was written"
        bound = out[:, PAD:PAD + n // 2].copy()
    else:
        assert (out == CANARY).all()
    if rnd:
        assert (ev[:PAD] == CANARY).all() and (ev[PAD + d + 1:] == CANARY).all(), "elements around the evals were written"
        evals = ev[PAD:PAD + d + 1].copy()
        if launches.value == 1:
            assert (work == CANARY).all(), "one workgroup does not touch the workspace"
    else:
        assert (ev == CANARY).all() and (work == CANARY).all()
    return bound, evals, launches.value


def refusal(mode, nl, order, n, n_tables=2, terms=((None, [0, 1]),), n_terms=None, null_mask=0, misalign=0, overlap=0, short_work=0, max_groups=4):
    """the hipError_t of a launcher on a job it must settle before any launch (never-read buffers; no device is touched); BadArgs
    when the job is one a correct launcher would launch.  The bits and the overlaps are listed at k18h_refusal"""
    tw = terms if isinstance(terms, np.ndarray) else term_words(list(terms))
    rc = lib().k18h_refusal(MODES.get(mode, mode), nl, ORDERS.get(order, order), n, n_tables, _ptr(tw), len(terms) if n_terms is None else n_terms, null_mask,
                            misalign, overlap, short_work, max_groups)
    if rc == -1:
        raise BadArgs("k18h_refusal")
    return rc

"""Shared by tests/test_scan_abi.py, tests/test_k17_cases.py, tests/test_gpu_k17_kernels.py and tests/test_gpu_scan.py: the operand sets
and the Python bignum references of include/lcpc_hip_scan.h -- running sums and products of canonical Python ints mod p -- and the
ctypes calls of the host entry points with canaries around the output and the total.  Everything is exact."""
import ctypes as C

import numpy as np

from lcpc_amd import _lib

import fft_cases as FC

FIELDS = FC.FIELDS
CANARY = FC.CANARY
ERR_ARG = FC.ERR_ARG
vp = FC.vp
OPS = ("sum", "product")
MODES = ("inclusive", "exclusive")
PAD = 8                                              # canary elements in front of and behind an output
# the places of the single zero of the "zero_at_edges" family: the first and the last element of a lane's chunk, of a tile and of the
# vector -- the exact position from which a product is zero
EDGES = ("zero_lane_first", "zero_lane_last", "zero_tile_first", "zero_tile_last", "zero_vec_first", "zero_vec_last")
SETS = ("random", "nonzero", "ones", "minus_ones", "zeros", "all_pm1_sum") + EDGES


def edge_position(name, n, tile, lane_elems):
    """where the zero of an EDGES set stands among n elements: in the LAST tile that holds the place whole, at lane 5's chunk for the
    lane edges (any lane but the first and the last of a wave does)"""
    base = ((n - 1) // tile) * tile                  # the last tile's first element
    if base and base + 6 * lane_elems > n:           # a ragged last tile too short for lane 5: the tile before it
        base -= tile
    at = {"zero_lane_first": base + 5 * lane_elems, "zero_lane_last": base + 6 * lane_elems - 1, "zero_tile_first": base,
          "zero_tile_last": base + tile - 1, "zero_vec_first": 0, "zero_vec_last": n - 1}[name]
    return min(at, n - 1)


def operands(fid, name, n, tile=4096, lane_elems=16, *key):
    """n canonical ints.  "random" has 0, 1 and p - 1 planted, "nonzero" has no zero (a product stays alive to the end).  "minus_ones": products alternate p - 1 and 1, sums wrap around p at every step; "all_pm1_sum": 1 and p - 1 at
    random, so a running sum walks to both sides of zero and a product changes sign at random; EDGES: one zero among nonzero random
    elements"""
    F = FC.field(fid)
    rnd = FC.rng("scan", fid, name, n, *key)
    if name == "ones":
        return [1] * n
    if name == "minus_ones":
        return [F.p - 1] * n
    if name == "zeros":
        return [0] * n
    if name == "all_pm1_sum":
        return [rnd.choice((1, F.p - 1)) for _ in range(n)]
    if name == "random":
        x = [rnd.randrange(F.p) for _ in range(n)]
        if n >= 8:
            for v in (0, 1, F.p - 1):
                x[rnd.randrange(n)] = v
        return x
    x = [rnd.randrange(1, F.p) for _ in range(n)]
    if name == "nonzero":
        return x
    x[edge_position(name, n, tile, lane_elems)] = 0
    return x


def scan_ref(fid, op, mode, x, init=None):
    """(out, total) by the definition: out[k] = c (+) x[0] (+) ... (+) x[k] (inclusive) or ... x[k - 1] (exclusive)"""
    F = FC.field(fid)
    run = (0 if op == "sum" else 1) if init is None else init % F.p
    out = []
    for v in x:
        if mode == "exclusive":
            out.append(run)
        run = (run + v) % F.p if op == "sum" else run * v % F.p
        if mode == "inclusive":
            out.append(run)
    return out, run


def ratio_terms(fid, num, den):
    """num[k] / den[k], zero where den[k] is zero"""
    F = FC.field(fid)
    return [u * pow(v, F.p - 2, F.p) % F.p for u, v in zip(num, den)]


def elem(fid, v):
    """one element: the L Montgomery limbs of a canonical int (None stays None)"""
    return None if v is None else FC.mont(fid, [v])[0].copy()


def _host(fn, ins, n, L, out, want_total, expect):
    """fn(*ins, out, total) with canaries around out (unless `out` is given: the in-place call) and around total.  rc checked.
    Returns (the n output elements, the total or None)"""
    tot = np.full((3, L), CANARY, np.uint64)
    buf = np.full((PAD + n + PAD, L), CANARY, np.uint64) if out is None else None
    o = buf[PAD:PAD + n] if out is None else out
    rc = fn(*[vp(a) for a in ins], vp(o), vp(tot[1:]) if want_total else None)
    assert rc == expect, rc
    assert (tot[0] == CANARY).all() and (tot[2] == CANARY).all(), "elements around the total were written"
    if buf is not None:
        assert (buf[:PAD] == CANARY).all() and (buf[PAD + n:] == CANARY).all(), "elements around the output were written"
    if expect or not want_total:
        assert (tot == CANARY).all(), "a total was written without being asked for"
    if expect and buf is not None:
        assert (buf == CANARY).all(), "an output was written on an error"
    return o, (tot[1].copy() if want_total and not expect else None)


def host_scan(fid, op, mode, x_limbs, init=None, want_total=True, out=None, n=None, expect=0):
    """lcpcs_scan; op and mode by name or number, init: L limbs or None"""
    n = x_limbs.shape[0] if n is None else n
    o = _lib.SCAN_OPS[op] if isinstance(op, str) else op
    m = _lib.SCAN_MODES[mode] if isinstance(mode, str) else mode
    lib = _lib.lib()
    return _host(lambda i, out_, tot: lib.lcpcs_scan(fid, o, m, i, out_, n, vp(init), tot), (x_limbs,), min(max(n, 1), x_limbs.shape[0]), x_limbs.shape[-1], out,
                 want_total, expect)


def host_scan_ratio(fid, op, mode, num_limbs, den_limbs, init=None, want_total=True, out=None, n=None, expect=0):
    n = num_limbs.shape[0] if n is None else n
    o = _lib.SCAN_OPS[op] if isinstance(op, str) else op
    m = _lib.SCAN_MODES[mode] if isinstance(mode, str) else mode
    lib = _lib.lib()
    return _host(lambda a, b, out_, tot: lib.lcpcs_scan_ratio(fid, o, m, a, b, out_, n, vp(init), tot), (num_limbs, den_limbs), min(max(n, 1), num_limbs.shape[0]),
                 num_limbs.shape[-1], out, want_total, expect)


REFUSAL_N, REFUSAL_VECS = 5000, 3


def refusal_buffer_bytes(lib, h, L):
    """the bytes of each of the six buffers device_refusals takes"""
    return REFUSAL_N * REFUSAL_VECS * 8 * L + lib.lcpcs_scan_work_bytes(h, REFUSAL_N, REFUSAL_VECS) + 64 * 8 * L


def device_refusals(lib, h, L, buffers):
    """every refusal of lcpcs_scan_device / lcpcs_scan_ratio_device that takes a context: each is settled before any HIP call.
    buffers: six device addresses of refusal_buffer_bytes each, aligned, which no refused call reads or writes -- they are real so
    that every pointer handed over, offsets included, stays inside an allocation"""
    eb, n, n_vecs = 8 * L, REFUSAL_N, REFUSAL_VECS
    wb = lib.lcpcs_scan_work_bytes
    need = wb(h, n, n_vecs)
    assert need > 0 and need % eb == 0
    # work_bytes: 0 for what the scan refuses, monotone in n
    assert wb(None, n, 1) == 0 and wb(h, 0, 1) == 0 and wb(h, n, 0) == 0 and wb(h, n, 65536) == 0 and wb(h, 1 << 39, 1) == 0
    assert wb(h, 1 << 38, 2) == 0 and wb(h, 1 << 34, 1) > 0 and wb(h, 1 << 36, 1) == 0       # (2^24 tiles or more: the grid)
    last = 0
    for k in list(range(1, 70)) + [2047, 2048, 2049, 4095, 4096, 4097, 1 << 20, (1 << 22) + 1, (1 << 24) + 1, 1 << 30, 1 << 34]:
        assert wb(h, k, 1) >= max(last, eb) and wb(h, k, 3) == (3 * wb(h, k, 1) if 3 * k < 1 << 39 else 0), k
        last = wb(h, k, 1)
    IN, OUT, DEN, INIT, TOT, WORK = (C.c_void_p(b) for b in buffers)
    span = n * n_vecs * eb

    def scan(op=1, mode=0, i=IN, o=OUT, n_=n, v=n_vecs, init=INIT, tot=TOT, work=WORK, bytes_=need, ctx=h):
        return lib.lcpcs_scan_device(ctx, op, mode, i, o, n_, v, init, tot, work, bytes_, None)

    def ratio(op=1, mode=1, a=IN, b=DEN, o=OUT, n_=n, v=n_vecs, init=INIT, tot=TOT, work=WORK, bytes_=need, ctx=h):
        return lib.lcpcs_scan_ratio_device(ctx, op, mode, a, b, o, n_, v, init, tot, work, bytes_, None)

    at = lambda p, off: C.c_void_p(p.value + off)
    for f in (scan, ratio):
        assert f(ctx=None) == ERR_ARG
        assert f(op=2) == ERR_ARG and f(mode=2) == ERR_ARG
        assert f(n_=0) == ERR_ARG and f(v=0) == ERR_ARG and f(v=65536) == ERR_ARG and f(n_=1 << 39, v=1) == ERR_ARG and f(n_=1 << 38, v=2) == ERR_ARG
        assert f(o=None) == ERR_ARG and f(work=None) == ERR_ARG
        assert f(bytes_=need - 1) == ERR_ARG and f(bytes_=0) == ERR_ARG
        for name in ("o", "init", "tot", "work"):                      # misaligned
            assert f(**{name: at({"o": OUT, "init": INIT, "tot": TOT, "work": WORK}[name], 4)}) == ERR_ARG, name
        # init, total and work meet nothing: the output, each other
        assert f(init=at(OUT, eb)) == ERR_ARG and f(tot=at(OUT, span - eb)) == ERR_ARG and f(work=at(OUT, span - eb)) == ERR_ARG
        assert f(init=TOT) == ERR_ARG and f(tot=at(INIT, 2 * eb)) == ERR_ARG
        assert f(work=at(INIT, 2 * eb)) == ERR_ARG and f(work=at(TOT, eb)) == ERR_ARG
        assert f(o=at(WORK, need - eb)) == ERR_ARG
        assert f(work=OUT) == ERR_ARG and f(o=WORK) == ERR_ARG and f(n_=1 << 36, v=1) == ERR_ARG
    assert scan(i=None) == ERR_ARG and scan(i=at(IN, 4)) == ERR_ARG
    assert scan(o=at(IN, eb)) == ERR_ARG and scan(i=at(OUT, eb)) == ERR_ARG and scan(o=at(IN, span - eb)) == ERR_ARG      # partial overlap
    assert scan(init=at(IN, eb)) == ERR_ARG and scan(tot=IN) == ERR_ARG and scan(work=at(IN, span - eb)) == ERR_ARG
    assert scan(work=IN) == ERR_ARG and scan(i=WORK) == ERR_ARG and scan(i=WORK, o=WORK) == ERR_ARG and ratio(work=DEN) == ERR_ARG and ratio(work=IN) == ERR_ARG
    for name, p in (("a", IN), ("b", DEN)):
        assert ratio(**{name: None}) == ERR_ARG and ratio(**{name: at(p, 4)}) == ERR_ARG
        assert ratio(**{name: at(OUT, eb)}) == ERR_ARG and ratio(o=at(p, eb)) == ERR_ARG
        assert ratio(init=at(p, eb)) == ERR_ARG and ratio(tot=p) == ERR_ARG and ratio(work=at(p, span - eb)) == ERR_ARG

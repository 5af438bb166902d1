"""Shared by tests/test_quot_abi.py, tests/test_gpu_k15_kernels.py and tests/test_gpu_quot.py: the operand sets and the Python bignum
references of include/lcpc_hip_quot.h -- pow(x, p - 2, p), the definitions of the two quotients point by point, synthetic division --
and the ctypes calls of the host entry points with canary-filled outputs.  Everything is exact: canonical Python ints mod p."""
import numpy as np

from lcpc_amd import _lib

import domain_cases as DC
import fft_cases as FC

FIELDS = FC.FIELDS
CANARY = FC.CANARY
ERR_ARG = FC.ERR_ARG
ORDERS = DC.ORDERS
OPS = ("add", "sub", "mul", "div")
vp = FC.vp
# the operand sets of an inversion; `tile` and `lanes` place the zeros of "edge_zeros" and "one_nonzero" (the host forms have no tile:
# any value does)
SETS = ("random", "ones", "minus_ones", "zeros", "edge_zeros", "one_nonzero")


def operands(fid, name, n, tile=4096, lanes=512, *key):
    """n canonical ints.  A lane of a tile takes the elements lane + j * lanes of it: "edge_zeros" puts a zero at the first and the last
    position of lane 0's and of the last lane's chunk in every tile, at both ends of every tile and at both ends of the vector, among
    random nonzero elements; "one_nonzero" leaves one element per tile (and the last of the vector) nonzero"""
    F = FC.field(fid)
    rnd = FC.rng("quot", fid, name, n, *key)
    if name == "ones":
        return [1] * n
    if name == "minus_ones":
        return [F.p - 1] * n
    if name == "zeros":
        return [0] * n
    if name == "random":
        x = [rnd.randrange(F.p) for _ in range(n)]
        for v in (0, 1, F.p - 1):
            if n >= 8:
                x[rnd.randrange(n)] = v
        return x
    if name == "edge_zeros":
        x = [rnd.randrange(1, F.p) for _ in range(n)]
        for base in range(0, n, tile):
            for off in (0, lanes - 1, tile - lanes, tile - 1, lanes, tile - lanes - 1):
                if 0 <= base + off < n:
                    x[base + off] = 0
        x[n - 1] = 0
        if n > 2:
            x[1] = rnd.randrange(1, F.p)      # (a nonzero neighbour of the first zero)
        return x
    assert name == "one_nonzero"
    x = [0] * n
    for base in range(0, n, tile):
        x[min(n - 1, base + rnd.randrange(tile))] = rnd.randrange(1, F.p)
    x[n - 1] = rnd.randrange(1, F.p)
    return x


def inverse_ref(fid, x):
    F = FC.field(fid)
    return [pow(v, F.p - 2, F.p) for v in x]          # (0^(p - 2) = 0: a zero gives zero)


def pointwise_ref(fid, op, a, b):
    F = FC.field(fid)
    if op == "add":
        return [(u + v) % F.p for u, v in zip(a, b)]
    if op == "sub":
        return [(u - v) % F.p for u, v in zip(a, b)]
    if op == "mul":
        return [u * v % F.p for u, v in zip(a, b)]
    return [u * pow(v, F.p - 2, F.p) % F.p for u, v in zip(a, b)]


def points(fid, s, log_m):
    """x_k = s w_m^k, natural"""
    F = FC.field(fid)
    w = FC.root(fid, log_m)
    out, x = [], s % F.p
    for _ in range(1 << log_m):
        out.append(x)
        x = x * w % F.p
    return out


def place(v, log_m, order):
    """natural values -> the stored order"""
    return FC.permute(list(v), log_m) if order == "bitrev" else list(v)


def linear_ref(fid, vals, s, z, y, order):
    """vals in the stored order -> (vals[k] - y) / (x_k - z) in the stored order, by the definition"""
    F = FC.field(fid)
    log_m = len(vals).bit_length() - 1
    nat = place(vals, log_m, order)                   # (the permutation is its own inverse)
    out = [(v - y) * pow((x - z) % F.p, F.p - 2, F.p) % F.p for v, x in zip(nat, points(fid, s, log_m))]
    return place(out, log_m, order)


def vanishing_ref(fid, vals, s, log_n, order):
    F = FC.field(fid)
    log_m = len(vals).bit_length() - 1
    nat = place(vals, log_m, order)
    out = [v * pow((pow(x, 1 << log_n, F.p) - 1) % F.p, F.p - 2, F.p) % F.p for v, x in zip(nat, points(fid, s, log_m))]
    return place(out, log_m, order)


def synthetic_division(fid, coeffs, z):
    """(q, r) with sum_i coeffs[i] X^i = q(X) (X - z) + r"""
    F = FC.field(fid)
    q, acc = [0] * (len(coeffs) - 1), 0
    for i in range(len(coeffs) - 1, 0, -1):
        acc = (acc * z + coeffs[i]) % F.p
        q[i - 1] = acc
    return q, (acc * z + coeffs[0]) % F.p


def off_domain(fid, s, log_m, *key):
    """a canonical z with (z / s)^m != 1"""
    F = FC.field(fid)
    rnd = FC.rng("z", fid, s, log_m, *key)
    while True:
        z = rnd.randrange(F.p)
        if pow(z * pow(s, -1, F.p) % F.p, 1 << log_m, F.p) != 1:
            return z


def coset_shifts(fid, log_m, *key):
    """name -> a canonical shift with shift^m != 1: the generator and one seeded random element"""
    F = FC.field(fid)
    rnd = FC.rng("qshift", fid, log_m, *key)
    while True:
        s = rnd.randrange(2, F.p)
        if pow(s, 1 << log_m, F.p) != 1:
            return {"gen": DC.GENERATORS[fid], "random": s}


def _call(fn, args, rows, L, out, expect):
    if out is not None:
        assert fn(*args, vp(out)) == expect
        return out
    buf = np.full((rows + 2, L), CANARY, np.uint64)
    rc = fn(*args, vp(buf))
    assert rc == expect, rc
    assert (buf[rows:] == CANARY).all()
    if expect:
        assert (buf == CANARY).all(), "an output was written on an error"
    return buf[:rows]


def host_inverse(fid, x_limbs, n=None, out=None, expect=0):
    """lcpcq_batch_inverse with a canary-filled output (or `out`, for the in-place call): rc checked -> the n output elements"""
    n = x_limbs.shape[0] if n is None else n
    lib = _lib.lib()
    return _call(lambda i, o: lib.lcpcq_batch_inverse(fid, i, o, n), (vp(x_limbs),), n, x_limbs.shape[-1], out, expect)


def host_pointwise(fid, op, a_limbs, b_limbs, n=None, out=None, expect=0):
    n = a_limbs.shape[0] if n is None else n
    o = _lib.QUOT_OPS[op] if isinstance(op, str) else op
    lib = _lib.lib()
    return _call(lambda a, b, out_: lib.lcpcq_pointwise(fid, o, a, b, out_, n), (vp(a_limbs), vp(b_limbs)), n, a_limbs.shape[-1], out, expect)


def host_divide_linear(fid, shift_limbs_, order, v_limbs, log_m, z_limbs, y_limbs, out=None, expect=0):
    o = _lib.DOMAIN_ORDERS[order] if isinstance(order, str) else order
    lib = _lib.lib()
    return _call(lambda s, i, z, y, out_: lib.lcpcq_divide_linear(fid, s, o, i, log_m, z, y, out_),
                 (vp(shift_limbs_), vp(v_limbs), vp(z_limbs), vp(y_limbs)), 1 << log_m if log_m < 20 else 1, v_limbs.shape[-1], out, expect)


def host_divide_vanishing(fid, shift_limbs_, order, v_limbs, log_m, log_n, out=None, expect=0):
    o = _lib.DOMAIN_ORDERS[order] if isinstance(order, str) else order
    lib = _lib.lib()
    return _call(lambda s, i, out_: lib.lcpcq_divide_vanishing(fid, s, o, i, log_m, log_n, out_), (vp(shift_limbs_), vp(v_limbs)),
                 1 << log_m if log_m < 20 else 1, v_limbs.shape[-1], out, expect)

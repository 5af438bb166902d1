#!/usr/bin/env python3
"""tools/bench_quot.py -- batch inversion and the domain quotients (include/lcpc_hip_quot.h) on one box, in one process, the variants
alternated call by call.  One JSON line per leg with the median and the spread (min, max) of every side; kept under
profiles/r19_quot.jsonl.  Wall clock around the calls and a synchronisation.

  python tools/bench_quot.py [--reps 7] [--host-reps 3] [--fields 3,0] [--sizes 20,22,24,26] [--host-max 22] [--tag TAG]

  inverse     per field and log2 n: lcpcq_batch_inverse_device next to lcpcq_pointwise_device LCPCQ_MUL of the same length (what the
              call would cost if inverses were free, at equal traffic) and LCPCQ_DIV; up to --host-max also the route without the
              extension: download, lcpcq_batch_inverse on one host thread, upload.  The two routes must have produced equal bytes
              (asserted) before anything is timed.
  linear      2^22, n_vecs 1 and 8: lcpcq_divide_linear_device next to LCPCQ_MUL by a precomputed vector over the same bytes; with
              y = 0 the two produce equal bytes (asserted).
  vanishing   2^22 values, n = 2^18: lcpcq_divide_vanishing_device next to the same LCPCQ_MUL.
  chain       two columns on H_n, n = 2^20: lde to g H_m, m = 2^22 -> a * b pointwise -> division by X^n - 1 -> commit from coset
              values; next to the same chain with the division on the host (download, lcpcq_divide_vanishing, upload).  Equal roots
              asserted.
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=7)
ap.add_argument("--host-reps", type=int, default=3)
ap.add_argument("--fields", default="3,0")
ap.add_argument("--sizes", default="20,22,24,26")
ap.add_argument("--host-max", type=int, default=22)
ap.add_argument("--tag", default="")
args = ap.parse_args()


def emit(d):
    d["tag"] = args.tag
    print(json.dumps(d), flush=True)


def spread(ts):
    return {"median": round(statistics.median(ts), 3), "min": round(min(ts), 3), "max": round(max(ts), 3)}


import numpy as np
import torch

import lcpc_amd
from lcpc_amd import LcCommit, LigeroEncoding

if not torch.cuda.is_available():
    sys.exit("bench_quot: no GPU")
DEV = "cuda:0"


def alternate(variants, reps):
    """variants: [(name, fn)]; every round runs each once, the order reversed every other round; two warm rounds.  ms per name"""
    ts = {name: [] for name, _ in variants}
    for i in range(reps + 2):
        for name, fn in (variants if i % 2 == 0 else variants[::-1]):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            dt = (time.perf_counter() - t0) * 1e3
            if i >= 2:
                ts[name].append(dt)
    return ts


def timed(fn, reps):
    return alternate([("x", fn)], reps)["x"]


def to_host(t):
    return t.cpu().numpy().view(np.uint64)


def to_dev(a):
    return torch.from_numpy(a.view(np.int64)).to(DEV)


def ratios(d, ts, over):
    for name in ts:
        if name != over:
            d["%s_over_%s" % (name, over)] = round(statistics.median(ts[name]) / statistics.median(ts[over]), 3)


for fid in (int(v) for v in args.fields.split(",") if v):
    enc = LigeroEncoding.new_from_dims(fid, 64, 128)
    L = enc.L
    gen = lcpc_amd.generator(fid)
    for log_n in (int(v) for v in args.sizes.split(",") if v):
        n = 1 << log_n
        x = enc.random_coeffs_device(n, seed=3)
        a = enc.random_coeffs_device(n, seed=4)
        out = torch.empty_like(x)
        d = {"leg": "inverse", "field": fid, "log_n": log_n, "bytes": n * 8 * L, "reps": args.reps}
        variants = [("inverse", lambda: enc.batch_inverse(x, out=out)), ("mul", lambda: enc.pointwise("mul", a, x, out=out)),
                    ("div", lambda: enc.pointwise("div", a, x, out=out))]
        if log_n <= args.host_max:
            def host_route():
                return to_dev(lcpc_amd.batch_inverse(fid, to_host(x)))
            enc.batch_inverse(x, out=out)
            assert torch.equal(out, host_route()), "the device and the host route disagree"
            d["equal_bytes"] = True
            d["host_route_ms"] = spread(timed(host_route, args.host_reps))
        ts = alternate(variants, args.reps)
        for name, v in ts.items():
            d[name + "_ms"] = spread(v)
        ratios(d, ts, "mul")
        if "host_route_ms" in d:
            d["host_route_over_inverse"] = round(d["host_route_ms"]["median"] / statistics.median(ts["inverse"]), 1)
        d["inverse_gelem_s"] = round(n / statistics.median(ts["inverse"]) / 1e6, 3)
        emit(d)
        del x, a, out
        torch.cuda.empty_cache()

    log_m, log_v = 22, 18
    m = 1 << log_m
    z = enc.from_ints([12345])[0].copy()
    for n_vecs in (1, 8):
        vals = enc.random_coeffs_device(n_vecs * m, seed=5).view(n_vecs, m, L)
        out = torch.empty_like(vals)
        y = torch.zeros((n_vecs, L), dtype=torch.int64, device=DEV)
        # the precomputed vector: 1 / (g w^k - z) by the division of a column of ones, tiled over the vectors
        ones = to_dev(np.tile(enc.from_ints([1]), (m, 1)))
        inv_lin = enc.divide_linear(ones, gen, z, y[:1]).repeat(n_vecs, 1).view(n_vecs, m, L).contiguous()
        inv_van = enc.divide_vanishing(ones, gen, log_v).repeat(n_vecs, 1).view(n_vecs, m, L).contiguous()
        del ones
        chk = enc.pointwise("mul", vals, inv_lin)
        assert torch.equal(enc.divide_linear(vals, gen, z, y), chk), "divide_linear and the multiply by the precomputed vector disagree"
        chk = enc.pointwise("mul", vals, inv_van)
        assert torch.equal(enc.divide_vanishing(vals, gen, log_v), chk)
        del chk
        ts = alternate([("divide_linear", lambda: enc.divide_linear(vals, gen, z, y, out=out)),
                        ("divide_vanishing", lambda: enc.divide_vanishing(vals, gen, log_v, out=out)),
                        ("mul", lambda: enc.pointwise("mul", vals, inv_lin, out=out))], args.reps)
        d = {"leg": "divide", "field": fid, "log_m": log_m, "log_n": log_v, "n_vecs": n_vecs, "bytes": n_vecs * m * 8 * L, "reps": args.reps,
             "equal_bytes": True}
        for name, v in ts.items():
            d[name + "_ms"] = spread(v)
        ratios(d, ts, "mul")
        emit(d)
        del vals, out, inv_lin, inv_van
        torch.cuda.empty_cache()

    log_n, log_m = 20, 22
    cols = enc.random_coeffs_device(2 << log_n, seed=6).view(2, 1 << log_n, L)
    enc2 = LigeroEncoding.new(fid, 1 << log_m)
    cm = LcCommit(enc2)

    def chain(host):
        ext, _ = enc2.lde(cols, log_m, gen)
        num = enc2.pointwise("mul", ext[0], ext[1])
        if host:
            q = to_dev(lcpc_amd.divide_vanishing(fid, to_host(num), gen, log_n))
        else:
            q = enc2.divide_vanishing(num, gen, log_n, out=num)
        return LcCommit.commit_coset_evals(q, gen, enc2, into=cm).get_root()

    assert chain(False) == chain(True), "the device chain and the chain with the host division disagree"
    d = {"leg": "chain", "field": fid, "log_n": log_n, "log_m": log_m, "reps": args.reps, "equal_roots": True}
    d["device_ms"] = spread(timed(lambda: chain(False), args.reps))
    d["host_division_ms"] = spread(timed(lambda: chain(True), args.host_reps))
    d["host_over_device"] = round(d["host_division_ms"]["median"] / d["device_ms"]["median"], 1)
    emit(d)
    del cols, cm, enc2, enc
    torch.cuda.empty_cache()

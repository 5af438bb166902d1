#!/usr/bin/env python3
"""tools/bench_scan.py -- prefix sums and products (include/lcpc_hip_scan.h) on one box, in one process, the variants alternated call
by call.  One JSON line per leg with the median and the spread (min, max) of every side; kept under profiles/r20_scan.jsonl.  Wall
clock around the calls and a synchronisation.

  python tools/bench_scan.py [--reps 7] [--host-reps 3] [--fields 3,0] [--sizes 20,24,26] [--host-max 24] [--tag TAG]

  scan     per field and log2 n: lcpcs_scan_device, product and sum (exclusive; the inclusive form runs the same instructions), next
           to lcpcq_pointwise_device LCPCQ_MUL resp. LCPCQ_ADD of the same length -- the one-pass yardstick: two reads and one write
           against the scan's two reads, one write and three operations per element; up to --host-max also the route without the
           extension: download, lcpcs_scan on one host thread, upload.  The two routes must have produced equal bytes (asserted)
           before anything is timed.
  ratio    lcpcs_scan_ratio_device (product, exclusive: the permutation accumulator) next to lcpcq_pointwise_device LCPCQ_DIV alone
           and to the scan alone: the ratio form is the two one after the other.

  python tools/bench_scan.py --trace-run [--fields 3] [--sizes 24]
           what a kernel trace wraps (rocprofv3 --kernel-trace -- python tools/bench_scan.py --trace-run, read with
           tools/rocpd_dispatches.py): three product scans, three sums and a LCPCQ_MUL / LCPCQ_ADD each, nothing timed -- the share
           of K17a, K17b and K17c in a call.
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
ap.add_argument("--sizes", default="20,24,26")
ap.add_argument("--host-max", type=int, default=24)
ap.add_argument("--tag", default="")
ap.add_argument("--trace-run", action="store_true")
args = ap.parse_args()


def emit(d):
    d["tag"] = args.tag
    print(json.dumps(d), flush=True)


def spread(ts):
    return {"median": round(statistics.median(ts), 3), "min": round(min(ts), 3), "max": round(max(ts), 3)}


import numpy as np
import torch

import lcpc_amd
from lcpc_amd import LigeroEncoding

if not torch.cuda.is_available():
    sys.exit("bench_scan: no GPU")
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


def to_host(t):
    return t.cpu().numpy().view(np.uint64)


def to_dev(a):
    return torch.from_numpy(a.view(np.int64)).to(DEV)


def over(d, ts, name, base):
    d["%s_over_%s" % (name, base)] = round(statistics.median(ts[name]) / statistics.median(ts[base]), 3)


for fid in (int(v) for v in args.fields.split(",") if v):
    enc = LigeroEncoding.new_from_dims(fid, 64, 128)
    L = enc.L
    for log_n in (int(v) for v in args.sizes.split(",") if v):
        n = 1 << log_n
        x = enc.random_coeffs_device(n, seed=3)
        a = enc.random_coeffs_device(n, seed=4)
        out = torch.empty_like(x)
        total = torch.empty((1, L), dtype=torch.int64, device=DEV)
        if args.trace_run:
            for _ in range(3):
                enc.scan(x, "product", exclusive=True, out=out, total=total)
                enc.pointwise("mul", a, x, out=out)
                enc.scan(x, "sum", exclusive=True, out=out, total=total)
                enc.pointwise("add", a, x, out=out)
            torch.cuda.synchronize()
            continue
        d = {"leg": "scan", "field": fid, "log_n": log_n, "bytes": n * 8 * L, "reps": args.reps}
        if log_n <= args.host_max:
            for op in ("product", "sum"):
                def host_route():
                    o, t = lcpc_amd.scan(fid, to_host(x), op, exclusive=True)
                    return to_dev(o), to_dev(t.reshape(1, L))
                enc.scan(x, op, exclusive=True, out=out, total=total)
                want, wtot = host_route()
                assert torch.equal(out, want) and torch.equal(total, wtot), "the device and the host route disagree"
                d["host_route_%s_ms" % op] = spread(alternate([("x", host_route)], args.host_reps)["x"])
            d["equal_bytes"] = True
        ts = alternate([("product", lambda: enc.scan(x, "product", exclusive=True, out=out, total=total)),
                        ("mul", lambda: enc.pointwise("mul", a, x, out=out)),
                        ("sum", lambda: enc.scan(x, "sum", exclusive=True, out=out, total=total)),
                        ("add", lambda: enc.pointwise("add", a, x, out=out))], args.reps)
        for name, v in ts.items():
            d[name + "_ms"] = spread(v)
        over(d, ts, "product", "mul")
        over(d, ts, "sum", "add")
        for op in ("product", "sum"):
            if "host_route_%s_ms" % op in d:
                d["host_route_over_%s" % op] = round(d["host_route_%s_ms" % op]["median"] / statistics.median(ts[op]), 1)
            d["%s_gelem_s" % op] = round(n / statistics.median(ts[op]) / 1e6, 3)
        emit(d)

        ts = alternate([("scan_ratio", lambda: enc.scan_ratio(a, x, "product", exclusive=True, out=out, total=total)),
                        ("div", lambda: enc.pointwise("div", a, x, out=out)),
                        ("product", lambda: enc.scan(x, "product", exclusive=True, out=out, total=total))], args.reps)
        d = {"leg": "ratio", "field": fid, "log_n": log_n, "bytes": n * 8 * L, "reps": args.reps}
        for name, v in ts.items():
            d[name + "_ms"] = spread(v)
        over(d, ts, "scan_ratio", "div")
        d["scan_ratio_over_div_plus_product"] = round(statistics.median(ts["scan_ratio"]) / (statistics.median(ts["div"]) + statistics.median(ts["product"])), 3)
        emit(d)
        del x, a, out
        torch.cuda.empty_cache()
    del enc

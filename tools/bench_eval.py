#!/usr/bin/env python3
"""tools/bench_eval.py -- p(z) on the device (include/lcpc_hip_eval.h) against the route a caller had to take before it, on one box,
in one process, the variants alternated call by call.  One JSON line per shape and point count with the median and the spread
(min, max) of every side; kept under profiles/r16_eval.jsonl.

  python tools/bench_eval.py [--reps 7] [--shapes 3:26,3:20,3:16] [--points 1,2,8,32] [--tag TAG]

Per shape (field : log2 n, Ligero) and n_points, on ONE commitment and the same points:
  eval            lcpce_eval: points in host memory, values in host memory.  Wall clock around the call, complete on return.
  eval_device     lcpce_eval_device: points and values in HBM.  Wall clock around the call and a synchronisation.
  collapse_device lcpc_collapse_device of n_points ready-made outer tensors, the same way: what eval_device adds to it are K10's
                  two steps in front and K11 behind.
  today           host powers (Python ints, a chain of multiplications by x, turned into Montgomery limbs by lcpci_from_ints), the
                  core host collapse from host memory, and the dot product of the collapsed polynomial with the inner tensor on the host:
                  canonical values by lcpci_to_canon, then numpy's dot over object arrays of Python ints and one reduction mod p
                  -- the product has no host field arithmetic a caller can reach, so this is what a Python caller writes.
                  --today-reps rounds; skipped where n_points * n_per_row > --today-max (it is linear in the points).
  time per call and per point; the values of all routes are compared before anything is timed.

  python tools/bench_eval.py --trace-run [--shapes 3:26] [--points 1]
           what a kernel trace wraps (rocprofv3 --kernel-trace --stats -- python tools/bench_eval.py --trace-run): a few
           lcpce_eval_device calls, nothing timed.
  python tools/bench_eval.py --kernel-stats FILE.csv
           the trace's kernel_stats.csv -> one line: the share of K10 (pairs, expansion), the collapse (to_r29, collapse, split sum)
           and K11 in the evaluation's kernel time.
"""
import argparse
import csv
import ctypes as C
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=7)
ap.add_argument("--today-reps", type=int, default=3)
ap.add_argument("--today-max", type=int, default=1 << 21)
ap.add_argument("--shapes", default="3:26,3:20,3:16")
ap.add_argument("--points", default="1,2,8,32")
ap.add_argument("--tag", default="")
ap.add_argument("--trace-run", action="store_true")
ap.add_argument("--kernel-stats", default="")
args = ap.parse_args()


def emit(d):
    d["tag"] = args.tag
    print(json.dumps(d), flush=True)


def spread(ts):
    return {"median": round(statistics.median(ts), 3), "min": round(min(ts), 3), "max": round(max(ts), 3)}


GROUPS = (("K10", ("eval_pairs_kernel", "eval_expand_kernel")), ("collapse", ("collapse_kernel", "collapse29_kernel", "to_r29_kernel", "field_sum_kernel")),
          ("K11", ("field_dot_kernel",)))

if args.kernel_stats:
    tot = {g: 0.0 for g, _ in GROUPS}
    per = {}
    for row in csv.DictReader(open(args.kernel_stats)):
        name = row.get("Name", "")
        for g, names in GROUPS:
            for k in names:
                if k + "<" in name or name.startswith(k) or (" " + k) in name:
                    ns = float(row["TotalDurationNs"])
                    tot[g] += ns
                    per[k] = {"calls": int(row["Calls"]), "avg_us": round(float(row["AverageNs"]) / 1e3, 2)}
    s = sum(tot.values()) or 1.0
    emit({"leg": "kernel trace", "share": {g: round(v / s, 4) for g, v in tot.items()}, "total_us": {g: round(v / 1e3, 1) for g, v in tot.items()},
          "kernels": per})
    sys.exit(0)

import torch

import lcpc_amd
from lcpc_amd import LcCommit, LigeroEncoding, _lib

if not torch.cuda.is_available():
    sys.exit("bench_eval: no GPU (there is no CPU path to measure)")
DEV = "cuda:0"
lib = _lib.lib()
POINTS = [int(v) for v in args.points.split(",")]


def to_dev(a):
    return torch.from_numpy(np.ascontiguousarray(a, np.uint64).view(np.int64)).to(DEV)


def alternate(variants, reps):
    """variants: [(name, fn)]; every round runs each once, the order reversed every other round; two warm rounds.  ms per name"""
    ts = {name: [] for name, _ in variants}
    for i in range(reps + 2):
        for name, fn in (variants if i % 2 == 0 else variants[::-1]):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            dt = (time.perf_counter() - t0) * 1e3
            if i >= 2:
                ts[name].append(dt)
    return ts


for shape in args.shapes.split(","):
    fid, log2 = (int(v) for v in shape.split(":"))
    n = 1 << log2
    enc = LigeroEncoding.new(fid, n)
    L, p = enc.L, lcpc_amd.FIELD_MODULUS[fid]
    coeffs = enc.random_coeffs_device(n, seed=1)
    cm = LcCommit.commit_device(coeffs.data_ptr(), n, enc)
    del coeffs
    n_rows, n_per_row = cm.n_rows, cm.n_per_row
    rng = np.random.default_rng(5)
    xs_int = [int.from_bytes(rng.bytes(8 * L), "little") % p for _ in range(max(POINTS))]
    xs = enc.from_ints(xs_int)
    base = {"shape": shape, "n": n, "field": fid, "n_rows": n_rows, "n_per_row": n_per_row, "reps": args.reps}

    def today(k):
        """the values at xs[:k] without this extension"""
        outer, inner = [], []
        for x in xs_int[:k]:
            y, cur, row = pow(x, n_per_row, p), 1, []
            for _ in range(n_per_row):
                row.append(cur)
                cur = cur * x % p
            inner.append(row)
            cur, col = 1, []
            for _ in range(n_rows):
                col.append(cur)
                cur = cur * y % p
            outer.append(col)
        polys = cm.eval_outer(np.stack([enc.from_ints(o) for o in outer]))
        out = []
        for t in range(k):
            canon = np.array(enc.to_ints(polys[t]), dtype=object)
            out.append(int(np.dot(canon, np.array(inner[t], dtype=object))) % p)
        return enc.from_ints(out)

    for k in POINTS:
        pts = np.ascontiguousarray(xs[:k])
        d_pts = to_dev(pts)
        d_ev = torch.empty((k, L), dtype=torch.int64, device=DEV)
        d_outer = torch.empty((k, n_rows, L), dtype=torch.int64, device=DEV)
        d_polys = torch.empty((k, n_per_row, L), dtype=torch.int64, device=DEV)
        assert lib.lcpce_tensors_device(enc._h, 0, C.c_void_p(d_pts.data_ptr()), 1, k, n_rows, n_per_row, C.c_void_p(d_outer.data_ptr()), None, None) == 0
        ev = np.zeros((k, L), np.uint64)

        def eval_host():
            assert lib.lcpce_eval(cm._h, 0, pts.ctypes.data_as(C.c_void_p), 1, k, ev.ctypes.data_as(C.c_void_p)) == 0

        def eval_device():
            assert lib.lcpce_eval_device(cm._h, 0, C.c_void_p(d_pts.data_ptr()), 1, k, None, C.c_void_p(d_ev.data_ptr())) == 0
            torch.cuda.synchronize()

        def collapse_device():
            assert lib.lcpc_collapse_device(cm._h, C.c_void_p(d_outer.data_ptr()), k, None, C.c_void_p(d_polys.data_ptr())) == 0
            torch.cuda.synchronize()

        if args.trace_run:
            for _ in range(5):
                eval_device()
            continue
        eval_host()
        eval_device()
        assert np.array_equal(d_ev.cpu().numpy().view(np.uint64), ev)
        do_today = k * n_per_row <= args.today_max
        if do_today:
            assert np.array_equal(today(k), ev), "the routes disagree"
        ts = alternate([("eval", eval_host), ("eval_device", eval_device), ("collapse_device", collapse_device)], args.reps)
        d = dict(base, leg="eval", n_points=k)
        for name, v in ts.items():
            d[name + "_ms"] = spread(v)
            d[name + "_ms_per_point"] = round(statistics.median(v) / k, 4)
        if do_today:
            tt = alternate([("today", lambda: today(k))], args.today_reps)["today"]
            d["today_ms"] = spread(tt)
            d["today_ms_per_point"] = round(statistics.median(tt) / k, 3)
        emit(d)
        del d_pts, d_ev, d_outer, d_polys
    del cm, enc
    torch.cuda.empty_cache()

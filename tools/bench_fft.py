#!/usr/bin/env python3
"""tools/bench_fft.py -- the whole-vector transform and the commit from evaluations (include/lcpc_hip_fft.h) on one box, in one
process, the variants alternated call by call.  One JSON line per leg with the median and the spread (min, max) of every side; kept
under profiles/r17_fft.jsonl.

  python tools/bench_fft.py [--reps 7] [--fields 3,0] [--sizes 16,20,24,26] [--commit 3:26] [--host 3:20] [--tag TAG]

  transform   per field and log2 n: lcpcf_fft_device in place, FFT_IO / IFFT_OI / FFT_II / IFFT_II alternated.  Wall clock around
              the call and a synchronisation.  Beside the time, the bytes per second against the floor of the form's own pass
              count, passes x 2 x n x 8 L bytes (the II forms count their permutation as a pass).
  commit      --commit field:log2n: lcpcf_commit_evals_device (natural and bit-reversed evaluations) next to lcpc_commit_device on
              the same object, alternated; the ratio of the medians is the number to write down.
  host        --host field:log2n: lcpcf_fft on the host, FFT_IO, a few rounds: the route without the device transform.

  python tools/bench_fft.py --trace-run [--fields 3] [--sizes 26]
           what a kernel trace wraps (rocprofv3 --kernel-trace --stats -- python tools/bench_fft.py --trace-run): a few in-place
           IFFT_II calls, nothing timed.
"""
import argparse
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
ap.add_argument("--fields", default="3,0")
ap.add_argument("--sizes", default="16,20,24,26")
ap.add_argument("--commit", default="3:26")
ap.add_argument("--host", default="3:20")
ap.add_argument("--host-reps", type=int, default=3)
ap.add_argument("--tag", default="")
ap.add_argument("--trace-run", action="store_true")
args = ap.parse_args()


def emit(d):
    d["tag"] = args.tag
    print(json.dumps(d), flush=True)


def spread(ts):
    return {"median": round(statistics.median(ts), 3), "min": round(min(ts), 3), "max": round(max(ts), 3)}


import torch

import lcpc_amd
from lcpc_amd import LcCommit, LigeroEncoding, _lib

if not torch.cuda.is_available():
    sys.exit("bench_fft: no GPU (the host leg alone is lcpc_amd.fft under a timer)")
DEV = "cuda:0"
lib = _lib.lib()
LOG_TILE = 10                       # FFT_MAX_LOG_TILE (lcpc_amd/csrc/kernels.h)


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


def passes(form, log_n):
    return -(-log_n // LOG_TILE) + (1 if form.endswith("_ii") else 0)


FORMS = ("fft_io", "ifft_oi", "fft_ii", "ifft_ii")
for fid in (int(v) for v in args.fields.split(",") if v):
    enc = LigeroEncoding.new_from_dims(fid, 64, 128)
    for log_n in (int(v) for v in args.sizes.split(",") if v):
        n = 1 << log_n
        buf = enc.random_coeffs_device(n, seed=3)

        def run(form):
            assert lib.lcpcf_fft_device(enc._h, _lib.FFT_FORMS[form], C.c_void_p(buf.data_ptr()), C.c_void_p(buf.data_ptr()), log_n, 1, None) == 0
            torch.cuda.synchronize()

        if args.trace_run:
            for _ in range(5):
                run("ifft_ii")
            continue
        ts = alternate([(f, (lambda f=f: run(f))) for f in FORMS], args.reps)
        d = {"leg": "transform", "field": fid, "log_n": log_n, "bytes": n * 8 * enc.L, "reps": args.reps}
        for f, v in ts.items():
            floor = passes(f, log_n) * 2 * n * 8 * enc.L
            d[f + "_ms"] = spread(v)
            d[f + "_passes"] = passes(f, log_n)
            d[f + "_gbps_of_floor"] = round(floor / (statistics.median(v) * 1e-3) / 1e9, 1)
        emit(d)
        del buf
        torch.cuda.empty_cache()
    del enc

if args.commit and not args.trace_run:
    fid, log_n = (int(v) for v in args.commit.split(":"))
    n = 1 << log_n
    enc = LigeroEncoding.new(fid, n)
    src = enc.random_coeffs_device(n, seed=1)
    cm = LcCommit(enc)
    root = (C.c_uint8 * enc.digest_len)()

    def commit_coeffs():
        assert lib.lcpc_commit_device(cm._h, C.c_void_p(src.data_ptr()), n, None, 0, root) == 0

    def commit_evals(order):
        assert lib.lcpcf_commit_evals_device(cm._h, order, C.c_void_p(src.data_ptr()), log_n, None, root) == 0

    ts = alternate([("commit_device", commit_coeffs), ("commit_evals_natural", lambda: commit_evals(0)), ("commit_evals_bitrev", lambda: commit_evals(1))],
                   args.reps)
    d = {"leg": "commit", "field": fid, "log_n": log_n, "reps": args.reps}
    for name, v in ts.items():
        d[name + "_ms"] = spread(v)
    for name in ("commit_evals_natural", "commit_evals_bitrev"):
        d[name + "_over_commit_device"] = round(statistics.median(ts[name]) / statistics.median(ts["commit_device"]), 3)
    emit(d)
    del cm, src, enc
    torch.cuda.empty_cache()

if args.host and not args.trace_run:
    fid, log_n = (int(v) for v in args.host.split(":"))
    L = lcpc_amd.FIELD_LIMBS[fid]
    enc = LigeroEncoding.new_from_dims(fid, 64, 128)
    x = enc.random_coeffs_device(1 << log_n, seed=2).cpu().numpy().view(np.uint64).reshape(-1, L)
    ts = []
    for _ in range(args.host_reps):
        t0 = time.perf_counter()
        lcpc_amd.fft(fid, x, "fft_io")
        ts.append((time.perf_counter() - t0) * 1e3)
    emit({"leg": "host", "field": fid, "log_n": log_n, "fft_io_ms": spread(ts), "reps": args.host_reps})

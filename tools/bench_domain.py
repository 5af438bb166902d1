#!/usr/bin/env python3
"""tools/bench_domain.py -- the low-degree extension and the commit from coset values (include/lcpc_hip_domain.h) on one box, in one
process, the variants alternated call by call.  One JSON line per leg with the median and the spread (min, max) of every side; kept
under profiles/r18_domain.jsonl.

  python tools/bench_domain.py [--reps 7] [--fields 3,0] [--sizes 16:18,20:22,22:26,24:26] [--commit 3:26] [--tag TAG]

  lde         per field and log2 n : log2 m, values on H_n -> values on s H_m, bit-reversed out, three variants alternated:
                lde_one    lcpcd_lde_device, shift_in = NULL, shift_out = 1
                three_step lcpcf_fft_device IFFT_II(n) -> hipMemsetAsync of m elements + copy of n -> lcpcf_fft_device FFT_IO(m): the
                           route without the extension; it cannot apply a shift
                lde_gen    lcpcd_lde_device with shift_out = the generator: the cost of the fused scale is lde_gen - lde_one
              Before anything is timed lde_one and three_step must have produced equal bytes (asserted).  Wall clock around the
              calls and a synchronisation.  three_over_lde is the ratio of the medians.
  commit      --commit field:log2n: lcpcd_commit_coset_evals_device next to lcpcf_commit_evals_device and lcpc_commit_device on one
              object, the three alternated.
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

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=7)
ap.add_argument("--fields", default="3,0")
ap.add_argument("--sizes", default="16:18,20:22,22:26,24:26")
ap.add_argument("--commit", default="3:26")
ap.add_argument("--tag", default="")
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
    sys.exit("bench_domain: no GPU")
DEV = "cuda:0"
lib = _lib.lib()
vp = lambda a: a.ctypes.data_as(C.c_void_p)
dp = lambda t: C.c_void_p(t.data_ptr())


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


for fid in (int(v) for v in args.fields.split(",") if v):
    enc = LigeroEncoding.new_from_dims(fid, 64, 128)
    L = enc.L
    gen = lcpc_amd.generator(fid)
    one = enc.from_ints([1])[0].copy()                           # the shift 1 in Montgomery limbs
    for pair in (v for v in args.sizes.split(",") if v):
        log_n, log_m = (int(v) for v in pair.split(":"))
        n, m = 1 << log_n, 1 << log_m
        src = enc.random_coeffs_device(n, seed=3)                # the values on H_n, natural order
        work = torch.empty_like(src)
        out = torch.empty((m, L), dtype=torch.int64, device=DEV)
        pad = torch.empty((m, L), dtype=torch.int64, device=DEV)

        def lde(shift):
            assert lib.lcpcd_lde_device(enc._h, 0, None, dp(src), log_n, vp(shift), log_m, 1, dp(out), dp(work), 1, None) == 0
            torch.cuda.synchronize()

        def three_step():
            assert lib.lcpcf_fft_device(enc._h, _lib.FFT_FORMS["ifft_ii"], dp(src), dp(work), log_n, 1, None) == 0
            pad.zero_()                                          # (hipMemsetAsync on the same stream)
            pad[:n].copy_(work)
            assert lib.lcpcf_fft_device(enc._h, _lib.FFT_FORMS["fft_io"], dp(pad), dp(pad), log_m, 1, None) == 0
            torch.cuda.synchronize()

        lde(one)
        three_step()
        assert torch.equal(out, pad), "the extension and the three-step route disagree"
        ts = alternate([("lde_one", lambda: lde(one)), ("three_step", three_step), ("lde_gen", lambda: lde(gen))], args.reps)
        d = {"leg": "lde", "field": fid, "log_n": log_n, "log_m": log_m, "out_bytes": m * 8 * L, "reps": args.reps, "equal_bytes": True}
        for name, v in ts.items():
            d[name + "_ms"] = spread(v)
        d["three_over_lde"] = round(statistics.median(ts["three_step"]) / statistics.median(ts["lde_one"]), 3)
        d["gen_over_one"] = round(statistics.median(ts["lde_gen"]) / statistics.median(ts["lde_one"]), 3)
        emit(d)
        del src, work, out, pad
        torch.cuda.empty_cache()
    del enc

if args.commit:
    fid, log_n = (int(v) for v in args.commit.split(":"))
    n = 1 << log_n
    enc = LigeroEncoding.new(fid, n)
    gen = lcpc_amd.generator(fid)
    src = enc.random_coeffs_device(n, seed=1)
    cm = LcCommit(enc)
    root = (C.c_uint8 * enc.digest_len)()

    def commit_coeffs():
        assert lib.lcpc_commit_device(cm._h, dp(src), n, None, 0, root) == 0

    def commit_evals():
        assert lib.lcpcf_commit_evals_device(cm._h, 0, dp(src), log_n, None, root) == 0

    def commit_coset():
        assert lib.lcpcd_commit_coset_evals_device(cm._h, 0, vp(gen), dp(src), log_n, None, root) == 0

    ts = alternate([("commit_device", commit_coeffs), ("commit_evals", commit_evals), ("commit_coset_evals", commit_coset)], args.reps)
    d = {"leg": "commit", "field": fid, "log_n": log_n, "reps": args.reps}
    for name, v in ts.items():
        d[name + "_ms"] = spread(v)
    for name in ("commit_evals", "commit_coset_evals"):
        d[name + "_over_commit_device"] = round(statistics.median(ts[name]) / statistics.median(ts["commit_device"]), 3)
    emit(d)

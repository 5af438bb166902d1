#!/usr/bin/env python3
"""tools/bench_ints.py -- commit from plain integers (include/lcpc_hip_ints.h) against the commit from stored Montgomery limbs, on
one box, in one process, the variants alternated call by call.  One JSON line per leg with the median and the spread (min, max) of
every side; kept under profiles/r15_ints.jsonl.

  python tools/bench_ints.py [--reps 7] [--shapes ligero:3:26,ligero:3:24,ligero:1:24,brakedown:3:24] [--tag TAG]

Per shape (encoder : field : log2 n) and kind (u32, u64, wide):
  host     lcpc_commit of the Montgomery limbs from pinned memory (the baseline: this entry point is what it was) | lcpci_commit_ints
           from pinned memory | lcpci_commit_ints from pageable memory.  Wall clock around the call, which is complete on return.
  device   owning lcpc_commit_device | lcpci_commit_ints_device.  Wall clock around the call with a root (it synchronises).
  kernel   the widening kernel alone (lcpci_from_ints_device): device events around --kernel-launches back-to-back launches, and the
           achieved GB/s over n * (kind bytes + 8 L).

  python tools/bench_ints.py --kernel-run [--log2 24]
           what a kernel trace wraps (rocprofv3 --kernel-trace --stats -- python tools/bench_ints.py --kernel-run): per field the
           widening kernel for every kind and to_mont_kernel through the k5 harness (tests/k5_harness.py) at the same n, a few
           launches each; nothing is timed here.
  python tools/bench_ints.py --kernel-stats FILE.csv [--log2 24]
           the trace's kernel_stats.csv -> one line per kernel: average time and GB/s over the bytes it moves at that n.
"""
import argparse
import csv
import ctypes as C
import json
import os
import re
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np

KIND_BYTES = {"u32": 4, "u64": 8}
FIELD_L = (1, 2, 3, 4)

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=7)
ap.add_argument("--shapes", default="ligero:3:26,ligero:3:24,ligero:1:24,brakedown:3:24")
ap.add_argument("--kinds", default="u32,u64,wide")
ap.add_argument("--kernel-launches", type=int, default=20)
ap.add_argument("--tag", default="")
ap.add_argument("--kernel-run", action="store_true")
ap.add_argument("--kernel-stats", default="")
ap.add_argument("--log2", type=int, default=24)
args = ap.parse_args()


def emit(d):
    d["tag"] = args.tag
    print(json.dumps(d), flush=True)


def kind_bytes(kind, L):
    return KIND_BYTES.get(kind, 8 * L)


def spread(ts):
    return {"median": round(statistics.median(ts), 3), "min": round(min(ts), 3), "max": round(max(ts), 3)}


if args.kernel_stats:
    n = 1 << args.log2
    for row in csv.DictReader(open(args.kernel_stats)):
        name = row.get("Name", "")
        if "from_ints_kernel" not in name and "to_mont_kernel" not in name:
            continue
        avg_ns = float(row["AverageNs"])
        d = {"leg": "kernel trace", "kernel": name, "calls": int(row["Calls"]), "avg_us": round(avg_ns / 1e3, 2), "log2": args.log2}
        m = re.search(r"from_ints_kernel<(\d+), (\d+)>", name)
        if m:                                                   # <NL, KIND>: reads the kind's bytes, writes 4 NL
            nl, k = int(m.group(1)), int(m.group(2))
            d["bytes"] = n * ((4 if k < 2 else 8 if k < 4 else 4 * nl) + 4 * nl)
        m = re.search(r"to_mont_kernel<(\d+)>", name)
        if m:                                                   # reads and writes 4 NL
            d["bytes"] = n * 8 * int(m.group(1))
        if "bytes" in d:
            d["GBps"] = round(d["bytes"] / avg_ns, 1)
        emit(d)
    sys.exit(0)

import torch

import lcpc_amd
from lcpc_amd import LcCommit, LigeroEncoding, SdigEncoding, _lib

if not torch.cuda.is_available():
    sys.exit("bench_ints: no GPU (there is no CPU path to measure)")

if args.kernel_run:
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    sys.path.insert(0, os.path.join(ROOT, "oracle"))
    import k5_harness as K5
    n = 1 << args.log2
    rng = np.random.default_rng(3)
    for fid in range(4):
        L = FIELD_L[fid]
        enc = LigeroEncoding.new_from_dims(fid, 64, 128)
        out = torch.empty((n, L), dtype=torch.int64, device="cuda:0")
        wide = rng.integers(0, 1 << 62, size=(n, L), dtype=np.uint64)
        for kind in args.kinds.split(","):
            src = wide if kind == "wide" else rng.integers(0, 1 << 31, size=n, dtype=np.uint32 if kind == "u32" else np.uint64)
            d = torch.from_numpy(src.view(np.int32 if kind == "u32" else np.int64)).cuda()
            for _ in range(5):
                assert _lib.lib().lcpci_from_ints_device(enc._h, _lib.INTS_KINDS[kind], C.c_void_p(d.data_ptr()), n, C.c_void_p(out.data_ptr()), None) == 0
            torch.cuda.synchronize()
        # to_mont_kernel: the k5 harness uploads, launches and downloads; the trace holds the launch
        hout = np.zeros((n, L), np.uint64)
        r2 = K5.r2_limbs(fid)
        for _ in range(3):
            rc = K5.lib().k5h_convert(K5.NL[fid], 1, wide.ctypes.data_as(C.c_void_p), n, r2.ctypes.data_as(C.c_void_p),
                                      hout.ctypes.data_as(C.c_void_p), n, 0)
            assert rc == 0, rc
    sys.exit(0)


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
    enc_name, fid, log2 = shape.split(":")
    fid, n = int(fid), 1 << int(log2)
    L = FIELD_L[fid]
    enc = LigeroEncoding.new(fid, n) if enc_name == "ligero" else SdigEncoding.new(fid, n, 0)
    rng = np.random.default_rng(1)
    # (n, L) limbs below 2^62: stored elements < p for the baseline, and as good a WIDE integer as any
    limbs_pin = torch.from_numpy(rng.integers(0, 1 << 62, size=(n, L), dtype=np.uint64).view(np.int64)).pin_memory()
    limbs = limbs_pin.numpy().view(np.uint64)
    limbs_dev = limbs_pin.cuda()
    cm_base, cm_ints = LcCommit(enc), LcCommit(enc)
    base = {"shape": shape, "n": n, "field": fid, "encoder": enc_name, "reps": args.reps}
    for kind in args.kinds.split(","):
        if kind == "wide":
            pin_t, pin = limbs_pin, limbs
        else:
            dt = np.uint32 if kind == "u32" else np.uint64
            pin_t = torch.from_numpy(rng.integers(0, np.iinfo(dt).max, size=n, dtype=dt).view(np.int32 if kind == "u32" else np.int64)).pin_memory()
            pin = pin_t.numpy().view(dt)
        page = np.empty_like(pin)
        np.copyto(page, pin)                                   # pageable: numpy's allocator
        dev = pin_t.cuda()
        kb = kind_bytes(kind, L)
        # host
        ts = alternate([("lcpc_commit_pinned", lambda: LcCommit.commit(limbs, enc, into=cm_base)),
                        ("commit_ints_pinned", lambda: LcCommit.commit_ints(pin, enc, kind=kind, into=cm_ints)),
                        ("commit_ints_pageable", lambda: LcCommit.commit_ints(page, enc, kind=kind, into=cm_ints))], args.reps)
        d = dict(base, leg="host", kind=kind, bus_bytes={"limbs": n * 8 * L, "ints": n * kb})
        d.update({k + "_ms": spread(v) for k, v in ts.items()})
        emit(d)
        # device
        ts = alternate([("lcpc_commit_device", lambda: LcCommit.commit_device(limbs_dev.data_ptr(), n, enc, into=cm_base)),
                        ("commit_ints_device", lambda: LcCommit.commit_ints(dev, enc, kind=kind, into=cm_ints))], args.reps)
        d = dict(base, leg="device", kind=kind)
        d.update({k + "_ms": spread(v) for k, v in ts.items()})
        emit(d)
        # the widening kernel alone
        out = torch.empty((n, L), dtype=torch.int64, device="cuda:0")
        k_id, K = _lib.INTS_KINDS[kind], args.kernel_launches
        per = []
        for r in range(args.reps + 1):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(K):
                _lib.lib().lcpci_from_ints_device(enc._h, k_id, C.c_void_p(dev.data_ptr()), n, C.c_void_p(out.data_ptr()), None)
            e1.record()
            torch.cuda.synchronize()
            if r:
                per.append(e0.elapsed_time(e1) / K)
        d = dict(base, leg="kernel", kind=kind, launches_per_window=K, from_ints_ms=spread(per), bytes=n * (kb + 8 * L),
                 GBps=round(n * (kb + 8 * L) / (statistics.median(per) * 1e-3) / 1e9, 1))
        emit(d)
        del page, dev, out
        if kind != "wide":
            del pin, pin_t
    del limbs_dev, limbs, limbs_pin, cm_base, cm_ints, enc
    torch.cuda.empty_cache()

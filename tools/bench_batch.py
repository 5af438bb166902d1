#!/usr/bin/env python3
"""Batched commit against the sequential loop it replaces, on one GPU (include/lcpc_hip_batch.h).

For one encoder shape and n_batch polynomials already in HBM: (a) n_batch lcpc_commit_device calls on one stream, enqueued
without roots and synchronised once, and (b) one lcpcx_commit_batch_device call, synchronised once.  The two ALTERNATE in one
process -- a, b, a, b, ... after a warm-up of both -- so that clocks and the allocator's state are shared; wall times of the
host (enqueue + drain), medians and min / max of --steps rounds.  One JSON line per shape on stdout, appended to --out
(profiles/r10_batch.jsonl by default).

  python tools/bench_batch.py [--shape FIELD:LOG2N[:DIGEST] ...] [--encoding ligero|brakedown] [--code C] [--seed S]
                              [--n-batch B] [--steps K] [--warmup W] [--out PATH]

FIELD: ft63 / ft127 / ft191 / ft255; default shapes: ft63:16 (BASELINE's C1) and ft255:16.  --encoding brakedown: SdigEncoding.new of
--code (1 / 3 / 6) and --seed; the sequential loop is then the single-commit Brakedown pipeline."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import torch  # noqa: E402

from lcpc_amd import LcCommit, LigeroEncoding, SdigEncoding, commit_batch  # noqa: E402

FIELDS = {"ft63": 0, "ft127": 1, "ft191": 2, "ft255": 3}


def run(field, log_n, digest, n_batch, steps, warmup, encoding="ligero", code=3, seed=0):
    n = 1 << log_n
    if encoding == "brakedown":
        enc = SdigEncoding.new(FIELDS[field], n, seed, code, digest=digest)
    else:
        enc = LigeroEncoding.new(FIELDS[field], n, digest=digest)
    x = enc.random_coeffs_device(n_batch * n, seed=0).reshape(n_batch, n * enc.L)
    seq = [LcCommit(enc) for _ in range(n_batch)]
    bat = [LcCommit(enc) for _ in range(n_batch)]
    ptrs = [x[i].data_ptr() for i in range(n_batch)]
    torch.cuda.synchronize()

    def sequential():
        t0 = time.perf_counter()
        for i in range(n_batch):
            LcCommit.commit_device(ptrs[i], n, enc, 0, sync=False, into=seq[i])
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3

    def batched():
        t0 = time.perf_counter()
        commit_batch(enc, x, sync=True, into=bat)
        return (time.perf_counter() - t0) * 1e3

    ts, tb = [], []
    for i in range(warmup + steps):
        a, b = sequential(), batched()
        if i >= warmup:
            ts.append(a)
            tb.append(b)
    assert all(s.get_root() == b.get_root() for s, b in zip(seq, bat)), "batch and loop disagree"
    bat[0].set_timing(True)
    commit_batch(enc, x, into=bat)
    t = bat[0].timings()
    ms, mb = statistics.median(ts), statistics.median(tb)
    extra = dict(code=code, seed=seed) if encoding == "brakedown" else {}
    return dict(tool="bench_batch", encoding=encoding, **extra, field=field, log_n=log_n, digest=digest, n_batch=n_batch, n_rows=bat[0].n_rows, n_cols=bat[0].n_cols,
                steps=steps, warmup=warmup, seq_ms=ms, seq_min_ms=min(ts), seq_max_ms=max(ts), batch_ms=mb, batch_min_ms=min(tb),
                batch_max_ms=max(tb), seq_over_batch=ms / mb, batch_encode_ms=t.encode_ms, batch_hash_ms=t.hash_ms,
                batch_merkle_ms=t.merkle_ms, batch_launches=[t.encode_launches, t.hash_launches, t.merkle_launches])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", nargs="*", default=["ft63:16", "ft255:16"], help="FIELD:LOG2N[:DIGEST]")
    ap.add_argument("--encoding", choices=["ligero", "brakedown"], default="ligero")
    ap.add_argument("--code", type=int, default=3, help="brakedown: SdigCode 1 / 3 / 6")
    ap.add_argument("--seed", type=int, default=0, help="brakedown: matgen seed")
    ap.add_argument("--n-batch", type=int, default=64)
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r10_batch.jsonl"))
    a = ap.parse_args()
    for sh in a.shape:
        parts = sh.split(":")
        r = run(parts[0], int(parts[1]), parts[2] if len(parts) > 2 else "blake3", a.n_batch, a.steps, a.warmup, a.encoding, a.code, a.seed)
        line = json.dumps(r)
        print(line, flush=True)
        if a.out:
            with open(a.out, "a") as f:
                f.write(line + "\n")


if __name__ == "__main__":
    main()

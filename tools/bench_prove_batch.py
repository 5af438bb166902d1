#!/usr/bin/env python3
"""Batched prove against the sequential loop it replaces, on one GPU (include/lcpc_hip_batch.h, lcpcx_prove_batch).

For one encoder shape and n_batch committed polynomials (one batched commit): (a) n_batch lcpc_prove calls one after the other
and (b) one lcpcx_prove_batch call, all members opened at ONE point (outer_stride 0).  The two ALTERNATE in one process -- a, b,
a, b, ... after a warm-up of both -- with fresh clones of the members' transcripts each round (made outside the timed region), so
that clocks, working sets and the proof-buffer pool are shared; wall times of the host, medians and min / max of --steps rounds.
The last round's proofs are compared byte for byte.  One JSON line per shape on stdout, appended to --out
(profiles/prove_batch.jsonl by default).

  python tools/bench_prove_batch.py [--shape FIELD:LOG2N[:DIGEST] ...] [--encoding ligero|brakedown] [--code C] [--seed S]
                                    [--n-batch B] [--steps K] [--warmup W] [--out PATH]

FIELD: ft63 / ft127 / ft191 / ft255; default shapes: ft63:16 and ft255:16.  With LCPC_DEBUG_TIMING=1 in the environment the
library prints the phase times of every call on stderr ([lcpc_prove] per single prove, [lcpcx_prove_batch] per batch): that is
where the share of the host absorb comes from."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from lcpc_amd import LigeroEncoding, SdigEncoding, Transcript, commit_batch, prove_batch  # noqa: E402

FIELDS = {"ft63": 0, "ft127": 1, "ft191": 2, "ft255": 3}


def run(field, log_n, digest, n_batch, steps, warmup, encoding="ligero", code=3, seed=0):
    n = 1 << log_n
    if encoding == "brakedown":
        enc = SdigEncoding.new(FIELDS[field], n, seed, code, digest=digest)
    else:
        enc = LigeroEncoding.new(FIELDS[field], n, digest=digest)
    x = enc.random_coeffs_device(n_batch * n, seed=0).reshape(n_batch, n * enc.L)
    cms = commit_batch(enc, x)
    outer = enc.random_coeffs_device(cms[0].n_rows, seed=1)
    torch.cuda.synchronize()
    outer = outer.cpu().numpy().view(np.uint64).reshape(cms[0].n_rows, enc.L).copy()
    base = []
    for i, cm in enumerate(cms):
        tr = Transcript(b"bench_prove_batch")
        tr.append_message(b"polycommit", cm.get_root())
        tr.append_message(b"member", i.to_bytes(8, "big"))
        base.append(tr)

    def sequential():
        trs = [t.clone() for t in base]
        t0 = time.perf_counter()
        pfs = [cm.prove(outer, enc, tr) for cm, tr in zip(cms, trs)]
        return (time.perf_counter() - t0) * 1e3, pfs

    def batched():
        trs = [t.clone() for t in base]
        t0 = time.perf_counter()
        pfs, stats = prove_batch(cms, outer, trs, return_stats=True)
        return (time.perf_counter() - t0) * 1e3, pfs, stats

    ts, tb = [], []
    for i in range(warmup + steps):
        a, pa = sequential()
        b, pb, stats = batched()
        if i >= warmup:
            ts.append(a)
            tb.append(b)
    assert all(p.to_bytes() == q.to_bytes() for p, q in zip(pa, pb)), "batch and loop disagree"
    ms, mb = statistics.median(ts), statistics.median(tb)
    extra = dict(code=code, seed=seed) if encoding == "brakedown" else {}
    return dict(tool="bench_prove_batch", encoding=encoding, **extra, field=field, log_n=log_n, digest=digest, n_batch=n_batch,
                n_rows=cms[0].n_rows, n_per_row=cms[0].n_per_row, n_cols=cms[0].n_cols, n_degree_tests=enc.get_n_degree_tests(),
                n_col_opens=enc.get_n_col_opens(), proof_bytes=len(pb[0].to_bytes()), steps=steps, warmup=warmup,
                seq_ms=ms, seq_min_ms=min(ts), seq_max_ms=max(ts), batch_ms=mb, batch_min_ms=min(tb), batch_max_ms=max(tb),
                seq_over_batch=ms / mb, groups=stats.groups, collapse_launches=stats.collapse_launches,
                open_launches=stats.open_launches, host_syncs=stats.host_syncs)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", nargs="*", default=["ft63:16", "ft255:16"], help="FIELD:LOG2N[:DIGEST]")
    ap.add_argument("--encoding", choices=["ligero", "brakedown"], default="ligero")
    ap.add_argument("--code", type=int, default=3, help="brakedown: SdigCode 1 / 3 / 6")
    ap.add_argument("--seed", type=int, default=0, help="brakedown: matgen seed")
    ap.add_argument("--n-batch", type=int, default=64)
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "prove_batch.jsonl"))
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

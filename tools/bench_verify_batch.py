#!/usr/bin/env python3
"""Batched verify against the sequential loop it replaces, on one GPU (include/lcpc_hip_verify.h, lcpcv_verify_batch).

For one encoder shape and n_batch proofs (one batched commit, one batched prove, all opened at ONE point): (a) n_batch lcpc_verify
calls one after the other and (b) one lcpcv_verify_batch call.  The two ALTERNATE in one process -- a, b, a, b, ... after a warm-up of
both -- with fresh clones of the members' transcripts each round (made outside the timed region), so that clocks and working sets are
shared; wall times of the host, medians and min / max of --steps rounds.  Every round's evaluations are compared.  The phase split
of the batch (parse + stage, transcripts, device, path folds) is read from the library's LCPC_DEBUG_TIMING line, on a second encoder
of the same shape after the timed rounds.  One JSON line per shape on stdout, appended to --out (profiles/verify_batch.jsonl by default).

  python tools/bench_verify_batch.py [--shape FIELD:LOG2N[:DIGEST] ...] [--encoding ligero|brakedown] [--code C] [--seed S]
                                     [--n-batch B] [--steps K] [--warmup W] [--out PATH]

FIELD: ft63 / ft127 / ft191 / ft255; default shapes: ft255:16, ft127:16 and ft255:16:sha3_256."""
import argparse
import json
import os
import re
import statistics
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from lcpc_amd import LigeroEncoding, SdigEncoding, Transcript, commit_batch, prove_batch, verify_batch  # noqa: E402

FIELDS = {"ft63": 0, "ft127": 1, "ft191": 2, "ft255": 3}
PHASES = re.compile(r"\[lcpcv_verify_batch\].*?parse \+ stage ([\d.]+) ms, transcripts ([\d.]+), device [^)]*\) ([\d.]+), path folds ([\d.]+), total ([\d.]+)")


def make_encoder(field, n, digest, encoding, code, seed):
    if encoding == "brakedown":
        return SdigEncoding.new(FIELDS[field], n, seed, code, digest=digest)
    return LigeroEncoding.new(FIELDS[field], n, digest=digest)


def host_elems(enc, n, seed):
    t = enc.random_coeffs_device(n, seed=seed)
    torch.cuda.synchronize()
    return t.cpu().numpy().view(np.uint64).reshape(n, enc.L).copy()


def phase_split(field, n, digest, encoding, code, seed, roots, outer, inner, proofs, base):
    """the [lcpcv_verify_batch] line of one warm call under an encoder created with LCPC_DEBUG_TIMING set"""
    os.environ["LCPC_DEBUG_TIMING"] = "1"
    try:
        enc = make_encoder(field, n, digest, encoding, code, seed)
    finally:
        del os.environ["LCPC_DEBUG_TIMING"]
    verify_batch(enc, roots, outer, inner, proofs, [t.clone() for t in base])          # warm: working set, pinned arena
    trs = [t.clone() for t in base]
    sys.stderr.flush()
    with tempfile.TemporaryFile() as tmp:
        saved = os.dup(2)
        os.dup2(tmp.fileno(), 2)
        try:
            verify_batch(enc, roots, outer, inner, proofs, trs)
        finally:
            os.dup2(saved, 2)
            os.close(saved)
        tmp.seek(0)
        text = tmp.read().decode(errors="replace")
    m = PHASES.search(text)
    if not m:
        return None
    keys = ("parse_stage_ms", "transcripts_ms", "device_ms", "path_folds_ms", "total_ms")
    return dict(zip(keys, (float(x) for x in m.groups())))


def run(field, log_n, digest, n_batch, steps, warmup, encoding="ligero", code=3, seed=0):
    n = 1 << log_n
    enc = make_encoder(field, n, digest, encoding, code, seed)
    x = enc.random_coeffs_device(n_batch * n, seed=0).reshape(n_batch, n * enc.L)
    cms = commit_batch(enc, x)
    outer = host_elems(enc, cms[0].n_rows, 1)
    inner = host_elems(enc, cms[0].n_per_row, 2)
    roots = [cm.get_root() for cm in cms]
    base = []
    for i, root in enumerate(roots):
        tr = Transcript(b"bench_verify_batch")
        tr.append_message(b"polycommit", root)
        tr.append_message(b"member", i.to_bytes(8, "big"))
        base.append(tr)
    proofs = prove_batch(cms, outer, [t.clone() for t in base])

    def sequential():
        trs = [t.clone() for t in base]
        t0 = time.perf_counter()
        evs = [pf.verify(root, outer, inner, enc, tr) for pf, root, tr in zip(proofs, roots, trs)]
        return (time.perf_counter() - t0) * 1e3, evs

    def batched():
        trs = [t.clone() for t in base]
        t0 = time.perf_counter()
        evals, status, stats = verify_batch(enc, roots, outer, inner, proofs, trs, return_stats=True)
        return (time.perf_counter() - t0) * 1e3, evals, status, stats

    ts, tb = [], []
    for i in range(warmup + steps):
        a, evs = sequential()
        b, evals, status, stats = batched()
        assert not status.any() and all(np.array_equal(e, f) for e, f in zip(evs, evals)), "batch and loop disagree"
        if i >= warmup:
            ts.append(a)
            tb.append(b)
    ms, mb = statistics.median(ts), statistics.median(tb)
    extra = dict(code=code, seed=seed) if encoding == "brakedown" else {}
    return dict(tool="bench_verify_batch", encoding=encoding, **extra, field=field, log_n=log_n, digest=digest, n_batch=n_batch,
                n_rows=cms[0].n_rows, n_per_row=cms[0].n_per_row, n_cols=cms[0].n_cols, n_degree_tests=enc.get_n_degree_tests(),
                n_col_opens=enc.get_n_col_opens(), proof_bytes=len(proofs[0].to_bytes()), steps=steps, warmup=warmup,
                seq_ms=ms, seq_min_ms=min(ts), seq_max_ms=max(ts), batch_ms=mb, batch_min_ms=min(tb), batch_max_ms=max(tb),
                seq_over_batch=ms / mb, groups=stats.groups, encode_launches=stats.encode_launches, hash_launches=stats.hash_launches,
                check_launches=stats.check_launches, host_syncs=stats.host_syncs,
                phases=phase_split(field, n, digest, encoding, code, seed, roots, outer, inner, proofs, base))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", nargs="*", default=["ft255:16", "ft127:16", "ft255:16:sha3_256"], help="FIELD:LOG2N[:DIGEST]")
    ap.add_argument("--encoding", choices=["ligero", "brakedown"], default="ligero")
    ap.add_argument("--code", type=int, default=3, help="brakedown: SdigCode 1 / 3 / 6")
    ap.add_argument("--seed", type=int, default=0, help="brakedown: matgen seed")
    ap.add_argument("--n-batch", type=int, default=64)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "verify_batch.jsonl"))
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

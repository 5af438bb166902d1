#!/usr/bin/env python3
"""tools/bench_concurrent.py [reps] -- T host threads proving ONE commitment at once, and verifying under ONE encoder at once
(include/lcpc_hip.h "Threads"), T = 1, 2, 4, 8; one JSON line per commitment.

Commitments: C5's (2^26 Ft255 Ligero, rho = 1/2) and a Brakedown 2^24 Ft255 one, committed from HBM.  Every thread has its own
outer tensor and transcript.  Per T and per direction (prove_xT, verify_xT): the wall time of the T calls started together (the
best of `reps` rounds), the median latency of one call over all rounds, calls per second (T / wall), and whether every proof /
evaluation equals the one the same thread's inputs give when proved / verified alone (bytes_equal_serial).  `*_x8_over_x1` is
the wall of eight calls over that of one: 1.0 would be perfect overlap, 8.0 none."""
import json
import os
import statistics
import sys
import threading
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tools")]
import numpy as np
import torch

import bench_configs as B
from common import mk_transcript
from lcpc_amd import LcCommit, LcEvalProof, LigeroEncoding, SdigEncoding, Transcript

THREADS = (1, 2, 4, 8)


def rand_host(n, L, seed):
    """n reduced Ft255 elements (top limb below 2^60 < p / 2^192)"""
    a = np.random.default_rng(seed).integers(0, 2 ** 64 - 1, (n, L), dtype=np.uint64, endpoint=True)
    a[:, L - 1] &= np.uint64((1 << 60) - 1)
    return a


def cpu_quota():
    """CPUs of time the cgroup grants this process (cgroup v2 cpu.max), else the CPUs it may run on"""
    try:
        with open("/sys/fs/cgroup/cpu.max") as f:
            q, p = f.read().split()[:2]
        if q != "max":
            return round(int(q) / int(p), 1)
    except (OSError, ValueError):
        pass
    return len(os.sched_getaffinity(0))


def together(fn, T):
    """fn(k) for k < T on T threads released by one barrier; (wall s, [per-call s])"""
    lat, errs = [0.0] * T, []
    start = threading.Barrier(T + 1)

    def body(k):
        try:
            start.wait()
            t0 = time.perf_counter()
            fn(k)
            lat[k] = time.perf_counter() - t0
        except Exception as ex:
            errs.append(repr(ex))

    th = [threading.Thread(target=body, args=(k,)) for k in range(T)]
    for t in th:
        t.start()
    start.wait()
    t0 = time.perf_counter()
    for t in th:
        t.join()
    wall = time.perf_counter() - t0
    if errs:
        raise RuntimeError(errs[0])
    return wall, lat


def run(name, enc, n, reps):
    fid, L = 3, 4
    coeffs = B.rand_coeffs(n, L, 7)
    st = torch.cuda.current_stream().cuda_stream
    c = LcCommit.commit_device(coeffs.data_ptr(), n, enc, st, sync=True)
    root, nco = c.get_root(), enc.get_n_col_opens()
    T_MAX = max(THREADS)
    outers = [rand_host(c.n_rows, L, 100 + k) for k in range(T_MAX)]
    inners = [rand_host(c.n_per_row, L, 200 + k) for k in range(T_MAX)]
    ref_pf = [c.prove(outers[k], enc, mk_transcript(Transcript, root, nco)).to_bytes() for k in range(T_MAX)]     # alone, one by one
    ref_ev = [LcEvalProof.from_bytes(ref_pf[k], L).verify(root, outers[k], inners[k], enc, mk_transcript(Transcript, root, nco)).tobytes()
              for k in range(T_MAX)]
    out = {"case": name, "field": "ft255", "dims": [c.n_rows, c.n_per_row, c.n_cols], "reps": reps, "cpu_quota": cpu_quota()}
    for what in ("prove", "verify"):
        for T in THREADS:
            got = [None] * T

            def prove(k):
                got[k] = c.prove(outers[k], enc, mk_transcript(Transcript, root, nco)).to_bytes()

            def verify(k):
                got[k] = LcEvalProof.from_bytes(ref_pf[k], L).verify(root, outers[k], inners[k], enc, mk_transcript(Transcript, root, nco)).tobytes()

            fn, ref = (prove, ref_pf) if what == "prove" else (verify, ref_ev)
            together(fn, T)                                   # warm: this many working sets exist
            walls, lats, same = [], [], True
            for _ in range(reps):
                wall, lat = together(fn, T)
                walls.append(wall)
                lats += lat
                same = same and got == ref[:T]
            wall = min(walls)
            out["%s_x%d" % (what, T)] = {"wall_ms": round(wall * 1e3, 3), "median_call_ms": round(statistics.median(lats) * 1e3, 3),
                                         "per_s": round(T / wall, 1), "bytes_equal_serial": same}
        out["%s_x8_over_x1" % what] = round(out["%s_x8" % what]["wall_ms"] / out["%s_x1" % what]["wall_ms"], 3)
    print(json.dumps(out), flush=True)
    del c, coeffs
    torch.cuda.empty_cache()


def main():
    reps = int(sys.argv[1]) if len(sys.argv) > 1 else 5
    run("c5_ligero_2^26", LigeroEncoding.new(3, 1 << 26, rho=(1, 2)), 1 << 26, reps)
    run("brakedown_2^24", SdigEncoding.new(3, 1 << 24, 0), 1 << 24, reps)


if __name__ == "__main__":
    main()

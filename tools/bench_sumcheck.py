#!/usr/bin/env python3
"""tools/bench_sumcheck.py -- the sumcheck round, the bind and the fused call (include/lcpc_hip_sumcheck.h) on one box, in one process,
the variants alternated call by call.  One JSON line per leg with the median and the spread (min, max) of every side; kept under
profiles/r21_sumcheck.jsonl.  Wall clock around the calls and a synchronisation.

  python tools/bench_sumcheck.py [--reps 7] [--host-reps 3] [--fields 3,0] [--sizes 20,24,26] [--host-max 20] [--order low] [--tag TAG]

  calls    per field, log2 n and term list (a b; eq (a b - c)): lcpcm_round_device on n, lcpcm_bind_device of every table on n, the
           fused lcpcm_bind_round_device on n, and what it replaces -- the bind on n followed by the round on n / 2 -- next to
           lcpcq_pointwise_device LCPCQ_MUL over as many input bytes as the round reads: the one-pass yardstick.  Up to --host-max
           also the host forms on one thread (lcpcm_round, lcpcm_bind of every table), the route without the extension.  The
           fused call and the two calls must have produced equal bytes (asserted) before anything is timed.
  whole    a whole sumcheck of log2 n rounds from tables of n elements, the d + 1 evaluations of every round downloaded before the
           next challenge is known: with the fused call, and with the two calls.  The challenge is a constant; a transcript costs
           the same on both sides.
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
ap.add_argument("--host-max", type=int, default=20)
ap.add_argument("--order", default="low")
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
from lcpc_amd import FIELD_MODULUS, LigeroEncoding

if not torch.cuda.is_available():
    sys.exit("bench_sumcheck: no GPU")
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


def mont(fid, v, L):
    """the Montgomery limbs of a canonical int"""
    x = v * (1 << (64 * L)) % FIELD_MODULUS[fid]
    return np.array([(x >> (64 * i)) & 0xFFFFFFFFFFFFFFFF for i in range(L)], np.uint64)


def term_lists(fid, L):
    minus_one = mont(fid, FIELD_MODULUS[fid] - 1, L)
    return (("ab", 2, [(None, [0, 1])]), ("eq_ab_minus_c", 4, [(mont(fid, 1, L), [0, 1, 2]), (minus_one, [0, 3])]))


def multiplies(terms, n_tables):
    """field multiplies per pair of the round, per pair of the bind (all tables), per lane of the fused call"""
    d = max(len(idx) for _, idx in terms)
    rnd = sum((len(idx) - 1) * (d + 1) for _, idx in terms)
    return {"round_per_pair": rnd, "bind_per_pair": n_tables, "fused_per_lane": 2 * n_tables + rnd}


for fid in (int(v) for v in args.fields.split(",") if v):
    enc = LigeroEncoding.new_from_dims(fid, 64, 128)
    L = enc.L
    eb = 8 * L
    r = mont(fid, 0x123456789ABCDEF % FIELD_MODULUS[fid], L)
    for log_n in (int(v) for v in args.sizes.split(",") if v):
        n = 1 << log_n
        for tname, n_tables, terms in term_lists(fid, L):
            tabs = [enc.random_coeffs_device(n, seed=10 + j) for j in range(n_tables)]
            outs = [torch.empty((n // 2, L), dtype=torch.int64, device=DEV) for _ in range(n_tables)]
            outs2 = [torch.empty((n // 2, L), dtype=torch.int64, device=DEV) for _ in range(n_tables)]
            d1 = max(len(idx) for _, idx in terms) + 1
            ev, ev2 = (torch.empty((d1, L), dtype=torch.int64, device=DEV) for _ in range(2))
            m = n_tables * n // 2                                      # LCPCQ_MUL reads 2 m elements: the round's input bytes
            pa, pb = enc.random_coeffs_device(m, seed=3), enc.random_coeffs_device(m, seed=4)
            po = torch.empty_like(pa)

            def two_calls():
                enc.sumcheck_bind(tabs, r, args.order, out=outs2)
                enc.sumcheck_round(outs2, terms, args.order, evals=ev2)

            enc.sumcheck_bind_round(tabs, terms, r, args.order, out=outs, evals=ev)
            two_calls()
            assert torch.equal(ev, ev2) and all(torch.equal(a, b) for a, b in zip(outs, outs2)), "the fused call and the two calls disagree"
            d = {"leg": "calls", "field": fid, "log_n": log_n, "terms": tname, "n_tables": n_tables, "order": args.order, "reps": args.reps,
                 "input_bytes": n_tables * n * eb, "equal_bytes": True, "multiplies": multiplies(terms, n_tables)}
            if log_n <= args.host_max:
                h_tabs = [to_host(t) for t in tabs]
                want = lcpc_amd.sumcheck_round(fid, h_tabs, terms, args.order)
                enc.sumcheck_round(tabs, terms, args.order, evals=ev2)
                assert np.array_equal(to_host(ev2), want), "the device and the host round disagree"
                hs = alternate([("host_round", lambda: lcpc_amd.sumcheck_round(fid, h_tabs, terms, args.order)),
                                ("host_bind", lambda: [lcpc_amd.sumcheck_bind(fid, t, r, args.order) for t in h_tabs])], args.host_reps)
                for name, v in hs.items():
                    d[name + "_ms"] = spread(v)
                del h_tabs
            ts = alternate([("round", lambda: enc.sumcheck_round(tabs, terms, args.order, evals=ev2)),
                            ("bind", lambda: enc.sumcheck_bind(tabs, r, args.order, out=outs2)),
                            ("fused", lambda: enc.sumcheck_bind_round(tabs, terms, r, args.order, out=outs, evals=ev)),
                            ("two_calls", two_calls),
                            ("mul", lambda: enc.pointwise("mul", pa, pb, out=po))], args.reps)
            for name, v in ts.items():
                d[name + "_ms"] = spread(v)
            med = {k: statistics.median(v) for k, v in ts.items()}
            d["round_over_mul"] = round(med["round"] / med["mul"], 3)
            d["fused_over_two_calls"] = round(med["fused"] / med["two_calls"], 3)
            d["round_gbyte_s"] = round(n_tables * n * eb / med["round"] / 1e6, 1)
            d["bind_gbyte_s"] = round(n_tables * (n + n // 2) * eb / med["bind"] / 1e6, 1)               # (read n, write n / 2, per table)
            d["fused_gbyte_s"] = round(n_tables * (n + n // 2) * eb / med["fused"] / 1e6, 1)
            d["mul_gbyte_s"] = round(3 * m * eb / med["mul"] / 1e6, 1)
            d["round_gmul_s"] = round(d["multiplies"]["round_per_pair"] * (n // 2) / med["round"] / 1e6, 2)
            d["fused_gmul_s"] = round(d["multiplies"]["fused_per_lane"] * (n // 4) / med["fused"] / 1e6, 2)
            if "host_round_ms" in d:
                d["host_over_device_round"] = round(d["host_round_ms"]["median"] / med["round"], 1)
            emit(d)
            del pa, pb, po, outs2

            # a whole sumcheck: level k writes tables of n >> (k + 1) elements into buffers of their own, so the inputs stay
            lv = [[outs[j][:n >> (k + 1)] if k == 0 else torch.empty((n >> (k + 1), L), dtype=torch.int64, device=DEV) for j in range(n_tables)]
                  for k in range(log_n)]

            def whole(fused):
                cur = tabs
                enc.sumcheck_round(cur, terms, args.order, evals=ev)
                g = ev.cpu()
                for k in range(log_n):
                    if k + 1 == log_n:
                        enc.sumcheck_bind(cur, r, args.order, out=lv[k])
                    elif fused:
                        enc.sumcheck_bind_round(cur, terms, r, args.order, out=lv[k], evals=ev)
                        g = ev.cpu()
                    else:
                        enc.sumcheck_bind(cur, r, args.order, out=lv[k])
                        enc.sumcheck_round(lv[k], terms, args.order, evals=ev)
                        g = ev.cpu()
                    cur = lv[k]
                return g

            a, b = whole(True), whole(False)
            assert torch.equal(a, b)
            ts = alternate([("whole_fused", lambda: whole(True)), ("whole_two_calls", lambda: whole(False))], args.reps)
            d = {"leg": "whole", "field": fid, "log_n": log_n, "terms": tname, "n_tables": n_tables, "order": args.order, "reps": args.reps, "rounds": log_n}
            for name, v in ts.items():
                d[name + "_ms"] = spread(v)
            d["fused_over_two_calls"] = round(statistics.median(ts["whole_fused"]) / statistics.median(ts["whole_two_calls"]), 3)
            emit(d)
            del tabs, outs, lv
            torch.cuda.empty_cache()
    del enc

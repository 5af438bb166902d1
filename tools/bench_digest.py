#!/usr/bin/env python3
"""BLAKE3 vs SHA3-256 vs BLAKE2b vs Keccak-256 vs SHA-256 commitment digest on one GPU: the kernel-group times of lcpc_get_timings for device-resident commits
(Ligero Ft255 2^20 / 2^24 / 2^26, Ligero Ft127 2^24, Brakedown Ft255 2^24), and prove / verify wall times at 2^24.

One JSON line per (config, digest) on stdout, then a Markdown table.  The same input vector (drawn on the device, seed 0) is
committed under every digest; the roots must differ.  Keccak-256 runs SHA3-256's instruction stream with another constant, so its times belong inside the spread that repeated
SHA3-256 measurements show: after the five digests the two are measured again, alternating ("sha3_256#2", "keccak256#2", ...
up to #4; each a fresh encoder and commitment, median of --steps commits), and the last lines report min / median / max of both.

  python tools/bench_digest.py [--steps K] [--warmup W] [--only NAME ...]
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "oracle")):
    if p not in sys.path:
        sys.path.insert(0, p)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from lcpc_amd import LcCommit, LcEvalProof, LigeroEncoding, SdigEncoding, Transcript  # noqa: E402

CONFIGS = [  # name, kind, field, log2 len, prove / verify timed
    ("lig_ft255_20", "ligero", 3, 20, False),
    ("lig_ft255_24", "ligero", 3, 24, True),
    ("lig_ft255_26", "ligero", 3, 26, False),
    ("lig_ft127_24", "ligero", 1, 24, True),
    ("sdig_ft255_24", "sdig", 3, 24, True),
]


DIGESTS = ("blake3", "sha3_256", "blake2b", "keccak256", "sha256")
REPEATS = tuple("%s#%d" % (d, k) for k in (2, 3, 4) for d in ("sha3_256", "keccak256"))


def make_enc(kind, fid, n, digest):
    if kind == "ligero":
        return LigeroEncoding.new(fid, n, digest=digest)
    return SdigEncoding.new(fid, n, 0, digest=digest)


def transcript(root, nco):
    tr = Transcript(b"bench_digest")
    tr.append_message(b"polycommit", bytes(root))
    tr.append_message(b"ncols", int(nco).to_bytes(8, "big"))
    return tr


def run(name, kind, fid, log_n, pv, digest, steps, warmup):
    n = 1 << log_n
    enc = make_enc(kind, fid, n, digest)
    x = enc.random_coeffs_device(n, seed=0)
    c = LcCommit(enc)
    c.set_timing(True)
    rec = []
    for i in range(warmup + steps):
        LcCommit.commit_device(x.data_ptr(), n, enc, 0, sync=True, into=c)
        if i >= warmup:
            t = c.timings()
            rec.append((t.encode_ms, t.hash_ms, t.merkle_ms, t.total_ms, t.hash_launches, t.merkle_launches))
    med = [statistics.median(r[k] for r in rec) for k in range(4)]
    out = dict(config=name, digest=digest, n_rows=c.n_rows, n_cols=c.n_cols, steps=steps, encode_ms=med[0], hash_ms=med[1],
               merkle_ms=med[2], total_ms=med[3], hash_launches=rec[-1][4], merkle_launches=rec[-1][5], root=c.get_root().hex()[:16])
    if pv:
        root, nco = c.get_root(), enc.get_n_col_opens()
        outer = enc.random_coeffs_device(c.n_rows, seed=1).cpu().numpy().view(np.uint64)
        inner = enc.random_coeffs_device(c.n_per_row, seed=2).cpu().numpy().view(np.uint64)
        pt, vt = [], []
        for i in range(1 + max(1, steps // 2)):            # the first prove / verify warms the pinned arenas
            t0 = time.perf_counter()
            pf = c.prove(outer, enc, transcript(root, nco))
            t1 = time.perf_counter()
            LcEvalProof.from_bytes(pf.to_bytes(), enc.L).verify(root, outer, inner, enc, transcript(root, nco))
            t2 = time.perf_counter()
            if i:
                pt.append((t1 - t0) * 1e3)
                vt.append((t2 - t1) * 1e3)
        out.update(prove_ms=statistics.median(pt), verify_ms=statistics.median(vt))
    del c, x, enc
    torch.cuda.empty_cache()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--only", nargs="*", default=None, help="config names (default: all)")
    a = ap.parse_args()
    rows = []
    for name, kind, fid, log_n, pv in CONFIGS:
        if a.only and name not in a.only:
            continue
        pair = {}
        for digest in DIGESTS + REPEATS:
            r = run(name, kind, fid, log_n, pv and "#" not in digest, digest.split("#")[0], a.steps, a.warmup)
            r["digest"] = digest
            print(json.dumps(r), flush=True)
            pair[digest] = r
            rows.append(r)
        assert all(pair[d]["root"] == pair[d.split("#")[0]]["root"] for d in REPEATS)
        assert len({r["root"] for d, r in pair.items() if "#" not in d}) == len(DIGESTS)
    print()
    print("| config | digest | rows x cols | encode ms | hash ms | merkle ms | total ms | prove ms | verify ms |")
    print("|---|---|---|---|---|---|---|---|---|")
    for r in rows:
        pv = ("%.1f" % r["prove_ms"], "%.1f" % r["verify_ms"]) if "prove_ms" in r else ("", "")
        print("| %s | %s | %d x %d | %.3f | %.3f | %.3f | %.3f | %s | %s |" % (r["config"], r["digest"], r["n_rows"], r["n_cols"],
              r["encode_ms"], r["hash_ms"], r["merkle_ms"], r["total_ms"], pv[0], pv[1]))
    print()
    by = {(r["config"], r["digest"]): r for r in rows}
    for name in sorted({r["config"] for r in rows}, key=[c[0] for c in CONFIGS].index):
        def spread(d, key):
            v = sorted(by[(name, x)][key] for x in (d,) + tuple(r for r in REPEATS if r.startswith(d + "#")))
            return "%.3f / %.3f / %.3f" % (v[0], statistics.median(v), v[-1])
        print("%s: hash ms min / median / max of 4: SHA3-256 %s, Keccak-256 %s; merkle: SHA3-256 %s, Keccak-256 %s; "
              "SHA-256 hash / SHA3-256 median hash = %.3f" % (name, spread("sha3_256", "hash_ms"), spread("keccak256", "hash_ms"),
                                                               spread("sha3_256", "merkle_ms"), spread("keccak256", "merkle_ms"),
                                                               by[(name, "sha256")]["hash_ms"] / statistics.median(
                                                                   by[(name, x)]["hash_ms"] for x in ("sha3_256",) + tuple(r for r in REPEATS if r.startswith("sha3_256#")))))


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""tools/bench_rs.py -- the matrix of the reference's `cargo bench` functions (lcpc-ligero-pc/src/bench.rs:23-212,
lcpc-brakedown-pc/src/bench.rs:22-155; feature `bench`): commit / prove / verify for Ft127 and Ft255 at 2^16, 2^20 and 2^24
coefficients, Ligero (its default rate there: rho = 1/2 alias) and Brakedown, on the MI355X path; one JSON line per cell
(tools/bench_pvs.run: mean of 10 iterations, encoder construction outside, root / proof on the host every iteration).

  python tools/bench_rs.py [--digest blake3|sha3_256|blake2b|keccak256|sha256]

The reference's published matrix (doc/benchmark-results) was measured with D = Blake2b: `--digest blake2b` runs it like for like;
the default stays BLAKE3."""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tools")]
import bench_pvs

ap = argparse.ArgumentParser()
ap.add_argument("--digest", default="blake3", choices=("blake3", "sha3_256", "blake2b", "keccak256", "sha256"))
args = ap.parse_args()
for kind in ("ligero_hlf", "sdig"):
    for fid in (1, 3):
        for lgl in (16, 20, 24):
            bench_pvs.run(kind, lgl, fid, digest=args.digest)

"""bench.py's host-side helpers that build the inputs of its `configs` legs without the oracle (so that the timed product path never
touches it): the C5 tensors (powers of x, lcpc-ligero-pc/src/tests.rs:120-128) in ff_derive's Montgomery limbs, the reference's test
transcript (tests.rs:243-245), and SURVEY.md 8(d)'s algorithmic byte count -- checked HERE against the oracle / the survey's table.  CPU only."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402
from common import dump_bytes, load_dump, mk_transcript, powers  # noqa: E402


def test_powers_mont_equals_oracle_conversion(oracle):
    for n, step in ((257, 1), (64, 131072), (5, 3)):
        assert (bench.powers_mont(bench.C5_X, n, step) == powers(oracle, 3, bench.C5_X, n, step)).all()



def test_bench_transcript_is_the_test_transcript(oracle):
    root = bytes(range(32))
    a = bench.mk_transcript(oracle.Transcript, root, 309)
    b = mk_transcript(oracle.Transcript, root, 309)
    assert a.challenge_bytes(b"x", 32) == b.challenge_bytes(b"x", 32)


def test_commit_bytes_follow_the_survey_formula():
    """B_commit = F nr npr + 2 F nr nc + 32 (2 np2 - 1) + 32 (2 np2 - 2).  (The survey's own table was filled in with ONE
    digest term -- its 10.754 GB at the headline is 16.8 MB below the formula's 10.771 -- the bench follows the formula as written.)"""
    for F, nr, npr, nc, table_gb in ((8, 32, 2048, 4096, 2.88e-3), (32, 256, 65536, 131072, 2.693), (32, 512, 131072, 262144, 10.754), (32, 1024, 262144, 524288, 42.98)):
        want = F * nr * npr + 2 * F * nr * nc + 32 * (2 * nc - 1) + 32 * (2 * nc - 2)
        assert bench.commit_bytes_8d(F, nr, npr, nc) == want
        assert 0 <= want / 1e9 - table_gb <= 32 * 2 * nc / 1e9 + 0.006          # the table: the same without the re-read term
    assert bench.commit_bytes_8d(32, 101, 166292, 252931) == 32 * 101 * 166292 + 2 * 32 * 101 * 252931 + 32 * (4 * (1 << 18) - 3)   # np2 of a non-power-of-two width


class _OracleCommit:
    """the accessors bench.dump_outputs reads of an LcCommit, over an oracle commitment"""

    def __init__(self, oc):
        self.oc, self.n_rows, self.n_per_row, self.n_cols = oc, oc.n_rows, oc.n_per_row, oc.n_cols

    def _refresh(self):
        return self

    def get_root(self):
        return self.oc.get_root()

    def hashes(self):
        return self.oc.hashes().copy()

    def comm(self, row0, n):
        return self.oc.comm()[row0 * self.n_cols:(row0 + n) * self.n_cols].copy()

    def coeffs(self, row0, n):
        return self.oc.coeffs()[row0 * self.n_per_row:(row0 + n) * self.n_per_row].copy()


def test_dump_outputs_are_the_commitment(oracle, tmp_path, monkeypatch):
    """--dump-outputs: every array decodes to the commitment's own root / hashes / comm / coeffs at the indices written beside it;
    the sample (shrunk here so that every array is sampled) is the same on every call"""
    monkeypatch.setattr(bench, "DUMP_MAX_HASHES", 7)
    monkeypatch.setattr(bench, "DUMP_ROWS", 3)
    monkeypatch.setattr(bench, "DUMP_COMM_COLS", 5)
    monkeypatch.setattr(bench, "DUMP_COEFF_COLS", 4)
    oc = oracle.Commit.commit(oracle.random_elems(3, 1 << 12, 0), oracle.Encoding.ligero(3, 1 << 12))
    assert oc.n_rows > 3
    names = bench.dump_outputs(_OracleCommit(oc), range(oc.n_rows), str(tmp_path / "a"))
    bench.dump_outputs(_OracleCommit(oc), range(oc.n_rows), str(tmp_path / "b"))
    d, again = load_dump(str(tmp_path / "a")), load_dump(str(tmp_path / "b"))
    assert sorted(d) == names and set(names) == {"root", "hashes", "hashes_index", "comm", "coeffs", "rows_index", "comm_cols_index",
                                                 "coeffs_cols_index"}
    for k in names:
        assert d[k].dtype == (np.float64 if k.endswith("_index") else np.float32), k
        assert (d[k] == again[k]).all(), k
    hi, r, cc, pc = (d[k].astype(np.int64) for k in ("hashes_index", "rows_index", "comm_cols_index", "coeffs_cols_index"))
    assert len(hi) == 7 and len(r) == 3 and len(cc) == 5 and len(pc) == 4
    assert dump_bytes(d["root"]).tobytes() == oc.get_root()
    assert (dump_bytes(d["hashes"]) == oc.hashes()[hi]).all()
    comm = oc.comm().view(np.uint8).reshape(oc.n_rows, oc.n_cols, 32)
    coeffs = oc.coeffs().view(np.uint8).reshape(oc.n_rows, oc.n_per_row, 32)
    assert (dump_bytes(d["comm"]) == comm[r][:, cc]).all()
    assert (dump_bytes(d["coeffs"]) == coeffs[r][:, pc]).all()


class _ZeroCommit:
    n_rows, n_per_row, n_cols = 1024, 1 << 18, 1 << 19          # bench.py --log-len 28: every array of the dump is at its cap

    def _refresh(self):
        return self

    def get_root(self):
        return bytes(32)

    def hashes(self):
        return np.zeros((2 * self.n_cols - 1, 32), np.uint8)

    def comm(self, row0, n):
        return np.zeros((n * self.n_cols, 4), np.uint64)

    def coeffs(self, row0, n):
        return np.zeros((n * self.n_per_row, 4), np.uint64)


def test_dump_outputs_stay_under_64_mb(tmp_path):
    bench.dump_outputs(_ZeroCommit(), range(_ZeroCommit.n_rows), str(tmp_path))
    assert sum(os.path.getsize(os.path.join(tmp_path, f)) for f in os.listdir(tmp_path)) <= 64 << 20

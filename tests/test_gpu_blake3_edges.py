"""BLAKE3's block and chunk edges (the row counts tests/test_k3_cases.py derives) through the library, which tests/test_gpu_k3_kernels.py
bypasses: commit.cpp's choice between the fused small-commit kernel, one chunk straight into `hashes`, and chunk CVs + fold with four
lanes or one lane per column (restated as tests/common.py k3_plan and confirmed here by timings().hash_launches), its CV buffer and the
tree behind it.  The reference is the C oracle's commitment: the whole `hashes` array, the root, and one prove / verify round so that the
host verifier hashes the same edge columns."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import common as CM  # noqa: E402
import digest_ref as DR  # noqa: E402
import test_k3_cases as K  # noqa: E402
from lcpc_amd import LcCommit, LcEvalProof, LigeroEncoding, SdigEncoding, Transcript  # noqa: E402

pytestmark = pytest.mark.gpu
PATHS = ("fused", "one_chunk", "quad", "lanes")


def path_of(fid, n_rows, n_cols):
    plan = CM.k3_plan(fid, n_rows, n_cols)
    return plan, plan["path"] if plan["path"] != "chunks+finish" else ("quad" if plan["quad"] else "lanes")


def edge_rows(fid, max_chunks):
    """the table's rows of up to max_chunks chunks that sit ON an edge: exact chunk fill and one more, short last chunk, exact block fill"""
    rows = set(K.exact_chunk_fill_rows(fid)) | {n + 1 for n in K.exact_chunk_fill_rows(fid)} | set(K.short_last_chunk_rows(fid))
    rows |= set(K.exact_block_fill_rows(fid).values())
    return sorted(n for n in rows if CM.leaf_n_chunks(fid, n) <= max_chunks)


def ligero_shapes(fid):
    """(n_rows, n_per_row, n_cols): 128 columns take the fused kernel up to two chunks and four lanes per column beyond; 64 columns are
    below the fused kernel (one chunk straight into hashes, or CVs + fold); 16384 columns x 5 chunks > 65536: one lane per column"""
    first = K.first_rows_of_chunk_count(fid)
    out = [(n, 64, 128) for n in edge_rows(fid, 3)] + [(n, 32, 64) for n in edge_rows(fid, 2)]
    return out + [(first[5], 8192, 16384)]


def check(O, c, oc, enc, oenc, fid, n_rows, n_cols, expect_launches, prove):
    label = (fid, n_rows, n_cols)
    got, want = c.hashes(), oc.hashes()
    bad = np.nonzero((got != want).any(axis=1))[0]
    assert got.shape == want.shape and bad.size == 0, "%s: hash slots differ from the oracle's: %s" % (label, bad[:8])
    assert c.get_root() == oc.get_root(), label
    if expect_launches is not None:
        assert c.timings().hash_launches == expect_launches, label
    if prove:
        root, nco = oc.get_root(), enc.get_n_col_opens()
        t = O.random_elems(fid, n_rows, 5)
        pf = c.prove(t, enc, CM.mk_transcript(Transcript, root, nco)).to_bytes()
        opf, _ = oc.prove(t, oenc, CM.mk_transcript(O.Transcript, root, nco))
        assert pf == opf, label
        cols = np.array([0, n_cols - 1, n_cols // 2], np.uint64)
        vals, paths = c.open_columns(cols)
        for k, col in enumerate(cols):
            assert O.hash_column(fid, vals[k]) == bytes(want[int(col)]), label
        x = 0x1234567
        p = K.P.FIELDS[fid].p
        inner = O.to_mont(fid, [pow(x, i, p) for i in range(c.n_per_row)])
        outer = O.to_mont(fid, [pow(pow(x, c.n_per_row, p), i, p) for i in range(n_rows)])
        pf2 = c.prove(outer, enc, CM.mk_transcript(Transcript, root, nco)).to_bytes()
        ev = LcEvalProof.from_bytes(pf2, enc.L).verify(root, outer, inner, enc, CM.mk_transcript(Transcript, root, nco))
        orc, oev = O.verify(oenc, root, outer, inner, pf2, CM.mk_transcript(O.Transcript, root, nco))
        assert orc == 0 and np.array_equal(np.asarray(ev).reshape(-1), oev), label


@pytest.mark.parametrize("fid", K.FIDS)
def test_ligero_from_parts_at_every_edge_and_path(oracle, fid):
    O = oracle
    seen, encs = {}, {}
    for n_rows, n_per_row, n_cols in ligero_shapes(fid):
        plan, path = path_of(fid, n_rows, n_cols)
        if n_cols not in encs:
            encs[n_cols] = (LigeroEncoding.new_from_dims(fid, n_per_row, n_cols), O.Encoding.ligero_from_dims(fid, n_per_row, n_cols))
        enc, oenc = encs[n_cols]
        oc = O.Commit.commit(DR.edge_elems(O, fid, n_rows * n_per_row - 1, n_rows), oenc, n_threads=16)
        c = LcCommit(enc)
        c.set_timing(True)
        LcCommit.from_parts(enc, oc.comm(), oc.coeffs(), n_rows, into=c)
        check(O, c, oc, enc, oenc, fid, n_rows, n_cols, plan["hash_launches"], prove=path not in seen)
        seen.setdefault(path, []).append(n_rows)
    assert set(seen) == set(PATHS), seen                                    # each of the four paths, for this field
    assert {CM.k3_plan(fid, n, 128)["hash_launches"] for n in seen["fused"]} == {1}


@pytest.mark.parametrize("fid", K.FIDS)
def test_brakedown_at_the_edges(oracle, fid):
    """Brakedown: from_parts keeps comm row-major in Montgomery form whatever the row count (Ft255 on many chunks: the one
    leaf_chunk_kernel<8, false, *> case the library reaches); commit from 24 rows on hashes the position-major canonical copy"""
    O = oracle
    n_per_row = 40
    oenc = O.Encoding.sdig_from_dims(fid, n_per_row, 0, 3, DR.SDIG_CODE)
    _, _, n_cols = oenc.get_dims(n_per_row)
    enc = SdigEncoding.new_from_dims(fid, n_per_row, n_cols, 3, DR.SDIG_CODE)
    rows = [n for n in edge_rows(fid, 3) if n >= 24]
    assert rows and {CM.leaf_n_chunks(fid, n) for n in rows} >= {2, 3} and n_cols % 64
    for i, n_rows in enumerate(rows):
        plan, path = path_of(fid, n_rows, n_cols)
        coeffs = DR.edge_elems(O, fid, n_rows * n_per_row - 3, 50 + n_rows)
        oc = O.Commit.commit(coeffs, oenc, n_threads=16)
        c = LcCommit(enc)
        c.set_timing(True)
        LcCommit.from_parts(enc, oc.comm(), oc.coeffs(), n_rows, into=c)
        check(O, c, oc, enc, oenc, fid, n_rows, n_cols, plan["hash_launches"], prove=i == 0)
        c2 = LcCommit.commit(coeffs, enc)
        check(O, c2, oc, enc, oenc, fid, n_rows, n_cols, None, prove=i == 1)


@pytest.mark.parametrize("fid", K.FIDS)
def test_refill_across_chunk_counts(oracle, fid):
    """one LcCommit refilled with row counts that move the chunk count up and down (1, 3, 2, 5, 1 chunks ..): a stale CV slot or tree
    level would show in `hashes`"""
    O = oracle
    n_per_row, n_cols = 32, 64
    oenc = O.Encoding.ligero_from_dims(fid, n_per_row, n_cols)
    enc = LigeroEncoding.new_from_dims(fid, n_per_row, n_cols)
    first = K.first_rows_of_chunk_count(fid)
    full = K.exact_chunk_fill_rows(fid)
    c = LcCommit(enc)
    counts = []
    for n_rows in (3, first[3], first[2], first[5], full[0], first[4] - 1, 1, full[-1] + 1, first[2] - 1):
        coeffs = DR.edge_elems(O, fid, n_rows * n_per_row - 1, 300 + n_rows)
        oc = O.Commit.commit(coeffs, oenc, n_threads=16)
        LcCommit.commit(coeffs, enc, into=c)
        assert c.n_rows == n_rows
        check(O, c, oc, enc, oenc, fid, n_rows, n_cols, None, prove=False)
        counts.append(CM.leaf_n_chunks(fid, n_rows))
    assert any(a < b for a, b in zip(counts, counts[1:])) and any(a > b for a, b in zip(counts, counts[1:])) and max(counts) >= 5

"""K1s's two factorisations of the Ft255 two-pass row NTT (lcpc_amd/csrc/ntt_l9s.hip): LCPC_NTT_FORM=coset (pure first pass, coset-form
last pass) against LCPC_NTT_FORM=dif (the twist on the first pass) and against the oracle, through the public path: commit (canonical
output: comm, hashes, root, coeffs) and encode (Montgomery output), every element.

Shapes: 2^11 (S = 1: the radix-2 peel alone), 2^12 (S = 2: the I-only round alone, which then converts every output), 2^13 (odd S with
one radix-4 round), 2^15 (S = 5: one pack round, the limb intermediate), 2^18 (the headline's 8 + 10: uniform round, packed
intermediate), 2^20 (S = 10).  Fills: n_cols / 2 (zero half), n_cols / 4 (zero three quarters), n_cols - 1 (no padding to speak of:
the API wants n_per_row < n_cols), and a ragged length whose last row is short; 1 and 3 rows.  The switch is read when an encoder is
created, so both forms live in one process; test_forms_agree_across_processes sets it before the child starts instead.  The worst-case
row (every low limb of the limb form at 2^29 - 1, and p - 1) is held to a Python-int transform computed here."""
import os
import random
import subprocess
import sys

import numpy as np
import pytest

from common import field_p, ntt_maxlimb, ntt_root, to_limbs
from lcpc_amd import LcCommit, LigeroEncoding

pytestmark = pytest.mark.gpu
FID = 3


def _enc(form, n_per_row, n_cols, rho):
    os.environ["LCPC_NTT_FORM"] = form                   # (switches are read once, when an encoder is created)
    try:
        return LigeroEncoding.new_from_dims(FID, n_per_row, n_cols, rho=rho)
    finally:
        del os.environ["LCPC_NTT_FORM"]


FILLS = {"half": lambda n: (n // 2, (1, 2), 3, 0), "quarter": lambda n: (n // 4, (1, 4), 1, 0),
         "full": lambda n: (n - 1, (38, 39), 1, 0), "ragged": lambda n: (n // 2 - 3, (1, 2), 3, 1)}


@pytest.mark.parametrize("log_n", [11, 12, 13, 15, 18, 20])
@pytest.mark.parametrize("fill", list(FILLS))
def test_coset_form_is_the_oracle_and_the_dif_form(oracle, log_n, fill):
    O = oracle
    n_cols = 1 << log_n
    n_per_row, rho, n_rows, ragged = FILLS[fill](n_cols)
    n = n_rows * n_per_row - (n_per_row - max(1, n_per_row // 3) if ragged else 0)
    coeffs = O.random_elems(FID, n, log_n * 11 + len(fill))
    oc = O.Commit.commit(coeffs, O.Encoding.ligero_from_dims(FID, n_per_row, n_cols, rho=rho), n_threads=8)
    rows = np.zeros((n_rows * n_cols, 4), np.uint64)
    for r in range(n_rows):
        seg = coeffs[r * n_per_row:(r + 1) * n_per_row]
        rows[r * n_cols:r * n_cols + len(seg)] = seg
    got = {}
    for form in ("coset", "dif"):
        enc = _enc(form, n_per_row, n_cols, rho)
        c = LcCommit.commit(coeffs, enc)
        assert (c.comm() == oc.comm()).all(), form
        assert (c.hashes() == oc.hashes()).all() and c.get_root() == oc.get_root(), form
        assert (c.coeffs() == oc.coeffs()).all(), form
        got[form] = enc.encode(rows)
    assert (got["coset"] == got["dif"]).all()
    # encode is the Montgomery-output path: the oracle's comm is in the same form
    assert (got["coset"] == oc.comm()).all()


CHILD = """
import hashlib, os, sys
sys.path[:0] = %r
import oracle_lib as O
from lcpc_amd import LcCommit, LigeroEncoding
for log_n in (13, 18):
    n_cols, n_per_row = 1 << log_n, 1 << (log_n - 1)
    coeffs = O.random_elems(3, n_per_row, log_n)
    c = LcCommit.commit(coeffs, LigeroEncoding.new_from_dims(3, n_per_row, n_cols))
    print(log_n, c.get_root().hex(), hashlib.sha256(c.comm().tobytes()).hexdigest())
"""


def test_forms_agree_across_processes(oracle):
    """the variable set before the process starts, one fresh child per value: same root and same comm bytes, at an odd first pass
    (2^13) and at the headline's shape"""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    paths = [root, os.path.join(root, "tests"), os.path.join(root, "oracle")]
    outs = {}
    for form in ("coset", "dif"):
        env = dict(os.environ, LCPC_NTT_FORM=form)
        r = subprocess.run([sys.executable, "-c", CHILD % (paths,)], capture_output=True, text=True, env=env, timeout=300)
        assert r.returncode == 0, r.stderr[-3000:]
        outs[form] = r.stdout.split("\n")
    assert outs["coset"] == outs["dif"] and len(outs["coset"]) >= 2
    O = oracle
    for line in outs["coset"][:2]:
        log_n, root_hex, _ = line.split()
        n_per_row = 1 << (int(log_n) - 1)
        oc = O.Commit.commit(O.random_elems(3, n_per_row, int(log_n)), O.Encoding.ligero_from_dims(3, n_per_row, 2 * n_per_row), n_threads=8)
        assert oc.get_root().hex() == root_hex


def _ntt_ints(x, k, w, p):
    """radix-2 DIF on Python ints, natural in, bit-reversed out (the reference's loop), from a table of w^i"""
    n = 1 << k
    tab = [1] * (n // 2)
    for i in range(1, n // 2):
        tab[i] = tab[i - 1] * w % p
    for s in range(k):
        gap = n >> (s + 1)
        for off in range(0, n, 2 * gap):
            for i in range(gap):
                a, b = x[off + i], x[off + i + gap]
                x[off + i], x[off + i + gap] = (a + b) % p, (a - b) * tab[i << s] % p
    return x


def test_worst_case_operands_headline_shape():
    """2^18 columns, one row, stored limbs at their extremes: the element whose eight low 29-bit limbs are all ones, p - 1 every 7th,
    random every 16th (so that a misplaced twiddle shows).  The transform acts on the stored (Montgomery) residues with plain twiddles,
    so encode's output is the integer transform of the stored values, and so is the comm that commit hands back (it keeps canonical values
    on the device -- the converting twiddles and the multiplies by 2^5 run there -- and returns the stored form); the bounds written
    in ntt_l9s.hip's coset rounds (|value| < 12.1p before the clamps, limbs inside (-2^30, 2^30)) are what these operands push."""
    log_n = 18
    p, n = field_p(FID), 1 << log_n
    n_per_row = n // 2
    rnd = random.Random(18)
    vals = [ntt_maxlimb(FID)] * n_per_row
    for i in range(4, n_per_row, 7):
        vals[i] = p - 1
    for i in range(9, n_per_row, 16):
        vals[i] = rnd.randrange(p)
    coeffs = to_limbs(vals, 4)
    want = _ntt_ints(vals + [0] * (n - n_per_row), log_n, ntt_root(FID, log_n), p)
    rows = np.zeros((n, 4), np.uint64)
    rows[:n_per_row] = coeffs
    b = b"".join(v.to_bytes(32, "little") for v in want)
    want_m = np.frombuffer(b, np.uint64).reshape(n, 4)
    for form in ("coset", "dif"):
        enc = _enc(form, n_per_row, n, (1, 2))
        assert (enc.encode(rows) == want_m).all(), form
        assert (LcCommit.commit(coeffs, enc).comm() == want_m).all(), form

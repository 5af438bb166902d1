"""The column hash of every digest behind the row-NTT switches.  LCPC_NTT_GENERAL and LCPC_NTT_MID_MAX_MB are read when a context is
created; they decide which kernels encode a Ligero row and, for Ft63 / Ft127 / Ft191, whether comm stays canonical on the device
-- that is LeafArgs::canon_in, i.e. which <NL, CANON> instantiation of sha3_leaf_kernel / blake2b_leaf_kernel / the BLAKE3 leaf
kernels hashes it (lcpc_amd/csrc/ctx.cpp comm_canon, commit.cpp).  One Ligero shape per field, the smallest n_cols with a two-pass
limb plan, under each switch and each digest, in a fresh child process with a time limit: whole `hashes` array, proof bytes and
verify's evaluation against the digest-generic reference (tests/digest_ref.py).

Which instantiation a case takes is asserted from the plan as tests/common.py restates it (ntt_plan, pinned to the library's
launches by tests/test_gpu_ntt_shapes.py); the table at the end of the module states what the matrix must reach."""
import json
import os
import subprocess
import sys

import pytest

import digest_ref as DR
from common import FIRST_TWO_PASS, ntt_plan

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N_ROWS = 3
SWITCHES = {"default": {}, "general": {"LCPC_NTT_GENERAL": "1"}, "mid0": {"LCPC_NTT_MID_MAX_MB": "0"}, "mid1": {"LCPC_NTT_MID_MAX_MB": "1"}}

CHILD = r"""
import json, sys
sys.path[:0] = [%r, %r, %r]
import oracle_lib as O
import digest_ref as DR
out = []
for fid, log_n in %r:
    n_cols = 1 << log_n
    oenc = O.Encoding.ligero_from_dims(fid, n_cols // 2, n_cols)
    coeffs = DR.edge_elems(O, fid, %d * (n_cols // 2) - 5, 40 + fid)
    for digest in DR.DIGEST_NAMES:
        enc = DR.make_enc("ligero", fid, 0, digest, dims=(n_cols // 2, n_cols))
        rc = DR.RefCase(O, oenc, coeffs, digest)
        DR.check_case(rc, enc, "%%s ft%%d 2^%%d" %% (digest, fid, log_n))
        out.append([fid, digest])
print("DONE " + json.dumps(out))
"""


def plan_facts(fid, name):
    """(canon_in, limb intermediate on) of the field's shape under a switch, from the plan restatement"""
    log_n = FIRST_TWO_PASS[fid]
    general = name == "general"
    mid_mb = {"mid0": 0, "mid1": 1}.get(name)
    plan = ntt_plan(fid, log_n, general, mid_mb, N_ROWS)
    return DR.leaf_canon_in(fid, "ligero", log_n, N_ROWS, general), bool(plan[0]["mid"]), plan[0]["kernel"]


@pytest.mark.parametrize("name", list(SWITCHES))
def test_digests_behind_ntt_switches(name):
    shapes = [(fid, FIRST_TWO_PASS[fid]) for fid in range(4)]
    env = {k: v for k, v in os.environ.items() if k not in ("LCPC_NTT_GENERAL", "LCPC_NTT_MID_MAX_MB")}
    env.update(SWITCHES[name])
    code = CHILD % (ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "oracle"), shapes, N_ROWS)
    r = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    done = json.loads(r.stdout.split("DONE ", 1)[1])
    assert sorted(map(tuple, done)) == sorted((fid, d) for fid in range(4) for d in DR.DIGEST_NAMES)
    # what this switch makes of each field's shape
    for fid in range(4):
        canon, mid, kernel = plan_facts(fid, name)
        assert kernel == ("general" if name == "general" else "K1s" if fid == 3 else "K1n")
        assert canon == (fid == 3 or name != "general")
        assert mid == (fid == 3 and name in ("default", "mid1"))


def test_switch_matrix_reaches_both_leaf_instantiations():
    """<NL, CANON = true> and <NL, false> for NL = 2, 4, 6 (Ft63 / Ft127 / Ft191); Ft255 Ligero is always canonical (its
    <8, false> runs for Brakedown below 24 rows: tests/test_gpu_digests_edges.py::test_block_edges_brakedown has no Ft255 case
    there, tests/test_gpu_digests_verify.py's Brakedown shape is Ft127 -- so state it here and cover it in from_parts, whose
    Brakedown Ft255 commitment has 6 rows); the limb intermediate on and off for Ft255"""
    reach = {(fid, plan_facts(fid, name)[0]) for fid in range(4) for name in SWITCHES}
    assert reach == {(0, True), (0, False), (1, True), (1, False), (2, True), (2, False), (3, True)}
    assert {plan_facts(3, name)[1] for name in SWITCHES} == {True, False}
    assert not DR.leaf_canon_in(3, "sdig", 0, 6) and DR.leaf_canon_in(3, "sdig", 0, 24)

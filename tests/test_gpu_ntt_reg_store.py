"""K1s rounds that store from the registers (lcpc_amd/csrc/ntt_l9s.hip, ntt_ln_dev.h clamp_store): the pure first pass's I-only round
(packed intermediate: each of its four outputs clamped once, packed and stored, no LDS round trip) and the final rounds of both last
passes (coset form r == 4, DIF form last_two), which clamp their outputs as the butterfly leaves them, un-normalised.  Every commit
is held to the oracle bit for bit through the public path: comm, hashes and root through LcCommit.commit (canonical output) and the
Montgomery-form rows through enc.encode.

Plans (the switches are read when an encoder is created, so all of them live in one process):
  * 2^16 .. 2^20 columns, the default plan: pure first pass of S = 6 .. 10 stages on the packed intermediate, coset last pass; under
    LCPC_NTT_MUL=split and =mont (2^18 x split: the headline's two instantiations);
  * 2^12 .. 2^15 columns with LCPC_NTT_FORM=coset: S = 2 .. 5 -- S = 2 is the first pass whose storing round is its first round (the
    barrier in front of its clamps), S = 3 and 5 have a radix-2 round in front.  Below 2^16 columns the limb intermediate is the
    default, so each runs twice: with it (the coset last pass's limb-tile instantiation) and with LCPC_NTT_MID_MAX_MB=0 (the packed
    intermediate: the first pass's register store); split and mont;
  * 2^11 .. 2^15 columns, the default plan (DIF form): the DIF last pass's last_two store, with the limb and the packed intermediate.
Rows and fills: 1 and 3 rows; a quarter, a half and n_cols - 1 coefficients per row (the rate <= 1/4 path, the zero-padded path and
the general first round).

Crafted inputs (tests/common.py stage_input_rows): rows whose values entering a DIF stage are all p - 1, alternating 0 / p - 1, or the
element whose low limbs are all 2^29 - 1, at the two stages of the first pass's storing round (S - 2, S - 1) and at the last two
stages of the row: the values that put the un-normalised clamp inputs at their extremes.

The limb-intermediate form of the first pass's register store was not built (LABNOTES.md), so no LCPC_NTT_MID_MAX_MB=64 case."""
import os

import numpy as np
import pytest

from common import field_p, ntt_maxlimb, stage_input_rows
from lcpc_amd import LcCommit, LigeroEncoding

pytestmark = pytest.mark.gpu
FID = 3
SWITCHES = ("LCPC_NTT_MUL", "LCPC_NTT_FORM", "LCPC_NTT_MID_MAX_MB")


def plans(log_n):
    """the encoder switches of every plan the module's head names for 2^log_n columns"""
    if log_n >= 16:
        return [{"LCPC_NTT_MUL": "split"}, {"LCPC_NTT_MUL": "mont"}]
    out = [{}, {"LCPC_NTT_MID_MAX_MB": "0"}]
    if log_n >= 12:
        for mul in ("split", "mont"):
            out.append({"LCPC_NTT_FORM": "coset", "LCPC_NTT_MUL": mul})
            out.append({"LCPC_NTT_FORM": "coset", "LCPC_NTT_MUL": mul, "LCPC_NTT_MID_MAX_MB": "0"})
    return out


def _enc(env, n_per_row, n_cols, rho):
    saved = {k: os.environ.pop(k, None) for k in SWITCHES}
    os.environ.update(env)                               # (switches are read once, when an encoder is created)
    try:
        return LigeroEncoding.new_from_dims(FID, n_per_row, n_cols, rho=rho)
    finally:
        for k in SWITCHES:
            os.environ.pop(k, None)
            if saved[k] is not None:
                os.environ[k] = saved[k]


FILLS = {"quarter": lambda n: (n // 4, (1, 4)), "half": lambda n: (n // 2, (1, 2)), "full": lambda n: (n - 1, (38, 39))}


def _check(O, coeffs, n_rows, n_per_row, n_cols, rho, what):
    oc = O.Commit.commit(coeffs, O.Encoding.ligero_from_dims(FID, n_per_row, n_cols, rho=rho), n_threads=16)
    want, want_hashes, want_root = oc.comm(), oc.hashes(), oc.get_root()
    rows = np.zeros((n_rows, n_cols, 4), np.uint64)
    rows[:, :n_per_row] = coeffs.reshape(n_rows, n_per_row, 4)
    rows = rows.reshape(-1, 4)
    for env in plans(n_cols.bit_length() - 1):
        enc = _enc(env, n_per_row, n_cols, rho)
        c = LcCommit.commit(coeffs, enc)
        assert (c.comm() == want).all(), (what, env, "comm")
        assert (c.hashes() == want_hashes).all() and c.get_root() == want_root, (what, env, "root")
        assert (enc.encode(rows) == want).all(), (what, env, "encode")     # the Montgomery-output path: the oracle's comm is in that form


@pytest.mark.parametrize("n_rows", [1, 3])
@pytest.mark.parametrize("fill", list(FILLS))
@pytest.mark.parametrize("log_n", list(range(11, 21)))
def test_register_stores_are_the_oracle(oracle, log_n, fill, n_rows):
    O = oracle
    n_cols = 1 << log_n
    n_per_row, rho = FILLS[fill](n_cols)
    coeffs = O.random_elems(FID, n_rows * n_per_row, log_n * 11 + len(fill) + n_rows)
    _check(O, coeffs, n_rows, n_per_row, n_cols, rho, (log_n, fill, n_rows))


def crafted_stages(log_n):
    """the two stages of the first pass's storing round and the last two of the row"""
    S = log_n - 10
    return sorted({s for s in (S - 2, S - 1, log_n - 2, log_n - 1) if s >= 0})


@pytest.mark.parametrize("log_n", list(range(11, 21)))
def test_register_stores_at_crafted_stage_inputs(oracle, log_n):
    """one row per (pattern, stage); rate 1/2"""
    O = oracle
    p, n = field_p(FID), 1 << log_n
    pats = [[p - 1], [0, p - 1], [ntt_maxlimb(FID)]]
    rows = np.concatenate([stage_input_rows(FID, log_n, crafted_stages(log_n), pat, 1) for pat in pats])
    _check(O, rows.reshape(-1, 4), rows.shape[0], n // 2, n, (1, 2), (log_n, "crafted"))


def test_plans_and_stages_cover_what_the_head_names():
    assert [len(plans(k)) for k in (11, 12, 15, 16, 20)] == [2, 6, 6, 2, 2]
    assert crafted_stages(11) == [0, 9, 10] and crafted_stages(12) == [0, 1, 10, 11] and crafted_stages(18) == [6, 7, 16, 17]

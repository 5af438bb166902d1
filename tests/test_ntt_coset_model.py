"""K1s's pure / coset factorisation (lcpc_amd/csrc/ntt_l9s.hip, NttPassArgs.form == 1) as a Python-integer model: the pure first pass,
then the coset last pass, with every twiddle taken by the index rules of the pack builders (tests/ntt_coset_rules.py restates them).
Exact arithmetic makes any stage grouping give the reference's bits; what it does not cover is the mapping tile -> coset and
sub-block -> twiddle, bit reversals included.  That mapping is what this test pins, against the definition
X[pos] = sum_i x_i w^(i bitrev(pos)) (the reference's order: natural in, bit-reversed out) and against the radix-2 DIF of
tests/common.py, for Ft255 at 2^11 .. 2^14 columns, tiles shrunk by a parameter, rates 1/2, 1/4 and 1, odd and even first passes."""
import random

import pytest

import ntt_coset_rules as R
from common import dif_stage, field_p, ntt_root

FID = 3

# (log n, log tile): the kernels' tile (10) where the model stays fast, smaller tiles for the longer first passes.
# S = log n - log tile covers 1 .. 10: the radix-2 peel alone (1), the I-only round alone (2), both (3), one pack round (4, 5),
# the uniform round (6 .. 10)
CASES = [(11, 10), (11, 6), (11, 4), (12, 10), (12, 6), (12, 4), (13, 10), (12, 8), (13, 4), (14, 4), (12, 2)]


def _row(k, n_valid, seed):
    rnd = random.Random(seed)
    p = field_p(FID)
    return [rnd.randrange(p) if i < n_valid else 0 for i in range(1 << k)]


def test_cases_cover_every_first_pass():
    assert {k - lt for k, lt in CASES} >= set(range(1, 11))
    assert {(11, 10), (12, 10), (13, 10)} <= set(CASES)                     # the kernels' own tile at 2^11, 2^12, 2^13
    assert {(k - lt) & 1 for k, lt in CASES} == {0, 1}


def test_shape_rules():
    """PureShape: distinct twiddle sets per radix-4 round 4^(NR4-1) .. 4, 1; the uniform round is the one with 4 sets and exists only
    behind a round that reads the pack, which is the converting round RC"""
    for S in range(1, 11):
        u0, nr4, sets, ru, rc = R.pure_shape(S)
        assert sets == [4 ** (nr4 - 1 - r) for r in range(nr4)]
        if ru >= 0:
            assert sets[ru] == 4 and rc == ru - 1 and sets[rc] == 16
        else:
            assert nr4 <= 2 and rc == (0 if nr4 == 2 else -1)
    # the headline, 8 + 10: lane-varying rounds 2 + 3, uniform 1 + 2, I-only 1 + 0
    assert R.pure_shape(8)[2] == [64, 16, 4, 1]


@pytest.mark.parametrize("k,lt", CASES, ids=["2^%d-tile2^%d" % c for c in CASES])
@pytest.mark.parametrize("rate", ["1/2", "1/4", "1"])
def test_model_is_the_dft(k, lt, rate):
    p, w, n = field_p(FID), ntt_root(FID, k), 1 << k
    n_valid = {"1/2": n // 2, "1/4": n // 4, "1": n}[rate]
    x = _row(k, n_valid, 100 * k + lt)
    fourth = pow(w, n // 4, p)
    got = R.run(list(x), k, lt, w, p, fourth)
    want = list(x)
    for s in range(k):
        dif_stage(want, s, w, p)
    assert got == want
    # the definition itself, at the corners and a few random positions (every position at 2^11 is ~2 M modular multiplies: too slow here)
    rnd = random.Random(k)
    for pos in [0, 1, n - 1, (1 << lt) - 1, 1 << lt] + [rnd.randrange(n) for _ in range(3)]:
        wj = pow(w, R.brev(pos, k), p)
        acc = 0
        for v in reversed(x[:n_valid]):
            acc = (acc * wj + v) % p
        assert got[pos] == acc, pos


def test_coset_exponents_stay_in_the_table():
    """E < n / 4, so the triple's largest index 3 E < n: one negation at most (ntt_lns.hip tab_entry_neg); round 0 is one triple per
    tile, and tile 0 (g = 1) multiplies by 1 there"""
    for k in (11, 15, 18, 20):
        S = k - 10
        for cls in {0, 1, (1 << S) - 1, (1 << S) // 2}:
            for r in range(5):
                for m in {0, 1, 4 ** r - 1}:
                    if m < 4 ** r:
                        assert 0 <= R.coset_exp(k, 10, cls, r, m) < (1 << (k - 2))
        assert R.coset_exp(k, 10, 0, 0, 0) == 0

"""The case builder of tests/k7_harness.py against Python-int dot products of oracle/pyref.py's fields, the harness's own argument
checks, and the separation of lib/liblcpc_k7_harness.so from the product.  No GPU."""
import numpy as np
import pytest

import k7_harness as H
import pyref as P
from common import to_int
from test_abi import _harness_is_a_separate_library


def test_k7_harness_is_a_separate_library():
    """lib/liblcpc_k7_harness.so (tests/native/k7_harness.cpp) exports the k7h_* entry points of tests/k7_harness.py and nothing of the
    product, which it links against instead of carrying a copy"""
    _harness_is_a_separate_library("k7_harness", "k7h_", "tests/native/k7_harness.cpp", "K7H_OUT")


@pytest.mark.parametrize("fid", [0, 1, 2, 3])
def test_expected_dots_are_the_field_dot_products(fid):
    """Case.dot is the stored form of sum_k tensor[k] * column[k] over the field, by canonical bignum arithmetic; the builder puts it
    into the encoded rows at the drawn column, so the honest case expects all-zero status"""
    F = P.FIELDS[fid]
    c = H.Case(fid, n_rows=61, n_t=3, n_cols=16, drawn=[[0, 15, 7, 7], [3, 3, 9, 1]], seed=fid + 1)
    for m in range(2):
        for i in range(4):
            for d in range(3):
                want = sum(F.from_mont(t) * F.from_mont(x) for t, x in zip(c.tensors[m][d], c.cols[m][i])) % F.p
                assert F.from_mont(c.dot(m, i, d)) == want
                assert c.enc[m][d][c.drawn[m][i]] == c.dot(m, i, d)
    assert c.cols[0][2] == c.cols[0][3] and c.cols[0][0] != c.cols[0][1]       # one column number, one column
    assert not c.expected().any()


def test_expected_status_bits():
    c = H.Case(3, n_rows=8, n_t=3, n_cols=8, drawn=[[0, 1, 2, 3, 9]])
    c.plant(0, 1, 0)                  # a degree-test row
    c.plant(0, 2, 2)                  # the eval row (the last tensor)
    c.plant(0, 3, 1)
    c.plant(0, 3, 2)
    assert c.expected().tolist() == [[0, H.DEGREE_BIT, H.EVAL_BIT, H.DEGREE_BIT | H.EVAL_BIT, H.DEGREE_BIT | H.EVAL_BIT]]
    one = H.Case(0, n_rows=1, n_t=1, n_cols=4, drawn=[[4, 0]])
    one.plant(0, 1, 0)
    assert one.expected().tolist() == [[H.EVAL_BIT, H.EVAL_BIT]]               # n_t == 1: the only tensor is the eval tensor


def test_arrays_layout_and_fills():
    c = H.Case(2, n_rows=5, n_t=2, n_cols=4, drawn=[[1, 2], [0, 3], [2, 2]], stride=13, fill="max")
    cols, tensors, enc, drawn = c.arrays()
    assert cols.shape == (3, 13, 3) and tensors.shape == (3, 2, 5, 3) and enc.shape == (3, 2, 4, 3) and drawn.shape == (3, 2)
    assert all(to_int(cols[m, k]) == c.p - 1 for m in range(3) for k in range(10))
    assert (cols[:, 10:] == np.uint64(H.POISON)).all()                          # the gap behind a member's columns
    assert all(to_int(tensors[m, d, k]) == c.p - 1 for m in range(3) for d in range(2) for k in range(5))
    assert to_int(enc[1, 1, 3]) == c.dot(1, 1, 1) == 5 * (c.p - 1) ** 2 * pow(1 << 192, -1, c.p) % c.p
    z = H.Case(0, n_rows=3, n_t=1, n_cols=2, drawn=[[1]], fill="zero")
    assert z.dot(0, 0, 0) == 0 and not z.arrays()[0].any()


def test_harness_refuses_what_it_cannot_bound():
    """tests/native/k7_harness.cpp checks its arguments before it touches the device: no GPU is needed to refuse"""
    a = np.zeros((1, 4, 1), np.uint64)
    d = np.zeros((1, 1), np.uint64)
    s = np.zeros((1, 1), np.uint32)
    f = H.lib().k7h_verify_columns
    ok = dict(nl=2, stride=4, n_rows=4, n_cols=4, n_open=1, n_t=1, n_batch=1)
    for bad in (dict(nl=3), dict(stride=3), dict(n_rows=0), dict(n_cols=0), dict(n_open=0), dict(n_t=0), dict(n_batch=0), dict(n_batch=65536)):
        k = dict(ok, **bad)
        rc = f(k["nl"], H._ptr(a), k["stride"], H._ptr(a), H._ptr(a), H._ptr(d), H._ptr(s), k["n_rows"], k["n_cols"], k["n_open"], k["n_t"],
               k["n_batch"])
        assert rc == -1, bad
    with pytest.raises(H.BadArgs):
        H.refusal(3, 1, 1, 1)         # a job the launcher would launch


@pytest.mark.parametrize("fid", [0, 1, 2, 3])
def test_launcher_settles_empty_and_oversized_jobs_before_any_launch(fid):
    assert H.refusal(fid, 0, 5, 2) == H.HIP_SUCCESS                  # no member
    assert H.refusal(fid, 3, 0, 2) == H.HIP_SUCCESS                  # no opened column
    assert H.refusal(fid, 65536, 5, 2) == H.HIP_ERROR_INVALID_VALUE  # more members than grid y
    assert H.refusal(fid, 3, 5, 0) == H.HIP_ERROR_INVALID_VALUE      # no tensor
    if fid == 3:
        assert H.refusal(fid, 3, 5, 2, limb=False) == H.HIP_ERROR_INVALID_VALUE   # Ft255 without the 29-bit-limb tensors

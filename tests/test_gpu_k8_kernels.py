"""K8b, the Merkle path folds of the batched verify and the column check (kernels.h launch_fold_paths_b3 / launch_chain_fold_paths),
directly against the reference digests (tests/k8_harness.py Case, itself checked by tests/test_k8_cases.py), for all five digests.

One lane folds one opened column, 256 lanes to a workgroup, the member in grid y: so the column counts are a single lane, one short of
a wave, a wave, one past it and one past a workgroup; the depths are no level at all (the leaf digest is compared with the root), one,
two and a tree of 2048 leaves; one member and three; and both sibling layouts.  Every member's buffers end in poison the kernel owns
no word of."""
import numpy as np
import pytest

import k8_harness as K8

gpu = pytest.mark.gpu
OK, INVALID = K8.HIP_SUCCESS, K8.HIP_ERROR_INVALID_VALUE
DEPTHS = [0, 1, 2, 11]
N_OPENS = [1, 63, 64, 65, 257]


def drawn_for(depth, n_open, n_batch):
    base = K8.column_numbers(depth, n_open)
    return [base[m:] + base[:m] for m in range(n_batch)]          # (each member draws them in another order)


def check(case, prefill=0):
    got = case.run(prefill)
    want = case.expected() | np.asarray(prefill, np.uint32)
    assert np.array_equal(got, want), np.argwhere(got != want)[:8].tolist()
    return got


@gpu
@pytest.mark.parametrize("depth", DEPTHS)
@pytest.mark.parametrize("name", K8.DIGESTS)
def test_honest_paths_at_every_shape(name, depth):
    """nothing is flagged, and nothing but the lanes' own status words is written, at every column count, member count and layout"""
    for n_open in N_OPENS:
        for n_batch in (1, 3):
            for layout in K8.LAYOUTS:
                c = K8.Case(name, depth, drawn_for(depth, n_open, n_batch), layout, gap=8)
                assert not check(c).any(), (n_open, n_batch, layout)


def faults(depth):
    """(what, plant(case)) -> the lanes that must be flagged; lane (member 1, column 40) unless the fault is a member's"""
    m, k = 1, 40
    out = [("leaf digest", lambda c: c.flip_leaf(m, k, bit=77), [(m, k)]),
           ("a member's root", lambda c: c.flip_root(2, bit=5), [(2, j) for j in range(65)])]
    if depth:
        out += [("level-0 sibling", lambda c: c.flip_sibling(m, k, 0, bit=1), [(m, k)]),
                ("last-level sibling", lambda c: c.flip_sibling(m, k, depth - 1, bit=8 * c.dl - 1), [(m, k)])]
    if depth >= 2:
        out += [("two siblings exchanged", lambda c: c.swap_siblings(m, k, 0, depth - 1), [(m, k)])]
    return out


@gpu
@pytest.mark.parametrize("layout", K8.LAYOUTS)
@pytest.mark.parametrize("depth", DEPTHS)
@pytest.mark.parametrize("name", K8.DIGESTS)
def test_each_fault_sets_the_path_bit_of_exactly_its_lane(name, depth, layout):
    for what, plant, lanes in faults(depth):
        c = K8.Case(name, depth, drawn_for(depth, 65, 3), layout, gap=4)
        plant(c)
        got = check(c)
        want = np.zeros((3, 65), np.uint32)
        for m, k in lanes:
            want[m, k] = K8.PATH_BIT
        assert np.array_equal(got, want), what


@gpu
@pytest.mark.parametrize("layout", K8.LAYOUTS)
@pytest.mark.parametrize("name", K8.DIGESTS)
def test_bits_of_the_column_check_are_kept(name, layout):
    """status words that hold 0, 1, 2 and 3 keep those bits, with and without the path bit beside them"""
    depth, n_open = 2, 257
    c = K8.Case(name, depth, drawn_for(depth, n_open, 3), layout, gap=8)
    for k in (0, 1, 2, 3, 64, 255, 256):
        c.flip_sibling(k % 3, k, k % depth, bit=k)
    prefill = (np.arange(3 * n_open, dtype=np.uint32).reshape(3, n_open) // 2) % 4
    got = check(c, prefill)
    assert int((got & K8.PATH_BIT).sum()) == 7 * K8.PATH_BIT and np.array_equal(got & 3, prefill)


@gpu
def test_a_number_drawn_twice_is_two_lanes():
    """the same leaf opened twice: a fault in one opening's path leaves the other alone"""
    for name in K8.DIGESTS:
        c = K8.Case(name, 11, [[1365, 7, 1365, 2047]], "column")
        c.flip_sibling(0, 2, 5, bit=9)
        assert check(c)[0].tolist() == [0, 0, K8.PATH_BIT, 0]


@pytest.mark.parametrize("name", K8.DIGESTS)
def test_launcher_refusals(name):
    """what the launchers settle before any launch, on null or never-read buffers: no device is touched"""
    assert K8.refusal(name, 0, 5, 3) == INVALID and K8.refusal(name, 65536, 5, 3) == INVALID
    assert K8.refusal(name, 0, 0, 3) == INVALID and K8.refusal(name, 65536, 0, 3) == INVALID      # (before the empty job)
    assert K8.refusal(name, 1, 5, 64) == INVALID and K8.refusal(name, 1, 0, 64) == INVALID
    for bit in range(5):
        assert K8.refusal(name, 1, 5, 3, 1 << bit) == INVALID, bit
        assert K8.refusal(name, 1, 0, 3, 1 << bit) == OK, bit                                      # no column: nothing is read
    assert K8.refusal(name, 1, 5, 0, 1 << 2) == INVALID                                            # no level either: still a pointer
    assert K8.refusal(name, 1, 0, 63) == OK and K8.refusal(name, 65535, 0, 0, 31) == OK
    with pytest.raises(K8.BadArgs):
        K8.refusal(name, 1, 5, 3)                 # a job a correct launcher would launch is not for this entry point


def test_harness_refuses_what_it_cannot_bound():
    """tests/native/k8_harness.cpp checks every index the kernel will form before it touches the device"""
    c = K8.Case("sha256", 2, [[0, 3, 1]], "level", gap=4)
    leaves, drawn, sibs, roots, status = c.arrays()
    ls, sm, sc, sl, ss = c.strides()
    f, P = K8.lib().k8h_fold_paths, K8._ptr
    ok = dict(d=3, lw=leaves.size, ls=ls, sw=sibs.size, sm=sm, sc=sc, sl=sl, stw=status.size, ss=ss, n_open=3, depth=2, n_batch=1)
    for bad in (dict(d=5), dict(d=-1), dict(n_batch=0), dict(n_batch=65536), dict(n_open=0), dict(depth=64), dict(lw=23), dict(sw=47),
                dict(stw=2), dict(ls=6), dict(sc=9), dict(sl=25), dict(n_batch=2), dict(depth=3), dict(n_open=4), dict(lw=1 << 27)):
        k = dict(ok, **bad)
        rc = f(k["d"], P(leaves), k["lw"], k["ls"], P(drawn), P(sibs), k["sw"], k["sm"], k["sc"], k["sl"], P(roots), P(status), k["stw"], k["ss"],
               k["n_open"], k["depth"], k["n_batch"])
        assert rc == -1, bad
    assert f(3, None, leaves.size, ls, P(drawn), P(sibs), sibs.size, sm, sc, sl, P(roots), P(status), status.size, ss, 3, 2, 1) == -1

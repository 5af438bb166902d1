"""The case builder of tests/k8_harness.py against real trees, on the CPU: what tests/test_gpu_k8_kernels.py expects of K8b is only as
good as the builder's own fold.  Trees over 8 and over 5 leaves (not a power of two: the slots behind the last leaf are zero digests)
under all five digests; for SHA3-256 and BLAKE2b the tree, the paths and the fold are also held to the second, independent statement
of tests/sha3_ref.py / tests/blake2b_ref.py (digest_ref.tree_ref)."""
import hashlib
import random

import numpy as np
import pytest

import digest_ref as DR
import k8_harness as K8


def _leaves(name, n, seed=7):
    rng = random.Random(seed)
    dl = DR.DLEN[name]
    return [rng.getrandbits(8 * dl).to_bytes(dl, "little") for _ in range(n)]


@pytest.mark.parametrize("name", K8.DIGESTS)
@pytest.mark.parametrize("n", [8, 5])
def test_every_leaf_folds_to_the_root(name, n):
    leaves = _leaves(name, n)
    hashes, np2 = K8.tree(name, leaves)
    assert np2 == 8 and len(hashes) == 15
    assert hashes[n:8] == [bytes(DR.DLEN[name])] * (8 - n)
    ref = DR.tree_ref(name)
    if ref is not None:
        assert ref.tree(leaves) == hashes
    for col in range(n):
        sibs = K8.path(hashes, np2, col)
        assert len(sibs) == 3
        assert K8.fold(name, leaves[col], col, sibs) == hashes[-1]
        if ref is not None:
            assert ref.path(hashes, np2, col) == sibs and ref.fold(leaves[col], col, sibs) == hashes[-1]
        # the wrong column number, a wrong sibling: not the root
        assert K8.fold(name, leaves[col], col ^ 1, sibs) != hashes[-1]
        assert K8.fold(name, leaves[col], col, sibs[::-1]) != hashes[-1] or sibs == sibs[::-1]


def test_the_hashlib_digests_are_hashlib():
    msg = bytes(range(64))
    assert K8.digest("sha3_256")(msg) == hashlib.sha3_256(msg).digest()
    assert K8.digest("sha256")(msg) == hashlib.sha256(msg).digest()
    assert K8.digest("blake2b")(msg) == hashlib.blake2b(msg, digest_size=64).digest()
    assert K8.digest("keccak256")(b"abc").hex() == "4e03657aea45a94fc7d47ba826c8d667c0d1e6e33a64a036ec44f58fa12d6c45"
    assert K8.digest("blake3")(b"").hex() == "af1349b9f5f9a1a6a0404dea36dcc9499bcb25c9adc112b7cc9a93cae41f3262"


@pytest.mark.parametrize("name", K8.DIGESTS)
@pytest.mark.parametrize("layout", K8.LAYOUTS)
def test_each_planted_fault_flips_exactly_its_column(name, layout):
    depth, drawn = 3, [[0, 7, 5, 2, 5], [4, 4, 1, 6, 3]]
    honest = K8.Case(name, depth, drawn, layout)
    assert not honest.expected().any()

    def only(case, lanes):
        want = np.zeros((2, 5), np.uint32)
        for m, k in lanes:
            want[m, k] = K8.PATH_BIT
        assert np.array_equal(case.expected(), want)

    c = K8.Case(name, depth, drawn, layout)
    c.flip_sibling(0, 1, 0, bit=3)
    only(c, [(0, 1)])
    c = K8.Case(name, depth, drawn, layout)
    c.flip_sibling(1, 3, depth - 1, bit=8 * c.dl - 1)
    only(c, [(1, 3)])
    c = K8.Case(name, depth, drawn, layout)
    c.flip_leaf(0, 2, bit=17)                  # column 5 is drawn twice: the other opening keeps its own, intact copy
    only(c, [(0, 2)])
    c = K8.Case(name, depth, drawn, layout)
    c.flip_root(1, bit=100)
    only(c, [(1, k) for k in range(5)])
    c = K8.Case(name, depth, drawn, layout)
    c.swap_siblings(0, 3, 0, 2)
    only(c, [(0, 3)])


@pytest.mark.parametrize("layout", K8.LAYOUTS)
def test_arrays_place_every_digest_where_the_strides_say(layout):
    c = K8.Case("blake2b", 2, [[0, 3, 1], [2, 2, 0]], layout, gap=8)
    leaves, drawn, sibs, roots, status = c.arrays(prefill=3)
    ls, sm, sc, sl, ss = c.strides()
    assert leaves.shape == (2, ls) and sibs.shape == (2, sm) and status.shape == (2, ss) and roots.shape == (2, 16)
    for m in range(2):
        for k in range(3):
            assert leaves[m, k * 16:(k + 1) * 16].tobytes() == c.leaves[m][k]
            for lvl in range(2):
                assert sibs[m, k * sc + lvl * sl:k * sc + lvl * sl + 16].tobytes() == c.sibs[m][k][lvl]
        assert (status[m, :3] == 3).all() and (status[m, 3:] == 0xA5A5A5A5).all()
        assert (leaves[m, 48:] == 0xA5A5A5A5).all() and (sibs[m, 96:] == 0xA5A5A5A5).all()
    assert drawn.tolist() == [[0, 3, 1], [2, 2, 0]]
    per_lane = np.arange(6, dtype=np.uint32).reshape(2, 3)
    assert np.array_equal(c.arrays(prefill=per_lane)[4][:, :3], per_lane)


def test_column_numbers_cover_the_edges():
    for depth in (1, 2, 11):
        for n_open in (63, 257):
            cn = K8.column_numbers(depth, n_open)
            top = (1 << depth) - 1
            assert len(cn) == n_open and 0 in cn and top in cn and all(0 <= x <= top for x in cn)
            assert len(set(cn)) < len(cn)
    assert K8.column_numbers(0, 3) == [0, 0, 0] and len(K8.column_numbers(11, 1)) == 1
    assert int("01" * 32, 2) & 2047 in K8.column_numbers(11, 64) and int("10" * 32, 2) & 2047 in K8.column_numbers(11, 64)

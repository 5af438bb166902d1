"""CPU checks of the BLAKE2b digest option: the in-test reference (tests/blake2b_ref.py) against RFC 7693's vector and the block
boundaries of the leaf message, and the Python `digest="blake2b"` argument against the header's and the sys crate's constants."""
import hashlib
import os
import re

import pytest

import blake2b_ref as B
import pyref as P

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HDR = os.path.join(ROOT, "include", "lcpc_hip.h")
SYS = os.path.join(ROOT, "bindings", "rust", "lcpc-hip-sys", "src", "lib.rs")

# RFC 7693 Appendix A: BLAKE2b-512("abc")
RFC_ABC = ("ba80a53f981c4d0d6a2797b69f12f6e94c212f14685ac4b74b12bb6fdbffa2d1"
           "7d87c5392aab792dc252d5de4533cc9518d38aa8dbf1925ab92386edd4009923")


def header_consts():
    return {k: int(v) for k, v in re.findall(r"(LCPC_\w+)\s*=\s*(\d+)", open(HDR).read())}


def test_reference_matches_rfc7693():
    assert B.b2(b"abc").hex() == RFC_ABC
    assert len(B.b2(b"")) == B.DLEN == 64


@pytest.mark.parametrize("fid", [0, 1, 2, 3])
def test_leaf_message_block_boundaries(fid):
    """exact and partial last blocks of the leaf message (8 + L R words): each length hashed incrementally (the device walks the
    message a 128-byte block at a time) equals hashlib's one-shot digest, and L R = 8 (mod 16) picks the exact ones"""
    F = P.FIELDS[fid]
    L = {0: 1, 1: 2, 2: 3, 3: 4}[fid]
    exact = [r for r in range(1, 40) if B.exact_last_block(L, r)]
    want_mod = {1: 16, 2: 8, 3: 16, 4: 4}[L]
    want_res = {1: 8, 2: 4, 3: 8, 4: 2}[L]
    assert exact == [r for r in range(1, 40) if r % want_mod == want_res]
    for n_rows in exact[:2] + [exact[0] + 1, exact[0] - 1 if exact[0] > 1 else 3]:
        col = [(F.p - 1 - 977 * k) % F.p for k in range(n_rows)]
        msg = b"\0" * 64 + b"".join(F.to_repr(v) for v in col)
        assert len(msg) == 8 * (8 + L * n_rows)
        assert (len(msg) % 128 == 0) == B.exact_last_block(L, n_rows)
        h = hashlib.blake2b()
        for off in range(0, len(msg), 128):
            h.update(msg[off:off + 128])
        assert h.digest() == hashlib.blake2b(msg).digest() == B.leaf_from_ints(F, col)


def test_reference_tree_rules():
    leaves = [B.b2(bytes([i])) for i in range(5)]
    h = B.tree(leaves)
    assert len(h) == 2 * 8 - 1 and h[5:8] == [b"\0" * 64] * 3
    assert h[8] == B.b2(leaves[0] + leaves[1]) and h[-1] == B.b2(h[12] + h[13])
    assert all(len(x) == 64 for x in h)
    for c in range(5):
        assert B.fold(leaves[c], c, B.path(h, 8, c)) == h[-1]


def test_digest_argument_blake2b():
    import lcpc_amd
    consts = header_consts()
    assert consts["LCPC_HASH_BLAKE2B"] == 2 and consts["LCPC_DIGEST_LEN_MAX"] == 64
    assert lcpc_amd._params(3, lcpc_amd.ENC_LIGERO, 0, digest="blake2b").hash == consts["LCPC_HASH_BLAKE2B"]
    assert lcpc_amd._params(0, lcpc_amd.ENC_SDIG, 0, digest="blake2b").hash == consts["LCPC_HASH_BLAKE2B"]
    assert lcpc_amd.ALL_DIGESTS == dict(lcpc_amd.DIGESTS, blake2b=consts["LCPC_HASH_BLAKE2B"])
    assert lcpc_amd.DIGEST_LEN == {"blake3": 32, "sha3_256": 32, "blake2b": consts["LCPC_DIGEST_LEN_MAX"]}
    with pytest.raises(ValueError):
        lcpc_amd._params(3, lcpc_amd.ENC_LIGERO, 0, digest="blake2s")


def test_digests_table_unchanged():
    import lcpc_amd
    assert lcpc_amd.DIGESTS == {"blake3": 0, "sha3_256": 1}


def test_sys_crate_declares_blake2b():
    txt = open(SYS).read()
    assert re.search(r"pub const LCPC_HASH_BLAKE2B\s*:\s*u32\s*=\s*2\s*;", txt)
    assert re.search(r"pub const LCPC_DIGEST_LEN_MAX\s*:\s*u32\s*=\s*64\s*;", txt)


def test_root_bincode_64():
    import lcpc_amd
    r = bytes(range(64))
    assert lcpc_amd.root_bincode(r) == (64).to_bytes(8, "little") + r

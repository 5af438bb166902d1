"""CPU checks of the SHA3-256 digest option: the in-test reference (tests/sha3_ref.py) against NIST vectors and the FIPS 202
padding boundaries, and the Python `digest=` argument against the header's LCPC_HASH_* constants."""
import os
import re

import pytest

import pyref as P
import sha3_ref as S

HDR = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "lcpc_hip.h")

# FIPS 202 example values (NIST CSRC "SHA3-256" example file) and the 1600-bit (200 x 0xA3) vector of the SHA-3 validation set
NIST = [
    (b"", "a7ffc6f8bf1ed76651c14756a061d662f580ff4de43b49fa82d80a4b80f8434a"),
    (b"abc", "3a985da74fe225b2045c172d6bd390bd855f086e3e9d525b46bfe24511431532"),
    (b"abcdbcdecdefdefgefghfghighijhijkijkljklmklmnlmnomnopnopq",
     "41c0dba2a9d6240849100376a8235e2c82e1b9998a999e21db32dd97496d3376"),
    (b"\xa3" * 200, "79f38adec5c20307a98ef76e8324afbfd46cfd81b22e3973c65fa1bd9de31787"),
]


@pytest.mark.parametrize("msg,digest", NIST)
def test_reference_sha3_matches_nist(msg, digest):
    assert S.sha3(msg).hex() == digest


def test_reference_leaf_and_tree_rules():
    F = P.FT255
    # leaf message = 0^32 || to_repr(...): 4 + L n_rows words; 30 rows of Ft255 = 124 words, past seven 17-word blocks
    col = [F.p - 1, 1 << 254, 0, 1] + list(range(26))
    msg = b"\0" * 32 + b"".join(x.to_bytes(32, "little") for x in col)
    assert S.leaf_from_ints(F, col) == S.sha3(msg)
    leaves = [S.sha3(bytes([i])) for i in range(5)]
    h = S.tree(leaves)
    assert len(h) == 2 * 8 - 1 and h[5:8] == [b"\0" * 32] * 3
    assert h[8] == S.sha3(leaves[0] + leaves[1]) and h[-1] == S.sha3(h[12] + h[13])
    for c in range(5):
        assert S.fold(leaves[c], c, S.path(h, 8, c)) == h[-1]


def test_reference_rate_boundaries():
    # 136-byte rate: messages of 135, 136 and 137 bytes cross the padding cases (one pad byte 0x86, a whole padding block)
    import hashlib
    for n in (135, 136, 137, 271, 272):
        m = bytes(range(256)) * 2
        assert S.sha3(m[:n]) == hashlib.new("sha3_256", m[:n]).digest()


def test_digest_argument_maps_to_header():
    import lcpc_amd
    txt = open(HDR).read()
    consts = dict((k, int(v)) for k, v in re.findall(r"(LCPC_HASH_\w+)\s*=\s*(\d+)", txt))
    assert lcpc_amd.DIGESTS == {"blake3": consts["LCPC_HASH_BLAKE3"], "sha3_256": consts["LCPC_HASH_SHA3_256"]}
    assert lcpc_amd._params(3, lcpc_amd.ENC_LIGERO, 0).hash == consts["LCPC_HASH_BLAKE3"]
    assert lcpc_amd._params(3, lcpc_amd.ENC_LIGERO, 0, digest="sha3_256").hash == consts["LCPC_HASH_SHA3_256"]
    assert lcpc_amd._params(1, lcpc_amd.ENC_SDIG, 0, digest="blake3").hash == consts["LCPC_HASH_BLAKE3"]
    with pytest.raises(ValueError):
        lcpc_amd._params(3, lcpc_amd.ENC_LIGERO, 0, digest="sha3_512")

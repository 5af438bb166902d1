"""keccak256_host and sha256_host (lcpc_amd/csrc/host_crypto.cpp: the verifier's hashes under LCPC_HASH_KECCAK256 / LCPC_HASH_SHA256)
against their references -- hashlib.sha256, and the Keccak-256 sponge of tests/digest_more.py on pyref's Keccak-f -- the way
tests/test_host_digests.py holds the other three: every length 0..600, every multiple of 8 up to 4 KiB, the exact leaf and node
messages 32 + 8 L n_rows and 64 for n_rows 1..70, L 1..4; Keccak-256 under each LCPC_KECCAK form; once under AddressSanitizer +
UndefinedBehaviorSanitizer.  And the public names: digest="keccak256" / "sha256" map to the header's constants, the three pinned
tables keep their contents, the sys crate declares both constants.  No GPU."""
import hashlib
import os
import re
import subprocess

import numpy as np
import pytest

import digest_more as DM
import digest_ref as DR
import pyref as P

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HDR = os.path.join(ROOT, "include", "lcpc_hip.h")
SYS = os.path.join(ROOT, "bindings", "rust", "lcpc-hip-sys", "src", "lib.rs")


def lengths():
    ls = set(range(601)) | set(range(0, 4097, 8)) | {64}
    ls |= {32 + 8 * L * r for L in (1, 2, 3, 4) for r in range(1, 71)}
    return sorted(ls)


def message(n):
    return bytes((7 * i + 3) & 0xFF for i in range(n))


# ---- the references themselves ---------------------------------------------------------------------------------------------------

def test_keccak256_reference_vectors():
    for m, want in DM.KAT.items():
        assert DM.keccak256(m).hex() == want
        assert DM.keccak256(m) != hashlib.sha3_256(m).digest()
    for n in (0, 1, 135, 136, 137, 271, 272, 500):
        m = message(n)
        assert DM.sha3_256_sponge(m) == hashlib.sha3_256(m).digest()       # the sponge, with the domain byte hashlib knows
        assert DM.keccak256(m) != hashlib.sha3_256(m).digest()


def test_keccak256_fast_and_batched_forms_are_the_reference(oracle):
    DM.register()
    assert DM.DIGESTS["keccak256"].fn is DM.keccak256_fast and DM.DIGESTS["keccak256"].size == 32 and DR.DLEN["keccak256"] == 32
    assert DR.ref_digest("sha256")(b"abc").hex() == "ba7816bf8f01cfea414140de5dae2223b00361a396177a9cb410ff61f20015ad"
    for n in list(range(0, 300, 7)) + [135, 136, 137, 271, 272, 273, 64, 32 + 8 * 4 * 70]:
        assert DM.keccak256_fast(message(n)) == DM.keccak256(message(n)), n
    rng = np.random.default_rng(3)
    for ln in (0, 8, 64, 128, 135, 136, 137, 272, 32 + 8 * 3 * 17):
        msgs = rng.integers(0, 256, (5, ln), dtype=np.uint8)
        got = DM.keccak256_many(msgs)
        assert [g.tobytes() for g in got] == [DM.keccak256(r.tobytes()) for r in msgs], ln
    assert [g.tobytes() for g in DM.many("sha256", np.zeros((2, 64), np.uint8))] == [hashlib.sha256(bytes(64)).digest()] * 2


def test_registration_leaves_the_fixed_lists_alone():
    assert DR.DIGEST_NAMES == ["blake3", "sha3_256", "blake2b"]
    assert list(P.DIGESTS) == ["blake3", "sha3_256", "blake2b"]            # tests/golden/make_golden.py iterates this table
    assert DR.ref_digest("sha3_256")(b"abc") == hashlib.sha3_256(b"abc").digest() and DR.ref_digest("blake2b").size == 64
    assert DR.ref_digest("keccak256") is DM.DIGESTS["keccak256"] and DR.ref_digest("sha256", None) is DM.DIGESTS["sha256"]


def test_edge_rows_reach_every_claimed_residue():
    """the (field, residue) pairs the GPU edge test covers, derived; an unreachable pair is stated, not skipped"""
    want_none = {0: set(), 1: {("sha256", 1), ("sha256", 7)}, 2: set(), 3: {("sha256", 1), ("sha256", 6), ("sha256", 7)}}
    for fid in range(4):
        rows = DM.edge_rows(fid)
        assert {k for k, v in rows.items() if v is None} == want_none[fid]
        for (name, res), r in rows.items():
            if r is not None:
                fn = DM.sha256_residue if name == "sha256" else DR.sha3_residue
                assert fn(DR.LIMBS[fid], r) == res


# ---- the host digests --------------------------------------------------------------------------------------------------------------

def build(tmp_path, name, flags):
    exe = str(tmp_path / name)
    csrc = os.path.join(ROOT, "lcpc_amd", "csrc")
    cc = subprocess.run(["g++", *flags, "-std=c++17", "-pthread", "-I" + csrc, os.path.join(ROOT, "tests", "native", "host_digest_more_dump.cpp"),
                         os.path.join(csrc, "host_crypto.cpp"), "-o", exe], capture_output=True, text=True, timeout=900)
    assert cc.returncode == 0, cc.stderr[-3000:]
    return exe


def run(exe, ls, keccak=None):
    env = dict(os.environ)
    env.pop("LCPC_KECCAK", None)
    if keccak:
        env["LCPC_KECCAK"] = keccak
    r = subprocess.run([exe], input="".join("%d\n" % n for n in ls), capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0 and "ERROR" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-3000:]
    rows = [ln.split() for ln in r.stdout.splitlines()]
    assert [int(x[0]) for x in rows] == list(ls)
    return rows


def check(rows, oracle):
    DM.register()
    kref = DM.keccak256_fast if oracle is not None else DM.keccak256
    bad = []
    for n, k, s2, s3 in rows:
        n = int(n)
        m = message(n)
        if k != kref(m).hex():
            bad.append(("keccak256", n, n % 136))
        if s2 != hashlib.sha256(m).hexdigest():
            bad.append(("sha256", n, n % 64))
        if s3 != hashlib.sha3_256(m).hexdigest():
            bad.append(("sha3_256", n, n % 136))
    assert not bad, "host digests differ from the reference at (digest, length, length mod block): %s" % bad[:12]


@pytest.fixture(scope="module")
def dump(tmp_path_factory):
    return build(tmp_path_factory.mktemp("host_digest_more"), "host_digest_more_dump", ["-O2"])


def test_lengths_cover_the_block_edges():
    ls = set(lengths())
    leaf = {32 + 8 * L * r for L in (1, 2, 3, 4) for r in range(1, 71)}
    assert leaf <= ls and 64 in ls
    assert {55, 56, 63, 64, 119, 120, 135, 136, 137, 271, 272} <= ls
    assert {n % 64 for n in leaf} == set(range(0, 64, 8))                      # every word residue of the SHA-256 block
    assert {n % 136 for n in ls if n % 8 == 0} == set(range(0, 136, 8))        # and of the Keccak rate
    assert any(n % 64 == 56 for n in leaf) and any(n % 64 == 0 for n in leaf) and any(n % 136 == 128 for n in leaf)


def test_host_digests_default(dump, oracle):
    rows = run(dump, lengths())
    check(rows, oracle)
    # a sample against the pure-Python sponge on pyref's Keccak-f itself (the whole list: the C oracle's permutation, held to
    # pyref's in test_keccak256_fast_and_batched_forms_are_the_reference)
    for n, k, _, _ in rows[::37]:
        assert k == DM.keccak256(message(int(n))).hex(), n


@pytest.mark.parametrize("mix", ["portable", "tern", "xor"])
def test_host_keccak256_under_each_keccak_form(dump, oracle, mix):
    check(run(dump, lengths(), mix), oracle)


def test_host_digests_under_sanitizers(tmp_path, oracle):
    exe = build(tmp_path, "host_digest_more_dump_san", ["-O1", "-g", "-fsanitize=address,undefined", "-fno-omit-frame-pointer",
                                                        "-fno-sanitize-recover=undefined"])
    ls = [n for n in lengths() if n <= 600 or n % 136 in (0, 128) or n % 64 in (0, 56)]
    for mix in (None, "portable", "tern", "xor"):
        check(run(exe, ls, mix), oracle)


# ---- the public names --------------------------------------------------------------------------------------------------------------

def header_consts():
    txt = open(HDR).read()
    return dict((k, int(v)) for k, v in re.findall(r"(LCPC_(?:HASH_\w+|DIGEST_LEN_MAX))\s*=\s*(\d+)", txt))


def test_digest_arguments_map_to_header():
    import lcpc_amd
    c = header_consts()
    assert c["LCPC_HASH_KECCAK256"] == 3 and c["LCPC_HASH_SHA256"] == 4 and c["LCPC_DIGEST_LEN_MAX"] == 64
    for kind in (lcpc_amd.ENC_LIGERO, lcpc_amd.ENC_SDIG):
        assert lcpc_amd._params(3, kind, 0, digest="keccak256").hash == c["LCPC_HASH_KECCAK256"]
        assert lcpc_amd._params(1, kind, 0, digest="sha256").hash == c["LCPC_HASH_SHA256"]
    assert lcpc_amd.DIGEST_TABLE == {"blake3": (c["LCPC_HASH_BLAKE3"], 32), "sha3_256": (c["LCPC_HASH_SHA3_256"], 32),
                                     "blake2b": (c["LCPC_HASH_BLAKE2B"], 64), "keccak256": (c["LCPC_HASH_KECCAK256"], 32),
                                     "sha256": (c["LCPC_HASH_SHA256"], 32)}
    assert sorted(v for k, v in c.items() if k.startswith("LCPC_HASH_")) == [0, 1, 2, 3, 4]
    for bad in ("sha3_512", "blake2s", "keccak", "sha2", "SHA256"):
        with pytest.raises(ValueError):
            lcpc_amd._params(3, lcpc_amd.ENC_LIGERO, 0, digest=bad)


def test_pinned_tables_unchanged():
    import lcpc_amd
    assert lcpc_amd.DIGESTS == {"blake3": 0, "sha3_256": 1}
    assert lcpc_amd.ALL_DIGESTS == {"blake3": 0, "sha3_256": 1, "blake2b": 2}
    assert lcpc_amd.DIGEST_LEN == {"blake3": 32, "sha3_256": 32, "blake2b": 64}
    assert all(lcpc_amd.DIGEST_TABLE[k] == (v, lcpc_amd.DIGEST_LEN[k]) for k, v in lcpc_amd.ALL_DIGESTS.items())


def test_sys_crate_declares_both():
    txt = open(SYS).read()
    assert re.search(r"pub const LCPC_HASH_KECCAK256\s*:\s*u32\s*=\s*3\s*;", txt)
    assert re.search(r"pub const LCPC_HASH_SHA256\s*:\s*u32\s*=\s*4\s*;", txt)
    assert int(re.search(r"#define LCPC_ABI_VERSION (\d+)", open(HDR).read()).group(1)) == 5

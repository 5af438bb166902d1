"""blake3_host, sha3_256_host and blake2b_host (lcpc_amd/csrc/host_crypto.cpp: the verifier's hashes) against hashlib and pyref's
BLAKE3, at every message length where a sponge or a HAIFA hash changes branch -- not only through a verify that happens to
succeed.  Lengths: every one from 0 to 600; every multiple of 8 up to 4 KiB; and the exact leaf and node messages of the
commitment, dl + 8 L n_rows and 2 dl for n_rows 1..70, L 1..4.  SHA3 under each LCPC_KECCAK form, and everything once under
AddressSanitizer + UndefinedBehaviorSanitizer.  No GPU."""
import hashlib
import os
import subprocess

import pytest

import pyref as P

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def lengths():
    ls = set(range(601)) | set(range(0, 4097, 8)) | {64, 128}
    for dl in (32, 64):
        ls |= {dl + 8 * L * r for L in (1, 2, 3, 4) for r in range(1, 71)}
    return sorted(ls)


def message(n):
    return bytes((7 * i + 3) & 0xFF for i in range(n))


def build(tmp_path, name, flags):
    exe = str(tmp_path / name)
    csrc = os.path.join(ROOT, "lcpc_amd", "csrc")
    cc = subprocess.run(["g++", *flags, "-std=c++17", "-pthread", "-I" + csrc, os.path.join(ROOT, "tests", "native", "host_digest_dump.cpp"),
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


def check(rows, blake3=True):
    bad = []
    for n, b3, s3, b2 in rows:
        n = int(n)
        m = message(n)
        if s3 != hashlib.sha3_256(m).hexdigest():
            bad.append(("sha3_256", n, n % 136))
        if b2 != hashlib.blake2b(m).hexdigest():
            bad.append(("blake2b", n, n % 128))
        if blake3 and b3 != P.blake3(m).hex():
            bad.append(("blake3", n, n % 64))
    assert not bad, "host digests differ from the reference at (digest, length, length mod block): %s" % bad[:12]


@pytest.fixture(scope="module")
def dump(tmp_path_factory):
    return build(tmp_path_factory.mktemp("host_digest"), "host_digest_dump", ["-O2"])


def test_lengths_cover_the_block_edges():
    ls = set(lengths())
    for dl in (32, 64):                                                         # leaf messages with one SHA3 word left / BLAKE2b exactly full
        leaf = {dl + 8 * L * r for L in (1, 2, 3, 4) for r in range(1, 71)}
        assert any(n % 136 == 128 for n in leaf) and any(n % 128 == 0 for n in leaf) and leaf <= ls
    assert {n % 136 for n in ls if n % 8 == 0} == set(range(0, 136, 8))         # every word residue of the SHA3 rate
    assert {n % 128 for n in ls if n % 8 == 0} == set(range(0, 128, 8))         # and of the BLAKE2b block
    assert {0, 128, 256, 136, 272, 135, 127, 129, 137} <= ls


def test_host_digests_default(dump):
    check(run(dump, lengths()))


@pytest.mark.parametrize("mix", ["portable", "tern", "xor"])
def test_host_sha3_under_each_keccak_form(dump, mix):
    check(run(dump, lengths(), mix), blake3=False)


def test_host_digests_under_sanitizers(tmp_path):
    exe = build(tmp_path, "host_digest_dump_san", ["-O1", "-g", "-fsanitize=address,undefined", "-fno-omit-frame-pointer",
                                                   "-fno-sanitize-recover=undefined"])
    ls = [n for n in lengths() if n <= 600 or n % 136 in (0, 128) or n % 128 in (0, 8)]
    check(run(exe, [n for n in ls if n <= 600]))
    for mix in (None, "portable", "tern", "xor"):
        check(run(exe, ls, mix), blake3=False)

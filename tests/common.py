"""helpers shared by the CPU (oracle) and GPU (HIP) test files."""
import hashlib
import json
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def load_golden(name):
    with open(os.path.join(GOLDEN, name)) as f:
        return json.load(f)


def hex_to_limbs(h, L):
    v = int(h, 16)
    return np.array([(v >> (64 * k)) & 0xFFFFFFFFFFFFFFFF for k in range(L)], np.uint64)


def golden_coeffs(oracle, case):
    """the deterministic inputs of tests/golden/make_golden.py, as (n, L) Montgomery limbs."""
    fid, n = case["field"], case["n_coeffs"]
    L = oracle.limbs(fid)
    if case["coeffs"] == "iota":
        v = np.arange(1, n + 1, dtype=np.uint64)
        out = np.zeros((n, L), np.uint64)
        oracle.lib().lo_f_from_u64(fid, oracle.ptr(v), oracle.ptr(out), n)
        return out
    return oracle.random_elems(fid, n, case["seed"])


def powers(oracle, fid, x_int, n, start_exp_step=1):
    """[x^(k*step)] for k < n as Montgomery limbs (python ints -> oracle conversion)."""
    import pyref as P
    F = P.FIELDS[fid]
    base = pow(x_int, start_exp_step, F.p)
    vals, cur = [], 1
    for _ in range(n):
        vals.append(cur)
        cur = cur * base % F.p
    return oracle.to_mont(fid, vals)


def sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def mk_transcript(T, root, n_col_opens):
    # lcpc-ligero-pc/src/tests.rs:243-245
    tr = T(b"test transcript")
    tr.append_message(b"polycommit", bytes(root))
    tr.append_message(b"ncols", int(n_col_opens).to_bytes(8, "big"))
    return tr


def load_dump(d):
    """the arrays `bench.py --dump-outputs d` wrote, by name"""
    return {f[:-4]: np.load(os.path.join(d, f)) for f in os.listdir(d) if f.endswith(".npy")}


def dump_bytes(words):
    """bench.words_f32 undone: (..., 16) float32 words -> (..., 32) uint8 digests / Montgomery limbs"""
    assert words.dtype == np.float32 and (words == np.round(words)).all() and words.min() >= 0 and words.max() < 65536
    return np.ascontiguousarray(words.astype("<u2")).view(np.uint8)


def commit_bincode(oc):
    """bincode 1.3 of WrappedLcCommit (lcpc-2d/src/lib.rs:186-197) built from a commitment's fields (oracle or HIP object with
    comm() / coeffs() / hashes() / n_rows / n_cols / n_per_row): Vec<F> = u64 len + raw Montgomery limbs; usize = u64;
    Vec<WrappedOutput> = u64 len + (u64 32 + 32 bytes) each."""
    import struct
    comm, coeffs, hashes = oc.comm(), oc.coeffs(), oc.hashes()
    out = [struct.pack("<Q", comm.shape[0]), comm.tobytes(), struct.pack("<Q", coeffs.shape[0]), coeffs.tobytes(),
           struct.pack("<QQQ", oc.n_rows, oc.n_cols, oc.n_per_row), struct.pack("<Q", hashes.shape[0])]
    for h in hashes:
        out.append(struct.pack("<Q", 32) + bytes(h))
    return b"".join(out)



def run_with_test_hooks(body, env=None, timeout=600):
    """run `body` (python source) in a child process whose lcpc_amd loads lib/liblcpc_hip_testhooks.so -- the library built with
    -DLCPC_TEST_HOOKS (lcpc_amd/csrc/Makefile), the only build that reads LCPC_TEST_FAIL.  The product library carries no such branch."""
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    hooks = os.path.join(root, "lcpc_amd", "lib", "liblcpc_hip_testhooks.so")
    assert os.path.exists(hooks), "lcpc_amd/csrc/Makefile builds it beside the product"
    pre = ("import os, sys\nsys.path[:0] = [%r, %r, %r]\nimport lcpc_amd._lib as _L\n_L.LIB_PATH = %r\n"
           "import numpy as np\nimport oracle_lib as O\nfrom lcpc_amd import LcCommit, LigeroEncoding\n"
           % (root, os.path.join(root, "tests"), os.path.join(root, "oracle"), hooks))
    e = dict(os.environ)
    e.update(env or {})
    r = subprocess.run([sys.executable, "-c", pre + body], capture_output=True, text=True, env=e, timeout=timeout)
    assert r.returncode == 0, r.stderr[-3000:]
    return r.stdout


# ---- worst-case operands and Python-int arithmetic of the lazy-reduction tests (test_lazy_bounds, test_gpu_lazy_worst,
# test_gpu_fullsize) ------------------------------------------------------------------------------------------------------------------
FIELD_L = {0: 1, 1: 2, 2: 3, 3: 4}


def field_p(fid):
    import pyref as P
    return P.FIELDS[fid].p


def maximal_limbs(fid, W, n_low):
    """the largest element < p whose n_low low W-bit limbs are all 2^W - 1"""
    p, s = field_p(fid), W * n_low
    return ((p >> s) << s) - 1


def maxc(fid):
    """the stored coefficient that makes the collapse's products largest: Ft255 splits it into 29-bit limbs (ln::from_packed: eight low
    limbs of 2^29 - 1), the other fields multiply 32-bit words (Wide<NL>: every word but the top one all ones)"""
    return maximal_limbs(fid, 29, 8) if fid == 3 else maximal_limbs(fid, 32, 2 * FIELD_L[fid] - 1)


def maxt(fid):
    """the stored tensor entry whose multiplied form is maxc: for Ft255 the kernel multiplies t * 2^5 mod p (to_r29_kernel)"""
    p = field_p(fid)
    return maxc(fid) * pow(32, -1, p) % p if fid == 3 else maxc(fid)


def ntt_maxlimb(fid):
    """the largest element < p whose low limbs in the row NTT's limb form are all ones (l9: 9 x 29 bits; ln: 3 x 26, 5 / 7 x 29)"""
    W, N = {0: (26, 3), 1: (29, 5), 2: (29, 7), 3: (29, 9)}[fid]
    return maximal_limbs(fid, W, N - 1)


def to_limbs(vals, L):
    """python ints -> (n, L) uint64 limbs"""
    return np.array([[(v >> (64 * k)) & ((1 << 64) - 1) for k in range(L)] for v in vals], np.uint64).reshape(-1, L)


def to_int(limbs):
    return sum(int(x) << (64 * k) for k, x in enumerate(limbs))


def ntt_root(fid, log_n):
    """w = ROOT_OF_UNITY^(2^(S - log n)) (oracle/lcpc_oracle.c lo_roots_table), as a plain residue"""
    import pyref as P
    F = P.FIELDS[fid]
    return pow(F.root_of_unity, 1 << (F.S - log_n), F.p)


def _butterflies(x, n, gap, w, p, inverse):
    """one DIF stage of a length-n transform (gap = n >> (k + 1), twiddle w^((n / 2 gap) idx)) over the blocks of 2 gap in x"""
    step = n // (2 * gap)
    tw = [pow(w, step * i, p) for i in range(gap)]
    if inverse:
        tw = [pow(t, -1, p) for t in tw]
        half = pow(2, -1, p)
    for off in range(0, len(x), 2 * gap):
        for i in range(gap):
            a, b = x[off + i], x[off + i + gap]
            if inverse:
                d = b * tw[i] % p
                x[off + i], x[off + i + gap] = (a + d) * half % p, (a - d) * half % p
            else:
                x[off + i], x[off + i + gap] = (a + b) % p, (a - b) * tw[i] % p


def dif_stage(x, k, w, p, inverse=False):
    """stage k of the row NTT's radix-2 DIF (oracle/lcpc_oracle.c fft_io_L: natural in, bit-reversed out), in place on a list of
    residues of length n: gap = n >> (k + 1); in every block of 2 gap, lo' = lo + hi, hi' = (lo - hi) w^((n / 2 gap) idx).  The
    stored (Montgomery) values transform the same way, the twiddles being plain residues.  inverse: undo that stage."""
    _butterflies(x, len(x), len(x) >> (k + 1), w, p, inverse)
    return x


def row_with_stage_input(fid, log_n, s, pattern):
    """the n/2 free entries x of a rate-1/2 row (x, 0) whose values entering DIF stage s equal `pattern` on the first half of the
    row.  Stage 0 maps (x, 0) to (x, x w^i); stages 1 .. s-1 work in blocks of at most n/2, so the first half enters them as x and
    never meets the second half again: running the inverse of stages s-1 .. 1 on the pattern gives x."""
    p, n = field_p(fid), 1 << log_n
    w = ntt_root(fid, log_n)
    x = [pattern[i % len(pattern)] for i in range(n // 2)]
    for k in range(s - 1, 0, -1):
        _butterflies(x, n, n >> (k + 1), w, p, True)
    return x

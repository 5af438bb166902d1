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


def _ln_fields():
    """{fid: (N, W, NL, STRIDE)} of lcpc_amd/csrc/field_ln.h's LnField specialisations"""
    import re
    t = open(os.path.join(os.path.dirname(GOLDEN), os.pardir, "lcpc_amd", "csrc", "field_ln.h")).read()
    out = {}
    for fid, name in enumerate(("FT63", "FT127", "FT191", "FT255")):
        m = re.search(r"struct LnField<%s> \{\s*static constexpr int FID = %s, N = (\d+), W = (\d+), NL = (\d+), WAVES = \d+, STRIDE = (\d+);"
                      % (name, name), t)
        out[fid] = tuple(int(v) for v in m.groups())
    return out


LN_SHAPE = {fid: v[:2] for fid, v in _ln_fields().items()}        # (N limbs, W bits): R' = 2^(N W)
LN_STRIDE = {fid: v[3] for fid, v in _ln_fields().items()}        # words per limb-form table entry


def ln_maxx(fid):
    """the gathered operand of the Brakedown limb dot products (Ft127 / Ft191 / Ft255: ln::from_packed<FT> of the stored element) whose
    limbs below the top one are all 2^W - 1; for Ft255 this is maxc"""
    N, W = LN_SHAPE[fid]
    return maximal_limbs(fid, W, N - 1)


def ln_maxv(fid):
    """the stored matrix value whose multiplied form has those limbs: the kernels multiply v R' / R mod p (R = 2^(64 L) the stored
    Montgomery form, R' = 2^(N W): launch_ntt_lns_roots; Ft255: five doublings, R' / R = 2^5, so this is maxt)"""
    p = field_p(fid)
    N, W = LN_SHAPE[fid]
    return ln_maxx(fid) * pow(2, 64 * FIELD_L[fid], p) * pow(2, -N * W, p) % p


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


def stage_input_rows(fid, log_n, stages, pattern, log_rate=1, n_threads=16):
    """row_with_stage_input, vectorised and at any rate 2^-log_rate: (len(stages), n >> log_rate, L) limbs, row j the free prefix
    x of a row (x, 0, ..., 0) whose values entering DIF stage stages[j] equal `pattern` (repeated) on the first n >> log_rate
    entries.  Stages 0 .. log_rate - 1 work in blocks of more than n >> log_rate and leave that prefix as it was (its partners
    are zero); from stage log_rate on the prefix is a union of whole blocks that never meets the rest of the row again.  So for
    s <= log_rate the prefix is the pattern, and for s > log_rate it is the pattern taken back through the inverse of stages
    s - 1 .. log_rate (oracle lo_dif_stage: one call per stage over every row that still needs it, rows by falling s)."""
    import oracle_lib as O
    L, m = FIELD_L[fid], (1 << log_n) >> log_rate
    stages = list(stages)
    assert all(0 <= s < log_n for s in stages) and m % len(pattern) == 0
    order = sorted(range(len(stages)), key=lambda j: -stages[j])
    rows = np.empty((len(stages), m, L), np.uint64)
    rows[:] = np.tile(to_limbs(pattern, L), (m // len(pattern), 1))
    for k in range(max(stages) - 1, log_rate - 1, -1):
        cnt = sum(1 for s in stages if s > k)
        assert O.lib().lo_dif_stage(fid, O.ptr(rows), cnt * m, log_n, k, 1, n_threads) == 0
    out = np.empty_like(rows)
    out[order] = rows
    return out


# ---- the row-NTT plan, restated (lcpc_amd/csrc/ctx.cpp plan_passes, build_limb_plan, ntt_mid_rows; kernels.h *_supported) -------------
NTT_NL = {0: 2, 1: 4, 2: 6, 3: 8}
FIELD_BITS = {0: 63, 1: 127, 2: 191, 3: 255}


def general_passes(fid, log_n, general=False):
    """plan_passes: the general kernel's passes as (t0, stages, log_tj, log_tile)"""
    k, NL = log_n, NTT_NL[fid]
    lt_small = 10 if NL >= 6 else (11 if NL == 4 else 12)
    lt_big = 11 if NL >= 6 else 12
    ltj_min = 0
    while (NL * 4 << ltj_min) < 128:
        ltj_min += 1
    if k <= lt_small:
        return [(0, k, 0, lt_small)]

    def n_pass(lt):
        return 1 + -(-(k - lt) // (lt - ltj_min))

    if fid == 3 and k in (19, 20) and not general:
        return [(0, k - 10, 20 - k, 10), (k - 10, 10, 0, 10)]
    LT = lt_big if n_pass(lt_small) > 2 and n_pass(lt_big) < n_pass(lt_small) else lt_small
    P, rem, t0, out = n_pass(LT), k - LT, 0, []
    for i in range(P - 1):
        s = -(-rem // (P - 1 - i))
        out.append((t0, s, LT - s, LT))
        t0, rem = t0 + s, rem - s
    return out + [(t0, LT, 0, LT)]


def ntt_mid_rows(fid, log_n, n_passes, n_rows, mid_mb=None):
    """rows per batch of K1s's 36-byte limb intermediate (0: packed intermediate); mid_mb is LCPC_NTT_MID_MAX_MB (None: unset)"""
    if n_passes != 2 or fid != 3 or n_rows == 0 or (mid_mb is None and log_n > 15):
        return 0
    max_mb = 6144 if mid_mb is None else mid_mb
    fit = (max_mb << 20) // ((1 << log_n) * 36)
    if max_mb == 0 or fit == 0:
        return 0
    if fit >= n_rows:
        return n_rows
    batches = -(-n_rows // fit)
    return -(-n_rows // batches)


def ntt_plan(fid, log_n, general=False, mid_mb=None, n_rows=1):
    """the passes a Ligero encoder of 2^log_n columns launches: dicts with kernel ("K1s", "K1n" or "general"), t0 / s (the stages
    [t0, t0 + s) of the whole row), first (the first-pass template), mid (rows per limb-intermediate batch, 0 = packed) and
    blk0_gone (canonical output: block 0 converted by the pass before)"""
    gp = general_passes(fid, log_n, general)
    n_pass = 0
    if not general:
        if fid == 3:
            n_pass = 2 if len(gp) == 2 and gp[0][3] == 10 and 11 <= log_n <= 20 else 3 if 21 <= log_n <= 26 else 0
        elif len(gp) >= 2:
            n_pass = 2 if 11 <= log_n <= 20 else 3 if 21 <= log_n <= 26 else 0
    if not n_pass:
        return [dict(kernel="general", t0=t0, s=s, first=i + 1 < len(gp), mid=0, blk0_gone=False, n_pass=len(gp))
                for i, (t0, s, _, _) in enumerate(gp)]
    s0 = log_n - 10 * (n_pass - 1)
    mid = ntt_mid_rows(fid, log_n, n_pass, n_rows, mid_mb)
    out = []
    for i in range(n_pass):
        last = i + 1 == n_pass
        s = s0 if i == 0 else 10
        out.append(dict(kernel="K1s" if fid == 3 else "K1n", t0=0 if i == 0 else s0 + 10 * (i - 1), s=s, first=not last, mid=mid,
                        blk0_gone=last and NTT_NL[fid] != 2 and out[i - 1]["s"] >= 8, n_pass=n_pass))
    return out


def ntt_instantiations(fid, plan, log_n):
    """the kernel instantiations a plan reaches, by name"""
    ft, names = "ft%d" % FIELD_BITS[fid], set()
    for i, p in enumerate(plan):
        if p["kernel"] == "general":
            names.add("general-%dpass-%s-2^%d" % (p["n_pass"], ft, log_n) if p["n_pass"] == 1 else "general-%s" % ft)
            continue
        k = "K1s" if fid == 3 else "K1n-" + ft
        mid = "-mid%d" % bool(p["mid"]) if fid == 3 else ""
        if p["first"]:
            names.add("%s-first-S%d%s" % (k, p["s"], mid))
            if i == 0 and p["n_pass"] == 3:
                names.add("3pass-%s-first-S%d" % (ft, p["s"]))
        else:
            names.add("%s-last%s-blk0%s" % (k, mid, "gone" if p["blk0_gone"] else "kept"))
    return names


def ntt_required_instantiations():
    """what the row-NTT worst-case matrix must reach (tests/test_gpu_lazy_worst.py NTT_CASES)"""
    req = {"K1s-first-S%d-mid%d" % (s, m) for s in range(1, 11) for m in (0, 1)}
    req |= {"K1s-last-mid%d-blk0%s" % (m, g) for m in (0, 1) for g in ("gone", "kept")}
    for fid in (0, 1, 2):
        req |= {"K1n-ft%d-first-S%d" % (FIELD_BITS[fid], s) for s in range(1, 11)}
    for fid in (1, 2):
        req |= {"K1n-ft%d-last-blk0%s" % (FIELD_BITS[fid], g) for g in ("gone", "kept")}
    req |= {"3pass-ft%d-first-S%d" % (FIELD_BITS[fid], s) for fid in range(4) for s in (1, 2)}
    for fid in range(4):
        k = max(k for k in range(1, 27) if len(general_passes(fid, k)) == 1)
        req.add("general-1pass-ft%d-2^%d" % (FIELD_BITS[fid], k))
    return req


# ---- the shape matrix of tests/test_gpu_lazy_worst.py::test_ntt_extremes_at_every_stage ----------------------------------------------
FIRST_TWO_PASS = {0: 13, 1: 12, 2: 11, 3: 11}      # smallest log2 n_cols with a two-pass plan, per field
# the 13 shapes the test started with (fid, log_n, LCPC_NTT_GENERAL), kept with their ids
NTT_LEGACY = [(3, 12, False), (3, 13, False), (3, 14, False), (3, 13, True), (0, 13, False), (0, 14, False), (0, 13, True),
              (1, 12, False), (1, 14, False), (1, 12, True), (2, 11, False), (2, 14, False), (2, 11, True)]


def ntt_worst_cases():
    """(fid, log_n, log_rate, LCPC_NTT_GENERAL, LCPC_NTT_MID_MAX_MB or None): the legacy shapes; every two-pass size to 2^20 (Ft255
    with the limb intermediate off and forced on, 64 MiB: row batches from 2^17 on); the three-pass plans at 2^21 / 2^22; each
    field's largest one-pass plan; the general kernel forced at 2^18 / 2^21 (Ft255, Ft127); rate 1/4 at 2^18 (Ft255) / 2^16 (Ft127)"""
    cases = [(f, k, 1, g, None) for f, k, g in NTT_LEGACY]
    for fid in (3, 0, 1, 2):
        for k in range(FIRST_TWO_PASS[fid], 21):
            if fid == 3:
                cases += [(3, k, 1, False, 0), (3, k, 1, False, 64)]
            elif (fid, k, False) not in NTT_LEGACY:
                cases.append((fid, k, 1, False, None))
    cases += [(fid, k, 1, False, None) for fid in (3, 0, 1, 2) for k in (21, 22)]
    cases += [(fid, max(k for k in range(1, 27) if len(general_passes(fid, k)) == 1), 1, False, None) for fid in (3, 0, 1, 2)]
    cases += [(fid, k, 1, True, None) for fid in (3, 1) for k in (18, 21)]
    cases += [(3, 18, 2, False, None), (1, 16, 2, False, None)]
    return cases


def ntt_case_stages(fid, log_n, general=False):
    """every stage up to 2^20 columns; above, stage 0, the last two, and each pass boundary t0 with its neighbours t0 +- 1
    (three-pass limb plans: s0 and s0 + 10): what differs between the stages inside one pass is the round they fall in, and the
    two-pass sizes already give every round of every pass template its crafted inputs"""
    if log_n <= 20:
        return list(range(log_n))
    st = {0, log_n - 2, log_n - 1}
    for p in ntt_plan(fid, log_n, general)[1:]:
        st |= {p["t0"] - 1, p["t0"], p["t0"] + 1}
    return sorted(st)


def ntt_case_id(fid, log_n, log_rate, general, mid_mb):
    if log_rate == 1 and mid_mb is None and (fid, log_n, general) in NTT_LEGACY:
        return "ft%d-2^%d%s" % (fid, log_n, "-general" if general else "")
    plan = ntt_plan(fid, log_n, general, mid_mb)
    out = "ft%d-2^%d%s" % (FIELD_BITS[fid], log_n, "-r%d" % (1 << log_rate) if log_rate != 1 else "")
    if plan[0]["kernel"] == "general":
        return out + "-general-%dpass%s" % (len(plan), "-forced" if general else "")
    out += "-S%d" % plan[0]["s"] + ("-3pass" if len(plan) == 3 else "")
    if fid == 3:
        out += "-mid%d" % bool(plan[0]["mid"]) + ("-mb%d" % mid_mb if mid_mb is not None else "")
    return out + ("-blk0gone" if plan[-1]["blk0_gone"] else "")


# ---- the BLAKE3 column hash and tree, restated (lcpc_amd/csrc/kernels.hip K3 / K4 launchers, commit.cpp merkleize_device) ---------------
K3_QUAD_MAX = 65536        # launch_leaf_chunks_nl: n_cols * n_chunks_local <= this runs four lanes per column; leaf_tree_supported's bound too
K3_SLICE = 32768           # launch_leaf_chunks: chunks per launch (grid.y)


def leaf_len(fid, n_rows):
    """bytes of a column's leaf message: the 32-byte zero prefix and 8 L bytes per row"""
    return 32 + 8 * FIELD_L[fid] * n_rows


def leaf_n_chunks(fid, n_rows):
    return max(1, -(-leaf_len(fid, n_rows) // 1024))


def leaf_last(fid, n_rows):
    """(bytes in the last chunk, its 64-byte blocks, bytes in its last block)"""
    b = leaf_len(fid, n_rows) - 1024 * (leaf_n_chunks(fid, n_rows) - 1)
    nb = max(1, -(-b // 64))
    return b, nb, b - 64 * (nb - 1)


def leaf_quad(n_cols, n_chunks_local):
    """launch_leaf_chunks_nl: QUAD (four lanes per column) or one lane per column"""
    return n_cols * n_chunks_local <= K3_QUAD_MAX


K3B_QUAD_MAX = 65536       # kernels.hip launch_leaf_chunks_nl with n_batch members: the (column, chunk) pairs of ALL members against the same number
K3B_MAX_BATCH = 65535      # the batch launchers: members per launch (a grid dimension)


def leaf_quad_batch(n_cols, n_chunks_local, n_batch):
    """launch_leaf_chunks_nl: QUAD or one lane per column, for the whole batch"""
    return n_cols * n_chunks_local * n_batch <= K3B_QUAD_MAX


def leaf_block_phases(fid, chunks):
    """leaf_chunk_cv block_row0: the word phases (first word of a block inside its first element) over the blocks of `chunks`"""
    nl = NTT_NL[fid]
    return {(16 * (16 * c + b) - 8) % nl for c in chunks for b in range(16)}


def leaf_tree_supported(n_cols, np2, chunk_begin, n_chunks_local, n_chunks_total):
    """kernels.hip leaf_tree_supported"""
    return (n_chunks_total <= 2 and n_chunks_local == n_chunks_total and chunk_begin == 0 and np2 == n_cols and n_cols >= 128
            and n_cols % 64 == 0 and n_cols * n_chunks_total <= K3_QUAD_MAX)


def merkle_launches(np2, levels_done=0):
    """launch_merkle_tree_from: [(BS, n_workgroups, lsub, branches)] -- branches: the sides of merkle_subtree_kernel's n_out > BS / 4 test
    its levels take ("lane": one compression per lane, "quad": one per four lanes)"""
    width, out = np2 >> levels_done, []
    while width > 1:
        lw = (width - 1).bit_length()
        bs, lsub, nwg = (1024, lw, 1) if lw <= 9 else (256, 9, width >> 9)
        out.append((bs, nwg, lsub, {"lane" if (1 << lsub >> j) > bs // 4 else "quad" for j in range(1, lsub + 1)}))
        if lw <= 9:
            break
        width >>= 9
    return out


def k3_plan(fid, n_rows, n_cols, np2=None):
    """what an unsharded BLAKE3 commit of n_rows x n_cols launches for its leaves (commit.cpp merkleize_device): path ("fused": leaf_tree_kernel;
    "one_chunk": leaf_chunk_kernel straight into hashes; "chunks+finish"), quad (None for fused, which is always four lanes per column),
    hash_launches, levels_done and the tree launches"""
    np2 = np2 or 1 << (n_cols - 1).bit_length()
    nc = leaf_n_chunks(fid, n_rows)
    if leaf_tree_supported(n_cols, np2, 0, nc, nc):
        return dict(path="fused", quad=None, n_chunks=nc, hash_launches=1, levels_done=6, tree=merkle_launches(np2, 6))
    path = "one_chunk" if nc == 1 else "chunks+finish"
    return dict(path=path, quad=leaf_quad(n_cols, nc), n_chunks=nc, hash_launches=1 + (nc > 1), levels_done=0,
                tree=merkle_launches(np2, 0))

"""GPU tests at BASELINE.json's full sizes (C2, C3, C5 / headline, C4's commitment on one GPU).
  * the WHOLE `hashes` array (every leaf digest, every Merkle layer, the root) == the oracle's commit of the same
    coefficients, at 2^24 and 2^26 Ligero and 2^24 Brakedown (the C oracle needs a few seconds and ~10 GB of host
    memory at 2^26; at 2^28 it would need 40 GB, so that size keeps to the checks below);
  * sampled rows of comm == oracle encode of the same coefficient row (bit-exact);
  * sampled columns: leaf digest == oracle hash of the opened column; Merkle path folds to the root;
  * linearity: columns of commit(a + b) == columns of commit(a) + columns of commit(b) (a + b formed on the GPU);
  * prove at full size -> the *oracle's* verify accepts and returns the true evaluation, and (wherever the oracle holds the
    whole commitment anyway) the proof bytes == the oracle prover's bytes on the same transcript;
  * the reference's other two published rate series (lcpc-ligero-pc/src/tests.rs:59-98: rho = 1/4 default, 38/39 "isz") at
    2^26 and 2^25, whole tree + proof bytes.
A whole-tree comparison that cannot run for lack of host memory FAILS (it used to skip): a skipped comparison would silently
downgrade a full-size parity claim to a sampled one.  At 2^28 the oracle's Commit.commit would need ~40 GB of host memory, so
the whole `hashes` array is compared with the oracle's STREAMING commit instead (tests/oracle_lib.py commit_streaming: ~2 GB;
tests/test_oracle_streaming.py pins it to Commit.commit) -- unconditionally; only the comparison of the proof bytes with the
oracle PROVER's, which needs the whole commitment on the host, is left to the smaller sizes there (the oracle VERIFIER checks
the 2^28 proof)."""
import random

import numpy as np
import pytest
import torch

import ctypes as C

import lcpc_amd
from common import mk_transcript, powers
from lcpc_amd import LcCommit, LigeroEncoding, SdigEncoding, Transcript

pytestmark = pytest.mark.gpu


def device_random_coeffs(enc, n, seed):
    """n uniform field elements over the whole of [0, p), generated on the GPU by Field::random (lcpc_random_coeffs_device, the
    bench's generator); a torch int64 CUDA tensor viewed as (n, L) limbs."""
    return enc.random_coeffs_device(n, seed)


def host_memory_available():
    avail = None
    for line in open("/proc/meminfo"):
        if line.startswith("MemAvailable:"):
            avail = int(line.split()[1]) * 1024
    try:
        lim = open("/sys/fs/cgroup/memory.max").read().strip()
        if lim != "max":
            avail = min(avail, int(lim) - int(open("/sys/fs/cgroup/memory.current").read()))
    except Exception:
        pass
    return avail


def check_whole_tree(O, c, coeffs_dev, oenc, n_threads=16, need_factor=12):
    """the oracle commits the same coefficients on the host; every digest of LcCommit.hashes must agree.  Returns the oracle's
    commitment (for proof-byte comparisons).  Not enough host memory = failure, never a skip."""
    n = coeffs_dev.shape[0]
    need = need_factor * n * 8 * coeffs_dev.shape[1]          # coeffs (numpy + oracle copy) + comm (+ slack)
    avail = host_memory_available()
    if avail is not None and avail < need + (6 << 30):
        pytest.fail("not enough host memory for the oracle's whole-tree comparison at this size (%d GB free, %d GB needed): "
                    "the full-size parity claim cannot be checked on this box" % (avail >> 30, (need + (6 << 30)) >> 30))
    host = coeffs_dev.cpu().numpy().view(np.uint64)
    oc = O.Commit.commit(host, oenc, n_threads=n_threads)
    assert c.get_root() == oc.get_root()
    assert (c.hashes() == oc.hashes()).all()
    return oc


def check_sampled(O, fid, enc, oenc, c, coeffs_host_rows, rnd, n_row_samples=2, n_col_samples=24):
    L = O.limbs(fid)
    root = c.get_root()
    hashes = c.hashes()
    for r in coeffs_host_rows:
        row = np.zeros((c.n_cols, L), np.uint64)
        row[:c.n_per_row] = coeffs_host_rows[r]
        assert (c.comm(r, 1) == oenc.encode(row)).all(), "row %d" % r
    cols = [0, c.n_cols - 1] + [rnd.randrange(c.n_cols) for _ in range(n_col_samples)]
    vals, paths = c.open_columns(cols)
    for k, col in enumerate(cols):
        h = O.hash_column(fid, vals[k])
        assert h == bytes(hashes[col])
        cn = col
        for p in paths[k]:
            h = O.blake3(h + bytes(p)) if cn % 2 == 0 else O.blake3(bytes(p) + h)
            cn >>= 1
        assert h == root
    assert bytes(hashes[-1]) == root


def run_ligero_fullsize(O, log_len, rho, dims, linearity):
    fid = 3
    rnd = random.Random(log_len * 100 + rho[1])
    n = 1 << log_len
    enc = LigeroEncoding.new(fid, n, rho=rho)
    nr, npr, nc = enc.get_dims(n)
    assert (nr, npr, nc) == dims
    coeffs = device_random_coeffs(enc, n, 5)
    c = LcCommit.commit_device(coeffs.data_ptr(), n, enc, torch.cuda.current_stream().cuda_stream)
    oenc = O.Encoding.ligero_from_dims(fid, npr, nc, rho=rho)
    rows = {}
    for r in (0, rnd.randrange(nr), nr - 1):
        row = np.zeros((npr, 4), np.uint64)
        chunk = coeffs[r * npr:min(n, (r + 1) * npr)].cpu().numpy().view(np.uint64)
        row[:chunk.shape[0]] = chunk
        rows[r] = row
    check_sampled(O, fid, enc, oenc, c, rows, rnd)
    # prove at full size; the oracle's verifier (CPU, sub-linear) must accept
    import pyref as P
    F = P.FIELDS[fid]
    x = rnd.randrange(F.p)
    inner = powers(O, fid, x, npr)
    outer = powers(O, fid, x, nr, npr)
    root = c.get_root()
    pf = c.prove(outer, enc, mk_transcript(Transcript, root, enc.get_n_col_opens()))
    # published proof sizes exist for odd exponents only; the size formula is checked instead
    assert len(pf.to_bytes()) == P.proof_size(F, nr, npr, nc, enc.get_n_col_opens(), enc.get_n_degree_tests())
    rc, ev = O.verify(oenc, root, outer, inner, pf.to_bytes(), mk_transcript(O.Transcript, root, enc.get_n_col_opens()))
    assert rc == 0
    # the evaluation equals <inner, eval_outer(outer)> recomputed by the oracle from the proof's p_eval
    ev_prod = pf.verify(root, outer, inner, enc, mk_transcript(Transcript, root, enc.get_n_col_opens()))
    assert (ev_prod == ev).all()
    # whole tree, and the oracle PROVER's bytes on the same transcript (lcpc-2d/src/lib.rs:1004-1093).  2^28: the oracle's
    # streaming commit (row blocks fetched from the device, ~2 GB of host memory) gives the same `hashes` array
    if log_len > 26:
        rows_of = lambda r0, r1: coeffs[r0 * npr:min(n, r1 * npr)].cpu().numpy().view(np.uint64)
        oh = O.commit_streaming(oenc, n, rows_of, n_threads=16)
        assert oh[-1].tobytes() == root
        assert (c.hashes() == oh).all()
        del oh
    else:
        oc = check_whole_tree(O, c, coeffs, oenc)
        opf, _ = oc.prove(outer, oenc, mk_transcript(O.Transcript, root, oenc.get_n_col_opens()))
        assert pf.to_bytes() == opf, "proof bytes differ from the oracle prover's"
        del oc, opf
    if not linearity:
        return
    # linearity of commit on sampled columns: comm(a + b) == comm(a) + comm(b), with a + b formed on the GPU
    # (lcpc_field_sum_device) and the column sums on the host (oracle field add)
    cols = [0, nc - 1] + [rnd.randrange(nc) for _ in range(8)]
    va, _ = c.open_columns(cols)
    ab = torch.empty((2, n, 4), dtype=torch.int64, device="cuda")
    ab[0].copy_(coeffs)
    enc.random_coeffs_device(n, 6, out_ptr=ab[1].data_ptr())
    total = torch.empty((n, 4), dtype=torch.int64, device="cuda")
    st = torch.cuda.current_stream().cuda_stream
    enc._check(lcpc_amd._lib.lib().lcpc_field_sum_device(enc._h, C.c_void_p(ab.data_ptr()), 2, n, C.c_void_p(st), C.c_void_p(total.data_ptr())))
    vb, _ = LcCommit.commit_device(ab[1].data_ptr(), n, enc, st).open_columns(cols)
    del ab
    vs, _ = LcCommit.commit_device(total.data_ptr(), n, enc, st, borrow=True).open_columns(cols)
    a_h, b_h = np.ascontiguousarray(va.reshape(-1, 4)), np.ascontiguousarray(vb.reshape(-1, 4))
    s = np.zeros_like(a_h)
    O.lib().lo_f_add(fid, O.ptr(a_h), O.ptr(b_h), O.ptr(s), a_h.shape[0])
    assert (vs.reshape(-1, 4) == s).all()
    assert not (vs.reshape(-1, 4) == a_h).all()


@pytest.mark.parametrize("log_len", [24, 26, 28])
def test_ligero_ft255_fullsize(oracle, log_len):
    """BASELINE configs[1] (2^24), the headline / configs[4] (2^26) and configs[3]'s commitment (2^28, here on ONE
    GPU: 8 + 16 GiB, 33 BLAKE3 chunks per leaf): commit + prove at full size, whole tree and proof bytes against the oracle."""
    dims = {24: (256, 65536, 131072), 26: (512, 131072, 262144), 28: (1024, 262144, 524288)}[log_len]
    run_ligero_fullsize(oracle, log_len, (1, 2), dims, linearity=log_len <= 26)


@pytest.mark.parametrize("log_len,rho,dims", [(26, (1, 4), (1024, 65536, 262144)), (25, (38, 39), (132, 255422, 262144))])
def test_ligero_ft255_fullsize_other_rates(oracle, log_len, rho, dims):
    """the reference's other two rate series at scale (lcpc-ligero-pc/src/tests.rs:59-98; doc/benchmark-results/
    20210807_64c_255bit_ligero_{dfl,isz}.txt): rho = 1/4 at 2^26 (8 GiB of comm, 33 chunks per leaf) and rho = 38/39 at 2^25
    (ragged last row, no zero half in the first NTT round)."""
    run_ligero_fullsize(oracle, log_len, rho, dims, linearity=False)


def test_brakedown_ft255_2e24(oracle):
    """BASELINE configs[2]: 101 x 166292 -> 252931, SdigCode3, seed 0."""
    O, fid = oracle, 3
    rnd = random.Random(3)
    n = 1 << 24
    enc = SdigEncoding.new(fid, n, 0)
    nr, npr, nc = enc.get_dims(n)
    assert (nr, npr, nc) == (101, 166292, 252931)
    coeffs = device_random_coeffs(enc, n, 8)
    c = LcCommit.commit_device(coeffs.data_ptr(), n, enc, torch.cuda.current_stream().cuda_stream)
    oenc = O.Encoding.sdig_from_dims(fid, npr, nc, 0, 3)
    rows = {}
    for r in (0, nr - 1):
        row = np.zeros((npr, 4), np.uint64)
        chunk = coeffs[r * npr:min(n, (r + 1) * npr)].cpu().numpy().view(np.uint64)
        row[:chunk.shape[0]] = chunk
        rows[r] = row
    check_sampled(O, fid, enc, oenc, c, rows, rnd, n_col_samples=12)
    assert (c.hashes()[nc:1 << 18] == 0).all()      # Merkle padding leaves stay zero (lcpc-2d lib.rs:656-666)
    oc = check_whole_tree(O, c, coeffs, oenc)
    # the oracle prover's bytes on the same transcript (6593 opened columns)
    import pyref as P
    x = rnd.randrange(P.FIELDS[fid].p)
    outer = powers(O, fid, x, nr, npr)
    root = c.get_root()
    pf = c.prove(outer, enc, mk_transcript(Transcript, root, enc.get_n_col_opens()))
    opf, _ = oc.prove(outer, oenc, mk_transcript(O.Transcript, root, oenc.get_n_col_opens()))
    assert pf.to_bytes() == opf
    del oc, opf
    # the whole encoded matrix of the first and last 3 rows == the oracle's (the position-major commitment read back row-major)
    host = coeffs.cpu().numpy().view(np.uint64)
    for r0 in (0, nr - 3):
        blk = np.zeros((3 * npr, 4), np.uint64)
        part = host[r0 * npr:min(n, (r0 + 3) * npr)]
        blk[:part.shape[0]] = part
        assert (c.comm(r0, 3) == O.Commit.commit(blk, oenc, n_threads=4).comm()).all()


def test_c4_fullsize_row_sharded_emulated(oracle):
    """BASELINE configs[3] as specified except for the wire: 2^28 Ft255 coefficients (1024 x 262144 -> 524288), rows split
    over 8 shard contexts (128 rows each, as on 8 GPUs) that here share ONE device; the all-gather of the subtree nodes is
    emulated by placing each rank's nodes in the gather buffer.  Every rank's root and full `hashes` must equal the
    unsharded 2^28 commit (which test_ligero_ft255_fullsize[28] pins to the oracle by rows, columns and proof)."""
    from test_gpu_sharded import run_sharded
    fid, n = 3, 1 << 28
    enc = LigeroEncoding.new(fid, n)
    nr, npr, nc = enc.get_dims(n)
    assert (nr, npr, nc) == (1024, 262144, 524288)
    coeffs = device_random_coeffs(enc, n, 9)
    ref = LcCommit.commit_device(coeffs.data_ptr(), n, enc, torch.cuda.current_stream().cuda_stream, borrow=True)
    root, hashes = ref.get_root(), ref.hashes().copy()
    del ref, enc
    torch.cuda.empty_cache()
    roots, engines = run_sharded(lambda sh: LigeroEncoding.new_from_dims(fid, npr, nc, shard=sh), 8, coeffs.reshape(nr, npr, 4), nr)
    assert all(r == root for r in roots)
    n_rows_seen = 0
    for g, eng in enumerate(engines):
        rb, re, cb, ce, nch = eng.layout(nr)
        # 33 chunks of 32 rows (the leaf message starts with a 32-byte prefix: chunk 0 holds 31 rows) over 8 ranks: 4 or 5 chunks each
        assert nch == 33 and rb == n_rows_seen and 127 <= re - rb <= 160
        n_rows_seen = re
        assert (eng.cm.hashes() == hashes).all(), "rank %d" % g
    assert n_rows_seen == nr


def test_ligero_ft255_2e26_maximal_operands(oracle):
    """The headline shape (2^26 Ft255 Ligero, 512 x 131072 -> 262144) with every coefficient the maximal stored pattern MAXC, the
    largest value < p whose eight low 29-bit limbs are all 2^29 - 1: every product of the row NTT's first round and of the collapse
    (collapse29_kernel at 1 split of 512 rows: lazy29 REDC chunks of 60 rows, normalise every 6) is at its largest.  Whole tree ==
    the oracle's commit; eval_outer of the tensor whose 2^261 form is MAXC == the Python-int sum 512 * t * MAXC / R mod p in every
    column; the proof bytes == the oracle prover's."""
    import pyref as P
    from common import maxc, maxt, to_int
    O, fid = oracle, 3
    p = P.FIELDS[fid].p
    n = 1 << 26
    enc = LigeroEncoding.new(fid, n)
    nr, npr, nc = enc.get_dims(n)
    assert (nr, npr, nc) == (512, 131072, 262144)
    limbs = [(maxc(fid) >> (64 * k)) & ((1 << 64) - 1) for k in range(4)]
    row = torch.tensor(np.array(limbs, np.uint64).view(np.int64), device="cuda")
    coeffs = row.expand(n, 4).contiguous()
    c = LcCommit.commit_device(coeffs.data_ptr(), n, enc, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    oenc = O.Encoding.ligero_from_dims(fid, npr, nc)
    oc = check_whole_tree(O, c, coeffs, oenc)
    t = np.array([[(maxt(fid) >> (64 * k)) & ((1 << 64) - 1) for k in range(4)]] * nr, np.uint64)
    poly = c.eval_outer(t)
    want = nr * maxt(fid) * maxc(fid) * pow(1 << 256, -1, p) % p
    assert to_int(poly[0]) == want
    assert (poly == poly[0]).all()
    root = c.get_root()
    pf = c.prove(t, enc, mk_transcript(Transcript, root, enc.get_n_col_opens()))
    opf, _ = oc.prove(t, oenc, mk_transcript(O.Transcript, root, oenc.get_n_col_opens()))
    assert pf.to_bytes() == opf
    del oc, opf

"""Edge cases on the GPU path: smallest shapes, single rows, length-1 inputs, maximum sizes, and the error
behaviour of the reference's Result enums / asserts (lcpc-2d/src/lib.rs:111-166, 630-632; ligero lib.rs:114-148)
mirrored as lcpc_status codes."""
import numpy as np
import pytest

import lcpc_amd
from common import mk_transcript
from lcpc_amd import LcCommit, LcEvalProof, LigeroEncoding, SdigEncoding, Transcript

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("fid", [0, 1, 2, 3])
@pytest.mark.parametrize("n_per_row,n_cols", [(1, 2), (1, 4), (3, 4), (7, 8), (2, 16)])
def test_tiny_shapes(oracle, fid, n_per_row, n_cols):
    """n_cols = 2..16 (log_n = 1 has a single, multiplication-free stage), 1..5 rows, ragged tails."""
    O = oracle
    for n in (1, n_per_row, n_per_row + 1, 5 * n_per_row - (1 if n_per_row > 1 else 0)):
        coeffs = O.random_elems(fid, n, n + n_cols)
        enc = LigeroEncoding.new_from_dims(fid, n_per_row, n_cols)
        oenc = O.Encoding.ligero_from_dims(fid, n_per_row, n_cols)
        c = LcCommit.commit(coeffs, enc)
        oc = O.Commit.commit(coeffs, oenc)
        assert (c.n_rows, c.n_per_row, c.n_cols) == (oc.n_rows, oc.n_per_row, oc.n_cols)
        assert (c.comm() == oc.comm()).all() and (c.coeffs() == oc.coeffs()).all()
        assert (c.hashes() == oc.hashes()).all() and c.get_root() == oc.get_root()
        t = O.random_elems(fid, c.n_rows, 3)
        assert (c.eval_outer(t) == oc.collapse(t)).all()
        # full prove/verify round trip on the tiny commitment (309 openings of a handful of columns)
        root = c.get_root()
        pf = c.prove(t, enc, mk_transcript(Transcript, root, enc.get_n_col_opens()))
        opf, _ = oc.prove(t, oenc, mk_transcript(O.Transcript, root, enc.get_n_col_opens()))
        assert pf.to_bytes() == opf
        inner = O.random_elems(fid, c.n_per_row, 4)
        ev = pf.verify(root, t, inner, enc, mk_transcript(Transcript, root, enc.get_n_col_opens()))
        rc, oev = O.verify(oenc, root, t, inner, opf, mk_transcript(O.Transcript, root, enc.get_n_col_opens()))
        assert rc == 0 and (ev == oev).all()


def test_all_zero_and_extreme_values(oracle):
    """coefficients 0, 1 and p-1 (Montgomery forms 0, R, p-R): carries / conditional subtractions at the borders."""
    O = oracle
    import pyref as P
    for fid in (0, 3):
        F = P.FIELDS[fid]
        vals = [0, 1, F.p - 1, 2, F.p - 2, (F.p - 1) // 2, (F.p + 1) // 2] * 40
        coeffs = O.to_mont(fid, vals)
        for enc, oenc in ((LigeroEncoding.new_from_dims(fid, 32, 64), O.Encoding.ligero_from_dims(fid, 32, 64)),
                          (LigeroEncoding.new_from_dims(fid, 2048, 4096), O.Encoding.ligero_from_dims(fid, 2048, 4096))):
            c = LcCommit.commit(coeffs, enc)
            oc = O.Commit.commit(coeffs, oenc)
            assert (c.comm() == oc.comm()).all() and c.get_root() == oc.get_root()
        z = np.zeros((300, O.limbs(fid)), np.uint64)
        enc, oenc = LigeroEncoding.new_from_dims(fid, 32, 64), O.Encoding.ligero_from_dims(fid, 32, 64)
        assert LcCommit.commit(z, enc).get_root() == O.Commit.commit(z, oenc).get_root()


def test_single_row_many_columns(oracle):
    """n_rows = 1: leaf message = 32 + F bytes, one BLAKE3 block; n_cols = 2^13 (two NTT passes for Ft255)."""
    O = oracle
    for fid, k in ((3, 13), (0, 14)):
        n = 1 << (k - 1)
        coeffs = O.random_elems(fid, n, 77)
        enc, oenc = LigeroEncoding.new_from_dims(fid, n, 2 * n), O.Encoding.ligero_from_dims(fid, n, 2 * n)
        c, oc = LcCommit.commit(coeffs, enc), O.Commit.commit(coeffs, oenc, n_threads=4)
        assert c.n_rows == 1 and (c.hashes() == oc.hashes()).all()


def test_constructor_errors():
    E = lcpc_amd.LcpcError
    with pytest.raises(E) as e:                                  # _dims_ok: n_per_row < n_cols (ligero lib.rs:114-118)
        LigeroEncoding.new_from_dims(3, 64, 64)
    assert e.value.code == lcpc_amd.ERR_DIMS
    with pytest.raises(E) as e:                                  # n_cols must be a power of two
        LigeroEncoding.new_from_dims(3, 10, 48)
    assert e.value.code == lcpc_amd.ERR_DIMS
    with pytest.raises(E) as e:                                  # rho_num < rho_den (ligero lib.rs:56)
        LigeroEncoding.new(3, 1 << 12, rho=(2, 2))
    assert e.value.code == lcpc_amd.ERR_ARG
    with pytest.raises(E) as e:                                  # unknown field id
        LigeroEncoding.new(9, 1 << 12)
    assert e.value.code == lcpc_amd.ERR_ARG
    with pytest.raises(E) as e:                                  # n_cols beyond the device path's 2^30 (and ft127's 2^40 cap upstream)
        LigeroEncoding.new_from_dims(0, 1 << 30, 1 << 31)
    assert e.value.code in (lcpc_amd.ERR_TOO_BIG, lcpc_amd.ERR_DIMS)
    with pytest.raises(E) as e:                                  # new_from_dims with a codeword length that matgen does not produce
        SdigEncoding.new_from_dims(3, 600, 1000, 0)
    assert e.value.code == lcpc_amd.ERR_DIMS
    with pytest.raises(E) as e:                                  # n <= baselen: matgen::get_dims assert (matgen.rs:62)
        SdigEncoding.new_from_dims(3, 20, 40, 0)
    assert e.value.code == lcpc_amd.ERR_DIMS
    with pytest.raises(E) as e:                                  # invalid SDIG code
        SdigEncoding.new(3, 1 << 12, 0, code=7)
    assert e.value.code == lcpc_amd.ERR_ARG
    with pytest.raises(E) as e:                                  # shard rank outside the shard count
        LigeroEncoding.new_from_dims(3, 64, 128, shard=(2, 2))
    assert e.value.code == lcpc_amd.ERR_ARG
    LigeroEncoding.new_from_dims(2, 64, 128, shard=(0, 2))       # (ft191 shards since round 4: tests/test_gpu_sharded.py)


def test_state_and_argument_errors(oracle):
    O = oracle
    E = lcpc_amd.LcpcError
    enc = LigeroEncoding.new_from_dims(0, 64, 128)
    empty = LcCommit(enc)                                        # lcpc_commit_create: bound to enc, nothing committed yet
    for call in (empty.get_root, empty.hashes, lambda: empty.open_columns([0]),
                 lambda: empty.prove(O.random_elems(0, 1, 2), enc, Transcript(b"t"))):
        with pytest.raises(E) as e:
            call()
        assert e.value.code == lcpc_amd.ERR_STATE
    with pytest.raises(E) as e:                                  # empty input (the reference asserts n_rows >= 1, lib.rs:630-631)
        LcCommit.commit(np.zeros((0, 1), np.uint64), enc)
    assert e.value.code == lcpc_amd.ERR_ARG
    c = LcCommit.commit(O.random_elems(0, 1000, 1), enc)
    with pytest.raises(E) as e:                                  # ProverError::OuterTensor (lib.rs:1016-1018)
        c.prove(O.random_elems(0, c.n_rows + 1, 2), enc, Transcript(b"t"))
    assert e.value.code == lcpc_amd.ERR_OUTER_TENSOR
    with pytest.raises(E) as e:                                  # ProverError::ColumnNumber (lib.rs:797-799)
        c.open_columns([0, 5, 128])
    assert e.value.code == lcpc_amd.ERR_COLUMN_NUMBER
    with pytest.raises(E) as e:                                  # encode(): row length != n_cols
        enc.encode(np.zeros((100, 1), np.uint64))
    assert e.value.code == lcpc_amd.ERR_ENCODE
    other = LigeroEncoding.new_from_dims(0, 64, 128)
    with pytest.raises(E) as e:                                  # prove with an encoding that does not own the commitment (check_comm)
        c.prove(O.random_elems(0, c.n_rows, 2), other, Transcript(b"t"))
    assert e.value.code == lcpc_amd.ERR_COMMIT
    # VerifierError::NumColOpens (lib.rs:845-848): truncate the columns vector of a valid proof
    t = O.random_elems(0, c.n_rows, 2)
    pf = c.prove(t, enc, Transcript(b"t"))
    raw = bytearray(pf.to_bytes())
    n_deg = enc.get_n_degree_tests()
    off = 8 + (8 + 64 * 8) + 8 + n_deg * (8 + 64 * 8)           # offset of the `columns` length prefix
    assert int.from_bytes(raw[off:off + 8], "little") == enc.get_n_col_opens()
    per_col = 8 + c.n_rows * 8 + 8 + 7 * 40
    cut = bytes(raw[:off]) + (enc.get_n_col_opens() - 1).to_bytes(8, "little") + bytes(raw[off + 8:len(raw) - per_col])
    with pytest.raises(E) as e:
        LcEvalProof.from_bytes(cut, 1).verify(c.get_root(), t, O.random_elems(0, 64, 3), enc, Transcript(b"t"))
    assert e.value.code == lcpc_amd.VERR_NUM_COL_OPENS
    # VerifierError::EncodingDims (lib.rs:858-860): verify against an encoding of a different shape
    wrong = LigeroEncoding.new_from_dims(0, 32, 128)
    with pytest.raises(E) as e:
        pf.verify(c.get_root(), t, O.random_elems(0, 64, 3), wrong, Transcript(b"t"))
    assert e.value.code == lcpc_amd.VERR_ENCODING_DIMS


def test_rate_variants_2e20(oracle):
    """the three rates the reference benchmarks (1/2 `hlf`, 1/4 default, 38/39 `isz`; ligero tests.rs:59-69) at 2^20
    Ft255: sampled rows/columns against the oracle (non-power-of-two n_per_row for 38/39: 2^k * 38 / 39)."""
    import random
    O = oracle
    rnd = random.Random(1)
    n = 1 << 20
    coeffs = O.random_elems(3, n, 8)
    for rho in ((1, 2), (1, 4), (38, 39)):
        enc, oenc = LigeroEncoding.new(3, n, rho), O.Encoding.ligero(3, n, rho)
        assert enc.get_dims(n) == oenc.get_dims(n)
        c = LcCommit.commit(coeffs, enc)
        nr, npr, nc = enc.get_dims(n)
        for r in (0, nr - 1, rnd.randrange(nr)):
            row = np.zeros((nc, 4), np.uint64)
            chunk = coeffs[r * npr:min(n, (r + 1) * npr)]
            row[:chunk.shape[0]] = chunk
            assert (c.comm(r, 1) == oenc.encode(row)).all(), (rho, r)
        cols = [0, nc - 1] + [rnd.randrange(nc) for _ in range(10)]
        vals, paths = c.open_columns(cols)
        hashes, root = c.hashes(), c.get_root()
        for k, col in enumerate(cols):
            h = O.hash_column(3, vals[k])
            assert h == bytes(hashes[col])
            cn = col
            for p in paths[k]:
                h = O.blake3(h + bytes(p)) if cn % 2 == 0 else O.blake3(bytes(p) + h)
                cn >>= 1
            assert h == root


def test_lazy_limb_ntt_range_stress(oracle):
    """The Ft255 NTT keeps elements loosely reduced between stages (signed 29-bit limbs, |value| < 4p) and relies on
    the range analysis of its multiplier and of a quotient-estimate clamp (field_ln.h, LnField<FT255>).  Inputs chosen to push every bound: rows of
    all p-1, all (p-1)/2, alternating 0 / p-1, and limbs with all 29-bit fields saturated -- at n_cols = 2^12 (one
    pass), 2^13 (two passes) and 2^18 (the headline row: 4+5 radix-4 rounds), rates 1/2 and 38/39 (n_per_row not a
    power of two); nearly full rows (38/39) at 2^19 / 2^20 (first passes of 9 / 10 stages, blk0_gone) and 2^21 (three passes),
    where no zero half shapes the stage inputs.  Bit-exact against the oracle."""
    import pyref as P
    O = oracle
    F = P.FT255
    sat = sum(((1 << 29) - 1) << (29 * k) for k in range(9)) % F.p
    pats = [[F.p - 1], [(F.p - 1) // 2], [0, F.p - 1], [sat, F.p - 2, 1], [F.p - 1, F.p - 1, F.p - 1, 0]]
    for log_n, n_per_row in ((12, 2048), (13, 4096), (13, 7983), (18, 131072), (19, (1 << 19) * 38 // 39), (20, (1 << 20) * 38 // 39),
                             (21, (1 << 21) * 38 // 39)):
        n = 1 << log_n
        enc = LigeroEncoding.new_from_dims(3, n_per_row, n)
        oenc = O.Encoding.ligero_from_dims(3, n_per_row, n)
        rows = np.zeros((len(pats), n, 4), np.uint64)
        for r, pat in enumerate(pats):
            m = O.to_mont(3, pat)
            reps = (n_per_row + len(pat) - 1) // len(pat)
            rows[r, :n_per_row] = np.tile(m, (reps, 1))[:n_per_row]
        got = enc.encode(rows).reshape(len(pats), n, 4)
        for r in range(len(pats)):
            assert (got[r] == oenc.encode(rows[r].copy())).all(), (log_n, n_per_row, r)


@pytest.mark.parametrize("log_n,n_per_row,n_rows", [(1, 1, 3), (2, 2, 5), (3, 4, 2), (5, 16, 33), (10, 512, 4), (11, 1024, 3), (11, 2047, 2),
                                                    (12, 1024, 3), (13, 4096, 2), (13, 7983, 2), (17, 65536, 2)])
def test_canonical_comm_commit_stress(oracle, log_n, n_per_row, n_rows):
    """The Ft255 Ligero commit keeps comm in canonical form on the device: the conversion rides on the NTT's twiddle
    multiplies (second table for "block 0" butterflies, an explicit reduction for the 2 or 4 elements per row that
    only ever meet trivial twiddles) and the column hash reads the result as it is.  Shapes cover: one stage only,
    a single radix-4 round, odd stage counts (radix-2 tail), one and two passes, rates 1/2 (zero upper half in the
    first round), 1/4 and ~1 (generic block-0 path).  Inputs push the signed lazy-limb bounds (all p-1, saturated
    29-bit fields, alternating 0 / p-1).  comm read back through the ABI is Montgomery form again, columns opened
    by prove() too."""
    import pyref as P
    O = oracle
    F = P.FT255
    n = 1 << log_n
    sat = sum(((1 << 29) - 1) << (29 * k) for k in range(9)) % F.p
    pats = [[F.p - 1], [0, F.p - 1], [sat, F.p - 2, 1], [(F.p - 1) // 2, F.p - 1, F.p - 1, 0, 3]]
    enc = LigeroEncoding.new_from_dims(3, n_per_row, n)
    oenc = O.Encoding.ligero_from_dims(3, n_per_row, n)
    for pi, pat in enumerate(pats):
        n_coeffs = n_rows * n_per_row - (pi % 2)                    # ragged last row every other time
        reps = (n_coeffs + len(pat) - 1) // len(pat)
        coeffs = np.tile(O.to_mont(3, pat), (reps, 1))[:n_coeffs]
        c = LcCommit.commit(coeffs, enc)
        oc = O.Commit.commit(coeffs, oenc)
        assert (c.comm() == oc.comm()).all(), (log_n, pi)
        assert (c.coeffs() == oc.coeffs()).all()
        assert (c.hashes() == oc.hashes()).all() and c.get_root() == oc.get_root()
        if c.n_rows > 1:
            assert (c.comm(1, 1) == oc.comm()[n:2 * n]).all()       # partial read-out converts the right rows
    coeffs = O.random_elems(3, n_rows * n_per_row, 5 + log_n)
    c = LcCommit.commit(coeffs, enc)
    oc = O.Commit.commit(coeffs, oenc)
    root = c.get_root()
    assert root == oc.get_root()
    t = O.random_elems(3, c.n_rows, 9)
    pf = c.prove(t, enc, mk_transcript(Transcript, root, enc.get_n_col_opens()))
    opf, _ = oc.prove(t, oenc, mk_transcript(O.Transcript, root, enc.get_n_col_opens()))
    assert pf.to_bytes() == opf


def test_concurrent_contexts_and_streams(oracle):
    """include/lcpc_hip.h: contexts are independent and may be used from different host threads at the same time; a
    device-resident commit may be given any HIP stream.  Four threads, each with its own context (two Ligero shapes,
    one Brakedown, one Ft63) and its own non-default stream, commit 5 different inputs each while the others run; every
    root must equal the oracle's."""
    import threading
    import torch
    O = oracle
    specs = [("ligero", 3, 1 << 16, 11), ("ligero", 3, 50000, 12), ("sdig", 3, 40000, 13), ("ligero", 0, 1 << 17, 14)]
    jobs = []
    for kind, fid, n, seed in specs:
        if kind == "ligero":
            enc, oenc = LigeroEncoding.new(fid, n), O.Encoding.ligero(fid, n)
        else:
            enc, oenc = SdigEncoding.new(fid, n, 7), O.Encoding.sdig(fid, n, 7)
        data = [O.random_elems(fid, n, seed * 10 + i) for i in range(5)]
        want = [O.Commit.commit(d, oenc, n_threads=2).get_root() for d in data]
        jobs.append((enc, data, want))
    errs = []

    def work(enc, data, want):
        try:
            st = torch.cuda.Stream()
            for d, w in zip(data, want):
                dev = torch.from_numpy(d.view(np.int64)).cuda()
                st.wait_stream(torch.cuda.current_stream())
                c = LcCommit.commit_device(dev.data_ptr(), d.shape[0], enc, st.cuda_stream, sync=True)
                if c.get_root() != w:
                    errs.append("root mismatch")
        except Exception as e:
            errs.append(repr(e))

    th = [threading.Thread(target=work, args=j) for j in jobs]
    for t in th:
        t.start()
    for t in th:
        t.join(300)
    assert not errs, errs


def test_concurrent_prove_and_verify_one_encoder(oracle):
    """one encoder shared by several host threads (the reference shares &E across Rayon workers, lib.rs:74-104): three
    commitments under it prove at the same time (each LcCommit has its own lock and buffers; the proof-buffer pool and the
    host worker pool are shared), then every proof is verified from three threads at once on that same context (verifies on
    one context are serialised internally).  Proof bytes must equal the oracle's, verdicts must all be accepts."""
    import threading
    from common import mk_transcript, powers
    from lcpc_amd import Transcript
    O, fid, n = oracle, 3, 1 << 14
    enc, oenc = LigeroEncoding.new(fid, n), O.Encoding.ligero(fid, n)
    nco = enc.get_n_col_opens()
    import pyref as P
    jobs = []
    for i in range(3):
        coeffs = O.random_elems(fid, n, 300 + i)
        c = LcCommit.commit(coeffs, enc)
        x = (0xabcdef + i) % P.FIELDS[fid].p
        inner, outer = powers(O, fid, x, c.n_per_row), powers(O, fid, x, c.n_rows, c.n_per_row)
        oc = O.Commit.commit(coeffs, oenc, n_threads=2)
        want, _ = oc.prove(outer, oenc, mk_transcript(O.Transcript, oc.get_root(), nco))
        jobs.append({"c": c, "root": c.get_root(), "inner": inner, "outer": outer, "want": want, "pf": []})
    errs = []

    def prove(j):
        try:
            for _ in range(6):
                pf = j["c"].prove(j["outer"], enc, mk_transcript(Transcript, j["root"], nco))
                if pf.to_bytes() != j["want"]:
                    errs.append("proof bytes differ")
                j["pf"].append(pf)
                del j["pf"][:-2]                     # older proofs are freed while other threads allocate theirs
        except Exception as e:
            errs.append(repr(e))

    def verify(j):
        try:
            for _ in range(6):
                j["pf"][-1].verify(j["root"], j["outer"], j["inner"], enc, mk_transcript(Transcript, j["root"], nco))
        except Exception as e:
            errs.append(repr(e))

    for fn in (prove, verify):
        th = [threading.Thread(target=fn, args=(j,)) for j in jobs]
        for t in th:
            t.start()
        for t in th:
            t.join(300)
        assert not errs, errs


@pytest.mark.parametrize("switch", ["LCPC_NTT_GENERAL"])
def test_ab_switch_paths_stay_correct(oracle, switch):
    """LCPC_NTT_GENERAL selects the general NTT kernel (K1) where a shape-specialised plan exists.  It is read
    when the context is created; the path must keep producing the oracle's commitment and proof."""
    import os
    O = oracle
    n = 3 * 4096 - 5
    coeffs = O.random_elems(3, n, 77)
    oenc = O.Encoding.ligero_from_dims(3, 4096, 8192)
    oc = O.Commit.commit(coeffs, oenc)
    os.environ[switch] = "1"
    try:
        enc = LigeroEncoding.new_from_dims(3, 4096, 8192)
    finally:
        del os.environ[switch]
    c = LcCommit.commit(coeffs, enc)
    assert (c.comm() == oc.comm()).all() and (c.hashes() == oc.hashes()).all()
    root = c.get_root()
    t = O.random_elems(3, c.n_rows, 78)
    pf = c.prove(t, enc, mk_transcript(Transcript, root, enc.get_n_col_opens()))
    opf, _ = oc.prove(t, oenc, mk_transcript(O.Transcript, root, enc.get_n_col_opens()))
    assert pf.to_bytes() == opf


@pytest.mark.parametrize("fid", [0, 1, 2, 3])
def test_brakedown_position_major_commitment_forms(oracle, fid):
    """Brakedown commits with >= 24 rows keep the commitment position-major on the device, as canonical values (converted once
    in the input transpose; every level is linear and keeps the form; the column hash reads them as they are).  Everything that
    leaves the library -- comm, coeffs, hashes, opened columns, proof bytes, the bincode of the commitment -- is the oracle's."""
    O = oracle
    n_per_row, n_rows = 900, 37
    oenc = O.Encoding.sdig_from_dims(fid, n_per_row, 0, 5)
    _, _, n_cols = oenc.get_dims(n_per_row)
    enc = SdigEncoding.new_from_dims(fid, n_per_row, n_cols, 5)
    coeffs = O.random_elems(fid, n_rows * n_per_row - 11, 40 + fid)
    c = LcCommit.commit(coeffs, enc)
    oc = O.Commit.commit(coeffs, oenc, n_threads=4)
    assert c.get_root() == oc.get_root() and (c.hashes() == oc.hashes()).all()
    cols = [0, 1, n_per_row - 1, n_per_row, n_cols - 1, n_cols // 2 + 3]
    vals, paths = c.open_columns(cols)
    ocomm = oc.comm().reshape(n_rows, n_cols, fid + 1)
    assert (vals == ocomm[:, cols].transpose(1, 0, 2)).all()
    assert (c.comm() == oc.comm()).all() and (c.coeffs() == oc.coeffs()).all()
    root = c.get_root()
    t = O.random_elems(fid, c.n_rows, 79)
    pf = c.prove(t, enc, mk_transcript(Transcript, root, enc.get_n_col_opens()))
    opf, _ = oc.prove(t, oenc, mk_transcript(O.Transcript, root, enc.get_n_col_opens()))
    assert pf.to_bytes() == opf
    from common import commit_bincode
    import io
    buf = io.BytesIO()
    c.to_bincode(buf)
    assert buf.getvalue() == commit_bincode(oc)


@pytest.mark.parametrize("n_rows", [37, 40, 48, 49, 101, 130, 167])
def test_brakedown_packed_tail_rows(oracle, n_rows):
    """Ft255 Brakedown, wide levels: a last group of <= 48 rows is computed by spmm_t_tail_kernel (lanes over (output, row) pairs,
    per-lane matrix entries) instead of a mostly idle wave of the lane = row kernel.  Equal to the oracle -- tail only (37, 40, 48 rows), just above the limit (49: no tail kernel), one and two whole groups
    before the tail (101, 130, 167).  n_per_row is large enough for the first levels to have >= 8192 outputs."""
    O, fid, n_per_row = oracle, 3, 70000
    oenc = O.Encoding.sdig_from_dims(fid, n_per_row, 0, 9)
    _, _, n_cols = oenc.get_dims(n_per_row)
    enc = SdigEncoding.new_from_dims(fid, n_per_row, n_cols, 9)
    coeffs = O.random_elems(fid, n_rows * n_per_row - 3, 50 + n_rows)
    oc = O.Commit.commit(coeffs, oenc, n_threads=8)
    c = LcCommit.commit(coeffs, enc)
    assert c.get_root() == oc.get_root()
    assert (c.hashes() == oc.hashes()).all()
    assert (c.comm() == oc.comm()).all()


def test_many_short_rows_exceed_grid_y(oracle):
    """A commitment made with new_from_dims and a small n_per_row has more BLAKE3 chunks per leaf message than a grid
    dimension may hold (65535): 2.2 M rows of 8 Ft255 coefficients -> 68 751 chunks.  The column hash launches the chunk
    range in slices; root and opened columns must still equal the oracle's."""
    O, fid = oracle, 3
    n_per_row, n_cols, n_rows = 8, 16, 2_200_001
    enc = LigeroEncoding.new_from_dims(fid, n_per_row, n_cols)
    oenc = O.Encoding.ligero_from_dims(fid, n_per_row, n_cols)
    coeffs = O.random_elems(fid, n_rows * n_per_row - 3, 91)
    c = LcCommit.commit(coeffs, enc)
    oc = O.Commit.commit(coeffs, oenc, n_threads=8)
    assert c.n_rows == n_rows
    assert c.get_root() == oc.get_root()
    assert (c.hashes() == oc.hashes()).all()
    vals, _ = c.open_columns([0, 15, 7])
    ocomm = oc.comm().reshape(n_rows, n_cols, 4)
    assert (vals == ocomm[:, [0, 15, 7]].transpose(1, 0, 2)).all()


def test_prove_right_after_async_commit_on_nonblocking_stream(oracle):
    """lcpc_commit_device with root = NULL only enqueues; prove / collapse / open / the getters run on the null stream, which a
    caller's NON-BLOCKING stream is not implicitly ordered with: the library orders them behind the commit by an event.  A 2^22
    commit (~1 ms of kernels) followed at once by the readers, several times over, against the oracle."""
    import torch
    from common import mk_transcript
    from lcpc_amd import Transcript
    O, fid, n = oracle, 3, 1 << 22
    enc, oenc = LigeroEncoding.new(fid, n), O.Encoding.ligero(fid, n)
    st = torch.cuda.Stream()                      # torch streams are created non-blocking
    for it in range(3):
        coeffs = O.random_elems(fid, n, 90 + it)
        dev = torch.from_numpy(coeffs.view(np.int64)).cuda()
        torch.cuda.synchronize()
        oc = O.Commit.commit(coeffs, oenc, n_threads=8)
        c = LcCommit(enc)
        with torch.cuda.stream(st):
            LcCommit.commit_device(dev.data_ptr(), n, enc, st.cuda_stream, sync=False, into=c)
        if it == 0:
            root = c.get_root()                   # getter right behind the enqueue
            assert root == oc.get_root()
        elif it == 1:
            t = O.random_elems(fid, c.n_rows, 5)
            assert (c.eval_outer(t) == oc.collapse(t)).all()
        root = oc.get_root()
        outer = O.random_elems(fid, oc.n_rows, 7)
        pf = c.prove(outer, enc, mk_transcript(Transcript, root, enc.get_n_col_opens()))
        opf, _ = oc.prove(outer, oenc, mk_transcript(O.Transcript, root, oenc.get_n_col_opens()))
        assert pf.to_bytes() == opf
        st.synchronize()


@pytest.mark.parametrize("kind", ["ligero", "sdig"])
@pytest.mark.parametrize("fid", [0, 1, 2, 3])
def test_commit_device_only_enqueues(kind, fid):
    """lcpc_commit_device with root = NULL must not wait for the GPU: no allocation, free or copy that synchronises may sit in the
    steady state of a refilled LcCommit (round 3 found one -- a capacity kept in elements made every Ft191 Brakedown commit
    hipFree + hipMalloc its working buffers, the 24-byte element not dividing the 256-byte rounding).  Ten commits of 2^23
    coefficients are enqueued in far less time than they take to run."""
    import time
    import torch
    n, L = 1 << 23, fid + 1
    enc = LigeroEncoding.new(fid, n) if kind == "ligero" else SdigEncoding.new(fid, n, 0)
    g = torch.Generator(device="cuda"); g.manual_seed(3)
    dev = torch.randint(0, 1 << 62, (n, L), dtype=torch.int64, device="cuda", generator=g)
    dev[:, L - 1] &= (1 << 60) - 1
    st = torch.cuda.current_stream().cuda_stream
    c = LcCommit(enc)
    for _ in range(3):
        LcCommit.commit_device(dev.data_ptr(), n, enc, st, sync=False, into=c)
    torch.cuda.synchronize()
    best = 1.0
    for _ in range(3):
        t0 = time.perf_counter()
        for _ in range(10):
            LcCommit.commit_device(dev.data_ptr(), n, enc, st, sync=False, into=c)
        t1 = time.perf_counter()
        torch.cuda.synchronize()
        t2 = time.perf_counter()
        best = min(best, (t1 - t0) / (t2 - t0))
    assert best < 0.6, "enqueueing took %.0f %% of the run time: something in the commit path synchronises" % (best * 100)


def test_refill_on_another_stream_right_after_async_commit(oracle):
    """An LcCommit refilled on stream B while the fill enqueued on (non-blocking) stream A may still be running: the library puts
    B behind A's fill by the object's event (lcpc_hip.h, "Refilling across streams").  Without that order the two fills write
    comm / coeffs / hashes concurrently.  A: a 2^24 commit (~3 ms); B: at once, a different 2^24 vector into the same object --
    then the same with B = the host-pointer entry points (small path, 64 MiB+ batched path, from_parts).  Every result is the
    oracle's for the LAST vector."""
    import torch
    O, fid, n = oracle, 3, 1 << 24
    enc, oenc = LigeroEncoding.new(fid, n), O.Encoding.ligero(fid, n)
    a, b = torch.cuda.Stream(), torch.cuda.Stream()
    x, y = O.random_elems(fid, n, 311), O.random_elems(fid, n, 312)
    dx, dy = torch.from_numpy(x.view(np.int64)).cuda(), torch.from_numpy(y.view(np.int64)).cuda()
    torch.cuda.synchronize()
    oy = O.Commit.commit(y, oenc, n_threads=8)
    c = LcCommit(enc)
    for it in range(3):
        LcCommit.commit_device(dx.data_ptr(), n, enc, a.cuda_stream, sync=False, into=c)
        LcCommit.commit_device(dy.data_ptr(), n, enc, b.cuda_stream, sync=False, into=c)
        assert c.get_root() == oy.get_root()
        assert (c.hashes() == oy.hashes()).all()
    assert (c.comm() == oy.comm()).all() and (c.coeffs() == oy.coeffs()).all()
    # host-pointer refills behind an async device fill: the batched path (>= 64 MiB of coefficients, >= 16 rows) ...
    LcCommit.commit_device(dx.data_ptr(), n, enc, a.cuda_stream, sync=False, into=c)
    LcCommit.commit(y, enc, into=c)
    assert c.get_root() == oy.get_root() and (c.hashes() == oy.hashes()).all()
    assert (c.comm() == oy.comm()).all() and (c.coeffs() == oy.coeffs()).all()
    # ... and from_parts (null stream)
    LcCommit.commit_device(dx.data_ptr(), n, enc, a.cuda_stream, sync=False, into=c)
    LcCommit.from_parts(enc, oy.comm(), oy.coeffs(), oy.n_rows, into=c)
    assert c.get_root() == oy.get_root() and (c.hashes() == oy.hashes()).all()
    a.synchronize(); b.synchronize()


def test_limb_intermediate_allocation_failure_degrades(oracle):
    """K1s keeps the rows between its two passes as 29-bit limbs in a separate buffer (n_cols <= 2^15: on by default).  When that
    buffer cannot be allocated the commit must fall back to the packed intermediate, not fail: HIP keeps a failed call's error
    until it is read, and the next launch check would otherwise return it.  LCPC_TEST_FAIL=mid (read at
    context creation by the TEST-HOOKS build of the library only: common.run_with_test_hooks) makes the allocation a request no
    device can satisfy, so the real hipMalloc failure path runs.  The product library ignores the variable."""
    from common import run_with_test_hooks
    out = run_with_test_hooks("""
fid, n_per_row, n_cols, n_rows = 3, 8192, 16384, 9
oenc = O.Encoding.ligero_from_dims(fid, n_per_row, n_cols)
coeffs = O.random_elems(fid, n_rows * n_per_row - 5, 313)
oc = O.Commit.commit(coeffs, oenc)
os.environ["LCPC_TEST_FAIL"] = "mid"
enc = LigeroEncoding.new_from_dims(fid, n_per_row, n_cols)
del os.environ["LCPC_TEST_FAIL"]
for _ in range(2):                    # the first commit meets the failure, the second runs with mid_failed set
    c = LcCommit.commit(coeffs, enc)
    assert c.get_root() == oc.get_root()
    assert (c.comm() == oc.comm()).all() and (c.hashes() == oc.hashes()).all()
ref = LcCommit.commit(coeffs, LigeroEncoding.new_from_dims(fid, n_per_row, n_cols))
assert ref.get_root() == oc.get_root()
print("degraded ok")
""")
    assert "degraded ok" in out


@pytest.mark.parametrize("fid,n_rows,n_per_row,n_cols", [
    (0, 32, 2048, 4096),        # C1: ft63 2^16, one chunk (32 + 32 * 8 bytes)
    (0, 200, 64, 128),          # ft63, 2 chunks (1632 bytes), the narrowest tree the fused kernel takes (128 leaves)
    (1, 16, 128, 256),          # ft127, one chunk
    (1, 100, 1024, 2048),       # ft127, 2 chunks
    (2, 40, 256, 512),          # ft191: one chunk of 992 bytes (24-byte elements: blocks start inside elements)
    (2, 60, 512, 1024),         # ft191: 2 chunks, an element straddles the chunk boundary
    (3, 8, 1024, 2048),         # ft255 2^13
    (3, 16, 2048, 4096),        # ft255 2^15
    (3, 31, 64, 128),           # ft255: exactly one full chunk (1024 bytes)
    (3, 32, 4096, 8192),        # ft255 2^17: 2 chunks, the second holds 32 bytes
    (3, 63, 16384, 32768),      # 2 full chunks x 32768 columns = the limit of 65536 (column, chunk) pairs
    (3, 5, 32768, 65536),       # one chunk x 65536 columns: 1024 workgroups, then the 512-leaf subtree kernel and the tail
])
def test_fused_leaf_tree_small_commits(oracle, fid, n_rows, n_per_row, n_cols):
    """Small commitments hash their columns AND fold the first six Merkle levels in one launch (leaf_tree_kernel: a quad of lanes
    per column, the one or two chunks of its leaf message in sequence, then 64 leaves -> 1 through LDS), the rest of the tree
    following from level 6.  The WHOLE `hashes` array -- leaf digests and every layer -- equals the oracle's, for every field, one
    and two chunks, the narrowest and widest trees (the unfused kernels serve every larger commitment)."""
    O = oracle
    coeffs = O.random_elems(fid, n_rows * n_per_row - 1, 900 + n_rows)
    oenc = O.Encoding.ligero_from_dims(fid, n_per_row, n_cols)
    oc = O.Commit.commit(coeffs, oenc, n_threads=4)
    enc = LigeroEncoding.new_from_dims(fid, n_per_row, n_cols)
    c = LcCommit.commit(coeffs, enc)
    assert c.get_root() == oc.get_root()
    assert (c.hashes() == oc.hashes()).all()
    c.set_timing(True)
    LcCommit.commit(coeffs, enc, into=c)
    assert c.timings().hash_launches == 1
    root = oc.get_root()
    t = O.random_elems(fid, c.n_rows, 78)
    pf = c.prove(t, enc, mk_transcript(Transcript, root, enc.get_n_col_opens()))
    opf, _ = oc.prove(t, oenc, mk_transcript(O.Transcript, root, enc.get_n_col_opens()))
    assert pf.to_bytes() == opf

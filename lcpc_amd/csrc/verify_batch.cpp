// lcpc_amd/csrc/verify_batch.cpp -- lcpcv_verify_batch (include/lcpc_hip_verify.h): LcEvalProof::verify (lcpc-2d lib.rs:832-1000;
// prove.cpp lcpc_verify) for every proof of a batch in one lockstep pipeline.
//
// Per group of g members (the header's arena formula):
//   1. host pool, one task per member: parse_proof (shared with lcpc_verify), the limb checks, the polynomials and the opened columns
//      into the pinned arena.  A member that fails keeps its status and leaves a hole: its polynomial and column slots are zero.
//   2. device, on the working set's stream: one upload (polynomials | columns); ONE row encode of the g (n_deg + 1) polynomials under
//      the encoder's lock (the encode workspace is the one lcpc_verify's encodes use), released when the encode's event has fired; the
//      leaf digests of the g n_col_opens opened columns -- each member's columns are a position-major matrix of n_col_opens columns -- by
//      the batch forms of the column-hash launchers.
//   3. host pool beside the hashes, one task per member: the whole transcript (tensors, absorbs, column draw), <inner, p_eval>.
//      Stage 1 also copies each member's root and path siblings, level-major, into the working set's second pinned buffer (not part of
//      the arena formula); they go up behind the hashes.
//   4. device: one upload (tensors | drawn columns), K7b (kernels.hip: all dot products against the encoded rows), K8b (kernels.h
//      FoldPathsArgs: every Merkle path folded from its leaf digest and compared with the root), one download (status words | leaf
//      digests), one synchronisation.
//   5. host pool over all g n_col_opens columns: K7b's and K8b's bits combined into the member's verdict under lcpc_verify's
//      precedence.  The columns K8b did not judge -- members past the header's path budget, paths of another length than the tree's
//      depth -- are folded here from the downloaded leaf digest.
// enqueue_leaf_digests / enqueue_fold_paths are shared with lcpcp_check_columns (columns.cpp).
#include "internal.h"
#include "../../include/lcpc_hip_verify.h"

using namespace lcpc;

namespace lcpc {
int VerifyBatchSet::make() {
  if (hipStreamCreateWithFlags(&st, hipStreamNonBlocking) != hipSuccess) return LCPC_ERR_HIP;
  if (hipEventCreateWithFlags(&ev_enc, hipEventDisableTiming) != hipSuccess) return LCPC_ERR_HIP;
  return 0;
}
VerifyBatchSet::~VerifyBatchSet() {
  if (st) (void)hipStreamSynchronize(st);
  dev_free(d); dev_free(t29); dev_free(d_path);
  if (ev_enc) (void)hipEventDestroy(ev_enc);
  if (st) (void)hipStreamDestroy(st);
  if (h_pin) (void)hipHostFree(h_pin);
  if (h_path) (void)hipHostFree(h_path);
}
int VerifyBatchSet::ensure_paths(ErrText* err, uint64_t bytes) {
  bytes = (bytes + 255) & ~(uint64_t)255;
  if (bytes > h_path_cap || !h_path) {
    if (h_path) (void)hipHostFree(h_path);
    h_path = nullptr; h_path_cap = 0;
    void* hp = nullptr;
    hipError_t e = hipHostMalloc(&hp, (size_t)bytes, hipHostMallocDefault);
    if (e != hipSuccess) return fail_hip(err, e, "hipHostMalloc");
    h_path = static_cast<uint8_t*>(hp); h_path_cap = bytes;
  }
  return ensure_dev(err, &d_path, &d_path_cap, bytes);
}

uint64_t staged_canon_bytes(const lcpc_ctx* c, uint64_t cols_bytes) { return !is_blake3(c) && c->NL == 8 ? cols_bytes : 0; }
uint64_t staged_cvs_bytes(const lcpc_ctx* c, uint64_t n_open, uint64_t n_rows) {
  const uint64_t n_chunks = is_blake3(c) ? leaf_chunks(c, n_rows) : 1;
  return n_chunks > 1 ? n_chunks * n_open * 32 : 0;
}

// each member's columns are a position-major matrix of n_open columns: element (row r, column k) at k * n_rows + r
int enqueue_leaf_digests(lcpc_ctx* c, const StagedColumns& sc, hipStream_t st, uint32_t* launches) {
  const int NL = c->NL;
  uint32_t n = 0;
  LeafArgs la{};
  la.comm = sc.cols; la.row_stride = 1; la.col_stride = sc.n_rows; la.n_cols = sc.n_open; la.row_base = 0; la.n_rows_total = sc.n_rows;
  la.canon_in = 0;
  if (is_blake3(c)) {
    const uint64_t n_chunks = leaf_chunks(c, sc.n_rows);
    la.chunk_begin = 0; la.n_chunks_local = la.n_chunks_total = (uint32_t)n_chunks;
    la.out = n_chunks > 1 ? sc.cvs : sc.digests;
    HIPCHK(c, launch_leaf_chunks_batch(NL, la, sc.n_batch, sc.cols_stride_w, n_chunks > 1 ? sc.cvs_stride_w : sc.dig_stride_w, st));
    n += (uint32_t)((n_chunks + 32767) / 32768);
    if (n_chunks > 1) {
      HIPCHK(c, launch_leaf_finish_batch(sc.cvs, (uint32_t)n_chunks, sc.n_open, sc.digests, sc.n_batch, sc.cvs_stride_w, sc.dig_stride_w, st));
      n++;
    }
  } else {
    la.chunk_begin = 0; la.n_chunks_local = la.n_chunks_total = 1;
    if (NL == 8) {                 // the chained batch kernels over Ft255 read canonical values only (kernels.h)
      HIPCHK(c, launch_to_canon(NL, sc.cols, (uint64_t)sc.n_batch * sc.cols_stride_w / NL, sc.canon, st));
      n++;
      la.comm = sc.canon; la.canon_in = 1;
    }
    la.out = sc.digests;
    HIPCHK(c, launch_chain_leaves_batch(chain_hash(c), NL, la, sc.n_batch, sc.cols_stride_w, sc.dig_stride_w, st));
    n++;
  }
  if (launches) *launches += n;
  return 0;
}

int enqueue_fold_paths(lcpc_ctx* c, const FoldPathsArgs& fa, hipStream_t st, uint32_t* launches) {
  if (is_blake3(c)) HIPCHK(c, launch_fold_paths_b3(fa, st));
  else HIPCHK(c, launch_chain_fold_paths(chain_hash(c), fa, st));
  if (launches) *launches += 1;
  return 0;
}
}  // namespace lcpc

namespace {

constexpr uint64_t ARENA_BUDGET = LCPCV_ARENA_BUDGET;
inline uint64_t align256(uint64_t x) { return (x + 255) & ~(uint64_t)255; }

// the pinned arena of a group of g members, mirrored on the device for the segments that cross the bus.  Bytes; every segment starts
// at a multiple of 256.  Up: [polys | cols] and [tensors | drawn]; down: [status | digests].  canon stays on the host.
struct Layout {
  uint64_t poly_b, cols_b, tens_b, drawn_b, stat_b, dig_b;      // per member
  uint64_t o_poly, o_cols, o_canon, o_tens, o_drawn, o_stat, o_dig, total;
  uint64_t per_member() const { return 2 * poly_b + tens_b + drawn_b + stat_b + dig_b + cols_b; }
  void place(uint64_t g) {
    o_poly = 0;
    o_cols = o_poly + align256(g * poly_b);
    o_canon = o_cols + align256(g * cols_b);
    o_tens = o_canon + align256(g * poly_b);
    o_drawn = o_tens + align256(g * tens_b);
    o_stat = o_drawn + align256(g * drawn_b);
    o_dig = o_stat + align256(g * stat_b);
    total = o_dig + align256(g * dig_b);
  }
};

// the encoder's lock around the row encode: released once nothing of the encode can still be in flight
struct EncodeLock {
  lcpc_ctx* c;
  hipStream_t st;
  bool drained = false;
  explicit EncodeLock(lcpc_ctx* c_, hipStream_t st_) : c(c_), st(st_) { c->mu.lock(); }
  ~EncodeLock() {
    if (!drained) (void)hipStreamSynchronize(st);
    c->mu.unlock();
  }
};

struct Args {
  lcpc_ctx* c;
  uint32_t n_batch;
  const uint8_t* roots;
  const uint64_t *outer, *inner;
  uint64_t n_outer, outer_stride, n_inner, inner_stride;
  const uint8_t* const* proofs;
  const uint64_t* proof_lens;
  lcpc_transcript* const* trs;
  uint64_t* evals;
  int32_t* status;
};

int verify_batch_run(const Args& A, lcpcv_verify_stats* stats) {
  lcpc_ctx* c = A.c;
  const FieldDesc& f = *c->f;
  const int L = f.L, NL = c->NL;
  const uint64_t F = elem_bytes(c), np = c->n_per_row, n_cols = c->n_cols, nr = A.n_outer;
  const uint64_t n_deg = lcpc_get_n_degree_tests(c), n_open = lcpc_get_n_col_opens(c), nt = n_deg + 1;
  const uint32_t hash = c->prm.hash, dw = digest_words(c);
  const uint64_t dl = digest_len(c);
  const bool dbg = c->sw_debug_timing;
  const double t_start = now_ms();
  double t_stage = 0, t_tr = 0, t_dev = 0, t_fold = 0;

  if (nr == 0) {
    // no honest proof has columns of no rows, and there is nothing for the device to multiply or hash: such a call is judged member by
    // member by the single verify (a crafted proof with empty columns gets exactly its verdict)
    for (uint32_t i = 0; i < A.n_batch; i++)
      A.status[i] = lcpc_verify(c, A.roots + (size_t)i * dl, A.outer, 0, A.inner + (size_t)i * A.inner_stride * L, A.n_inner, A.proofs[i],
                                A.proof_lens[i], A.trs[i], A.evals + (size_t)i * L);
    if (stats) *stats = lcpcv_verify_stats{};
    return 0;
  }
  Layout lay{};
  // (a member's columns: whole elements and a multiple of 16 bytes, the stride rule of the batch hash launchers -- an even count of
  // the 8- and 24-byte elements)
  lay.poly_b = nt * np * F; lay.cols_b = (L % 2 ? (n_open * nr + 1) & ~(uint64_t)1 : n_open * nr) * F; lay.tens_b = nt * nr * F;
  lay.drawn_b = n_open * 8; lay.stat_b = n_open * 4; lay.dig_b = n_open * dl;
  uint64_t gmax = ARENA_BUDGET / std::max<uint64_t>(lay.per_member(), 1);
  if (gmax < 1) gmax = 1;
  if (gmax > A.n_batch) gmax = A.n_batch;
  lcpcv_verify_stats stt{};
  stt.groups = (uint32_t)((A.n_batch + gmax - 1) / gmax);
  lay.place(gmax);

  HIPCHK(c, hipSetDevice(c->prm.device));
  SetLease<VerifyBatchSet> ws{c->verify_batch_sets};
  if (int rc = c->verify_batch_sets.take(lay.total, &ws.s)) return rc;
  hipStream_t st = ws.s->st;
  // device: the mirrored segments, then [encoded rows][canonical columns: a chained digest over Ft255][chunk CVs: BLAKE3 leaves of > 1 chunk]
  const uint64_t enc_b = align256(gmax * nt * n_cols * F), ccols_b = align256(gmax * staged_canon_bytes(c, lay.cols_b));
  const uint64_t cvs_member_b = staged_cvs_bytes(c, n_open, nr), cvs_b = align256(gmax * cvs_member_b);
  if (int rc = ensure_dev(&c->err, &ws.s->d, &ws.s->d_cap, lay.total + enc_b + ccols_b + cvs_b)) return rc;
  if (NL == 8)
    if (int rc = ensure_dev(&c->err, &ws.s->t29, &ws.s->t29_cap, gmax * nt * nr * 48)) return rc;
  // the path buffer, beside the arena: [roots of the group][siblings of the members that fold on the device, level-major].  The first
  // n_fold members of a group fold on the device (the header's path budget); a group's last members and every column whose path has
  // another number of entries than the tree's depth fold on the host
  const uint32_t path_len = c->path_len;
  const uint64_t path_b = n_open * path_len * dl;                // P
  const uint64_t n_fold_max = path_b ? std::min<uint64_t>(gmax, std::max<uint64_t>(1, LCPCV_PATH_BUDGET / path_b)) : gmax;
  const uint64_t o_sibs = align256(gmax * dl);
  if (int rc = ws.s->ensure_paths(&c->err, o_sibs + n_fold_max * path_b)) return rc;
  uint8_t* const hp = ws.s->h_path;
  uint8_t* const dp = ws.s->d_path;
  std::unique_ptr<uint8_t[]> host_fold(new uint8_t[(size_t)gmax * n_open]);      // 1: this column's path is folded on the host
  std::vector<uint64_t> n_host_fold(gmax);
  uint64_t cols_dev = 0, cols_host = 0;
  uint8_t* const hb = ws.s->h_pin;
  uint8_t* const db = ws.s->d;
  auto d32 = [&](uint64_t off) { return reinterpret_cast<uint32_t*>(db + off); };
  uint32_t* const d_enc = d32(lay.total);
  uint32_t* const d_ccols = d32(lay.total + enc_b);
  uint32_t* const d_cvs = d32(lay.total + enc_b + ccols_b);

  std::vector<ProofView> views(gmax);
  std::vector<uint64_t> eval_acc(gmax * MAXL);

  for (uint32_t g0 = 0; g0 < A.n_batch; g0 += (uint32_t)gmax) {
    const uint32_t g = (uint32_t)std::min<uint64_t>(gmax, A.n_batch - g0);
    int32_t* const status = A.status + g0;
    const uint64_t n_fold = std::min<uint64_t>(g, n_fold_max);
    // ---- 1. parse, check, stage ---------------------------------------------------------------------------------------------------
    double t0 = now_ms();
    parallel_for(g, 1, [&](uint64_t mb, uint64_t me) {
      for (uint64_t i = mb; i < me; i++) {
        ProofView& pv = views[i];
        pv = ProofView{};
        uint64_t* polys = reinterpret_cast<uint64_t*>(hb + lay.o_poly + i * lay.poly_b);
        uint64_t* cols = reinterpret_cast<uint64_t*>(hb + lay.o_cols + i * lay.cols_b);
        int rc = parse_proof(c, A.proofs[g0 + i], A.proof_lens[g0 + i], A.n_outer, A.n_inner, &pv);
        // untrusted limbs: nothing >= p reaches the device arithmetic.  lcpc_verify's order: p_eval, every p_random, then the columns
        auto reduced = [&](const uint64_t* v, uint64_t n) {
          for (uint64_t k = 0; k < n; k++) if (h_ge_p(f, v + k * L)) return false;
          return true;
        };
        if (!rc && !reduced(pv.p_eval.data(), np)) rc = LCPC_VERR_MALFORMED;
        for (size_t d = 0; !rc && d < pv.p_random.size(); d++)
          if (!reduced(pv.p_random[d].data(), pv.p_random[d].size() / L)) rc = LCPC_VERR_MALFORMED;
        if (!rc) {
          for (uint64_t d = 0; d < n_deg; d++) memcpy(polys + d * np * L, pv.p_random[d].data(), np * F);
          memcpy(polys + n_deg * np * L, pv.p_eval.data(), np * F);
          for (uint64_t k = 0; k < n_open && !rc; k++) {         // (the copy is the limb check of the columns)
            const uint64_t* src = pv.cols[k].data();
            uint64_t* dst = cols + k * nr * L;
            for (uint64_t r = 0; r < nr; r++) {
              if (h_ge_p(f, src + r * L)) { rc = LCPC_VERR_MALFORMED; break; }
              memcpy(dst + r * L, src + r * L, F);
            }
          }
        }
        if (rc) { memset(polys, 0, lay.poly_b); memset(cols, 0, lay.cols_b); }     // the hole: zeros, never read as data
        else if (lay.cols_b > n_open * nr * F) memset(reinterpret_cast<uint8_t*>(cols) + n_open * nr * F, 0, lay.cols_b - n_open * nr * F);
        // the root and the path siblings, level-major: entry lvl of column k at (lvl * n_open + k) * D of the member's slot
        memcpy(hp + i * dl, A.roots + (size_t)(g0 + i) * dl, dl);
        uint8_t* const hf = host_fold.get() + i * n_open;
        n_host_fold[i] = 0;
        if (i >= n_fold) {
          memset(hf, 1, n_open);
          n_host_fold[i] = n_open;
        } else if (rc) {
          memset(hp + o_sibs + i * path_b, 0, path_b);
          memset(hf, 0, n_open);
        } else {
          uint8_t* const sibs = hp + o_sibs + i * path_b;
          for (uint64_t k = 0; k < n_open; k++) {
            hf[k] = pv.paths[k].n != path_len;
            n_host_fold[i] += hf[k];
          }
          // level by level, so that the writes run through the slot in order (the reads step from column to column of the proof)
          for (uint64_t lvl = 0; lvl < path_len; lvl++) {
            uint8_t* dst = sibs + lvl * n_open * dl;
            const uint64_t off = (8 + dl) * lvl + 8;
            for (uint64_t k = 0; k < n_open; k++, dst += dl) {
              if (hf[k]) memset(dst, 0, dl);
              else if (dl == 32) memcpy(dst, pv.paths[k].p + off, 32);
              else memcpy(dst, pv.paths[k].p + off, 64);
            }
          }
        }
        status[i] = rc;
      }
    });
    t_stage += now_ms() - t0;
    // ---- 2. upload, row encode, leaf digests --------------------------------------------------------------------------------------
    t0 = now_ms();
    HIPCHK(c, hipMemcpyAsync(db + lay.o_poly, hb + lay.o_poly, lay.o_cols + (size_t)g * lay.cols_b, hipMemcpyHostToDevice, st));
    StagedColumns sc{};
    sc.cols = d32(lay.o_cols); sc.cols_stride_w = lay.cols_b / 4; sc.canon = d_ccols; sc.cvs = d_cvs; sc.cvs_stride_w = cvs_member_b / 4;
    sc.digests = d32(lay.o_dig); sc.dig_stride_w = n_open * dw; sc.n_open = n_open; sc.n_rows = nr; sc.n_batch = g;
    {
      EncodeLock lk(c, st);
      EncodeJob j;
      j.src = d32(lay.o_poly); j.src_stride = np; j.n_valid = np; j.dst = d_enc; j.n_rows = (uint64_t)g * nt;
      if (int rc = encode_rows_device(c, &c->ws, j, st, &c->err, &stt.encode_launches)) return rc;
      HIPCHK(c, hipEventRecord(ws.s->ev_enc, st));
      // the hashes do not touch the encode workspace; they are enqueued before the wait so that they run behind the encode at once
      if (int rc = enqueue_leaf_digests(c, sc, st, &stt.hash_launches)) return rc;
      HIPCHK(c, hipEventSynchronize(ws.s->ev_enc));
      stt.host_syncs++;
      lk.drained = true;
    }
    // roots and paths go up behind the polynomials on the same stream, beside the transcripts: nothing waits for them before the fold
    HIPCHK(c, hipMemcpyAsync(dp, hp, o_sibs + (size_t)n_fold * path_b, hipMemcpyHostToDevice, st));
    t_dev += now_ms() - t0;
    // ---- 3. transcripts, beside the hashes ------------------------------------------------------------------------------------------
    t0 = now_ms();
    parallel_for(g, 1, [&](uint64_t mb, uint64_t me) {
      for (uint64_t i = mb; i < me; i++) {
        uint64_t* tens = reinterpret_cast<uint64_t*>(hb + lay.o_tens + i * lay.tens_b);
        uint64_t* drawn = reinterpret_cast<uint64_t*>(hb + lay.o_drawn + i * lay.drawn_b);
        if (status[i]) { memset(tens, 0, lay.tens_b); memset(drawn, 0, lay.drawn_b); continue; }
        Transcript& tr = A.trs[g0 + i]->t;
        const uint64_t* polys = reinterpret_cast<const uint64_t*>(hb + lay.o_poly + i * lay.poly_b);
        uint64_t* canon = reinterpret_cast<uint64_t*>(hb + lay.o_canon + i * lay.poly_b);
        for (uint64_t k = 0; k < nt * np; k++) h_canon(f, canon + k * L, polys + k * L);
        for (uint64_t d = 0; d < n_deg; d++) {                                      // lib.rs:868-920
          uint8_t key[32];
          tr.challenge_bytes(LBL_DT, 6, key, 32);
          ChaCha20Rng rng(key);
          for (uint64_t r = 0; r < nr; r++) rng.field_random(f, &tens[(d * nr + r) * L]);
          tr.append_messages(LBL_PR, 6, reinterpret_cast<const uint8_t*>(canon + d * np * L), 8 * L, np);
        }
        memcpy(tens + n_deg * nr * L, A.outer + (size_t)(g0 + i) * A.outer_stride * L, nr * F);
        tr.append_messages(LBL_PE, 6, reinterpret_cast<const uint8_t*>(canon + n_deg * np * L), 8 * L, np);
        draw_columns(tr, c, drawn, n_open);
        // <inner_tensor, p_eval> (lib.rs:947-951)
        const uint64_t* inner = A.inner + (size_t)(g0 + i) * A.inner_stride * L;
        const uint64_t* pe = polys + n_deg * np * L;
        uint64_t acc[MAXL] = {0, 0, 0, 0}, t[MAXL];
        for (uint64_t k = 0; k < np; k++) { h_mul(f, t, inner + k * L, pe + k * L); h_add(f, acc, acc, t); }
        memcpy(&eval_acc[i * MAXL], acc, F);
      }
    });
    t_tr += now_ms() - t0;
    // ---- 4. tensors and drawn columns up, the column check, status and digests down -------------------------------------------------
    t0 = now_ms();
    HIPCHK(c, hipMemcpyAsync(db + lay.o_tens, hb + lay.o_tens, lay.o_drawn - lay.o_tens + (size_t)g * lay.drawn_b, hipMemcpyHostToDevice, st));
    VerifyColsArgs va{};
    va.cols = d32(lay.o_cols); va.cols_stride = lay.cols_b / F; va.tensors = d32(lay.o_tens); va.enc = d_enc;
    va.drawn = reinterpret_cast<const uint64_t*>(db + lay.o_drawn); va.status = d32(lay.o_stat);
    va.n_rows = nr; va.n_cols = n_cols; va.n_open = (uint32_t)n_open; va.n_t = (uint32_t)nt; va.n_batch = g;
    if (NL == 8) {
      HIPCHK(c, launch_to_r29(va.tensors, (uint64_t)g * nt * nr, ws.s->t29, st));
      va.tensors29 = ws.s->t29;
      stt.check_launches++;
    }
    HIPCHK(c, launch_verify_columns_batch(NL, va, st));
    stt.check_launches += (uint32_t)((n_open + (1u << 20) - 1) >> 20);
    // K8b behind K7b, which has written every status word: the path bit of the first n_fold members' columns
    FoldPathsArgs fa{};
    fa.leaves = d32(lay.o_dig); fa.leaves_stride = n_open * dw; fa.drawn = va.drawn;
    fa.sibs = reinterpret_cast<const uint32_t*>(dp + o_sibs); fa.sib_member = path_b / 4; fa.sib_col = dw; fa.sib_lvl = n_open * dw;
    fa.roots = reinterpret_cast<const uint32_t*>(dp); fa.status = va.status; fa.status_stride = n_open;
    fa.n_open = (uint32_t)n_open; fa.depth = path_len; fa.n_batch = (uint32_t)n_fold;
    if (int rc = enqueue_fold_paths(c, fa, st, &stt.hash_launches)) return rc;
    HIPCHK(c, hipMemcpyAsync(hb + lay.o_stat, db + lay.o_stat, lay.o_dig - lay.o_stat + (size_t)g * lay.dig_b, hipMemcpyDeviceToHost, st));
    HIPCHK(c, hipStreamSynchronize(st));
    stt.host_syncs++;
    t_dev += now_ms() - t0;
    // ---- 5. Merkle paths and verdicts ------------------------------------------------------------------------------------------------
    // the error reported is that of the first failing column, with the reference's precedence degree > eval > path
    t0 = now_ms();
    const uint32_t* h_stat = reinterpret_cast<const uint32_t*>(hb + lay.o_stat);
    const uint8_t* h_dig = hb + lay.o_dig;
    const uint64_t* h_drawn = reinterpret_cast<const uint64_t*>(hb + lay.o_drawn);
    std::unique_ptr<uint8_t[]> col_code(new uint8_t[(size_t)g * n_open]);
    parallel_for((uint64_t)g * n_open, 32, [&](uint64_t b, uint64_t e) {
      for (uint64_t id = b; id < e; id++) {
        const uint64_t i = id / n_open, k = id % n_open;
        if (status[i]) { col_code[id] = 0; continue; }
        const uint32_t bits = h_stat[i * n_open + k];
        bool pth = !(bits & FOLD_PATH_BIT);                                        // K8b's verdict
        if (host_fold[id]) {                                                       // verify_column_path lib.rs:955-982
          const ProofView::Path& path = views[i].paths[k];
          uint8_t h[64], blk[128];
          memcpy(h, h_dig + i * lay.dig_b + k * dl, dl);
          uint64_t cc = h_drawn[i * n_open + k];
          for (uint64_t lvl = 0; lvl < path.n; lvl++) {
            const uint8_t* pk = path.p + (8 + dl) * lvl + 8;
            if (cc % 2 == 0) { memcpy(blk, h, dl); memcpy(blk + dl, pk, dl); } else { memcpy(blk, pk, dl); memcpy(blk + dl, h, dl); }
            digest_host(hash, blk, 2 * dl, h);
            cc >>= 1;
          }
          pth = memcmp(h, A.roots + (size_t)(g0 + i) * dl, dl) == 0;
        }
        const int code = (bits & 1u) ? LCPC_VERR_COLUMN_DEGREE : ((bits & 2u) ? LCPC_VERR_COLUMN_EVAL : (!pth ? LCPC_VERR_COLUMN_PATH : 0));
        col_code[id] = (uint8_t)(-code);
      }
    });
    for (uint32_t i = 0; i < g; i++) {
      if (status[i]) continue;
      cols_host += n_host_fold[i];
      cols_dev += n_open - n_host_fold[i];
      for (uint64_t k = 0; k < n_open; k++)
        if (col_code[(size_t)i * n_open + k]) { status[i] = -(int)col_code[(size_t)i * n_open + k]; break; }
      if (!status[i]) memcpy(A.evals + (size_t)(g0 + i) * L, &eval_acc[i * MAXL], F);
    }
    t_fold += now_ms() - t0;
  }
  if (stats) *stats = stt;
  if (dbg)
    fprintf(stderr, "[lcpcv_verify_batch] %u members in %u groups: parse + stage %.2f ms, transcripts %.2f, device (uploads, encode wait, check, "
                    "download) %.2f, path folds %.2f, total %.2f; %u encode + %u hash + %u check launches, %u syncs; %llu columns folded on the "
                    "device, %llu on the host\n",
            A.n_batch, stt.groups, t_stage, t_tr, t_dev, t_fold, now_ms() - t_start, stt.encode_launches, stt.hash_launches, stt.check_launches,
            stt.host_syncs, (unsigned long long)cols_dev, (unsigned long long)cols_host);
  return 0;
}

}  // namespace

extern "C" {

int lcpcv_version(void) { return LCPCV_VERSION; }

int lcpcv_verify_batch(lcpc_ctx* c, uint32_t n_batch, const uint8_t* roots, const uint64_t* outer_tensors, uint64_t n_outer, uint64_t outer_stride,
                       const uint64_t* inner_tensors, uint64_t n_inner, uint64_t inner_stride, const uint8_t* const* proofs,
                       const uint64_t* proof_lens, lcpc_transcript* const* trs, uint64_t* evals, int32_t* status, lcpcv_verify_stats* stats) {
  if (!c || !roots || !outer_tensors || !inner_tensors || !proofs || !proof_lens || !trs || !evals || !status) return LCPC_ERR_ARG;
  if (n_batch == 0 || n_batch > 65535) return LCPC_ERR_ARG;
  if ((outer_stride != 0 && outer_stride < n_outer) || (inner_stride != 0 && inner_stride < n_inner)) return LCPC_ERR_ARG;
  for (uint32_t i = 0; i < n_batch; i++)
    if (!proofs[i] || !trs[i]) return LCPC_ERR_ARG;
  int rc;
  try {
    {
      std::vector<lcpc_transcript*> t(trs, trs + n_batch);
      std::sort(t.begin(), t.end(), std::less<lcpc_transcript*>());
      if (std::adjacent_find(t.begin(), t.end()) != t.end()) return LCPC_ERR_ARG;                 // a transcript listed twice
    }
    const Args a{c, n_batch, roots, outer_tensors, inner_tensors, n_outer, outer_stride, n_inner, inner_stride, proofs, proof_lens, trs, evals, status};
    rc = c->prm.shard_count > 1 ? LCPC_ERR_STATE : verify_batch_run(a, stats);
  } catch (const std::bad_alloc&) {
    c->err = "host allocation failed";
    rc = LCPC_ERR_NOMEM;
  } catch (const std::exception& ex) {
    c->err = ex.what();
    rc = LCPC_ERR_STATE;
  } catch (...) {
    rc = LCPC_ERR_STATE;
  }
  if (rc)                          // a sharded encoder, a device or allocation failure: no member was judged
    for (uint32_t i = 0; i < n_batch; i++) status[i] = rc;
  return rc;
}

}  // extern "C"

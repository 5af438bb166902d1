// lcpc_amd/csrc/batch.cpp -- lcpcx_commit_batch_device (include/lcpc_hip_batch.h): n_batch equal-shape polynomials committed under
// one encoder in one pipeline.
//
// Ligero, under every digest: the members' comm / coeffs / hashes live member-major in one slab (internal.h BatchSlab), the row NTT runs
// once over n_batch * n_rows rows (encode_rows_device: rows are independent), and the column hash and the tree run as batched kernels
// -- as many launches as ONE commit of the shape.  BLAKE3: kernels.hip (K3b / K4b: chunk CVs, fold, or leaf digests with the
// first six tree levels).  SHA3-256 / Keccak-256 / SHA-256 / BLAKE2b: one serial chain per column, so one leaf launch and one tree
// call over the batch (the batch forms of chain_dev.h); hashes slots are digest_words(c) words.
//
// Brakedown: the expander matrices are the same for every row of every member, so the encode is one pass over the n_batch * n_rows
// stacked rows, in one commit's launches.  Members of < SDIG_T_MIN_ROWS rows keep a row-major comm, as a single commit of theirs
// does: the same pipeline as Ligero (from 24 STACKED rows on, encode_rows_device runs the position-major kernels on a working T
// and transposes back).  Members of >= SDIG_T_MIN_ROWS rows keep their own position-major T_i[pos][row] (comm_t), member-major in
// the slab's `t` segment, written by the batch forms of the K2 kernels (kernels.hip K2b: lane = batch row).  BLAKE3: the batched
// hash and tree kernels read either layout through LeafArgs' strides.  Under the four chained digests the hash and tree of a
// Brakedown batch run member by member through the one-shot launchers (merkleize_device):
// tests/test_gpu_commit_batch_digests.py::test_brakedown_under_a_chained_digest pins that launch count.  A batch with more stacked
// rows than the batch launchers' grids carry runs the single-commit pipeline (commit.cpp commit_device_locked) member by member.
//
// lcpcx_prove_batch, the other half of the header, is at the end of this file: every member of a batch opened in lockstep.
#include "internal.h"
#include "../../include/lcpc_hip_batch.h"
#include <functional>

using namespace lcpc;

namespace {

constexpr uint64_t align256(uint64_t b) { return (b + 255) & ~(uint64_t)255; }

struct BatchShape {
  uint64_t n_rows, n_chunks, stride;   // stride: elements between polynomials
  bool contiguous;                     // whole rows, back to back: the encode reads the caller's buffer in place
  bool borrow;
  bool tree;                           // BLAKE3: leaf_tree_supported
  bool chained;                        // SHA3-256 / Keccak-256 / SHA-256 / BLAKE2b: no chunk CVs, no leaf_tree form
  bool pos_major;                      // Brakedown, n_rows >= SDIG_T_MIN_ROWS: the members hold T_i (slab segment `t`), not a row-major comm
  bool member_hash;                    // Brakedown under a chained digest: hash and tree member by member, by the one-shot launchers
  bool need_coeffs() const { return !(borrow && contiguous); }   // (a strided borrow still stages the rows for the encode)
  bool need_cvs() const { return !chained && !tree && n_chunks > 1; }
};

LeafArgs batch_leaf_args(const lcpc_ctx* c, const BatchShape& s, const uint32_t* comm) {
  LeafArgs la{};
  la.comm = comm; la.canon_in = c->comm_canon ? 1u : 0u; la.row_stride = c->n_cols; la.col_stride = 1; la.n_cols = c->n_cols;
  if (s.pos_major) { la.canon_in = 1u; la.row_stride = 1; la.col_stride = s.n_rows; }   // (commit.cpp leaf_args, comm_t)
  la.row_base = 0; la.n_rows_total = s.n_rows;
  la.chunk_begin = 0; la.n_chunks_local = la.n_chunks_total = (uint32_t)s.n_chunks;
  return la;
}

int make_slab(const lcpc_ctx* c, ErrText* err, const BatchShape& s, uint32_t n_batch, std::shared_ptr<BatchSlab>* out) {
  std::shared_ptr<BatchSlab> sl(new BatchSlab());
  const uint64_t eb = elem_bytes(c);
  sl->n_batch = n_batch; sl->n_rows = s.n_rows;
  sl->comm_stride = s.pos_major ? 0 : s.n_rows * c->n_cols * c->NL;
  // a member's T rounded up to 256 bytes: a multiple of 16 for every field (Ft63 with odd n_rows too), as the hash launchers ask
  sl->t_stride = s.pos_major ? align256(s.n_rows * c->n_cols * eb) / 4 : 0;
  sl->tmp_stride = s.pos_major ? align256(s.n_rows * c->d_pre.back().n_out * eb) / 4 : 0;
  sl->coeffs_stride = s.need_coeffs() ? s.n_rows * c->n_per_row * c->NL : 0;
  sl->hashes_stride = (2 * c->np2 - 1) * digest_words(c);
  sl->cvs_stride = s.need_cvs() ? s.n_chunks * c->n_cols * 8 : 0;
  uint64_t off = 0;
  sl->off_comm = off; off = align256(off + (uint64_t)n_batch * sl->comm_stride * 4);
  sl->off_t = off; off = align256(off + (uint64_t)n_batch * sl->t_stride * 4);
  sl->off_coeffs = off; off = align256(off + (uint64_t)n_batch * sl->coeffs_stride * 4);
  sl->off_hashes = off; off = align256(off + (uint64_t)n_batch * sl->hashes_stride * 4);
  sl->off_cvs = off; off = align256(off + (uint64_t)n_batch * sl->cvs_stride * 4);
  if (int rc = dev_alloc(err, &sl->d, (size_t)off)) return rc;
  void* hp = nullptr;              // without the mapping the roots are copied out (fetch_roots)
  if (hipHostMalloc(&hp, (size_t)n_batch * digest_len(c), hipHostMallocMapped) == hipSuccess) {
    void* dp = nullptr;
    if (hipHostGetDevicePointer(&dp, hp, 0) == hipSuccess) { sl->h_roots = static_cast<uint32_t*>(hp); sl->d_roots_alias = static_cast<uint32_t*>(dp); }
    else (void)hipHostFree(hp);
  }
  if (!sl->h_roots) (void)hipGetLastError();
  *out = std::move(sl);
  return 0;
}

// the slab these members were last filled into together, if this batch fits it as it is
std::shared_ptr<BatchSlab> reusable_slab(lcpc_commit_t* const* cms, uint32_t n_batch, const BatchShape& s) {
  const std::shared_ptr<BatchSlab>& sl = cms[0]->slab;
  if (!sl || sl->n_batch != n_batch || sl->n_rows != s.n_rows) return nullptr;
  if ((sl->t_stride != 0) != s.pos_major || (sl->comm_stride != 0) == s.pos_major) return nullptr;     // the other regime's segments
  if ((s.need_coeffs() && !sl->coeffs_stride) || (s.need_cvs() && !sl->cvs_stride)) return nullptr;
  for (uint32_t i = 0; i < n_batch; i++)
    if (cms[i]->slab != sl || cms[i]->slab_index != i) return nullptr;
  return sl;
}

// every member's root on the host behind ONE synchronisation of st
int fetch_roots(lcpc_commit_t* const* cms, uint32_t n_batch, const BatchSlab* sl, hipStream_t st, uint8_t* roots) {
  lcpc_commit_t* m0 = cms[0];
  const lcpc_ctx* c = m0->enc;
  const uint32_t dl = digest_len(c);
  if (sl && sl->d_roots_alias && c->np2 > 1) {
    HIPCHK(m0, hipStreamSynchronize(st));
    memcpy(roots, sl->h_roots, (size_t)n_batch * dl);
    return 0;
  }
  for (uint32_t i = 0; i < n_batch; i++)
    HIPCHK(m0, hipMemcpyAsync(roots + (size_t)i * dl, cms[i]->d_hashes + (2 * c->np2 - 2) * digest_words(c), dl, hipMemcpyDeviceToHost, st));
  HIPCHK(m0, hipStreamSynchronize(st));
  return 0;
}

// the position-major encode of the whole batch into the members' T_i: sdig_walk once over the batch launchers (ctx.cpp
// encode_rows_device's fast path with row -> batch row).  src: the members' rows stacked
int encode_batch_t(const lcpc_ctx* c, ErrText* err, BatchSlab* sl, const uint32_t* src, uint32_t* copy_dst, hipStream_t st, uint32_t* launches) {
  const DevCsr& pl = c->d_pre.back();
  const uint32_t n_batch = sl->n_batch;
  if (int rc = ensure_dev(err, &sl->ws.d_tmp, &sl->ws.tmp_cap, (uint64_t)n_batch * sl->tmp_stride * 4)) return rc;
  uint32_t* t0 = sl->seg(sl->off_t, sl->t_stride, 0);
  hipError_t e = launch_transpose_to_t_batch(c->NL, src, c->n_per_row, c->n_per_row, sl->n_rows, t0, n_batch, sl->t_stride, st, ~(uint64_t)0,
                                             copy_dst, true);
  if (e != hipSuccess) return fail_hip(err, e, "launch_transpose_to_t_batch");
  ++*launches;
  SpmmTArgs a{};
  a.t = t0; a.n_rows = sl->n_rows;
  auto mat = [&](const DevCsr& m, uint64_t in_off, uint64_t out_off, bool to_tmp) -> int {
    a.out_alt = to_tmp ? sl->ws.d_tmp : nullptr; a.in_off = in_off; a.out_off = out_off;
    a.rowptr = m.rowptr; a.colidx = m.colidx; a.vals = m.vals; a.vals29 = m.vals29; a.m = m.n_out;
    hipError_t he = launch_spmm_t_batch(c->NL, a, n_batch, sl->t_stride, sl->tmp_stride, st);
    if (he != hipSuccess) return fail_hip(err, he, "launch_spmm_t_batch");
    ++*launches;
    return 0;
  };
  auto rs = [&](uint64_t out_off, uint64_t n_out) -> int {
    hipError_t he = launch_sdig_rs_t_batch(c->NL, sl->ws.d_tmp, (uint32_t)pl.n_out, t0, out_off, (uint32_t)n_out, sl->n_rows, c->d_r2, n_batch,
                                           sl->tmp_stride, sl->t_stride, st);
    if (he != hipSuccess) return fail_hip(err, he, "launch_sdig_rs_t_batch");
    ++*launches;
    return 0;
  };
  return sdig_walk(c, mat, rs);
}

// Ligero and Brakedown, every digest (every member's fill_mu and mu held, the device current)
int commit_batch_fast(lcpc_commit_t* const* cms, uint32_t n_batch, const uint64_t* coeffs_dev, uint64_t n_coeffs, uint64_t poly_stride,
                      hipStream_t st, uint32_t flags, uint8_t* roots) {
  lcpc_commit_t* m0 = cms[0];
  const lcpc_ctx* c = m0->enc;
  BatchShape s{};
  s.n_rows = (n_coeffs + c->n_per_row - 1) / c->n_per_row;
  s.n_chunks = leaf_chunks(c, s.n_rows);
  s.stride = poly_stride ? poly_stride : n_coeffs;
  const bool whole = s.n_rows * c->n_per_row == n_coeffs;
  s.contiguous = whole && s.stride == n_coeffs;
  s.borrow = (flags & LCPC_COMMIT_BORROW_COEFFS) && whole;
  s.chained = !is_blake3(c);
  const bool sdig = c->prm.encoding == LCPC_ENC_SDIG;
  s.pos_major = sdig && s.n_rows >= SDIG_T_MIN_ROWS;
  s.member_hash = sdig && s.chained;
  s.tree = !s.chained && leaf_tree_supported(batch_leaf_args(c, s, nullptr), c->np2);
  int rc;
  // st behind every member's last fill; the members are un-committed from here until the batch is sealed
  for (uint32_t i = 0; i < n_batch; i++)
    if ((rc = begin_commit(cms[i], st, s.n_rows, 0, s.n_rows, 0, s.n_chunks))) { m0->err = cms[i]->err.c_str(); return rc; }
  std::shared_ptr<BatchSlab> sl = reusable_slab(cms, n_batch, s);
  if (!sl) {
    if ((rc = make_slab(c, &m0->err, s, n_batch, &sl))) return rc;
    for (uint32_t i = 0; i < n_batch; i++) {
      lcpc_commit_t* m = cms[i];
      leave_slab(m);               // (the views of another slab are dropped; what is left is the member's own)
      dev_free(m->d_comm); dev_free(m->d_coeffs); dev_free(m->d_hashes);
      m->d_comm = m->d_coeffs = m->d_hashes = nullptr;
      m->cap_comm_rows = m->cap_coeff_rows = 0;
      if (s.pos_major) { dev_free(m->ws.d_t); m->ws.d_t = nullptr; m->ws.t_cap = 0; }       // ws.d_t becomes a view
      m->slab = sl; m->slab_index = i;
    }
  }
  for (uint32_t i = 0; i < n_batch; i++) {       // the views (a reused slab may have grown a use for its coeffs segment)
    lcpc_commit_t* m = cms[i];
    if (sl->comm_stride) m->d_comm = sl->seg(sl->off_comm, sl->comm_stride, i);           // (else null, or the member's own row-major copy)
    else { m->ws.d_t = sl->seg(sl->off_t, sl->t_stride, i); m->ws.t_cap = sl->t_stride * 4; m->comm_t = true; }
    m->d_coeffs = sl->coeffs_stride ? sl->seg(sl->off_coeffs, sl->coeffs_stride, i) : nullptr;
    m->d_hashes = sl->seg(sl->off_hashes, sl->hashes_stride, i);
  }
  const bool timing = m0->timing;
  uint32_t launches[3] = {0, 0, 0};
  if (timing) HIPCHK(m0, hipEventRecord(m0->ev[0], st));

  // ---- encode: one matrix of n_batch * n_rows rows
  uint32_t* comm0 = s.pos_major ? sl->seg(sl->off_t, sl->t_stride, 0) : sl->seg(sl->off_comm, sl->comm_stride, 0);
  const uint64_t comm_stride = s.pos_major ? sl->t_stride : sl->comm_stride;
  uint32_t* coeffs0 = sl->coeffs_stride ? sl->seg(sl->off_coeffs, sl->coeffs_stride, 0) : nullptr;
  EncodeJob j;
  j.src_stride = c->n_per_row; j.n_valid = c->n_per_row; j.dst = comm0; j.n_rows = (uint64_t)n_batch * s.n_rows;
  j.canon_out = c->comm_canon;
  // Brakedown below SDIG_T_MIN_ROWS stacked rows: the row-major kernels write no coeffs copy on the way, so the rows are placed first
  const bool place_first = sdig && j.n_rows < SDIG_T_MIN_ROWS && !s.borrow;
  if (s.contiguous && !place_first) {
    // read in place; the first pass writes the members' coeffs copies as it streams the source (unless they are borrowed)
    j.src = reinterpret_cast<const uint32_t*>(coeffs_dev);
    j.copy_dst = s.borrow ? nullptr : coeffs0;
  } else {
    // ragged rows or a stride: the polynomials into the slab's padded coeffs rows first (one launch: copy + zero tails)
    HIPCHK(m0, launch_batch_place(coeffs_dev, s.stride * c->L, n_coeffs * c->L, reinterpret_cast<uint64_t*>(coeffs0),
                                  s.n_rows * c->n_per_row * c->L, n_batch, st));
    launches[0]++;
    j.src = coeffs0;
  }
  if (s.pos_major) rc = encode_batch_t(c, &m0->err, sl.get(), j.src, j.copy_dst, st, &launches[0]);
  else rc = encode_rows_device(c, &sl->ws, j, st, &m0->err, &launches[0]);
  if (rc) return rc;
  if (timing) HIPCHK(m0, hipEventRecord(m0->ev[1], st));

  // ---- column hash + tree: the launches of one commit, each over the whole batch (commit.cpp merkleize_device)
  LeafArgs la = batch_leaf_args(c, s, comm0);
  uint32_t* hashes0 = sl->seg(sl->off_hashes, sl->hashes_stride, 0);
  const uint32_t dw = digest_words(c);
  uint32_t levels_done = 0;
  hipEvent_t ev_end = m0->ev[3];
  float hash_ms = 0.f, merkle_ms = 0.f;
  if (s.member_hash) {
    // the one-shot hash and tree on each member's views; phase times are sums over the members (between the members' own events)
    for (uint32_t i = 0; i < n_batch; i++) {
      lcpc_commit_t* m = cms[i];
      const bool own_timing = m->timing;
      m->timing = timing;            // (merkleize_device records m->ev[2] between its hash and its tree)
      rc = merkleize_device(m, st);
      m->timing = own_timing;
      if (rc) { if (m != m0) m0->err = m->err.c_str(); return rc; }
      if (timing) HIPCHK(m0, hipEventRecord(m->ev[3], st));
      launches[1] += m->launches[1]; launches[2] += m->launches[2];
    }
    if (timing) {
      ev_end = cms[n_batch - 1]->ev[3];
      HIPCHK(m0, hipEventSynchronize(ev_end));
      for (uint32_t i = 0; i < n_batch; i++) {
        float h = 0.f, t = 0.f;
        (void)hipEventElapsedTime(&h, i ? cms[i - 1]->ev[3] : m0->ev[1], cms[i]->ev[2]);
        (void)hipEventElapsedTime(&t, cms[i]->ev[2], cms[i]->ev[3]);
        hash_ms += h; merkle_ms += t;
      }
    }
  } else if (s.chained) {
    // one serial chain per column over the whole leaf message: the digests themselves, in one launch
    la.out = hashes0;
    HIPCHK(m0, launch_chain_leaves_batch(chain_hash(c), c->NL, la, n_batch, comm_stride, sl->hashes_stride, st));
    launches[1]++;
  } else if (s.tree) {
    HIPCHK(m0, launch_leaf_tree_batch(c->NL, la, hashes0, c->np2, n_batch, comm_stride, sl->hashes_stride, st));
    launches[1]++;
    levels_done = 6;
  } else {
    uint32_t* cvs0 = s.need_cvs() ? sl->seg(sl->off_cvs, sl->cvs_stride, 0) : nullptr;
    la.out = cvs0 ? cvs0 : hashes0;              // (one chunk: the digests themselves)
    HIPCHK(m0, launch_leaf_chunks_batch(c->NL, la, n_batch, comm_stride, cvs0 ? sl->cvs_stride : sl->hashes_stride, st));
    launches[1]++;
    if (cvs0) {
      HIPCHK(m0, launch_leaf_finish_batch(cvs0, (uint32_t)s.n_chunks, c->n_cols, hashes0, n_batch, sl->cvs_stride, sl->hashes_stride, st));
      launches[1]++;
    }
  }
  if (timing && !s.member_hash) HIPCHK(m0, hipEventRecord(m0->ev[2], st));
  if (c->np2 > c->n_cols && !s.member_hash)          // hashes[n_cols..np2) of every member stay zero (lib.rs:656-666)
    HIPCHK(m0, hipMemset2DAsync(hashes0 + c->n_cols * dw, (size_t)sl->hashes_stride * 4, 0, (size_t)(c->np2 - c->n_cols) * digest_len(c), n_batch, st));
  if (c->np2 > 1 && !s.member_hash) {
    if (!is_blake3(c)) HIPCHK(m0, launch_chain_merkle_tree_batch(chain_hash(c), hashes0, c->np2, n_batch, sl->hashes_stride, st, sl->d_roots_alias));
    else HIPCHK(m0, launch_merkle_tree_from_batch(hashes0, c->np2, levels_done, n_batch, sl->hashes_stride, st, sl->d_roots_alias));
    launches[2]++;
  }

  // ---- seal (commit.cpp seal_commit, for every member)
  if (timing) {
    if (!s.member_hash) HIPCHK(m0, hipEventRecord(ev_end, st));
    HIPCHK(m0, hipEventSynchronize(ev_end));
    lcpc_timings t{};
    (void)hipEventElapsedTime(&t.encode_ms, m0->ev[0], m0->ev[1]);
    if (s.member_hash) { t.hash_ms = hash_ms; t.merkle_ms = merkle_ms; }
    else {
      (void)hipEventElapsedTime(&t.hash_ms, m0->ev[1], m0->ev[2]);
      (void)hipEventElapsedTime(&t.merkle_ms, m0->ev[2], m0->ev[3]);
    }
    (void)hipEventElapsedTime(&t.total_ms, m0->ev[0], ev_end);
    for (uint32_t i = 0; i < n_batch; i++) {     // phase times and launch counts only: the other fields are the member's own (begin_commit reset them)
      lcpc_timings& l = cms[i]->last;
      l.encode_ms = t.encode_ms; l.hash_ms = t.hash_ms; l.merkle_ms = t.merkle_ms; l.total_ms = t.total_ms;
      l.encode_launches = launches[0]; l.hash_launches = launches[1]; l.merkle_launches = launches[2];
    }
  }
  for (uint32_t i = 0; i < n_batch; i++) {
    lcpc_commit_t* m = cms[i];
    m->launches[0] = launches[0]; m->launches[1] = launches[1]; m->launches[2] = launches[2];
    m->coeffs_view = s.borrow ? reinterpret_cast<const uint32_t*>(coeffs_dev) + (size_t)i * s.stride * c->NL : m->d_coeffs;
    if (!m->ev_done) HIPCHK(m0, hipEventCreateWithFlags(&m->ev_done, hipEventDisableTiming));
    HIPCHK(m0, hipEventRecord(m->ev_done, st));
  }
  for (uint32_t i = 0; i < n_batch; i++) cms[i]->committed = true;
  return roots ? fetch_roots(cms, n_batch, s.member_hash ? nullptr : sl.get(), st, roots) : 0;   // (member_hash: each member's own root slot)
}

// a Brakedown batch of more stacked rows than the batch launchers take: the single-commit pipeline member by member on st; the
// batch's timings are the sums
int commit_batch_each(lcpc_commit_t* const* cms, uint32_t n_batch, const uint64_t* coeffs_dev, uint64_t n_coeffs, uint64_t poly_stride,
                      hipStream_t st, uint32_t flags, uint8_t* roots) {
  lcpc_commit_t* m0 = cms[0];
  const lcpc_ctx* c = m0->enc;
  const uint64_t stride = poly_stride ? poly_stride : n_coeffs;
  const bool timing = m0->timing;
  lcpc_timings sum{};
  for (uint32_t i = 0; i < n_batch; i++) {
    lcpc_commit_t* m = cms[i];
    const bool own_timing = m->timing;
    m->timing = timing;
    int rc = commit_device_locked(m, coeffs_dev + (size_t)i * stride * c->L, n_coeffs, st, flags, nullptr);
    m->timing = own_timing;
    if (rc) {
      if (m != m0) m0->err = m->err.c_str();
      return rc;
    }
    if (timing) {
      sum.encode_ms += m->last.encode_ms; sum.hash_ms += m->last.hash_ms; sum.merkle_ms += m->last.merkle_ms; sum.total_ms += m->last.total_ms;
      sum.encode_launches += m->last.encode_launches; sum.hash_launches += m->last.hash_launches; sum.merkle_launches += m->last.merkle_launches;
    }
  }
  if (timing)
    for (uint32_t i = 0; i < n_batch; i++) {
      lcpc_timings& t = cms[i]->last;
      t.encode_ms = sum.encode_ms; t.hash_ms = sum.hash_ms; t.merkle_ms = sum.merkle_ms; t.total_ms = sum.total_ms;
      t.encode_launches = sum.encode_launches; t.hash_launches = sum.hash_launches; t.merkle_launches = sum.merkle_launches;
    }
  return roots ? fetch_roots(cms, n_batch, nullptr, st, roots) : 0;
}

// =====================================================================================================
// lcpcx_prove_batch: LcCommit::prove (lcpc-2d lib.rs:1004-1093; prove.cpp prove_impl) for every member of a batch in lockstep.
// Per group of members: each degree-test round is one upload of all tensors, the batched collapse chain (kernels.hip K5b), one
// copy down and ONE synchronisation, then every member absorbs its p_random on the host pool; the open is one upload of all
// column numbers, the two batched gathers (K6b), the copies down and ONE synchronisation.  Round 0 fuses the outer tensor as the
// second tensor, as the sharded prove does.  A member's transcript work of one step -- absorb, the copy into its proof, the draw
// for the next step -- is one task of the pool, so the members' serial STROBE absorbs overlap each other.
// =====================================================================================================
constexpr uint64_t PROVE_ARENA_BUDGET = LCPCX_PROVE_ARENA_BUDGET;      // pinned bytes of one group (include/lcpc_hip_batch.h, groups)

// one member as the K5b / K6b kernels see it (commit.cpp collapse_prepare, open_columns_device)
ProveMember describe_member(const lcpc_commit_t* m) {
  const lcpc_ctx* c = m->enc;
  ProveMember d{};
  d.coeffs = m->coeffs_view; d.hashes = m->d_hashes;
  if (m->comm_t) { d.comm = m->ws.d_t; d.comm_row_stride = 1; d.comm_col_stride = m->n_rows_local; d.comm_canon = 1u; }
  else { d.comm = m->d_comm; d.comm_row_stride = c->n_cols; d.comm_col_stride = 1; d.comm_canon = c->comm_canon ? 1u : 0u; }
  return d;
}

struct ProofBufs {                 // the proofs of a call that does not succeed go back, and the caller sees NULLs
  uint8_t** p; uint32_t n; bool keep = false;
  ~ProofBufs() {
    if (keep) return;
    for (uint32_t i = 0; i < n; i++) { proof_buf_free(p[i]); p[i] = nullptr; }
  }
};

// every member's fill_mu held shared; arguments checked
int prove_batch_locked(lcpc_commit_t* const* cms, uint32_t n_batch, const uint64_t* outer, uint64_t outer_stride, lcpc_transcript* const* trs,
                       uint8_t** proofs, uint64_t* proof_lens, uint64_t* cols_opened, lcpcx_prove_stats* stats) {
  lcpc_commit_t* m0 = cms[0];
  const lcpc_ctx* c = m0->enc;
  const FieldDesc& f = *c->f;
  const int L = f.L;
  const uint64_t F = elem_bytes(c), nr = m0->n_rows, np = c->n_per_row;
  const ProofLayout pl = proof_layout(c, nr);
  const uint64_t n_deg = pl.n_deg, n_open = pl.n_open;
  const uint32_t path_len = c->path_len, splits = collapse_splits(m0);
  const bool dbg = c->sw_debug_timing;
  const double t_start = now_ms();
  double t_draw = 0, t_dev = 0, t_absorb = 0, t_open = 0, t_frame = 0;
  // the pinned arena of one member (the header's A): tensors | polynomials and canonical forms | columns | opened values | paths
  const uint64_t a_t = 2 * nr * F, a_p = 4 * np * F, a_c = n_open * 8, a_v = n_open * nr * F, a_h = n_open * path_len * pl.dl;
  const uint64_t arena = a_t + a_p + a_c + a_v + a_h;
  uint64_t gmax = PROVE_ARENA_BUDGET / arena;
  if (gmax < 1) gmax = 1;
  if (gmax > n_batch) gmax = n_batch;
  lcpcx_prove_stats stt{};
  stt.groups = (uint32_t)((n_batch + gmax - 1) / gmax);

  std::vector<ProveMember> desc(n_batch);        // (outlives the working set's stream: it is the source of an asynchronous copy)
  for (uint32_t i = 0; i < n_batch; i++) desc[i] = describe_member(cms[i]);
  std::vector<uint64_t> eval_canon;              // to_repr of p_eval from round 0, absorbed after the last round
  if (n_deg > 1) eval_canon.resize(gmax * np * L);
  ProofBufs bufs{proofs, n_batch};
  for (uint32_t i = 0; i < n_batch; i++)
    if (!(proofs[i] = static_cast<uint8_t*>(proof_buf_alloc(pl.total ? pl.total : 1)))) return LCPC_ERR_NOMEM;

  SetLease<CallSet> ws{m0->sets};
  int rc = take_call_set(m0, gmax * arena, &ws.s);
  if (rc) return rc;
  hipStream_t st = ws.s->st;
  for (uint32_t i = 1; i < n_batch; i++)
    if ((rc = order_after_commit(cms[i], st))) { m0->err = cms[i]->err.c_str(); return rc; }
  // device scratch: [descriptors][tensors][polys | canon][partials][cols][vals][paths], each segment 256-byte aligned
  const uint64_t s_desc = align256((uint64_t)n_batch * sizeof(ProveMember)), s_t = align256(gmax * a_t), s_p = align256(gmax * a_p);
  const uint64_t s_part = splits > 1 ? align256(gmax * splits * 2 * np * F) : 0;
  const uint64_t s_c = align256(gmax * a_c), s_v = align256(gmax * a_v), s_h = align256(gmax * a_h);
  if ((rc = ensure_scratch(m0, &ws.s->sc, s_desc + s_t + s_p + s_part + s_c + s_v + s_h))) return rc;
  uint8_t* base = reinterpret_cast<uint8_t*>(ws.s->sc.d);
  const ProveMember* d_desc = reinterpret_cast<const ProveMember*>(base);
  uint32_t* d_t = reinterpret_cast<uint32_t*>(base + s_desc);
  uint32_t* d_p = reinterpret_cast<uint32_t*>(base + s_desc + s_t);
  uint32_t* d_part = reinterpret_cast<uint32_t*>(base + s_desc + s_t + s_p);
  uint64_t* d_cols = reinterpret_cast<uint64_t*>(base + s_desc + s_t + s_p + s_part);
  uint32_t* d_vals = reinterpret_cast<uint32_t*>(base + s_desc + s_t + s_p + s_part + s_c);
  uint32_t* d_paths = reinterpret_cast<uint32_t*>(base + s_desc + s_t + s_p + s_part + s_c + s_v);
  if (c->NL == 8 && (rc = ensure_dev(&m0->err, &ws.s->sc.t29, &ws.s->sc.t29_cap, gmax * 2 * nr * 48))) return rc;
  HIPCHK(m0, hipMemcpyAsync(base, desc.data(), (size_t)n_batch * sizeof(ProveMember), hipMemcpyHostToDevice, st));

  for (uint32_t g0 = 0; g0 < n_batch; g0 += (uint32_t)gmax) {
    const uint32_t g = (uint32_t)std::min<uint64_t>(gmax, n_batch - g0);
    uint64_t* h_t = reinterpret_cast<uint64_t*>(ws.s->h_pin);
    uint64_t* h_p = reinterpret_cast<uint64_t*>(ws.s->h_pin + g * a_t);
    uint64_t* h_cols = reinterpret_cast<uint64_t*>(ws.s->h_pin + g * (a_t + a_p));
    uint64_t* h_vals = reinterpret_cast<uint64_t*>(ws.s->h_pin + g * (a_t + a_p + a_c));
    uint8_t* h_paths = ws.s->h_pin + g * (a_t + a_p + a_c + a_v);
    // member i of the group draws the tensor of its next round ([member][tensor][n_rows]; round 0 takes the outer tensor second)
    auto draw_tensor = [&](uint32_t i, uint32_t nt) {
      uint8_t key[32];
      trs[g0 + i]->t.challenge_bytes(LBL_DT, 6, key, 32);                       // lib.rs:1024-1043
      ChaCha20Rng rng(key);
      uint64_t* t = h_t + (size_t)i * nt * nr * L;
      for (uint64_t r = 0; r < nr; r++) rng.field_random(f, &t[r * L]);
      if (nt == 2) memcpy(t + nr * L, outer + (size_t)(g0 + i) * outer_stride * L, nr * F);
    };
    double t0 = now_ms();
    parallel_for(g, 1, [&](uint64_t b, uint64_t e) { for (uint64_t i = b; i < e; i++) draw_tensor((uint32_t)i, 2); });
    t_draw += now_ms() - t0;
    for (uint64_t round = 0; round < n_deg; round++) {
      const uint32_t nt = round == 0 ? 2 : 1;
      const uint64_t n_poly = (uint64_t)g * nt * np;                               // elements of all polynomials of this round
      t0 = now_ms();
      HIPCHK(m0, hipMemcpyAsync(d_t, h_t, (size_t)g * nt * nr * F, hipMemcpyHostToDevice, st));
      CollapseArgs b{};                                                           // the batch form: member = grid z
      b.members = d_desc + g0; b.n_batch = g; b.tensors = d_t; b.out = splits == 1 ? d_p : d_part;
      b.n_rows = nr; b.n_per_row = np; b.n_tensors = nt; b.n_splits = splits;
      if (c->NL == 8) {
        HIPCHK(m0, launch_to_r29(d_t, (uint64_t)g * nt * nr, ws.s->sc.t29, st));
        b.tensors29 = ws.s->sc.t29;
        stt.collapse_launches++;
      }
      HIPCHK(m0, launch_collapse(c->NL, b, st));
      stt.collapse_launches++;
      if (splits > 1) {
        HIPCHK(m0, launch_field_sum_batch(c->NL, d_part, splits, (uint64_t)nt * np, d_p, g, st));
        stt.collapse_launches++;
      }
      HIPCHK(m0, launch_to_canon(c->NL, d_p, n_poly, d_p + n_poly * c->NL, st));   // the canonical forms right behind the polynomials
      stt.collapse_launches++;
      HIPCHK(m0, hipMemcpyAsync(h_p, d_p, (size_t)2 * n_poly * F, hipMemcpyDeviceToHost, st));
      HIPCHK(m0, hipStreamSynchronize(st));
      stt.host_syncs++;
      t_dev += now_ms() - t0;
      t0 = now_ms();
      const bool last = round + 1 == n_deg;
      parallel_for(g, 1, [&](uint64_t mb, uint64_t me) {
        for (uint64_t i = mb; i < me; i++) {
          Transcript& tr = trs[g0 + i]->t;
          uint8_t* out = proofs[g0 + i];
          const uint64_t* polys = h_p + i * nt * np * L;
          const uint64_t* canon = h_p + (n_poly + i * nt * np) * L;
          tr.append_messages(LBL_PR, 6, reinterpret_cast<const uint8_t*>(canon), 8 * L, np);          // lib.rs:1045-1047
          memcpy(out + pl.off_rand0 + round * (8 + pl.pbytes), polys, pl.pbytes);
          if (round == 0) {
            memcpy(out + pl.off_eval, polys + np * L, pl.pbytes);
            if (n_deg > 1) memcpy(&eval_canon[i * np * L], canon + np * L, pl.pbytes);
          }
          if (!last) { draw_tensor((uint32_t)i, 1); continue; }
          const uint64_t* pe = n_deg > 1 ? &eval_canon[i * np * L] : canon + np * L;
          tr.append_messages(LBL_PE, 6, reinterpret_cast<const uint8_t*>(pe), 8 * L, np);             // lib.rs:1066-1068
          draw_columns(tr, c, h_cols + i * n_open, n_open);
          proof_write_head(pl, out);
        }
      });
      t_absorb += now_ms() - t0;
    }
    t0 = now_ms();
    HIPCHK(m0, hipMemcpyAsync(d_cols, h_cols, (size_t)g * a_c, hipMemcpyHostToDevice, st));
    HIPCHK(m0, launch_gather_columns_batch(c->NL, d_desc + g0, g, nr, d_cols, (uint32_t)n_open, d_vals, c->d_r2, st));
    stt.open_launches += (uint32_t)((n_open + 32767) / 32768);
    HIPCHK(m0, hipMemcpyAsync(h_vals, d_vals, (size_t)g * a_v, hipMemcpyDeviceToHost, st));
    if (path_len) {
      HIPCHK(m0, launch_gather_paths_batch(d_desc + g0, g, c->np2, path_len, d_cols, (uint32_t)n_open, d_paths, digest_words(c), st));
      stt.open_launches++;
      HIPCHK(m0, hipMemcpyAsync(h_paths, d_paths, (size_t)g * a_h, hipMemcpyDeviceToHost, st));
    }
    HIPCHK(m0, hipStreamSynchronize(st));
    stt.host_syncs++;
    t_open += now_ms() - t0;
    t0 = now_ms();
    // framing, values and paths of every opened column of every member: flat over (member, column)
    parallel_for((uint64_t)g * n_open, 256, [&](uint64_t b, uint64_t e) {
      while (b < e) {
        const uint64_t i = b / n_open, k0 = b % n_open, k1 = std::min<uint64_t>(n_open, k0 + (e - b));
        proof_write_columns(pl, proofs[g0 + i], h_paths + i * a_h, h_vals + i * n_open * nr * L, k0, k1);
        b += k1 - k0;
      }
    });
    if (cols_opened) memcpy(cols_opened + (size_t)g0 * n_open, h_cols, (size_t)g * a_c);
    t_frame += now_ms() - t0;
  }
  for (uint32_t i = 0; i < n_batch; i++) proof_lens[i] = pl.total;
  bufs.keep = true;
  if (stats) *stats = stt;
  if (dbg)
    fprintf(stderr, "[lcpcx_prove_batch] %u members in %u groups: draw tensors %.2f ms, collapse (device + copies) %.2f, absorb + draw %.2f, "
                    "open %.2f, bincode %.2f, total %.2f; %u collapse + %u open launches, %u syncs\n",
            n_batch, stt.groups, t_draw, t_dev, t_absorb, t_open, t_frame, now_ms() - t_start, stt.collapse_launches, stt.open_launches,
            stt.host_syncs);
  return 0;
}

}  // namespace

extern "C" {

int lcpcx_batch_version(void) { return LCPCX_BATCH_VERSION; }

int lcpcx_prove_batch(lcpc_commit_t* const* cms, uint32_t n_batch, const uint64_t* outer_tensors, uint64_t n_outer, uint64_t outer_stride,
                      lcpc_transcript* const* trs, uint8_t** proofs, uint64_t* proof_lens, uint64_t* cols_opened, lcpcx_prove_stats* stats) {
  if (!proofs || n_batch == 0 || n_batch > 65535) return LCPC_ERR_ARG;
  for (uint32_t i = 0; i < n_batch; i++) proofs[i] = nullptr;                 // whatever fails from here on, no proof is returned
  if (!cms || !trs || !outer_tensors || !proof_lens || (outer_stride != 0 && outer_stride < n_outer)) return LCPC_ERR_ARG;
  for (uint32_t i = 0; i < n_batch; i++)
    if (!cms[i] || !trs[i] || cms[i]->enc != cms[0]->enc) return LCPC_ERR_ARG;
  lcpc_commit_t* m0 = cms[0];
  const lcpc_ctx* c = m0->enc;
  LCPC_TRY
  std::vector<lcpc_commit_t*> order(cms, cms + n_batch);
  std::sort(order.begin(), order.end(), std::less<lcpc_commit_t*>());
  if (std::adjacent_find(order.begin(), order.end()) != order.end()) return LCPC_ERR_ARG;       // a member listed twice
  {
    std::vector<lcpc_transcript*> t(trs, trs + n_batch);
    std::sort(t.begin(), t.end(), std::less<lcpc_transcript*>());
    if (std::adjacent_find(t.begin(), t.end()) != t.end()) return LCPC_ERR_ARG;                 // a transcript listed twice
  }
  if (c->prm.shard_count > 1) return LCPC_ERR_STATE;
  // a reader of every member, in the batch commit's lock order: a refill of any member waits, readers run beside
  std::vector<std::shared_lock<FillLock>> readers;
  readers.reserve(n_batch);
  for (lcpc_commit_t* m : order) readers.emplace_back(m->fill_mu);
  for (uint32_t i = 0; i < n_batch; i++)
    if (!cms[i]->committed) return LCPC_ERR_STATE;
  for (uint32_t i = 0; i < n_batch; i++)
    if (cms[i]->n_rows != m0->n_rows) return LCPC_ERR_ARG;
  if (!lcpc_dims_ok(c, c->n_per_row, c->n_cols)) return LCPC_ERR_COMMIT;      // check_comm lib.rs:1015
  if (n_outer != m0->n_rows) return LCPC_ERR_OUTER_TENSOR;                     // lib.rs:1016-1018
  return prove_batch_locked(cms, n_batch, outer_tensors, outer_stride, trs, proofs, proof_lens, cols_opened, stats);
  LCPC_CATCH(m0)
}

int lcpcx_commit_batch_device(lcpc_commit_t* const* cms, uint32_t n_batch, const uint64_t* coeffs_dev, uint64_t n_coeffs,
                              uint64_t poly_stride, void* stream, uint32_t flags, uint8_t* roots) {
  if (!cms || !coeffs_dev || n_batch == 0 || n_batch > 65535 || n_coeffs == 0 || (poly_stride != 0 && poly_stride < n_coeffs)) return LCPC_ERR_ARG;
  for (uint32_t i = 0; i < n_batch; i++)
    if (!cms[i] || cms[i]->enc != cms[0]->enc) return LCPC_ERR_ARG;
  lcpc_commit_t* m0 = cms[0];
  const lcpc_ctx* c = m0->enc;
  LCPC_TRY
  // one global lock order -- by address -- whatever order the caller lists the members in: overlapping batches cannot deadlock
  std::vector<lcpc_commit_t*> order(cms, cms + n_batch);
  std::sort(order.begin(), order.end(), std::less<lcpc_commit_t*>());
  if (std::adjacent_find(order.begin(), order.end()) != order.end()) return LCPC_ERR_ARG;       // a member listed twice
  if (c->prm.shard_count > 1) return LCPC_ERR_STATE;
  std::vector<std::unique_lock<FillLock>> fills;
  std::vector<std::unique_lock<std::mutex>> mus;
  fills.reserve(n_batch); mus.reserve(n_batch);
  for (lcpc_commit_t* m : order) fills.emplace_back(m->fill_mu);     // fills: each waits for the readers in flight (internal.h)
  for (lcpc_commit_t* m : order) mus.emplace_back(m->mu);
  HIPCHK(m0, hipSetDevice(c->prm.device));
  hipStream_t st = (hipStream_t)stream;
  // Brakedown: the stacked rows are one grid dimension of the transposes, in tiles of 32 (kernels.h launch_transpose_to_t_batch)
  const uint64_t n_rows = (n_coeffs + c->n_per_row - 1) / c->n_per_row;
  const bool fast = c->prm.encoding == LCPC_ENC_LIGERO || (uint64_t)n_batch * n_rows <= (uint64_t)65535 * 32;
  int rc = fast ? commit_batch_fast(cms, n_batch, coeffs_dev, n_coeffs, poly_stride, st, flags, roots)
                : commit_batch_each(cms, n_batch, coeffs_dev, n_coeffs, poly_stride, st, flags, roots);
  if (rc)                          // a failed batch leaves no member committed
    for (uint32_t i = 0; i < n_batch; i++) cms[i]->committed = false;
  return rc;
  LCPC_CATCH(m0)
}

}  // extern "C"

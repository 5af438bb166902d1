// lcpc_amd/csrc/columns.cpp -- lcpcp_check_columns (include/lcpc_hip_columns.h): verify_column_path (lcpc-2d lib.rs:955-982) for columns
// opened outside a proof, on the device.
//
// The columns run in slices.  Per slice of s columns:
//   1. host pool, one task per column: the limb check and the copy of the column's values into the pinned arena -- the slice is a
//      position-major matrix of s columns, as a member's opened columns are in verify_batch.cpp -- and of its path, as it came
//      (column-major).  A column with a limb >= p leaves a hole of zeros and is answered 0.
//   2. device, on the working set's stream: ONE upload (values | column numbers | zeroed status words | root | siblings), the leaf
//      digests and K8b on the column-major layout (both shared with the batched verify: verify_batch.cpp), ONE download of the status
//      words, one synchronisation.
// The working set is one of the batched verify's; the encoder's lock is not taken: nothing here touches the encode workspace.
#include "internal.h"
#include "../../include/lcpc_hip_verify.h"
#include "../../include/lcpc_hip_columns.h"

using namespace lcpc;

namespace {

inline uint64_t align256(uint64_t x) { return (x + 255) & ~(uint64_t)255; }

int check_columns_run(lcpc_ctx* c, const uint8_t* root, const uint64_t* cols, uint32_t n, uint64_t nr, const uint64_t* col_vals,
                      const uint8_t* paths, uint8_t* ok) {
  const FieldDesc& f = *c->f;
  const int L = f.L;
  const uint64_t F = elem_bytes(c), dl = digest_len(c), path_len = c->path_len;
  const uint32_t dw = digest_words(c);
  for (uint32_t i = 0; i < n; i++)
    if (cols[i] >= c->n_cols) return LCPC_ERR_COLUMN_NUMBER;
  // a slice: its values (with the column number, the status word and the digest of each column) within the arena budget, its siblings
  // within the path budget, at least one column
  const uint64_t col_b = nr * F, sib_b = path_len * dl;
  uint64_t s_max = std::max<uint64_t>(1, LCPCV_ARENA_BUDGET / (col_b + 12 + dl));
  if (sib_b) s_max = std::min(s_max, std::max<uint64_t>(1, LCPCV_PATH_BUDGET / sib_b));
  s_max = std::min<uint64_t>(s_max, n);
  // bytes; every segment starts at a multiple of 256.  (The values: whole elements and a multiple of 16 bytes, as the hash launchers want)
  const uint64_t vals_b = (L % 2 ? (s_max * nr + 1) & ~(uint64_t)1 : s_max * nr) * F;
  const uint64_t o_drawn = align256(vals_b), o_stat = o_drawn + align256(s_max * 8), o_root = o_stat + align256(s_max * 4);
  const uint64_t o_sibs = o_root + align256(dl), up_b = o_sibs + align256(std::max<uint64_t>(s_max * sib_b, 16));
  const uint64_t o_dig = up_b, o_canon = o_dig + align256(s_max * dl), canon_b = align256(staged_canon_bytes(c, vals_b));
  const uint64_t o_cvs = o_canon + canon_b, cvs_b = staged_cvs_bytes(c, s_max, nr);

  HIPCHK(c, hipSetDevice(c->prm.device));
  SetLease<VerifyBatchSet> ws{c->verify_batch_sets};
  if (int rc = c->verify_batch_sets.take(up_b, &ws.s)) return rc;
  if (int rc = ensure_dev(&c->err, &ws.s->d, &ws.s->d_cap, o_cvs + align256(cvs_b))) return rc;
  hipStream_t st = ws.s->st;
  uint8_t* const hb = ws.s->h_pin;
  uint8_t* const db = ws.s->d;
  auto d32 = [&](uint64_t off) { return reinterpret_cast<uint32_t*>(db + off); };
  std::unique_ptr<uint8_t[]> bad(new uint8_t[s_max]);
  memcpy(hb + o_root, root, dl);

  for (uint64_t k0 = 0; k0 < n; k0 += s_max) {
    const uint64_t s = std::min<uint64_t>(s_max, n - k0);
    const uint64_t used_b = (L % 2 ? (s * nr + 1) & ~(uint64_t)1 : s * nr) * F;
    parallel_for(s, 1, [&](uint64_t b, uint64_t e) {
      for (uint64_t k = b; k < e; k++) {
        const uint64_t* src = col_vals + (k0 + k) * nr * L;
        uint64_t* dst = reinterpret_cast<uint64_t*>(hb) + k * nr * L;
        bad[k] = 0;
        for (uint64_t r = 0; r < nr; r++)
          if (h_ge_p(f, src + r * L)) { bad[k] = 1; break; }
        if (bad[k]) memset(dst, 0, col_b);                       // the hole: zeros, never read as data
        else memcpy(dst, src, col_b);
        if (sib_b) memcpy(hb + o_sibs + k * sib_b, paths + (k0 + k) * sib_b, sib_b);
      }
    });
    if (used_b > s * col_b) memset(hb + s * col_b, 0, used_b - s * col_b);
    memcpy(hb + o_drawn, cols + k0, s * 8);
    memset(hb + o_stat, 0, s * 4);
    HIPCHK(c, hipMemcpyAsync(db, hb, o_sibs + std::max<uint64_t>(s * sib_b, 16), hipMemcpyHostToDevice, st));
    StagedColumns sc{};
    sc.cols = d32(0); sc.cols_stride_w = used_b / 4; sc.canon = d32(o_canon); sc.cvs = d32(o_cvs); sc.cvs_stride_w = 0;
    sc.digests = d32(o_dig); sc.dig_stride_w = s * dw; sc.n_open = s; sc.n_rows = nr; sc.n_batch = 1;
    if (int rc = enqueue_leaf_digests(c, sc, st, nullptr)) return rc;
    FoldPathsArgs fa{};
    fa.leaves = d32(o_dig); fa.leaves_stride = 0; fa.drawn = reinterpret_cast<const uint64_t*>(db + o_drawn);
    fa.sibs = d32(o_sibs); fa.sib_member = 0; fa.sib_col = path_len * dw; fa.sib_lvl = dw;      // column-major [column][lvl]
    fa.roots = d32(o_root); fa.status = d32(o_stat); fa.status_stride = 0;
    fa.n_open = (uint32_t)s; fa.depth = (uint32_t)path_len; fa.n_batch = 1;
    if (int rc = enqueue_fold_paths(c, fa, st, nullptr)) return rc;
    HIPCHK(c, hipMemcpyAsync(hb + o_stat, db + o_stat, s * 4, hipMemcpyDeviceToHost, st));
    HIPCHK(c, hipStreamSynchronize(st));
    const uint32_t* h_stat = reinterpret_cast<const uint32_t*>(hb + o_stat);
    for (uint64_t k = 0; k < s; k++) ok[k0 + k] = !bad[k] && !(h_stat[k] & FOLD_PATH_BIT);
  }
  return 0;
}

}  // namespace

extern "C" {

int lcpcp_version(void) { return LCPCP_VERSION; }

int lcpcp_check_columns(lcpc_ctx* c, const uint8_t* root, const uint64_t* cols, uint32_t n, uint64_t n_rows, const uint64_t* col_vals,
                        const uint8_t* paths, uint8_t* ok) {
  if (!c || !root || !cols || !col_vals || !paths || !ok || n_rows == 0) return LCPC_ERR_ARG;
  if (n == 0) return 0;
  LCPC_TRY
  if (c->prm.shard_count > 1) return LCPC_ERR_STATE;
  return check_columns_run(c, root, cols, n, n_rows, col_vals, paths, ok);
  LCPC_CATCH(c)
}

}  // extern "C"

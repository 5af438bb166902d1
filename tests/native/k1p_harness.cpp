// tests/native/k1p_harness.cpp -- test-only C entry points that LAUNCH the pass kernels of the Ligero row NTT (K1) one at a time: one
// step of a real context's plan through the launcher the product calls for it (kernels.h launch_ntt_pass, launch_ntt_pass_l9s,
// launch_ntt_pass_lns), the general kernel on a free split of the stages, and the launchers' documented refusals.  In the manner of
// k1_harness.cpp, which reads the tables these passes load: built by lcpc_amd/csrc/Makefile into lcpc_amd/lib/liblcpc_k1p_harness.so and
// linked against the product library, which gains nothing by it (tests/k1p_harness.py, tests/k1_pass_model.py,
// tests/test_gpu_k1_passes.py).
//
// The context is made by the public lcpc_ctx_create (the LCPC_NTT_* switches are read there, so the caller sets them around k1p_open)
// and read through internal.h -- compiled WITHOUT LCPC_TEST_HOOKS, so struct lcpc_ctx has the product's layout.  NttPassArgs is filled
// by fill_step below, which restates the loop body of ctx.cpp encode_rows_device; what a caller may vary is what a job varies there (rows,
// source stride, n_valid, n_src_total, copy_dst, canonical output, the limb intermediate) and what the kernels honour besides: a dst
// stride larger than a row (every pass kernel addresses dst by row * dst_stride), a src stride larger than a row on the later steps
// (src by row * src_stride), in place or out of place on the steps the product runs in place.  a.mid has no stride (row << log_n).
//
// Every buffer a pass may write -- dst, mid, copy_dst -- is one device allocation [canary | body | canary] filled with 0xA5 bytes and
// returned whole, gaps between rows included.  Host buffers come with their sizes; a request that is out of range or inconsistent is
// refused (K1P_BAD_ARGS) before the device is touched, and the sizes the caller states must be exactly the ones computed here.  The
// source is uploaded into an allocation of exactly the words the pass may read.
#include <string.h>

#include <algorithm>
#include <memory>

#include "harness.h"
#include "../../lcpc_amd/csrc/internal.h"

// the entry points also return lcpc status codes: a hipError_t comes back as 1000 + e, a refused call as -1000
#define K1P_BAD_ARGS (-1000)
#define K1P_TRY(expr) H_TRY_OFF(expr, 1000)

namespace {

using namespace lcpc;

constexpr uint64_t CANARY_WORDS = 1024;                 // in front of and behind every body
constexpr uint32_t CANARY = 0xA5A5A5A5u;
// per buffer: 1 GiB of Ft255; rows: a device filled with one-tile rows (tests/test_gpu_k1_saturated.py: 2 x CUs x 8 workgroups)
constexpr uint64_t MAX_ROWS = 8192, MAX_ELEMS = (uint64_t)1 << 25;
enum : uint64_t { F_COPY = 1, F_CANON = 2, F_MID = 4, F_INPLACE = 8, F_MONTWORD = 16 };
constexpr uint64_t UNLIMITED = ~(uint64_t)0;

// not harness.h's DevBuf: [canary | body | canary] in one allocation, fetched whole
struct CanaryBuf {
  uint32_t* p = nullptr;
  uint64_t body = 0;                                    // words between the canaries
  ~CanaryBuf() { if (p) (void)hipFree(p); }
  hipError_t alloc_plain(uint64_t words) { return hipMalloc((void**)&p, words ? words * 4 : 16); }
  hipError_t alloc_canary(uint64_t words) {
    body = words;
    hipError_t e = hipMalloc((void**)&p, (words + 2 * CANARY_WORDS) * 4);
    return e != hipSuccess ? e : hipMemset(p, 0xA5, (words + 2 * CANARY_WORDS) * 4);
  }
  uint32_t* at() const { return p + CANARY_WORDS; }
  hipError_t fetch(uint32_t* host) const { return hipMemcpy(host, p, (body + 2 * CANARY_WORDS) * 4, hipMemcpyDeviceToHost); }
};

const lcpc_ctx* ctx_of(const void* h) {
  const lcpc_ctx* c = static_cast<const lcpc_ctx*>(h);
  return c && c->prm.encoding == LCPC_ENC_LIGERO ? c : nullptr;
}
uint32_t classes_of(const NttStep& p) {                 // the rule of ctx.cpp build_limb_plan
  if (p.kernel == NttStep::GENERAL) return 0;
  const bool nf = p.a.form != 0;
  return p.first != nf ? 1u << (p.a.log_n - 10) : 1u;
}

// what a caller chooses for one launch
struct Req {
  uint64_t n_rows, src_stride, dst_stride, n_valid, n_src_total, flags;
  bool has(uint64_t f) const { return (flags & f) != 0; }
};
// the buffers of one launch, in elements / words
struct Sizes { uint64_t n_sub, len, src_words, dst_words, mid_words, copy_words; };

bool common_ok(const Req& r, uint64_t len, uint64_t n_sub, bool reads_job) {
  if (r.n_rows == 0 || r.n_rows > MAX_ROWS || n_sub * len > MAX_ELEMS) return false;
  if (r.dst_stride < len || r.dst_stride > 4 * len || r.src_stride == 0 || r.src_stride > 4 * len) return false;
  if (n_sub * r.dst_stride > MAX_ELEMS || n_sub * r.src_stride > MAX_ELEMS) return false;
  if (r.n_valid > len) return false;
  if (reads_job) return r.n_valid <= r.src_stride;
  return r.n_valid == len && r.n_src_total == UNLIMITED && r.src_stride >= len && !r.has(F_COPY);
}
// elements of the source a pass may read: g < n_valid of every row, the flat index below n_src_total
uint64_t src_elems(const Req& r, uint64_t n_sub) { return std::min(r.n_src_total, (n_sub - 1) * r.src_stride + r.n_valid); }

// one step of the plan: false = refused
bool step_sizes(const lcpc_ctx* c, uint32_t step, const Req& r, Sizes& z) {
  if (step >= c->ntt.size() || (r.flags & ~(F_COPY | F_CANON | F_MID | F_INPLACE))) return false;
  const NttStep& p = c->ntt[step];
  const bool first = step == 0;
  z.len = (uint64_t)1 << p.a.log_n;
  z.n_sub = r.n_rows << (c->log_n - p.a.log_n);
  if (!common_ok(r, z.len, z.n_sub, first)) return false;
  if (r.has(F_CANON) && !p.roots29c) return false;
  // the limb intermediate exists between the two passes of a K1s two-pass plan only (ctx.cpp ntt_mid_rows); it is never in place
  if (r.has(F_MID) && (p.kernel != NttStep::K1S || c->ntt.size() != 2 || r.has(F_INPLACE))) return false;
  if (r.has(F_INPLACE) && (first || r.src_stride != r.dst_stride)) return false;
  const uint64_t NL = (uint64_t)c->NL;
  z.mid_words = r.has(F_MID) ? z.n_sub * z.len * 9 : 0;
  z.src_words = (r.has(F_MID) && !first) ? z.mid_words : src_elems(r, z.n_sub) * NL;
  z.dst_words = z.n_sub * r.dst_stride * NL;
  z.copy_words = r.has(F_COPY) ? r.n_rows * r.src_stride * NL : 0;
  return true;
}

// NttPassArgs of step `step` as encode_rows_device (ctx.cpp) fills it for one batch of r.n_rows rows starting at row 0: a job with
// src / src_stride / n_valid / n_src_total / copy_dst / canon_out; later steps work on dst (here: on `src`, which is dst when the caller
// asks for the in-place run the product does)
NttPassArgs fill_step(const lcpc_ctx* c, uint32_t step, const Req& r, const uint32_t* src, uint32_t* dst, uint32_t* mid, uint32_t* copy) {
  const NttStep& p = c->ntt[step];
  const bool first = step == 0;
  const uint64_t len = (uint64_t)1 << p.a.log_n;
  NttPassArgs a = p.a;
  if (r.has(F_CANON)) { a.roots29c = p.roots29c; a.mont_prefix = p.mont_prefix; a.blk0_gone = p.blk0_gone; }
  a.dst = dst;
  a.src = src;
  a.src_stride = r.src_stride;
  a.dst_stride = r.dst_stride;
  a.n_valid = first ? r.n_valid : len;
  a.n_src_total = first ? r.n_src_total : UNLIMITED;
  a.copy_dst = first ? copy : nullptr;
  a.n_rows = r.n_rows << (c->log_n - p.a.log_n);
  a.mid = mid;
  return a;
}
hipError_t launch_step(const lcpc_ctx* c, const NttStep& p, const NttPassArgs& a) {
  switch (p.kernel) {
    case NttStep::K1S: return launch_ntt_pass_l9s(a, p.first, p.pack, p.pack_info, nullptr);
    case NttStep::K1N: return launch_ntt_pass_lns(c->NL, a, p.first, p.pack, p.pack_info, nullptr);
    case NttStep::GENERAL: return launch_ntt_pass(c->NL, p.log_tile, a, nullptr);
  }
  return hipErrorInvalidValue;
}

Req req_of(const uint64_t* q) { return Req{q[0], q[1], q[2], q[3], q[4], q[5]}; }

// launch_ntt_pass's instantiations (kernels.hip NTT_CASE; the lazy-limb Ft255 kernel has 2^10 and 2^11 tiles)
bool general_tile_ok(int nl, uint64_t log_tile) {
  if (log_tile < 10 || log_tile > 12) return false;
  return log_tile < 12 || nl <= 4;
}

}  // namespace

H_DEVICE_COUNT(k1p_)
H_EXPORT uint64_t k1p_canary_words() { return CANARY_WORDS; }

// a Ligero context of `fid` with new_from_dims(n_per_row, n_cols) at rate rho_num / rho_den: the status of lcpc_ctx_create
H_EXPORT int k1p_open(uint32_t fid, uint64_t n_per_row, uint64_t n_cols, uint32_t rho_num, uint32_t rho_den, void** out) {
  if (!out) return K1P_BAD_ARGS;
  *out = nullptr;
  if (fid > 3 || !n_per_row || n_per_row >= n_cols || (n_cols & (n_cols - 1)) || n_cols > ((uint64_t)1 << 22)) return K1P_BAD_ARGS;
  lcpc_params prm{};
  prm.field = fid; prm.encoding = LCPC_ENC_LIGERO; prm.hash = LCPC_HASH_BLAKE3;
  prm.rho_num = rho_num; prm.rho_den = rho_den;
  prm.n_per_row = n_per_row; prm.n_cols = n_cols;
  lcpc_ctx* c = nullptr;
  const int rc = lcpc_ctx_create(&prm, &c);
  if (rc == 0) *out = c;
  return rc;
}
H_EXPORT void k1p_close(void* h) {
  if (h) lcpc_ctx_destroy(static_cast<lcpc_ctx*>(h));
}
H_EXPORT const char* k1p_last_error(const void* h) { return h ? lcpc_last_error(static_cast<const lcpc_ctx*>(h)) : ""; }

// out[8]: NL, N, W, STRIDE, log_n, steps of the plan, comm_canon, the lazy-limb tables exist (d_rootsl and d_qpl)
H_EXPORT int k1p_info(const void* h, uint32_t* out, uint32_t out_words) {
  const lcpc_ctx* c = ctx_of(h);
  if (!c || !out || out_words < 8) return K1P_BAD_ARGS;
  out[0] = (uint32_t)c->NL; out[1] = (uint32_t)ntt_lns_limbs(c->NL); out[2] = (uint32_t)ntt_lns_limb_bits(c->NL);
  out[3] = (uint32_t)ntt_lns_stride(c->NL);
  out[4] = c->log_n; out[5] = (uint32_t)c->ntt.size(); out[6] = c->comm_canon ? 1u : 0u; out[7] = c->d_rootsl && c->d_qpl ? 1u : 0u;
  return 0;
}
// one step of the plan c->ntt, out[16]: kind (0 general, 1 K1s, 2 K1n), first, log_n, t0, s, log_tj, log_tile, form, pack_info.mul2,
// mont_prefix, blk0_gone, canon_row_mask, tile_group, pack classes (0: no pack), the step has a converting table (canonical output can
// be asked for), 0
H_EXPORT int k1p_plan(const void* h, uint32_t step, uint32_t* out, uint32_t out_words) {
  const lcpc_ctx* c = ctx_of(h);
  if (!c || !out || out_words < 16 || step >= c->ntt.size()) return K1P_BAD_ARGS;
  const NttStep& p = c->ntt[step];
  out[0] = p.kernel == NttStep::GENERAL ? 0u : (p.kernel == NttStep::K1S ? 1u : 2u);
  out[1] = p.first ? 1u : 0u;
  out[2] = p.a.log_n; out[3] = p.a.t0; out[4] = p.a.s; out[5] = p.a.log_tj; out[6] = (uint32_t)p.log_tile;
  out[7] = p.a.form; out[8] = p.pack_info.mul2;
  out[9] = p.mont_prefix; out[10] = p.blk0_gone; out[11] = p.a.canon_row_mask; out[12] = p.a.tile_group;
  out[13] = p.pack ? classes_of(p) : 0u;
  out[14] = p.roots29c ? 1u : 0u; out[15] = 0;
  return 0;
}

// ONE step of the plan.  req[6]: n_rows (whole rows of the context; a step on sub-rows runs n_rows << (log_n - its log_n) of them),
// src_stride, dst_stride (elements per (sub-)row), n_valid, n_src_total (~0: unlimited), flags (1 copy_dst, 2 canonical output, 4 limb
// intermediate, 8 in place).  Step 0 reads the job: n_valid <= src_stride, any n_src_total.  Later steps read whole rows: n_valid = the
// row length, n_src_total unlimited, no copy_dst, src_stride >= the row length; in place needs src_stride == dst_stride.
// src: step 0: the first min(n_src_total, (n_rows - 1) src_stride + n_valid) elements of the job's source; later steps: (n_sub - 1)
// src_stride + len elements, or -- the K1s last pass with the limb intermediate -- n_sub x len records of 9 words in the tile layout of
// ntt_l9s.hip.  dst / mid / copy: canary + body + canary words, body = n_sub dst_stride NL / n_sub len 9 / n_rows src_stride NL (a buffer
// that was not asked for: null, 0 words).  All sizes must be exact.
H_EXPORT int k1p_run_step(const void* h, uint32_t step, const uint64_t* req, uint32_t req_words, const uint32_t* src, uint64_t src_words,
                          uint32_t* dst, uint64_t dst_words, uint32_t* mid, uint64_t mid_words, uint32_t* copy, uint64_t copy_words) {
  const lcpc_ctx* c = ctx_of(h);
  if (!c || !req || req_words != 6 || !src || !dst) return K1P_BAD_ARGS;
  const Req r = req_of(req);
  Sizes z;
  if (!step_sizes(c, step, r, z)) return K1P_BAD_ARGS;
  const uint64_t C2 = 2 * CANARY_WORDS;
  if (src_words != z.src_words || dst_words != z.dst_words + C2) return K1P_BAD_ARGS;
  if (r.has(F_MID) ? (!mid || mid_words != z.mid_words + C2) : (mid || mid_words)) return K1P_BAD_ARGS;
  if (r.has(F_COPY) ? (!copy || copy_words != z.copy_words + C2) : (copy || copy_words)) return K1P_BAD_ARGS;
  const NttStep& p = c->ntt[step];
  K1P_TRY(hipSetDevice(c->prm.device));
  CanaryBuf d_src, d_dst, d_mid, d_copy;
  K1P_TRY(d_dst.alloc_canary(z.dst_words));
  if (r.has(F_MID)) K1P_TRY(d_mid.alloc_canary(z.mid_words));
  if (r.has(F_COPY)) K1P_TRY(d_copy.alloc_canary(z.copy_words));
  const uint32_t* a_src;
  if (r.has(F_MID) && step > 0) {                        // the last pass reads the records; src is what the product passes: dst
    if (src_words) K1P_TRY(hipMemcpy(d_mid.at(), src, src_words * 4, hipMemcpyHostToDevice));
    a_src = d_dst.at();
  } else if (r.has(F_INPLACE)) {
    if (src_words) K1P_TRY(hipMemcpy(d_dst.at(), src, src_words * 4, hipMemcpyHostToDevice));
    a_src = d_dst.at();
  } else {
    K1P_TRY(d_src.alloc_plain(src_words));
    if (src_words) K1P_TRY(hipMemcpy(d_src.p, src, src_words * 4, hipMemcpyHostToDevice));
    a_src = d_src.p;
  }
  const NttPassArgs a = fill_step(c, step, r, a_src, d_dst.at(), r.has(F_MID) ? d_mid.at() : nullptr, r.has(F_COPY) ? d_copy.at() : nullptr);
  K1P_TRY(launch_step(c, p, a));
  K1P_TRY(hipDeviceSynchronize());
  K1P_TRY(d_dst.fetch(dst));
  if (r.has(F_MID)) K1P_TRY(d_mid.fetch(mid));
  if (r.has(F_COPY)) K1P_TRY(d_copy.fetch(copy));
  return 0;
}

// launch_ntt_pass with a free split on the context's tables.  req[10]: the six of k1p_run_step (flags: 1 copy_dst, 2 canonical output --
// the lazy-limb Ft255 kernel only --, 8 in place, 16 the Montgomery-word Ft255 kernel: qp29 = null), then log_tile, t0, s, log_tj.
// Every pass of the general kernel applies n_valid / n_src_total / copy_dst, so they are free here whatever t0 is; in place needs whole
// rows (n_valid = the row length, n_src_total unlimited, equal strides) and no copy_dst.  mont_prefix is plan_passes' (canonical output,
// t0 + s = log_n).  src: the first min(n_src_total, (n_rows - 1) src_stride + n_valid) elements.
H_EXPORT int k1p_run_general(const void* h, const uint64_t* req, uint32_t req_words, const uint32_t* src, uint64_t src_words, uint32_t* dst,
                             uint64_t dst_words, uint32_t* copy, uint64_t copy_words) {
  const lcpc_ctx* c = ctx_of(h);
  if (!c || !req || req_words != 10 || !src || !dst) return K1P_BAD_ARGS;
  const Req r = req_of(req);
  const uint64_t log_tile = req[6], t0 = req[7], s = req[8], log_tj = req[9], k = c->log_n, len = (uint64_t)1 << k;
  if (r.flags & ~(F_COPY | F_CANON | F_INPLACE | F_MONTWORD)) return K1P_BAD_ARGS;
  if (!general_tile_ok(c->NL, log_tile) || s == 0 || s > k || t0 > k - s || log_tj > log_tile || s + log_tj > log_tile || s + log_tj > k)
    return K1P_BAD_ARGS;
  if (!c->d_roots || !common_ok(r, len, r.n_rows, true)) return K1P_BAD_ARGS;
  const bool l9 = c->NL == 8 && !r.has(F_MONTWORD);
  if (r.has(F_MONTWORD) && c->NL != 8) return K1P_BAD_ARGS;
  if (c->NL == 8 && (!c->d_rootsl || !c->d_qpl || !c->d_wq_w)) return K1P_BAD_ARGS;
  if (l9 && log_tile > 11) return K1P_BAD_ARGS;
  if (r.has(F_CANON) && (!l9 || !c->d_rootslc)) return K1P_BAD_ARGS;
  if (r.has(F_INPLACE) && (r.has(F_COPY) || r.n_valid != len || r.n_src_total != UNLIMITED || r.src_stride != r.dst_stride)) return K1P_BAD_ARGS;
  const uint64_t NL = (uint64_t)c->NL, C2 = 2 * CANARY_WORDS;
  const uint64_t want_src = src_elems(r, r.n_rows) * NL, want_dst = r.n_rows * r.dst_stride * NL;
  const uint64_t want_copy = r.has(F_COPY) ? r.n_rows * r.src_stride * NL : 0;
  if (src_words != want_src || dst_words != want_dst + C2) return K1P_BAD_ARGS;
  if (r.has(F_COPY) ? (!copy || copy_words != want_copy + C2) : (copy || copy_words)) return K1P_BAD_ARGS;
  K1P_TRY(hipSetDevice(c->prm.device));
  CanaryBuf d_src, d_dst, d_copy;
  K1P_TRY(d_dst.alloc_canary(want_dst));
  if (r.has(F_COPY)) K1P_TRY(d_copy.alloc_canary(want_copy));
  const uint32_t* a_src;
  if (r.has(F_INPLACE)) {
    if (src_words) K1P_TRY(hipMemcpy(d_dst.at(), src, src_words * 4, hipMemcpyHostToDevice));
    a_src = d_dst.at();
  } else {
    K1P_TRY(d_src.alloc_plain(src_words));
    if (src_words) K1P_TRY(hipMemcpy(d_src.p, src, src_words * 4, hipMemcpyHostToDevice));
    a_src = d_src.p;
  }
  NttPassArgs a{};                                       // the tables as plan_passes sets them
  a.roots = c->d_roots; a.roots29 = c->d_rootsl; a.qp29 = r.has(F_MONTWORD) ? nullptr : c->d_qpl; a.wq_w = c->d_wq_w;
  a.log_n = (uint32_t)k; a.t0 = (uint32_t)t0; a.s = (uint32_t)s; a.log_tj = (uint32_t)log_tj;
  if (r.has(F_CANON)) { a.roots29c = c->d_rootslc; a.mont_prefix = t0 + s == k ? (s % 2 == 0 ? 4u : 2u) : 0u; }
  a.src = a_src; a.dst = d_dst.at();
  a.src_stride = r.src_stride; a.dst_stride = r.dst_stride;
  a.n_valid = r.n_valid; a.n_src_total = r.n_src_total;
  a.copy_dst = r.has(F_COPY) ? d_copy.at() : nullptr;
  a.n_rows = r.n_rows;
  K1P_TRY(launch_ntt_pass(c->NL, (int)log_tile, a, nullptr));
  K1P_TRY(hipDeviceSynchronize());
  K1P_TRY(d_dst.fetch(dst));
  if (r.has(F_COPY)) K1P_TRY(d_copy.fetch(copy));
  return 0;
}

// A launcher's documented refusal, on a context whose plan has the pass it is about.  The arguments are those of a one-row launch of
// that step (Montgomery output, whole row, dst and copy_dst given) with the ONE field changed that the launcher rejects; the buffers have
// the sizes of that launch.  out[2]: the hipError_t the launcher returned, and 1 if every word of dst and copy_dst is still canary.
//   0  launch_ntt_pass: s + log_tj > log_tile (any context)
//   1  K1s last pass with mont_prefix != 0
//   2  K1s first pass with a tile_group the tile count cannot carry (tiles_per_row >> tile_group < 8)
//   3  K1s first pass of a three-pass plan with form != 0
//   4  K1s first pass of the pure form with S = 2, 7 or 9 and pack_info.mul2 (ntt_l9s_mul2_supported names no such pass)
//   5  K1n last pass with a tile_group
// BAD_ARGS if the context has no such pass.
H_EXPORT int k1p_refused(const void* h, uint32_t which, uint32_t* out, uint32_t out_words) {
  const lcpc_ctx* c = ctx_of(h);
  if (!c || !out || out_words < 2 || which > 5 || c->ntt.empty()) return K1P_BAD_ARGS;
  const uint32_t last = (uint32_t)c->ntt.size() - 1;
  const uint32_t step = which == 0 ? 0u : (which == 1 || which == 5 ? last : 0u);
  const NttStep& p = c->ntt[step];
  bool ok = false;
  switch (which) {
    case 0: ok = true; break;
    case 1: ok = p.kernel == NttStep::K1S && !p.first && last > 0; break;
    case 2: ok = p.kernel == NttStep::K1S && p.first; break;
    case 3: ok = p.kernel == NttStep::K1S && p.first && c->ntt.size() == 3 && p.a.form == 0; break;
    case 4: ok = p.kernel == NttStep::K1S && p.first && p.a.form == 1 && !ntt_l9s_mul2_supported(p.a.s, true) && !p.pack_info.mul2; break;
    case 5: ok = p.kernel == NttStep::K1N && !p.first && last > 0; break;
  }
  if (!ok) return K1P_BAD_ARGS;
  const uint64_t len = (uint64_t)1 << p.a.log_n;
  const Req r{1, len, len, len, UNLIMITED, step == 0 ? (uint64_t)F_COPY : 0};
  Sizes z;
  if (!step_sizes(c, step, r, z)) return K1P_BAD_ARGS;
  K1P_TRY(hipSetDevice(c->prm.device));
  CanaryBuf d_src, d_dst, d_copy;
  K1P_TRY(d_dst.alloc_canary(z.dst_words));
  K1P_TRY(d_copy.alloc_canary(z.copy_words));
  K1P_TRY(d_src.alloc_plain(z.src_words));
  K1P_TRY(hipMemset(d_src.p, 0, z.src_words * 4));
  NttPassArgs a = fill_step(c, step, r, d_src.p, d_dst.at(), nullptr, step == 0 ? d_copy.at() : nullptr);
  NttPackInfo pi = p.pack_info;
  hipError_t e = hipSuccess;
  switch (which) {
    case 0: {
      const int lt = p.kernel == NttStep::GENERAL ? p.log_tile : 10;
      a.t0 = 0; a.s = 1; a.log_tj = (uint32_t)lt;         // one stage on tiles twice the size of the instantiation's
      e = launch_ntt_pass(c->NL, lt, a, nullptr);
      break;
    }
    case 1: a.mont_prefix = 4; e = launch_ntt_pass_l9s(a, false, p.pack, pi, nullptr); break;
    case 2: a.tile_group = p.a.log_n - 10 >= 2 ? p.a.log_n - 12 : 1u; e = launch_ntt_pass_l9s(a, true, p.pack, pi, nullptr); break;
    case 3: a.form = 1; e = launch_ntt_pass_l9s(a, true, p.pack, pi, nullptr); break;
    case 4: pi.mul2 = 1; e = launch_ntt_pass_l9s(a, true, p.pack, pi, nullptr); break;
    case 5: a.tile_group = 1; e = launch_ntt_pass_lns(c->NL, a, false, p.pack, pi, nullptr); break;
  }
  K1P_TRY(hipDeviceSynchronize());
  bool intact = true;
  for (const CanaryBuf* b : {&d_dst, &d_copy}) {
    const uint64_t words = b->body + 2 * CANARY_WORDS;
    std::unique_ptr<uint32_t[]> host(new uint32_t[words]);
    K1P_TRY(b->fetch(host.get()));
    for (uint64_t i = 0; i < words; i++) intact = intact && host[i] == CANARY;
  }
  out[0] = (uint32_t)e;
  out[1] = intact ? 1u : 0u;
  return 0;
}

// tests/native/k1_harness.cpp -- test-only C entry points that READ the tables of the Ligero row NTT (K1) out of a real context: the
// twiddle tables d_roots / d_rootsl / d_rootslc and their three-pass subtables, the clamp table d_qpl, the fourth root's shifted
// multiples d_wq_w, and the lane-order packs of the K1s / K1n passes (lcpc_amd/csrc/ctx.cpp build_limb_plan, ntt_lns.hip).  In the manner
// of k8_harness.cpp: built by lcpc_amd/csrc/Makefile into lcpc_amd/lib/liblcpc_k1_harness.so and linked against the product library,
// which gains nothing by it (tests/k1_harness.py, tests/k1_tables.py, tests/test_gpu_k1_tables.py).
//
// The context is made by the public lcpc_ctx_create (the LCPC_NTT_* switches are read there, so the caller sets them around k1h_open)
// and read through internal.h -- compiled WITHOUT LCPC_TEST_HOOKS, so struct lcpc_ctx has the product's layout.  Nothing here launches a
// pass kernel.  The one kernel of this file, k1h_dump_kernel, loads pack entries with the product's own pack_get (ntt_ln_dev.h), so a
// test sees exactly the words a pass kernel would load; every record it is handed has been checked on the host to lie inside the class
// block the plan allocated.  Every entry point takes host buffers with their sizes and refuses (K1H_BAD_ARGS) any request that is out
// of range before it touches the device.
//
// What a pack holds is enumerated here from Shape<S, LBT>, PureShape<S> and coset_sets (ntt_ln_dev.h), skipping what the pack kernels
// skip (a round with t + 2 == k, positions jl >= period):
//   DIF / K1n pass   radix-2 slot: variants (plain, converting) x 512; radix-4 slot r: (w0, w3, w2) plain then converting x period4(r);
//                    uniform rounds (has_mul_u, S >= 8): table ((ru * 4 + jl0) * 3 + v) at u_off
//   pure first pass  the same at LBT = 0 and one class; its one uniform round: table (jl0 * 3 + v)
//   coset last pass  rounds 2 .. 4: (w, w^2, w^3) x 4^r sub-blocks; rounds 0, 1: table ((r * 4 + m) * 3 + v), m < 4^r
// A split pack (NttPackInfo.mul2) has twice the variants: b0 of variant v at v, b1 at NV + v; all of them are dumped.
#include <vector>

#include "harness.h"
#include "../../lcpc_amd/csrc/internal.h"
#include "../../lcpc_amd/csrc/ntt_ln_dev.h"

// the entry points also return lcpc status codes: a hipError_t comes back as 1000 + e, a refused call as -1000
#define K1H_BAD_ARGS (-1000)
#define K1H_TRY(expr) H_TRY_OFF(expr, 1000)

namespace {

using namespace lcpc;

// one lane-varying slot of a class block
struct Slot { uint32_t slot, off, nv, period; };       // round_off index, word offset in the class, variants stored (NV or 2 NV), positions
// one shifted-multiples table of a class block
struct UTab { uint32_t round, pos, v, off; };
struct PackShape {
  std::vector<Slot> slots;
  std::vector<UTab> utabs;
  uint32_t n_classes = 0;
  uint64_t records = 0;                                // lane-varying records per class
};
// one record the dump kernel fetches
struct Rec { uint64_t blk; uint32_t period, variant, jl, nv; };

template <class FT> __global__ void __launch_bounds__(256) k1h_dump_kernel(const u32* pack, const Rec* recs, u32 n, u32* out, u32 rec_words) {
  const u32 i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const Rec r = recs[i];
  const u32* blk = pack + r.blk;
  LN<FT::N> e;
  switch (r.nv) {
    case 2: e = pack_get<FT, 2>(blk, r.period, r.variant, r.jl); break;
    case 3: e = pack_get<FT, 3>(blk, r.period, r.variant, r.jl); break;
    case 4: e = pack_get<FT, 4>(blk, r.period, r.variant, r.jl); break;
    case 6: e = pack_get<FT, 6>(blk, r.period, r.variant, r.jl); break;
    case 12: e = pack_get<FT, 12>(blk, r.period, r.variant, r.jl); break;
    default: return;
  }
#pragma unroll
  for (int k = 0; k < FT::N; k++) out[(size_t)i * rec_words + 4 + k] = e.v[k];
}

uint32_t u_slot_words(int N) { return (uint32_t)(N * N + 31) & ~31u; }
uint32_t classes_of(const NttStep& p) {                 // the rule of ctx.cpp build_limb_plan
  if (p.kernel == NttStep::GENERAL) return 0;
  const bool nf = p.a.form != 0;
  return p.first != nf ? 1u << (p.a.log_n - 10) : 1u;
}

// a DIF / K1n pass, or (LBT = 0, one class) the pure first pass
template <int S, int LBT> void shape_dif(const NttStep& p, int N, bool has_u, PackShape& d) {
  using SH = Shape<S, LBT>;
  const NttPackInfo& pi = p.pack_info;
  const uint32_t k = p.a.log_n, t0 = p.a.t0, nb = pi.mul2 ? 2u : 1u, US = u_slot_words(N);
  if (SH::U0) d.slots.push_back({0u, pi.round_off[0], 2 * nb, SH::period2});
  for (int r = 0; r < SH::NR4; r++) {
    if (t0 + SH::U0 + 2 * r + 2 == k) continue;
    d.slots.push_back({(uint32_t)(SH::U0 + r), pi.round_off[SH::U0 + r], 6 * nb, p.a.form ? PureShape<S>::sets(r) : SH::period4(r)});
  }
  if (p.a.form) {
    if (PureShape<S>::RU >= 0)
      for (uint32_t jl0 = 0; jl0 < 4; jl0++)
        for (uint32_t v = 0; v < 3; v++) d.utabs.push_back({0u, jl0, v, pi.u_off + (jl0 * 3 + v) * US});
  } else if (has_u && SH::RU >= 0) {
    for (int ru = 0; ru < SH::NRU; ru++) {
      if (t0 + SH::U0 + 2 * (SH::RU + ru) + 2 == k) continue;
      for (uint32_t jl0 = 0; jl0 < 4; jl0++)
        for (uint32_t v = 0; v < 3; v++) d.utabs.push_back({(uint32_t)ru, jl0, v, pi.u_off + (((uint32_t)ru * 4 + jl0) * 3 + v) * US});
    }
  }
}
void shape_coset(const NttStep& p, int N, PackShape& d) {
  const NttPackInfo& pi = p.pack_info;
  const uint32_t nb = pi.mul2 ? 2u : 1u, US = u_slot_words(N);
  for (uint32_t r = 2; r < 5; r++) d.slots.push_back({r, pi.round_off[r], 3 * nb, coset_sets((int)r)});
  for (uint32_t r = 0; r < 2; r++)
    for (uint32_t m = 0; m < coset_sets((int)r); m++)
      for (uint32_t v = 0; v < 3; v++) d.utabs.push_back({r, m, v, pi.u_off + ((r * 4 + m) * 3 + v) * US});
}
#define K1H_S_CASES(X) X(1) X(2) X(3) X(4) X(5) X(6) X(7) X(8) X(9) X(10)
// false: not a pass with a pack, or a shape the plan never builds
bool pack_shape(const lcpc_ctx* c, const NttStep& p, PackShape& d) {
  if (p.kernel == NttStep::GENERAL || !p.pack) return false;
  const int N = ntt_lns_limbs(c->NL);
  const bool has_u = N >= 5;
  d.n_classes = classes_of(p);
  if (p.a.form && c->NL != 8) return false;
  if (p.a.form && !p.first) {
    if (p.a.s != 10) return false;
    shape_coset(p, N, d);
  } else if (!p.first) {
    if (p.a.s != 10) return false;
    shape_dif<10, 0>(p, N, has_u, d);
  } else if (p.a.form) {
    switch (p.a.s) {
#define X(SV) case SV: shape_dif<SV, 0>(p, N, has_u, d); break;
      K1H_S_CASES(X)
#undef X
      default: return false;
    }
  } else {
    switch (p.a.s) {
#define X(SV) case SV: shape_dif<SV, 10 - SV>(p, N, has_u, d); break;
      K1H_S_CASES(X)
#undef X
      default: return false;
    }
  }
  // everything enumerated lies inside the class block (pack_get reaches nv * period * N words from the slot's start)
  const uint64_t cw = p.pack_info.class_words;
  for (const Slot& s : d.slots) {
    if (s.off % 4 || (uint64_t)s.off + (uint64_t)s.nv * s.period * N > cw) return false;
    d.records += (uint64_t)s.nv * s.period;
  }
  for (const UTab& u : d.utabs)
    if ((uint64_t)u.off + u_slot_words(N) > cw) return false;
  return cw % 4 == 0;
}

template <class FT> hipError_t launch_dump(const u32* pack, const Rec* recs, u32 n, u32* out, u32 rec_words) {
  hipLaunchKernelGGL((k1h_dump_kernel<FT>), dim3((n + 255) / 256), dim3(256), 0, nullptr, pack, recs, n, out, rec_words);
  return hipGetLastError();
}
hipError_t dump(int nl, const u32* pack, const Rec* recs, u32 n, u32* out, u32 rec_words) {
  switch (nl) {
    case 2: return launch_dump<LnField<FT63>>(pack, recs, n, out, rec_words);
    case 4: return launch_dump<LnField<FT127>>(pack, recs, n, out, rec_words);
    case 6: return launch_dump<LnField<FT191>>(pack, recs, n, out, rec_words);
    case 8: return launch_dump<LnField<FT255>>(pack, recs, n, out, rec_words);
  }
  return hipErrorInvalidValue;
}

// table numbers of k1h_table / k1h_tables
enum { T_ROOTS = 0, T_ROOTSL, T_ROOTSLC, T_ROOTSLS, T_ROOTSLCS, T_QPL, T_WQ_W, T_COUNT };
// -> device pointer (null: the context has no such table), entries, words per entry
const uint32_t* table_of(const lcpc_ctx* c, int which, uint64_t* entries, uint32_t* words) {
  const uint64_t half = (uint64_t)1 << (c->log_n ? c->log_n - 1 : 0);
  const uint32_t stride = (uint32_t)ntt_lns_stride(c->NL);
  const uint32_t* p = nullptr;
  switch (which) {
    case T_ROOTS: p = c->d_roots; *entries = half; *words = (uint32_t)c->NL; break;
    case T_ROOTSL: p = c->d_rootsl; *entries = half; *words = stride; break;
    case T_ROOTSLC: p = c->d_rootslc; *entries = half; *words = stride; break;
    case T_ROOTSLS: p = c->d_rootsls; *entries = (uint64_t)1 << 19; *words = stride; break;
    case T_ROOTSLCS: p = c->d_rootslcs; *entries = (uint64_t)1 << 19; *words = stride; break;
    case T_QPL: p = c->d_qpl; *entries = 64; *words = stride; break;
    case T_WQ_W: p = c->d_wq_w; *entries = 1; *words = 96; break;
    default: *entries = 0; *words = 0; break;
  }
  if (!p) *entries = 0;
  return p;
}
const lcpc_ctx* ctx_of(const void* h) {
  const lcpc_ctx* c = static_cast<const lcpc_ctx*>(h);
  return c && c->prm.encoding == LCPC_ENC_LIGERO ? c : nullptr;
}

}  // namespace

H_DEVICE_COUNT(k1h_)

// a Ligero context of `fid` with new_from_dims(n_per_row, n_cols) at rate rho_num / rho_den: the status of lcpc_ctx_create
H_EXPORT int k1h_open(uint32_t fid, uint64_t n_per_row, uint64_t n_cols, uint32_t rho_num, uint32_t rho_den, void** out) {
  if (!out) return K1H_BAD_ARGS;
  *out = nullptr;
  if (fid > 3 || !n_per_row || n_per_row >= n_cols || (n_cols & (n_cols - 1)) || n_cols > ((uint64_t)1 << 22)) return K1H_BAD_ARGS;
  lcpc_params prm{};
  prm.field = fid; prm.encoding = LCPC_ENC_LIGERO; prm.hash = LCPC_HASH_BLAKE3;
  prm.rho_num = rho_num; prm.rho_den = rho_den;
  prm.n_per_row = n_per_row; prm.n_cols = n_cols;
  lcpc_ctx* c = nullptr;
  const int rc = lcpc_ctx_create(&prm, &c);
  if (rc == 0) *out = c;
  return rc;
}
H_EXPORT void k1h_close(void* h) {
  if (h) lcpc_ctx_destroy(static_cast<lcpc_ctx*>(h));
}

// out[8]: NL, N, W, STRIDE, log_n, passes of the plan, comm_canon, U_SLOT words
H_EXPORT int k1h_info(const void* h, uint32_t* out, uint32_t out_words) {
  const lcpc_ctx* c = ctx_of(h);
  if (!c || !out || out_words < 8) return K1H_BAD_ARGS;
  const int N = ntt_lns_limbs(c->NL);
  out[0] = (uint32_t)c->NL; out[1] = (uint32_t)N; out[2] = (uint32_t)ntt_lns_limb_bits(c->NL); out[3] = (uint32_t)ntt_lns_stride(c->NL);
  out[4] = c->log_n; out[5] = (uint32_t)c->ntt.size(); out[6] = c->comm_canon ? 1u : 0u; out[7] = u_slot_words(N);
  return 0;
}
// out[7]: entries of d_roots, d_rootsl, d_rootslc, d_rootsls, d_rootslcs, d_qpl, d_wq_w (0: the context has no such table)
H_EXPORT int k1h_tables(const void* h, uint64_t* out, uint32_t out_words) {
  const lcpc_ctx* c = ctx_of(h);
  if (!c || !out || out_words < T_COUNT) return K1H_BAD_ARGS;
  for (int t = 0; t < T_COUNT; t++) {
    uint32_t w;
    (void)table_of(c, t, &out[t], &w);
  }
  return 0;
}
// one pass of the plan, out[24]: kind (0 general, 1 K1s, 2 K1n), first, log_n, t0, s, log_tj, form, round_off[8], class_words, u_off,
// mul2, tile classes (0: no pack), log_tile, lane-varying records per class, shifted-multiples tables per class, 0, 0
H_EXPORT int k1h_plan(const void* h, uint32_t pass, uint32_t* out, uint32_t out_words) {
  const lcpc_ctx* c = ctx_of(h);
  if (!c || !out || out_words < 24 || pass >= c->ntt.size()) return K1H_BAD_ARGS;
  const NttStep& p = c->ntt[pass];
  out[0] = p.kernel == NttStep::GENERAL ? 0u : (p.kernel == NttStep::K1S ? 1u : 2u);
  out[1] = p.first ? 1u : 0u;
  out[2] = p.a.log_n; out[3] = p.a.t0; out[4] = p.a.s; out[5] = p.a.log_tj; out[6] = p.a.form;
  for (int i = 0; i < 8; i++) out[7 + i] = p.pack_info.round_off[i];
  out[15] = p.pack_info.class_words; out[16] = p.pack_info.u_off; out[17] = p.pack_info.mul2;
  out[18] = classes_of(p);
  out[19] = (uint32_t)p.log_tile;
  PackShape d;
  const bool ok = pack_shape(c, p, d);
  if (p.kernel != NttStep::GENERAL && !ok) return K1H_BAD_ARGS;
  out[20] = (uint32_t)d.records; out[21] = (uint32_t)d.utabs.size(); out[22] = out[23] = 0;
  return 0;
}
// entries [first, first + count) of table `which` (0 d_roots, 1 d_rootsl, 2 d_rootslc, 3 d_rootsls, 4 d_rootslcs, 5 d_qpl, 6 d_wq_w) at
// their full stride, pad words included, into out
H_EXPORT int k1h_table(const void* h, int which, uint64_t first, uint64_t count, uint32_t* out, uint64_t out_words) {
  const lcpc_ctx* c = ctx_of(h);
  if (!c || !out || which < 0 || which >= T_COUNT) return K1H_BAD_ARGS;
  uint64_t entries;
  uint32_t words;
  const uint32_t* p = table_of(c, which, &entries, &words);
  if (!p || count == 0 || first >= entries || count > entries - first || count * words > out_words) return K1H_BAD_ARGS;
  K1H_TRY(hipSetDevice(c->prm.device));
  K1H_TRY(hipMemcpy(out, p + first * words, count * words * 4, hipMemcpyDeviceToHost));
  return 0;
}
// every lane-varying entry of pass `pass` for the classes listed: records (class, slot, variant, jl, N limbs), 4 + N words each, class
// by class in the order of the list, inside a class by slot, variant, jl.  out_words must hold n_cls x records-per-class of them
H_EXPORT int k1h_pack_entries(const void* h, uint32_t pass, const uint32_t* classes, uint32_t n_cls, uint32_t* out, uint64_t out_words) {
  const lcpc_ctx* c = ctx_of(h);
  if (!c || !classes || !out || !n_cls || pass >= c->ntt.size()) return K1H_BAD_ARGS;
  const NttStep& p = c->ntt[pass];
  PackShape d;
  if (!pack_shape(c, p, d)) return K1H_BAD_ARGS;
  const uint32_t N = (uint32_t)ntt_lns_limbs(c->NL), rw = 4 + N;
  const uint64_t total = d.records * n_cls;
  if (total == 0 || total > ((uint64_t)1 << 24) || total * rw > out_words) return K1H_BAD_ARGS;
  for (uint32_t i = 0; i < n_cls; i++)
    if (classes[i] >= d.n_classes) return K1H_BAD_ARGS;
  std::vector<Rec> recs;
  std::vector<uint32_t> head;                           // (class, slot, variant, jl) of each record
  recs.reserve(total);
  head.reserve(total * 4);
  for (uint32_t i = 0; i < n_cls; i++)
    for (const Slot& s : d.slots)
      for (uint32_t v = 0; v < s.nv; v++)
        for (uint32_t jl = 0; jl < s.period; jl++) {
          recs.push_back({(uint64_t)classes[i] * p.pack_info.class_words + s.off, s.period, v, jl, s.nv});
          head.insert(head.end(), {classes[i], s.slot, v, jl});
        }
  K1H_TRY(hipSetDevice(c->prm.device));
  DevBuf d_recs, d_out;
  K1H_TRY(d_recs.alloc(total * sizeof(Rec)));
  K1H_TRY(d_out.alloc(total * rw * 4));
  K1H_TRY(hipMemcpy(d_recs.p, recs.data(), total * sizeof(Rec), hipMemcpyHostToDevice));
  K1H_TRY(hipMemset(d_out.p, 0xA5, total * rw * 4));
  K1H_TRY(dump(c->NL, p.pack, reinterpret_cast<const Rec*>(d_recs.p), (u32)total, d_out.p, rw));
  K1H_TRY(hipDeviceSynchronize());
  K1H_TRY(hipMemcpy(out, d_out.p, total * rw * 4, hipMemcpyDeviceToHost));
  for (uint64_t i = 0; i < total; i++)
    for (int z = 0; z < 4; z++) out[i * rw + z] = head[i * 4 + z];
  return 0;
}
// every shifted-multiples table of pass `pass` for the classes listed: records (class, round, position, v, U_SLOT raw words), 4 +
// U_SLOT words each.  round: the uniform round's number among the pass's uniform rounds (DIF / K1n), 0 (pure) or the round r (coset);
// position: jl0 < 4, or the coset sub-block m
H_EXPORT int k1h_uniform(const void* h, uint32_t pass, const uint32_t* classes, uint32_t n_cls, uint32_t* out, uint64_t out_words) {
  const lcpc_ctx* c = ctx_of(h);
  if (!c || !classes || !out || !n_cls || pass >= c->ntt.size()) return K1H_BAD_ARGS;
  const NttStep& p = c->ntt[pass];
  PackShape d;
  if (!pack_shape(c, p, d) || d.utabs.empty()) return K1H_BAD_ARGS;
  const uint32_t US = u_slot_words(ntt_lns_limbs(c->NL)), rw = 4 + US;
  const uint64_t total = (uint64_t)d.utabs.size() * n_cls;
  if (total > ((uint64_t)1 << 20) || total * rw > out_words) return K1H_BAD_ARGS;
  for (uint32_t i = 0; i < n_cls; i++)
    if (classes[i] >= d.n_classes) return K1H_BAD_ARGS;
  K1H_TRY(hipSetDevice(c->prm.device));
  // the tables of a class are one run of words from the first table's offset to the last one's end
  uint32_t lo = d.utabs[0].off, hi = 0;
  for (const UTab& u : d.utabs) { lo = std::min(lo, u.off); hi = std::max(hi, u.off + US); }
  std::unique_ptr<uint32_t[]> run(new uint32_t[hi - lo]);
  uint64_t o = 0;
  for (uint32_t i = 0; i < n_cls; i++) {
    K1H_TRY(hipMemcpy(run.get(), p.pack + (size_t)classes[i] * p.pack_info.class_words + lo, (size_t)(hi - lo) * 4, hipMemcpyDeviceToHost));
    for (const UTab& u : d.utabs) {
      out[o] = classes[i]; out[o + 1] = u.round; out[o + 2] = u.pos; out[o + 3] = u.v;
      memcpy(out + o + 4, run.get() + (u.off - lo), (size_t)US * 4);
      o += rw;
    }
  }
  return 0;
}
H_EXPORT const char* k1h_last_error(const void* h) { return h ? lcpc_last_error(static_cast<const lcpc_ctx*>(h)) : ""; }

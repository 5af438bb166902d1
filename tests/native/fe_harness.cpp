// tests/native/fe_harness.cpp -- test-only C entry points over the device field primitives of lcpc_amd/csrc/field_dev.h (packed 32-bit
// words: fe_add / fe_sub / fe_mul / fe_canon / fe_reduce_once / wide_mac + wide_reduce) and lcpc_amd/csrc/field_ln.h (lazy signed limbs:
// ln::from_packed / to_packed / normalize / clamp_q + clamp_apply / mul / mul_u / lazy_*, and Ft255's ln::clamp, to_packed_reduced,
// fe_mul_r29, fe_canon_r29), so that a test can call each primitive once per lane on operands of its own making (tests/fe_harness.py,
// tests/test_gpu_fe_primitives.py), and over the host arithmetic of host_field.h (tests/test_host_field.py).  Built by
// lcpc_amd/csrc/Makefile into lcpc_amd/lib/liblcpc_fe_harness.so; it includes the product's headers, links the product library for
// field_desc() only, and the product gains nothing by it.
//
// One thin kernel per primitive: lane i loads operand(s) i, calls the primitive once, stores result i; blocks of 256 lanes.  Every
// wrapper takes HOST pointers, copies in, launches on the null stream, synchronises and copies the output buffers back whole (out_n >= n
// elements, so the caller sees what was written past element n - 1 too).  The return value is the first hipError_t, or H_BAD_ARGS for
// a call the harness refuses (nothing is launched then): a field or word count it has no instantiation for, a count out of range, or an
// operand whose table index (clamp_q, ln::clamp) would leave the 64-entry table.
#include "harness.h"
#include "../../lcpc_amd/csrc/field_ln.h"
#include "../../lcpc_amd/csrc/host_field.h"

using namespace lcpc;

namespace {

constexpr u32 MAX_N = 1u << 20;          // lanes per launch
constexpr u32 MAX_WIDE_K = 1u << 12;     // terms per lane of wide_dot (every caller reduces after 8)
constexpr u32 MAX_LAZY_K = 60;           // field_ln.h: one Montgomery reduction per <= 60 terms
constexpr u32 MAX_LAZY_C = 6;            //             a normalise at least every 6 terms
constexpr u32 WT_STRIDE = 96;            // words per shifted-multiples table (ctx.cpp wmul_table: N^2 <= 81 words, padded)

bool counts_ok(u32 n, u32 out_n) { return n <= MAX_N && out_n >= n && out_n <= MAX_N + 1; }
dim3 grid(u32 n) { return dim3((n + 255) / 256 ? (n + 255) / 256 : 1); }
__device__ __forceinline__ u32 lane_id() { return blockIdx.x * 256u + threadIdx.x; }

template <int N> __device__ __forceinline__ LN<N> limbs_get(const u32* p, size_t i) {
  LN<N> r;
#pragma unroll
  for (int k = 0; k < N; k++) r.v[k] = p[i * N + k];
  return r;
}
template <int N> __device__ __forceinline__ void limbs_put(u32* p, size_t i, const LN<N>& a) {
#pragma unroll
  for (int k = 0; k < N; k++) p[i * N + k] = a.v[k];
}

// ---- packed layer ---------------------------------------------------------------------------------------------------------------
enum { OP_ADD = 0, OP_SUB = 1, OP_MUL = 2, OP_CANON = 3 };

template <int NL, int OP> __global__ void __launch_bounds__(256) k_binop(const u32* a, const u32* b, u32* out, u32 n) {
  const u32 i = lane_id();
  if (i >= n) return;
  const Fe<NL> x = fe_load<NL>(a + (size_t)i * NL), y = fe_load<NL>(b + (size_t)i * NL);
  Fe<NL> r;
  if constexpr (OP == OP_ADD) r = fe_add<NL>(x, y);
  else if constexpr (OP == OP_SUB) r = fe_sub<NL>(x, y);
  else r = fe_mul<NL>(x, y);
  fe_store<NL>(out + (size_t)i * NL, r);
}
template <int NL> __global__ void __launch_bounds__(256) k_canon(const u32* a, u32* out, u32 n) {
  const u32 i = lane_id();
  if (i >= n) return;
  fe_store<NL>(out + (size_t)i * NL, fe_canon<NL>(fe_load<NL>(a + (size_t)i * NL)));
}
// top == nullptr: the one-argument form (Ft255: the carry chain)
template <int NL> __global__ void __launch_bounds__(256) k_reduce_once(const u32* t, const u32* top, u32* out, u32 n) {
  const u32 i = lane_id();
  if (i >= n) return;
  const Fe<NL> x = fe_load<NL>(t + (size_t)i * NL);
  const Fe<NL> r = top ? fe_reduce_once<NL>(x.v, top[i]) : fe_reduce_once<NL>(x.v);
  fe_store<NL>(out + (size_t)i * NL, r);
}
template <int NL> __global__ void __launch_bounds__(256) k_wide_dot(const u32* a, const u32* b, u32 k, u32* out, u32 n) {
  const u32 i = lane_id();
  if (i >= n) return;
  Wide<NL> w = wide_zero<NL>();
  for (u32 j = 0; j < k; j++) {
    const size_t e = (size_t)i * k + j;
    wide_mac<NL>(w, fe_load<NL>(a + e * NL), fe_load<NL>(b + e * NL));
  }
  fe_store<NL>(out + (size_t)i * NL, wide_reduce<NL>(w));
}

// ---- limb layer -----------------------------------------------------------------------------------------------------------------
template <class FT> __global__ void __launch_bounds__(256) k_from_packed(const u32* a, u32* out, u32 n) {
  const u32 i = lane_id();
  if (i >= n) return;
  limbs_put<FT::N>(out, i, ln::from_packed<FT>(fe_load<FT::NL>(a + (size_t)i * FT::NL)));
}
template <class FT> __global__ void __launch_bounds__(256) k_to_packed(const u32* l, u32* out, u32 n) {
  const u32 i = lane_id();
  if (i >= n) return;
  const LN<FT::N> x = limbs_get<FT::N>(l, i);
  Fe<FT::NL> r;
  ln::to_packed<FT>(r.v, x.v);
  fe_store<FT::NL>(out + (size_t)i * FT::NL, r);
}
template <class FT> __global__ void __launch_bounds__(256) k_normalize(const u32* l, u32* out, u32 n) {
  const u32 i = lane_id();
  if (i >= n) return;
  LN<FT::N> x = limbs_get<FT::N>(l, i);
  ln::normalize<FT>(x);
  limbs_put<FT::N>(out, i, x);
}
template <class FT> __global__ void __launch_bounds__(256) k_clamp_qa(const u32* l, const u32* nqp, u32* out, u32* q_out, u32 n) {
  const u32 i = lane_id();
  if (i >= n) return;
  LN<FT::N> x = limbs_get<FT::N>(l, i);
  const u32 q = ln::clamp_q<FT>(x.v[FT::N - 1]);
  ln::clamp_apply<FT>(x, ln::clamp_row<FT>(nqp, q));
  limbs_put<FT::N>(out, i, x);
  q_out[i] = q;
}
template <class FT> __global__ void __launch_bounds__(256) k_mul(const u32* a, const u32* w, u32* out, u32 n) {
  const u32 i = lane_id();
  if (i >= n) return;
  limbs_put<FT::N>(out, i, ln::mul<FT>(limbs_get<FT::N>(a, i), limbs_get<FT::N>(w, i)));
}
// the table is a scalar operand: every lane of block b multiplies by table b mod n_tabs
template <class FT> __global__ void __launch_bounds__(256) k_mul_u(const u32* a, const u32* wt, u32 n_tabs, u32* out, u32 n) {
  const u32 i = lane_id();
  if (i >= n) return;
  limbs_put<FT::N>(out, i, ln::mul_u<FT>(limbs_get<FT::N>(a, i), wt + (size_t)(blockIdx.x % n_tabs) * WT_STRIDE));
}
// x: packed elements (split by from_packed, as the kernels do), v: limbs
template <class FT> __global__ void __launch_bounds__(256) k_lazy_dot(const u32* x, const u32* v, u32 k, u32 c, u32* out, u32 n) {
  const u32 i = lane_id();
  if (i >= n) return;
  ln::LazyN<FT> acc;
  ln::lazy_zero<FT>(acc);
  u32 since = 0;
  for (u32 j = 0; j < k; j++) {
    const size_t e = (size_t)i * k + j;
    ln::lazy_mac<FT>(acc, ln::from_packed<FT>(fe_load<FT::NL>(x + e * FT::NL)), limbs_get<FT::N>(v, e));
    if (++since == c) { ln::lazy_normalize<FT>(acc); since = 0; }
  }
  fe_store<FT::NL>(out + (size_t)i * FT::NL, ln::lazy_reduce<FT>(acc));
}

// ---- Ft255 only -----------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) k_clamp9(const u32* l, const u32* qp, u32* out, u32 n) {
  const u32 i = lane_id();
  if (i >= n) return;
  LN<9> x = limbs_get<9>(l, i);
  ln::clamp(x, qp);
  limbs_put<9>(out, i, x);
}
__global__ void __launch_bounds__(256) k_to_packed_reduced(const u32* l, const u32* qp, u32* out, u32 n) {
  const u32 i = lane_id();
  if (i >= n) return;
  fe_store<8>(out + (size_t)i * 8, ln::to_packed_reduced(limbs_get<9>(l, i), qp));
}
__global__ void __launch_bounds__(256) k_mul_r29(const u32* a, const u32* b, u32* out, u32 n) {
  const u32 i = lane_id();
  if (i >= n) return;
  fe_store<8>(out + (size_t)i * 8, fe_mul_r29(fe_load<8>(a + (size_t)i * 8), limbs_get<9>(b, i)));
}
__global__ void __launch_bounds__(256) k_canon_r29(const u32* a, u32* out, u32 n) {
  const u32 i = lane_id();
  if (i >= n) return;
  fe_store<8>(out + (size_t)i * 8, fe_canon_r29(fe_load<8>(a + (size_t)i * 8)));
}

// the index clamp_q / ln::clamp form from a top limb stays inside the 64-entry table
template <class FT> bool tops_ok(const u32* l, u32 n) {
  constexpr u32 PTOP1 = FT::limb(FT::N - 1) + 1;
  for (u32 i = 0; i < n; i++)
    if (l[(size_t)i * FT::N + FT::N - 1] + (u32)(ln::QOFF * PTOP1 - ln::QBIAS) >= 64u * PTOP1) return false;
  return true;
}

// out (out_n elements of `ow` words) is copied in, written by `launch(d_out)`, and copied back whole
template <class F> int run_out(u32* out, u32 out_n, int ow, F launch) {
  DevBuf d_out;
  const size_t bytes = (size_t)out_n * ow * 4;
  H_TRY(d_out.put(out, bytes));
  launch(d_out.p);
  H_TRY(hipGetLastError());
  H_TRY(hipDeviceSynchronize());
  return (int)d_out.get(out, bytes);
}

#define FEH_NL_SWITCH(nl, BODY) \
  switch (nl) { \
    case 2: { constexpr int NLV = 2; BODY; } break; \
    case 4: { constexpr int NLV = 4; BODY; } break; \
    case 6: { constexpr int NLV = 6; BODY; } break; \
    case 8: { constexpr int NLV = 8; BODY; } break; \
    default: return H_BAD_ARGS; \
  }
#define FEH_FT_SWITCH(fid, BODY) \
  switch (fid) { \
    case FT63: { using FT = LnField<FT63>; BODY; } break; \
    case FT127: { using FT = LnField<FT127>; BODY; } break; \
    case FT191: { using FT = LnField<FT191>; BODY; } break; \
    case FT255: { using FT = LnField<FT255>; BODY; } break; \
    default: return H_BAD_ARGS; \
  }
// the fields with a shifted-multiples multiply and a limb dot product
#define FEH_FT_SWITCH3(fid, BODY) \
  switch (fid) { \
    case FT127: { using FT = LnField<FT127>; BODY; } break; \
    case FT191: { using FT = LnField<FT191>; BODY; } break; \
    case FT255: { using FT = LnField<FT255>; BODY; } break; \
    default: return H_BAD_ARGS; \
  }

template <int NL> int binop(int op, const u32* a, const u32* b, u32* out, u32 n, u32 out_n) {
  DevBuf d_a, d_b;
  H_TRY(d_a.put(a, (size_t)n * NL * 4));
  H_TRY(d_b.put(b, (size_t)n * NL * 4));
  return run_out(out, out_n, NL, [&](u32* d_out) {
    if (op == OP_ADD) hipLaunchKernelGGL((k_binop<NL, OP_ADD>), grid(n), dim3(256), 0, nullptr, d_a.p, d_b.p, d_out, n);
    else if (op == OP_SUB) hipLaunchKernelGGL((k_binop<NL, OP_SUB>), grid(n), dim3(256), 0, nullptr, d_a.p, d_b.p, d_out, n);
    else hipLaunchKernelGGL((k_binop<NL, OP_MUL>), grid(n), dim3(256), 0, nullptr, d_a.p, d_b.p, d_out, n);
  });
}

template <class FT> int lazy_dot(const u32* x, const u32* v, u32 k, u32 c, u32* out, u32 n, u32 out_n) {
  DevBuf d_x, d_v;
  H_TRY(d_x.put(x, (size_t)n * k * FT::NL * 4));
  H_TRY(d_v.put(v, (size_t)n * k * FT::N * 4));
  return run_out(out, out_n, FT::NL, [&](u32* d_out) {
    hipLaunchKernelGGL((k_lazy_dot<FT>), grid(n), dim3(256), 0, nullptr, d_x.p, d_v.p, k, c, d_out, n);
  });
}
template <class FT> int mul_u(const u32* a, const u32* wt, u32 n_tabs, u32* out, u32 n, u32 out_n) {
  DevBuf d_a, d_w;
  H_TRY(d_a.put(a, (size_t)n * FT::N * 4));
  H_TRY(d_w.put(wt, (size_t)n_tabs * WT_STRIDE * 4));
  return run_out(out, out_n, FT::N, [&](u32* d_out) {
    hipLaunchKernelGGL((k_mul_u<FT>), grid(n), dim3(256), 0, nullptr, d_a.p, d_w.p, n_tabs, d_out, n);
  });
}

}  // namespace

H_DEVICE_COUNT(feh_)

// ---- packed layer: elements are nl words ----------------------------------------------------------------------------------------
// op: 0 fe_add, 1 fe_sub, 2 fe_mul
H_EXPORT int feh_binop(int op, int nl, const u32* a, const u32* b, u32* out, u32 n, u32 out_n) {
  if (op < OP_ADD || op > OP_MUL || !counts_ok(n, out_n)) return H_BAD_ARGS;
  FEH_NL_SWITCH(nl, return binop<NLV>(op, a, b, out, n, out_n));
  return H_BAD_ARGS;
}
H_EXPORT int feh_canon(int nl, const u32* a, u32* out, u32 n, u32 out_n) {
  if (!nl_ok(nl) || !counts_ok(n, out_n)) return H_BAD_ARGS;
  DevBuf d_a;
  H_TRY(d_a.put(a, (size_t)n * nl * 4));
  FEH_NL_SWITCH(nl, return run_out(out, out_n, NLV, [&](u32* d_out) {
    hipLaunchKernelGGL((k_canon<NLV>), grid(n), dim3(256), 0, nullptr, d_a.p, d_out, n);
  }));
  return H_BAD_ARGS;
}
// top: n words for the (t, top) form, null for the one-argument form
H_EXPORT int feh_reduce_once(int nl, const u32* t, const u32* top, u32* out, u32 n, u32 out_n) {
  if (!nl_ok(nl) || !counts_ok(n, out_n)) return H_BAD_ARGS;
  DevBuf d_t, d_top;
  H_TRY(d_t.put(t, (size_t)n * nl * 4));
  if (top) H_TRY(d_top.put(top, (size_t)n * 4));
  FEH_NL_SWITCH(nl, return run_out(out, out_n, NLV, [&](u32* d_out) {
    hipLaunchKernelGGL((k_reduce_once<NLV>), grid(n), dim3(256), 0, nullptr, d_t.p, top ? d_top.p : nullptr, d_out, n);
  }));
  return H_BAD_ARGS;
}
// a, b: n * k elements, lane i takes pairs [i k, (i + 1) k): k wide_mac, one wide_reduce
H_EXPORT int feh_wide_dot(int nl, const u32* a, const u32* b, u32 k, u32* out, u32 n, u32 out_n) {
  if (!nl_ok(nl) || !counts_ok(n, out_n) || k > MAX_WIDE_K) return H_BAD_ARGS;
  DevBuf d_a, d_b;
  H_TRY(d_a.put(a, (size_t)n * k * nl * 4));
  H_TRY(d_b.put(b, (size_t)n * k * nl * 4));
  FEH_NL_SWITCH(nl, return run_out(out, out_n, NLV, [&](u32* d_out) {
    hipLaunchKernelGGL((k_wide_dot<NLV>), grid(n), dim3(256), 0, nullptr, d_a.p, d_b.p, k, d_out, n);
  }));
  return H_BAD_ARGS;
}

// ---- limb layer: fid selects LnField<fid>; a limb-form element is N words, a packed one NL ---------------------------------------
H_EXPORT int feh_from_packed(int fid, const u32* a, u32* out, u32 n, u32 out_n) {
  if (!counts_ok(n, out_n)) return H_BAD_ARGS;
  DevBuf d_a;
  FEH_FT_SWITCH(fid, {
    H_TRY(d_a.put(a, (size_t)n * FT::NL * 4));
    return run_out(out, out_n, FT::N, [&](u32* d_out) { hipLaunchKernelGGL((k_from_packed<FT>), grid(n), dim3(256), 0, nullptr, d_a.p, d_out, n); });
  });
  return H_BAD_ARGS;
}
H_EXPORT int feh_to_packed(int fid, const u32* l, u32* out, u32 n, u32 out_n) {
  if (!counts_ok(n, out_n)) return H_BAD_ARGS;
  DevBuf d_l;
  FEH_FT_SWITCH(fid, {
    H_TRY(d_l.put(l, (size_t)n * FT::N * 4));
    return run_out(out, out_n, FT::NL, [&](u32* d_out) { hipLaunchKernelGGL((k_to_packed<FT>), grid(n), dim3(256), 0, nullptr, d_l.p, d_out, n); });
  });
  return H_BAD_ARGS;
}
H_EXPORT int feh_normalize(int fid, const u32* l, u32* out, u32 n, u32 out_n) {
  if (!counts_ok(n, out_n)) return H_BAD_ARGS;
  DevBuf d_l;
  FEH_FT_SWITCH(fid, {
    H_TRY(d_l.put(l, (size_t)n * FT::N * 4));
    return run_out(out, out_n, FT::N, [&](u32* d_out) { hipLaunchKernelGGL((k_normalize<FT>), grid(n), dim3(256), 0, nullptr, d_l.p, d_out, n); });
  });
  return H_BAD_ARGS;
}
// clamp_q on the top limb, clamp_row from nqp (64 rows of STRIDE words: the limb-wise negated (i - QOFF) p table), clamp_apply; q_out
// (out_n words) receives clamp_q's index
H_EXPORT int feh_clamp_qa(int fid, const u32* l, const u32* nqp, u32* out, u32* q_out, u32 n, u32 out_n) {
  if (!counts_ok(n, out_n)) return H_BAD_ARGS;
  DevBuf d_l, d_t, d_q;
  FEH_FT_SWITCH(fid, {
    if (!tops_ok<FT>(l, n)) return H_BAD_ARGS;
    H_TRY(d_l.put(l, (size_t)n * FT::N * 4));
    H_TRY(d_t.put(nqp, (size_t)64 * FT::STRIDE * 4));
    H_TRY(d_q.put(q_out, (size_t)out_n * 4));
    const int rc = run_out(out, out_n, FT::N, [&](u32* d_out) {
      hipLaunchKernelGGL((k_clamp_qa<FT>), grid(n), dim3(256), 0, nullptr, d_l.p, d_t.p, d_out, d_q.p, n);
    });
    return rc ? rc : (int)d_q.get(q_out, (size_t)out_n * 4);
  });
  return H_BAD_ARGS;
}
H_EXPORT int feh_mul(int fid, const u32* a, const u32* w, u32* out, u32 n, u32 out_n) {
  if (!counts_ok(n, out_n)) return H_BAD_ARGS;
  DevBuf d_a, d_w;
  FEH_FT_SWITCH(fid, {
    H_TRY(d_a.put(a, (size_t)n * FT::N * 4));
    H_TRY(d_w.put(w, (size_t)n * FT::N * 4));
    return run_out(out, out_n, FT::N, [&](u32* d_out) { hipLaunchKernelGGL((k_mul<FT>), grid(n), dim3(256), 0, nullptr, d_a.p, d_w.p, d_out, n); });
  });
  return H_BAD_ARGS;
}
// wt: n_tabs tables of 96 words (the first N^2 used); the lanes of block b (256 lanes) multiply by table b mod n_tabs.  Ft127 / Ft191 /
// Ft255 (has_mul_u)
H_EXPORT int feh_mul_u(int fid, const u32* a, const u32* wt, u32 n_tabs, u32* out, u32 n, u32 out_n) {
  if (!counts_ok(n, out_n) || !n_tabs || n_tabs > 4096) return H_BAD_ARGS;
  FEH_FT_SWITCH3(fid, return mul_u<FT>(a, wt, n_tabs, out, n, out_n));
  return H_BAD_ARGS;
}
// x: n * k packed elements, v: n * k limb-form values; lane i takes pairs [i k, (i + 1) k): lazy_mac each, lazy_normalize every c terms,
// one lazy_reduce.  Ft127 / Ft191 / Ft255 (the fields whose kernels use it)
H_EXPORT int feh_lazy_dot(int fid, const u32* x, const u32* v, u32 k, u32 c, u32* out, u32 n, u32 out_n) {
  if (!counts_ok(n, out_n) || k > MAX_LAZY_K || !c || c > MAX_LAZY_C) return H_BAD_ARGS;
  FEH_FT_SWITCH3(fid, return lazy_dot<FT>(x, v, k, c, out, n, out_n));
  return H_BAD_ARGS;
}

// ---- Ft255 only: qp is the (i - QOFF) p table itself, 64 rows of 12 words ------------------------------------------------------------
// which: 0 ln::clamp (out: 9 words per element), 1 ln::to_packed_reduced (out: 8 words)
H_EXPORT int feh_clamp9(int which, const u32* l, const u32* qp, u32* out, u32 n, u32 out_n) {
  if (!counts_ok(n, out_n) || (which != 0 && which != 1) || !tops_ok<LnField<FT255>>(l, n)) return H_BAD_ARGS;
  DevBuf d_l, d_t;
  H_TRY(d_l.put(l, (size_t)n * 9 * 4));
  H_TRY(d_t.put(qp, (size_t)64 * 12 * 4));
  return run_out(out, out_n, which ? 8 : 9, [&](u32* d_out) {
    if (which) hipLaunchKernelGGL(k_to_packed_reduced, grid(n), dim3(256), 0, nullptr, d_l.p, d_t.p, d_out, n);
    else hipLaunchKernelGGL(k_clamp9, grid(n), dim3(256), 0, nullptr, d_l.p, d_t.p, d_out, n);
  });
}
// a: packed, b: 9 limbs
H_EXPORT int feh_mul_r29(const u32* a, const u32* b, u32* out, u32 n, u32 out_n) {
  if (!counts_ok(n, out_n)) return H_BAD_ARGS;
  DevBuf d_a, d_b;
  H_TRY(d_a.put(a, (size_t)n * 8 * 4));
  H_TRY(d_b.put(b, (size_t)n * 9 * 4));
  return run_out(out, out_n, 8, [&](u32* d_out) { hipLaunchKernelGGL(k_mul_r29, grid(n), dim3(256), 0, nullptr, d_a.p, d_b.p, d_out, n); });
}
H_EXPORT int feh_canon_r29(const u32* a, u32* out, u32 n, u32 out_n) {
  if (!counts_ok(n, out_n)) return H_BAD_ARGS;
  DevBuf d_a;
  H_TRY(d_a.put(a, (size_t)n * 8 * 4));
  return run_out(out, out_n, 8, [&](u32* d_out) { hipLaunchKernelGGL(k_canon_r29, grid(n), dim3(256), 0, nullptr, d_a.p, d_out, n); });
}

// ---- host_field.h: op 0 h_add, 1 h_sub, 2 h_mul, 3 h_canon (b unused) over n elements of L u64 limbs; no device involved -----------
H_EXPORT int feh_host_op(int op, int fid, const uint64_t* a, const uint64_t* b, uint64_t* out, uint64_t n) {
  const FieldDesc* f = field_desc(fid);
  if (!f || op < OP_ADD || op > OP_CANON) return H_BAD_ARGS;
  for (uint64_t i = 0; i < n; i++) {
    const uint64_t *x = a + i * f->L, *y = b ? b + i * f->L : nullptr;
    uint64_t* o = out + i * f->L;
    if (op == OP_CANON) h_canon(*f, o, x);
    else if (!y) return H_BAD_ARGS;
    else if (op == OP_ADD) h_add(*f, o, x, y);
    else if (op == OP_SUB) h_sub(*f, o, x, y);
    else h_mul(*f, o, x, y);
  }
  return 0;
}

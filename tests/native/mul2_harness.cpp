// tests/native/mul2_harness.cpp -- test-only C entry points over Ft255's two-table multiply of lcpc_amd/csrc/field_ln.h: ln::mul2 (the
// lane-varying twiddle multiply of K1s's split plans, ntt_l9s.hip) and ln::mul2_pair (what the pack kernels of ntt_lns.hip make of a
// table entry), one call per lane on operands of the test's making (tests/test_gpu_ntt_mul2.py).  Built by lcpc_amd/csrc/Makefile into
// lcpc_amd/lib/liblcpc_mul2_harness.so; it includes the product's header and links nothing of the product.
//
// Every wrapper takes HOST pointers to n elements of 9 words, copies in, launches on the null stream (blocks of 256 lanes, lanes >= n
// idle), synchronises and copies out_n >= n elements back.  Returns the first hipError_t, or H_BAD_ARGS for a count out of range.
#include "harness.h"
#include "../../lcpc_amd/csrc/field_ln.h"

using namespace lcpc;

namespace {

using FT = LnField<FT255>;
constexpr u32 MAX_N = 1u << 20;

__device__ __forceinline__ LN<9> limbs_get(const u32* p, size_t i) {
  LN<9> r;
#pragma unroll
  for (int k = 0; k < 9; k++) r.v[k] = p[i * 9 + k];
  return r;
}
__device__ __forceinline__ void limbs_put(u32* p, size_t i, const LN<9>& a) {
#pragma unroll
  for (int k = 0; k < 9; k++) p[i * 9 + k] = a.v[k];
}
__global__ void __launch_bounds__(256) k_mul2(const u32* x, const u32* b0, const u32* b1, u32* out, u32 n) {
  const u32 i = blockIdx.x * 256u + threadIdx.x;
  if (i >= n) return;
  limbs_put(out, i, ln::mul2<FT>(limbs_get(x, i), limbs_get(b0, i), limbs_get(b1, i)));
}
__global__ void __launch_bounds__(256) k_pair(const u32* e, u32* o0, u32* o1, u32 n) {
  const u32 i = blockIdx.x * 256u + threadIdx.x;
  if (i >= n) return;
  LN<9> b0, b1;
  ln::mul2_pair<FT>(limbs_get(e, i), b0, b1);
  limbs_put(o0, i, b0);
  limbs_put(o1, i, b1);
}
bool counts_ok(u32 n, u32 out_n) { return n <= MAX_N && out_n >= n && out_n <= MAX_N + 1; }
dim3 grid(u32 n) { return dim3((n + 255) / 256 ? (n + 255) / 256 : 1); }

}  // namespace

H_DEVICE_COUNT(m2h_)
// out[i] = ln::mul2(x[i], b0[i], b1[i]); out holds out_n elements, those past n - 1 come back as they went in
H_EXPORT int m2h_mul2(const u32* x, const u32* b0, const u32* b1, u32* out, u32 n, u32 out_n) {
  if (!counts_ok(n, out_n)) return H_BAD_ARGS;
  DevBuf d_x, d_0, d_1, d_o;
  H_TRY(d_x.put(x, (size_t)n * 36));
  H_TRY(d_0.put(b0, (size_t)n * 36));
  H_TRY(d_1.put(b1, (size_t)n * 36));
  H_TRY(d_o.put(out, (size_t)out_n * 36));
  hipLaunchKernelGGL(k_mul2, grid(n), dim3(256), 0, nullptr, d_x.p, d_0.p, d_1.p, d_o.p, n);
  H_TRY(hipGetLastError());
  H_TRY(hipDeviceSynchronize());
  return (int)d_o.get(out, (size_t)out_n * 36);
}
// (o0[i], o1[i]) = ln::mul2_pair(e[i])
H_EXPORT int m2h_pair(const u32* e, u32* o0, u32* o1, u32 n, u32 out_n) {
  if (!counts_ok(n, out_n)) return H_BAD_ARGS;
  DevBuf d_e, d_0, d_1;
  H_TRY(d_e.put(e, (size_t)n * 36));
  H_TRY(d_0.put(o0, (size_t)out_n * 36));
  H_TRY(d_1.put(o1, (size_t)out_n * 36));
  hipLaunchKernelGGL(k_pair, grid(n), dim3(256), 0, nullptr, d_e.p, d_0.p, d_1.p, n);
  H_TRY(hipGetLastError());
  H_TRY(hipDeviceSynchronize());
  H_TRY(d_0.get(o0, (size_t)out_n * 36));
  return (int)d_1.get(o1, (size_t)out_n * 36);
}

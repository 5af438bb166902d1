// lcpc_amd/csrc/eval.hip -- K10: tensors of an opening from a point; K11: field dot product (include/lcpc_hip_eval.h).
//
// K10 runs in two steps.  Every basis of the header is one formula, out[i] = product over k of (bit k of idx ? hi_k : lo_k) with
// idx = i * stride (stride 1 for the inner tensor, n_per_row for the outer one).  The pair kernel, one lane per point, writes the
// K pairs (lo_k, hi_k) of its point -- for the powers basis the chain of squarings x^(2^k), K covering every bit of the largest
// idx, which may need more than 32 of them.  The expansion kernel runs one output element per lane (64-bit index, no grid-stride
// loop: no element count takes a path of its own) with the point as the grid's second dimension.  A lane multiplies the selected
// factors of its index; where lo_k is 1 (powers, monomial) a clear bit costs nothing and the loop ends with the index's top bit.
// Bits above the sixth are uniform across a wave, so most of the branches on them are not divergent.  Every output is a product of
// fully reduced elements by fe_mul, so it is fully reduced: the Ft255 collapse converts the tensors with launch_to_r29 and relies
// on that.  What bounds it: the multiplier for short tensors with many bits (at most 64 fe_mul per element), the store otherwise.
//
// K11: workgroups of 256 lanes.  Lanes stride over their range of n, multiply with the full Montgomery multiply and add mod p, so
// every partial sum is a fully reduced element; the sums of a wave's lanes are folded by shuffles with fe_add, the four waves'
// through LDS.  Lanes past the end hold zero, so every n is exact.  One workgroup per pair is bound by its own chain of n / 256
// dependent multiply-adds per lane -- measured 753 us for one pair of 131072 Ft255 elements, twice the collapse in front of it
// (profiles/r16_eval.jsonl) -- so from 4096 elements on a pair is cut into chunks of at least 2048 elements (at most 256 chunks,
// at most 4096 workgroups in all), each chunk's sum goes to `parts`, and the split sum of the collapse (launch_field_sum) adds them.
#include "kernels.h"
#include "field_dev.h"

namespace lcpc {

namespace {

template <int NL>
__global__ void __launch_bounds__(64) eval_pairs_kernel(const u32* points, u32 n_point, u32 n_points, int basis, u32 n_bits, Fe<NL> one,
                                                        u32* tab) {
  const u32 t = blockIdx.x * 64 + threadIdx.x;
  if (t >= n_points) return;
  const u32* z = points + (u64)t * n_point * NL;
  u32* o = tab + (u64)t * n_bits * 2 * NL;
  if (basis == EVAL_POWERS) {
    Fe<NL> h = fe_load<NL>(z);
    for (u32 k = 0; k < n_bits; k++) {
      fe_store<NL>(o + (u64)(2 * k) * NL, one);
      fe_store<NL>(o + (u64)(2 * k + 1) * NL, h);
      h = fe_mul<NL>(h, h);
    }
  } else {
    for (u32 k = 0; k < n_bits; k++) {
      const Fe<NL> zk = fe_load<NL>(z + (u64)k * NL);
      fe_store<NL>(o + (u64)(2 * k) * NL, basis == EVAL_ML_LAGRANGE ? fe_sub<NL>(one, zk) : one);
      fe_store<NL>(o + (u64)(2 * k + 1) * NL, zk);
    }
  }
}

// LO: lo_k is not 1 (the Lagrange basis): every bit selects a factor
template <int NL, bool LO>
__global__ void __launch_bounds__(256) eval_expand_kernel(const u32* tab, u32 tab_bits, u32 n_bits, u64 n, u64 stride, Fe<NL> one, u32* out) {
  const u64 i = (u64)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const u32 t = blockIdx.y;
  const u32* tb = tab + (u64)t * tab_bits * 2 * NL;
  const u64 idx = i * stride;
  Fe<NL> acc = one;
  if constexpr (LO) {
    for (u32 k = 0; k < n_bits; k++) {
      const u32 bit = (u32)(idx >> k) & 1u;
      acc = fe_mul<NL>(acc, fe_load<NL>(tb + (u64)(2 * k + bit) * NL));
    }
  } else {
    for (u32 k = 0; k < n_bits && (idx >> k) != 0; k++)
      if ((idx >> k) & 1u) acc = fe_mul<NL>(acc, fe_load<NL>(tb + (u64)(2 * k + 1) * NL));
  }
  fe_store<NL>(out + ((u64)t * n + i) * NL, acc);
}

// chunk blockIdx.x of pair blockIdx.y: elements [c * chunk, min(n, (c + 1) * chunk)) -> out[(c * n_pairs + t)] (one chunk: out[t])
template <int NL>
__global__ void __launch_bounds__(256) field_dot_kernel(const u32* a, u64 a_stride, const u32* b, u64 b_stride, u64 n, u64 chunk, u32* out) {
  __shared__ u32 red[4][NL];
  const u32 c = blockIdx.x, t = blockIdx.y;
  const u32* pa = a + (u64)t * a_stride * NL;
  const u32* pb = b + (u64)t * b_stride * NL;
  const u64 i0 = (u64)c * chunk, i1 = i0 + chunk < n ? i0 + chunk : n;
  Fe<NL> acc = fe_zero<NL>();
  for (u64 i = i0 + threadIdx.x; i < i1; i += 256) acc = fe_add<NL>(acc, fe_mul<NL>(fe_load<NL>(pa + i * NL), fe_load<NL>(pb + i * NL)));
  // lane l takes lane l + off: after the last step lane 0 of a wave holds the sum of its 64 lanes (what the upper lanes hold is unused)
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) {
    Fe<NL> o;
#pragma unroll
    for (int l = 0; l < NL; l++) o.v[l] = __shfl_down(acc.v[l], off, 64);
    acc = fe_add<NL>(acc, o);
  }
  const u32 lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  if (lane == 0) {
#pragma unroll
    for (int l = 0; l < NL; l++) red[w][l] = acc.v[l];
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int ww = 1; ww < 4; ww++) {
      Fe<NL> o;
#pragma unroll
      for (int l = 0; l < NL; l++) o.v[l] = red[ww][l];
      acc = fe_add<NL>(acc, o);
    }
    fe_store<NL>(out + ((u64)c * gridDim.y + t) * NL, acc);
  }
}

template <int NL> Fe<NL> fe_arg(const u32* w) {
  Fe<NL> r;
  for (int i = 0; i < NL; i++) r.v[i] = w[i];
  return r;
}

template <int NL>
void pairs_nl(const u32* points, u32 n_point, u32 n_points, int basis, u32 n_bits, const u32* one, u32* tab, hipStream_t st) {
  hipLaunchKernelGGL((eval_pairs_kernel<NL>), dim3((n_points + 63) / 64), dim3(64), 0, st, points, n_point, n_points, basis, n_bits,
                     fe_arg<NL>(one), tab);
}
template <int NL>
void expand_nl(const u32* tab, u32 tab_bits, u32 n_bits, bool lo, u64 n, u64 stride, u32 n_points, const u32* one, u32* out, hipStream_t st) {
  const dim3 grid((unsigned)((n + 255) / 256), n_points);
  if (lo) hipLaunchKernelGGL((eval_expand_kernel<NL, true>), grid, dim3(256), 0, st, tab, tab_bits, n_bits, n, stride, fe_arg<NL>(one), out);
  else hipLaunchKernelGGL((eval_expand_kernel<NL, false>), grid, dim3(256), 0, st, tab, tab_bits, n_bits, n, stride, fe_arg<NL>(one), out);
}

}  // namespace

hipError_t launch_eval_pairs(int nl, int basis, const uint32_t* points, uint32_t n_point, uint32_t n_points, uint32_t n_bits,
                             const uint32_t* one, uint32_t* tab, hipStream_t st) {
  if (n_points == 0 || n_bits == 0) return hipSuccess;
  if (!nl_ok(nl) || basis < EVAL_POWERS || basis > EVAL_ML_LAGRANGE || n_bits > 64 || !points || !one || !tab) return hipErrorInvalidValue;
  if (basis == EVAL_POWERS ? n_point != 1 : n_point < n_bits) return hipErrorInvalidValue;      // (the lanes read n_bits variables)
  if (!elem_aligned(points, nl) || !elem_aligned(tab, nl)) return hipErrorInvalidValue;
  switch (nl) {
    case 2: pairs_nl<2>(points, n_point, n_points, basis, n_bits, one, tab, st); break;
    case 4: pairs_nl<4>(points, n_point, n_points, basis, n_bits, one, tab, st); break;
    case 6: pairs_nl<6>(points, n_point, n_points, basis, n_bits, one, tab, st); break;
    default: pairs_nl<8>(points, n_point, n_points, basis, n_bits, one, tab, st); break;
  }
  return hipGetLastError();
}

hipError_t launch_eval_expand(int nl, int basis, const uint32_t* tab, uint32_t tab_bits, uint32_t n_bits, uint64_t n, uint64_t stride, uint32_t n_points,
                              const uint32_t* one, uint32_t* out, hipStream_t st) {
  if (n == 0 || n_points == 0) return hipSuccess;
  if (!nl_ok(nl) || basis < EVAL_POWERS || basis > EVAL_ML_LAGRANGE || n_bits > 64 || n_bits > tab_bits || n_points > 65535 || !one || !out || (n_bits && !tab))
    return hipErrorInvalidValue;
  if (!elem_aligned(out, nl) || (n_bits && !elem_aligned(tab, nl))) return hipErrorInvalidValue;
  if ((n + 255) / 256 > 0x7fffffffu) return hipErrorInvalidValue;                                // grid.x
  if (stride == 0 || (n - 1) > ~(uint64_t)0 / stride) return hipErrorInvalidValue;               // the largest index fits 64 bits
  if (n_bits < 64 && (((n - 1) * stride) >> n_bits) != 0) return hipErrorInvalidValue;           // ... and the table covers its bits
  const bool lo = basis == EVAL_ML_LAGRANGE;
  switch (nl) {
    case 2: expand_nl<2>(tab, tab_bits, n_bits, lo, n, stride, n_points, one, out, st); break;
    case 4: expand_nl<4>(tab, tab_bits, n_bits, lo, n, stride, n_points, one, out, st); break;
    case 6: expand_nl<6>(tab, tab_bits, n_bits, lo, n, stride, n_points, one, out, st); break;
    default: expand_nl<8>(tab, tab_bits, n_bits, lo, n, stride, n_points, one, out, st); break;
  }
  return hipGetLastError();
}

uint32_t field_dot_chunks(uint64_t n, uint32_t n_pairs) {
  uint64_t c = n / 2048;                                   // at least 8 elements per lane and chunk
  if (c > 256) c = 256;
  if (n_pairs && c > 4096 / n_pairs) c = 4096 / n_pairs;   // (enough workgroups without them)
  return c < 2 ? 1u : (uint32_t)c;
}

hipError_t launch_field_dot(int nl, const uint32_t* a, uint64_t a_stride, const uint32_t* b, uint64_t b_stride, uint64_t n,
                            uint32_t n_pairs, uint32_t* out, uint32_t* parts, hipStream_t st) {
  if (n_pairs == 0) return hipSuccess;
  if (!nl_ok(nl) || n_pairs > 65535 || !out || (n && (!a || !b))) return hipErrorInvalidValue;
  if (!elem_aligned(out, nl) || !elem_aligned(a, nl) || !elem_aligned(b, nl) || !elem_aligned(parts, nl)) return hipErrorInvalidValue;
  const uint32_t n_chunks = parts ? field_dot_chunks(n, n_pairs) : 1;
  const uint64_t chunk = n_chunks > 1 ? (n + n_chunks - 1) / n_chunks : n;
  uint32_t* dst = n_chunks > 1 ? parts : out;
  const dim3 grid(n_chunks, n_pairs);
  switch (nl) {
    case 2: hipLaunchKernelGGL((field_dot_kernel<2>), grid, dim3(256), 0, st, a, a_stride, b, b_stride, n, chunk, dst); break;
    case 4: hipLaunchKernelGGL((field_dot_kernel<4>), grid, dim3(256), 0, st, a, a_stride, b, b_stride, n, chunk, dst); break;
    case 6: hipLaunchKernelGGL((field_dot_kernel<6>), grid, dim3(256), 0, st, a, a_stride, b, b_stride, n, chunk, dst); break;
    default: hipLaunchKernelGGL((field_dot_kernel<8>), grid, dim3(256), 0, st, a, a_stride, b, b_stride, n, chunk, dst); break;
  }
  hipError_t e = hipGetLastError();
  if (e != hipSuccess || n_chunks == 1) return e;
  return launch_field_sum(nl, parts, n_chunks, n_pairs, out, st);
}

}  // namespace lcpc

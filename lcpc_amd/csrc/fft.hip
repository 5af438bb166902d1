// lcpc_amd/csrc/fft.hip -- K12: one pass of a whole-vector transform; K13: the bit-reversal permutation (include/lcpc_hip_fft.h).
//
// A transform of n = 2^log_n points is cut into passes by fft_plan.  Pass (t0, s) works on the sub-transforms of 2^(log_n - t0)
// points that the passes before it left behind: with r = log_n - t0 - s an element's index is (top, m, low) -- t0 + vector bits,
// s bits, r bits -- and the pass runs the 2^s-point transform over m for every (top, low), a "column".  In decimation in frequency
// (natural in, bit-reversed out) that is s radix-2 stages (a + b, (a - b) v^e) with the twiddles of the 2^s-point transform alone,
// followed by ONE multiplication per element with the twist v^((low * rev_s(m)) << t0); the last pass (r == 0) has no twist.
// Decimation in time (bit-reversed in, natural out) is the same network backwards: the passes from the last to the first, in each the
// twist first and then the stages (a + b v^e, a - b v^e) from the shortest distance to the longest.  Every pass reads and writes the
// same places, so a transform runs in place; the first pass may read another buffer.  The inverse forms run the same passes with
// v = w^-1 and multiply by n^-1 in the store of the last pass.
//
// A workgroup holds 2^log_c columns, 2^(s + log_c) elements, in LDS, one 32-bit limb plane after the other (lanes that walk
// consecutive elements hit consecutive banks).  Adjacent columns are adjacent in memory: a global access of the workgroup is a run
// of min(2^log_c, 2^r) * (r < log_c ? 2^s : 1) contiguous elements per row, never one lane per stride.  The vector index and the t0
// top bits are one number (vectors lie n apart), so n_vecs only lengthens the column list; columns past its end are masked.
// Twiddles: the 2^(s-1) twiddles of the 2^s-point transform are built in LDS by every workgroup from the two-level table
// (one multiplication each), the twist is one more product of two table entries.  All arithmetic is field_dev.h's fe_mul / fe_add /
// fe_sub on fully reduced elements, so every intermediate and every stored element is fully reduced.  All element indices are 64-bit.
//
// The pass's arguments, LDS layout and table look-up are fft_dev.h's, which K14 (domain.hip) shares.
//
// K13: out[rev(i)] = in[i], one element per lane; in place it swaps the pairs i < rev(i).  One side of it is scattered.
#include "fft_dev.h"

namespace lcpc {

namespace {

template <int NL>
__global__ void __launch_bounds__(1024) fft_pass_kernel(FftPass a, Fe<NL> n_inv) {
  extern __shared__ __attribute__((aligned(16))) u32 lds[];
  const u32 s = a.s, r = a.log_n - a.t0 - a.s, lc = a.log_c;
  const u32 rows = 1u << s, T = rows << lc, half = rows >> 1;
  u32* tile = lds;                       // [NL][T], element (m, col) at tile_at(m, col, lc)
  u32* tw = lds + (size_t)NL * T;        // [NL][half]: v^(i << (log_n - s))
  const u32 tid = threadIdx.x, nt = blockDim.x;
  const u64 q0 = (u64)blockIdx.x << lc;
  // how a tile element number e is read as (column, row) for the global accesses: the low min(lc, r) column bits vary fastest, then
  // the row, then the remaining column bits -- consecutive lanes take consecutive addresses as far as the layout has them
  const u32 lcl = lc < r ? lc : r;
  const u64 low_mask = ((u64)1 << r) - 1;

  for (u32 i = tid; i < half; i += nt) lds_put<NL>(tw, half, i, tab_pow<NL>(a.tab, a.h, (u64)i << (a.log_n - s)));

  for (u32 e = tid; e < T; e += nt) {
    const u32 cl = e & ((1u << lcl) - 1), m = (e >> lcl) & (rows - 1), ct = e >> (lcl + s);
    const u32 col = (ct << lcl) | cl;
    const u64 q = q0 + col;
    if (q < a.n_cols) {
      const u64 top = q >> r, low = q & low_mask;
      const u64 g = (top << (s + r)) + ((u64)m << r) + low;
      Fe<NL> v = fe_load<NL>(a.src + g * NL);
      if (a.dit && r) v = fe_mul<NL>(v, tab_pow<NL>(a.tab, a.h, (low * (u64)(__brev(m) >> (32 - s))) << a.t0));
      lds_put<NL>(tile, T, tile_at(m, col, lc), v);
    }
  }
  __syncthreads();

  for (u32 k = 0; k < s; k++) {
    const u32 u = a.dit ? s - 1 - k : k;         // stage u pairs rows 2^(s - 1 - u) apart
    const u32 lhw = s - 1 - u;
    for (u32 b = tid; b < (T >> 1); b += nt) {
      const u32 col = b & ((1u << lc) - 1), pb = b >> lc;
      const u32 jl = pb & ((1u << lhw) - 1);
      const u32 i0 = ((pb >> lhw) << (lhw + 1)) | jl;
      const u32 e0 = tile_at(i0, col, lc), e1 = tile_at(i0 + (1u << lhw), col, lc);
      const Fe<NL> x = lds_get<NL>(tile, T, e0);
      Fe<NL> y = lds_get<NL>(tile, T, e1);
      if (lhw == 0) {                            // neighbouring rows: every twiddle of the stage is v^0 (uniform: no multiply)
        lds_put<NL>(tile, T, e0, fe_add<NL>(x, y));
        lds_put<NL>(tile, T, e1, fe_sub<NL>(x, y));
      } else if (a.dit) {
        y = fe_mul<NL>(y, lds_get<NL>(tw, half, jl << u));
        lds_put<NL>(tile, T, e0, fe_add<NL>(x, y));
        lds_put<NL>(tile, T, e1, fe_sub<NL>(x, y));
      } else {
        lds_put<NL>(tile, T, e0, fe_add<NL>(x, y));
        lds_put<NL>(tile, T, e1, fe_mul<NL>(fe_sub<NL>(x, y), lds_get<NL>(tw, half, jl << u)));
      }
    }
    __syncthreads();
  }

  for (u32 e = tid; e < T; e += nt) {
    const u32 cl = e & ((1u << lcl) - 1), m = (e >> lcl) & (rows - 1), ct = e >> (lcl + s);
    const u32 col = (ct << lcl) | cl;
    const u64 q = q0 + col;
    if (q < a.n_cols) {
      const u64 top = q >> r, low = q & low_mask;
      const u64 g = (top << (s + r)) + ((u64)m << r) + low;
      Fe<NL> v = lds_get<NL>(tile, T, tile_at(m, col, lc));
      if (!a.dit && r) v = fe_mul<NL>(v, tab_pow<NL>(a.tab, a.h, (low * (u64)(__brev(m) >> (32 - s))) << a.t0));
      if (a.scale) v = fe_mul<NL>(v, n_inv);
      fe_store<NL>(a.dst + g * NL, v);
    }
  }
}

// total = n_vecs << log_n elements, log_n >= 1
template <int NL>
__global__ void __launch_bounds__(256) fft_bitrev_kernel(const u32* in, u32* out, u32 log_n, u64 total) {
  const u64 g = (u64)blockIdx.x * 256 + threadIdx.x;
  if (g >= total) return;
  const u64 i = g & (((u64)1 << log_n) - 1);
  const u64 j = __brevll(i) >> (64 - log_n);
  const u64 gj = g - i + j;
  if (in != out) {
    fe_store<NL>(out + gj * NL, fe_load<NL>(in + g * NL));
  } else if (i < j) {
    const Fe<NL> x = fe_load<NL>(in + g * NL), y = fe_load<NL>(in + gj * NL);
    fe_store<NL>(out + g * NL, y);
    fe_store<NL>(out + gj * NL, x);
  }
}

template <int NL>
hipError_t pass_nl(const FftPass& a, const u32* n_inv, hipStream_t st) {
  const size_t lds_bytes = pass_lds_bytes(NL, a);
  const uint64_t blocks = pass_blocks(a);
  const unsigned nt = pass_lanes(a);
  // (idempotent and cheap; set on every launch rather than cached in an unsynchronised static)
  hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(&fft_pass_kernel<NL>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_bytes);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL((fft_pass_kernel<NL>), dim3((unsigned)blocks), dim3(nt), lds_bytes, st, a, fe_arg<NL>(n_inv));
  return hipGetLastError();
}

hipError_t pass_any(int nl, const FftPass& a, const u32* n_inv, hipStream_t st) {
  switch (nl) {
    case 2: return pass_nl<2>(a, n_inv, st);
    case 4: return pass_nl<4>(a, n_inv, st);
    case 6: return pass_nl<6>(a, n_inv, st);
    default: return pass_nl<8>(a, n_inv, st);
  }
}

hipError_t bitrev_any(int nl, const u32* in, u32* out, u32 log_n, u64 total, hipStream_t st) {
  const dim3 grid((unsigned)((total + 255) / 256));
  switch (nl) {
    case 2: hipLaunchKernelGGL((fft_bitrev_kernel<2>), grid, dim3(256), 0, st, in, out, log_n, total); break;
    case 4: hipLaunchKernelGGL((fft_bitrev_kernel<4>), grid, dim3(256), 0, st, in, out, log_n, total); break;
    case 6: hipLaunchKernelGGL((fft_bitrev_kernel<6>), grid, dim3(256), 0, st, in, out, log_n, total); break;
    default: hipLaunchKernelGGL((fft_bitrev_kernel<8>), grid, dim3(256), 0, st, in, out, log_n, total); break;
  }
  return hipGetLastError();
}

}  // namespace

hipError_t launch_fft_bitrev(int nl, const uint32_t* in, uint32_t* out, uint32_t log_n, uint64_t total, hipStream_t st) {
  if (!nl_ok(nl) || !in || !out || !elem_aligned(in, nl) || !elem_aligned(out, nl) || log_n == 0 || log_n > FFT_MAX_LOG_N) return hipErrorInvalidValue;
  if (total == 0 || total >= ((uint64_t)1 << 39) || (total & (((uint64_t)1 << log_n) - 1))) return hipErrorInvalidValue;
  return bitrev_any(nl, in, out, log_n, total, st);
}

int fft_plan(uint32_t log_n, uint32_t log_tile, uint32_t s[]) {
  if (log_tile == 0 || log_tile > FFT_MAX_LOG_TILE || log_n > FFT_MAX_LOG_N) return -1;
  int n = 0;
  for (uint32_t left = log_n; left; n++) {
    s[n] = left < log_tile ? left : log_tile;
    left -= s[n];
  }
  return n;
}

hipError_t launch_fft(int nl, int form, uint32_t log_n, uint32_t log_tile, uint32_t n_vecs, const uint32_t* in, uint32_t* out,
                      const uint32_t* tab, const uint32_t* n_inv, hipStream_t st, uint32_t* n_launches) {
  uint32_t s[FFT_MAX_PASSES];
  const int n_pass = fft_plan(log_n, log_tile, s);
  const bool inverse = form >= FFT_IFFT_II;
  if (!nl_ok(nl) || form < FFT_FFT_II || form > FFT_IFFT_OI || n_pass < 0 || n_vecs == 0 || n_vecs > 65535) return hipErrorInvalidValue;
  if (!in || !out || !elem_aligned(in, nl) || !elem_aligned(out, nl)) return hipErrorInvalidValue;
  if (log_n && (!tab || !elem_aligned(tab, nl) || (inverse && !n_inv))) return hipErrorInvalidValue;
  const uint64_t total = (uint64_t)n_vecs << log_n;                 // (n_vecs < 2^16, log_n <= 32: no overflow)
  if (total >= ((uint64_t)1 << 39)) return hipErrorInvalidValue;    // K13's grid; a pass has at most total / 2 columns, 2^31 workgroups
  if (n_launches) *n_launches = 0;
  if (log_n == 0) {
    if (in == out) return hipSuccess;
    return hipMemcpyAsync(out, in, (size_t)total * nl * 4, hipMemcpyDeviceToDevice, st);
  }
  const bool ii = form == FFT_FFT_II || form == FFT_IFFT_II;
  const bool dit = ii || form == FFT_FFT_OI || form == FFT_IFFT_OI;
  uint32_t launches = 0;
  const uint32_t* src = in;
  if (ii) {
    hipError_t e = bitrev_any(nl, in, out, log_n, total, st);
    if (e != hipSuccess) return e;
    launches++;
    src = out;
  }
  uint32_t t0s[FFT_MAX_PASSES], t0 = 0;
  for (int p = 0; p < n_pass; p++) { t0s[p] = t0; t0 += s[p]; }
  for (int k = 0; k < n_pass; k++) {
    const int p = dit ? n_pass - 1 - k : k;
    FftPass a;
    a.src = src; a.dst = out; a.tab = tab;
    a.log_n = log_n; a.t0 = t0s[p]; a.s = s[p]; a.h = fft_tab_split(log_n);
    a.log_c = log_cols(nl, s[p]);
    a.n_cols = (uint64_t)n_vecs << (log_n - s[p]);
    a.dit = dit; a.scale = inverse && k == n_pass - 1;
    hipError_t e = pass_any(nl, a, n_inv, st);
    if (e != hipSuccess) return e;
    launches++;
    src = out;
  }
  if (n_launches) *n_launches = launches;
  return hipSuccess;
}

}  // namespace lcpc

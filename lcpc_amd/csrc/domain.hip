// lcpc_amd/csrc/domain.hip -- K14: the passes of a coset transform and of the low-degree extension (include/lcpc_hip_domain.h).
//
// A coset transform is the plain transform of x[j] s^j (forward) or the plain inverse followed by s^-j (inverse).  K14 is K12's pass
// (described in fft.hip) with that scale fused into the one pass that touches the data first or last: the pass that loads
// the input of a forward transform multiplies every element by s^j on its way into LDS, the pass that stores the output of an inverse
// multiplies by s^-j n^-1 on the way out.  j is the element's natural index whatever order it is stored in, and the power comes from a
// two-level table of the shift, as the twiddles do.  The transform therefore takes the launches of the plain one: no pass over
// memory scales.
//
// The extension Y[k] = sum_{j < n_coeffs} x[j] s^j w_m^(jk), k < m = 2^b n, never pads.  The first b stages of a decimation-in-
// frequency transform of the zero-padded input only copy and twist; what they leave are 2^b transforms of length n of the same
// coefficients: block c of the bit-reversed output is FFT_IO of x[j] (s w_m^rev_b(c))^j.  So the launcher runs the n-point plan on
// n_vecs 2^b output vectors; the loading pass reads vector V's input from source vector V >> b (zero from n_coeffs on) and scales by
// the block's own shift, and every pass takes its twiddles from the table of m points (w_n = w_m^(2^b)).  The natural order is K13 in
// place on the output.
#include "fft_dev.h"

namespace lcpc {

namespace {

// K12's pass (fft.hip fft_pass_kernel, stage for stage) with the additions of MODE (fft_dev.h DomPass)
template <int NL, int MODE>
__global__ void __launch_bounds__(1024) dom_pass_kernel(FftPass a, DomPass d) {
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
  const u32 tsh = d.tw_shift;
  const u64 in_vec = ((u64)1 << a.log_n) - 1;

  for (u32 i = tid; i < half; i += nt) lds_put<NL>(tw, half, i, tab_pow<NL>(a.tab, a.h, ((u64)i << (a.log_n - s)) << tsh));

  for (u32 e = tid; e < T; e += nt) {
    const u32 cl = e & ((1u << lcl) - 1), m = (e >> lcl) & (rows - 1), ct = e >> (lcl + s);
    const u32 col = (ct << lcl) | cl;
    const u64 q = q0 + col;
    if (q < a.n_cols) {
      const u64 top = q >> r, low = q & low_mask;
      const u64 g = (top << (s + r)) + ((u64)m << r) + low;
      Fe<NL> v;
      if constexpr (MODE == DOM_LOAD) {
        const u64 vec = g >> a.log_n, i = g & in_vec;
        const u64 j = a.dit ? __brevll(i) >> (64 - a.log_n) : i;
        if (j < d.n_coeffs) {
          v = fe_load<NL>(a.src + (((vec >> d.b) << d.src_log) + i) * NL);
          Fe<NL> sc = tab_pow<NL>(d.stab, d.hs, j);
          if (d.b) sc = fe_mul<NL>(sc, tab_pow<NL>(a.tab, a.h, (u64)(__brev((u32)vec & ((1u << d.b) - 1)) >> (32 - d.b)) * j));
          v = fe_mul<NL>(v, sc);
        } else {
#pragma unroll
          for (int l = 0; l < NL; l++) v.v[l] = 0;
        }
      } else {
        v = fe_load<NL>(a.src + g * NL);
      }
      if (a.dit && r) v = fe_mul<NL>(v, tab_pow<NL>(a.tab, a.h, ((low * (u64)(__brev(m) >> (32 - s))) << a.t0) << tsh));
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
      if (!a.dit && r) v = fe_mul<NL>(v, tab_pow<NL>(a.tab, a.h, ((low * (u64)(__brev(m) >> (32 - s))) << a.t0) << tsh));
      if constexpr (MODE == DOM_STORE) {
        const u64 i = g & in_vec;
        v = fe_mul<NL>(v, tab_pow<NL>(d.stab, d.hs, a.dit ? i : __brevll(i) >> (64 - a.log_n)));
      }
      fe_store<NL>(a.dst + g * NL, v);
    }
  }
}

template <int NL, int MODE>
hipError_t dom_pass_nl(const FftPass& a, const DomPass& d, hipStream_t st) {
  const size_t lds_bytes = pass_lds_bytes(NL, a);
  hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(&dom_pass_kernel<NL, MODE>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_bytes);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL((dom_pass_kernel<NL, MODE>), dim3((unsigned)pass_blocks(a)), dim3(pass_lanes(a)), lds_bytes, st, a, d);
  return hipGetLastError();
}

template <int MODE>
hipError_t dom_pass_mode(int nl, const FftPass& a, const DomPass& d, hipStream_t st) {
  switch (nl) {
    case 2: return dom_pass_nl<2, MODE>(a, d, st);
    case 4: return dom_pass_nl<4, MODE>(a, d, st);
    case 6: return dom_pass_nl<6, MODE>(a, d, st);
    default: return dom_pass_nl<8, MODE>(a, d, st);
  }
}

hipError_t dom_pass_any(int nl, int mode, const FftPass& a, const DomPass& d, hipStream_t st) {
  return mode == DOM_LOAD ? dom_pass_mode<DOM_LOAD>(nl, a, d, st) : mode == DOM_STORE ? dom_pass_mode<DOM_STORE>(nl, a, d, st) : dom_pass_mode<DOM_MID>(nl, a, d, st);
}

inline bool words_overlap(const uint32_t* a, uint64_t na, const uint32_t* b, uint64_t nb) {
  const uintptr_t x = reinterpret_cast<uintptr_t>(a), y = reinterpret_cast<uintptr_t>(b);
  return x < y + nb * 4 && y < x + na * 4;
}

}  // namespace

hipError_t launch_coset_fft(int nl, int form, uint32_t log_n, uint32_t log_tile, uint32_t n_vecs, const uint32_t* in, uint32_t* out,
                            const uint32_t* tab, const uint32_t* stab, hipStream_t st, uint32_t* n_launches) {
  uint32_t s[FFT_MAX_PASSES];
  const int n_pass = fft_plan(log_n, log_tile, s);
  const bool inverse = form >= FFT_IFFT_II;
  if (!nl_ok(nl) || form < FFT_FFT_II || form > FFT_IFFT_OI || n_pass < 0 || n_vecs == 0 || n_vecs > 65535) return hipErrorInvalidValue;
  if (!in || !out || !elem_aligned(in, nl) || !elem_aligned(out, nl)) return hipErrorInvalidValue;
  if (log_n && (!tab || !elem_aligned(tab, nl) || !stab || !elem_aligned(stab, nl))) return hipErrorInvalidValue;
  const uint64_t total = (uint64_t)n_vecs << log_n;                 // (n_vecs < 2^16, log_n <= 32: no overflow)
  if (total >= ((uint64_t)1 << 39)) return hipErrorInvalidValue;
  if (in != out && words_overlap(in, total * nl, out, total * nl)) return hipErrorInvalidValue;
  if (n_launches) *n_launches = 0;
  if (log_n == 0) {                                                 // one point: s^0 = 1
    if (in == out) return hipSuccess;
    return hipMemcpyAsync(out, in, (size_t)total * nl * 4, hipMemcpyDeviceToDevice, st);
  }
  const bool ii = form == FFT_FFT_II || form == FFT_IFFT_II;
  const bool dit = ii || form == FFT_FFT_OI || form == FFT_IFFT_OI;
  uint32_t launches = 0;
  const uint32_t* src = in;
  if (ii) {
    hipError_t e = launch_fft_bitrev(nl, in, out, log_n, total, st);
    if (e != hipSuccess) return e;
    launches++;
    src = out;
  }
  uint32_t t0s[FFT_MAX_PASSES], t0 = 0;
  for (int p = 0; p < n_pass; p++) { t0s[p] = t0; t0 += s[p]; }
  DomPass d;
  d.stab = stab; d.hs = fft_tab_split(log_n); d.b = 0; d.src_log = log_n; d.n_coeffs = (uint64_t)1 << log_n; d.tw_shift = 0;
  for (int k = 0; k < n_pass; k++) {
    const int p = dit ? n_pass - 1 - k : k;
    FftPass a;
    a.src = src; a.dst = out; a.tab = tab;
    a.log_n = log_n; a.t0 = t0s[p]; a.s = s[p]; a.h = fft_tab_split(log_n);
    a.log_c = log_cols(nl, s[p]);
    a.n_cols = (uint64_t)n_vecs << (log_n - s[p]);
    a.dit = dit; a.scale = 0;
    const int mode = !inverse && k == 0 ? DOM_LOAD : inverse && k == n_pass - 1 ? DOM_STORE : DOM_MID;
    hipError_t e = dom_pass_any(nl, mode, a, d, st);
    if (e != hipSuccess) return e;
    launches++;
    src = out;
  }
  if (n_launches) *n_launches = launches;
  return hipSuccess;
}

hipError_t launch_extend(int nl, uint64_t n_coeffs, uint32_t log_m, int natural, uint32_t log_tile, uint32_t n_vecs, const uint32_t* coeffs,
                         uint32_t* out, const uint32_t* tab_m, const uint32_t* stab, hipStream_t st, uint32_t* n_launches) {
  if (!nl_ok(nl) || log_m > FFT_MAX_LOG_N || n_coeffs == 0 || n_coeffs > ((uint64_t)1 << log_m) || n_vecs == 0) return hipErrorInvalidValue;
  const uint32_t src_log = ext_src_log(n_coeffs), log_n = ext_log_n(n_coeffs, log_m), b = log_m - log_n;
  uint32_t s[FFT_MAX_PASSES];
  const int n_pass = fft_plan(log_n, log_tile, s);
  if (n_pass < 0 || (natural != 0 && natural != 1) || ((uint64_t)n_vecs << (log_m - src_log)) > 65535) return hipErrorInvalidValue;
  if (!coeffs || !out || !elem_aligned(coeffs, nl) || !elem_aligned(out, nl)) return hipErrorInvalidValue;
  if (log_m && (!tab_m || !elem_aligned(tab_m, nl) || !stab || !elem_aligned(stab, nl))) return hipErrorInvalidValue;
  const uint64_t total = (uint64_t)n_vecs << log_m;                 // (n_vecs < 2^16, log_m <= 32: no overflow)
  if (total >= ((uint64_t)1 << 39)) return hipErrorInvalidValue;
  if (words_overlap(coeffs, ext_src_elems(n_coeffs, n_vecs) * nl, out, total * nl)) return hipErrorInvalidValue;
  if (n_launches) *n_launches = 0;
  if (log_m == 0) return hipMemcpyAsync(out, coeffs, (size_t)total * nl * 4, hipMemcpyDeviceToDevice, st);      // Y[0] = x[0]
  uint32_t launches = 0, t0 = 0;
  DomPass d;
  d.stab = stab; d.hs = fft_tab_split(log_n); d.b = b; d.src_log = src_log; d.n_coeffs = n_coeffs; d.tw_shift = b;
  for (int p = 0; p < n_pass; p++) {
    FftPass a;
    a.src = p ? out : coeffs; a.dst = out; a.tab = tab_m;
    a.log_n = log_n; a.t0 = t0; a.s = s[p]; a.h = fft_tab_split(log_m);
    a.log_c = log_cols(nl, s[p]);
    a.n_cols = ((uint64_t)n_vecs << b) << (log_n - s[p]);
    a.dit = 0; a.scale = 0;
    hipError_t e = dom_pass_any(nl, p ? DOM_MID : DOM_LOAD, a, d, st);
    if (e != hipSuccess) return e;
    launches++;
    t0 += s[p];
  }
  if (natural) {
    hipError_t e = launch_fft_bitrev(nl, out, out, log_m, total, st);
    if (e != hipSuccess) return e;
    launches++;
  }
  if (n_launches) *n_launches = launches;
  return hipSuccess;
}

}  // namespace lcpc

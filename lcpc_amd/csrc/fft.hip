// lcpc_amd/csrc/fft.hip -- K12: the plain pass of a whole-vector transform; K13: the bit-reversal permutation; fft_plan and the
// launchers of include/lcpc_hip_fft.h.
//
// K12 is fft_dev.h's pass (pass_body, described there) in its plain mode: the twiddle table of 2^log_n points, n^-1 in the store of
// an inverse transform's last pass.  K14 (domain.hip) wraps the same body in its three other modes.
//
// K13: out[rev(i)] = in[i], one element per lane; in place it swaps the pairs i < rev(i).  One side of it is scattered.
#include "fft_dev.h"

namespace lcpc {

namespace {

template <int NL>
__global__ void __launch_bounds__(1024) fft_pass_kernel(FftPass a, Fe<NL> n_inv) {
  pass_body<NL, PASS_PLAIN>(a, DomPass{}, n_inv);
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

hipError_t bitrev_any(int nl, const u32* in, u32* out, u32 log_n, u64 total, hipStream_t st) {
  return with_nl(nl, [&](auto n) {
    hipLaunchKernelGGL((fft_bitrev_kernel<decltype(n)::value>), dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, in, out, log_n, total);
    return hipGetLastError();
  });
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
  const bool inverse = form >= FFT_IFFT_II;
  if (form < FFT_FFT_II || form > FFT_IFFT_OI || (log_n && inverse && !n_inv)) return hipErrorInvalidValue;
  return run_passes(form_run(nl, form, log_n, log_tile, n_vecs, in, out, tab, st, n_launches), {tab}, [&](int k, int n_pass, FftPass a) {
    a.scale = inverse && k == n_pass - 1;
    return with_nl(nl, [&](auto n) {
      constexpr int NL = decltype(n)::value;
      return pass_launch<NL>(&fft_pass_kernel<NL>, a, fe_arg<NL>(n_inv), st);
    });
  });
}

}  // namespace lcpc

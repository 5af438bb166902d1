// lcpc_amd/csrc/domain.hip -- K14: the passes of a coset transform and of the low-degree extension (include/lcpc_hip_domain.h).
//
// A coset transform is the plain transform of x[j] s^j (forward) or the plain inverse followed by s^-j (inverse).  K14 is fft_dev.h's
// pass (pass_body, described there) with that scale fused into the one pass that touches the data first or last: the pass that loads
// the input of a forward transform multiplies every element by s^j on its way into LDS (DOM_LOAD), the pass that stores the output of
// an inverse multiplies by s^-j n^-1 on the way out (DOM_STORE), every other pass is DOM_MID.  j is the element's natural index
// whatever order it is stored in, and the power comes from a two-level table of the shift, as the twiddles do.  The transform
// therefore takes the launches of the plain one: no pass over memory scales.
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

template <int NL, int MODE>
__global__ void __launch_bounds__(1024) dom_pass_kernel(FftPass a, DomPass d) {
  pass_body<NL, MODE>(a, d, Fe<NL>{});
}

hipError_t dom_pass_any(int nl, int mode, const FftPass& a, const DomPass& d, hipStream_t st) {
  return with_nl(nl, [&](auto n) {
    constexpr int NL = decltype(n)::value;
    return pass_launch<NL>(mode == DOM_LOAD ? &dom_pass_kernel<NL, DOM_LOAD> : mode == DOM_STORE ? &dom_pass_kernel<NL, DOM_STORE> : &dom_pass_kernel<NL, DOM_MID>,
                           a, d, st);
  });
}

}  // namespace

hipError_t launch_coset_fft(int nl, int form, uint32_t log_n, uint32_t log_tile, uint32_t n_vecs, const uint32_t* in, uint32_t* out,
                            const uint32_t* tab, const uint32_t* stab, hipStream_t st, uint32_t* n_launches) {
  if (form < FFT_FFT_II || form > FFT_IFFT_OI) return hipErrorInvalidValue;
  const bool inverse = form >= FFT_IFFT_II;
  return run_passes(form_run(nl, form, log_n, log_tile, n_vecs, in, out, tab, st, n_launches), {tab, stab}, [&](int k, int n_pass, const FftPass& a) {
    DomPass d;
    d.stab = stab; d.hs = fft_tab_split(log_n); d.b = 0; d.src_log = log_n; d.n_coeffs = (uint64_t)1 << log_n; d.tw_shift = 0;
    return dom_pass_any(nl, !inverse && k == 0 ? DOM_LOAD : inverse && k == n_pass - 1 ? DOM_STORE : DOM_MID, a, d, st);
  });
}

hipError_t launch_extend(int nl, uint64_t n_coeffs, uint32_t log_m, int natural, uint32_t log_tile, uint32_t n_vecs, const uint32_t* coeffs,
                         uint32_t* out, const uint32_t* tab_m, const uint32_t* stab, hipStream_t st, uint32_t* n_launches) {
  if (log_m > FFT_MAX_LOG_N || n_coeffs == 0 || n_coeffs > ((uint64_t)1 << log_m) || n_vecs == 0 || (natural != 0 && natural != 1)) return hipErrorInvalidValue;
  const uint32_t src_log = ext_src_log(n_coeffs), log_n = ext_log_n(n_coeffs, log_m), b = log_m - log_n;
  if (((uint64_t)n_vecs << (log_m - src_log)) > 65535) return hipErrorInvalidValue;
  FftRun f;
  f.nl = nl; f.log_n = log_n; f.log_tab = log_m; f.log_tile = log_tile; f.n_vecs = (uint64_t)n_vecs << b;
  f.dit = false; f.rev = natural;
  f.in = coeffs; f.in_elems = ext_src_elems(n_coeffs, n_vecs); f.in_place = false; f.out = out; f.tab = tab_m; f.st = st; f.n_launches = n_launches;
  DomPass d;
  d.stab = stab; d.hs = fft_tab_split(log_n); d.b = b; d.src_log = src_log; d.n_coeffs = n_coeffs; d.tw_shift = b;
  return run_passes(f, {tab_m, stab}, [&](int k, int, const FftPass& a) { return dom_pass_any(nl, k ? DOM_MID : DOM_LOAD, a, d, st); });
}

}  // namespace lcpc

// tests/native/k14_harness.cpp -- test-only C entry points over the coset transform and the extension (K14: launch_coset_fft and
// launch_extend of lcpc_amd/csrc/kernels.h), in the manner of k12_harness.cpp: built by lcpc_amd/csrc/Makefile into
// lcpc_amd/lib/liblcpc_k14_harness.so and linked against the product library, which gains nothing by it (tests/k14_harness.py,
// tests/test_gpu_k14_kernels.py).
//
// The product always passes the largest tile; these pass the caller's log_tile, so that plans of many passes run at a few dozen points,
// and the caller's own twiddle and shift tables, so that the kernels are held to tables the product did not build.  They take HOST
// pointers and the sizes of the buffers behind them, check that every element the launcher may touch stays inside them (a refused
// call returns H_BAD_ARGS and launches nothing), allocate device buffers, copy in, launch on the null stream, synchronise and copy
// the WHOLE output buffer back, the words around the output included, and the input buffer as the kernels left it.  k14h_*_refusal
// hand the launchers arguments they must settle BEFORE any launch, with never-read buffers: they touch no device.
#include "harness.h"
#include "../../lcpc_amd/csrc/kernels.h"

H_DEVICE_COUNT(k14h_)

H_EXPORT uint32_t k14h_ext_src_log(uint64_t n_coeffs) { return lcpc::ext_src_log(n_coeffs); }
H_EXPORT uint32_t k14h_ext_log_n(uint64_t n_coeffs, uint32_t log_m) { return lcpc::ext_log_n(n_coeffs, log_m); }

// in: n_vecs << log_n elements of nl words (written back as the device left them).  out: out_words words of which the elements
// [out_off, out_off + (n_vecs << log_n) * nl) receive the result; everything else in it must come back as it went in.  in_place: the
// input is first copied to its place in out and the transform runs there.  tab, stab: tab_elems elements each (kernels.h)
H_EXPORT int k14h_coset_fft(int nl, int form, uint32_t log_n, uint32_t log_tile, uint32_t n_vecs, uint32_t* in, uint32_t* out,
                            uint64_t out_words, uint64_t out_off, int in_place, const uint32_t* tab, const uint32_t* stab, uint64_t tab_elems,
                            uint32_t* n_launches) {
  if (!nl_ok(nl) || form < 0 || form > 5 || log_n > 27 || n_vecs == 0 || n_vecs > 65535 || !in || !out || !tab || !stab || !n_launches) return H_BAD_ARGS;
  uint32_t s[lcpc::FFT_MAX_PASSES];
  if (lcpc::fft_plan(log_n, log_tile, s) < 0) return H_BAD_ARGS;
  const uint64_t words = ((uint64_t)n_vecs << log_n) * nl;
  if (!span_ok(words, out_words, out_off, nl)) return H_BAD_ARGS;
  if (tab_elems != lcpc::fft_tab_elems(log_n)) return H_BAD_ARGS;                  // what the kernels index, in both tables
  DevBuf d_in, d_out, d_tab, d_stab;
  H_TRY(d_out.put(out, out_words * 4));
  H_TRY(d_tab.put(tab, tab_elems * nl * 4));
  H_TRY(d_stab.put(stab, tab_elems * nl * 4));
  const uint32_t* src;
  if (in_place) {
    H_TRY(hipMemcpy(d_out.p + out_off, in, words * 4, hipMemcpyHostToDevice));
    src = d_out.p + out_off;
  } else {
    H_TRY(d_in.put(in, words * 4));
    src = d_in.p;
  }
  H_TRY(lcpc::launch_coset_fft(nl, form, log_n, log_tile, n_vecs, src, d_out.p + out_off, d_tab.p, d_stab.p, nullptr, n_launches));
  H_TRY(hipDeviceSynchronize());
  if (!in_place) H_TRY(d_in.get(in, words * 4));
  return (int)d_out.get(out, out_words * 4);
}

// coeffs: coeffs_words words holding n_vecs source vectors 2^ext_src_log(n_coeffs) elements apart of which the launcher may read the
// first n_coeffs each -- the buffer need not be longer than the last of those (written back as the device left it).  out as above
// with n_vecs << log_m elements.  tab_m: fft_tab_elems(log_m) elements; stab: fft_tab_elems(ext_log_n(n_coeffs, log_m))
H_EXPORT int k14h_extend(int nl, uint64_t n_coeffs, uint32_t log_m, int natural, uint32_t log_tile, uint32_t n_vecs, uint32_t* coeffs,
                         uint64_t coeffs_words, uint32_t* out, uint64_t out_words, uint64_t out_off, const uint32_t* tab_m, uint64_t tab_m_elems,
                         const uint32_t* stab, uint64_t stab_elems, uint32_t* n_launches) {
  if (!nl_ok(nl) || log_m > 27 || n_coeffs == 0 || n_coeffs > ((uint64_t)1 << log_m) || n_vecs == 0 || (natural != 0 && natural != 1)) return H_BAD_ARGS;
  if (!coeffs || !out || !tab_m || !stab || !n_launches) return H_BAD_ARGS;
  const uint32_t src_log = lcpc::ext_src_log(n_coeffs), log_n = lcpc::ext_log_n(n_coeffs, log_m);
  uint32_t s[lcpc::FFT_MAX_PASSES];
  if (lcpc::fft_plan(log_n, log_tile, s) < 0 || ((uint64_t)n_vecs << (log_m - src_log)) > 65535) return H_BAD_ARGS;
  const uint64_t words = ((uint64_t)n_vecs << log_m) * nl;
  const uint64_t need = ((((uint64_t)n_vecs - 1) << src_log) + n_coeffs) * nl;       // the last element the mask lets through
  if (!span_ok(words, out_words, out_off, nl)) return H_BAD_ARGS;
  if (coeffs_words > MAX_WORDS || coeffs_words < need) return H_BAD_ARGS;
  if (tab_m_elems != lcpc::fft_tab_elems(log_m) || stab_elems != lcpc::fft_tab_elems(log_n)) return H_BAD_ARGS;
  DevBuf d_in, d_out, d_tab, d_stab;
  H_TRY(d_in.put(coeffs, coeffs_words * 4));
  H_TRY(d_out.put(out, out_words * 4));
  H_TRY(d_tab.put(tab_m, tab_m_elems * nl * 4));
  H_TRY(d_stab.put(stab, stab_elems * nl * 4));
  H_TRY(lcpc::launch_extend(nl, n_coeffs, log_m, natural, log_tile, n_vecs, d_in.p, d_out.p + out_off, d_tab.p, d_stab.p, nullptr, n_launches));
  H_TRY(hipDeviceSynchronize());
  H_TRY(d_in.get(coeffs, coeffs_words * 4));
  return (int)d_out.get(out, out_words * 4);
}

// What launch_coset_fft answers to a job it must settle before any launch -- so this refuses (H_BAD_ARGS) every job a correct
// launcher would launch.  null_mask: bit 0 in, 1 out, 2 tab, 3 stab are NULL; misalign: the same bits, 4 bytes off; overlap: out starts
// one element behind in.  The pointers point at words nothing reads.  Returns the launcher's hipError_t
H_EXPORT int k14h_coset_refusal(int nl, int form, uint32_t log_n, uint32_t log_tile, uint32_t n_vecs, uint32_t null_mask, uint32_t misalign,
                                int overlap) {
  uint32_t s[lcpc::FFT_MAX_PASSES];
  const bool settled = !nl_ok(nl) || form < 0 || form > 5 || lcpc::fft_plan(log_n, log_tile, s) < 0 || n_vecs == 0 || n_vecs > 65535 ||
                       (null_mask & 3u) || (log_n && (null_mask & 12u)) || (misalign & 3u) || (log_n && (misalign & 12u)) ||
                       (log_n <= 32 && ((uint64_t)n_vecs << log_n) >= ((uint64_t)1 << 39)) || (overlap && (((uint64_t)n_vecs << log_n) > 1));
  if (!settled) return H_BAD_ARGS;
  alignas(16) static uint32_t dummy[64];
  auto arg = [&](unsigned bit) -> uint32_t* { return (null_mask >> bit) & 1u ? nullptr : dummy + 16 * bit + ((misalign >> bit) & 1u); };
  uint32_t launches = 0;
  uint32_t* in = arg(0);
  uint32_t* out = overlap && nl_ok(nl) ? dummy + nl : arg(1);
  if (overlap) in = dummy;
  return (int)lcpc::launch_coset_fft(nl, form, log_n, log_tile, n_vecs, in, out, arg(2), arg(3), nullptr, &launches);
}

// the same for launch_extend; null_mask / misalign: bit 0 coeffs, 1 out, 2 tab_m, 3 stab; overlap: out starts at coeffs
H_EXPORT int k14h_extend_refusal(int nl, uint64_t n_coeffs, uint32_t log_m, int natural, uint32_t log_tile, uint32_t n_vecs, uint32_t null_mask,
                                 uint32_t misalign, int overlap) {
  uint32_t s[lcpc::FFT_MAX_PASSES];
  bool settled = !nl_ok(nl) || log_m > lcpc::FFT_MAX_LOG_N || n_coeffs == 0 || n_vecs == 0 || (natural != 0 && natural != 1);
  if (!settled) settled = n_coeffs > ((uint64_t)1 << log_m);
  if (!settled)
    settled = lcpc::fft_plan(lcpc::ext_log_n(n_coeffs, log_m), log_tile, s) < 0 || ((uint64_t)n_vecs << (log_m - lcpc::ext_src_log(n_coeffs))) > 65535 ||
              (null_mask & 3u) || (log_m && (null_mask & 12u)) || (misalign & 3u) || (log_m && (misalign & 12u)) ||
              ((uint64_t)n_vecs << log_m) >= ((uint64_t)1 << 39) || overlap;
  if (!settled) return H_BAD_ARGS;
  alignas(16) static uint32_t dummy[64];
  auto arg = [&](unsigned bit) -> uint32_t* { return (null_mask >> bit) & 1u ? nullptr : dummy + 16 * bit + ((misalign >> bit) & 1u); };
  uint32_t launches = 0;
  return (int)lcpc::launch_extend(nl, n_coeffs, log_m, natural, log_tile, n_vecs, arg(0), overlap ? dummy : arg(1), arg(2), arg(3), nullptr, &launches);
}

// tests/native/k12_harness.cpp -- test-only C entry points over the whole-vector transform (K12 / K13: launch_fft and fft_plan of
// lcpc_amd/csrc/kernels.h), in the manner of k8_harness.cpp: built by lcpc_amd/csrc/Makefile into lcpc_amd/lib/liblcpc_k12_harness.so
// and linked against the product library, which gains nothing by it (tests/k12_harness.py, tests/test_gpu_k12_kernels.py).
//
// The product always passes the largest tile; k12h_fft passes the caller's log_tile, so that plans of three and more passes run at a
// few dozen points, and the caller's own twiddle table, so that the kernels are held to a table the product did not build.  It takes
// HOST pointers and the sizes of the buffers behind them, checks that every element the launcher may touch stays inside them (a
// refused call returns H_BAD_ARGS and launches nothing), allocates device buffers, copies in, launches on the null stream,
// synchronises and copies the WHOLE output buffer back, the words around the output included.  k12h_refusal hands the launcher
// arguments it must settle BEFORE any launch, with never-read buffers: it touches no device.
#include "harness.h"
#include "../../lcpc_amd/csrc/kernels.h"

H_DEVICE_COUNT(k12h_)

H_EXPORT int k12h_max_log_tile() { return (int)lcpc::FFT_MAX_LOG_TILE; }
H_EXPORT int k12h_max_passes() { return (int)lcpc::FFT_MAX_PASSES; }
H_EXPORT uint32_t k12h_tab_split(uint32_t log_n) { return lcpc::fft_tab_split(log_n); }
H_EXPORT uint64_t k12h_tab_elems(uint32_t log_n) { return lcpc::fft_tab_elems(log_n); }
// the product's own plan: s[k12h_max_passes()] -> the number of passes, -1 for a log_tile or log_n the launcher refuses
H_EXPORT int k12h_plan(uint32_t log_n, uint32_t log_tile, uint32_t* s) { return lcpc::fft_plan(log_n, log_tile, s); }

// in: n_vecs << log_n elements of nl words.  out: out_words words of which the elements [out_off, out_off + (n_vecs << log_n) * nl)
// receive the result; everything else in it must come back as it went in.  in_place: the input is first copied to its place in out
// and the transform runs there (`in` itself then never reaches the launcher).  tab: tab_elems elements, n_inv: one element (read by
// the inverse forms).  *n_launches: what the launcher reports
H_EXPORT int k12h_fft(int nl, int form, uint32_t log_n, uint32_t log_tile, uint32_t n_vecs, const uint32_t* in, uint32_t* out,
                      uint64_t out_words, uint64_t out_off, int in_place, const uint32_t* tab, uint64_t tab_elems, const uint32_t* n_inv,
                      uint32_t* n_launches) {
  if (!nl_ok(nl) || form < 0 || form > 5 || log_n > 27 || n_vecs == 0 || n_vecs > 65535 || !in || !out || !tab || !n_inv || !n_launches) return H_BAD_ARGS;
  uint32_t s[lcpc::FFT_MAX_PASSES];
  if (lcpc::fft_plan(log_n, log_tile, s) < 0) return H_BAD_ARGS;
  const uint64_t words = ((uint64_t)n_vecs << log_n) * nl;
  if (!span_ok(words, out_words, out_off, nl)) return H_BAD_ARGS;
  if (tab_elems != lcpc::fft_tab_elems(log_n)) return H_BAD_ARGS;                  // what the kernels index
  DevBuf d_in, d_out, d_tab;
  H_TRY(d_out.put(out, out_words * 4));
  H_TRY(d_tab.put(tab, tab_elems * nl * 4));
  const uint32_t* src;
  if (in_place) {
    H_TRY(hipMemcpy(d_out.p + out_off, in, words * 4, hipMemcpyHostToDevice));
    src = d_out.p + out_off;
  } else {
    H_TRY(d_in.put(in, words * 4));
    src = d_in.p;
  }
  H_TRY(lcpc::launch_fft(nl, form, log_n, log_tile, n_vecs, src, d_out.p + out_off, d_tab.p, n_inv, nullptr, n_launches));
  H_TRY(hipDeviceSynchronize());
  return (int)d_out.get(out, out_words * 4);
}

// What the launcher answers to a job it must settle before any launch -- so this refuses (H_BAD_ARGS) every job a correct launcher
// would launch.  null_mask: bit 0 in, 1 out, 2 tab, 3 n_inv are NULL; misalign: bit 0 in, 1 out, 2 tab are 4 bytes off; the others
// point at words nothing reads.  Returns the launcher's hipError_t
H_EXPORT int k12h_refusal(int nl, int form, uint32_t log_n, uint32_t log_tile, uint32_t n_vecs, uint32_t null_mask, uint32_t misalign) {
  uint32_t s[lcpc::FFT_MAX_PASSES];
  const bool inverse = form >= 3;
  const bool settled = !nl_ok(nl) || form < 0 || form > 5 || lcpc::fft_plan(log_n, log_tile, s) < 0 || n_vecs == 0 || n_vecs > 65535 ||
                       (null_mask & 3u) || (log_n && (null_mask & 4u)) || (log_n && inverse && (null_mask & 8u)) || (misalign & 3u) ||
                       (log_n && (misalign & 4u)) || (log_n <= 32 && ((uint64_t)n_vecs << log_n) >= ((uint64_t)1 << 39));
  if (!settled) return H_BAD_ARGS;
  alignas(16) static uint32_t dummy[16];
  auto arg = [&](unsigned bit) -> uint32_t* { return (null_mask >> bit) & 1u ? nullptr : dummy + ((misalign >> bit) & 1u); };
  uint32_t launches = 0;
  return (int)lcpc::launch_fft(nl, form, log_n, log_tile, n_vecs, arg(0), arg(1), arg(2), (null_mask & 8u) ? nullptr : dummy, nullptr, &launches);
}

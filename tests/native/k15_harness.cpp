// tests/native/k15_harness.cpp -- test-only C entry points over the inverse, pointwise and domain-quotient launchers (K15 / K16:
// launch_batch_inverse, launch_pointwise and launch_domain_quotient of lcpc_amd/csrc/kernels.h), in the manner of k14_harness.cpp: built
// by lcpc_amd/csrc/Makefile into lcpc_amd/lib/liblcpc_k15_harness.so and linked against the product library, which gains nothing by it
// (tests/k15_harness.py, tests/test_gpu_k15_kernels.py).
//
// They take HOST pointers and the sizes of the buffers behind them, check that every element the launcher may touch stays inside them
// (a refused call returns H_BAD_ARGS and launches nothing), allocate device buffers, copy in, launch on the null stream,
// synchronise and copy the WHOLE output buffer back, the words around the output included, and the inputs as the kernels left them.
// The twiddle table of K16 is the caller's.  k15h_*_refusal hand the launchers arguments they must settle BEFORE any launch, with
// never-read buffers: they touch no device.
#include "harness.h"
#include "../../lcpc_amd/csrc/kernels.h"

H_DEVICE_COUNT(k15h_)
H_CU_COUNT(k15h_)

// the elements of a workgroup's tile
H_EXPORT uint32_t k15h_tile(int nl) { return nl_ok(nl) ? lcpc::quot_tile(nl) : 0; }

// op 0..3: launch_pointwise; op -1: launch_batch_inverse of b (a is not read).  a, b: n elements of nl words each (written back as the
// device left them).  out: out_words words of which the elements from out_off on receive the result; everything else in it must come
// back as it went in.  in_place: 0 no, 1 the output is where a is, 2 where b is (the operand is first copied to its place in out)
H_EXPORT int k15h_pointwise(int nl, int op, uint32_t* a, uint32_t* b, uint64_t n, uint32_t* out, uint64_t out_words, uint64_t out_off, int in_place) {
  if (!nl_ok(nl) || op < -1 || op > 3 || n == 0 || !b || !out || (op >= 0 && !a) || in_place < 0 || in_place > 2 || (op < 0 && in_place == 1)) return H_BAD_ARGS;
  if (n > MAX_WORDS / nl) return H_BAD_ARGS;
  const uint64_t words = n * nl;
  if (!span_ok(words, out_words, out_off, nl)) return H_BAD_ARGS;
  DevBuf d_a, d_b, d_out;
  H_TRY(d_out.put(out, out_words * 4));
  const uint32_t *pa = nullptr, *pb = nullptr;
  if (in_place == 1) { H_TRY(hipMemcpy(d_out.p + out_off, a, words * 4, hipMemcpyHostToDevice)); pa = d_out.p + out_off; }
  else if (op >= 0) { H_TRY(d_a.put(a, words * 4)); pa = d_a.p; }
  if (in_place == 2) { H_TRY(hipMemcpy(d_out.p + out_off, b, words * 4, hipMemcpyHostToDevice)); pb = d_out.p + out_off; }
  else { H_TRY(d_b.put(b, words * 4)); pb = d_b.p; }
  if (op < 0) H_TRY(lcpc::launch_batch_inverse(nl, pb, d_out.p + out_off, n, nullptr));
  else H_TRY(lcpc::launch_pointwise(nl, op, pa, pb, d_out.p + out_off, n, nullptr));
  H_TRY(hipDeviceSynchronize());
  if (d_a.p) H_TRY(d_a.get(a, words * 4));
  if (d_b.p) H_TRY(d_b.get(b, words * 4));
  return (int)d_out.get(out, out_words * 4);
}

// in: n_vecs << log_m elements; out as above; tab: tab_elems == fft_tab_elems(log_m) elements, the forward table; shift: nl words (the
// shift for kind 0 or NULL, shift^n for kind 1), z: nl words, y: n_vecs elements (kind 0)
H_EXPORT int k15h_domain_quotient(int nl, int kind, int bitrev, uint32_t log_m, uint32_t log_n, uint32_t n_vecs, uint32_t* in, uint32_t* out,
                                  uint64_t out_words, uint64_t out_off, int in_place, const uint32_t* tab, uint64_t tab_elems, const uint32_t* shift,
                                  const uint32_t* z, const uint32_t* y) {
  if (!nl_ok(nl) || (kind != 0 && kind != 1) || log_m > 24 || n_vecs == 0 || n_vecs > 65535 || !in || !out || !tab) return H_BAD_ARGS;
  if (kind == 0 ? (!z || !y) : (!shift || log_n > log_m)) return H_BAD_ARGS;
  const uint64_t words = ((uint64_t)n_vecs << log_m) * nl;
  if (!span_ok(words, out_words, out_off, nl) || tab_elems != lcpc::fft_tab_elems(log_m)) return H_BAD_ARGS;
  DevBuf d_in, d_out, d_tab, d_y;
  H_TRY(d_out.put(out, out_words * 4));
  H_TRY(d_tab.put(tab, tab_elems * nl * 4));
  if (kind == 0) H_TRY(d_y.put(y, (size_t)n_vecs * nl * 4));
  const uint32_t* src;
  if (in_place) {
    H_TRY(hipMemcpy(d_out.p + out_off, in, words * 4, hipMemcpyHostToDevice));
    src = d_out.p + out_off;
  } else {
    H_TRY(d_in.put(in, words * 4));
    src = d_in.p;
  }
  H_TRY(lcpc::launch_domain_quotient(nl, kind, bitrev, log_m, log_n, n_vecs, src, d_out.p + out_off, d_tab.p, shift, z, d_y.p, nullptr));
  H_TRY(hipDeviceSynchronize());
  if (!in_place) H_TRY(d_in.get(in, words * 4));
  return (int)d_out.get(out, out_words * 4);
}

// What launch_batch_inverse (op -1) or launch_pointwise answers to a job it must settle before any launch -- so this refuses
// (H_BAD_ARGS) every job a correct launcher would launch.  null_mask / misalign: bit 0 a, 1 b, 2 out (NULL, or 4 bytes off);
// overlap: out starts one element behind b.  The pointers point at words nothing reads.  Returns the launcher's hipError_t
H_EXPORT int k15h_pointwise_refusal(int nl, int op, uint64_t n, uint32_t null_mask, uint32_t misalign, int overlap) {
  const uint32_t used = op == -1 ? 6u : 7u;
  const bool settled = !nl_ok(nl) || op < -1 || op > 3 || n == 0 || n >= ((uint64_t)1 << 39) || (null_mask & used) || (misalign & used) || (overlap && n > 1);
  if (!settled) return H_BAD_ARGS;
  alignas(16) static uint32_t dummy[64];
  auto arg = [&](unsigned bit) -> uint32_t* { return (null_mask >> bit) & 1u ? nullptr : dummy + 16 * bit + ((misalign >> bit) & 1u); };
  uint32_t* b = overlap ? dummy : arg(1);
  uint32_t* out = overlap && nl_ok(nl) ? dummy + nl : arg(2);
  if (op == -1) return (int)lcpc::launch_batch_inverse(nl, b, out, n, nullptr);
  return (int)lcpc::launch_pointwise(nl, op, arg(0), b, out, n, nullptr);
}

// the same for launch_domain_quotient; bits: 0 in, 1 out, 2 tab, 3 y (kind 0), 4 shift (kind 1; NULL only), 5 z (kind 0; NULL only);
// overlap: out starts one element behind in
H_EXPORT int k15h_quotient_refusal(int nl, int kind, uint32_t log_m, uint32_t log_n, uint32_t n_vecs, uint32_t null_mask, uint32_t misalign, int overlap) {
  bool settled = !nl_ok(nl) || (kind != 0 && kind != 1) || log_m > lcpc::FFT_MAX_LOG_N || n_vecs == 0 || n_vecs > 65535;
  if (!settled)
    settled = (null_mask & 3u) || (misalign & 3u) || (log_m && ((null_mask | misalign) & 4u)) || (kind == 0 && (((null_mask | misalign) & 8u) || (null_mask & 32u))) ||
              (kind == 1 && ((null_mask & 16u) || log_n > log_m)) || ((uint64_t)n_vecs << log_m) >= ((uint64_t)1 << 39) ||
              (overlap && ((uint64_t)n_vecs << log_m) > 1);
  if (!settled) return H_BAD_ARGS;
  alignas(16) static uint32_t dummy[128];
  auto arg = [&](unsigned bit) -> uint32_t* { return (null_mask >> bit) & 1u ? nullptr : dummy + 16 * bit + ((misalign >> bit) & 1u); };
  uint32_t* in = overlap ? dummy : arg(0);
  uint32_t* out = overlap && nl_ok(nl) ? dummy + nl : arg(1);
  return (int)lcpc::launch_domain_quotient(nl, kind, 0, log_m, log_n, n_vecs, in, out, arg(2), arg(4), arg(5), arg(3), nullptr);
}

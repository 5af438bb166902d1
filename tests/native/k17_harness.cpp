// tests/native/k17_harness.cpp -- test-only C entry points over the scan launcher (K17: launch_scan of lcpc_amd/csrc/kernels.h), in the
// manner of k15_harness.cpp: built by lcpc_amd/csrc/Makefile into lcpc_amd/lib/liblcpc_k17_harness.so and linked against the product
// library, which gains nothing by it (tests/k17_harness.py, tests/test_gpu_k17_kernels.py).
//
// They take HOST pointers and the sizes of the buffers behind them, check that every element the launcher may touch stays inside them
// (a refused call returns H_BAD_ARGS and launches nothing), allocate device buffers, copy in, launch on the null stream,
// synchronise and copy the WHOLE output, total and work buffers back, the words around them included, and the input as the kernels
// left it.  k17h_scan_refusal hands the launcher arguments it must settle BEFORE any launch, with never-read buffers: it touches no
// device.
#include "harness.h"
#include "../../lcpc_amd/csrc/kernels.h"

H_DEVICE_COUNT(k17h_)
H_CU_COUNT(k17h_)

// the elements of a workgroup's tile, the consecutive elements of a lane, the totals K17b takes per recursion level, and the elements
// of the workspace
H_EXPORT uint32_t k17h_tile(int nl) { return nl_ok(nl) ? lcpc::scan_tile(nl) : 0; }
H_EXPORT uint32_t k17h_lane_elems(int nl) { return nl_ok(nl) ? lcpc::scan_lane_elems(nl) : 0; }
H_EXPORT uint32_t k17h_mid_chunk(int nl) { return nl_ok(nl) ? lcpc::scan_mid_chunk(nl) : 0; }
H_EXPORT uint64_t k17h_work_elems(int nl, uint64_t n, uint32_t n_vecs) {
  return nl_ok(nl) && n && n < ((uint64_t)1 << 39) && n_vecs && n_vecs <= 65535 ? lcpc::scan_work_elems(nl, n, n_vecs) : 0;
}

// launch_scan.  in: n_vecs * n elements of nl words (written back as the device left them).  out: out_words words of which the
// elements from out_off on receive the result; in_place: the input is first copied to its place in out and scanned there.  init:
// n_vecs elements or NULL.  total: NULL, or total_words words of which n_vecs elements from total_off on receive the totals.  work:
// work_words words of which the scan_work_elems elements from work_off on are the workspace.  one: R mod p.  Everything else in out, total
// and work must come back as it went in.  *n_launches (may be NULL): the kernels launched
H_EXPORT int k17h_scan(int nl, int op, int mode, uint32_t* in, uint64_t n, uint32_t n_vecs, uint32_t* out, uint64_t out_words, uint64_t out_off,
                       int in_place, const uint32_t* init, uint32_t* total, uint64_t total_words, uint64_t total_off, const uint32_t* one,
                       uint32_t* work, uint64_t work_words, uint64_t work_off, uint32_t* n_launches) {
  if (!nl_ok(nl) || !in || !out || !one || !work || n == 0 || n_vecs == 0 || n_vecs > 65535 || n > MAX_WORDS / nl / n_vecs) return H_BAD_ARGS;
  const uint64_t words = n * n_vecs * nl, ends = (uint64_t)n_vecs * nl, need = lcpc::scan_work_elems(nl, n, n_vecs);
  if (!span_ok(words, out_words, out_off, nl) || (total && !span_ok(ends, total_words, total_off, nl))) return H_BAD_ARGS;
  if (!span_ok(need * nl, work_words, work_off, nl)) return H_BAD_ARGS;
  DevBuf d_in, d_out, d_init, d_total, d_work;
  H_TRY(d_out.put(out, out_words * 4));
  H_TRY(d_work.put(work, work_words * 4));
  if (init) H_TRY(d_init.put(init, ends * 4));
  if (total) H_TRY(d_total.put(total, total_words * 4));
  const uint32_t* src;
  if (in_place) {
    H_TRY(hipMemcpy(d_out.p + out_off, in, words * 4, hipMemcpyHostToDevice));
    src = d_out.p + out_off;
  } else {
    H_TRY(d_in.put(in, words * 4));
    src = d_in.p;
  }
  H_TRY(lcpc::launch_scan(nl, op, mode, src, d_out.p + out_off, n, n_vecs, d_init.p, total ? d_total.p + total_off : nullptr, one,
                             d_work.p + work_off, need, nullptr, n_launches));
  H_TRY(hipDeviceSynchronize());
  if (!in_place) H_TRY(d_in.get(in, words * 4));
  if (total) H_TRY(d_total.get(total, total_words * 4));
  H_TRY(d_work.get(work, work_words * 4));
  return (int)d_out.get(out, out_words * 4);
}

// K17b alone: what the scan does with the tile totals of n_vecs vectors, n_totals each -- their exclusive scan in place, seeded with
// init, and the totals of the vectors.  The buffers as for k17h_scan, `totals` in the place of out
H_EXPORT int k17h_scan_totals(int nl, int op, uint32_t* totals_in, uint64_t n_totals, uint32_t n_vecs, uint32_t* totals, uint64_t totals_words,
                              uint64_t totals_off, const uint32_t* init, uint32_t* total, uint64_t total_words, uint64_t total_off,
                              const uint32_t* one, uint32_t* work, uint64_t work_words, uint64_t work_off) {
  return k17h_scan(nl, op, lcpc::SCAN_EXCLUSIVE, totals_in, n_totals, n_vecs, totals, totals_words, totals_off, 1, init, total, total_words, total_off,
                   one, work, work_words, work_off, nullptr);
}

// What launch_scan answers to a job it must settle before any launch -- so this refuses (H_BAD_ARGS) every job a correct launcher
// would launch.  null_mask / misalign: bit 0 in, 1 out, 2 work, 3 init, 4 total, 5 one (NULL only).  overlap: 1 out starts one element
// behind in; 2 init is the output's first element; 3 total lies in the input; 4 work starts at the output's last element; 5 init is total.
// short_work: work_elems is one less than needed.  The pointers point at words nothing reads.  Returns the launcher's hipError_t
H_EXPORT int k17h_scan_refusal(int nl, int op, int mode, uint64_t n, uint32_t n_vecs, uint32_t null_mask, uint32_t misalign, int overlap,
                               int short_work) {
  bool settled = !nl_ok(nl) || op < 0 || op > 1 || mode < 0 || mode > 1 || n == 0 || n >= ((uint64_t)1 << 39) || n_vecs == 0 || n_vecs > 65535;
  if (!settled) settled = n * n_vecs >= ((uint64_t)1 << 39) || lcpc::scan_tiles(nl, n) >= lcpc::SCAN_MAX_TILES || (null_mask & 39u) || (misalign & ~null_mask & 31u) || short_work || (overlap >= 2 && overlap <= 5) ||
                          (overlap == 1 && n * n_vecs > 1);
  if (!settled || overlap < 0 || overlap > 5) return H_BAD_ARGS;
  // the buffers lie far apart in an address range that is never touched: 2^50 bytes per buffer
  auto arg = [&](unsigned bit) -> uint32_t* {
    if ((null_mask >> bit) & 1u) return nullptr;
    return reinterpret_cast<uint32_t*>(((uintptr_t)(bit + 1) << 50) + 4 * ((misalign >> bit) & 1u));
  };
  alignas(16) static const uint32_t one[8] = {1, 0, 0, 0, 0, 0, 0, 0};
  const uint32_t* in = arg(0);
  uint32_t *out = arg(1), *work = arg(2), *init = arg(3), *total = arg(4);
  const uint64_t words = nl_ok(nl) ? n * n_vecs * nl : 0;
  if (overlap == 1) out = const_cast<uint32_t*>(in) + nl;
  if (overlap == 2) init = out;
  if (overlap == 3) total = const_cast<uint32_t*>(in);
  if (overlap == 4) work = out + words - nl;
  if (overlap == 5) init = total = reinterpret_cast<uint32_t*>((uintptr_t)5 << 50);
  uint64_t need = nl_ok(nl) && n && n < ((uint64_t)1 << 39) && n_vecs ? lcpc::scan_work_elems(nl, n, n_vecs) : 1;
  return (int)lcpc::launch_scan(nl, op, mode, in, out, n, n_vecs, init, total, (null_mask >> 5) & 1u ? nullptr : one, work, need - (short_work ? 1 : 0),
                                nullptr, nullptr);
}

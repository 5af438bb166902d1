// tests/native/k18_harness.cpp -- test-only C entry points over the sumcheck launchers (K18 / K19: launch_sumcheck_round,
// launch_sumcheck_bind, launch_sumcheck_bind_round of lcpc_amd/csrc/kernels.h), in the manner of k17_harness.cpp: built by
// lcpc_amd/csrc/Makefile into lcpc_amd/lib/liblcpc_k18_harness.so and linked against the product library, which gains nothing by it
// (tests/k18_harness.py, tests/test_gpu_k18_kernels.py).
//
// k18h_run takes HOST pointers and the sizes of the buffers behind them, checks that every element the launcher may touch stays
// inside them (a refused call returns H_BAD_ARGS and launches nothing), allocates device buffers, copies in, launches on the null
// stream with the caller's max_groups, synchronises and copies the WHOLE output, evals and work buffers back, the words around them
// included, and the input as the kernels left it.  k18h_refusal hands a launcher a job it must settle BEFORE any launch, with
// never-read buffers: it touches no device.
#include "harness.h"
#include "../../lcpc_amd/csrc/kernels.h"

namespace {

enum { MODE_BIND = 0, MODE_ROUND = 1, MODE_FUSED = 2 };

}  // namespace

H_DEVICE_COUNT(k18h_)
H_CU_COUNT(k18h_)

// the pairs a workgroup takes per stride (P), the product's max_groups, and the elements of the workspace of a round over `pairs` pairs
H_EXPORT uint32_t k18h_tile_pairs(int nl) { return lcpc::nl_ok(nl) ? lcpc::sumcheck_tile_pairs(nl) : 0; }
H_EXPORT uint32_t k18h_default_groups() { return lcpc::SUMCHECK_GROUPS; }
H_EXPORT uint64_t k18h_work_elems(uint64_t pairs, uint32_t n_terms, uint32_t max_groups) {
  return pairs && n_terms && n_terms <= lcpc::SUMCHECK_MAX_TERMS && max_groups ? lcpc::sumcheck_work_elems(pairs, n_terms, max_groups) : 0;
}

// mode 0: launch_sumcheck_bind, 1: launch_sumcheck_round, 2: launch_sumcheck_bind_round.  in: n_tables tables of n elements of nl words,
// one after the other (written back as the device left them).  out (modes 0, 2): n_tables slots of slot_words words; table j's
// output starts out_off words into slot j; in_place: table j is first copied to that place (n elements) and bound there.  terms:
// n_terms records of 1 + SUMCHECK_MAX_FACTORS words; coeffs: n_terms elements or NULL; one, r: one element each.  evals (modes 1, 2):
// evals_words words of which the d + 1 elements from evals_off on receive the result; work: work_words words of which the
// sumcheck_work_elems elements from work_off on are the workspace.  Everything else in out, evals and work must come back as it went
// in.  *n_launches (may be NULL): the kernels launched
H_EXPORT int k18h_run(int mode, int nl, int order, uint32_t* in, uint64_t n, uint32_t n_tables, uint32_t* out, uint64_t slot_words,
                      uint64_t out_off, int in_place, const uint32_t* terms, uint32_t n_terms, const uint32_t* coeffs, const uint32_t* one,
                      const uint32_t* r, uint32_t* evals, uint64_t evals_words, uint64_t evals_off, uint32_t* work, uint64_t work_words,
                      uint64_t work_off, uint32_t max_groups, uint32_t* n_launches) {
  const bool bind = mode != MODE_ROUND, round = mode != MODE_BIND;
  if (mode < MODE_BIND || mode > MODE_FUSED || !lcpc::nl_ok(nl) || !in || n_tables == 0 || n_tables > lcpc::SUMCHECK_MAX_TABLES) return H_BAD_ARGS;
  if (n < (mode == MODE_FUSED ? 4u : 2u) || (n & (n - 1)) || n > MAX_WORDS / nl / n_tables) return H_BAD_ARGS;
  if (in_place && (!bind || order != lcpc::SUMCHECK_HIGH_FIRST)) return H_BAD_ARGS;
  const uint64_t words = n * nl;
  const lcpc::SumcheckTerm* tm = reinterpret_cast<const lcpc::SumcheckTerm*>(terms);
  uint64_t need = 0;
  if (bind && (!out || !r || slot_words > MAX_WORDS / n_tables || !span_ok(in_place ? words : words / 2, slot_words, out_off, nl) || !off_ok(slot_words, nl)))
    return H_BAD_ARGS;
  if (round) {
    if (!evals || !work || !one || max_groups == 0 || lcpc::sumcheck_degree(n_tables, tm, n_terms) == 0) return H_BAD_ARGS;
    need = lcpc::sumcheck_work_elems(mode == MODE_FUSED ? n / 4 : n / 2, n_terms, max_groups);
    if (!span_ok((lcpc::SUMCHECK_MAX_FACTORS + 1) * nl, evals_words, evals_off, nl) || !span_ok(need * nl, work_words, work_off, nl)) return H_BAD_ARGS;
  }
  DevBuf d_in, d_out, d_evals, d_work;
  const uint32_t* ins[lcpc::SUMCHECK_MAX_TABLES];
  uint32_t* outs[lcpc::SUMCHECK_MAX_TABLES];
  if (bind) H_TRY(d_out.put(out, n_tables * slot_words * 4));
  if (round) {
    H_TRY(d_evals.put(evals, evals_words * 4));
    H_TRY(d_work.put(work, work_words * 4));
  }
  if (!in_place) H_TRY(d_in.put(in, n_tables * words * 4));
  for (uint32_t j = 0; j < n_tables; j++) {
    outs[j] = bind ? d_out.p + j * slot_words + out_off : nullptr;
    if (in_place) {
      H_TRY(hipMemcpy(outs[j], in + j * words, words * 4, hipMemcpyHostToDevice));
      ins[j] = outs[j];
    } else {
      ins[j] = d_in.p + j * words;
    }
  }
  if (n_launches) *n_launches = 0;
  if (mode == MODE_BIND) {
    H_TRY(lcpc::launch_sumcheck_bind(nl, order, ins, outs, n_tables, n, r, nullptr));
    if (n_launches) *n_launches = 1;
  } else if (mode == MODE_ROUND) {
    H_TRY(lcpc::launch_sumcheck_round(nl, order, ins, n_tables, tm, n_terms, coeffs, one, n, d_evals.p + evals_off, d_work.p + work_off, need, max_groups,
                                         nullptr, n_launches));
  } else {
    H_TRY(lcpc::launch_sumcheck_bind_round(nl, order, ins, outs, n_tables, tm, n_terms, coeffs, one, n, r, d_evals.p + evals_off, d_work.p + work_off, need,
                                              max_groups, nullptr, n_launches));
  }
  H_TRY(hipDeviceSynchronize());
  if (!in_place) H_TRY(d_in.get(in, n_tables * words * 4));
  if (round) {
    H_TRY(d_evals.get(evals, evals_words * 4));
    H_TRY(d_work.get(work, work_words * 4));
  }
  return bind ? (int)d_out.get(out, n_tables * slot_words * 4) : 0;
}

// What a launcher answers to a job it must settle before any launch -- so this refuses (H_BAD_ARGS) every job a correct launcher
// would launch.  null_mask / misalign: bit 0 the array `in`, 1 in[0], 2 the array `out`, 3 out[0], 4 evals, 5 work, 6 one, 7 r, 8 terms
// (misalign: bits 1, 3, 4, 5).  overlap: 1 out[0] is in[0] (in place); 2 out[0] starts one element behind in[0]; 3 out[1] is out[0];
// 4 evals lies in in[0]; 5 work starts at out[0]; 6 evals is work; 7 out[0] is in[1]; 8 in[1] is in[0] and out[0] too; 9 out[0] is the upper half
// of in[0]; 10 evals lies in out[0].  short_work: work_elems is one less than needed.  The pointers point at words nothing reads.  Returns the
// launcher's hipError_t
H_EXPORT int k18h_refusal(int mode, int nl, int order, uint64_t n, uint32_t n_tables, const uint32_t* terms, uint32_t n_terms, uint32_t null_mask,
                          uint32_t misalign, int overlap, int short_work, uint32_t max_groups) {
  if (mode < MODE_BIND || mode > MODE_FUSED || overlap < 0 || overlap > 10) return H_BAD_ARGS;
  const bool bind = mode != MODE_ROUND, round = mode != MODE_BIND;
  // the buffers lie far apart in an address range that is never touched: 2^44 bytes per buffer
  auto far = [&](unsigned slot, unsigned bit) -> uint32_t* {
    if ((null_mask >> bit) & 1u) return nullptr;
    return reinterpret_cast<uint32_t*>(((uintptr_t)(slot + 1) << 44) + 4 * ((misalign >> bit) & 1u));
  };
  const uint32_t* ins[lcpc::SUMCHECK_MAX_TABLES + 1];
  uint32_t* outs[lcpc::SUMCHECK_MAX_TABLES + 1];
  for (unsigned j = 0; j <= lcpc::SUMCHECK_MAX_TABLES; j++) {
    ins[j] = far(j, j == 0 ? 1 : 31);
    outs[j] = far(16 + j, j == 0 ? 3 : 31);
  }
  uint32_t *evals = far(40, 4), *work = far(41, 5);
  const uint64_t words = lcpc::nl_ok(nl) && n < ((uint64_t)1 << 39) ? n * nl : 0;
  const int enl = lcpc::nl_ok(nl) ? nl : 2;
  if (overlap == 1) outs[0] = const_cast<uint32_t*>(ins[0]);
  if (overlap == 2) outs[0] = const_cast<uint32_t*>(ins[0]) + enl;
  if (overlap == 3) outs[1] = outs[0];
  if (overlap == 4) evals = const_cast<uint32_t*>(ins[0]) + enl;
  if (overlap == 5) work = outs[0];
  if (overlap == 6) evals = work;
  if (overlap == 7) outs[0] = const_cast<uint32_t*>(ins[1]);
  if (overlap == 8) { ins[1] = ins[0]; outs[0] = const_cast<uint32_t*>(ins[0]); }
  if (overlap == 9) outs[0] = const_cast<uint32_t*>(ins[0]) + words / 2;
  if (overlap == 10) evals = outs[0] + enl;
  const lcpc::SumcheckTerm* tm = (null_mask >> 8) & 1u ? nullptr : reinterpret_cast<const lcpc::SumcheckTerm*>(terms);
  alignas(16) static const uint32_t one[8] = {1, 0, 0, 0, 0, 0, 0, 0};
  const uint32_t* onep = (null_mask >> 6) & 1u ? nullptr : one;
  const uint32_t* rp = (null_mask >> 7) & 1u ? nullptr : one;
  const uint64_t pairs = mode == MODE_FUSED ? n / 4 : n / 2;
  uint64_t need = round && n_terms && n_terms <= lcpc::SUMCHECK_MAX_TERMS && max_groups && pairs ? lcpc::sumcheck_work_elems(pairs, n_terms, max_groups) : 1;
  if (short_work) need -= 1;
  const lcpc::SumcheckJob j = {nl, order, bind, round, (null_mask & 1u) ? nullptr : ins, (null_mask & 4u) ? nullptr : outs, n_tables, tm, n_terms, n, evals, work,
                               need, max_groups};
  // the job is one the launcher settles on the host: by its own test of the shape, or by a missing one / r
  const bool settled = !lcpc::sumcheck_job_ok(j) || (round && !onep) || (bind && !rp);
  if (!settled) return H_BAD_ARGS;
  if (mode == MODE_BIND) return (int)lcpc::launch_sumcheck_bind(nl, order, j.in, j.out, n_tables, n, rp, nullptr);
  if (mode == MODE_ROUND) return (int)lcpc::launch_sumcheck_round(nl, order, j.in, n_tables, tm, n_terms, nullptr, onep, n, evals, work, need, max_groups, nullptr, nullptr);
  return (int)lcpc::launch_sumcheck_bind_round(nl, order, j.in, j.out, n_tables, tm, n_terms, nullptr, onep, n, rp, evals, work, need, max_groups, nullptr, nullptr);
}

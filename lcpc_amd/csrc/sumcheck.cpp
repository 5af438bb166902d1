// lcpc_amd/csrc/sumcheck.cpp -- the sumcheck extension of the C ABI (include/lcpc_hip_sumcheck.h): the round sums and the binding of a
// variable on the host (sumcheck_host.h, no HIP call) and on the device (K18 / K19, sumcheck.hip).  Every refusal is settled on the
// host before anything is enqueued: the shape of the job by sumcheck_job_ok (kernels.h), which the launchers run as well, the
// values of r and the coefficients here.  lcpcm_round_work_bytes is the one place that knows the size of the workspace.
#include <stddef.h>

#include "internal.h"
#include "sumcheck_host.h"
#include "../../include/lcpc_hip_domain.h"
#include "../../include/lcpc_hip_sumcheck.h"

using namespace lcpc;

static_assert(LCPCM_LOW_FIRST == SUMCHECK_LOW_FIRST && LCPCM_HIGH_FIRST == SUMCHECK_HIGH_FIRST && LCPCM_LOW_FIRST == HM_LOW_FIRST &&
                  LCPCM_HIGH_FIRST == HM_HIGH_FIRST,
              "lcpcm_order, the launcher's values and the host's are one numbering");
static_assert(LCPCM_MAX_TABLES == SUMCHECK_MAX_TABLES && LCPCM_MAX_TERMS == SUMCHECK_MAX_TERMS && LCPCM_MAX_FACTORS == SUMCHECK_MAX_FACTORS &&
                  LCPCM_MAX_TABLES == HM_MAX_TABLES && LCPCM_MAX_TERMS == HM_MAX_TERMS && LCPCM_MAX_FACTORS == HM_MAX_FACTORS,
              "the limits of a composition are one set");
static_assert(sizeof(lcpcm_term) == sizeof(SumcheckTerm) && sizeof(lcpcm_term) == sizeof(HmTerm) && offsetof(lcpcm_term, table) == offsetof(SumcheckTerm, table) &&
                  offsetof(lcpcm_term, table) == offsetof(HmTerm, table),
              "lcpcm_term, the launcher's term and the host's are one layout");

namespace {

inline const uint32_t* words(const uint64_t* p) { return reinterpret_cast<const uint32_t*>(p); }
inline uint32_t* words(uint64_t* p) { return reinterpret_cast<uint32_t*>(p); }
inline const SumcheckTerm* dev_terms(const lcpcm_term* t) { return reinterpret_cast<const SumcheckTerm*>(t); }
inline const HmTerm* host_terms(const lcpcm_term* t) { return reinterpret_cast<const HmTerm*>(t); }

// host limbs that travel as kernel arguments: n elements, each below p (null: none given)
bool limbs_ok(const FieldDesc& f, const uint64_t* e, uint32_t n) { return !e || elems_reduced(f, e, n); }

// the job of a device call, or false: the context, the pointer arrays themselves and the limits that guard reading them
struct DevJob {
  const uint32_t* in[SUMCHECK_MAX_TABLES];
  uint32_t* out[SUMCHECK_MAX_TABLES];
  SumcheckJob j;
};
bool dev_job(DevJob* dj, const lcpc_ctx* c, uint32_t order, bool bind, bool round, const uint64_t* const* in_dev, uint64_t* const* out_dev,
             uint32_t n_tables, const lcpcm_term* terms, uint32_t n_terms, uint64_t n, const uint64_t* evals_dev, const void* work_dev,
             uint64_t work_bytes) {
  if (!c || order > LCPCM_HIGH_FIRST || !in_dev || (bind && !out_dev) || n_tables == 0 || n_tables > LCPCM_MAX_TABLES) return false;
  for (uint32_t t = 0; t < n_tables; t++) {
    dj->in[t] = words(in_dev[t]);
    dj->out[t] = bind ? words(out_dev[t]) : nullptr;
  }
  dj->j = {c->NL, (int)order, bind, round, dj->in, bind ? dj->out : nullptr, n_tables, dev_terms(terms), n_terms, n, words(evals_dev),
           static_cast<const uint32_t*>(work_dev), work_bytes / elem_bytes(c), SUMCHECK_GROUPS};
  return sumcheck_job_ok(dj->j);
}

}  // namespace

extern "C" {

int lcpcm_version(void) { return LCPCM_VERSION; }

int lcpcm_bind(uint32_t field, uint32_t order, const uint64_t* in, uint64_t* out, uint64_t n, const uint64_t* r) {
  const FieldDesc* f = field_desc((int)field);
  if (!f || order > LCPCM_HIGH_FIRST || !in || !out || !r || !hm_len_ok(n, 2) || h_ge_p(*f, r)) return LCPC_ERR_ARG;
  // out == in, or clear of it: the n / 2 outputs against the n inputs
  if (out != in && ranges_meet(in, n * 8 * f->L, out, n / 2 * 8 * f->L)) return LCPC_ERR_ARG;
  if (!elems_reduced(*f, in, n)) return LCPC_ERR_ARG;
  host_bind(*f, order, in, out, n, r);
  return 0;
}

int lcpcm_round(uint32_t field, uint32_t order, const uint64_t* const* tables, uint32_t n_tables, const lcpcm_term* terms, uint32_t n_terms,
                const uint64_t* coeffs, uint64_t n, uint64_t* evals) {
  const FieldDesc* f = field_desc((int)field);
  if (!f || order > LCPCM_HIGH_FIRST || !tables || !evals || !hm_len_ok(n, 2)) return LCPC_ERR_ARG;
  const uint32_t d = hm_degree(n_tables, host_terms(terms), n_terms);
  if (d == 0 || !limbs_ok(*f, coeffs, n_terms)) return LCPC_ERR_ARG;
  for (uint32_t t = 0; t < n_tables; t++) {
    if (!tables[t] || ranges_meet(tables[t], n * 8 * f->L, evals, (uint64_t)(d + 1) * 8 * f->L)) return LCPC_ERR_ARG;
    if (!elems_reduced(*f, tables[t], n)) return LCPC_ERR_ARG;
  }
  host_round(*f, order, tables, host_terms(terms), n_terms, coeffs, n, d, evals);
  return 0;
}

uint64_t lcpcm_round_work_bytes(const lcpc_ctx* c, uint64_t n, uint32_t n_terms) {
  if (!c || !hm_len_ok(n, 2) || n_terms == 0 || n_terms > LCPCM_MAX_TERMS) return 0;
  return sumcheck_work_elems(n / 2, n_terms, SUMCHECK_GROUPS) * elem_bytes(c);
}

int lcpcm_bind_device(lcpc_ctx* c, uint32_t order, const uint64_t* const* in_dev, uint64_t* const* out_dev, uint32_t n_tables, uint64_t n,
                      const uint64_t* r, void* stream) {
  DevJob dj;
  if (!dev_job(&dj, c, order, true, false, in_dev, out_dev, n_tables, nullptr, 0, n, nullptr, nullptr, 0)) return LCPC_ERR_ARG;
  if (!r || h_ge_p(*c->f, r)) return LCPC_ERR_ARG;
  LCPC_TRY
  HIPCHK(c, hipSetDevice(c->prm.device));
  HIPCHK(c, launch_sumcheck_bind(c->NL, (int)order, dj.in, dj.out, n_tables, n, words(r), (hipStream_t)stream));
  return 0;
  LCPC_CATCH(c)
}

int lcpcm_round_device(lcpc_ctx* c, uint32_t order, const uint64_t* const* tables_dev, uint32_t n_tables, const lcpcm_term* terms,
                       uint32_t n_terms, const uint64_t* coeffs, uint64_t n, uint64_t* evals_dev, void* work_dev, uint64_t work_bytes,
                       void* stream) {
  DevJob dj;
  if (!dev_job(&dj, c, order, false, true, tables_dev, nullptr, n_tables, terms, n_terms, n, evals_dev, work_dev, work_bytes)) return LCPC_ERR_ARG;
  if (!limbs_ok(*c->f, coeffs, n_terms)) return LCPC_ERR_ARG;
  LCPC_TRY
  HIPCHK(c, hipSetDevice(c->prm.device));
  HIPCHK(c, launch_sumcheck_round(c->NL, (int)order, dj.in, n_tables, dj.j.terms, n_terms, words(coeffs), words(c->f->r), n, words(evals_dev),
                                  static_cast<uint32_t*>(work_dev), dj.j.work_elems, SUMCHECK_GROUPS, (hipStream_t)stream, nullptr));
  return 0;
  LCPC_CATCH(c)
}

int lcpcm_bind_round_device(lcpc_ctx* c, uint32_t order, const uint64_t* const* in_dev, uint64_t* const* out_dev, uint32_t n_tables,
                            const lcpcm_term* terms, uint32_t n_terms, const uint64_t* coeffs, uint64_t n, const uint64_t* r,
                            uint64_t* evals_dev, void* work_dev, uint64_t work_bytes, void* stream) {
  DevJob dj;
  if (!dev_job(&dj, c, order, true, true, in_dev, out_dev, n_tables, terms, n_terms, n, evals_dev, work_dev, work_bytes)) return LCPC_ERR_ARG;
  if (!r || h_ge_p(*c->f, r) || !limbs_ok(*c->f, coeffs, n_terms)) return LCPC_ERR_ARG;
  LCPC_TRY
  HIPCHK(c, hipSetDevice(c->prm.device));
  HIPCHK(c, launch_sumcheck_bind_round(c->NL, (int)order, dj.in, dj.out, n_tables, dj.j.terms, n_terms, words(coeffs), words(c->f->r), n, words(r),
                                       words(evals_dev), static_cast<uint32_t*>(work_dev), dj.j.work_elems, SUMCHECK_GROUPS, (hipStream_t)stream,
                                       nullptr));
  return 0;
  LCPC_CATCH(c)
}

}  // extern "C"

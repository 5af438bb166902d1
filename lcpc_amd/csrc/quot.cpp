// lcpc_amd/csrc/quot.cpp -- the quotient extension of the C ABI (include/lcpc_hip_quot.h): batch inversion, pointwise arithmetic and the
// division of values on a domain by X - z or X^n - 1, on the host (quot_host.h, no HIP call) and on the device (K15 / K16, quot.hip)
// with the context's forward twiddle table (fft.cpp fft_table).  Every refusal, the tests on z and the shift included, is settled on the
// host before anything is enqueued.
#include "internal.h"
#include "quot_host.h"
#include "../../include/lcpc_hip_domain.h"
#include "../../include/lcpc_hip_quot.h"

using namespace lcpc;

static_assert(LCPCQ_ADD == QUOT_ADD && LCPCQ_SUB == QUOT_SUB && LCPCQ_MUL == QUOT_MUL && LCPCQ_DIV == QUOT_DIV && LCPCQ_ADD == HQ_ADD &&
                  LCPCQ_SUB == HQ_SUB && LCPCQ_MUL == HQ_MUL && LCPCQ_DIV == HQ_DIV,
              "lcpcq_op, the launcher's ops and the host's are one numbering");

namespace {

inline bool elem_ok(const FieldDesc& f, const uint64_t* e) { return e && !h_ge_p(f, e); }
inline const uint32_t* words(const uint64_t* p) { return reinterpret_cast<const uint32_t*>(p); }

// what the two device divisions refuse alike; *total: elements of the output
bool divide_dims_ok(const lcpc_ctx* c, uint32_t order, const uint64_t* in_dev, uint64_t* out_dev, uint32_t log_m, uint32_t n_vecs, uint64_t* total) {
  return order <= LCPCD_BITREV && dev_vectors_ok(c, in_dev, out_dev, log_m, n_vecs, total);
}

// K16 on `st` with the context's forward table of 2^log_m points (takes c->mu)
int divide_enqueue(lcpc_ctx* c, int kind, uint32_t order, uint32_t log_m, uint32_t log_n, uint32_t n_vecs, const uint64_t* in_dev, uint64_t* out_dev,
                   const uint64_t* shift, const uint64_t* z, const uint64_t* y_dev, hipStream_t st) {
  std::lock_guard<std::mutex> g(c->mu);
  const uint32_t* tab = nullptr;
  if (log_m) {
    int rc = fft_table(c, &c->err, log_m, false, &tab);
    if (rc) return rc;
  }
  hipError_t e = launch_domain_quotient(c->NL, kind, order == LCPCD_BITREV, log_m, log_n, n_vecs, words(in_dev), reinterpret_cast<uint32_t*>(out_dev),
                                        tab, words(shift), words(z), words(y_dev), st);
  if (e != hipSuccess) return fail_hip(&c->err, e, "launch_domain_quotient");
  return 0;
}

}  // namespace

extern "C" {

int lcpcq_version(void) { return LCPCQ_VERSION; }

int lcpcq_batch_inverse(uint32_t field, const uint64_t* in, uint64_t* out, uint64_t n) {
  const FieldDesc* f = field_desc((int)field);
  if (!f || !in || !out || n == 0 || n >= ((uint64_t)1 << 39)) return LCPC_ERR_ARG;
  if (ranges_overlap(in, out, n * 8 * f->L) || !elems_reduced(*f, in, n)) return LCPC_ERR_ARG;
  try {
    host_batch_inverse(*f, in, out, n);
  } catch (const std::exception&) {
    return LCPC_ERR_NOMEM;
  }
  return 0;
}

int lcpcq_pointwise(uint32_t field, uint32_t op, const uint64_t* a, const uint64_t* b, uint64_t* out, uint64_t n) {
  const FieldDesc* f = field_desc((int)field);
  if (!f || op > LCPCQ_DIV || !a || !b || !out || n == 0 || n >= ((uint64_t)1 << 39)) return LCPC_ERR_ARG;
  const uint64_t bytes = n * 8 * f->L;
  if (ranges_overlap(a, out, bytes) || ranges_overlap(b, out, bytes)) return LCPC_ERR_ARG;
  if (!elems_reduced(*f, a, n) || !elems_reduced(*f, b, n)) return LCPC_ERR_ARG;
  try {
    host_pointwise(*f, op, a, b, out, n);
  } catch (const std::exception&) {
    return LCPC_ERR_NOMEM;
  }
  return 0;
}

int lcpcq_divide_linear(uint32_t field, const uint64_t* shift, uint32_t order, const uint64_t* in, uint32_t log_m, const uint64_t* z,
                        const uint64_t* y, uint64_t* out) {
  const FieldDesc* f = field_desc((int)field);
  if (!f || order > LCPCD_BITREV || (shift && !shift_ok(*f, shift)) || !in || !out || log_m > f->S) return LCPC_ERR_ARG;
  if (!elem_ok(*f, z) || !elem_ok(*f, y)) return LCPC_ERR_ARG;
  const uint64_t m = (uint64_t)1 << log_m;
  if (ranges_overlap(in, out, m * 8 * f->L) || !elems_reduced(*f, in, m) || z_on_domain(*f, shift, z, log_m)) return LCPC_ERR_ARG;
  try {
    uint64_t s[MAXL], zz[MAXL], yy[MAXL];               // (shift, z and y may lie in the output)
    if (shift) memcpy(s, shift, 8 * f->L);
    memcpy(zz, z, 8 * f->L);
    memcpy(yy, y, 8 * f->L);
    std::vector<uint64_t> den((size_t)m * f->L);
    linear_denominators(*f, shift ? s : nullptr, order == LCPCD_BITREV, log_m, zz, den.data());
    host_divide(*f, in, yy, den.data(), out, m);
  } catch (const std::exception&) {
    return LCPC_ERR_NOMEM;
  }
  return 0;
}

int lcpcq_divide_vanishing(uint32_t field, const uint64_t* shift, uint32_t order, const uint64_t* in, uint32_t log_m, uint32_t log_n,
                           uint64_t* out) {
  const FieldDesc* f = field_desc((int)field);
  if (!f || order > LCPCD_BITREV || !shift_ok(*f, shift) || !in || !out || log_m > f->S || log_n > log_m) return LCPC_ERR_ARG;
  const uint64_t m = (uint64_t)1 << log_m;
  if (ranges_overlap(in, out, m * 8 * f->L) || !elems_reduced(*f, in, m) || shift_on_subgroup(*f, shift, log_m)) return LCPC_ERR_ARG;
  try {
    uint64_t s[MAXL];
    memcpy(s, shift, 8 * f->L);
    std::vector<uint64_t> den((size_t)m * f->L);
    vanishing_denominators(*f, s, order == LCPCD_BITREV, log_m, log_n, den.data());
    host_divide(*f, in, nullptr, den.data(), out, m);
  } catch (const std::exception&) {
    return LCPC_ERR_NOMEM;
  }
  return 0;
}

int lcpcq_batch_inverse_device(lcpc_ctx* c, const uint64_t* in_dev, uint64_t* out_dev, uint64_t n, void* stream) {
  if (!c || !in_dev || !out_dev || !dev_aligned(in_dev, c->L) || !dev_aligned(out_dev, c->L)) return LCPC_ERR_ARG;
  if (n == 0 || n >= ((uint64_t)1 << 39) || ranges_overlap(in_dev, out_dev, n * elem_bytes(c))) return LCPC_ERR_ARG;
  LCPC_TRY
  HIPCHK(c, hipSetDevice(c->prm.device));
  HIPCHK(c, launch_batch_inverse(c->NL, words(in_dev), reinterpret_cast<uint32_t*>(out_dev), n, (hipStream_t)stream));
  return 0;
  LCPC_CATCH(c)
}

int lcpcq_pointwise_device(lcpc_ctx* c, uint32_t op, const uint64_t* a_dev, const uint64_t* b_dev, uint64_t* out_dev, uint64_t n, void* stream) {
  if (!c || op > LCPCQ_DIV || !a_dev || !b_dev || !out_dev) return LCPC_ERR_ARG;
  if (!dev_aligned(a_dev, c->L) || !dev_aligned(b_dev, c->L) || !dev_aligned(out_dev, c->L) || n == 0 || n >= ((uint64_t)1 << 39)) return LCPC_ERR_ARG;
  if (ranges_overlap(a_dev, out_dev, n * elem_bytes(c)) || ranges_overlap(b_dev, out_dev, n * elem_bytes(c))) return LCPC_ERR_ARG;
  LCPC_TRY
  HIPCHK(c, hipSetDevice(c->prm.device));
  HIPCHK(c, launch_pointwise(c->NL, (int)op, words(a_dev), words(b_dev), reinterpret_cast<uint32_t*>(out_dev), n, (hipStream_t)stream));
  return 0;
  LCPC_CATCH(c)
}

int lcpcq_divide_linear_device(lcpc_ctx* c, const uint64_t* shift, uint32_t order, const uint64_t* in_dev, uint32_t log_m, uint32_t n_vecs,
                               const uint64_t* z, const uint64_t* y_dev, uint64_t* out_dev, void* stream) {
  uint64_t total = 0;
  if (!c || (shift && !shift_ok(*c->f, shift)) || !elem_ok(*c->f, z) || !y_dev || !dev_aligned(y_dev, c->L)) return LCPC_ERR_ARG;
  if (!divide_dims_ok(c, order, in_dev, out_dev, log_m, n_vecs, &total)) return LCPC_ERR_ARG;
  if (ranges_meet(y_dev, n_vecs * elem_bytes(c), out_dev, total * elem_bytes(c)) || z_on_domain(*c->f, shift, z, log_m)) return LCPC_ERR_ARG;
  LCPC_TRY
  HIPCHK(c, hipSetDevice(c->prm.device));
  return divide_enqueue(c, QUOT_LINEAR, order, log_m, 0, n_vecs, in_dev, out_dev, shift, z, y_dev, (hipStream_t)stream);
  LCPC_CATCH(c)
}

int lcpcq_divide_vanishing_device(lcpc_ctx* c, const uint64_t* shift, uint32_t order, const uint64_t* in_dev, uint32_t log_m, uint32_t log_n,
                                  uint32_t n_vecs, uint64_t* out_dev, void* stream) {
  uint64_t total = 0;
  if (!c || !shift_ok(*c->f, shift) || log_n > log_m) return LCPC_ERR_ARG;
  if (!divide_dims_ok(c, order, in_dev, out_dev, log_m, n_vecs, &total) || shift_on_subgroup(*c->f, shift, log_m)) return LCPC_ERR_ARG;
  LCPC_TRY
  HIPCHK(c, hipSetDevice(c->prm.device));
  uint64_t sn[MAXL] = {0, 0, 0, 0};
  h_pow(*c->f, sn, shift, (uint64_t)1 << log_n);
  return divide_enqueue(c, QUOT_VANISH, order, log_m, log_n, n_vecs, in_dev, out_dev, sn, nullptr, nullptr, (hipStream_t)stream);
  LCPC_CATCH(c)
}

}  // extern "C"

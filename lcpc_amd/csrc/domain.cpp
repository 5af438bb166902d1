// lcpc_amd/csrc/domain.cpp -- the domain extension of the C ABI (include/lcpc_hip_domain.h): coset transforms and the extension on
// the host (fft_host.h, no HIP call) and on the device (K14, domain.hip) with the context's cache of shift tables (fft.cpp
// cached_table), the low-degree extension built from the two, the commit entry points that read values on a coset (fft.cpp
// commit_evals_entry) and the reader that writes a commitment's values on a domain.
#include "internal.h"
#include "fft_host.h"
#include "../../include/lcpc_hip_domain.h"
#include "../../include/lcpc_hip_fft.h"

using namespace lcpc;

static_assert((int)LCPCD_NATURAL == (int)LCPCF_NATURAL && (int)LCPCD_BITREV == (int)LCPCF_BITREV,
              "commit_evals_entry (fft.cpp) reads both extensions' orders");
static_assert(LCPCD_FFT_II == FFT_FFT_II && LCPCD_FFT_IO == FFT_FFT_IO && LCPCD_FFT_OI == FFT_FFT_OI && LCPCD_IFFT_II == FFT_IFFT_II &&
                  LCPCD_IFFT_IO == FFT_IFFT_IO && LCPCD_IFFT_OI == FFT_IFFT_OI,
              "lcpcd_form and the launcher's forms are one numbering");

namespace {

// the context's shift table of (shift, log_n, direction), c->mu held: cached_table (fft.cpp) on t = shift forward, t = shift^-1 with
// n^-1 in the upper level inverse
int dom_table(lcpc_ctx* c, ErrText* err, const uint64_t* shift, uint32_t log_n, bool inverse, const uint32_t** tab) {
  return cached_table(c, err, c->dom_tabs, 8, shift, log_n, inverse,
                      [](const FieldDesc& f, const uint64_t* shift, uint32_t log_n, bool inverse, uint64_t* v, uint64_t* factor) {
                        if (inverse) { h_inv(f, v, shift); n_inverse(f, log_n, factor); } else memcpy(v, shift, 8 * f.L);
                        return inverse;
                      }, tab);
}

// what lcpcd_extend_device refuses beyond pointers, order and shift; *total: elements of the output
bool extend_dims_ok(const FieldDesc& f, uint64_t n_coeffs, uint32_t log_m, uint32_t n_vecs, uint64_t* total) {
  if (log_m > dev_max_log_n(f) || n_coeffs == 0 || n_coeffs > ((uint64_t)1 << log_m) || n_vecs == 0) return false;
  if (((uint64_t)n_vecs << (log_m - ext_src_log(n_coeffs))) > 65535) return false;
  *total = (uint64_t)n_vecs << log_m;
  return *total < ((uint64_t)1 << 39);
}

}  // namespace

int lcpc::coset_enqueue(lcpc_ctx* c, ErrText* err, int form, const uint64_t* shift, const uint32_t* in, uint32_t* out, uint32_t log_n,
                        uint32_t n_vecs, hipStream_t st) {
  std::lock_guard<std::mutex> g(c->mu);
  const uint32_t *tab = nullptr, *stab = nullptr;
  if (log_n) {
    int rc = fft_table(c, err, log_n, form_inverse((uint32_t)form), &tab);
    if (rc) return rc;
    if ((rc = dom_table(c, err, shift, log_n, form_inverse((uint32_t)form), &stab))) return rc;
  }
  hipError_t e = launch_coset_fft(c->NL, form, log_n, FFT_MAX_LOG_TILE, n_vecs, in, out, tab, stab, st, nullptr);
  if (e != hipSuccess) return fail_hip(err, e, "launch_coset_fft");
  return 0;
}

int lcpc::extend_enqueue(lcpc_ctx* c, ErrText* err, const uint64_t* shift, const uint32_t* coeffs, uint64_t n_coeffs, uint32_t log_m,
                         bool natural, uint32_t* out, uint32_t n_vecs, hipStream_t st) {
  std::lock_guard<std::mutex> g(c->mu);
  const uint32_t *tab = nullptr, *stab = nullptr;
  if (log_m) {
    int rc = fft_table(c, err, log_m, false, &tab);
    if (rc) return rc;
    if ((rc = dom_table(c, err, shift, ext_log_n(n_coeffs, log_m), false, &stab))) return rc;
  }
  hipError_t e = launch_extend(c->NL, n_coeffs, log_m, natural ? 1 : 0, FFT_MAX_LOG_TILE, n_vecs, coeffs, out, tab, stab, st, nullptr);
  if (e != hipSuccess) return fail_hip(err, e, "launch_extend");
  return 0;
}

extern "C" {

int lcpcd_version(void) { return LCPCD_VERSION; }

int lcpcd_generator(uint32_t field, uint64_t* out) {
  const FieldDesc* f = field_desc((int)field);
  if (!f || !out) return LCPC_ERR_ARG;
  host_generator(*f, out);
  return 0;
}

int lcpcd_coset_fft(uint32_t field, uint32_t form, const uint64_t* shift, const uint64_t* in, uint64_t* out, uint32_t log_n) {
  const FieldDesc* f = field_desc((int)field);
  if (!f || form > LCPCD_IFFT_OI || !shift_ok(*f, shift) || !in || !out || log_n > f->S) return LCPC_ERR_ARG;
  const uint64_t n = (uint64_t)1 << log_n;
  if (ranges_overlap(in, out, n * 8 * f->L) || !elems_reduced(*f, in, n)) return LCPC_ERR_ARG;
  try {
    const std::vector<uint64_t> s(shift, shift + f->L);       // (the shift may lie in the output)
    std::vector<uint64_t> a(in, in + (size_t)n * f->L);
    host_coset_fft(*f, form, s.data(), a.data(), log_n);
    memcpy(out, a.data(), a.size() * 8);
  } catch (const std::exception&) {
    return LCPC_ERR_NOMEM;
  }
  return 0;
}

int lcpcd_extend(uint32_t field, const uint64_t* shift, const uint64_t* coeffs, uint64_t n_coeffs, uint32_t log_m, uint32_t order,
                 uint64_t* out) {
  const FieldDesc* f = field_desc((int)field);
  if (!f || order > LCPCD_BITREV || !shift_ok(*f, shift) || !coeffs || !out || log_m > f->S) return LCPC_ERR_ARG;
  const uint64_t m = (uint64_t)1 << log_m;
  if (n_coeffs == 0 || n_coeffs > m) return LCPC_ERR_ARG;
  if (coeffs != out && ranges_meet(coeffs, n_coeffs * 8 * f->L, out, m * 8 * f->L)) return LCPC_ERR_ARG;
  if (!elems_reduced(*f, coeffs, n_coeffs)) return LCPC_ERR_ARG;
  try {
    const std::vector<uint64_t> s(shift, shift + f->L);
    std::vector<uint64_t> a((size_t)m * f->L);
    memcpy(a.data(), coeffs, (size_t)n_coeffs * 8 * f->L);
    host_extend(*f, s.data(), a.data(), n_coeffs, log_m, order == LCPCD_BITREV);
    memcpy(out, a.data(), a.size() * 8);
  } catch (const std::exception&) {
    return LCPC_ERR_NOMEM;
  }
  return 0;
}

int lcpcd_coset_fft_device(lcpc_ctx* c, uint32_t form, const uint64_t* shift, const uint64_t* in_dev, uint64_t* out_dev, uint32_t log_n,
                           uint32_t n_vecs, void* stream) {
  uint64_t total = 0;
  if (!c || form > LCPCD_IFFT_OI || !shift_ok(*c->f, shift) || !dev_vectors_ok(c, in_dev, out_dev, log_n, n_vecs, &total)) return LCPC_ERR_ARG;
  LCPC_TRY
  HIPCHK(c, hipSetDevice(c->prm.device));
  return coset_enqueue(c, &c->err, (int)form, shift, reinterpret_cast<const uint32_t*>(in_dev), reinterpret_cast<uint32_t*>(out_dev), log_n,
                       n_vecs, (hipStream_t)stream);
  LCPC_CATCH(c)
}

int lcpcd_extend_device(lcpc_ctx* c, const uint64_t* shift, const uint64_t* coeffs_dev, uint64_t n_coeffs, uint32_t log_m, uint32_t order,
                        uint64_t* out_dev, uint32_t n_vecs, void* stream) {
  if (!c || order > LCPCD_BITREV || !shift_ok(*c->f, shift) || !coeffs_dev || !out_dev) return LCPC_ERR_ARG;
  if (!dev_aligned(coeffs_dev, c->L) || !dev_aligned(out_dev, c->L)) return LCPC_ERR_ARG;
  uint64_t total = 0;
  if (!extend_dims_ok(*c->f, n_coeffs, log_m, n_vecs, &total)) return LCPC_ERR_ARG;
  if (ranges_meet(coeffs_dev, ext_src_elems(n_coeffs, n_vecs) * elem_bytes(c), out_dev, total * elem_bytes(c))) return LCPC_ERR_ARG;
  LCPC_TRY
  HIPCHK(c, hipSetDevice(c->prm.device));
  return extend_enqueue(c, &c->err, shift, reinterpret_cast<const uint32_t*>(coeffs_dev), n_coeffs, log_m, order == LCPCD_NATURAL,
                        reinterpret_cast<uint32_t*>(out_dev), n_vecs, (hipStream_t)stream);
  LCPC_CATCH(c)
}

int lcpcd_lde_device(lcpc_ctx* c, uint32_t in_order, const uint64_t* shift_in, const uint64_t* in_dev, uint32_t log_n, const uint64_t* shift_out,
                     uint32_t log_m, uint32_t out_order, uint64_t* out_dev, uint64_t* work_dev, uint32_t n_vecs, void* stream) {
  if (!c || in_order > LCPCD_BITREV || out_order > LCPCD_BITREV || !in_dev || !out_dev || !work_dev) return LCPC_ERR_ARG;
  if ((shift_in && !shift_ok(*c->f, shift_in)) || !shift_ok(*c->f, shift_out)) return LCPC_ERR_ARG;
  if (!dev_aligned(in_dev, c->L) || !dev_aligned(out_dev, c->L) || !dev_aligned(work_dev, c->L)) return LCPC_ERR_ARG;
  if (log_m < log_n || n_vecs > 65535) return LCPC_ERR_ARG;
  uint64_t total = 0;
  if (!extend_dims_ok(*c->f, (uint64_t)1 << log_n, log_m, n_vecs, &total)) return LCPC_ERR_ARG;      // (log_n <= log_m <= 32)
  const uint64_t eb = elem_bytes(c), n_in = ((uint64_t)n_vecs << log_n) * eb;
  if (ranges_overlap(in_dev, work_dev, n_in) || ranges_meet(work_dev, n_in, out_dev, total * eb) || ranges_meet(in_dev, n_in, out_dev, total * eb))
    return LCPC_ERR_ARG;
  LCPC_TRY
  HIPCHK(c, hipSetDevice(c->prm.device));
  const int form = in_order == LCPCD_NATURAL ? FFT_IFFT_II : FFT_IFFT_OI;
  const uint32_t* in = reinterpret_cast<const uint32_t*>(in_dev);
  uint32_t* work = reinterpret_cast<uint32_t*>(work_dev);
  int rc = shift_in ? coset_enqueue(c, &c->err, form, shift_in, in, work, log_n, n_vecs, (hipStream_t)stream)
                    : fft_enqueue(c, &c->err, form, in, work, log_n, n_vecs, (hipStream_t)stream);
  if (rc) return rc;
  return extend_enqueue(c, &c->err, shift_out, work, (uint64_t)1 << log_n, log_m, out_order == LCPCD_NATURAL, reinterpret_cast<uint32_t*>(out_dev),
                        n_vecs, (hipStream_t)stream);
  LCPC_CATCH(c)
}

int lcpcd_commit_coset_evals_device(lcpc_commit_t* m, uint32_t order, const uint64_t* shift, const uint64_t* evals_dev, uint32_t log_n,
                                    void* stream, uint8_t* root) {
  return commit_evals_entry(m, order, true, shift, evals_dev, log_n, false, (hipStream_t)stream, root);
}

int lcpcd_commit_coset_evals(lcpc_commit_t* m, uint32_t order, const uint64_t* shift, const uint64_t* evals_host, uint32_t log_n, uint8_t* root) {
  return commit_evals_entry(m, order, true, shift, evals_host, log_n, true, nullptr, root);
}

int lcpcd_commit_values_device(lcpc_commit_t* m, const uint64_t* shift, uint32_t log_m, uint32_t order, uint64_t* out_dev, void* stream) {
  if (!m || !out_dev || order > LCPCD_BITREV) return LCPC_ERR_ARG;
  lcpc_ctx* c = m->enc;
  if (!shift_ok(*c->f, shift) || !dev_aligned(out_dev, c->L) || log_m > dev_max_log_n(*c->f)) return LCPC_ERR_ARG;
  if (c->prm.shard_count > 1) return LCPC_ERR_STATE;
  LCPC_TRY
  std::shared_lock<FillLock> rd(m->fill_mu);
  if (!m->committed) return LCPC_ERR_STATE;
  const uint64_t n_coeffs = m->n_rows_local * c->n_per_row;
  uint64_t total = 0;
  if (!extend_dims_ok(*c->f, n_coeffs, log_m, 1, &total)) return LCPC_ERR_ARG;
  if (ranges_meet(m->coeffs_view, n_coeffs * elem_bytes(c), out_dev, total * elem_bytes(c))) return LCPC_ERR_ARG;
  std::lock_guard<std::mutex> g(m->mu);
  HIPCHK(m, hipSetDevice(c->prm.device));
  int rc = order_after_commit(m, (hipStream_t)stream);
  if (rc) return rc;
  return extend_enqueue(c, &m->err, shift, m->coeffs_view, n_coeffs, log_m, order == LCPCD_NATURAL, reinterpret_cast<uint32_t*>(out_dev), 1,
                        (hipStream_t)stream);
  LCPC_CATCH(m)
}

}  // extern "C"

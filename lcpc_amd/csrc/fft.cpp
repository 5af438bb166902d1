// lcpc_amd/csrc/fft.cpp -- the transform extension of the C ABI (include/lcpc_hip_fft.h): the six FieldFFT forms on the host
// (fft_host.h, no HIP call) and on the device (K12 / K13, fft.hip) with the context's cache of two-level twiddle tables, and the
// two commit entry points that read evaluations.  The commit pipeline itself is commit.cpp's (commit_evals_locked).
#include "internal.h"
#include "fft_host.h"
#include "../../include/lcpc_hip_fft.h"

using namespace lcpc;

static_assert(LCPCF_FFT_II == FFT_FFT_II && LCPCF_FFT_IO == FFT_FFT_IO && LCPCF_FFT_OI == FFT_FFT_OI && LCPCF_IFFT_II == FFT_IFFT_II &&
                  LCPCF_IFFT_IO == FFT_IFFT_IO && LCPCF_IFFT_OI == FFT_IFFT_OI,
              "lcpcf_form and the launcher's forms are one numbering");

namespace {

inline bool dev_aligned(const void* p, int L) { return reinterpret_cast<uintptr_t>(p) % (L % 2 ? 8 : 16) == 0; }
inline uint32_t dev_max_log_n(const FieldDesc& f) { return f.S < FFT_MAX_LOG_N ? f.S : FFT_MAX_LOG_N; }

}  // namespace

// the context's table of (log_n, inverse), c->mu held: found, or built on the host, uploaded and put in place of the entry used
// longest ago
int lcpc::fft_table(lcpc_ctx* c, ErrText* err, uint32_t log_n, bool inverse, const uint32_t** tab) {
  FftTab* victim = &c->fft_tabs[0];
  for (auto& t : c->fft_tabs) {
    if (t.d && t.log_n == log_n && t.inverse == inverse) { t.stamp = ++c->fft_stamp; *tab = t.d; return 0; }
    if (!t.d ? victim->d != nullptr : (victim->d && t.stamp < victim->stamp)) victim = &t;
  }
  const FieldDesc& f = *c->f;
  const uint32_t h = fft_tab_split(log_n);
  const uint64_t n_lo = (uint64_t)1 << h, n_hi = (uint64_t)1 << (log_n - h);
  std::vector<uint64_t> host((size_t)(n_lo + n_hi) * f.L);
  uint64_t v[MAXL];
  root_of(f, log_n, inverse, v);
  powers(f, v, n_lo, host.data());
  h_pow(f, v, v, n_lo);
  powers(f, v, n_hi, host.data() + (size_t)n_lo * f.L);
  dev_free(victim->d);                 // (waits for whatever still reads it)
  victim->d = nullptr;
  int rc = dev_alloc(err, &victim->d, host.size() * 8);
  if (rc) return rc;
  hipError_t e = hipMemcpy(victim->d, host.data(), host.size() * 8, hipMemcpyHostToDevice);
  if (e != hipSuccess) { dev_free(victim->d); victim->d = nullptr; return fail_hip(err, e, "hipMemcpy (fft table)"); }
  victim->log_n = log_n; victim->inverse = inverse; victim->stamp = ++c->fft_stamp;
  *tab = victim->d;
  return 0;
}

int lcpc::fft_enqueue(lcpc_ctx* c, ErrText* err, int form, const uint32_t* in, uint32_t* out, uint32_t log_n, uint32_t n_vecs, hipStream_t st) {
  std::lock_guard<std::mutex> g(c->mu);
  const uint32_t* tab = nullptr;
  uint64_t ni[MAXL] = {0, 0, 0, 0};
  if (log_n) {
    int rc = fft_table(c, err, log_n, form_inverse((uint32_t)form), &tab);
    if (rc) return rc;
    if (form_inverse((uint32_t)form)) n_inverse(*c->f, log_n, ni);
  }
  hipError_t e = launch_fft(c->NL, form, log_n, FFT_MAX_LOG_TILE, n_vecs, in, out, tab, reinterpret_cast<const uint32_t*>(ni), st, nullptr);
  if (e != hipSuccess) return fail_hip(err, e, "launch_fft");
  return 0;
}

extern "C" {

int lcpcf_version(void) { return LCPCF_VERSION; }

uint32_t lcpcf_max_log_n(uint32_t field) {
  const FieldDesc* f = field_desc((int)field);
  return f ? f->S : 0;
}

int lcpcf_fft(uint32_t field, uint32_t form, const uint64_t* in, uint64_t* out, uint32_t log_n) {
  const FieldDesc* f = field_desc((int)field);
  if (!f || form > LCPCF_IFFT_OI || !in || !out || log_n > f->S) return LCPC_ERR_ARG;
  const uint64_t n = (uint64_t)1 << log_n;
  if (ranges_overlap(in, out, n * 8 * f->L) || !elems_reduced(*f, in, n)) return LCPC_ERR_ARG;
  try {
    std::vector<uint64_t> a(in, in + (size_t)n * f->L);
    host_fft(*f, form, a.data(), log_n);
    memcpy(out, a.data(), a.size() * 8);
  } catch (const std::exception&) {
    return LCPC_ERR_NOMEM;
  }
  return 0;
}

int lcpcf_fft_device(lcpc_ctx* c, uint32_t form, const uint64_t* in_dev, uint64_t* out_dev, uint32_t log_n, uint32_t n_vecs, void* stream) {
  if (!c || form > LCPCF_IFFT_OI || !in_dev || !out_dev || n_vecs == 0 || n_vecs > 65535) return LCPC_ERR_ARG;
  if (!dev_aligned(in_dev, c->L) || !dev_aligned(out_dev, c->L) || log_n > dev_max_log_n(*c->f)) return LCPC_ERR_ARG;
  const uint64_t total = (uint64_t)n_vecs << log_n;
  if (total >= ((uint64_t)1 << 39) || ranges_overlap(in_dev, out_dev, total * elem_bytes(c))) return LCPC_ERR_ARG;
  LCPC_TRY
  HIPCHK(c, hipSetDevice(c->prm.device));
  return fft_enqueue(c, &c->err, (int)form, reinterpret_cast<const uint32_t*>(in_dev), reinterpret_cast<uint32_t*>(out_dev), log_n, n_vecs,
                     (hipStream_t)stream);
  LCPC_CATCH(c)
}

int lcpcf_commit_evals_device(lcpc_commit_t* m, uint32_t order, const uint64_t* evals_dev, uint32_t log_n, void* stream, uint8_t* root) {
  if (!m || !evals_dev || order > LCPCF_BITREV) return LCPC_ERR_ARG;
  const lcpc_ctx* c = m->enc;
  if (!dev_aligned(evals_dev, c->L) || log_n > dev_max_log_n(*c->f)) return LCPC_ERR_ARG;
  if (c->prm.shard_count > 1) return LCPC_ERR_STATE;
  LCPC_TRY
  std::unique_lock<FillLock> fill(m->fill_mu);      // a fill: waits for the readers in flight (internal.h)
  std::lock_guard<std::mutex> g(m->mu);
  HIPCHK(m, hipSetDevice(c->prm.device));
  return commit_evals_locked(m, order == LCPCF_NATURAL ? FFT_IFFT_II : FFT_IFFT_OI, evals_dev, log_n, false, (hipStream_t)stream, root);
  LCPC_CATCH(m)
}

int lcpcf_commit_evals(lcpc_commit_t* m, uint32_t order, const uint64_t* evals_host, uint32_t log_n, uint8_t* root) {
  if (!m || !evals_host || order > LCPCF_BITREV) return LCPC_ERR_ARG;
  const lcpc_ctx* c = m->enc;
  if (log_n > dev_max_log_n(*c->f)) return LCPC_ERR_ARG;
  if (c->prm.shard_count > 1) return LCPC_ERR_STATE;
  if (!elems_reduced(*c->f, evals_host, (uint64_t)1 << log_n)) return LCPC_ERR_ARG;
  LCPC_TRY
  std::unique_lock<FillLock> fill(m->fill_mu);
  std::lock_guard<std::mutex> g(m->mu);
  HIPCHK(m, hipSetDevice(c->prm.device));
  return commit_evals_locked(m, order == LCPCF_NATURAL ? FFT_IFFT_II : FFT_IFFT_OI, evals_host, log_n, true, nullptr, root);
  LCPC_CATCH(m)
}

}  // extern "C"

// lcpc_amd/csrc/fft.cpp -- the transform extension of the C ABI (include/lcpc_hip_fft.h): the six FieldFFT forms on the host
// (fft_host.h, no HIP call) and on the device (K12 / K13, fft.hip) with the context's cache of two-level tables -- cached_table, the one
// routine behind the twiddle tables here (fft_table) and the shift tables of domain.cpp -- and the commit entry points that read
// evaluations (commit_evals_entry, which lcpcd_commit_coset_evals* share).  The commit pipeline itself is commit.cpp's
// (commit_evals_locked).
#include "internal.h"
#include "fft_host.h"
#include "../../include/lcpc_hip_fft.h"

using namespace lcpc;

static_assert(LCPCF_FFT_II == FFT_FFT_II && LCPCF_FFT_IO == FFT_FFT_IO && LCPCF_FFT_OI == FFT_FFT_OI && LCPCF_IFFT_II == FFT_IFFT_II &&
                  LCPCF_IFFT_IO == FFT_IFFT_IO && LCPCF_IFFT_OI == FFT_IFFT_OI,
              "lcpcf_form and the launcher's forms are one numbering");

int lcpc::cached_table(lcpc_ctx* c, ErrText* err, FftTab* tabs, int n_tabs, const uint64_t* shift, uint32_t log_n, bool inverse, TabBase base,
                       const uint32_t** tab) {
  const FieldDesc& f = *c->f;
  uint64_t key[MAXL] = {0, 0, 0, 0};
  if (shift) memcpy(key, shift, 8 * f.L);
  FftTab* victim = &tabs[0];
  for (FftTab* t = tabs; t < tabs + n_tabs; t++) {
    if (t->d && t->log_n == log_n && t->inverse == inverse && !memcmp(t->shift, key, sizeof key)) { t->stamp = ++c->fft_stamp; *tab = t->d; return 0; }
    if (!t->d ? victim->d != nullptr : (victim->d && t->stamp < victim->stamp)) victim = t;
  }
  const uint32_t h = fft_tab_split(log_n);
  const uint64_t n_lo = (uint64_t)1 << h, n_hi = (uint64_t)1 << (log_n - h);
  std::vector<uint64_t> host((size_t)(n_lo + n_hi) * f.L);
  uint64_t v[MAXL], factor[MAXL];
  const bool scaled = base(f, shift, log_n, inverse, v, factor);
  two_level_table(f, v, n_lo, n_hi, scaled ? factor : nullptr, host.data());
  dev_free(victim->d);                 // (waits for whatever still reads it)
  victim->d = nullptr;
  int rc = dev_alloc(err, &victim->d, host.size() * 8);
  if (rc) return rc;
  hipError_t e = hipMemcpy(victim->d, host.data(), host.size() * 8, hipMemcpyHostToDevice);
  if (e != hipSuccess) { dev_free(victim->d); victim->d = nullptr; return fail_hip(err, e, shift ? "hipMemcpy (shift table)" : "hipMemcpy (fft table)"); }
  memcpy(victim->shift, key, sizeof key);
  victim->log_n = log_n; victim->inverse = inverse; victim->stamp = ++c->fft_stamp;
  *tab = victim->d;
  return 0;
}

int lcpc::fft_table(lcpc_ctx* c, ErrText* err, uint32_t log_n, bool inverse, const uint32_t** tab) {
  return cached_table(c, err, c->fft_tabs, 4, nullptr, log_n, inverse,
                      [](const FieldDesc& f, const uint64_t*, uint32_t log_n, bool inverse, uint64_t* v, uint64_t*) { root_of(f, log_n, inverse, v); return false; }, tab);
}

int lcpc::commit_evals_entry(lcpc_commit_t* m, uint32_t order, bool coset, const uint64_t* shift, const uint64_t* evals, uint32_t log_n, bool host,
                             hipStream_t st, uint8_t* root) {
  if (!m || !evals || order > LCPCF_BITREV) return LCPC_ERR_ARG;
  const lcpc_ctx* c = m->enc;
  if ((coset && !shift_ok(*c->f, shift)) || (!host && !dev_aligned(evals, c->L)) || log_n > dev_max_log_n(*c->f)) return LCPC_ERR_ARG;
  if (c->prm.shard_count > 1) return LCPC_ERR_STATE;
  if (host && !elems_reduced(*c->f, evals, (uint64_t)1 << log_n)) return LCPC_ERR_ARG;
  LCPC_TRY
  std::unique_lock<FillLock> fill(m->fill_mu);      // a fill: waits for the readers in flight (internal.h)
  std::lock_guard<std::mutex> g(m->mu);
  HIPCHK(m, hipSetDevice(c->prm.device));
  return commit_evals_locked(m, order == LCPCF_NATURAL ? FFT_IFFT_II : FFT_IFFT_OI, evals, log_n, host, host ? nullptr : st, root, coset ? shift : nullptr);
  LCPC_CATCH(m)
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
  uint64_t total = 0;
  if (!c || form > LCPCF_IFFT_OI || !dev_vectors_ok(c, in_dev, out_dev, log_n, n_vecs, &total)) return LCPC_ERR_ARG;
  LCPC_TRY
  HIPCHK(c, hipSetDevice(c->prm.device));
  return fft_enqueue(c, &c->err, (int)form, reinterpret_cast<const uint32_t*>(in_dev), reinterpret_cast<uint32_t*>(out_dev), log_n, n_vecs,
                     (hipStream_t)stream);
  LCPC_CATCH(c)
}

int lcpcf_commit_evals_device(lcpc_commit_t* m, uint32_t order, const uint64_t* evals_dev, uint32_t log_n, void* stream, uint8_t* root) {
  return commit_evals_entry(m, order, false, nullptr, evals_dev, log_n, false, (hipStream_t)stream, root);
}

int lcpcf_commit_evals(lcpc_commit_t* m, uint32_t order, const uint64_t* evals_host, uint32_t log_n, uint8_t* root) {
  return commit_evals_entry(m, order, false, nullptr, evals_host, log_n, true, nullptr, root);
}

}  // extern "C"

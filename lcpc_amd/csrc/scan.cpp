// lcpc_amd/csrc/scan.cpp -- the scan extension of the C ABI (include/lcpc_hip_scan.h): prefix sums and products on the host
// (scan_host.h, no HIP call) and on the device (K17, scan.hip); the ratio form on the device is K15's DIV into the output followed by
// the scan in place.  Every refusal is settled on the host before anything is enqueued; lcpcs_scan_work_bytes is the one place that
// knows the size of the workspace.
#include "internal.h"
#include "scan_host.h"
#include "../../include/lcpc_hip_domain.h"
#include "../../include/lcpc_hip_scan.h"

using namespace lcpc;

static_assert(LCPCS_SUM == SCAN_SUM && LCPCS_PRODUCT == SCAN_PRODUCT && LCPCS_SUM == HS_SUM && LCPCS_PRODUCT == HS_PRODUCT &&
                  LCPCS_INCLUSIVE == SCAN_INCLUSIVE && LCPCS_EXCLUSIVE == SCAN_EXCLUSIVE && LCPCS_INCLUSIVE == HS_INCLUSIVE &&
                  LCPCS_EXCLUSIVE == HS_EXCLUSIVE,
              "lcpcs_op and lcpcs_mode, the launcher's values and the host's are one numbering");

namespace {

inline const uint32_t* words(const uint64_t* p) { return reinterpret_cast<const uint32_t*>(p); }
inline uint32_t* words(uint64_t* p) { return reinterpret_cast<uint32_t*>(p); }

// (SCAN_MAX_TILES: the grid of K17a / K17c, kernels.h)
bool dims_ok(int nl, uint64_t n, uint32_t n_vecs) {
  return n != 0 && n < ((uint64_t)1 << 39) && n_vecs != 0 && n_vecs <= 65535 && n * n_vecs < ((uint64_t)1 << 39) &&   // (no overflow: 2^55)
         scan_tiles(nl, n) < SCAN_MAX_TILES;
}

// what the host forms refuse alike, the inputs apart
bool host_ends_ok(const FieldDesc* f, uint32_t op, uint32_t mode, const uint64_t* out, uint64_t n, const uint64_t* init) {
  return f && op <= LCPCS_PRODUCT && mode <= LCPCS_EXCLUSIVE && out && n != 0 && n < ((uint64_t)1 << 39) && !(init && h_ge_p(*f, init));
}

// what the device forms refuse alike: `ins` are the one or two inputs, each the output itself or clear of it; init, total and work
// meet nothing
bool dev_args_ok(const lcpc_ctx* c, uint32_t op, uint32_t mode, std::initializer_list<const uint64_t*> ins, const uint64_t* out_dev, uint64_t n,
                 uint32_t n_vecs, const uint64_t* init_dev, const uint64_t* total_dev, const void* work_dev, uint64_t work_bytes) {
  if (!c || op > LCPCS_PRODUCT || mode > LCPCS_EXCLUSIVE || !out_dev || !work_dev || !dims_ok(c->NL, n, n_vecs)) return false;
  const uint64_t need = lcpcs_scan_work_bytes(c, n, n_vecs), bytes = n * n_vecs * elem_bytes(c), ends = n_vecs * elem_bytes(c);
  if (work_bytes < need || !dev_aligned(out_dev, c->L) || !dev_aligned(work_dev, c->L)) return false;
  if ((init_dev && !dev_aligned(init_dev, c->L)) || (total_dev && !dev_aligned(total_dev, c->L))) return false;
  if (init_dev && total_dev && ranges_meet(init_dev, ends, total_dev, ends)) return false;
  auto ends_clear_of = [&](const void* p, uint64_t p_bytes) {     // neither init nor total meets p
    return !(init_dev && ranges_meet(init_dev, ends, p, p_bytes)) && !(total_dev && ranges_meet(total_dev, ends, p, p_bytes));
  };
  if (!ends_clear_of(work_dev, need) || !ends_clear_of(out_dev, bytes) || ranges_meet(work_dev, need, out_dev, bytes)) return false;
  for (const uint64_t* in : ins) {
    if (!in || !dev_aligned(in, c->L) || !ends_clear_of(in, bytes) || ranges_meet(work_dev, need, in, bytes)) return false;
    if (in != out_dev && ranges_meet(in, bytes, out_dev, bytes)) return false;
  }
  return true;
}

int scan_enqueue(lcpc_ctx* c, uint32_t op, uint32_t mode, const uint64_t* in_dev, uint64_t* out_dev, uint64_t n, uint32_t n_vecs,
                 const uint64_t* init_dev, uint64_t* total_dev, void* work_dev, hipStream_t st) {
  hipError_t e = launch_scan(c->NL, (int)op, (int)mode, words(in_dev), words(out_dev), n, n_vecs, words(init_dev), words(total_dev), words(c->f->r),
                             static_cast<uint32_t*>(work_dev), scan_work_elems(c->NL, n, n_vecs), st, nullptr);
  if (e != hipSuccess) return fail_hip(&c->err, e, "launch_scan");
  return 0;
}

}  // namespace

extern "C" {

int lcpcs_version(void) { return LCPCS_VERSION; }

int lcpcs_scan(uint32_t field, uint32_t op, uint32_t mode, const uint64_t* in, uint64_t* out, uint64_t n, const uint64_t* init, uint64_t* total) {
  const FieldDesc* f = field_desc((int)field);
  if (!in || !host_ends_ok(f, op, mode, out, n, init)) return LCPC_ERR_ARG;
  if (ranges_overlap(in, out, n * 8 * f->L) || !elems_reduced(*f, in, n)) return LCPC_ERR_ARG;
  host_scan(*f, op, mode, in, out, n, init, total);
  return 0;
}

int lcpcs_scan_ratio(uint32_t field, uint32_t op, uint32_t mode, const uint64_t* num, const uint64_t* den, uint64_t* out, uint64_t n,
                     const uint64_t* init, uint64_t* total) {
  const FieldDesc* f = field_desc((int)field);
  if (!num || !den || !host_ends_ok(f, op, mode, out, n, init)) return LCPC_ERR_ARG;
  const uint64_t bytes = n * 8 * f->L;
  if (ranges_overlap(num, out, bytes) || ranges_overlap(den, out, bytes)) return LCPC_ERR_ARG;
  if (!elems_reduced(*f, num, n) || !elems_reduced(*f, den, n)) return LCPC_ERR_ARG;
  try {
    host_scan_ratio(*f, op, mode, num, den, out, n, init, total);
  } catch (const std::exception&) {
    return LCPC_ERR_NOMEM;
  }
  return 0;
}

uint64_t lcpcs_scan_work_bytes(const lcpc_ctx* c, uint64_t n, uint32_t n_vecs) {
  if (!c || !dims_ok(c->NL, n, n_vecs)) return 0;
  return scan_work_elems(c->NL, n, n_vecs) * elem_bytes(c);
}

int lcpcs_scan_device(lcpc_ctx* c, uint32_t op, uint32_t mode, const uint64_t* in_dev, uint64_t* out_dev, uint64_t n, uint32_t n_vecs,
                      const uint64_t* init_dev, uint64_t* total_dev, void* work_dev, uint64_t work_bytes, void* stream) {
  if (!dev_args_ok(c, op, mode, {in_dev}, out_dev, n, n_vecs, init_dev, total_dev, work_dev, work_bytes)) return LCPC_ERR_ARG;
  LCPC_TRY
  HIPCHK(c, hipSetDevice(c->prm.device));
  return scan_enqueue(c, op, mode, in_dev, out_dev, n, n_vecs, init_dev, total_dev, work_dev, (hipStream_t)stream);
  LCPC_CATCH(c)
}

int lcpcs_scan_ratio_device(lcpc_ctx* c, uint32_t op, uint32_t mode, const uint64_t* num_dev, const uint64_t* den_dev, uint64_t* out_dev,
                            uint64_t n, uint32_t n_vecs, const uint64_t* init_dev, uint64_t* total_dev, void* work_dev, uint64_t work_bytes,
                            void* stream) {
  if (!dev_args_ok(c, op, mode, {num_dev, den_dev}, out_dev, n, n_vecs, init_dev, total_dev, work_dev, work_bytes)) return LCPC_ERR_ARG;
  LCPC_TRY
  HIPCHK(c, hipSetDevice(c->prm.device));
  // (dev_args_ok has refused everything launch_scan refuses, so behind the division only a failed launch can stop the scan)
  HIPCHK(c, launch_pointwise(c->NL, QUOT_DIV, words(num_dev), words(den_dev), words(out_dev), n * n_vecs, (hipStream_t)stream));
  return scan_enqueue(c, op, mode, out_dev, out_dev, n, n_vecs, init_dev, total_dev, work_dev, (hipStream_t)stream);
  LCPC_CATCH(c)
}

}  // extern "C"

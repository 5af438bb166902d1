// lcpc_amd/csrc/scan_host.h -- the host forms of include/lcpc_hip_scan.h on one thread over host_field.h (no HIP): the prefix sum or
// product of one vector in O(n), and the scan of the ratios num[k] / den[k] over quot_host.h's batch inversion.  scan.cpp holds the
// entry points; tools/check_scan_host.cpp compiles this header without the HIP runtime.
#pragma once
#include "quot_host.h"

namespace lcpc {

enum : uint32_t { HS_SUM = 0, HS_PRODUCT = 1 };
enum : uint32_t { HS_INCLUSIVE = 0, HS_EXCLUSIVE = 1 };

// out[k] = c (+) in[0] (+) ... (+) in[k] (inclusive) or ... (+) in[k - 1] (exclusive), c = *init or the identity; *total (may be null)
// receives c (+) every element.  out == in allowed: in[k] is read before out[k] is written.  init is read before and total written
// after everything else, so either may lie in the output; n >= 1
inline void host_scan(const FieldDesc& f, uint32_t op, uint32_t mode, const uint64_t* in, uint64_t* out, uint64_t n, const uint64_t* init,
                      uint64_t* total) {
  const int L = f.L;
  uint64_t run[MAXL] = {0, 0, 0, 0}, x[MAXL];
  if (init) memcpy(run, init, 8 * L);
  else if (op == HS_PRODUCT) memcpy(run, f.r, 8 * L);
  for (uint64_t k = 0; k < n; k++) {
    memcpy(x, in + k * L, 8 * L);
    if (mode == HS_EXCLUSIVE) memcpy(out + k * L, run, 8 * L);
    if (op == HS_SUM) h_add(f, run, run, x);
    else h_mul(f, run, run, x);
    if (mode == HS_INCLUSIVE) memcpy(out + k * L, run, 8 * L);
  }
  if (total) memcpy(total, run, 8 * L);
}

// the same over the terms num[k] den[k]^-1, zero where den[k] is zero; out may be num or den.  The terms go through a copy of n
// elements (std::bad_alloc when the host cannot hold it, before anything is written)
inline void host_scan_ratio(const FieldDesc& f, uint32_t op, uint32_t mode, const uint64_t* num, const uint64_t* den, uint64_t* out,
                            uint64_t n, const uint64_t* init, uint64_t* total) {
  std::vector<uint64_t> terms((size_t)n * f.L);
  host_pointwise(f, HQ_DIV, num, den, terms.data(), n);
  host_scan(f, op, mode, terms.data(), out, n, init, total);
}

}  // namespace lcpc

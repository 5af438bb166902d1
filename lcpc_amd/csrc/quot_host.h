// lcpc_amd/csrc/quot_host.h -- the host forms of include/lcpc_hip_quot.h on one thread over host_field.h and fft_host.h (no HIP):
// Montgomery's batch inversion, the pointwise operations and the two quotients on a domain, and the tests on z and the shift that
// the device calls make on the host as well.  quot.cpp holds the entry points; tools/check_quot_host.cpp compiles this header without
// the HIP runtime.
#pragma once
#include "fft_host.h"

namespace lcpc {

enum : uint32_t { HQ_ADD = 0, HQ_SUB = 1, HQ_MUL = 2, HQ_DIV = 3 };

// out[i] = in[i]^-1, zero for zero: one h_inv and 3 (n - 1) multiplies.  out == in allowed; n >= 1
inline void host_batch_inverse(const FieldDesc& f, const uint64_t* in, uint64_t* out, uint64_t n) {
  const int L = f.L;
  std::vector<uint64_t> pre((size_t)n * L);      // pre[i]: the product of the nonzero elements up to and including i
  uint64_t run[MAXL];
  memcpy(run, f.r, 8 * L);
  for (uint64_t i = 0; i < n; i++) {
    if (!h_is_zero(f, in + i * L)) h_mul(f, run, run, in + i * L);
    memcpy(pre.data() + i * L, run, 8 * L);
  }
  uint64_t inv[MAXL];
  h_inv(f, inv, run);
  for (uint64_t i = n; i-- > 0;) {
    uint64_t x[MAXL];
    memcpy(x, in + i * L, 8 * L);
    if (h_is_zero(f, x)) { memset(out + i * L, 0, 8 * L); continue; }
    if (i) h_mul(f, out + i * L, inv, pre.data() + (i - 1) * L); else memcpy(out + i * L, inv, 8 * L);
    h_mul(f, inv, inv, x);
  }
}

// out[i] = a[i] op b[i]; out may be a or b
inline void host_pointwise(const FieldDesc& f, uint32_t op, const uint64_t* a, const uint64_t* b, uint64_t* out, uint64_t n) {
  const int L = f.L;
  if (op == HQ_DIV) {
    std::vector<uint64_t> bi((size_t)n * L);
    host_batch_inverse(f, b, bi.data(), n);
    for (uint64_t i = 0; i < n; i++) h_mul(f, out + i * L, a + i * L, bi.data() + i * L);
    return;
  }
  for (uint64_t i = 0; i < n; i++) {
    if (op == HQ_ADD) h_add(f, out + i * L, a + i * L, b + i * L);
    else if (op == HQ_SUB) h_sub(f, out + i * L, a + i * L, b + i * L);
    else h_mul(f, out + i * L, a + i * L, b + i * L);
  }
}

// z is one of the points shift w_m^k: (z / shift)^m == 1.  shift == nullptr: the subgroup
inline bool z_on_domain(const FieldDesc& f, const uint64_t* shift, const uint64_t* z, uint32_t log_m) {
  uint64_t t[MAXL];
  memcpy(t, z, 8 * f.L);
  if (shift) {
    h_inv(f, t, shift);
    h_mul(f, t, t, z);
  }
  h_pow(f, t, t, (uint64_t)1 << log_m);
  return h_eq(f, t, f.r);
}
// shift^m == 1: X^n - 1 has a root on shift H_m for every n | m
inline bool shift_on_subgroup(const FieldDesc& f, const uint64_t* shift, uint32_t log_m) {
  uint64_t t[MAXL];
  h_pow(f, t, shift, (uint64_t)1 << log_m);
  return h_eq(f, t, f.r);
}

// den[place of k] = shift w_m^k - z
inline void linear_denominators(const FieldDesc& f, const uint64_t* shift, bool rev, uint32_t log_m, const uint64_t* z, uint64_t* den) {
  uint64_t w[MAXL], x[MAXL];
  root_of(f, log_m, false, w);
  memcpy(x, shift ? shift : f.r, 8 * f.L);
  for (uint64_t k = 0; k < ((uint64_t)1 << log_m); k++) {
    h_sub(f, den + (rev ? h_rev(k, log_m) : k) * f.L, x, z);
    h_mul(f, x, x, w);
  }
}
// den[place of k] = (shift w_m^k)^n - 1, n = 2^log_n <= m
inline void vanishing_denominators(const FieldDesc& f, const uint64_t* shift, bool rev, uint32_t log_m, uint32_t log_n, uint64_t* den) {
  uint64_t w[MAXL], x[MAXL];
  root_of(f, log_m - log_n, false, w);            // w_m^n
  h_pow(f, x, shift, (uint64_t)1 << log_n);
  for (uint64_t k = 0; k < ((uint64_t)1 << log_m); k++) {
    h_sub(f, den + (rev ? h_rev(k, log_m) : k) * f.L, x, f.r);
    h_mul(f, x, x, w);
  }
}

// out[i] = (in[i] - y) den[i]^-1 (y == nullptr: in[i] den[i]^-1); den is overwritten.  out == in allowed
inline void host_divide(const FieldDesc& f, const uint64_t* in, const uint64_t* y, uint64_t* den, uint64_t* out, uint64_t m) {
  host_batch_inverse(f, den, den, m);
  for (uint64_t i = 0; i < m; i++) {
    uint64_t t[MAXL];
    memcpy(t, in + i * f.L, 8 * f.L);
    if (y) h_sub(f, t, t, y);
    h_mul(f, out + i * f.L, t, den + i * f.L);
  }
}

}  // namespace lcpc

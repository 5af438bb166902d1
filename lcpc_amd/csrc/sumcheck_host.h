// lcpc_amd/csrc/sumcheck_host.h -- the host forms of include/lcpc_hip_sumcheck.h on one thread over host_field.h (no HIP): the binding of
// one variable of a table and the round sums of a composition of tables.  sumcheck.cpp holds the entry points;
// tools/check_sumcheck_host.cpp compiles this header without the HIP runtime.
#pragma once
#include "fft_host.h"

namespace lcpc {

enum : uint32_t { HM_LOW_FIRST = 0, HM_HIGH_FIRST = 1 };
constexpr uint32_t HM_MAX_TABLES = 8, HM_MAX_TERMS = 4, HM_MAX_FACTORS = 4;
struct HmTerm { uint32_t n_factors; uint32_t table[HM_MAX_FACTORS]; };

// what every form refuses alike: the shape of a composition.  Returns the degree d = max n_factors, 0 for a refusal
inline uint32_t hm_degree(uint32_t n_tables, const HmTerm* terms, uint32_t n_terms) {
  if (n_tables == 0 || n_tables > HM_MAX_TABLES || !terms || n_terms == 0 || n_terms > HM_MAX_TERMS) return 0;
  uint32_t d = 0;
  for (uint32_t m = 0; m < n_terms; m++) {
    if (terms[m].n_factors == 0 || terms[m].n_factors > HM_MAX_FACTORS) return 0;
    for (uint32_t k = 0; k < terms[m].n_factors; k++)
      if (terms[m].table[k] >= n_tables) return 0;
    if (terms[m].n_factors > d) d = terms[m].n_factors;
  }
  return d;
}
// n = 2^v with v >= 1 (v >= 2 for the fused form: min_n = 4), below 2^39
inline bool hm_len_ok(uint64_t n, uint64_t min_n) { return n >= min_n && n < ((uint64_t)1 << 39) && (n & (n - 1)) == 0; }

// the places of pair i of a table of 2 h elements
inline uint64_t hm_lo(uint32_t order, uint64_t i, uint64_t) { return order == HM_LOW_FIRST ? 2 * i : i; }
inline uint64_t hm_hi(uint32_t order, uint64_t i, uint64_t h) { return order == HM_LOW_FIRST ? 2 * i + 1 : i + h; }

// out[i] = lo_i + r (hi_i - lo_i), i < n / 2.  out == in allowed: out[i] is written after both places of pair i are read, and no pair
// j > i has a place below i + 1
inline void host_bind(const FieldDesc& f, uint32_t order, const uint64_t* in, uint64_t* out, uint64_t n, const uint64_t* r) {
  const int L = f.L;
  const uint64_t h = n / 2;
  uint64_t rr[MAXL], lo[MAXL], hi[MAXL];
  memcpy(rr, r, 8 * L);
  for (uint64_t i = 0; i < h; i++) {
    memcpy(lo, in + hm_lo(order, i, h) * L, 8 * L);
    memcpy(hi, in + hm_hi(order, i, h) * L, 8 * L);
    h_sub(f, hi, hi, lo);
    h_mul(f, hi, hi, rr);
    h_add(f, lo, lo, hi);
    memcpy(out + i * L, lo, 8 * L);
  }
}

// evals[t] = sum_i sum_m c_m prod_k ext(table[m][k], i, t), t = 0 .. d; coeffs [n_terms][L] or null (all one).  The sums are kept per
// term and t, and c_m is applied once to each
inline void host_round(const FieldDesc& f, uint32_t order, const uint64_t* const* tables, const HmTerm* terms, uint32_t n_terms,
                       const uint64_t* coeffs, uint64_t n, uint32_t d, uint64_t* evals) {
  const int L = f.L;
  const uint64_t h = n / 2;
  uint64_t acc[HM_MAX_TERMS][HM_MAX_FACTORS + 1][MAXL] = {};
  uint64_t prod[HM_MAX_FACTORS + 1][MAXL], v[MAXL], diff[MAXL];
  for (uint64_t i = 0; i < h; i++) {
    for (uint32_t m = 0; m < n_terms; m++) {
      for (uint32_t k = 0; k < terms[m].n_factors; k++) {
        const uint64_t* tb = tables[terms[m].table[k]];
        memcpy(v, tb + hm_lo(order, i, h) * L, 8 * L);
        h_sub(f, diff, tb + hm_hi(order, i, h) * L, v);
        for (uint32_t t = 0; t <= d; t++) {
          if (t) h_add(f, v, v, diff);
          if (k) h_mul(f, prod[t], prod[t], v); else memcpy(prod[t], v, 8 * L);
        }
      }
      for (uint32_t t = 0; t <= d; t++) h_add(f, acc[m][t], acc[m][t], prod[t]);
    }
  }
  for (uint32_t t = 0; t <= d; t++) {
    uint64_t s[MAXL] = {0, 0, 0, 0};
    for (uint32_t m = 0; m < n_terms; m++) {
      if (coeffs) h_mul(f, acc[m][t], acc[m][t], coeffs + (size_t)m * L);
      h_add(f, s, s, acc[m][t]);
    }
    memcpy(evals + (size_t)t * L, s, 8 * L);
  }
}

}  // namespace lcpc

// tools/check_sumcheck_host.cpp -- the host forms of include/lcpc_hip_sumcheck.h under AddressSanitizer and UBSan, without the HIP
// runtime: lcpc_amd/csrc/sumcheck_host.h (what lcpcm_bind and lcpcm_round run) over fft_host.h and host_field.h, with the field table of
// encoding.cpp.  Every buffer is a heap allocation of exactly the size the call may touch.
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -Ilcpc_amd/csrc tools/check_sumcheck_host.cpp \
//       lcpc_amd/csrc/encoding.cpp lcpc_amd/csrc/host_crypto.cpp -lpthread -o check_sumcheck_host && ./check_sumcheck_host
// Checks, for the four fields, both orders and n = 2 .. 1024: every output is reduced; a bind in place equals the bind out of place
// and leaves the upper half alone; g(0) + g(1) is the plain sum of the composition; g(0) and g(1) are the sums over the lo and the hi
// places; after a bind by r the next round's g'(0) + g'(1) is g(r) by Lagrange interpolation, down to one element per table; the
// full composition (8 tables, 4 terms, coefficients) and a square.
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "sumcheck_host.h"

using namespace lcpc;

static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static uint64_t rnd() {
  rng_state ^= rng_state << 13; rng_state ^= rng_state >> 7; rng_state ^= rng_state << 17;
  return rng_state;
}
static void rand_elem(const FieldDesc& f, uint64_t* e) {
  do {
    for (int i = 0; i < f.L; i++) e[i] = rnd();
    e[f.L - 1] &= f.top_mask;
  } while (h_ge_p(f, e));
}
#define CHECK(c) do { if (!(c)) { fprintf(stderr, "check failed at line %d: %s\n", __LINE__, #c); exit(1); } } while (0)

typedef std::vector<uint64_t> Vec;

// the small integer k as an element
static void small(const FieldDesc& f, uint64_t k, uint64_t* o) {
  uint64_t acc[MAXL] = {0, 0, 0, 0};
  for (uint64_t i = 0; i < k; i++) h_add(f, acc, acc, f.r);
  memcpy(o, acc, 8 * f.L);
}
// g(x) from g(0) .. g(d)
static void interpolate(const FieldDesc& f, const Vec& evals, uint32_t d, const uint64_t* x, uint64_t* o) {
  const int L = f.L;
  uint64_t s[MAXL] = {0, 0, 0, 0};
  for (uint32_t t = 0; t <= d; t++) {
    uint64_t num[MAXL], den[MAXL], a[MAXL], b[MAXL];
    memcpy(num, f.r, 8 * L);
    memcpy(den, f.r, 8 * L);
    for (uint32_t u = 0; u <= d; u++) {
      if (u == t) continue;
      small(f, u, a);
      h_sub(f, b, x, a);
      h_mul(f, num, num, b);
      small(f, t, b);
      h_sub(f, b, b, a);
      h_mul(f, den, den, b);
    }
    h_inv(f, den, den);
    h_mul(f, num, num, den);
    h_mul(f, num, num, evals.data() + (size_t)t * L);
    h_add(f, s, s, num);
  }
  memcpy(o, s, 8 * L);
}
// sum over the places `at` of sum_m c_m prod_k table[m][k][at]; at = all places when both is set
static void plain_sum(const FieldDesc& f, uint32_t order, const std::vector<Vec>& tabs, const HmTerm* terms, uint32_t n_terms, const uint64_t* coeffs,
                      size_t n, int which, uint64_t* o) {
  const int L = f.L;
  uint64_t s[MAXL] = {0, 0, 0, 0};
  for (size_t x = 0; x < n; x++) {
    if (which >= 0) {                                     // 0: the lo places only, 1: the hi places only
      const bool hi = order == HM_LOW_FIRST ? (x & 1) : x >= n / 2;
      if ((int)hi != which) continue;
    }
    for (uint32_t m = 0; m < n_terms; m++) {
      uint64_t p[MAXL];
      memcpy(p, coeffs ? coeffs + (size_t)m * L : f.r, 8 * L);
      for (uint32_t k = 0; k < terms[m].n_factors; k++) h_mul(f, p, p, tabs[terms[m].table[k]].data() + x * L);
      h_add(f, s, s, p);
    }
  }
  memcpy(o, s, 8 * L);
}

int main() {
  const HmTerm full[4] = {{4, {0, 1, 2, 3}}, {2, {4, 5}}, {3, {6, 7, 0}}, {1, {7}}};
  const HmTerm square[2] = {{2, {0, 0}}, {3, {1, 0, 1}}};
  for (int fid = 0; fid < 4; fid++) {
    const FieldDesc& f = *field_desc(fid);
    const size_t L = f.L;
    for (uint32_t order : {(uint32_t)HM_LOW_FIRST, (uint32_t)HM_HIGH_FIRST}) {
      for (size_t n0 : {(size_t)2, (size_t)4, (size_t)8, (size_t)64, (size_t)1024}) {
        for (int shape = 0; shape < 2; shape++) {
          const HmTerm* terms = shape ? square : full;
          const uint32_t n_terms = shape ? 2 : 4, n_tables = shape ? 2 : 8;
          const uint32_t d = hm_degree(n_tables, terms, n_terms);
          CHECK(d == (shape ? 3u : 4u) && hm_len_ok(n0, 2) && !hm_len_ok(n0 + 1, 2) && !hm_len_ok(2, 4));
          std::vector<Vec> tabs(n_tables, Vec(n0 * L));
          for (auto& t : tabs)
            for (size_t i = 0; i < n0; i++) rand_elem(f, t.data() + i * L);
          Vec coeffs(n_terms * L), claim(L), r(L), evals((d + 1) * L), t0(L), t1(L);
          for (uint32_t m = 0; m < n_terms; m++) rand_elem(f, coeffs.data() + m * L);
          const uint64_t* cs = shape ? nullptr : coeffs.data();       // the square runs without coefficients
          plain_sum(f, order, tabs, terms, n_terms, cs, n0, -1, claim.data());
          for (size_t n = n0; n >= 2; n /= 2) {
            std::vector<const uint64_t*> ptrs;
            for (auto& t : tabs) ptrs.push_back(t.data());
            host_round(f, order, ptrs.data(), terms, n_terms, cs, n, d, evals.data());
            CHECK(elems_reduced(f, evals.data(), d + 1));
            plain_sum(f, order, tabs, terms, n_terms, cs, n, 0, t0.data());
            plain_sum(f, order, tabs, terms, n_terms, cs, n, 1, t1.data());
            CHECK(h_eq(f, t0.data(), evals.data()) && h_eq(f, t1.data(), evals.data() + L));
            h_add(f, t0.data(), t0.data(), t1.data());
            CHECK(h_eq(f, t0.data(), claim.data()));
            rand_elem(f, r.data());
            interpolate(f, evals, d, r.data(), claim.data());
            for (auto& t : tabs) {
              Vec out((n / 2) * L), io(t);                            // exact sizes: n / 2 outputs, n inputs
              host_bind(f, order, t.data(), out.data(), n, r.data());
              host_bind(f, order, io.data(), io.data(), n, r.data()); // in place: one thread walks upward
              CHECK(elems_reduced(f, out.data(), n / 2));
              CHECK(memcmp(io.data(), out.data(), (n / 2) * L * 8) == 0 && memcmp(io.data() + (n / 2) * L, t.data() + (n / 2) * L, (n / 2) * L * 8) == 0);
              t = out;
            }
          }
          // one element per table is left: their composition is the last claim
          plain_sum(f, order, tabs, terms, n_terms, cs, 1, -1, t0.data());
          CHECK(h_eq(f, t0.data(), claim.data()));
        }
      }
    }
  }
  printf("check_sumcheck_host ok\n");
  return 0;
}

// tools/check_quot_host.cpp -- the host forms of include/lcpc_hip_quot.h under AddressSanitizer and UBSan, without the HIP runtime:
// lcpc_amd/csrc/quot_host.h (what lcpcq_batch_inverse, lcpcq_pointwise, lcpcq_divide_linear and lcpcq_divide_vanishing run) over
// fft_host.h and host_field.h, with the field table of encoding.cpp.  Every buffer is a heap allocation of exactly the size the call
// may touch.
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -Ilcpc_amd/csrc tools/check_quot_host.cpp \
//       lcpc_amd/csrc/encoding.cpp lcpc_amd/csrc/host_crypto.cpp -lpthread -o check_quot_host && ./check_quot_host
// Checks: x inv(x) is one off the zeros and zero on them, in place as well; DIV(a, b) is MUL(a, inverse(b)); SUB undoes ADD; the two
// quotients times their denominators, computed point by point with h_pow, give the numerators back, in both orders; the tests on z and
// on the shift accept and refuse what they must.
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "quot_host.h"

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

int main() {
  for (int fid = 0; fid < 4; fid++) {
    const FieldDesc& f = *field_desc(fid);
    const int L = f.L;
    for (size_t n : {(size_t)1, (size_t)2, (size_t)3, (size_t)64, (size_t)1000}) {
      std::vector<uint64_t> x(n * L), a(n * L), inv(n * L), t(n * L), u(n * L);
      for (size_t i = 0; i < n; i++) { rand_elem(f, x.data() + i * L); rand_elem(f, a.data() + i * L); }
      for (size_t i : {(size_t)0, n / 2, n - 1})
        if (n >= 3 || i == 0) memset(x.data() + i * L, 0, 8 * L);      // zeros at both ends and inside; the first alone below 3
      host_batch_inverse(f, x.data(), inv.data(), n);
      CHECK(elems_reduced(f, inv.data(), n));
      host_pointwise(f, HQ_MUL, x.data(), inv.data(), t.data(), n);
      for (size_t i = 0; i < n; i++) {
        if (h_is_zero(f, x.data() + i * L)) CHECK(h_is_zero(f, inv.data() + i * L) && h_is_zero(f, t.data() + i * L));
        else CHECK(h_eq(f, t.data() + i * L, f.r));
      }
      std::vector<uint64_t> ip(x);
      host_batch_inverse(f, ip.data(), ip.data(), n);              // in place
      CHECK(ip == inv);
      host_pointwise(f, HQ_DIV, a.data(), x.data(), t.data(), n);
      host_pointwise(f, HQ_MUL, a.data(), inv.data(), u.data(), n);
      CHECK(t == u);
      std::vector<uint64_t> oa(a), ob(x);
      host_pointwise(f, HQ_DIV, oa.data(), x.data(), oa.data(), n);  // out == a, out == b
      host_pointwise(f, HQ_DIV, a.data(), ob.data(), ob.data(), n);
      CHECK(oa == t && ob == t);
      host_pointwise(f, HQ_ADD, a.data(), x.data(), t.data(), n);
      host_pointwise(f, HQ_SUB, t.data(), x.data(), t.data(), n);
      CHECK(t == a);
    }
    uint64_t g[MAXL], s[MAXL];
    host_generator(f, g);
    do rand_elem(f, s); while (h_is_zero(f, s) || shift_on_subgroup(f, s, 9));
    CHECK(!shift_on_subgroup(f, g, 9) && shift_on_subgroup(f, f.r, 9));
    for (uint32_t log_m : {0u, 1u, 2u, 5u, 9u}) {
      const size_t m = (size_t)1 << log_m;
      std::vector<uint64_t> v(m * L), out(m * L), den(m * L);
      for (size_t i = 0; i < m; i++) rand_elem(f, v.data() + i * L);
      uint64_t w[MAXL], z[MAXL], y[MAXL];
      root_of(f, log_m, false, w);
      rand_elem(f, y);
      for (const uint64_t* shift : {(const uint64_t*)nullptr, (const uint64_t*)g, (const uint64_t*)s}) {
        uint64_t on[MAXL];                                          // shift w^5 (w^(5 mod m)) lies on the domain
        h_pow(f, on, w, 5);
        if (shift) h_mul(f, on, on, shift);
        CHECK(z_on_domain(f, shift, on, log_m));
        do rand_elem(f, z); while (z_on_domain(f, shift, z, log_m));
        for (bool rev : {false, true}) {
          linear_denominators(f, shift, rev, log_m, z, den.data());
          host_divide(f, v.data(), y, den.data(), out.data(), m);
          CHECK(elems_reduced(f, out.data(), m));
          for (size_t k = 0; k < m; k++) {
            const size_t at = rev ? h_rev(k, log_m) : k;
            uint64_t x[MAXL], t[MAXL];
            h_pow(f, x, w, k);
            if (shift) h_mul(f, x, x, shift);
            h_sub(f, x, x, z);
            h_mul(f, t, out.data() + at * L, x);
            h_add(f, t, t, y);
            CHECK(h_eq(f, t, v.data() + at * L));
          }
          if (!shift) continue;
          for (uint32_t log_n = 0; log_n <= log_m; log_n++) {
            std::vector<uint64_t> io(v);
            vanishing_denominators(f, shift, rev, log_m, log_n, den.data());
            host_divide(f, io.data(), nullptr, den.data(), io.data(), m);      // in place
            for (size_t k = 0; k < m; k++) {
              const size_t at = rev ? h_rev(k, log_m) : k;
              uint64_t x[MAXL], t[MAXL];
              h_pow(f, x, w, k);
              h_mul(f, x, x, shift);
              h_pow(f, x, x, (uint64_t)1 << log_n);
              h_sub(f, x, x, f.r);
              h_mul(f, t, io.data() + at * L, x);
              CHECK(h_eq(f, t, v.data() + at * L));
            }
          }
        }
      }
    }
  }
  printf("check_quot_host ok\n");
  return 0;
}

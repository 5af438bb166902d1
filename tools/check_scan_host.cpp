// tools/check_scan_host.cpp -- the host forms of include/lcpc_hip_scan.h under AddressSanitizer and UBSan, without the HIP runtime:
// lcpc_amd/csrc/scan_host.h (what lcpcs_scan and lcpcs_scan_ratio run) over quot_host.h and host_field.h, with the field table of
// encoding.cpp.  Every buffer is a heap allocation of exactly the size the call may touch.
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -Ilcpc_amd/csrc tools/check_scan_host.cpp \
//       lcpc_amd/csrc/encoding.cpp lcpc_amd/csrc/host_crypto.cpp -lpthread -o check_scan_host && ./check_scan_host
// Checks: an inclusive scan is the exclusive one shifted by one, and its last element the total; out[k] (+) in[k + 1] = out[k + 1];
// in place equals out of place; two calls chained through total -> init equal one; a zero turns a product to zero from its place
// on; the ratio form is the scan of DIV's terms, with out == num and out == den; init and total inside the output.
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "scan_host.h"

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
  } while (h_ge_p(f, e) || h_is_zero(f, e));
}
#define CHECK(c) do { if (!(c)) { fprintf(stderr, "check failed at line %d: %s\n", __LINE__, #c); exit(1); } } while (0)

static void combine(const FieldDesc& f, uint32_t op, uint64_t* o, const uint64_t* a, const uint64_t* b) {
  if (op == HS_SUM) h_add(f, o, a, b); else h_mul(f, o, a, b);
}

int main() {
  for (int fid = 0; fid < 4; fid++) {
    const FieldDesc& f = *field_desc(fid);
    const size_t L = f.L;
    for (size_t n : {(size_t)1, (size_t)2, (size_t)3, (size_t)64, (size_t)1000}) {
      std::vector<uint64_t> x(n * L), num(n * L), den(n * L), init(L), zero(L, 0);
      for (size_t i = 0; i < n; i++) { rand_elem(f, x.data() + i * L); rand_elem(f, num.data() + i * L); rand_elem(f, den.data() + i * L); }
      rand_elem(f, init.data());
      if (n >= 3) memset(den.data() + (n / 2) * L, 0, 8 * L);             // a zero denominator: a zero term
      for (uint32_t op : {(uint32_t)HS_SUM, (uint32_t)HS_PRODUCT}) {
        const uint64_t* e = op == HS_SUM ? zero.data() : f.r;
        for (const uint64_t* c : {(const uint64_t*)nullptr, (const uint64_t*)init.data()}) {
          std::vector<uint64_t> inc(n * L), exc(n * L), ti(L), te(L), t(L);
          host_scan(f, op, HS_INCLUSIVE, x.data(), inc.data(), n, c, ti.data());
          host_scan(f, op, HS_EXCLUSIVE, x.data(), exc.data(), n, c, te.data());
          CHECK(elems_reduced(f, inc.data(), n) && elems_reduced(f, exc.data(), n));
          CHECK(ti == te && h_eq(f, ti.data(), inc.data() + (n - 1) * L) && h_eq(f, exc.data(), c ? c : e));
          for (size_t k = 0; k + 1 < n; k++) {
            CHECK(h_eq(f, exc.data() + (k + 1) * L, inc.data() + k * L));
            combine(f, op, t.data(), inc.data() + k * L, x.data() + (k + 1) * L);
            CHECK(h_eq(f, t.data(), inc.data() + (k + 1) * L));
          }
          host_scan(f, op, HS_INCLUSIVE, x.data(), exc.data(), n, c, nullptr);      // no total
          CHECK(exc == inc);
          for (uint32_t mode : {(uint32_t)HS_INCLUSIVE, (uint32_t)HS_EXCLUSIVE}) {
            std::vector<uint64_t> whole(n * L), io(x), tw(L), ta(L), tb(L);
            host_scan(f, op, mode, x.data(), whole.data(), n, c, tw.data());
            host_scan(f, op, mode, io.data(), io.data(), n, c, ta.data());          // in place
            CHECK(io == whole && ta == tw);
            if (n >= 2) {                                                          // chained through the total
              const size_t cut = n / 3 + 1;
              std::vector<uint64_t> a(cut * L), b((n - cut) * L);
              host_scan(f, op, mode, x.data(), a.data(), cut, c, ta.data());
              host_scan(f, op, mode, x.data() + cut * L, b.data(), n - cut, ta.data(), tb.data());
              a.insert(a.end(), b.begin(), b.end());
              CHECK(a == whole && tb == tw);
            }
            // the ratio form: the scan of DIV's terms; out == num, out == den
            std::vector<uint64_t> terms(n * L), want(n * L), got(n * L), on(num), od(den);
            host_pointwise(f, HQ_DIV, num.data(), den.data(), terms.data(), n);
            host_scan(f, op, mode, terms.data(), want.data(), n, c, tw.data());
            host_scan_ratio(f, op, mode, num.data(), den.data(), got.data(), n, c, ta.data());
            CHECK(got == want && ta == tw);
            host_scan_ratio(f, op, mode, on.data(), den.data(), on.data(), n, c, ta.data());
            host_scan_ratio(f, op, mode, num.data(), od.data(), od.data(), n, c, tb.data());
            CHECK(on == want && od == want && ta == tw && tb == tw);
            if (op == HS_PRODUCT && n >= 3) {                                      // zero from the zero term on
              const size_t at = n / 2 + (mode == HS_EXCLUSIVE ? 1 : 0);
              for (size_t k = 0; k < n; k++) CHECK(h_is_zero(f, want.data() + k * L) == (k >= at));
              CHECK(h_is_zero(f, tw.data()));
            }
          }
        }
        if (n >= 8) {                                                              // init and total inside the output
          std::vector<uint64_t> io(x), want(n * L), tw(L), c(x.begin() + 3 * L, x.begin() + 4 * L);
          host_scan(f, op, HS_EXCLUSIVE, x.data(), want.data(), n, c.data(), tw.data());
          host_scan(f, op, HS_EXCLUSIVE, io.data(), io.data(), n, io.data() + 3 * L, io.data() + 6 * L);
          memcpy(want.data() + 6 * L, tw.data(), 8 * L);
          CHECK(io == want);
        }
      }
    }
  }
  printf("check_scan_host ok\n");
  return 0;
}

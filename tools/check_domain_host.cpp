// tools/check_domain_host.cpp -- the host forms of include/lcpc_hip_domain.h under AddressSanitizer and UBSan, without the HIP runtime:
// lcpc_amd/csrc/fft_host.h (what lcpcd_coset_fft, lcpcd_extend and lcpcd_generator run) over host_field.h, with the field table of
// encoding.cpp.  Every buffer is a heap allocation of exactly the size the call may touch.
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -Ilcpc_amd/csrc tools/check_domain_host.cpp \
//       lcpc_amd/csrc/encoding.cpp lcpc_amd/csrc/host_crypto.cpp -lpthread -o check_domain_host && ./check_domain_host
// Checks: coset forward then inverse is the identity in every pairing of forms; shift 1 is the plain transform; block c of the
// bit-reversed extension is the FFT_IO coset transform with the shift s w_m^rev_b(c); the natural extension is its permutation; the
// two-level tables of the device caches (two_level_table), with and without a factor, hold the powers they stand for.
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "fft_host.h"

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
  static const uint32_t undo[6] = {HF_IFFT_II, HF_IFFT_OI, HF_IFFT_IO, HF_FFT_II, HF_FFT_OI, HF_FFT_IO};
  for (int fid = 0; fid < 4; fid++) {
    const FieldDesc& f = *field_desc(fid);
    const int L = f.L;
    uint64_t g[MAXL], s[MAXL];
    host_generator(f, g);
    CHECK(shift_ok(f, g));
    rand_elem(f, s);
    for (uint32_t log_n : {0u, 1u, 2u, 5u, 9u}) {
      const size_t n = (size_t)1 << log_n;
      std::vector<uint64_t> x(n * L);
      for (size_t i = 0; i < n; i++) rand_elem(f, x.data() + i * L);
      for (uint32_t form = 0; form < 6; form++) {
        std::vector<uint64_t> a(x);
        host_coset_fft(f, form, s, a.data(), log_n);
        CHECK(elems_reduced(f, a.data(), n));
        host_coset_fft(f, undo[form], s, a.data(), log_n);
        CHECK(a == x);
        std::vector<uint64_t> b(x), c(x);
        host_coset_fft(f, form, f.r, b.data(), log_n);      // shift 1
        host_fft(f, form, c.data(), log_n);
        CHECK(b == c);
      }
      for (size_t nc : {n, n - (n > 2 ? 1 : 0), n / 2 + 1}) {
        if (nc == 0 || nc > n || (n > 1 && 2 * nc <= n)) continue;
        for (uint32_t b = 0; b < 4; b++) {
          const uint32_t log_m = log_n + b;
          const size_t m = (size_t)1 << log_m;
          std::vector<uint64_t> rev_out(m * L), nat_out(m * L);
          memcpy(rev_out.data(), x.data(), nc * L * 8);
          memcpy(nat_out.data(), x.data(), nc * L * 8);
          host_extend(f, g, rev_out.data(), nc, log_m, true);
          host_extend(f, g, nat_out.data(), nc, log_m, false);
          for (size_t k = 0; k < m; k++) CHECK(!memcmp(nat_out.data() + k * L, rev_out.data() + h_rev(k, log_m) * L, 8 * L));
          uint64_t wm[MAXL];
          root_of(f, log_m, false, wm);
          for (size_t c = 0; c < ((size_t)1 << b); c++) {
            uint64_t sc[MAXL];
            h_pow(f, sc, wm, h_rev(c, b));
            h_mul(f, sc, sc, g);
            std::vector<uint64_t> blk(n * L, 0);
            memcpy(blk.data(), x.data(), nc * L * 8);
            host_coset_fft(f, HF_FFT_IO, sc, blk.data(), log_n);
            CHECK(!memcmp(blk.data(), rev_out.data() + c * n * L, n * L * 8));
          }
        }
      }
    }
  }
  // the two-level tables the device reads: a twiddle table (no factor) and a shift table (factor n^-1), each in a buffer of exactly
  // n_lo + n_hi elements, against the plain powers: v^e = tab[e mod n_lo] * tab[n_lo + e / n_lo] (times the factor)
  for (int fid = 0; fid < 4; fid++) {
    const FieldDesc& f = *field_desc(fid);
    const int L = f.L;
    uint64_t s[MAXL];
    rand_elem(f, s);
    for (uint32_t log_n : {0u, 1u, 5u}) {
      const uint32_t h = log_n / 2;
      const size_t n = (size_t)1 << log_n, n_lo = (size_t)1 << h, n_hi = (size_t)1 << (log_n - h);
      uint64_t w[MAXL], ni[MAXL];
      root_of(f, log_n, false, w);
      n_inverse(f, log_n, ni);
      for (int shifted = 0; shifted < 2; shifted++) {
        const uint64_t* v = shifted ? s : w;
        std::vector<uint64_t> tab((n_lo + n_hi) * L), pw(n * L);
        two_level_table(f, v, n_lo, n_hi, shifted ? ni : nullptr, tab.data());
        powers(f, v, n, pw.data());
        for (size_t e = 0; e < n; e++) {
          uint64_t got[MAXL], want[MAXL];
          h_mul(f, got, tab.data() + (e % n_lo) * L, tab.data() + (n_lo + e / n_lo) * L);
          memcpy(want, pw.data() + e * L, 8 * L);
          if (shifted) h_mul(f, want, want, ni);
          CHECK(!memcmp(got, want, 8 * L));
        }
      }
    }
  }
  printf("check_domain_host ok\n");
  return 0;
}

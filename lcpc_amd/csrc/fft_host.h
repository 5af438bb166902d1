// lcpc_amd/csrc/fft_host.h -- the transforms on the host, on one thread, over host_field.h alone (no HIP): the six FieldFFT forms of
// include/lcpc_hip_fft.h, and over them the coset forms and the extension of include/lcpc_hip_domain.h.  Also what the device side
// builds its tables from: the root of a size and direction, n^-1, powers, the inverse of an element, and the two-level table itself
// (two_level_table).  fft.cpp and domain.cpp hold the entry points; tools/check_domain_host.cpp compiles this header without the HIP
// runtime.
#pragma once
#include <vector>

#include "host_field.h"

namespace lcpc {

// the forms: lcpcf_form's and lcpcd's numbering, and the launchers' (kernels.h FFT_*)
enum : uint32_t { HF_FFT_II = 0, HF_FFT_IO = 1, HF_FFT_OI = 2, HF_IFFT_II = 3, HF_IFFT_IO = 4, HF_IFFT_OI = 5 };
inline bool form_inverse(uint32_t form) { return form >= HF_IFFT_II; }
inline bool form_ii(uint32_t form) { return form == HF_FFT_II || form == HF_IFFT_II; }
inline bool form_dit(uint32_t form) { return form != HF_FFT_IO && form != HF_IFFT_IO; }      // the natural-output forms
inline bool form_in_rev(uint32_t form) { return form == HF_FFT_OI || form == HF_IFFT_OI; }    // input stored bit-reversed
inline bool form_out_rev(uint32_t form) { return form == HF_FFT_IO || form == HF_IFFT_IO; }   // output stored bit-reversed

inline uint64_t h_rev(uint64_t i, uint32_t bits) {
  uint64_t j = 0;
  for (uint32_t b = 0; b < bits; b++) j |= ((i >> b) & 1) << (bits - 1 - b);
  return j;
}

// two ranges of `bytes` bytes overlap without being the same range
inline bool ranges_overlap(const void* a, const void* b, uint64_t bytes) {
  const uintptr_t x = reinterpret_cast<uintptr_t>(a), y = reinterpret_cast<uintptr_t>(b);
  return x != y && (x < y ? y - x < bytes : x - y < bytes);
}

inline bool elems_reduced(const FieldDesc& f, const uint64_t* e, uint64_t n) {
  for (uint64_t i = 0; i < n; i++)
    if (h_ge_p(f, e + i * f.L)) return false;
  return true;
}

inline void h_pow(const FieldDesc& f, uint64_t* o, const uint64_t* base, uint64_t e) {
  uint64_t acc[MAXL], b[MAXL];
  memcpy(acc, f.r, 8 * f.L);
  memcpy(b, base, 8 * f.L);
  for (; e; e >>= 1) {
    if (e & 1) h_mul(f, acc, acc, b);
    h_mul(f, b, b, b);
  }
  memcpy(o, acc, 8 * f.L);
}

// a^-1 = a^(p - 2), a != 0 (p's lowest limb is ...0001 in all four fields: no borrow)
inline void h_inv(const FieldDesc& f, uint64_t* o, const uint64_t* a) {
  uint64_t acc[MAXL], b[MAXL], e[MAXL];
  memcpy(acc, f.r, 8 * f.L);
  memcpy(b, a, 8 * f.L);
  memcpy(e, f.p, 8 * f.L);
  e[0] -= 2;
  for (int i = 0; i < 64 * f.L; i++) {
    if ((e[i / 64] >> (i % 64)) & 1) h_mul(f, acc, acc, b);
    h_mul(f, b, b, b);
  }
  memcpy(o, acc, 8 * f.L);
}

// the root of the direction: w = ROOT_OF_UNITY^(2^(S - log_n)), or w^-1 = w^(n - 1)
inline void root_of(const FieldDesc& f, uint32_t log_n, bool inverse, uint64_t* v) {
  memcpy(v, f.rou, 8 * f.L);
  for (unsigned i = log_n; i < f.S; i++) h_mul(f, v, v, v);
  if (inverse) h_pow(f, v, v, ((uint64_t)1 << log_n) - 1);         // (log_n <= S < 64)
}

// n^-1 = ((p + 1) / 2)^log_n
inline void n_inverse(const FieldDesc& f, uint32_t log_n, uint64_t* o) {
  uint64_t half[MAXL] = {0, 0, 0, 0};
  for (int i = 0; i < f.L; i++) half[i] = (f.p[i] >> 1) | (i + 1 < f.L ? f.p[i + 1] << 63 : 0);      // (p - 1) / 2
  for (int i = 0; i < f.L && ++half[i] == 0; i++) {}
  h_mul(f, half, half, f.r2);
  h_pow(f, o, half, log_n);
}

// out[i] = v^i for i < n
inline void powers(const FieldDesc& f, const uint64_t* v, uint64_t n, uint64_t* out) {
  memcpy(out, f.r, 8 * f.L);
  for (uint64_t i = 1; i < n; i++) h_mul(f, out + i * f.L, out + (i - 1) * f.L, v);
}

// the two-level table of the powers of v that the device kernels read (kernels.h launch_fft, launch_coset_fft): out[i] = v^i for
// i < n_lo, out[n_lo + i] = c v^(i n_lo) for i < n_hi; c null: one.  v^e for e < n_lo n_hi is then one product of two entries
inline void two_level_table(const FieldDesc& f, const uint64_t* v, uint64_t n_lo, uint64_t n_hi, const uint64_t* c, uint64_t* out) {
  uint64_t step[MAXL];
  powers(f, v, n_lo, out);
  h_pow(f, step, v, n_lo);
  uint64_t* hi = out + n_lo * f.L;
  powers(f, step, n_hi, hi);
  if (c)
    for (uint64_t i = 0; i < n_hi; i++) h_mul(f, hi + i * f.L, hi + i * f.L, c);
}

inline void host_fft(const FieldDesc& f, uint32_t form, uint64_t* a, uint32_t log_n) {
  if (log_n == 0) return;
  const int L = f.L;
  const uint64_t n = (uint64_t)1 << log_n;
  uint64_t v[MAXL];
  root_of(f, log_n, form_inverse(form), v);
  std::vector<uint64_t> tab((size_t)(n / 2) * L);
  powers(f, v, n / 2, tab.data());
  if (form_ii(form)) {
    uint64_t t[MAXL];
    for (uint64_t i = 0; i < n; i++) {
      const uint64_t j = h_rev(i, log_n);
      if (i < j) {
        memcpy(t, a + i * L, 8 * L); memcpy(a + i * L, a + j * L, 8 * L); memcpy(a + j * L, t, 8 * L);
      }
    }
  }
  const bool dit = form_dit(form);
  for (uint32_t k = 0; k < log_n; k++) {
    const uint32_t t = dit ? log_n - 1 - k : k;
    const uint64_t h = n >> (t + 1);
    for (uint64_t base = 0; base < n; base += 2 * h)
      for (uint64_t j = 0; j < h; j++) {
        uint64_t* x = a + (base + j) * L;
        uint64_t* y = x + h * L;
        const uint64_t* w = tab.data() + (size_t)(j << t) * L;
        uint64_t s[MAXL];
        if (dit) {
          h_mul(f, y, y, w);
          h_add(f, s, x, y);
          h_sub(f, y, x, y);
          memcpy(x, s, 8 * L);
        } else {
          h_add(f, s, x, y);
          h_sub(f, y, x, y);
          h_mul(f, y, y, w);
          memcpy(x, s, 8 * L);
        }
      }
  }
  if (form_inverse(form)) {
    uint64_t ni[MAXL];
    n_inverse(f, log_n, ni);
    for (uint64_t i = 0; i < n; i++) h_mul(f, a + i * L, a + i * L, ni);
  }
}

// a shift of include/lcpc_hip_domain.h: fully reduced and not zero
inline bool shift_ok(const FieldDesc& f, const uint64_t* s) { return s && !h_ge_p(f, s) && !h_is_zero(f, s); }

// the element with natural index j of every vector times t^j; rev: index j is stored at rev(j)
inline void scale_powers(const FieldDesc& f, uint64_t* a, uint64_t n_scaled, uint32_t log_n, const uint64_t* t, bool rev) {
  uint64_t pw[MAXL];
  memcpy(pw, f.r, 8 * f.L);
  for (uint64_t j = 0; j < n_scaled; j++) {
    uint64_t* e = a + (rev ? h_rev(j, log_n) : j) * f.L;
    h_mul(f, e, e, pw);
    h_mul(f, pw, pw, t);
  }
}

// the coset forms: X[k] = sum_j x[j] s^j w^(jk), and its inverse; in place on a[2^log_n]
inline void host_coset_fft(const FieldDesc& f, uint32_t form, const uint64_t* shift, uint64_t* a, uint32_t log_n) {
  const uint64_t n = (uint64_t)1 << log_n;
  if (!form_inverse(form)) {
    scale_powers(f, a, n, log_n, shift, form_in_rev(form));
    host_fft(f, form, a, log_n);
  } else {
    uint64_t t[MAXL];
    h_inv(f, t, shift);
    host_fft(f, form, a, log_n);
    scale_powers(f, a, n, log_n, t, form_out_rev(form));
  }
}

// the extension: a[2^log_m] holds n_coeffs coefficients in front; Y[k] = sum_j x[j] s^j w_m^(jk) lands at a[k], or at a[rev(k)]
inline void host_extend(const FieldDesc& f, const uint64_t* shift, uint64_t* a, uint64_t n_coeffs, uint32_t log_m, bool out_rev) {
  const uint64_t m = (uint64_t)1 << log_m;
  memset(a + n_coeffs * f.L, 0, (size_t)(m - n_coeffs) * 8 * f.L);
  scale_powers(f, a, n_coeffs, log_m, shift, false);
  host_fft(f, out_rev ? HF_FFT_IO : HF_FFT_II, a, log_m);
}

// ff's multiplicative_generator() in Montgomery limbs
inline void host_generator(const FieldDesc& f, uint64_t* o) {
  uint64_t g[MAXL] = {f.gen, 0, 0, 0};
  h_mul(f, o, g, f.r2);
}

}  // namespace lcpc

// lcpc_amd/csrc/field_ln.h -- lazy signed reduced-radix arithmetic for the four test fields of
// /root/reference/lcpc-test-fields/src/lib.rs:13-59 (ff_derive [3P]: Montgomery form, R = 2^(64 L)): the row NTTs (ntt_l9s.hip for
// Ft255, ntt_lns.hip for the others, kernels.hip ntt_pass_l9_kernel), the carry-free lazy dot products (collapse, SpMV, SpMM).
//
//   field   N limbs x W bits   R' = 2^(N W)   spare bits N W - log2 p   top limb of p (PTOP)
//   Ft63    3 x 26             2^78           15.9                      0x46d     (p >> 52)
//   Ft127   5 x 29             2^145          18.2                      0x6e7     (p >> 116)
//   Ft191   7 x 29             2^203          12.9                      0x8a6e    (p >> 174)
//   Ft255   9 x 29             2^261           6.3                      0x663c79  (p >> 232)
// (26-bit limbs for Ft63: with 29 the top limb of p would be 17, too coarse for the quotient estimate of the clamp.)
//
// Why limbs (measured issue costs on gfx950, profiles/r01_ubench_valu.txt): plain v_add/v_sub/v_and/v_xor cost 2.4 cycles per wave64
// instruction, but v_addc/v_subb (carry chains), v_alignbit, v_add3, 64-bit adds AND v_mad_u64_u32 all ~4.3-4.5.  In the packed 32-bit
// representation a butterfly spends ~25 % of its cycles on carry-chain add/sub and on conversions around the multiply; with W-bit limbs
// a whole Comba column of the Montgomery multiply fits one 64-bit accumulator (a pure chain of mads, no carry handling), and an element
// stays in the multiplier's own format between stages:
//     invariant I ("normalised"):  limbs 0..N-2 in [0, 2^W), top limb two's complement;  |value| < 4p;  value == true value (mod p).
// add / sub are N plain limb operations (differences simply go negative: no bias constants, no borrows); the Montgomery multiply
// (field_ln_gen.h / field_r29_gen.h: ONE asm statement, N^2 + N(N-1) v_mad_i64_i32 on a single 64-bit accumulator, negative quotient
// digits; p == 1 mod 2^W, so the quotient digit is a negate-and-mask) accepts limbs in (-2^(W+1), 2^(W+1)), |value| < 16p, and returns
// a normalised value in (-p - eps, eps], eps = 16 p^2 / R' (Ft255: (-1.2p, 0.2p]); sums of sums are brought back to [0, p + 64 B),
// B = 2^(W(N-1)), by the quotient-estimate clamp.  Data stays in ff_derive's R = 2^(32 NL) form in HBM: the twiddles are pre-scaled
// to w^i R' mod p, so that REDC_R'(a R * w R') = (a w) R.  Exact reduction to [0, p) happens once per element, at the last pass's
// store.  Bounds are stated at every step here and in the kernels; tests/test_gpu_edges.py and tests/test_gpu_lazy_worst.py push them.
#pragma once
#include "field_dev.h"

namespace lcpc {

// k-th W-bit limb of the modulus of NL 32-bit words
template <int NL, int W> constexpr u32 mod_limb(int k) {
  const int b = W * k, w = b / 32, sh = b % 32;
  const u64 lo = Mod<NL>::P[w], hi = (w + 1 < NL) ? Mod<NL>::P[w + 1] : 0;
  return (u32)(((lo | (hi << 32)) >> sh) & ((1u << W) - 1));
}
// WAVES: the occupancy the row NTT of the field is built for; STRIDE: words per entry of the limb-form tables (twiddles, q*p rows)
template <int FID> struct LnField;
template <> struct LnField<FT63> {
  static constexpr int FID = FT63, N = 3, W = 26, NL = 2, WAVES = 8, STRIDE = 4;
  static constexpr u32 limb(int k) { return mod_limb<NL, W>(k); }
};
template <> struct LnField<FT127> {
  static constexpr int FID = FT127, N = 5, W = 29, NL = 4, WAVES = 7, STRIDE = 8;
  static constexpr u32 limb(int k) { return mod_limb<NL, W>(k); }
};
template <> struct LnField<FT191> {
  static constexpr int FID = FT191, N = 7, W = 29, NL = 6, WAVES = 5, STRIDE = 8;
  static constexpr u32 limb(int k) { return mod_limb<NL, W>(k); }
};
template <> struct LnField<FT255> {
  static constexpr int FID = FT255, N = 9, W = 29, NL = 8, WAVES = 4, STRIDE = 12;
  static constexpr u32 limb(int k) { return mod_limb<NL, W>(k); }
};

#include "field_ln_gen.h"    // ln_mul1s_ft63 / _ft127 / _ft191
#include "field_r29_gen.h"   // Ft255: r29_columns (fe_mul_r29's Comba/Montgomery chain as asm blocks), r29_mul1s, r29_mul2s
#include "field_wmul_gen.h"  // wmul_u / _ft127 / _ft191: x * w mod p for a WAVE-UNIFORM w given as its shifted multiples (scalar operands)

template <int N> struct LN {
  u32 v[N];       // two's complement; the top limb (and un-normalised intermediates) may be negative
};

namespace ln {
constexpr int QOFF = 24;          // clamp table: entry i = (i - QOFF) * p, i in [0, 64)
constexpr int QBIAS = 40;         // subtracted from the top limb before the quotient estimate (keeps remainders >= 0)

// packed NL x 32 (value < 2^(32 NL)) -> N x W, normalised, non-negative.  The top limb takes every bit from W (N - 1) up:
// 12 bits for Ft63 / Ft127, 18 for Ft191, 24 for Ft255.
template <class FT> LCPC_DEV LN<FT::N> from_packed(const Fe<FT::NL>& a) {
  constexpr int N = FT::N, W = FT::W, NL = FT::NL;
  LN<N> r;
#pragma unroll
  for (int k = 0; k < N; k++) {
    const int b = W * k, w = b / 32, sh = b % 32;
    u32 x;
    if (sh == 0) x = a.v[w];
    else if (w + 1 < NL) x = __builtin_amdgcn_alignbit(a.v[w + 1], a.v[w], sh);
    else x = a.v[w] >> sh;
    r.v[k] = k + 1 < N ? (x & ((1u << W) - 1)) : x;
  }
  return r;
}
// N x W (limbs 0..N-2 in [0, 2^W), top limb >= 0, value < 2^(32 NL)) -> packed
template <class FT> LCPC_DEV void to_packed(u32* out, const u32* l) {
  constexpr int N = FT::N, W = FT::W, NL = FT::NL;
#pragma unroll
  for (int w = 0; w < NL; w++) {
    u32 x = 0;
#pragma unroll
    for (int k = 0; k < N; k++) {
      const int off = W * k - 32 * w;                 // bit position of limb k inside word w
      if (off >= 0 && off < 32) x |= l[k] << off;
      else if (off < 0 && off > -32) x |= l[k] >> (-off);
    }
    out[w] = x;
  }
}
// N consecutive words (16-byte aligned) as uint4 / uint2 / u32 loads: limbs 0-3 (N >= 5) and 4-7 (N = 9) as uint4, a uint2 for
// limbs 0-1 (N = 3) or 4-5 (N = 7), then the top limb
template <int N> LCPC_DEV LN<N> load_limbs(const u32* t) {
  LN<N> r;
  if constexpr (N == 3) {
    const uint2 a = *reinterpret_cast<const uint2*>(t);
    r.v[0] = a.x; r.v[1] = a.y; r.v[2] = t[2];
  } else {
    const uint4 a = *reinterpret_cast<const uint4*>(t);
    r.v[0] = a.x; r.v[1] = a.y; r.v[2] = a.z; r.v[3] = a.w;
    if constexpr (N == 5) r.v[4] = t[4];
    else if constexpr (N == 7) { const uint2 b = *reinterpret_cast<const uint2*>(t + 4); r.v[4] = b.x; r.v[5] = b.y; r.v[6] = t[6]; }
    else { const uint4 b = *reinterpret_cast<const uint4*>(t + 4); r.v[4] = b.x; r.v[5] = b.y; r.v[6] = b.z; r.v[7] = b.w; r.v[8] = t[8]; }
  }
  return r;
}
template <int N> LCPC_DEV LN<N> add(const LN<N>& a, const LN<N>& b) {
  LN<N> r;
#pragma unroll
  for (int k = 0; k < N; k++) r.v[k] = a.v[k] + b.v[k];
  return r;
}
template <int N> LCPC_DEV LN<N> sub(const LN<N>& a, const LN<N>& b) {
  LN<N> r;
#pragma unroll
  for (int k = 0; k < N; k++) r.v[k] = a.v[k] - b.v[k];
  return r;
}
// carry-propagate signed limbs (|limb| < 2^31): limbs 0..N-2 -> [0, 2^W), the top limb takes what is left (signed)
template <class FT> LCPC_DEV void normalize(LN<FT::N>& a) {
#pragma unroll
  for (int k = 0; k + 1 < FT::N; k++) {
    a.v[k + 1] += (u32)((int32_t)a.v[k] >> FT::W);
    a.v[k] &= (1u << FT::W) - 1;
  }
}
// ---- normalise + clamp in ONE carry pass -----------------------------------------------------------------------------------------
// a: |value| < 16p, the top limb signed, and limbs 0..N-2 of one of two classes (W = 29):
//   (a) in [0, 2^31 - 4]: the sum of four normalised values.  The carries still in the lower limbs are c in [0, 3];
//   (b) signed, in (-2^30, 2^30): differences and sums of up to two differences of normalised values, un-normalised (K1s, ntt_l9s.hip:
//       the outputs of a butterfly as they leave it).  c in [-2, 2]: the lower limbs hold a value in (-2.01 B, 2.01 B).
// With B = 2^(W(N-1)), V = t B + low, q = floor((t - QBIAS) / (PTOP + 1)) estimated from the UN-normalised top limb (c is not in it yet):
//   V - q p = q (B - plow) + (rem + QBIAS + c) B + low'  (0 <= low' < B, 0 <= rem <= PTOP, 0 < B - plow <= B)
//   (a)  >= (QBIAS - |q|) B >= 0,         <  (PTOP + 1 + QBIAS + |q| + 3) B        for |q| <= 17 + 1,
//   (b)  >= (QBIAS - |q| - 2.01) B > 0,   <  (PTOP + 1 + QBIAS + |q| + 2.01) B     for |q| <= 18:   both inside [0, p + 64 B).
// The carry pass is signed: d below stays inside an i32 for either class ((a): < 2^31 - 4 + 3; (b): the row's limbs lie in (-2^W, 0],
// so d > -2^30 - 2^29 - 4), and leaves limbs 0..N-2 in [0, 2^W) and a top limb in [0, PTOP + 64]: a normalised value that to_packed takes.
// The table index n / (PTOP + 1) lies in [0, 64): |t| < 16 (PTOP + 1) + 3.  tests/test_clamp_lazy_inputs.py runs this on integers at the
// extremes of both classes.
// The row -(q p) comes from a table in LDS (the kernel negates ctx.cpp's (i - QOFF) p table when it copies it).
template <class FT> LCPC_DEV u32 clamp_q(u32 top) {
  constexpr u32 PTOP1 = FT::limb(FT::N - 1) + 1;
  constexpr int SH = 31 - __builtin_clz(PTOP1);                         // floor(log2 PTOP1)
  constexpr u32 MAGIC = (u32)((((u64)1 << (32 + SH)) + PTOP1 - 1) / PTOP1);   // ceil(2^(32+SH) / PTOP1) < 2^32
  // exact floor(n / PTOP1) while n * (MAGIC * PTOP1 - 2^(32+SH)) < 2^(32+SH): n < 64 PTOP1 here, the excess is < PTOP1
  static_assert((u64)64 * PTOP1 * PTOP1 < ((u64)1 << (32 + SH)), "magic division range");
  const u32 n = top + (u32)(QOFF * PTOP1 - QBIAS);                       // in [0, 64 PTOP1) for |value| < 16p
  return __umulhi(n, MAGIC) >> SH;
}
template <class FT> LCPC_DEV LN<FT::N> clamp_row(const u32* nqp, u32 q) { return load_limbs<FT::N>(nqp + q * FT::STRIDE); }
template <class FT> LCPC_DEV void clamp_apply(LN<FT::N>& a, const LN<FT::N>& nt) {
  int32_t c = 0;
#pragma unroll
  for (int k = 0; k + 1 < FT::N; k++) {
    const int32_t d = (int32_t)(a.v[k] + nt.v[k] + (u32)c);             // in (-2^W - 1, 2^31): fits i32
    a.v[k] = (u32)d & ((1u << FT::W) - 1);
    c = d >> FT::W;
  }
  a.v[FT::N - 1] = a.v[FT::N - 1] + nt.v[FT::N - 1] + (u32)c;
}
// (a * w) / R' mod p, loosely: a limbs in (-2^(W+1), 2^(W+1)), |value| < 16p; w normalised, in [0, p) (R'-Montgomery form).
// Ft255: column sums stay inside i64 (9 * 2^59 + 8 * 2^58 + 2^34 < 2^63); result normalised, in (-1.2p, 0.2p].
template <class FT> LCPC_DEV LN<FT::N> mul(const LN<FT::N>& a, const LN<FT::N>& w) {
  LN<FT::N> r;
  if constexpr (FT::FID == FT63) ln_mul1s_ft63(a.v, w.v, r.v);
  else if constexpr (FT::FID == FT127) ln_mul1s_ft127(a.v, w.v, r.v);
  else if constexpr (FT::FID == FT191) ln_mul1s_ft191(a.v, w.v, r.v);
  else r29_mul1s(a.v, w.v, r.v);
  return r;
}
// Ft255, the two-table form of the same multiply for a lane-varying twiddle (K1s's split plans, ntt_l9s.hip): a = AL + 2^145 AH (limbs
// 0-4 | 5-8) and the twiddle as TWO entries b0 = w c 2^145 mod p, b1 = w c 2^290 mod p, both normalised in [0, p) (c: the scale of the
// table entry w c R', 1 or 2^5 / R'; the packs of ntt_lns.hip hold both).  Z = AL b0 + AH b1 == a w c 2^145 fills 13 columns, so five
// Montgomery digits instead of nine bring it back to nine limbs: 81 + 40 mads against 81 + 72 (field_r29_gen.h r29_mul2s, 148
// instructions against 188).  a: limbs in (-2^30, 2^30) -- no bound on the value beyond that.  Column sums stay inside i64 (9 * 2^59 +
// 5 * 2^58 + 2^35 < 2^63).  Result == a w c (mod p), normalised, in (Z / 2^145 - p, Z / 2^145]:
//   limbs in (-2^30, 2^30):                                          (-3.01p, 2.01p)
//   a difference of two normalised values (limbs 0-7 in (-2^29, 2^29)): (-2.01p, 1.01p)
//   a normalised value:                                              (-1.01p, 1.01p)
// (wider than mul()'s (-1.2p, 0.2p] because only 2^145, not 2^261, is divided out; tests/test_gen_r29_mul2.py proves and checks them).
template <class FT> LCPC_DEV LN<FT::N> mul2(const LN<FT::N>& a, const LN<FT::N>& b0, const LN<FT::N>& b1) {
  static_assert(FT::FID == FT255, "the two-table multiply exists for Ft255 only");
  LN<FT::N> r = b1;                                            // (b1 arrives in the result registers: it is dead before they are written)
  r29_mul2s(a.v, b0.v, r.v);
  return r;
}
// a table entry e = w c R' in [0, p) -> the pair (b0, b1) of mul2: e 2^-116 and e 2^29, fully reduced (pack kernels, ntt_lns.hip)
template <class FT> LCPC_DEV void mul2_pair(const LN<FT::N>& e, LN<FT::N>& b0, LN<FT::N>& b1) {
  static_assert(FT::FID == FT255, "the two-table multiply exists for Ft255 only");
#pragma unroll
  for (int t = 0; t < 2; t++) {
    LN<FT::N> kk;
#pragma unroll
    for (int z = 0; z < FT::N; z++) kk.v[z] = t ? R29_MUL2_KB[z] : R29_MUL2_KA[z];
    LN<FT::N> x = mul<FT>(kk, e);                              // (-1.2p, 0.2p], normalised: + p while negative lands in [0, p)
    for (int it = 0; it < 2; it++) {
      if ((int32_t)x.v[FT::N - 1] < 0) {
#pragma unroll
        for (int z = 0; z < FT::N; z++) x.v[z] += FT::limb(z);
        normalize<FT>(x);
      }
    }
    (t ? b1 : b0) = x;
  }
}
// a * w mod p for a wave-uniform w given as its N shifted multiples W_j = balanced(w 2^(W j) mod p) (N^2 words t = N k + j, host:
// ctx.cpp wmul_table; field_wmul_gen.h).  a: limbs of a normalised value or of a difference of two (sum |limb| < N 2^W).  Result:
// normalised, in (-2.5p, 1.6p) (gen_wmul_asm.py wmul_bounds; Ft255: (-2p, 2.7p)).  Ft127: 50 instructions against mul()'s 64, Ft191:
// 80 against 118, Ft255: 119 against 188 (tools/lab, profiles/r05_ubench_wmul.jsonl: 1.6-1.8 x per second).
// Ft63 has no such form: at 3 limbs the Montgomery multiply (22 instructions) is the shorter one (28).
template <class FT> constexpr bool has_mul_u = FT::N >= 5;
template <class FT> LCPC_DEV LN<FT::N> mul_u(const LN<FT::N>& a, const u32* wt) {
  static_assert(has_mul_u<FT>, "no shifted-multiples multiply for this field");
  LN<FT::N> r;
  if constexpr (FT::FID == FT127) wmul_u_ft127(a.v, wt, r.v);
  else if constexpr (FT::FID == FT191) wmul_u_ft191(a.v, wt, r.v);
  else {
    u32 np2[9];
#pragma unroll
    for (int j = 0; j < 9; j++) np2[j] = 0u - 2u * FT::limb(j);           // the limbs of -2p (the quotient counts units of 2p)
    wmul_u(a.v, np2, wt, r.v);
  }
  return r;
}
// Ft255, the K1s kernels' form of the same multiply (ntt_l9s.hip): wmul_us, whose top limb is formed from the low words of its column
// alone -- two instructions and a carry pair fewer, bit for bit mul_u's result (gen_wmul_asm.py build(short_tail);
// tests/test_gen_short_tails.py runs both lists on integers)
template <class FT> LCPC_DEV LN<FT::N> mul_us(const LN<FT::N>& a, const u32* wt) {
  static_assert(FT::FID == FT255, "the short-tail statement exists for Ft255 only");
  LN<FT::N> r;
  u32 np2[9];
#pragma unroll
  for (int j = 0; j < 9; j++) np2[j] = 0u - 2u * FT::limb(j);
  wmul_us(a.v, np2, wt, r.v);
  return r;
}
// ---- carry-free lazy dot product (collapse, SpMV, SpMM) -----------------------------------------------------------------------------
// acc += x * v with x, v as N unsigned W-bit limbs (x: a packed element < p split by from_packed; v: a matrix / tensor value in the
// R'-Montgomery form, v R' mod p): N^2 v_mad_u64_u32 into 2N u64 columns, no carries.  A column receives <= N products
// < 2^(2W) per term: 6 terms fit (6 * 9 * 2^58 < 2^64) before lazy_normalize() must move the excess up; the value is
// Montgomery-reduced once per <= 60 terms: (sum + m p) / R' < 60 p^2 / R' + p < 2p since R' / p > 2^6 (Ft255: value < 64 p^2;
// tests/test_lazy_bounds.py derives the limits).
template <class FT> struct LazyN {
  u64 c[2 * FT::N];
};
template <class FT> LCPC_DEV void lazy_zero(LazyN<FT>& a) {
#pragma unroll
  for (int k = 0; k < 2 * FT::N; k++) a.c[k] = 0;
}
template <class FT> LCPC_DEV void lazy_mac(LazyN<FT>& a, const LN<FT::N>& x, const LN<FT::N>& v) {
#pragma unroll
  for (int i = 0; i < FT::N; i++)
#pragma unroll
    for (int j = 0; j < FT::N; j++) a.c[i + j] += (u64)x.v[i] * v.v[j];
}
template <class FT> LCPC_DEV void lazy_normalize(LazyN<FT>& a) {
#pragma unroll
  for (int k = 0; k + 1 < 2 * FT::N; k++) {
    a.c[k + 1] += a.c[k] >> FT::W;
    a.c[k] &= (1u << FT::W) - 1;
  }
}
// value / R' mod p, fully reduced, packed
template <class FT> LCPC_DEV Fe<FT::NL> lazy_reduce(LazyN<FT>& a) {
  constexpr int N = FT::N, W = FT::W;
  constexpr u32 M = (1u << W) - 1;
  lazy_normalize<FT>(a);
  u32 m[N], r[N];
  u64 acc = 0;
#pragma unroll
  for (int k = 0; k < 2 * N; k++) {
    acc += a.c[k];
#pragma unroll
    for (int i = 0; i < N; i++) {
      const int j = k - i;
      if (i < k && j >= 1 && j < N) acc += (u64)m[i] * FT::limb(j);
    }
    if (k < N) {
      m[k] = (0u - (u32)acc) & M;          // p == 1 mod 2^W: the quotient digit is a negate-and-mask
      acc += m[k];
      acc >>= W;
    } else {
      r[k - N] = (u32)acc & M;
      acc >>= W;
    }
  }
  u32 t[FT::NL];
  to_packed<FT>(t, r);
  return fe_reduce_once<FT::NL>(t);        // < 2p < 2^(32 NL)
}

// ---- Ft255 only: the general row NTT (kernels.hip ntt_pass_l9_kernel) and its canonical store ----------------------------------------
// a: normalised, |value| < 16p  ->  normalised, value in [0, p + 2^239) (== a mod p).  qp[i] = (i - QOFF) * p as normalised signed
// limbs (12-word stride).  With t the signed top limb, V = t * 2^232 + low, 0 <= low < 2^232, and q = floor((t - QBIAS) / (ptop + 1)),
// ptop = floor(p / 2^232):  t - QBIAS = q (ptop + 1) + rem, so  V - q p = q (2^232 - plow) + (rem + QBIAS) 2^232 + low  with
// plow = p mod 2^232:  >= (QBIAS - |q|) 2^232 >= 0 for |q| <= 17 + 1 and < (ptop + 1 + QBIAS + |q| + 1) 2^232 < p + 2^239.
LCPC_DEV void clamp(LN<9>& a, const u32* qp) {
  constexpr u32 M = (1u << 29) - 1;
  constexpr u32 PTOP1 = LnField<FT255>::limb(8) + 1;                     // floor(p / 2^232) + 1 (23 bits)
  constexpr u64 MAGIC = (((u64)1 << 52) + PTOP1 - 1) / PTOP1;            // ceil(2^52 / PTOP1) < 2^30
  const u32 n = a.v[8] + (u32)(QOFF * PTOP1 - QBIAS);                    // in [0, 2^29) for |value| < 16p
  const u32 q = (u32)(((u64)n * MAGIC) >> 52);                           // exact floor(n / PTOP1) for n < 2^29
  const u32* t = qp + q * 12;
  int32_t d[9];
#pragma unroll
  for (int k = 0; k < 9; k++) d[k] = (int32_t)(a.v[k] - t[k]);
#pragma unroll
  for (int k = 0; k < 8; k++) {                                         // borrow-propagate
    d[k + 1] += d[k] >> 31;                                             // -1 if limb k went negative
    a.v[k] = (u32)d[k] & M;                                             // + 2^29 in that case
  }
  a.v[8] = (u32)d[8];
}
// exact: normalised |value| < 16p -> packed, fully reduced
LCPC_DEV Fe<8> to_packed_reduced(LN<9> a, const u32* qp) {
  clamp(a, qp);                   // [0, p + 2^239) < 2^256
  u32 t[8];
  to_packed<LnField<FT255>>(t, a.v);
  return fe_reduce_once<8>(t);
}
}  // namespace ln

// r = a * b * 2^-261 mod p, fully reduced, packed.  a: packed element < p; b: 9 limbs < 2^29 (a table entry, w 2^261 mod p, so that
// REDC_261(a R * w 2^261) = (a w) R).  The product and the reduction are one pure chain of 153 v_mad_u64_u32 (field_r29_gen.h).
LCPC_DEV Fe<8> fe_mul_r29(const Fe<8>& a, const LN<9>& b) {
  const LN<9> x = ln::from_packed<LnField<FT255>>(a);
  u32 m[9], r[9];
  r29_columns(x.v, b.v, m, r);
  u32 t[8];
  ln::to_packed<LnField<FT255>>(t, r);
  return fe_reduce_once<8>(t);         // REDC output < 2p < 2^256
}

// Montgomery form (R = 2^256) -> canonical value for Ft255, reduction only: a * 2^-256 = REDC_261(a * 2^5).
// The "product" a << 5 needs no multiplies; the 9-step reduction is 72 v_mad_u64_u32, carry-free.
LCPC_DEV Fe<8> fe_canon_r29(const Fe<8>& a) {
  using FT = LnField<FT255>;
  constexpr u32 M = (1u << 29) - 1;
  // limbs of (a << 5): bit b of the shifted value is bit b-5 of a
  u32 x[9];
#pragma unroll
  for (int k = 0; k < 9; k++) {
    const int b = 29 * k - 5;            // first source bit of limb k (negative for k = 0)
    u32 v;
    if (k == 0) v = (a.v[0] << 5);
    else {
      const int w = b / 32, sh = b % 32;
      if (sh == 0) v = a.v[w];
      else if (w + 1 < 8) v = __builtin_amdgcn_alignbit(a.v[w + 1], a.v[w], sh);
      else v = a.v[w] >> sh;
    }
    x[k] = v & M;
  }
  u32 m[9], r[9];
  u64 acc = 0;
#pragma unroll
  for (int k = 0; k < 17; k++) {
    if (k < 9) acc += x[k];
#pragma unroll
    for (int i = 0; i < 9; i++) {
      const int j = k - i;
      if (i < k && j >= 1 && j < 9) acc += (u64)m[i] * FT::limb(j);
    }
    if (k < 9) {
      m[k] = (0u - (u32)acc) & M;
      acc += m[k];
      acc >>= 29;
    } else {
      r[k - 9] = (u32)acc & M;
      acc >>= 29;
    }
  }
  r[8] = (u32)acc;
  u32 t[8];
  ln::to_packed<FT>(t, r);
  return fe_reduce_once<8>(t);
}

}  // namespace lcpc

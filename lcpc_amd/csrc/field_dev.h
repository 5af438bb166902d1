// lcpc_amd/csrc/field_dev.h -- device-side prime-field arithmetic for gfx950 (MI355X).
//
// Replaces, on the GPU, what `#[derive(PrimeField)]` generates for the reference's four test
// fields (/root/reference/lcpc-test-fields/src/lib.rs:13-59, ff_derive [3P]): elements are
// a*R mod p with R = 2^(64 L), stored as L little-endian u64 limbs, always fully reduced (< p).
// On the device the same bytes are viewed as NL = 2L little-endian 32-bit limbs, because the
// widest integer multiplier CDNA4 has is v_mad_u64_u32 (32x32+64 -> 64).
//
// All four moduli are == 1 mod 2^32, so -p^-1 mod 2^32 = 0xffffffff and the Montgomery
// quotient digit is just a negation (m = -t0): no multiply for it, and m*p[0] is free.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace lcpc {

// Wave priority around the memory phases of the VALU-bound kernels (the row NTTs, the column hash): a wave that is about to issue its
// few loads / LDS reads and then wait for them (tile load, the reads and twiddle loads at the top of a round, the store phase) takes
// priority 1, a wave inside its multiplier / compression chains priority 0 -- so the memory instructions of one wave are not queued
// behind hundreds of arithmetic instructions of its three neighbours on the SIMD and its latency starts to run at once.  Measured,
// same box, interleaved: headline commit 9.57 -> 9.32 ms (levels 1, 2, 3 alike).  Placement only; results are unaffected.
__device__ __forceinline__ void mem_phase(bool on) {
#ifdef __HIP_DEVICE_COMPILE__
  if (on) __builtin_amdgcn_s_setprio(1);
  else __builtin_amdgcn_s_setprio(0);
#else
  (void)on;
#endif
}

typedef uint32_t u32;
typedef uint64_t u64;

#define LCPC_DEV __device__ __forceinline__

// field ids match include/lcpc_hip.h
enum { FT63 = 0, FT127 = 1, FT191 = 2, FT255 = 3 };

template <int NL> struct Mod;   // modulus, 32-bit limbs, little-endian
template <> struct Mod<2> { static constexpr u32 P[2] = {0x00000001u, 0x46d07600u}; };
template <> struct Mod<4> { static constexpr u32 P[4] = {0x00000001u, 0x7f2bd900u, 0xba20e0bfu, 0x6e754097u}; };
template <> struct Mod<6> { static constexpr u32 P[6] = {0x00000001u, 0xd2468200u, 0x0ceecbcdu, 0x93688827u, 0x3fbc8ddau, 0x453708aau}; };
template <> struct Mod<8> { static constexpr u32 P[8] = {0x00000001u, 0x02a4f200u, 0x86595f30u, 0xef73c790u,
                                                        0xb9575969u, 0xfda9df04u, 0x6e4d2900u, 0x663c799bu}; };

// ---- element container: NL 32-bit limbs in registers ------------------------------------------
template <int NL> struct Fe {
  u32 v[NL];
};

template <int NL> LCPC_DEV Fe<NL> fe_zero() {
  Fe<NL> r;
#pragma unroll
  for (int i = 0; i < NL; i++) r.v[i] = 0;
  return r;
}

// global memory access: an element is NL*4 contiguous bytes (8, 16, 24 or 32), 8-byte aligned.
template <int NL> LCPC_DEV Fe<NL> fe_load(const u32* __restrict__ p) {
  Fe<NL> r;
  if constexpr (NL % 4 == 0) {
    const uint4* q = reinterpret_cast<const uint4*>(p);
#pragma unroll
    for (int i = 0; i < NL / 4; i++) {
      uint4 t = q[i];
      r.v[4 * i] = t.x; r.v[4 * i + 1] = t.y; r.v[4 * i + 2] = t.z; r.v[4 * i + 3] = t.w;
    }
  } else {
    const uint2* q = reinterpret_cast<const uint2*>(p);
#pragma unroll
    for (int i = 0; i < NL / 2; i++) {
      uint2 t = q[i];
      r.v[2 * i] = t.x; r.v[2 * i + 1] = t.y;
    }
  }
  return r;
}
template <int NL> LCPC_DEV void fe_store(u32* __restrict__ p, const Fe<NL>& a) {
  if constexpr (NL % 4 == 0) {
    uint4* q = reinterpret_cast<uint4*>(p);
#pragma unroll
    for (int i = 0; i < NL / 4; i++) q[i] = make_uint4(a.v[4 * i], a.v[4 * i + 1], a.v[4 * i + 2], a.v[4 * i + 3]);
  } else {
    uint2* q = reinterpret_cast<uint2*>(p);
#pragma unroll
    for (int i = 0; i < NL / 2; i++) q[i] = make_uint2(a.v[2 * i], a.v[2 * i + 1]);
  }
}


// ---- add / sub --------------------------------------------------------------------------------
// r = a + b mod p; 2p < 2^(32 NL) so the plain sum never carries out.
template <int NL> LCPC_DEV Fe<NL> fe_add(const Fe<NL>& a, const Fe<NL>& b) {
  Fe<NL> s, d;
  u32 c = 0;
#pragma unroll
  for (int i = 0; i < NL; i++) {
    u64 t = (u64)a.v[i] + b.v[i] + c;
    s.v[i] = (u32)t;
    c = (u32)(t >> 32);
  }
  u32 br = 0;
#pragma unroll
  for (int i = 0; i < NL; i++) {
    u64 t = (u64)s.v[i] - Mod<NL>::P[i] - br;
    d.v[i] = (u32)t;
    br = (u32)(t >> 63);
  }
#pragma unroll
  for (int i = 0; i < NL; i++) s.v[i] = br ? s.v[i] : d.v[i];
  return s;
}
template <int NL> LCPC_DEV Fe<NL> fe_sub(const Fe<NL>& a, const Fe<NL>& b) {
  Fe<NL> d, s;
  u32 br = 0;
#pragma unroll
  for (int i = 0; i < NL; i++) {
    u64 t = (u64)a.v[i] - b.v[i] - br;
    d.v[i] = (u32)t;
    br = (u32)(t >> 63);
  }
  u32 c = 0;
#pragma unroll
  for (int i = 0; i < NL; i++) {
    u64 t = (u64)d.v[i] + Mod<NL>::P[i] + c;
    s.v[i] = (u32)t;
    c = (u32)(t >> 32);
  }
#pragma unroll
  for (int i = 0; i < NL; i++) d.v[i] = br ? s.v[i] : d.v[i];
  return d;
}

// ---- Ft255 add / sub as explicit VCC carry chains ---------------------------------------------
// hipcc lowers the portable u64-based add/sub above to ~90 instructions (64-bit adds + moves);
// the hardware carry chain is 8 + 8 + 8.  Two asm statements each, so that no carry flag lives
// across a statement boundary (hipcc does not model VCC inside an asm string).
#define LCPC_P8_1 "0x02a4f200"
#define LCPC_P8_2 "0x86595f30"
#define LCPC_P8_3 "0xef73c790"
#define LCPC_P8_4 "0xb9575969"
#define LCPC_P8_5 "0xfda9df04"
#define LCPC_P8_6 "0x6e4d2900"
#define LCPC_P8_7 "0x663c799b"
template <> LCPC_DEV Fe<8> fe_add<8>(const Fe<8>& a, const Fe<8>& b) {
  Fe<8> r;
  u32 d0, d1, d2, d3, d4, d5, d6, d7;
  asm("v_add_co_u32 %0, vcc, %8, %16\n\t"
      "v_addc_co_u32 %1, vcc, %9, %17, vcc\n\t"
      "v_addc_co_u32 %2, vcc, %10, %18, vcc\n\t"
      "v_addc_co_u32 %3, vcc, %11, %19, vcc\n\t"
      "v_addc_co_u32 %4, vcc, %12, %20, vcc\n\t"
      "v_addc_co_u32 %5, vcc, %13, %21, vcc\n\t"
      "v_addc_co_u32 %6, vcc, %14, %22, vcc\n\t"
      "v_addc_co_u32 %7, vcc, %15, %23, vcc"
      : "=&v"(r.v[0]), "=&v"(r.v[1]), "=&v"(r.v[2]), "=&v"(r.v[3]), "=&v"(r.v[4]), "=&v"(r.v[5]), "=&v"(r.v[6]), "=&v"(r.v[7])
      : "v"(a.v[0]), "v"(a.v[1]), "v"(a.v[2]), "v"(a.v[3]), "v"(a.v[4]), "v"(a.v[5]), "v"(a.v[6]), "v"(a.v[7]),
        "v"(b.v[0]), "v"(b.v[1]), "v"(b.v[2]), "v"(b.v[3]), "v"(b.v[4]), "v"(b.v[5]), "v"(b.v[6]), "v"(b.v[7])
      : "vcc");
  // d = r - p; keep r if that borrows (r < p)
  asm("v_subrev_co_u32 %8, vcc, 1, %0\n\t"
      "v_subbrev_co_u32 %9, vcc, %16, %1, vcc\n\t"
      "v_subbrev_co_u32 %10, vcc, %17, %2, vcc\n\t"
      "v_subbrev_co_u32 %11, vcc, %18, %3, vcc\n\t"
      "v_subbrev_co_u32 %12, vcc, %19, %4, vcc\n\t"
      "v_subbrev_co_u32 %13, vcc, %20, %5, vcc\n\t"
      "v_subbrev_co_u32 %14, vcc, %21, %6, vcc\n\t"
      "v_subbrev_co_u32 %15, vcc, %22, %7, vcc\n\t"
      "v_cndmask_b32 %0, %8, %0, vcc\n\t"
      "v_cndmask_b32 %1, %9, %1, vcc\n\t"
      "v_cndmask_b32 %2, %10, %2, vcc\n\t"
      "v_cndmask_b32 %3, %11, %3, vcc\n\t"
      "v_cndmask_b32 %4, %12, %4, vcc\n\t"
      "v_cndmask_b32 %5, %13, %5, vcc\n\t"
      "v_cndmask_b32 %6, %14, %6, vcc\n\t"
      "v_cndmask_b32 %7, %15, %7, vcc"
      : "+v"(r.v[0]), "+v"(r.v[1]), "+v"(r.v[2]), "+v"(r.v[3]), "+v"(r.v[4]), "+v"(r.v[5]), "+v"(r.v[6]), "+v"(r.v[7]),
        "=&v"(d0), "=&v"(d1), "=&v"(d2), "=&v"(d3), "=&v"(d4), "=&v"(d5), "=&v"(d6), "=&v"(d7)
      : "v"(Mod<8>::P[1]), "v"(Mod<8>::P[2]), "v"(Mod<8>::P[3]), "v"(Mod<8>::P[4]), "v"(Mod<8>::P[5]), "v"(Mod<8>::P[6]), "v"(Mod<8>::P[7])
      : "vcc");
  return r;
}
template <> LCPC_DEV Fe<8> fe_sub<8>(const Fe<8>& a, const Fe<8>& b) {
  Fe<8> r;
  u32 mask, t0, t1, t2, t3, t4, t5, t6, t7;
  asm("v_sub_co_u32 %0, vcc, %9, %17\n\t"
      "v_subb_co_u32 %1, vcc, %10, %18, vcc\n\t"
      "v_subb_co_u32 %2, vcc, %11, %19, vcc\n\t"
      "v_subb_co_u32 %3, vcc, %12, %20, vcc\n\t"
      "v_subb_co_u32 %4, vcc, %13, %21, vcc\n\t"
      "v_subb_co_u32 %5, vcc, %14, %22, vcc\n\t"
      "v_subb_co_u32 %6, vcc, %15, %23, vcc\n\t"
      "v_subb_co_u32 %7, vcc, %16, %24, vcc\n\t"
      "v_cndmask_b32 %8, 0, -1, vcc"
      : "=&v"(r.v[0]), "=&v"(r.v[1]), "=&v"(r.v[2]), "=&v"(r.v[3]), "=&v"(r.v[4]), "=&v"(r.v[5]), "=&v"(r.v[6]), "=&v"(r.v[7]),
        "=&v"(mask)
      : "v"(a.v[0]), "v"(a.v[1]), "v"(a.v[2]), "v"(a.v[3]), "v"(a.v[4]), "v"(a.v[5]), "v"(a.v[6]), "v"(a.v[7]),
        "v"(b.v[0]), "v"(b.v[1]), "v"(b.v[2]), "v"(b.v[3]), "v"(b.v[4]), "v"(b.v[5]), "v"(b.v[6]), "v"(b.v[7])
      : "vcc");
  // r += p & mask  (mask = all ones iff a < b)
  asm("v_and_b32 %8, 1, %16\n\t"
      "v_and_b32 %9, " LCPC_P8_1 ", %16\n\t"
      "v_and_b32 %10, " LCPC_P8_2 ", %16\n\t"
      "v_and_b32 %11, " LCPC_P8_3 ", %16\n\t"
      "v_and_b32 %12, " LCPC_P8_4 ", %16\n\t"
      "v_and_b32 %13, " LCPC_P8_5 ", %16\n\t"
      "v_and_b32 %14, " LCPC_P8_6 ", %16\n\t"
      "v_and_b32 %15, " LCPC_P8_7 ", %16\n\t"
      "v_add_co_u32 %0, vcc, %0, %8\n\t"
      "v_addc_co_u32 %1, vcc, %1, %9, vcc\n\t"
      "v_addc_co_u32 %2, vcc, %2, %10, vcc\n\t"
      "v_addc_co_u32 %3, vcc, %3, %11, vcc\n\t"
      "v_addc_co_u32 %4, vcc, %4, %12, vcc\n\t"
      "v_addc_co_u32 %5, vcc, %5, %13, vcc\n\t"
      "v_addc_co_u32 %6, vcc, %6, %14, vcc\n\t"
      "v_addc_co_u32 %7, vcc, %7, %15, vcc"
      : "+v"(r.v[0]), "+v"(r.v[1]), "+v"(r.v[2]), "+v"(r.v[3]), "+v"(r.v[4]), "+v"(r.v[5]), "+v"(r.v[6]), "+v"(r.v[7]),
        "=&v"(t0), "=&v"(t1), "=&v"(t2), "=&v"(t3), "=&v"(t4), "=&v"(t5), "=&v"(t6), "=&v"(t7)
      : "v"(mask)
      : "vcc");
  return r;
}
// conditional final subtraction: t (NL limbs + top word) in [0, 2p) -> [0, p)
template <int NL> LCPC_DEV Fe<NL> fe_reduce_once(const u32* t, u32 top) {
  Fe<NL> d, r;
  u32 br = 0;
#pragma unroll
  for (int i = 0; i < NL; i++) {
    u64 x = (u64)t[i] - Mod<NL>::P[i] - br;
    d.v[i] = (u32)x;
    br = (u32)(x >> 63);
  }
  const bool ge = (top != 0) | (br == 0);
#pragma unroll
  for (int i = 0; i < NL; i++) r.v[i] = ge ? d.v[i] : t[i];
  return r;
}

// t (NL limbs) in [0, 2p) -> [0, p)
template <int NL> LCPC_DEV Fe<NL> fe_reduce_once(const u32* t) { return fe_reduce_once<NL>(t, 0u); }
// Ft255: the same as one carry chain
template <> LCPC_DEV Fe<8> fe_reduce_once<8>(const u32* t) {
  Fe<8> r;
#pragma unroll
  for (int i = 0; i < 8; i++) r.v[i] = t[i];
  u32 d0, d1, d2, d3, d4, d5, d6, d7;
  asm("v_subrev_co_u32 %8, vcc, 1, %0\n\t"
      "v_subbrev_co_u32 %9, vcc, %16, %1, vcc\n\t"
      "v_subbrev_co_u32 %10, vcc, %17, %2, vcc\n\t"
      "v_subbrev_co_u32 %11, vcc, %18, %3, vcc\n\t"
      "v_subbrev_co_u32 %12, vcc, %19, %4, vcc\n\t"
      "v_subbrev_co_u32 %13, vcc, %20, %5, vcc\n\t"
      "v_subbrev_co_u32 %14, vcc, %21, %6, vcc\n\t"
      "v_subbrev_co_u32 %15, vcc, %22, %7, vcc\n\t"
      "v_cndmask_b32 %0, %8, %0, vcc\n\t"
      "v_cndmask_b32 %1, %9, %1, vcc\n\t"
      "v_cndmask_b32 %2, %10, %2, vcc\n\t"
      "v_cndmask_b32 %3, %11, %3, vcc\n\t"
      "v_cndmask_b32 %4, %12, %4, vcc\n\t"
      "v_cndmask_b32 %5, %13, %5, vcc\n\t"
      "v_cndmask_b32 %6, %14, %6, vcc\n\t"
      "v_cndmask_b32 %7, %15, %7, vcc"
      : "+v"(r.v[0]), "+v"(r.v[1]), "+v"(r.v[2]), "+v"(r.v[3]), "+v"(r.v[4]), "+v"(r.v[5]), "+v"(r.v[6]), "+v"(r.v[7]),
        "=&v"(d0), "=&v"(d1), "=&v"(d2), "=&v"(d3), "=&v"(d4), "=&v"(d5), "=&v"(d6), "=&v"(d7)
      : "v"(Mod<8>::P[1]), "v"(Mod<8>::P[2]), "v"(Mod<8>::P[3]), "v"(Mod<8>::P[4]), "v"(Mod<8>::P[5]), "v"(Mod<8>::P[6]), "v"(Mod<8>::P[7])
      : "vcc");
  return r;
}

// ---- Montgomery multiplication ----------------------------------------------------------------
// r = a*b*R^-1 mod p, fully reduced.  CIOS over 32-bit limbs, one v_mad_u64_u32 per limb product.
template <int NL> LCPC_DEV Fe<NL> fe_mul(const Fe<NL>& a, const Fe<NL>& b) {
  u32 t[NL + 2];
#pragma unroll
  for (int i = 0; i < NL + 2; i++) t[i] = 0;
#pragma unroll
  for (int i = 0; i < NL; i++) {
    u32 c = 0;
#pragma unroll
    for (int j = 0; j < NL; j++) {
      u64 s = (u64)a.v[i] * b.v[j] + t[j] + c;
      t[j] = (u32)s;
      c = (u32)(s >> 32);
    }
    u64 s = (u64)t[NL] + c;
    t[NL] = (u32)s;
    t[NL + 1] = (u32)(s >> 32);
    const u32 m = 0u - t[0];            // -p^-1 = -1 mod 2^32
    c = (t[0] != 0) ? 1u : 0u;          // carry out of t[0] + m*p[0], p[0] = 1
#pragma unroll
    for (int j = 1; j < NL; j++) {
      s = (u64)m * Mod<NL>::P[j] + t[j] + c;
      t[j - 1] = (u32)s;
      c = (u32)(s >> 32);
    }
    s = (u64)t[NL] + c;
    t[NL - 1] = (u32)s;
    t[NL] = t[NL + 1] + (u32)(s >> 32);
  }
  return fe_reduce_once<NL>(t, t[NL]);
}

// Montgomery reduction of a single element == multiply by 1: Montgomery form -> canonical value.
// This is PrimeField::to_repr (lcpc-2d/src/lib.rs:55-57) before the little-endian byte dump.
template <int NL> LCPC_DEV Fe<NL> fe_canon(const Fe<NL>& a) {
  u32 t[NL + 1];
#pragma unroll
  for (int i = 0; i < NL; i++) t[i] = a.v[i];
  t[NL] = 0;
#pragma unroll
  for (int i = 0; i < NL; i++) {
    const u32 m = 0u - t[0];
    u32 c = (t[0] != 0) ? 1u : 0u;
#pragma unroll
    for (int j = 1; j < NL; j++) {
      u64 s = (u64)m * Mod<NL>::P[j] + t[j] + c;
      t[j - 1] = (u32)s;
      c = (u32)(s >> 32);
    }
    u64 s = (u64)t[NL] + c;
    t[NL - 1] = (u32)s;
    t[NL] = (u32)(s >> 32);
  }
  return fe_reduce_once<NL>(t, t[NL]);
}


// ---- lazy (unreduced) accumulation: sum of products, one Montgomery reduction at the end -------
// Used by collapse_columns and the expander SpMV: acc += a*b as a plain 2NL(+1)-limb integer.
// With <= 2^32 terms of size < p^2 < 2^(64NL-2) the sum fits 2NL+1 limbs.
template <int NL> struct Wide {
  u32 v[2 * NL + 1];
};
template <int NL> LCPC_DEV Wide<NL> wide_zero() {
  Wide<NL> w;
#pragma unroll
  for (int i = 0; i < 2 * NL + 1; i++) w.v[i] = 0;
  return w;
}
template <int NL> LCPC_DEV void wide_mac(Wide<NL>& w, const Fe<NL>& a, const Fe<NL>& b) {
#pragma unroll
  for (int i = 0; i < NL; i++) {
    u32 c = 0;
#pragma unroll
    for (int j = 0; j < NL; j++) {
      u64 s = (u64)a.v[i] * b.v[j] + w.v[i + j] + c;
      w.v[i + j] = (u32)s;
      c = (u32)(s >> 32);
    }
#pragma unroll
    for (int j = i + NL; j < 2 * NL + 1; j++) {
      u64 s = (u64)w.v[j] + c;
      w.v[j] = (u32)s;
      c = (u32)(s >> 32);
    }
  }
}
// w mod p in Montgomery sense: returns w * R^-1 mod p.  The top word (bits >= 64 NL) is folded in
// first by reducing it against R^2-free arithmetic: w = lo + hi*2^(64NL) where lo < 2^(64NL);
// mont_reduce(lo) + hi * (2^(64NL) * R^-1 = 1) ... i.e. result = REDC(lo) + hi (mod p).
template <int NL> LCPC_DEV Fe<NL> wide_reduce(const Wide<NL>& w) {
  u32 t[2 * NL + 1];
#pragma unroll
  for (int i = 0; i < 2 * NL + 1; i++) t[i] = w.v[i];
  // REDC over the low 2NL limbs; carries spill into t[2NL]
#pragma unroll
  for (int i = 0; i < NL; i++) {
    const u32 m = 0u - t[i];
    u32 c = (t[i] != 0) ? 1u : 0u;
#pragma unroll
    for (int j = 1; j < NL; j++) {
      u64 s = (u64)m * Mod<NL>::P[j] + t[i + j] + c;
      t[i + j] = (u32)s;
      c = (u32)(s >> 32);
    }
#pragma unroll
    for (int j = i + NL; j < 2 * NL + 1; j++) {
      u64 s = (u64)t[j] + c;
      t[j] = (u32)s;
      c = (u32)(s >> 32);
    }
  }
  // value = t[NL .. 2NL] (NL+1 limbs), < (sum + m p)/R; bring into [0,p) by repeated subtraction
  // (top word < 2^32 terms / small: loop runs at most a few times per 2^k of terms; bounded below)
  u32 top = t[2 * NL];
  u32 x[NL];
#pragma unroll
  for (int i = 0; i < NL; i++) x[i] = t[NL + i];
  // subtract p while value >= p.  value < n_terms * p, n_terms is small in every caller (<= 2^21);
  // do it bit-serially from a shifted p to stay O(log) : here simple loop on (top:x) >= p.
  for (;;) {
    u32 d[NL];
    u32 br = 0;
#pragma unroll
    for (int i = 0; i < NL; i++) {
      u64 s = (u64)x[i] - Mod<NL>::P[i] - br;
      d[i] = (u32)s;
      br = (u32)(s >> 63);
    }
    if (top == 0 && br) break;
    top -= br;
#pragma unroll
    for (int i = 0; i < NL; i++) x[i] = d[i];
  }
  Fe<NL> r;
#pragma unroll
  for (int i = 0; i < NL; i++) r.v[i] = x[i];
  return r;
}

}  // namespace lcpc

// lcpc_amd/csrc/ntt_ln_dev.h -- what the lazy-limb row NTTs share: the pass shape of the two-pass kernels (K1s, ntt_l9s.hip; K1n,
// ntt_lns.hip), the layout of an LDS tile in the multiplier's own format (field_ln.h: N signed limbs of W bits; also the general Ft255
// kernel ntt_pass_l9_kernel, kernels.hip), and the layout of the twiddle packs that ntt_lns.hip builds for both pass kernels.
#pragma once
#include "field_ln.h"

namespace lcpc {

// round structure of a pass with S stages on tiles of 2^S x 2^LBT slots: an odd S peels stage 0 as a radix-2 round
// (slot 0 of the pack), the radix-4 rounds r = 0, 1, .. then cover stages (U0 + 2r, U0 + 2r + 1)
template <int S, int LBT> struct Shape {
  static constexpr int U0 = S & 1;
  static constexpr int NR4 = S / 2;
  static constexpr u32 period2 = 1u << (S - 1 + LBT);                     // radix-2 round: all 512 pairs differ
  static constexpr u32 period4(int r) { return 1u << (S - U0 - 2 * r - 2 + LBT); }
  // the radix-4 round whose twiddle period is 4 (quads q and q + 4 share their twiddles): with the lanes dealt so that wave w holds
  // the quads q = w mod 4, every lane of a wave multiplies by the SAME three twiddles -- the shifted-multiples multiply with scalar
  // operands (ln::mul_u; Ft255: 119 instructions against 188).  The same deal serves periods 2 and 1.  S + LBT == 10: the period
  // is 2^(8 - U0 - 2 r), i.e. <= 4 from round 3 on: RU = 3 where the pass has four radix-4 rounds (S >= 8), -1: none.  NRU: how
  // many rounds from RU on (a last pass ends with the trivial stages k-2, k-1, which have their own form).
  static constexpr int RU = NR4 >= 4 ? 3 : -1;
  static constexpr int NRU = RU < 0 ? 0 : NR4 - RU;
};
// ---- K1s, the Ft255 two-pass plans in the pure / coset form (ntt_l9s.hip, head comment).  The first pass is a plain 2^S-point DIF on
//      every column of its tile: the twiddles of a round depend on the sub-block position only, sets(r) distinct triples in radix-4 round
//      r -- 4^k down to 1.  The round with 4 sets is wave-uniform (RU; only where a lane-varying radix-4 round precedes it, which is where
//      block 0 gets converted: RC), the round with 1 set multiplies by I alone.  RC: the last round that reads its twiddles from the
//      pack; with canonical output it converts its pure sum c0 as well, so that nothing is left in Montgomery form after it.  RC < 0
//      (S <= 3): the radix-2 round (S = 1, 3) or the I-only round (S = 2) converts every output instead.
template <int S> struct PureShape {
  static constexpr int U0 = S & 1;
  static constexpr int NR4 = S / 2;
  static constexpr u32 sets(int r) { return 1u << (S - U0 - 2 * r - 2); }
  static constexpr int RU = NR4 >= 3 ? NR4 - 2 : -1;
  static constexpr int RC = NR4 >= 3 ? NR4 - 3 : (NR4 == 2 ? 0 : -1);
};
// the last pass, coset form: five multiply-then-butterfly radix-4 rounds on a 1024-element tile; round r (stages 2r, 2r + 1) has
// 4^r sub-blocks of 4^(5 - r) elements and one twiddle triple per sub-block.  Rounds 0 and 1 take theirs as shifted multiples (one per
// tile, one per wave), rounds 2 .. 4 from the pack: [tile class][round][3 variants w, w^2, w^3][sub-block]
constexpr u32 coset_sets(int r) { return 1u << (2 * r); }

// words per shifted-multiples table in the packs: N^2 = 25 / 49 / 81 used of 32 / 64 / 96
template <class FT> constexpr u32 U_SLOT = (FT::N * FT::N + 31) & ~31u;
// word alignment of a pack's shifted-multiples tables (NttPackInfo.u_off): 64 bytes; Ft255's have always followed the last round's
// block at its 16-byte alignment
template <class FT> constexpr u32 U_ALIGN = FT::N == 9 ? 4u : 16u;

// ---- global addresses of a K1s pass: a wave-uniform 64-bit base held in scalar registers plus an UNSIGNED 32-bit byte offset per
//      lane -- the saddr + voffset form of global_load / global_store, so that no address costs a 64-bit vector shift or carry add
//      (VOP3, 4.3 cycles each).  ubase(): p is uniform by construction (kernel arguments, blockIdx, compile-time constants); the
//      readfirstlane pair says so and keeps the compiler from folding the uniform part back into a shared per-lane 64-bit sum.
//      lane_at(): the caller states the largest offset it forms.  Everything row-, tile- or class-sized stays on the 64-bit side: a
//      commitment matrix exceeds 4 GiB at the headline (2^18 columns x 512 rows x 32 B).
template <class T> LCPC_DEV T* ubase(T* p) {
  const u64 v = reinterpret_cast<u64>(p);
  const u32 lo = __builtin_amdgcn_readfirstlane((u32)v), hi = __builtin_amdgcn_readfirstlane((u32)(v >> 32));
  // (rebuilt from integers, the pointer would be a generic one -- flat instructions, which have no scalar base: it names global memory)
  typedef __attribute__((address_space(1))) T* GP;
  return (T*)(GP)(((u64)hi << 32) | lo);
}
LCPC_DEV const u32* lane_at(const u32* base, u32 byte_off) { return reinterpret_cast<const u32*>(reinterpret_cast<const char*>(base) + byte_off); }
LCPC_DEV u32* lane_at(u32* base, u32 byte_off) { return reinterpret_cast<u32*>(reinterpret_cast<char*>(base) + byte_off); }

// ---- an array of `cnt` elements in planes: limbs 0-3 as uint4 (N >= 5), then a uint2 plane (N = 3: limbs 0-1; N = 7: limbs 4-5)
//      or a second uint4 plane (N = 9: limbs 4-7), then the top limb as u32.  The LDS tile (cnt = the tile size: unit-stride
//      lanes are conflict-free in every plane; the q*p table follows it) and K1n's twiddle packs (cnt = variants x period).  cnt: a
//      u32, or a std::integral_constant where the caller's count is a compile-time constant that the address arithmetic should see
//      as one from the start (the general kernel's 2^LT-slot tile, kernels.hip) ------------------------------------------------------
template <class FT, class C = u32> LCPC_DEV LN<FT::N> planes_get(const u32* base, C cnt, u32 e) {
  constexpr int N = FT::N;
  LN<N> r;
  if constexpr (N == 3) {
    const uint2 a = *reinterpret_cast<const uint2*>(base + (size_t)e * 2);
    r.v[0] = a.x; r.v[1] = a.y; r.v[2] = base[(size_t)cnt * 2 + e];
  } else {
    const uint4 a = *reinterpret_cast<const uint4*>(base + (size_t)e * 4);
    r.v[0] = a.x; r.v[1] = a.y; r.v[2] = a.z; r.v[3] = a.w;
    if constexpr (N == 5) {
      r.v[4] = base[(size_t)cnt * 4 + e];
    } else if constexpr (N == 7) {
      const uint2 b = *reinterpret_cast<const uint2*>(base + (size_t)cnt * 4 + (size_t)e * 2);
      r.v[4] = b.x; r.v[5] = b.y; r.v[6] = base[(size_t)cnt * 6 + e];
    } else {
      const uint4 b = *reinterpret_cast<const uint4*>(base + ((size_t)cnt + e) * 4);
      r.v[4] = b.x; r.v[5] = b.y; r.v[6] = b.z; r.v[7] = b.w; r.v[8] = base[(size_t)cnt * 8 + e];
    }
  }
  return r;
}
template <class FT, class C = u32> LCPC_DEV void planes_put(u32* base, C cnt, u32 e, const LN<FT::N>& x) {
  constexpr int N = FT::N;
  if constexpr (N == 3) {
    *reinterpret_cast<uint2*>(base + (size_t)e * 2) = make_uint2(x.v[0], x.v[1]);
    base[(size_t)cnt * 2 + e] = x.v[2];
  } else {
    *reinterpret_cast<uint4*>(base + (size_t)e * 4) = make_uint4(x.v[0], x.v[1], x.v[2], x.v[3]);
    if constexpr (N == 5) {
      base[(size_t)cnt * 4 + e] = x.v[4];
    } else if constexpr (N == 7) {
      *reinterpret_cast<uint2*>(base + (size_t)cnt * 4 + (size_t)e * 2) = make_uint2(x.v[4], x.v[5]);
      base[(size_t)cnt * 6 + e] = x.v[6];
    } else {
      *reinterpret_cast<uint4*>(base + ((size_t)cnt + e) * 4) = make_uint4(x.v[4], x.v[5], x.v[6], x.v[7]);
      base[(size_t)cnt * 8 + e] = x.v[8];
    }
  }
}

// ---- an element leaves its tile from the registers (K1s: the pure first pass's I-only round, both last passes' final rounds): clamped
//      straight from the butterfly's sums -- ln::clamp_apply IS the carry pass, so nothing normalises in front of it; x is of one of the
//      two input classes field_ln.h names there -- to [0, p + 64 B) < 2^(32 NL), packed and stored.  REDUCE (a last pass): -> [0, p).
//      After the clamp, value >= p needs the top limb to reach floor(p / B) -- Ft255: about one element in 2^17; the conditional
//      subtract runs only in the waves that hold such an element.  nqp: the NEGATED q*p rows in LDS, visible to the wave (a barrier
//      has run since the kernel copied them)
template <class FT, bool REDUCE> LCPC_DEV void clamp_store(u32* dst, LN<FT::N> x, const u32* nqp) {
  constexpr int N = FT::N, NL = FT::NL;
  ln::clamp_apply<FT>(x, ln::clamp_row<FT>(nqp, ln::clamp_q<FT>(x.v[N - 1])));
  u32 w[NL];
  ln::to_packed<FT>(w, x.v);
  Fe<NL> v;
#pragma unroll
  for (int i = 0; i < NL; i++) v.v[i] = w[i];
  if constexpr (REDUCE) {
    if (__any((int)(x.v[N - 1] >= FT::limb(N - 1)))) v = fe_reduce_once<NL>(w);
  }
  fe_store<NL>(dst, v);
}

// one entry of a limb-form table (twiddles w^i R' mod p, STRIDE words per entry).  Ft255's 12-word entries are 16-byte aligned:
// two uint4 loads and a word
template <class FT> LCPC_DEV LN<FT::N> tab_entry(const u32* tab, u32 idx) {
  if constexpr (FT::STRIDE == 12) {
    return ln::load_limbs<FT::N>(tab + (size_t)idx * 12);
  } else {
    LN<FT::N> t;
#pragma unroll
    for (int k = 0; k < FT::N; k++) t.v[k] = tab[(size_t)idx * FT::STRIDE + k];
    return t;
  }
}

// ---- the twiddle pack of one (class, round): NV variants of `period` twiddles each, in lane order (ntt_lns.hip builds it, the pass
//      kernels read it).  N = 9: [NV][2 planes of 16 B][period] uint4, then [NV][period] u32 (the top limb), read with 32-bit byte
//      offsets from the (wave-uniform) block pointer: scalar base + vector offset addressing, no 64-bit VALU adds (a class block is
//      < 2^20 words).  N = 3, 5, 7: planes over all NV x period entries (planes_get) ------------------------------------------------
template <class FT, u32 NV> LCPC_DEV LN<FT::N> pack_get(const u32* blk, u32 period, u32 variant, u32 jl) {
  if constexpr (FT::N == 9) {
    const char* base = reinterpret_cast<const char*>(blk);
    const uint4 a = *reinterpret_cast<const uint4*>(base + (((variant * 2 + 0) * period + jl) << 4));
    const uint4 b = *reinterpret_cast<const uint4*>(base + (((variant * 2 + 1) * period + jl) << 4));
    const u32 c = *reinterpret_cast<const u32*>(base + ((NV * 2 * period * 4 + variant * period + jl) << 2));
    LN<9> t;
    t.v[0] = a.x; t.v[1] = a.y; t.v[2] = a.z; t.v[3] = a.w; t.v[4] = b.x; t.v[5] = b.y; t.v[6] = b.z; t.v[7] = b.w; t.v[8] = c;
    return t;
  } else {
    return planes_get<FT>(blk, NV * period, variant * period + jl);
  }
}
// the same entry for the K1s pass kernels, whose block pointer and period are wave-uniform by construction (class = the workgroup's
// tile or none, round and period compile-time): entry (uv + lv) with uv the wave-uniform part of the variant (which twiddle of the
// triple, which table of an ln::mul2 pair) and lv the part that may differ by lane (plain or converting set).  Each of the three loads
// takes a scalar base of its own (ubase) and the lanes add (2 lv period + jl) * 16 resp. (lv period + jl) * 4 bytes: lv < 6 and
// jl < period <= 512, so a lane offset stays below 104 KiB -- 32 bits whatever the plan, since a class block does not grow with the
// transform (<= 2^20 columns in two passes, <= 2^26 in three: the same rounds, the same periods).
// == pack_get<FT, NV>(blk, period, uv + lv, jl), which serves a block pointer of any kind (tests/native/k1_harness.cpp)
template <u32 NV> LCPC_DEV LN<9> pack_get_u(const u32* blk, u32 period, u32 uv, u32 lv, u32 jl) {
  const u32 o16 = (lv * 2 * period + jl) << 4, o4 = (lv * period + jl) << 2;
  const uint4 a = *reinterpret_cast<const uint4*>(lane_at(ubase(blk + (size_t)(uv * 2 + 0) * period * 4), o16));
  const uint4 b = *reinterpret_cast<const uint4*>(lane_at(ubase(blk + (size_t)(uv * 2 + 1) * period * 4), o16));
  const u32 c = *lane_at(ubase(blk + (size_t)NV * 2 * period * 4 + (size_t)uv * period), o4);
  LN<9> t;
  t.v[0] = a.x; t.v[1] = a.y; t.v[2] = a.z; t.v[3] = a.w; t.v[4] = b.x; t.v[5] = b.y; t.v[6] = b.z; t.v[7] = b.w; t.v[8] = c;
  return t;
}
template <class FT, u32 NV> LCPC_DEV void pack_put(u32* blk, u32 period, u32 variant, u32 jl, const LN<FT::N>& x) {
  if constexpr (FT::N == 9) {
    *reinterpret_cast<uint4*>(blk + ((size_t)(variant * 2 + 0) * period + jl) * 4) = make_uint4(x.v[0], x.v[1], x.v[2], x.v[3]);
    *reinterpret_cast<uint4*>(blk + ((size_t)(variant * 2 + 1) * period + jl) * 4) = make_uint4(x.v[4], x.v[5], x.v[6], x.v[7]);
    blk[(size_t)NV * 2 * period * 4 + (size_t)variant * period + jl] = x.v[8];
  } else {
    planes_put<FT>(blk, NV * period, variant * period + jl, x);
  }
}

}  // namespace lcpc

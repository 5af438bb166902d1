// lcpc_amd/csrc/keccak_dev.h -- Keccak-f[1600] for gfx950, one sponge per lane (SHA3-256, FIPS 202; Keccak-256).
//
// The digest D of LcCommit<D, E> (lcpc-2d/src/lib.rs:172-184) when the encoder is built with LCPC_HASH_SHA3_256:
// leaf = SHA3-256(0^32 || to_repr(col[0]) || ...) (lib.rs:719-735), parent = SHA3-256(left || right) (lib.rs:770-775).
//
// The 25 lanes are 50 VGPRs (two 32-bit halves each).  A round is ~180 VALU instructions:
//  - theta: the five column parities are two 3-input XORs per half (v_bitop3_b32 0x96; gfx950 has no v_xor3_b32), and
//    a[x][y] ^= C[x-1] ^ rotl(C[x+1], 1) is one more per half;
//  - rho: a 64-bit rotate is two v_alignbit_b32 (by 32: a register rename);
//  - chi: a ^ (~b & c) is one v_bitop3_b32 0xD2 per half (clang emits v_bfi_b32 + v_xor_b32 for the plain expression).
// Truth tables use the usual operand constants src0 = 0xF0, src1 = 0xCC, src2 = 0xAA.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace lcpc {
namespace kc {

struct Lane { uint32_t lo, hi; };

// the byte that opens pad10*1 (the domain bits and the first padding bit): SHA3-256 (FIPS 202), and Keccak-256, the pre-FIPS
// padding of LCPC_HASH_KECCAK256 -- the same sponge otherwise (rate 136, 32-byte output)
constexpr uint32_t KC_DOM_SHA3 = 0x06u, KC_DOM_KECCAK = 0x01u;

__device__ __forceinline__ uint32_t xor3(uint32_t a, uint32_t b, uint32_t c) {
  uint32_t r;
  asm("v_bitop3_b32 %0, %1, %2, %3 bitop3:0x96" : "=v"(r) : "v"(a), "v"(b), "v"(c));
  return r;
}
// a ^ (~b & c)
__device__ __forceinline__ uint32_t chi3(uint32_t a, uint32_t b, uint32_t c) {
  uint32_t r;
  asm("v_bitop3_b32 %0, %1, %2, %3 bitop3:0xD2" : "=v"(r) : "v"(a), "v"(b), "v"(c));
  return r;
}
__device__ __forceinline__ Lane xor3(Lane a, Lane b, Lane c) { return {xor3(a.lo, b.lo, c.lo), xor3(a.hi, b.hi, c.hi)}; }
__device__ __forceinline__ Lane chi3(Lane a, Lane b, Lane c) { return {chi3(a.lo, b.lo, c.lo), chi3(a.hi, b.hi, c.hi)}; }

template <int N> __device__ __forceinline__ Lane rotl(Lane x) {
  constexpr int n = N & 63;
  if constexpr (n == 0) return x;
  else if constexpr (n == 32) return {x.hi, x.lo};
  else if constexpr (n < 32) return {__builtin_amdgcn_alignbit(x.lo, x.hi, 32 - n), __builtin_amdgcn_alignbit(x.hi, x.lo, 32 - n)};
  else return {__builtin_amdgcn_alignbit(x.hi, x.lo, 64 - n), __builtin_amdgcn_alignbit(x.lo, x.hi, 64 - n)};
}

__constant__ static const uint32_t KC_RC[48] = {
    0x00000001u, 0x00000000u, 0x00008082u, 0x00000000u, 0x0000808Au, 0x80000000u, 0x80008000u, 0x80000000u,
    0x0000808Bu, 0x00000000u, 0x80000001u, 0x00000000u, 0x80008081u, 0x80000000u, 0x00008009u, 0x80000000u,
    0x0000008Au, 0x00000000u, 0x00000088u, 0x00000000u, 0x80008009u, 0x00000000u, 0x8000000Au, 0x00000000u,
    0x8000808Bu, 0x00000000u, 0x0000008Bu, 0x80000000u, 0x00008089u, 0x80000000u, 0x00008003u, 0x80000000u,
    0x00008002u, 0x80000000u, 0x00000080u, 0x80000000u, 0x0000800Au, 0x00000000u, 0x8000000Au, 0x80000000u,
    0x80008081u, 0x80000000u, 0x00008080u, 0x80000000u, 0x80000001u, 0x00000000u, 0x80008008u, 0x80000000u};

// lane (x, y) at a[x + 5 y]
__device__ __forceinline__ void keccak_f(Lane a[25]) {
  for (int r = 0; r < 24; r++) {
    Lane c[5], d[5];
#pragma unroll
    for (int x = 0; x < 5; x++) c[x] = xor3(xor3(a[x], a[x + 5], a[x + 10]), a[x + 15], a[x + 20]);
#pragma unroll
    for (int x = 0; x < 5; x++) d[x] = rotl<1>(c[(x + 1) % 5]);
#pragma unroll
    for (int y = 0; y < 25; y += 5)
#pragma unroll
      for (int x = 0; x < 5; x++) a[y + x] = xor3(a[y + x], c[(x + 4) % 5], d[x]);
    // rho + pi: b[y, 2x + 3y] = rotl(a[x, y], r[x, y])
    Lane b[25];
    b[0] = a[0];
    b[10] = rotl<1>(a[1]);  b[20] = rotl<62>(a[2]); b[5] = rotl<28>(a[3]);  b[15] = rotl<27>(a[4]);
    b[16] = rotl<36>(a[5]); b[1] = rotl<44>(a[6]);  b[11] = rotl<6>(a[7]);  b[21] = rotl<55>(a[8]); b[6] = rotl<20>(a[9]);
    b[7] = rotl<3>(a[10]);  b[17] = rotl<10>(a[11]); b[2] = rotl<43>(a[12]); b[12] = rotl<25>(a[13]); b[22] = rotl<39>(a[14]);
    b[23] = rotl<41>(a[15]); b[8] = rotl<45>(a[16]); b[18] = rotl<15>(a[17]); b[3] = rotl<21>(a[18]); b[13] = rotl<8>(a[19]);
    b[14] = rotl<18>(a[20]); b[24] = rotl<2>(a[21]); b[9] = rotl<61>(a[22]); b[19] = rotl<56>(a[23]); b[4] = rotl<14>(a[24]);
#pragma unroll
    for (int y = 0; y < 25; y += 5)
#pragma unroll
      for (int x = 0; x < 5; x++) a[y + x] = chi3(b[y + x], b[y + (x + 1) % 5], b[y + (x + 2) % 5]);
    a[0].lo ^= KC_RC[2 * r];
    a[0].hi ^= KC_RC[2 * r + 1];
  }
}

}  // namespace kc

// the chain traits (chain_dev.h) of the two sponges: rate 17 lanes, every message word one lane, 32-byte output.  DOM = KC_DOM_SHA3 /
// KC_DOM_KECCAK
template <uint32_t DOM> struct KeccakChain {
  static constexpr int PREFIX = 4, BLOCK = 17, DIGEST_WORDS = 8, STATE_WORDS = 50, N_ELEMS = 25;
  using Elem = kc::Lane;
  using Word = uint2;          // one lane: the state pointer must be 8-byte aligned
  struct Msg {};               // a sponge absorbs into its state
  static constexpr uint64_t n_blocks(uint64_t n_words) { return n_words / 17 + 1; }   // the padding always fits: a message of 17 k words takes a block of its own
  static constexpr int batch_waves(int, bool) { return 0; }
  static __device__ __forceinline__ Word word(Elem e) { return make_uint2(e.lo, e.hi); }
  static __device__ __forceinline__ Elem elem(Word w) { return {w.x, w.y}; }
  static __device__ __forceinline__ void init(Elem s[25]) {
#pragma unroll
    for (int i = 0; i < 25; i++) s[i] = {0u, 0u};
  }
  static __device__ __forceinline__ void absorb(Elem s[25], Msg&, int p, uint32_t lo, uint32_t hi) { s[p].lo ^= lo; s[p].hi ^= hi; }
  static __device__ __forceinline__ void finish_block(Elem s[25], Msg&, uint64_t blk, uint64_t n_words, uint64_t) {
    if (17 * blk + 17 > n_words) {
      // the block that holds the end of the message: pad10*1 behind the domain bits (DOM ... 0x80); the message is whole words, so the
      // DOM byte starts lane n_words - 17 blk.  The byte comes from a scalar register the compiler cannot see through, so that it does not
      // turn `? 1 : 0` (Keccak-256) into a per-lane boolean and allocate the whole kernel differently from the SHA3-256 instantiation
      const uint32_t q = (uint32_t)(n_words - 17 * blk);
      uint32_t dom = DOM;
      asm volatile("" : "+s"(dom));
#pragma unroll
      for (uint32_t p = 0; p < 17; p++) s[p].lo ^= (p == q) ? dom : 0u;
      s[16].hi ^= 0x80000000u;
    }
    kc::keccak_f(s);
  }
  static __device__ __forceinline__ void store_digest(uint32_t* o, const Elem s[25]) {
    *reinterpret_cast<uint4*>(o) = make_uint4(s[0].lo, s[0].hi, s[1].lo, s[1].hi);
    *reinterpret_cast<uint4*>(o + 4) = make_uint4(s[2].lo, s[2].hi, s[3].lo, s[3].hi);
  }
  // parent = D(left || right): 8 words, one permutation
  static __device__ __forceinline__ void node(uint32_t o[8], const uint32_t* l, const uint32_t* r) {
    Elem s[25];
    init(s);
#pragma unroll
    for (int i = 0; i < 4; i++) { s[i] = {l[2 * i], l[2 * i + 1]}; s[4 + i] = {r[2 * i], r[2 * i + 1]}; }
    s[8].lo = DOM;
    s[16].hi = 0x80000000u;
    kc::keccak_f(s);
#pragma unroll
    for (int i = 0; i < 4; i++) { o[2 * i] = s[i].lo; o[2 * i + 1] = s[i].hi; }
  }
};

}  // namespace lcpc

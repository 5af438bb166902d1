// lcpc_amd/csrc/sha256_dev.h -- the SHA-256 compression (FIPS 180-4) for gfx950, one hash chain per lane.
//
// The digest D of LcCommit<D, E> (lcpc-2d/src/lib.rs:172-184) when the encoder is built with LCPC_HASH_SHA256:
// leaf = SHA-256(0^32 || to_repr(col[0]) || ...) (lib.rs:719-735), parent = SHA-256(left || right) (lib.rs:770-775).
//
// State (8 words) and a rolling 16-word schedule live in registers.  A round is:
//  - Sigma0 / Sigma1: three rotates (v_alignbit_b32 with both sources the same register) and one 3-input XOR
//    (v_bitop3_b32 0x96; gfx950 has no v_xor3_b32);
//  - Ch(e, f, g) = (e & f) | (~e & g): one v_bfi_b32;  Maj(a, b, c) = bfi(a ^ b, c, b): one v_xor_b32 and one v_bfi_b32;
//  - the sums: v_add3_u32 where the compiler pairs them.
// Rounds 16..63 also extend the schedule: sigma0 / sigma1 are two rotates, one shift and one 3-input XOR each.
// The 64 rounds run as four passes of one 16-round body (the schedule index is static inside it), so a kernel that inlines the
// compression once per block of its group (sha256.hip) stays well inside the instruction cache.
// Truth tables use the usual operand constants src0 = 0xF0, src1 = 0xCC, src2 = 0xAA.
//
// SHA-256 reads its message as big-endian 32-bit words; the commitment's words are little-endian limbs, so every message word
// is byte-swapped on the way in (bswap: one v_perm_b32) and every digest word on the way out.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace lcpc {
namespace s256 {

#define LCPC_SHA256_K                                                                                                               \
  0x428a2f98u, 0x71374491u, 0xb5c0fbcfu, 0xe9b5dba5u, 0x3956c25bu, 0x59f111f1u, 0x923f82a4u, 0xab1c5ed5u, 0xd807aa98u, 0x12835b01u, \
  0x243185beu, 0x550c7dc3u, 0x72be5d74u, 0x80deb1feu, 0x9bdc06a7u, 0xc19bf174u, 0xe49b69c1u, 0xefbe4786u, 0x0fc19dc6u, 0x240ca1ccu, \
  0x2de92c6fu, 0x4a7484aau, 0x5cb0a9dcu, 0x76f988dau, 0x983e5152u, 0xa831c66du, 0xb00327c8u, 0xbf597fc7u, 0xc6e00bf3u, 0xd5a79147u, \
  0x06ca6351u, 0x14292967u, 0x27b70a85u, 0x2e1b2138u, 0x4d2c6dfcu, 0x53380d13u, 0x650a7354u, 0x766a0abbu, 0x81c2c92eu, 0x92722c85u, \
  0xa2bfe8a1u, 0xa81a664bu, 0xc24b8b70u, 0xc76c51a3u, 0xd192e819u, 0xd6990624u, 0xf40e3585u, 0x106aa070u, 0x19a4c116u, 0x1e376c08u, \
  0x2748774cu, 0x34b0bcb5u, 0x391c0cb3u, 0x4ed8aa4au, 0x5b9cca4fu, 0x682e6ff3u, 0x748f82eeu, 0x78a5636fu, 0x84c87814u, 0x8cc70208u, \
  0x90befffau, 0xa4506cebu, 0xbef9a3f7u, 0xc67178f2u

__constant__ static const uint32_t K[64] = {LCPC_SHA256_K};

// K[t] + W[t] of the second block of a 64-byte message (0x80, zeros, bit length 512): the same for every tree node, so its
// schedule is worked out at compile time
struct PadSchedule {
  uint32_t kw[64];
  constexpr PadSchedule() : kw{} {
    constexpr uint32_t k[64] = {LCPC_SHA256_K};
    uint32_t w[64] = {};
    w[0] = 0x80000000u;
    w[15] = 512u;
    for (int t = 16; t < 64; t++) {
      const uint32_t a = w[t - 15], b = w[t - 2];
      const uint32_t s0 = ((a >> 7) | (a << 25)) ^ ((a >> 18) | (a << 14)) ^ (a >> 3);
      const uint32_t s1 = ((b >> 17) | (b << 15)) ^ ((b >> 19) | (b << 13)) ^ (b >> 10);
      w[t] = w[t - 16] + s0 + w[t - 7] + s1;
    }
    for (int t = 0; t < 64; t++) kw[t] = k[t] + w[t];
  }
};
__constant__ static const PadSchedule PAD64{};
#undef LCPC_SHA256_K

__device__ __forceinline__ uint32_t xor3(uint32_t a, uint32_t b, uint32_t c) {
  uint32_t r;
  asm("v_bitop3_b32 %0, %1, %2, %3 bitop3:0x96" : "=v"(r) : "v"(a), "v"(b), "v"(c));
  return r;
}
// (s & x) | (~s & y)
__device__ __forceinline__ uint32_t bfi(uint32_t s, uint32_t x, uint32_t y) {
  uint32_t r;
  asm("v_bfi_b32 %0, %1, %2, %3" : "=v"(r) : "v"(s), "v"(x), "v"(y));
  return r;
}
template <int N> __device__ __forceinline__ uint32_t rotr(uint32_t x) { return __builtin_amdgcn_alignbit(x, x, N); }
__device__ __forceinline__ uint32_t bswap(uint32_t x) { return __builtin_bswap32(x); }

__device__ __forceinline__ uint32_t big_sigma0(uint32_t x) { return xor3(rotr<2>(x), rotr<13>(x), rotr<22>(x)); }
__device__ __forceinline__ uint32_t big_sigma1(uint32_t x) { return xor3(rotr<6>(x), rotr<11>(x), rotr<25>(x)); }
__device__ __forceinline__ uint32_t sigma0(uint32_t x) { return xor3(rotr<7>(x), rotr<18>(x), x >> 3); }
__device__ __forceinline__ uint32_t sigma1(uint32_t x) { return xor3(rotr<17>(x), rotr<19>(x), x >> 10); }

__device__ __forceinline__ void init(uint32_t h[8]) {
  h[0] = 0x6a09e667u; h[1] = 0xbb67ae85u; h[2] = 0x3c6ef372u; h[3] = 0xa54ff53au;
  h[4] = 0x510e527fu; h[5] = 0x9b05688cu; h[6] = 0x1f83d9abu; h[7] = 0x5be0cd19u;
}

// round i of a 16-round pass: the working variables stay where they are and the roles rotate, a = s[(0 - i) & 7], ...; kw is the
// round's constant and schedule word, already summed
template <int I>
__device__ __forceinline__ void round(uint32_t s[8], uint32_t kw) {
  constexpr int A = (0 - I) & 7, B = (1 - I) & 7, C = (2 - I) & 7, D = (3 - I) & 7, E = (4 - I) & 7, F = (5 - I) & 7, G = (6 - I) & 7,
                H = (7 - I) & 7;
  const uint32_t t1 = s[H] + big_sigma1(s[E]) + bfi(s[E], s[F], s[G]) + kw;
  const uint32_t t2 = big_sigma0(s[A]) + bfi(s[A] ^ s[B], s[C], s[B]);
  s[D] += t1;
  s[H] = t1 + t2;
}

template <int I>
__device__ __forceinline__ void rounds16(uint32_t s[8], uint32_t w[16], const uint32_t* k, bool extend) {
  if constexpr (I < 16) {
    if (extend) w[I] += sigma0(w[(I + 1) & 15]) + w[(I + 9) & 15] + sigma1(w[(I + 14) & 15]);
    round<I>(s, k[I] + w[I]);
    rounds16<I + 1>(s, w, k, extend);
  }
}

// h <- compress(h, w): w[0..15] the block's big-endian words (clobbered: the rolling schedule)
__device__ __forceinline__ void compress(uint32_t h[8], uint32_t w[16]) {
  uint32_t s[8];
#pragma unroll
  for (int i = 0; i < 8; i++) s[i] = h[i];
  rounds16<0>(s, w, K, false);
#pragma unroll 1
  for (int t = 16; t < 64; t += 16) rounds16<0>(s, w, K + t, true);
#pragma unroll
  for (int i = 0; i < 8; i++) h[i] += s[i];
}

template <int I>
__device__ __forceinline__ void pad_rounds16(uint32_t s[8], const uint32_t* kw) {
  if constexpr (I < 16) {
    round<I>(s, kw[I]);
    pad_rounds16<I + 1>(s, kw);
  }
}

// h <- compress(h, the padding block of a 64-byte message): no schedule arithmetic
__device__ __forceinline__ void compress_pad64(uint32_t h[8]) {
  uint32_t s[8];
#pragma unroll
  for (int i = 0; i < 8; i++) s[i] = h[i];
#pragma unroll 1
  for (int t = 0; t < 64; t += 16) pad_rounds16<0>(s, PAD64.kw + t);
#pragma unroll
  for (int i = 0; i < 8; i++) h[i] += s[i];
}

}  // namespace s256

// the chain traits (chain_dev.h): a 64-byte block is 8 message words; word p goes into words 2 p, 2 p + 1 of the block, each half
// byte-swapped.  Padding: the byte 0x80, zeros, the bit length as a big-endian 64-bit word at the end of a block.  With q = n_words mod 8
// words in the block that holds the end of the message, 0x80 opens word q and the length is word 7 of the same block -- except q = 7,
// where the length takes one more block; q = 0 is a block of padding alone.
struct Sha256Chain {
  static constexpr int PREFIX = 4, BLOCK = 8, DIGEST_WORDS = 8, STATE_WORDS = 8, N_ELEMS = 8;
  using Elem = uint32_t;       // the working h[], not byte-swapped
  using Word = uint32_t;
  struct Msg { uint32_t w[16]; };
  static constexpr uint64_t n_blocks(uint64_t n_words) { return n_words / 8 + 1 + ((n_words & 7) == 7 ? 1 : 0); }   // 0x80 and the length need two words
  // the batch leaf kernel's second launch bound is the one-shot twin's occupancy in waves per SIMD: without it the register allocator
  // spreads the same instruction stream over twice the VGPRs
  static constexpr int batch_waves(int nl, bool canon) { return (nl == 6 && !canon) ? 7 : 8; }
  static __device__ __forceinline__ Word word(Elem e) { return e; }
  static __device__ __forceinline__ Elem elem(Word w) { return w; }
  static __device__ __forceinline__ void init(Elem h[8]) { s256::init(h); }
  static __device__ __forceinline__ void absorb(Elem*, Msg& m, int p, uint32_t lo, uint32_t hi) {
    m.w[2 * p] = s256::bswap(lo);
    m.w[2 * p + 1] = s256::bswap(hi);
  }
  static __device__ __forceinline__ void finish_block(Elem h[8], Msg& m, uint64_t blk, uint64_t n_words, uint64_t n_blocks) {
    if (blk == n_words / 8) {
      // the block that holds the end of the message: the message is whole words, so the 0x80 byte is the first byte of word
      // n_words - 8 blk, i.e. the top byte of its first big-endian half (that word is zero so far)
      const uint32_t q = (uint32_t)(n_words - 8 * blk);
#pragma unroll
      for (uint32_t p = 0; p < 8; p++) m.w[2 * p] |= (p == q) ? 0x80000000u : 0u;
    }
    if (blk + 1 == n_blocks) {
      const uint64_t bits = 64 * n_words;
      m.w[14] = (uint32_t)(bits >> 32);
      m.w[15] = (uint32_t)bits;
    }
    s256::compress(h, m.w);
  }
  static __device__ __forceinline__ void store_digest(uint32_t* o, const Elem h[8]) {
    *reinterpret_cast<uint4*>(o) = make_uint4(s256::bswap(h[0]), s256::bswap(h[1]), s256::bswap(h[2]), s256::bswap(h[3]));
    *reinterpret_cast<uint4*>(o + 4) = make_uint4(s256::bswap(h[4]), s256::bswap(h[5]), s256::bswap(h[6]), s256::bswap(h[7]));
  }
  // parent = SHA-256(left || right): 64 message bytes are one block, the padding a second one that is the same for every node
  static __device__ __forceinline__ void node(uint32_t o[8], const uint32_t* l, const uint32_t* r) {
    uint32_t m[16], h[8];
#pragma unroll
    for (int i = 0; i < 8; i++) { m[i] = s256::bswap(l[i]); m[8 + i] = s256::bswap(r[i]); }
    s256::init(h);
    s256::compress(h, m);
    s256::compress_pad64(h);
#pragma unroll
    for (int i = 0; i < 8; i++) o[i] = s256::bswap(h[i]);
  }
};

}  // namespace lcpc

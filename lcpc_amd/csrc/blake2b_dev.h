// lcpc_amd/csrc/blake2b_dev.h -- the BLAKE2b compression (RFC 7693) for gfx950, one hash chain per lane (BLAKE2b-512, unkeyed).
//
// The digest D of LcCommit<D, E> (lcpc-2d/src/lib.rs:172-184) when the encoder is built with LCPC_HASH_BLAKE2B:
// leaf = BLAKE2b(0^64 || to_repr(col[0]) || ...) (lib.rs:719-735), parent = BLAKE2b(left64 || right64) (lib.rs:770-775).
//
// The chaining value (8 words), the work vector (16) and the message block (16) are 64-bit values in VGPR pairs.  The 12 rounds
// are unrolled, so every message index of the schedule is a compile-time register.  Per G: four 64-bit adds (add + add-with-carry,
// or one v_lshl_add_u64), four XORs on both halves and four rotations -- by 32 a register swap, by 24 / 16 / 63 two
// v_alignbit_b32 each.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace lcpc {
namespace b2b {

constexpr uint64_t IV[8] = {0x6a09e667f3bcc908ull, 0xbb67ae8584caa73bull, 0x3c6ef372fe94f82bull, 0xa54ff53a5f1d36f1ull,
                            0x510e527fade682d1ull, 0x9b05688c2b3e6c1full, 0x1f83d9abfb41bd6bull, 0x5be0cd19137e2179ull};
// h[0] of an unkeyed BLAKE2b with a 64-byte digest: IV[0] ^ 0x0101kknn, kk = 0, nn = 64
constexpr uint64_t H0 = IV[0] ^ 0x01010040ull;

constexpr uint8_t SIGMA[10][16] = {
    {0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15}, {14, 10, 4, 8, 9, 15, 13, 6, 1, 12, 0, 2, 11, 7, 5, 3},
    {11, 8, 12, 0, 5, 2, 15, 13, 10, 14, 3, 6, 7, 1, 9, 4}, {7, 9, 3, 1, 13, 12, 11, 14, 2, 6, 5, 10, 4, 0, 15, 8},
    {9, 0, 5, 7, 2, 4, 10, 15, 14, 1, 11, 12, 6, 8, 3, 13}, {2, 12, 6, 10, 0, 11, 8, 3, 4, 13, 7, 5, 15, 14, 1, 9},
    {12, 5, 1, 15, 14, 13, 4, 10, 0, 7, 6, 3, 9, 2, 8, 11}, {13, 11, 7, 14, 12, 1, 3, 9, 5, 0, 15, 4, 8, 6, 2, 10},
    {6, 15, 14, 9, 11, 3, 0, 8, 12, 2, 13, 7, 1, 4, 10, 5}, {10, 2, 8, 4, 7, 6, 1, 5, 15, 11, 9, 14, 3, 12, 13, 0}};

__device__ __forceinline__ uint32_t lo32(uint64_t x) { return (uint32_t)x; }
__device__ __forceinline__ uint32_t hi32(uint64_t x) { return (uint32_t)(x >> 32); }
__device__ __forceinline__ uint64_t pack(uint32_t lo, uint32_t hi) { return ((uint64_t)hi << 32) | lo; }

// rotate right by N, 0 < N < 64, N != 32: two v_alignbit_b32 (alignbit(a, b, s) = low 32 bits of (a:b) >> s)
template <int N> __device__ __forceinline__ uint64_t rotr(uint64_t x) {
  const uint32_t l = lo32(x), h = hi32(x);
  if constexpr (N == 32) return pack(h, l);
  else if constexpr (N < 32) return pack(__builtin_amdgcn_alignbit(h, l, N), __builtin_amdgcn_alignbit(l, h, N));
  else return pack(__builtin_amdgcn_alignbit(l, h, N - 32), __builtin_amdgcn_alignbit(h, l, N - 32));
}

// a + b + c as two 64-bit adds
__device__ __forceinline__ uint64_t add3(uint64_t a, uint64_t b, uint64_t c) { return a + b + c; }

template <int A, int B, int C, int D>
__device__ __forceinline__ void g(uint64_t v[16], uint64_t x, uint64_t y) {
  v[A] = add3(v[A], v[B], x);
  v[D] = rotr<32>(v[D] ^ v[A]);
  v[C] = v[C] + v[D];
  v[B] = rotr<24>(v[B] ^ v[C]);
  v[A] = add3(v[A], v[B], y);
  v[D] = rotr<16>(v[D] ^ v[A]);
  v[C] = v[C] + v[D];
  v[B] = rotr<63>(v[B] ^ v[C]);
}

template <int R>
__device__ __forceinline__ void round(uint64_t v[16], const uint64_t m[16]) {
  constexpr int s = R % 10;
  g<0, 4, 8, 12>(v, m[SIGMA[s][0]], m[SIGMA[s][1]]);
  g<1, 5, 9, 13>(v, m[SIGMA[s][2]], m[SIGMA[s][3]]);
  g<2, 6, 10, 14>(v, m[SIGMA[s][4]], m[SIGMA[s][5]]);
  g<3, 7, 11, 15>(v, m[SIGMA[s][6]], m[SIGMA[s][7]]);
  g<0, 5, 10, 15>(v, m[SIGMA[s][8]], m[SIGMA[s][9]]);
  g<1, 6, 11, 12>(v, m[SIGMA[s][10]], m[SIGMA[s][11]]);
  g<2, 7, 8, 13>(v, m[SIGMA[s][12]], m[SIGMA[s][13]]);
  g<3, 4, 9, 14>(v, m[SIGMA[s][14]], m[SIGMA[s][15]]);
  if constexpr (R + 1 < 12) round<R + 1>(v, m);
}

// F(h, m, t, f): t = bytes hashed so far including this block (< 2^64 here), last = the final block
__device__ __forceinline__ void compress(uint64_t h[8], const uint64_t m[16], uint64_t t, bool last) {
  uint64_t v[16];
#pragma unroll
  for (int i = 0; i < 8; i++) { v[i] = h[i]; v[8 + i] = IV[i]; }
  v[12] ^= t;
  v[14] = last ? ~v[14] : v[14];
  round<0>(v, m);
#pragma unroll
  for (int i = 0; i < 8; i++) h[i] ^= v[i] ^ v[8 + i];
}

__device__ __forceinline__ void init(uint64_t h[8]) {
  h[0] = H0;
#pragma unroll
  for (int i = 1; i < 8; i++) h[i] = IV[i];
}

}  // namespace b2b

// the chain traits (chain_dev.h): Output<Blake2b>::default() is 64 zero bytes, so the prefix is 8 words; every message word is one
// BLAKE2b message word, 16 to a block.  A message that fills its last block exactly gets no extra block: the final compression is the
// full last block with t = the message length and f0 = ~0.  The byte counter of a block that is not the last is 128 (blk + 1), so the
// chaining value is all a later launch needs.  Digests are 64 bytes = 16 u32 words.
struct Blake2bChain {
  static constexpr int PREFIX = 8, BLOCK = 16, DIGEST_WORDS = 16, STATE_WORDS = 16, N_ELEMS = 8;
  using Elem = uint64_t;
  using Word = uint64_t;       // the state pointer must be 8-byte aligned
  struct Msg { uint64_t w[16]; };
  static constexpr uint64_t n_blocks(uint64_t n_words) { return (n_words + 15) / 16; }   // no padding block
  // no occupancy bound on the batch leaf kernel: held to the one-shot twin's 5 / 4 waves per SIMD the register allocator spills 36 .. 116
  // bytes per lane; left alone it takes 116 .. 136 VGPRs -- one wave per SIMD fewer -- and no scratch
  static constexpr int batch_waves(int, bool) { return 0; }
  static __device__ __forceinline__ Word word(Elem e) { return e; }
  static __device__ __forceinline__ Elem elem(Word w) { return w; }
  static __device__ __forceinline__ void init(Elem h[8]) { b2b::init(h); }
  static __device__ __forceinline__ void absorb(Elem*, Msg& m, int p, uint32_t lo, uint32_t hi) { m.w[p] = b2b::pack(lo, hi); }
  static __device__ __forceinline__ void finish_block(Elem h[8], Msg& m, uint64_t blk, uint64_t n_words, uint64_t n_blocks) {
    const bool last = blk + 1 == n_blocks;
    b2b::compress(h, m.w, last ? 8 * n_words : 128 * (blk + 1), last);
  }
  static __device__ __forceinline__ void store_digest(uint32_t* o, const Elem h[8]) {
#pragma unroll
    for (int i = 0; i < 8; i += 2)
      *reinterpret_cast<uint4*>(o + 2 * i) = make_uint4(b2b::lo32(h[i]), b2b::hi32(h[i]), b2b::lo32(h[i + 1]), b2b::hi32(h[i + 1]));
  }
  // parent = BLAKE2b(left || right): 16 words, one compression with t = 128 and the last-block flag
  static __device__ __forceinline__ void node(uint32_t o[16], const uint32_t* l, const uint32_t* r) {
    uint64_t m[16], h[8];
#pragma unroll
    for (int i = 0; i < 8; i++) { m[i] = b2b::pack(l[2 * i], l[2 * i + 1]); m[8 + i] = b2b::pack(r[2 * i], r[2 * i + 1]); }
    b2b::init(h);
    b2b::compress(h, m, 128, true);
#pragma unroll
    for (int i = 0; i < 8; i++) { o[2 * i] = b2b::lo32(h[i]); o[2 * i + 1] = b2b::hi32(h[i]); }
  }
};

}  // namespace lcpc

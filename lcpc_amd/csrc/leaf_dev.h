// lcpc_amd/csrc/leaf_dev.h -- device functions of the BLAKE3 column hash that more than one translation unit needs: the chaining
// value of one 1 KiB chunk of a column's leaf message (kernels.hip K3: leaf_chunk_kernel, leaf_tree_kernel; batch_kernels.hip: their
// batch forms) and the 8-word digest loads / stores of the fold and tree kernels.
#pragma once
#include "kernels.h"
#include "field_dev.h"
#include "field_ln.h"
#include "blake3_dev.h"

namespace lcpc {

__device__ __forceinline__ void ld8(u32 d[8], const u32* p) {
  uint4 x = *reinterpret_cast<const uint4*>(p), y = *reinterpret_cast<const uint4*>(p + 4);
  d[0] = x.x; d[1] = x.y; d[2] = x.z; d[3] = x.w; d[4] = y.x; d[5] = y.y; d[6] = y.z; d[7] = y.w;
}
__device__ __forceinline__ void st8(u32* p, const u32 d[8]) {
  *reinterpret_cast<uint4*>(p) = make_uint4(d[0], d[1], d[2], d[3]);
  *reinterpret_cast<uint4*>(p + 4) = make_uint4(d[4], d[5], d[6], d[7]);
}
template <int NL, int PH> struct LeafRaw {
  static constexpr int NEL = (PH + 16 + NL - 1) / NL;     // elements a 16-word block touches
  Fe<NL> el[NEL];
};
// issue the global loads of one 64-byte block's elements (Montgomery form, not yet converted)
template <int NL, int PH>
__device__ __forceinline__ void leaf_load_raw(LeafRaw<NL, PH>& r, const LeafArgs& a, u64 col, int64_t row0) {
#pragma unroll
  for (int x = 0; x < LeafRaw<NL, PH>::NEL; x++) {
    const int64_t row = row0 + x;
    if (row >= 0 && (u64)row < a.n_rows_total) r.el[x] = fe_load<NL>(a.comm + ((u64)(row - a.row_base) * a.row_stride + col * a.col_stride) * NL);
    else r.el[x] = fe_zero<NL>();        // the 32-byte zero prefix (rows -1, -2, ..) and the tail past the message
  }
}
// Montgomery -> canonical little-endian words (PrimeField::to_repr), laid out as the block's 16 message words
template <int NL, int PH, bool CANON = false>
__device__ __forceinline__ void leaf_build_block(u32 m[16], const LeafRaw<NL, PH>& r) {
  Fe<NL> c[LeafRaw<NL, PH>::NEL];
#pragma unroll
  for (int x = 0; x < LeafRaw<NL, PH>::NEL; x++) {
    if constexpr (CANON) c[x] = r.el[x];                    // comm already canonical (LeafArgs::canon_in)
    else if constexpr (NL == 8) c[x] = fe_canon_r29(r.el[x]);
    else c[x] = fe_canon<NL>(r.el[x]);
  }
#pragma unroll
  for (int p = 0; p < 16; p++) m[p] = c[(PH + p) / NL].v[(PH + p) % NL];
}
template <int NL, int PH, bool CANON = false>
__device__ __forceinline__ void leaf_fill_block(u32 m[16], const LeafArgs& a, u64 col, int64_t row0) {
  LeafRaw<NL, PH> r;
  leaf_load_raw<NL, PH>(r, a, col, row0);
  leaf_build_block<NL, PH, CANON>(m, r);
}

// QUAD: four lanes per column, one compression per quad (b3_compress_quad): a small commitment has fewer (column, chunk)
// pairs than the chip has lanes, and a chunk is a chain of up to 16 dependent compressions -- ~300 instead of ~700 dependent
// instructions each.  The four lanes build the same message block (their loads coalesce to one); 64 columns per workgroup.
// Chaining value of chunk `chunk` of column `col`'s leaf message: in cv[8] (one lane per column), or spread over the quad
// (lane q: words q and 4 + q in cv_lo / cv_hi).
template <int NL, bool CANON, bool QUAD>
__device__ __forceinline__ void leaf_chunk_cv(const LeafArgs& a, u64 col, u32 chunk, u32 q, u32 cv[8], u32& cv_lo, u32& cv_hi) {
  const u64 total_len = 32 + (u64)NL * 4 * a.n_rows_total;
  const u64 chunk_off = (u64)chunk * 1024;
  const u32 chunk_len = (u32)((total_len - chunk_off) < 1024 ? (total_len - chunk_off) : 1024);
  const u32 nblocks = (chunk_len + 63) / 64;
  b3_set_iv(cv);
  cv_lo = b3_sel4(q, B3_IV0, B3_IV1, B3_IV2, B3_IV3); cv_hi = b3_sel4(q, B3_IV4, B3_IV5, B3_IV6, B3_IV7);   // QUAD: this lane's two words
  auto compress = [&](const u32* m, u32 blen, u32 flags) {
    if constexpr (QUAD) b3_compress_quad(q, cv_lo, cv_hi, m, chunk, blen, flags);
    else b3_compress(cv, m, chunk, blen, flags);
  };
  // element-word offset of block b's first word is 16*(16*chunk + b) - 8 (the zero prefix is words -8..-1)
  auto block_row0 = [&](u32 b, int& ph) -> int64_t {
    const int64_t s0 = ((int64_t)chunk * 16 + b) * 16 - 8;
    const int64_t r0 = s0 >= 0 ? s0 / NL : -((-s0 + NL - 1) / NL);
    ph = (int)(s0 - r0 * NL);
    return r0;
  };
  if constexpr (NL != 6) {
    // every block starts on an element boundary (PH == 0): software-pipeline the loads one block ahead
    // (two blocks per trip, their operands in two register sets that swap roles: no copy of the block fetched ahead)
    int ph;
    LeafRaw<NL, 0> ra, rb;
    auto one = [&](const LeafRaw<NL, 0>& r, u32 b) {
      u32 m[16];
      leaf_build_block<NL, 0, CANON>(m, r);
      const u32 rem = chunk_len - 64 * b;
      const u32 blen = rem < 64 ? rem : 64;
      u32 flags = (b == 0 ? B3_CHUNK_START : 0u);
      if (b == nblocks - 1) flags |= B3_CHUNK_END | (a.n_chunks_total == 1 ? B3_ROOT : 0u);
      compress(m, blen, flags);
    };
    leaf_load_raw<NL, 0>(ra, a, col, block_row0(0, ph));
    for (u32 b = 0; b < nblocks; b += 2) {
      if (b + 1 < nblocks) leaf_load_raw<NL, 0>(rb, a, col, block_row0(b + 1, ph));
      one(ra, b);
      if (b + 1 < nblocks) {
        if (b + 2 < nblocks) leaf_load_raw<NL, 0>(ra, a, col, block_row0(b + 2, ph));
        one(rb, b + 1);
      }
    }
  } else {
    for (u32 b = 0; b < nblocks; b++) {
      int ph;
      const int64_t row0 = block_row0(b, ph);
      u32 m[16];
      if (ph == 0) leaf_fill_block<NL, 0, CANON>(m, a, col, row0);
      else if (ph == 2) leaf_fill_block<NL, 2, CANON>(m, a, col, row0);
      else leaf_fill_block<NL, 4, CANON>(m, a, col, row0);
      const u32 rem = chunk_len - 64 * b;
      const u32 blen = rem < 64 ? rem : 64;
      u32 flags = (b == 0 ? B3_CHUNK_START : 0u);
      if (b == nblocks - 1) flags |= B3_CHUNK_END | (a.n_chunks_total == 1 ? B3_ROOT : 0u);
      compress(m, blen, flags);
    }
  }
}
}  // namespace lcpc

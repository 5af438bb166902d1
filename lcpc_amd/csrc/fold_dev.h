// lcpc_amd/csrc/fold_dev.h -- K8b, the Merkle path fold (kernels.h FoldPathsArgs): one lane's work, written once over the node function.
// N supplies DIGEST_WORDS and node(o, l, r): the chain digests' traits (chain_dev.h) and BLAKE3's (kernels.hip).
#pragma once
#include "kernels.h"

namespace lcpc {

template <int DW>
__device__ __forceinline__ void fold_ld(uint32_t d[DW], const uint32_t* p) {
#pragma unroll
  for (int i = 0; i < DW; i += 4) {
    const uint4 x = *reinterpret_cast<const uint4*>(p + i);
    d[i] = x.x; d[i + 1] = x.y; d[i + 2] = x.z; d[i + 3] = x.w;
  }
}

// The running digest, the sibling and the node's two operands are arrays indexed by compile-time constants only: they stay in registers
// (the level loop is not unrolled, its body is).  Which side the sibling goes to differs from lane to lane, so the operands are built
// by selects, not by a branch around two calls of the node function.
template <class N>
__device__ __forceinline__ void fold_path_lane(const FoldPathsArgs& a) {
  constexpr int DW = N::DIGEST_WORDS;
  const uint32_t k = blockIdx.x * 256u + threadIdx.x;
  if (k >= a.n_open) return;
  const uint64_t m = blockIdx.y;
  uint32_t h[DW], sib[DW], l[DW], r[DW], o[DW];
  fold_ld<DW>(h, a.leaves + m * a.leaves_stride + (uint64_t)k * DW);
  uint64_t cc = a.drawn[m * a.n_open + k];
  const uint32_t* s = a.sibs + m * a.sib_member + (uint64_t)k * a.sib_col;
  for (uint32_t lvl = 0; lvl < a.depth; lvl++, s += a.sib_lvl) {
    fold_ld<DW>(sib, s);
    const bool odd = (cc & 1) != 0;
#pragma unroll
    for (int i = 0; i < DW; i++) { l[i] = odd ? sib[i] : h[i]; r[i] = odd ? h[i] : sib[i]; }
    N::node(o, l, r);
#pragma unroll
    for (int i = 0; i < DW; i++) h[i] = o[i];
    cc >>= 1;
  }
  fold_ld<DW>(sib, a.roots + m * DW);
  uint32_t diff = 0;
#pragma unroll
  for (int i = 0; i < DW; i++) diff |= h[i] ^ sib[i];
  if (diff) {
    uint32_t* w = a.status + m * a.status_stride + k;
    *w = *w | FOLD_PATH_BIT;
  }
}

}  // namespace lcpc

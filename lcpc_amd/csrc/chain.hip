// lcpc_amd/csrc/chain.hip -- the host-callable launchers of the serial-chain digests (kernels.h: launch_chain_*): one switch from
// ChainHash to the digest's traits.  The kernels and the launch logic are chain_dev.h's, compiled in sha3.hip, sha256.hip and blake2b.hip.
#include "keccak_dev.h"
#include "sha256_dev.h"
#include "blake2b_dev.h"
#include "chain_dev.h"

namespace lcpc {

using Sha3Chain = KeccakChain<kc::KC_DOM_SHA3>;
using Keccak256Chain = KeccakChain<kc::KC_DOM_KECCAK>;
LCPC_CHAIN_LAUNCHERS(extern, Sha3Chain)
LCPC_CHAIN_LAUNCHERS(extern, Keccak256Chain)
LCPC_CHAIN_LAUNCHERS(extern, Sha256Chain)
LCPC_CHAIN_LAUNCHERS(extern, Blake2bChain)

// kernels.h's chain_shape is the traits restated for the host
template <class D> constexpr bool shape_matches(ChainHash h) {
  for (int nl = 2; nl <= 8; nl += 2)
    for (uint64_t r = 0; r < 40; r++) {
      const ChainShape s = chain_shape(h, nl, r);
      if (s.prefix_words != D::PREFIX || s.block_words != D::BLOCK || s.state_words != D::STATE_WORDS || s.digest_words != D::DIGEST_WORDS ||
          s.n_blocks != D::n_blocks(D::PREFIX + (uint64_t)(nl / 2) * r) || sizeof(typename D::Word) * D::N_ELEMS != 4 * D::STATE_WORDS)
        return false;
    }
  return true;
}
static_assert(shape_matches<Sha3Chain>(ChainHash::Sha3_256) && shape_matches<Keccak256Chain>(ChainHash::Keccak256) &&
              shape_matches<Sha256Chain>(ChainHash::Sha256) && shape_matches<Blake2bChain>(ChainHash::Blake2b), "chain_shape (kernels.h)");

// f(D{}) for the traits type D of h
template <class F> static hipError_t with_chain(ChainHash h, const F& f) {
  switch (h) {
    case ChainHash::Sha3_256: return f(Sha3Chain{});
    case ChainHash::Keccak256: return f(Keccak256Chain{});
    case ChainHash::Sha256: return f(Sha256Chain{});
    case ChainHash::Blake2b: return f(Blake2bChain{});
  }
  return hipErrorInvalidValue;
}

hipError_t launch_chain_leaves(ChainHash h, int nl, const LeafArgs& a, hipStream_t st) {
  return with_chain(h, [&](auto d) { return chain_leaves<decltype(d)>(nl, a, st); });
}
hipError_t launch_chain_leaves_batch(ChainHash h, int nl, const LeafArgs& a, u32 n_batch, u64 comm_stride, u64 out_stride, hipStream_t st) {
  return with_chain(h, [&](auto d) { return chain_leaves_batch<decltype(d)>(nl, a, n_batch, comm_stride, out_stride, st); });
}
hipError_t launch_chain_leaves_range(ChainHash h, int nl, const LeafArgs& a, u64 blk_begin, u64 blk_end, u32* state, hipStream_t st) {
  return with_chain(h, [&](auto d) { return chain_leaves_range<decltype(d)>(nl, a, blk_begin, blk_end, state, st); });
}
hipError_t launch_chain_merkle_tree(ChainHash h, u32* hashes, u64 np2, hipStream_t st, u32* root_out) {
  return with_chain(h, [&](auto d) { return chain_merkle_tree<decltype(d), false>(hashes, np2, 1, 0, st, root_out); });
}
hipError_t launch_chain_merkle_tree_batch(ChainHash h, u32* hashes, u64 np2, u32 n_batch, u64 hashes_stride, hipStream_t st, u32* root_out) {
  return with_chain(h, [&](auto d) { return chain_merkle_tree<decltype(d), true>(hashes, np2, n_batch, hashes_stride, st, root_out); });
}
hipError_t launch_chain_fold_paths(ChainHash h, const FoldPathsArgs& a, hipStream_t st) {
  return with_chain(h, [&](auto d) { return chain_fold_paths<decltype(d)>(a, st); });
}

}  // namespace lcpc

// lcpc_amd/csrc/chain_dev.h -- the column hash and Merkle tree of the serial-chain digests (SHA3-256, Keccak-256, SHA-256, BLAKE2b)
// for gfx950, written once over a digest traits type D (KeccakChain<DOM> in keccak_dev.h, Sha256Chain in sha256_dev.h, Blake2bChain in
// blake2b_dev.h).  BLAKE3's chunked tree is another algorithm (kernels.hip K3 / K4).
//
//   leaf[c] = D(0^P || to_repr(comm[0][c]) || ... || to_repr(comm[R-1][c]))   (lcpc-2d lib.rs:719-735; P = 8 D::PREFIX bytes, one Output<D>)
//   node    = D(left || right)                                                 (lib.rs:770-775)
//
// The leaf message is D::PREFIX + L R little-endian 64-bit words, one canonical limb each; a block of the digest is D::BLOCK of them:
// word k of the message is word k mod BLOCK of block k / BLOCK.  The hash is one serial chain per column, so the grid is one lane per
// column and nothing else.  L blocks (BLOCK L words) hold exactly BLOCK elements, so a kernel walks the message in groups of L blocks
// whose word -> (row, limb) map is a compile-time table.
//
// What D supplies:
//   PREFIX, BLOCK, DIGEST_WORDS (u32 words of a digest), STATE_WORDS (u32 words of a column's chaining value)
//   Elem / N_ELEMS: the chaining value in registers, Elem st[N_ELEMS];  Word, word(Elem), elem(Word): the same value in memory
//   Msg: the block being assembled (empty for a sponge, which absorbs into st)
//   init(st);  absorb(st, m, p, lo, hi): word p of the block;  finish_block(st, m, blk, n_words, n_blocks): the end-of-message padding
//   where blk holds it, then the compression;  store_digest(o, st);  node(o, l, r);  n_blocks(n_words)
//   batch_waves(nl, canon): the second launch bound of the batch leaf kernel, 0 = none
#pragma once
#include "kernels.h"
#include "field_ln.h"
#include "fold_dev.h"

namespace lcpc {

constexpr int chain_fdiv(int a, int b) { return a >= 0 ? a / b : -((-a + b - 1) / b); }

// block B (0 <= B < L) of the group starting at row BLOCK j: words BLOCK B .. BLOCK B + BLOCK - 1 of the group, word w of the group
// being limb (w - PREFIX) mod L of row BLOCK j + (w - PREFIX) div L
template <class D, int NL, bool CANON, int B>
__device__ __forceinline__ void chain_load_block(typename D::Elem* st, typename D::Msg& m, const LeafArgs& a, u64 col, int64_t row_g) {
  constexpr int L = NL / 2, W = D::BLOCK, P = D::PREFIX;
  constexpr int X0 = chain_fdiv(W * B - P, L), X1 = chain_fdiv(W * B + W - 1 - P, L), NE = X1 - X0 + 1;
  Fe<NL> el[NE];
#pragma unroll
  for (int x = 0; x < NE; x++) {
    const int64_t row = row_g + X0 + x;
    if (row >= 0 && (u64)row < a.n_rows_total) {
      el[x] = fe_load<NL>(a.comm + ((u64)(row - a.row_base) * a.row_stride + col * a.col_stride) * NL);
      if constexpr (!CANON) {
        if constexpr (NL == 8) el[x] = fe_canon_r29(el[x]);
        else el[x] = fe_canon<NL>(el[x]);
      }
    } else {
      el[x] = fe_zero<NL>();       // the zero prefix (rows < 0) and the zero words past the message
    }
  }
#pragma unroll
  for (int p = 0; p < W; p++) {
    const int w = W * B + p - P;
    const int x = chain_fdiv(w, L), l = w - x * L;
    D::absorb(st, m, p, el[x - X0].v[2 * l], el[x - X0].v[2 * l + 1]);
  }
}

// blocks B, B + 1, .. L - 1 of group j that lie in [b0, b1): a block outside the range is neither loaded nor compressed.  WHOLE (the
// range is the whole message, b0 = 0): the first block behind the end leaves the group, where a true range tests every block -- the
// same blocks run either way, but each entry point keeps its register allocation only with its own form (LABNOTES.md)
template <class D, int NL, bool CANON, bool WHOLE, int B>
__device__ __forceinline__ void chain_step(typename D::Elem* st, const LeafArgs& a, u64 col, u64 j, u64 n_words, u64 n_blocks, u64 b0, u64 b1) {
  constexpr int L = NL / 2;
  const u64 blk = j * L + B;
  if constexpr (WHOLE) { if (blk >= b1) return; }
  if (blk >= b0 && blk < b1) {
    typename D::Msg m;
    chain_load_block<D, NL, CANON, B>(st, m, a, col, (int64_t)(D::BLOCK * j));
    D::finish_block(st, m, blk, n_words, n_blocks);
  }
  if constexpr (B + 1 < L) chain_step<D, NL, CANON, WHOLE, B + 1>(st, a, col, j, n_words, n_blocks, b0, b1);
}

// one column's chain over blocks [b0, b1).  It starts from D::init when b0 == 0 and from `state` otherwise; it leaves the chaining value
// in `state` when b1 is not the message's last block and the digest in a.out when it is.  state: word i of column c at
// state[i * n_cols + c], so that a wave reads and writes 64 consecutive words per index.  whole = the one-shot and batch kernels:
// [0, n_blocks), no state
template <class D, int NL, bool CANON, bool WHOLE>
__device__ __forceinline__ void chain_column(const LeafArgs& a, u64 col, u64 b0, u64 b1, typename D::Word* state) {
  constexpr int L = NL / 2;
  const u64 n_words = D::PREFIX + (u64)L * a.n_rows_total;
  const u64 n_blocks = D::n_blocks(n_words);
  if constexpr (WHOLE) { b0 = 0; b1 = n_blocks; }
  typename D::Elem st[D::N_ELEMS];
  if (b0 == 0) {
    D::init(st);
  } else {
#pragma unroll
    for (int i = 0; i < D::N_ELEMS; i++) st[i] = D::elem(state[(u64)i * a.n_cols + col]);
  }
  for (u64 j = b0 / L; j * L < b1; j++) chain_step<D, NL, CANON, WHOLE, 0>(st, a, col, j, n_words, n_blocks, b0, b1);
  if (b1 == n_blocks) {
    D::store_digest(a.out + col * D::DIGEST_WORDS, st);
  } else {
#pragma unroll
    for (int i = 0; i < D::N_ELEMS; i++) state[(u64)i * a.n_cols + col] = D::word(st[i]);
  }
}

// Three entry points and not one: the register allocator treats them differently (see batch_waves of the traits), so the one-shot
// kernel is not the batch kernel with one member.
template <class D, int NL, bool CANON>
__global__ void __launch_bounds__(256) chain_leaf_kernel(LeafArgs a) {
  const u64 col = (u64)blockIdx.x * 256 + threadIdx.x;
  if (col >= a.n_cols) return;
  chain_column<D, NL, CANON, true>(a, col, 0, 0, nullptr);
}

// n_batch equal-shape members of one encoder, the member index blockIdx.y: the same chain per column on member i's comm and out, which
// start i * comm_stride / i * out_stride words behind member 0's
template <class D, int NL, bool CANON>
__global__ void __launch_bounds__(256, D::batch_waves(NL, CANON)) chain_leaf_batch_kernel(LeafArgs a, u64 comm_stride, u64 out_stride) {
  const u64 col = (u64)blockIdx.x * 256 + threadIdx.x;
  if (col >= a.n_cols) return;
  a.comm += (u64)blockIdx.y * comm_stride;
  a.out += (u64)blockIdx.y * out_stride;
  chain_column<D, NL, CANON, true>(a, col, 0, 0, nullptr);
}

template <class D, int NL, bool CANON>
__global__ void __launch_bounds__(256) chain_leaf_range_kernel(LeafArgs a, u64 b0, u64 b1, typename D::Word* state) {
  const u64 col = (u64)blockIdx.x * 256 + threadIdx.x;
  if (col >= a.n_cols) return;
  chain_column<D, NL, CANON, false>(a, col, b0, b1, state);
}

// each workgroup folds 2^lsub consecutive nodes of a level `lsub` levels up through LDS, one node per lane, writing every level to its
// slot of the flat `hashes` array (lib.rs:656-666, 747-760).  BATCH: member blockIdx.y's hashes start blockIdx.y * hashes_stride words
// behind member 0's, its root goes to root_out (may be null) + DIGEST_WORDS blockIdx.y.  A single commit runs the instantiation without
// the member offset: with it (grid.y = 1, stride 0) the sponges' trees measured 4 - 7 % slower (LABNOTES.md)
template <class D, bool BATCH>
__global__ void __launch_bounds__(256) chain_merkle_subtree_kernel(u32* hashes, u64 in_off, u64 width, u32 lsub, u32* root_out, u64 hashes_stride) {
  constexpr int DW = D::DIGEST_WORDS;
  __shared__ u32 buf[256 * DW];
  if constexpr (BATCH) hashes += (u64)blockIdx.y * hashes_stride;
  const u32 tid = threadIdx.x;
  const u64 base = (u64)blockIdx.x << lsub;
  u64 layer_in = in_off, w = width, layer_out = in_off + width;
  u32 n_out = 1u << (lsub - 1);
  u32 o[DW];
  if (tid < n_out) {
    const u32* g = hashes + (layer_in + base + 2 * tid) * DW;
    u32 l[DW], r[DW];
#pragma unroll
    for (int i = 0; i < DW; i++) { l[i] = g[i]; r[i] = g[DW + i]; }
    D::node(o, l, r);
    u32* d = hashes + (layer_out + (base >> 1) + tid) * DW;
#pragma unroll
    for (int i = 0; i < DW; i++) { d[i] = o[i]; buf[tid * DW + i] = o[i]; }
  }
  for (u32 j = 2; j <= lsub; j++) {
    __syncthreads();
    layer_in = layer_out;
    w >>= 1;
    layer_out = layer_in + w;
    n_out >>= 1;
    const bool act = tid < n_out;
    if (act) D::node(o, buf + 2 * tid * DW, buf + (2 * tid + 1) * DW);
    __syncthreads();
    if (act) {
      u32* d = hashes + (layer_out + (base >> j) + tid) * DW;
#pragma unroll
      for (int i = 0; i < DW; i++) { d[i] = o[i]; buf[tid * DW + i] = o[i]; }
    }
  }
  if (root_out != nullptr) {
    __syncthreads();
    if (tid < DW) root_out[(BATCH ? (u64)blockIdx.y * DW : 0) + tid] = buf[tid];
  }
}

// K8b (kernels.h FoldPathsArgs, fold_dev.h): one lane folds one opened column's path with D::node and compares with the member's root
template <class D>
__global__ void __launch_bounds__(256) chain_fold_paths_kernel(FoldPathsArgs a) {
  fold_path_lane<D>(a);
}

// ---- the launchers of one digest: chain.hip switches over ChainHash to these; each is instantiated in its digest's .hip ----
// F<NL, CANON>: a functor that launches one instantiation; the nl / canon_in switch written once
template <class F>
static void chain_dispatch(int nl, bool canon, const F& f) {
  switch (nl) {
    case 2: if (canon) f.template operator()<2, true>(); else f.template operator()<2, false>(); break;
    case 4: if (canon) f.template operator()<4, true>(); else f.template operator()<4, false>(); break;
    case 6: if (canon) f.template operator()<6, true>(); else f.template operator()<6, false>(); break;
    case 8: if (canon) f.template operator()<8, true>(); else f.template operator()<8, false>(); break;
  }
}

template <class D> struct ChainLeafLaunch {
  const LeafArgs& a; dim3 grid; hipStream_t st;
  template <int NL, bool CANON> void operator()() const { hipLaunchKernelGGL((chain_leaf_kernel<D, NL, CANON>), grid, dim3(256), 0, st, a); }
};
template <class D> struct ChainLeafBatchLaunch {
  const LeafArgs& a; dim3 grid; u64 comm_stride, out_stride; hipStream_t st;
  template <int NL, bool CANON> void operator()() const {
    // Ft255's Ligero comm is canonical: the other form has no batch user and is refused by the launcher
    if constexpr (!(NL == 8 && !CANON)) hipLaunchKernelGGL((chain_leaf_batch_kernel<D, NL, CANON>), grid, dim3(256), 0, st, a, comm_stride, out_stride);
  }
};
template <class D> struct ChainLeafRangeLaunch {
  const LeafArgs& a; dim3 grid; u64 b0, b1; typename D::Word* state; hipStream_t st;
  template <int NL, bool CANON> void operator()() const {
    hipLaunchKernelGGL((chain_leaf_range_kernel<D, NL, CANON>), grid, dim3(256), 0, st, a, b0, b1, state);
  }
};

template <class D> hipError_t chain_leaves(int nl, const LeafArgs& a, hipStream_t st) {
  if (a.n_cols == 0) return hipSuccess;
  if (!nl_ok(nl)) return hipErrorInvalidValue;
  chain_dispatch(nl, a.canon_in != 0, ChainLeafLaunch<D>{a, dim3((unsigned)((a.n_cols + 255) / 256)), st});
  return hipGetLastError();
}

template <class D> hipError_t chain_leaves_batch(int nl, const LeafArgs& a, u32 n_batch, u64 comm_stride, u64 out_stride, hipStream_t st) {
  if (n_batch > 65535) return hipErrorInvalidValue;          // grid.y
  if (!nl_ok(nl)) return hipErrorInvalidValue;
  if (nl == 8 && !a.canon_in) return hipErrorInvalidValue;
  if (a.n_cols == 0 || n_batch == 0) return hipSuccess;
  chain_dispatch(nl, a.canon_in != 0, ChainLeafBatchLaunch<D>{a, dim3((unsigned)((a.n_cols + 255) / 256), n_batch), comm_stride, out_stride, st});
  return hipGetLastError();
}

template <class D> hipError_t chain_leaves_range(int nl, const LeafArgs& a, u64 b0, u64 b1, u32* state, hipStream_t st) {
  if (!nl_ok(nl)) return hipErrorInvalidValue;
  if (b0 > b1 || b1 > D::n_blocks(D::PREFIX + (u64)(nl / 2) * a.n_rows_total)) return hipErrorInvalidValue;
  if (a.n_cols == 0 || b0 == b1) return hipSuccess;
  chain_dispatch(nl, a.canon_in != 0,
                 ChainLeafRangeLaunch<D>{a, dim3((unsigned)((a.n_cols + 255) / 256)), b0, b1, reinterpret_cast<typename D::Word*>(state), st});
  return hipGetLastError();
}

// the whole tree above the np2 leaf digests of every member, in as few launches as possible (nine levels each).  BATCH = false: one
// member, whatever n_batch and hashes_stride say
template <class D, bool BATCH> hipError_t chain_merkle_tree(u32* hashes, u64 np2, u32 n_batch, u64 hashes_stride, hipStream_t st, u32* root_out) {
  if (n_batch > 65535) return hipErrorInvalidValue;          // grid.y
  if (n_batch == 0) return hipSuccess;
  u64 in_off = 0, width = np2;
  while (width > 1) {
    u32 lw = 0;
    while (((u64)1 << lw) < width) lw++;
    const u32 lsub = lw < 9 ? lw : 9;
    const u64 nwg = width >> lsub;
    hipLaunchKernelGGL((chain_merkle_subtree_kernel<D, BATCH>), dim3((unsigned)nwg, BATCH ? n_batch : 1), dim3(256), 0, st, hashes, in_off, width,
                       lsub, lsub == lw ? root_out : (u32*)nullptr, hashes_stride);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    for (u32 j = 0; j < lsub; j++) { in_off += width; width >>= 1; }
  }
  return hipSuccess;
}

template <class D> hipError_t chain_fold_paths(const FoldPathsArgs& a, hipStream_t st) {
  const int job = fold_paths_job(a);
  if (job <= 0) return job ? hipErrorInvalidValue : hipSuccess;
  hipLaunchKernelGGL((chain_fold_paths_kernel<D>), dim3((a.n_open + 255) / 256, a.n_batch), dim3(256), 0, st, a);
  return hipGetLastError();
}

// LCPC_CHAIN_LAUNCHERS(, D) in D's .hip instantiates the six; LCPC_CHAIN_LAUNCHERS(extern, D) in chain.hip names them without compiling them
#define LCPC_CHAIN_LAUNCHERS(EXT, D)                                                                                    \
  EXT template hipError_t chain_leaves<D>(int, const LeafArgs&, hipStream_t);                                           \
  EXT template hipError_t chain_leaves_batch<D>(int, const LeafArgs&, u32, u64, u64, hipStream_t);                      \
  EXT template hipError_t chain_leaves_range<D>(int, const LeafArgs&, u64, u64, u32*, hipStream_t);                     \
  EXT template hipError_t chain_merkle_tree<D, false>(u32*, u64, u32, u64, hipStream_t, u32*);                          \
  EXT template hipError_t chain_merkle_tree<D, true>(u32*, u64, u32, u64, hipStream_t, u32*);                           \
  EXT template hipError_t chain_fold_paths<D>(const FoldPathsArgs&, hipStream_t);

}  // namespace lcpc

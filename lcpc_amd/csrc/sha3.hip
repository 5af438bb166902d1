// lcpc_amd/csrc/sha3.hip -- SHA3-256 and Keccak-256 column hash and Merkle tree (LcCommit<Sha3_256, E>, LcCommit<Keccak256, E>)
// for gfx950.  The two differ in one constant, the byte DOM that opens the padding: 0x06 for SHA3-256 (FIPS 202), 0x01 for
// Keccak-256 (the pre-FIPS padding, the EVM's KECCAK256).  It is a template parameter of every kernel here; what follows is
// written for SHA3-256.
//
//   leaf[c] = SHA3-256(0^32 || to_repr(comm[0][c]) || ... || to_repr(comm[R-1][c]))   (lcpc-2d lib.rs:719-735)
//   node    = SHA3-256(left || right)                                               (lib.rs:770-775)
//
// The leaf message is 4 + L R little-endian 64-bit words, one canonical limb each, so every word is one Keccak lane:
// word k goes into lane k mod 17 of block k / 17 (the 136-byte rate).  Unlike BLAKE3's chunks the sponge is one serial
// chain per column, so the grid is one lane per column and nothing else.  L blocks (17 L words) hold exactly 17 elements,
// so the kernel walks the message in groups of L blocks whose word -> (row, limb) map is a compile-time table.
#include "kernels.h"
#include "field_ln.h"
#include "keccak_dev.h"

namespace lcpc {

using kc::Lane;

constexpr int fdiv(int a, int b) { return a >= 0 ? a / b : -((-a + b - 1) / b); }

// absorb block b (0 <= b < L) of the group starting at row 17 j into s: words 17 b .. 17 b + 16 of the group, word w of the
// group being limb (w - 4) mod L of row 17 j + (w - 4) div L
template <int NL, bool CANON, int B>
__device__ __forceinline__ void sha3_absorb_block(Lane s[25], const LeafArgs& a, u64 col, int64_t row_g) {
  constexpr int L = NL / 2;
  constexpr int X0 = fdiv(17 * B - 4, L), X1 = fdiv(17 * B + 12, L), NE = X1 - X0 + 1;
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
      el[x] = fe_zero<NL>();       // the 32-byte zero prefix (rows < 0) and the zero words past the message
    }
  }
#pragma unroll
  for (int p = 0; p < 17; p++) {
    const int w = 17 * B + p - 4;
    const int x = fdiv(w, L), l = w - x * L;
    s[p].lo ^= el[x - X0].v[2 * l];
    s[p].hi ^= el[x - X0].v[2 * l + 1];
  }
}

template <int NL, bool CANON, u32 DOM, int B>
__device__ __forceinline__ void sha3_group_step(Lane s[25], const LeafArgs& a, u64 col, u64 j, u64 n_words, u64 n_blocks) {
  constexpr int L = NL / 2;
  const u64 blk = j * L + B;
  if (blk >= n_blocks) return;
  sha3_absorb_block<NL, CANON, B>(s, a, col, (int64_t)(17 * j));
  if (17 * blk + 17 > n_words) {
    // the block that holds the end of the message: pad10*1 behind the domain bits (DOM ... 0x80; SHA3: 0x06); the message is whole
    // words, so the DOM byte starts lane n_words - 17 blk
    const u32 q = (u32)(n_words - 17 * blk);
    if constexpr (DOM == kc::KC_DOM_SHA3) {
#pragma unroll
      for (u32 p = 0; p < 17; p++) s[p].lo ^= (p == q) ? DOM : 0u;
    } else {
      // the same selects as the SHA3-256 instantiation: the byte comes from a scalar register the compiler cannot see through,
      // so that it does not turn `? 1 : 0` into a per-lane boolean and allocate the whole kernel differently
      u32 dom = DOM;
      asm volatile("" : "+s"(dom));
#pragma unroll
      for (u32 p = 0; p < 17; p++) s[p].lo ^= (p == q) ? dom : 0u;
    }
    s[16].hi ^= 0x80000000u;
  }
  kc::keccak_f(s);
  if constexpr (B + 1 < L) sha3_group_step<NL, CANON, DOM, B + 1>(s, a, col, j, n_words, n_blocks);
}

template <int NL, bool CANON, u32 DOM>
__global__ void __launch_bounds__(256) sha3_leaf_kernel(LeafArgs a) {
  const u64 col = (u64)blockIdx.x * 256 + threadIdx.x;
  if (col >= a.n_cols) return;
  constexpr int L = NL / 2;
  const u64 n_words = 4 + (u64)L * a.n_rows_total;
  const u64 n_blocks = n_words / 17 + 1;          // the padding always fits: a message of 17 k words takes a block of its own
  Lane s[25];
#pragma unroll
  for (int i = 0; i < 25; i++) s[i] = {0u, 0u};
  for (u64 j = 0; j * L < n_blocks; j++) sha3_group_step<NL, CANON, DOM, 0>(s, a, col, j, n_words, n_blocks);
  u32* o = a.out + col * 8;
  *reinterpret_cast<uint4*>(o) = make_uint4(s[0].lo, s[0].hi, s[1].lo, s[1].hi);
  *reinterpret_cast<uint4*>(o + 4) = make_uint4(s[2].lo, s[2].hi, s[3].lo, s[3].hi);
}

template <u32 DOM>
static hipError_t launch_keccak_leaves(int nl, const LeafArgs& a, hipStream_t st) {
  if (a.n_cols == 0) return hipSuccess;
  const dim3 grid((unsigned)((a.n_cols + 255) / 256));
#define SHA3_CASE(NLV)                                                                                          \
  case NLV:                                                                                                     \
    if (a.canon_in) hipLaunchKernelGGL((sha3_leaf_kernel<NLV, true, DOM>), grid, dim3(256), 0, st, a);       \
    else hipLaunchKernelGGL((sha3_leaf_kernel<NLV, false, DOM>), grid, dim3(256), 0, st, a);                 \
    break;
  switch (nl) {
    SHA3_CASE(2) SHA3_CASE(4) SHA3_CASE(6) SHA3_CASE(8)
    default: return hipErrorInvalidValue;
  }
#undef SHA3_CASE
  return hipGetLastError();
}
hipError_t launch_sha3_leaves(int nl, const LeafArgs& a, hipStream_t st) { return launch_keccak_leaves<kc::KC_DOM_SHA3>(nl, a, st); }
hipError_t launch_keccak256_leaves(int nl, const LeafArgs& a, hipStream_t st) { return launch_keccak_leaves<kc::KC_DOM_KECCAK>(nl, a, st); }

// ---- the batch form (kernels.h: launch_sha3_leaves_batch; batch.cpp) ----
// sha3_leaf_kernel for n_batch equal-shape members of one encoder, the member index blockIdx.y: the same chain per column on
// member i's comm and out, which start i * comm_stride / i * out_stride words behind member 0's
template <int NL, bool CANON, u32 DOM>
__global__ void __launch_bounds__(256) sha3_leaf_batch_kernel(LeafArgs a, u64 comm_stride, u64 out_stride) {
  const u64 col = (u64)blockIdx.x * 256 + threadIdx.x;
  if (col >= a.n_cols) return;
  a.comm += (u64)blockIdx.y * comm_stride;
  a.out += (u64)blockIdx.y * out_stride;
  constexpr int L = NL / 2;
  const u64 n_words = 4 + (u64)L * a.n_rows_total;
  const u64 n_blocks = n_words / 17 + 1;
  Lane s[25];
#pragma unroll
  for (int i = 0; i < 25; i++) s[i] = {0u, 0u};
  for (u64 j = 0; j * L < n_blocks; j++) sha3_group_step<NL, CANON, DOM, 0>(s, a, col, j, n_words, n_blocks);
  u32* o = a.out + col * 8;
  *reinterpret_cast<uint4*>(o) = make_uint4(s[0].lo, s[0].hi, s[1].lo, s[1].hi);
  *reinterpret_cast<uint4*>(o + 4) = make_uint4(s[2].lo, s[2].hi, s[3].lo, s[3].hi);
}

template <u32 DOM>
static hipError_t launch_keccak_leaves_batch(int nl, const LeafArgs& a, u32 n_batch, u64 comm_stride, u64 out_stride, hipStream_t st) {
  if (n_batch > 65535) return hipErrorInvalidValue;          // grid.y
  if (nl != 2 && nl != 4 && nl != 6 && nl != 8) return hipErrorInvalidValue;
  if (nl == 8 && !a.canon_in) return hipErrorInvalidValue;   // Ft255's Ligero comm is canonical: the other form has no batch user
  if (a.n_cols == 0 || n_batch == 0) return hipSuccess;
  const dim3 grid((unsigned)((a.n_cols + 255) / 256), n_batch);
#define SHA3_CASE(NLV)                                                                                                                  \
  case NLV:                                                                                                                             \
    if (a.canon_in) hipLaunchKernelGGL((sha3_leaf_batch_kernel<NLV, true, DOM>), grid, dim3(256), 0, st, a, comm_stride, out_stride);   \
    else hipLaunchKernelGGL((sha3_leaf_batch_kernel<NLV, false, DOM>), grid, dim3(256), 0, st, a, comm_stride, out_stride);             \
    break;
  switch (nl) {
    SHA3_CASE(2) SHA3_CASE(4) SHA3_CASE(6)
    case 8: hipLaunchKernelGGL((sha3_leaf_batch_kernel<8, true, DOM>), grid, dim3(256), 0, st, a, comm_stride, out_stride); break;
  }
#undef SHA3_CASE
  return hipGetLastError();
}
hipError_t launch_sha3_leaves_batch(int nl, const LeafArgs& a, u32 n_batch, u64 comm_stride, u64 out_stride, hipStream_t st) {
  return launch_keccak_leaves_batch<kc::KC_DOM_SHA3>(nl, a, n_batch, comm_stride, out_stride, st);
}
hipError_t launch_keccak256_leaves_batch(int nl, const LeafArgs& a, u32 n_batch, u64 comm_stride, u64 out_stride, hipStream_t st) {
  return launch_keccak_leaves_batch<kc::KC_DOM_KECCAK>(nl, a, n_batch, comm_stride, out_stride, st);
}

// ---- the same chain a block range at a time (kernels.h: launch_sha3_leaves_range) ----
// sha3_group_step for the blocks of group j that lie in [b0, b1): a block outside the range is neither loaded nor permuted
template <int NL, bool CANON, u32 DOM, int B>
__device__ __forceinline__ void sha3_range_step(Lane s[25], const LeafArgs& a, u64 col, u64 j, u64 n_words, u64 b0, u64 b1) {
  constexpr int L = NL / 2;
  const u64 blk = j * L + B;
  if (blk >= b0 && blk < b1) {
    sha3_absorb_block<NL, CANON, B>(s, a, col, (int64_t)(17 * j));
    if (17 * blk + 17 > n_words) {          // the block that holds the end of the message: padded as in sha3_group_step
      const u32 q = (u32)(n_words - 17 * blk);
      u32 dom = DOM;
      asm volatile("" : "+s"(dom));
#pragma unroll
      for (u32 p = 0; p < 17; p++) s[p].lo ^= (p == q) ? dom : 0u;
      s[16].hi ^= 0x80000000u;
    }
    kc::keccak_f(s);
  }
  if constexpr (B + 1 < L) sha3_range_step<NL, CANON, DOM, B + 1>(s, a, col, j, n_words, b0, b1);
}

// state: lane i of column c at state[i * n_cols + c] -- a wave reads and writes 64 consecutive 8-byte words per lane index
template <int NL, bool CANON, u32 DOM>
__global__ void __launch_bounds__(256) sha3_leaf_range_kernel(LeafArgs a, u64 b0, u64 b1, uint2* state) {
  const u64 col = (u64)blockIdx.x * 256 + threadIdx.x;
  if (col >= a.n_cols) return;
  constexpr int L = NL / 2;
  const u64 n_words = 4 + (u64)L * a.n_rows_total;
  const u64 n_blocks = n_words / 17 + 1;
  Lane s[25];
  if (b0 == 0) {
#pragma unroll
    for (int i = 0; i < 25; i++) s[i] = {0u, 0u};
  } else {
#pragma unroll
    for (int i = 0; i < 25; i++) { const uint2 v = state[(u64)i * a.n_cols + col]; s[i] = {v.x, v.y}; }
  }
  for (u64 j = b0 / L; j * L < b1; j++) sha3_range_step<NL, CANON, DOM, 0>(s, a, col, j, n_words, b0, b1);
  if (b1 == n_blocks) {
    u32* o = a.out + col * 8;
    *reinterpret_cast<uint4*>(o) = make_uint4(s[0].lo, s[0].hi, s[1].lo, s[1].hi);
    *reinterpret_cast<uint4*>(o + 4) = make_uint4(s[2].lo, s[2].hi, s[3].lo, s[3].hi);
  } else {
#pragma unroll
    for (int i = 0; i < 25; i++) state[(u64)i * a.n_cols + col] = make_uint2(s[i].lo, s[i].hi);
  }
}

template <u32 DOM>
static hipError_t launch_keccak_leaves_range(int nl, const LeafArgs& a, u64 b0, u64 b1, uint64_t* state, hipStream_t st) {
  if (nl != 2 && nl != 4 && nl != 6 && nl != 8) return hipErrorInvalidValue;
  if (b0 > b1 || b1 > sha3_leaf_blocks(nl, a.n_rows_total)) return hipErrorInvalidValue;
  if (a.n_cols == 0 || b0 == b1) return hipSuccess;
  const dim3 grid((unsigned)((a.n_cols + 255) / 256));
  uint2* s2 = reinterpret_cast<uint2*>(state);
#define SHA3_CASE(NLV)                                                                                                      \
  case NLV:                                                                                                                 \
    if (a.canon_in) hipLaunchKernelGGL((sha3_leaf_range_kernel<NLV, true, DOM>), grid, dim3(256), 0, st, a, b0, b1, s2);    \
    else hipLaunchKernelGGL((sha3_leaf_range_kernel<NLV, false, DOM>), grid, dim3(256), 0, st, a, b0, b1, s2);              \
    break;
  switch (nl) { SHA3_CASE(2) SHA3_CASE(4) SHA3_CASE(6) SHA3_CASE(8) }
#undef SHA3_CASE
  return hipGetLastError();
}
hipError_t launch_sha3_leaves_range(int nl, const LeafArgs& a, uint64_t blk_begin, uint64_t blk_end, uint64_t* state, hipStream_t st) {
  return launch_keccak_leaves_range<kc::KC_DOM_SHA3>(nl, a, blk_begin, blk_end, state, st);
}
hipError_t launch_keccak256_leaves_range(int nl, const LeafArgs& a, uint64_t blk_begin, uint64_t blk_end, uint64_t* state, hipStream_t st) {
  return launch_keccak_leaves_range<kc::KC_DOM_KECCAK>(nl, a, blk_begin, blk_end, state, st);
}

// parent = SHA3-256(left || right) (DOM = 0x01: Keccak-256): 8 words, one permutation
template <u32 DOM>
__device__ __forceinline__ void sha3_node(u32 o[8], const u32* l, const u32* r) {
  Lane s[25];
#pragma unroll
  for (int i = 0; i < 25; i++) s[i] = {0u, 0u};
#pragma unroll
  for (int i = 0; i < 4; i++) { s[i] = {l[2 * i], l[2 * i + 1]}; s[4 + i] = {r[2 * i], r[2 * i + 1]}; }
  s[8].lo = DOM;
  s[16].hi = 0x80000000u;
  kc::keccak_f(s);
#pragma unroll
  for (int i = 0; i < 4; i++) { o[2 * i] = s[i].lo; o[2 * i + 1] = s[i].hi; }
}

// the counterpart of merkle_subtree_kernel (kernels.hip): each workgroup folds 2^lsub consecutive nodes of a level `lsub` levels
// up through LDS, one node per lane, writing every level to its slot of the flat `hashes` array (lib.rs:656-666, 747-760)
template <u32 DOM>
__global__ void __launch_bounds__(256) sha3_merkle_subtree_kernel(u32* hashes, u64 in_off, u64 width, u32 lsub, u32* root_out) {
  __shared__ u32 buf[256 * 8];
  const u32 tid = threadIdx.x;
  const u64 base = (u64)blockIdx.x << lsub;
  u64 layer_in = in_off, w = width, layer_out = in_off + width;
  u32 n_out = 1u << (lsub - 1);
  u32 l[8], r[8], o[8];
  if (tid < n_out) {
    const u32* g = hashes + (layer_in + base + 2 * tid) * 8;
#pragma unroll
    for (int i = 0; i < 8; i++) { l[i] = g[i]; r[i] = g[8 + i]; }
    sha3_node<DOM>(o, l, r);
    u32* d = hashes + (layer_out + (base >> 1) + tid) * 8;
#pragma unroll
    for (int i = 0; i < 8; i++) { d[i] = o[i]; buf[tid * 8 + i] = o[i]; }
  }
  for (u32 j = 2; j <= lsub; j++) {
    __syncthreads();
    layer_in = layer_out;
    w >>= 1;
    layer_out = layer_in + w;
    n_out >>= 1;
    const bool act = tid < n_out;
    if (act) sha3_node<DOM>(o, buf + 2 * tid * 8, buf + (2 * tid + 1) * 8);
    __syncthreads();
    if (act) {
      u32* d = hashes + (layer_out + (base >> j) + tid) * 8;
#pragma unroll
      for (int i = 0; i < 8; i++) { d[i] = o[i]; buf[tid * 8 + i] = o[i]; }
    }
  }
  if (root_out != nullptr) {
    __syncthreads();
    if (tid < 8) root_out[tid] = buf[tid];
  }
}

template <u32 DOM>
static hipError_t launch_keccak_merkle_tree(u32* hashes, u64 np2, hipStream_t st, u32* root_out) {
  u64 in_off = 0, width = np2;
  while (width > 1) {
    u32 lw = 0;
    while (((u64)1 << lw) < width) lw++;
    const u32 lsub = lw < 9 ? lw : 9;
    const u64 nwg = width >> lsub;
    hipLaunchKernelGGL(sha3_merkle_subtree_kernel<DOM>, dim3((unsigned)nwg), dim3(256), 0, st, hashes, in_off, width, lsub,
                       lsub == lw ? root_out : (u32*)nullptr);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    for (u32 j = 0; j < lsub; j++) { in_off += width; width >>= 1; }
  }
  return hipSuccess;
}
hipError_t launch_sha3_merkle_tree(u32* hashes, u64 np2, hipStream_t st, u32* root_out) {
  return launch_keccak_merkle_tree<kc::KC_DOM_SHA3>(hashes, np2, st, root_out);
}
hipError_t launch_keccak256_merkle_tree(u32* hashes, u64 np2, hipStream_t st, u32* root_out) {
  return launch_keccak_merkle_tree<kc::KC_DOM_KECCAK>(hashes, np2, st, root_out);
}


// sha3_merkle_subtree_kernel per member (blockIdx.y): member i's hashes start i * hashes_stride words behind member 0's; root_out
// (may be null): [n_batch][8], member i's root at root_out + 8 i
template <u32 DOM>
__global__ void __launch_bounds__(256) sha3_merkle_subtree_batch_kernel(u32* hashes, u64 in_off, u64 width, u32 lsub, u32* root_out,
                                                                        u64 hashes_stride) {
  __shared__ u32 buf[256 * 8];
  hashes += (u64)blockIdx.y * hashes_stride;
  const u32 tid = threadIdx.x;
  const u64 base = (u64)blockIdx.x << lsub;
  u64 layer_in = in_off, w = width, layer_out = in_off + width;
  u32 n_out = 1u << (lsub - 1);
  u32 l[8], r[8], o[8];
  if (tid < n_out) {
    const u32* g = hashes + (layer_in + base + 2 * tid) * 8;
#pragma unroll
    for (int i = 0; i < 8; i++) { l[i] = g[i]; r[i] = g[8 + i]; }
    sha3_node<DOM>(o, l, r);
    u32* d = hashes + (layer_out + (base >> 1) + tid) * 8;
#pragma unroll
    for (int i = 0; i < 8; i++) { d[i] = o[i]; buf[tid * 8 + i] = o[i]; }
  }
  for (u32 j = 2; j <= lsub; j++) {
    __syncthreads();
    layer_in = layer_out;
    w >>= 1;
    layer_out = layer_in + w;
    n_out >>= 1;
    const bool act = tid < n_out;
    if (act) sha3_node<DOM>(o, buf + 2 * tid * 8, buf + (2 * tid + 1) * 8);
    __syncthreads();
    if (act) {
      u32* d = hashes + (layer_out + (base >> j) + tid) * 8;
#pragma unroll
      for (int i = 0; i < 8; i++) { d[i] = o[i]; buf[tid * 8 + i] = o[i]; }
    }
  }
  if (root_out != nullptr) {
    __syncthreads();
    if (tid < 8) root_out[(u64)blockIdx.y * 8 + tid] = buf[tid];
  }
}

// launch_keccak_merkle_tree for every member: the same launches, each over the whole batch
template <u32 DOM>
static hipError_t launch_keccak_merkle_tree_batch(u32* hashes, u64 np2, u32 n_batch, u64 hashes_stride, hipStream_t st, u32* root_out) {
  if (n_batch > 65535) return hipErrorInvalidValue;          // grid.y
  if (n_batch == 0) return hipSuccess;
  u64 in_off = 0, width = np2;
  while (width > 1) {
    u32 lw = 0;
    while (((u64)1 << lw) < width) lw++;
    const u32 lsub = lw < 9 ? lw : 9;
    const u64 nwg = width >> lsub;
    hipLaunchKernelGGL(sha3_merkle_subtree_batch_kernel<DOM>, dim3((unsigned)nwg, n_batch), dim3(256), 0, st, hashes, in_off, width, lsub,
                       lsub == lw ? root_out : (u32*)nullptr, hashes_stride);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    for (u32 j = 0; j < lsub; j++) { in_off += width; width >>= 1; }
  }
  return hipSuccess;
}
hipError_t launch_sha3_merkle_tree_batch(u32* hashes, u64 np2, u32 n_batch, u64 hashes_stride, hipStream_t st, u32* root_out) {
  return launch_keccak_merkle_tree_batch<kc::KC_DOM_SHA3>(hashes, np2, n_batch, hashes_stride, st, root_out);
}
hipError_t launch_keccak256_merkle_tree_batch(u32* hashes, u64 np2, u32 n_batch, u64 hashes_stride, hipStream_t st, u32* root_out) {
  return launch_keccak_merkle_tree_batch<kc::KC_DOM_KECCAK>(hashes, np2, n_batch, hashes_stride, st, root_out);
}

}  // namespace lcpc

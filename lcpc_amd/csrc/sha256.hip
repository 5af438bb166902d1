// lcpc_amd/csrc/sha256.hip -- SHA-256 column hash and Merkle tree (LcCommit<Sha256, E>) for gfx950.
//
//   leaf[c] = SHA-256(0^32 || to_repr(comm[0][c]) || ... || to_repr(comm[R-1][c]))   (lcpc-2d lib.rs:719-735)
//   node    = SHA-256(left || right)                                                (lib.rs:770-775)
//
// The leaf message is 4 + L R little-endian 64-bit words, one canonical limb each; a 64-byte block is 8 of them: word k goes into
// words 2 (k mod 8), 2 (k mod 8) + 1 of block k / 8, each half byte-swapped (SHA-256 reads big-endian 32-bit words).  As for SHA3
// and BLAKE2b the hash is one serial chain per column, so the grid is one lane per column.  L blocks (8 L words) hold exactly 8
// elements, so the kernel walks the message in groups of L blocks whose word -> (row, limb) map is a compile-time table.
// Padding: the byte 0x80, zeros, the bit length as a big-endian 64-bit word at the end of a block.  With q = (4 + L R) mod 8 words
// in the block that holds the end of the message, 0x80 opens word q and the length is word 7 of the same block -- except q = 7,
// where the length takes one more block; q = 0 is a block of padding alone.
#include "kernels.h"
#include "field_ln.h"
#include "sha256_dev.h"

namespace lcpc {

constexpr int s2_fdiv(int a, int b) { return a >= 0 ? a / b : -((-a + b - 1) / b); }

// the message of block B (0 <= B < L) of the group starting at row 8 j: words 8 B .. 8 B + 7 of the group, word w of the group
// being limb (w - 4) mod L of row 8 j + (w - 4) div L
template <int NL, bool CANON, int B>
__device__ __forceinline__ void s2_load_block(u32 m[16], const LeafArgs& a, u64 col, int64_t row_g) {
  constexpr int L = NL / 2;
  constexpr int X0 = s2_fdiv(8 * B - 4, L), X1 = s2_fdiv(8 * B + 3, L), NE = X1 - X0 + 1;
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
  for (int p = 0; p < 8; p++) {
    const int w = 8 * B + p - 4;
    const int x = s2_fdiv(w, L), l = w - x * L;
    m[2 * p] = s256::bswap(el[x - X0].v[2 * l]);
    m[2 * p + 1] = s256::bswap(el[x - X0].v[2 * l + 1]);
  }
}

template <int NL, bool CANON, int B>
__device__ __forceinline__ void s2_group_step(u32 h[8], const LeafArgs& a, u64 col, u64 j, u64 n_words, u64 n_blocks) {
  constexpr int L = NL / 2;
  const u64 blk = j * L + B;
  if (blk >= n_blocks) return;
  u32 m[16];
  s2_load_block<NL, CANON, B>(m, a, col, (int64_t)(8 * j));
  if (blk == n_words / 8) {
    // the block that holds the end of the message: the message is whole words, so the 0x80 byte is the first byte of word
    // n_words - 8 blk, i.e. the top byte of its first big-endian half (that word is zero so far)
    const u32 q = (u32)(n_words - 8 * blk);
#pragma unroll
    for (u32 p = 0; p < 8; p++) m[2 * p] |= (p == q) ? 0x80000000u : 0u;
  }
  if (blk + 1 == n_blocks) {
    const u64 bits = 64 * n_words;
    m[14] = (u32)(bits >> 32);
    m[15] = (u32)bits;
  }
  s256::compress(h, m);
  if constexpr (B + 1 < L) s2_group_step<NL, CANON, B + 1>(h, a, col, j, n_words, n_blocks);
}

template <int NL, bool CANON>
__global__ void __launch_bounds__(256) sha256_leaf_kernel(LeafArgs a) {
  const u64 col = (u64)blockIdx.x * 256 + threadIdx.x;
  if (col >= a.n_cols) return;
  constexpr int L = NL / 2;
  const u64 n_words = 4 + (u64)L * a.n_rows_total;
  const u64 n_blocks = n_words / 8 + 1 + ((n_words & 7) == 7 ? 1 : 0);   // 0x80 and the length need two words
  u32 h[8];
  s256::init(h);
  for (u64 j = 0; j * L < n_blocks; j++) s2_group_step<NL, CANON, 0>(h, a, col, j, n_words, n_blocks);
  u32* o = a.out + col * 8;
  *reinterpret_cast<uint4*>(o) = make_uint4(s256::bswap(h[0]), s256::bswap(h[1]), s256::bswap(h[2]), s256::bswap(h[3]));
  *reinterpret_cast<uint4*>(o + 4) = make_uint4(s256::bswap(h[4]), s256::bswap(h[5]), s256::bswap(h[6]), s256::bswap(h[7]));
}

hipError_t launch_sha256_leaves(int nl, const LeafArgs& a, hipStream_t st) {
  if (a.n_cols == 0) return hipSuccess;
  const dim3 grid((unsigned)((a.n_cols + 255) / 256));
#define S2_CASE(NLV)                                                                                            \
  case NLV:                                                                                                     \
    if (a.canon_in) hipLaunchKernelGGL((sha256_leaf_kernel<NLV, true>), grid, dim3(256), 0, st, a);          \
    else hipLaunchKernelGGL((sha256_leaf_kernel<NLV, false>), grid, dim3(256), 0, st, a);                    \
    break;
  switch (nl) {
    S2_CASE(2) S2_CASE(4) S2_CASE(6) S2_CASE(8)
    default: return hipErrorInvalidValue;
  }
#undef S2_CASE
  return hipGetLastError();
}

// ---- the batch form (kernels.h: launch_sha256_leaves_batch; batch.cpp) ----
// sha256_leaf_kernel for n_batch equal-shape members of one encoder, the member index blockIdx.y: the same chain per column on
// member i's comm and out, which start i * comm_stride / i * out_stride words behind member 0's
// (The second launch bound is the one-shot twin's occupancy in waves per SIMD: without it the register allocator spreads the same
// instruction stream over twice the VGPRs.)
template <int NL, bool CANON>
__global__ void __launch_bounds__(256, (NL == 6 && !CANON) ? 7 : 8) sha256_leaf_batch_kernel(LeafArgs a, u64 comm_stride, u64 out_stride) {
  const u64 col = (u64)blockIdx.x * 256 + threadIdx.x;
  if (col >= a.n_cols) return;
  a.comm += (u64)blockIdx.y * comm_stride;
  a.out += (u64)blockIdx.y * out_stride;
  constexpr int L = NL / 2;
  const u64 n_words = 4 + (u64)L * a.n_rows_total;
  const u64 n_blocks = n_words / 8 + 1 + ((n_words & 7) == 7 ? 1 : 0);
  u32 h[8];
  s256::init(h);
  for (u64 j = 0; j * L < n_blocks; j++) s2_group_step<NL, CANON, 0>(h, a, col, j, n_words, n_blocks);
  u32* o = a.out + col * 8;
  *reinterpret_cast<uint4*>(o) = make_uint4(s256::bswap(h[0]), s256::bswap(h[1]), s256::bswap(h[2]), s256::bswap(h[3]));
  *reinterpret_cast<uint4*>(o + 4) = make_uint4(s256::bswap(h[4]), s256::bswap(h[5]), s256::bswap(h[6]), s256::bswap(h[7]));
}

hipError_t launch_sha256_leaves_batch(int nl, const LeafArgs& a, u32 n_batch, u64 comm_stride, u64 out_stride, hipStream_t st) {
  if (n_batch > 65535) return hipErrorInvalidValue;          // grid.y
  if (nl != 2 && nl != 4 && nl != 6 && nl != 8) return hipErrorInvalidValue;
  if (nl == 8 && !a.canon_in) return hipErrorInvalidValue;   // Ft255's Ligero comm is canonical: the other form has no batch user
  if (a.n_cols == 0 || n_batch == 0) return hipSuccess;
  const dim3 grid((unsigned)((a.n_cols + 255) / 256), n_batch);
#define S2_CASE(NLV)                                                                                                                \
  case NLV:                                                                                                                         \
    if (a.canon_in) hipLaunchKernelGGL((sha256_leaf_batch_kernel<NLV, true>), grid, dim3(256), 0, st, a, comm_stride, out_stride);  \
    else hipLaunchKernelGGL((sha256_leaf_batch_kernel<NLV, false>), grid, dim3(256), 0, st, a, comm_stride, out_stride);            \
    break;
  switch (nl) {
    S2_CASE(2) S2_CASE(4) S2_CASE(6)
    case 8: hipLaunchKernelGGL((sha256_leaf_batch_kernel<8, true>), grid, dim3(256), 0, st, a, comm_stride, out_stride); break;
  }
#undef S2_CASE
  return hipGetLastError();
}

// ---- the same chain a block range at a time (kernels.h: launch_sha256_leaves_range) ----
// s2_group_step for the blocks of group j that lie in [b0, b1): a block outside the range is neither loaded nor compressed
template <int NL, bool CANON, int B>
__device__ __forceinline__ void s2_range_step(u32 h[8], const LeafArgs& a, u64 col, u64 j, u64 n_words, u64 n_blocks, u64 b0, u64 b1) {
  constexpr int L = NL / 2;
  const u64 blk = j * L + B;
  if (blk >= b0 && blk < b1) {
    u32 m[16];
    s2_load_block<NL, CANON, B>(m, a, col, (int64_t)(8 * j));
    if (blk == n_words / 8) {               // 0x80 behind the last message word, as in s2_group_step
      const u32 q = (u32)(n_words - 8 * blk);
#pragma unroll
      for (u32 p = 0; p < 8; p++) m[2 * p] |= (p == q) ? 0x80000000u : 0u;
    }
    if (blk + 1 == n_blocks) {
      const u64 bits = 64 * n_words;
      m[14] = (u32)(bits >> 32);
      m[15] = (u32)bits;
    }
    s256::compress(h, m);
  }
  if constexpr (B + 1 < L) s2_range_step<NL, CANON, B + 1>(h, a, col, j, n_words, n_blocks, b0, b1);
}

// state: word i of column c at state[i * n_cols + c] (the working h[], not byte-swapped)
template <int NL, bool CANON>
__global__ void __launch_bounds__(256) sha256_leaf_range_kernel(LeafArgs a, u64 b0, u64 b1, u32* state) {
  const u64 col = (u64)blockIdx.x * 256 + threadIdx.x;
  if (col >= a.n_cols) return;
  constexpr int L = NL / 2;
  const u64 n_words = 4 + (u64)L * a.n_rows_total;
  const u64 n_blocks = n_words / 8 + 1 + ((n_words & 7) == 7 ? 1 : 0);
  u32 h[8];
  if (b0 == 0) {
    s256::init(h);
  } else {
#pragma unroll
    for (int i = 0; i < 8; i++) h[i] = state[(u64)i * a.n_cols + col];
  }
  for (u64 j = b0 / L; j * L < b1; j++) s2_range_step<NL, CANON, 0>(h, a, col, j, n_words, n_blocks, b0, b1);
  if (b1 == n_blocks) {
    u32* o = a.out + col * 8;
    *reinterpret_cast<uint4*>(o) = make_uint4(s256::bswap(h[0]), s256::bswap(h[1]), s256::bswap(h[2]), s256::bswap(h[3]));
    *reinterpret_cast<uint4*>(o + 4) = make_uint4(s256::bswap(h[4]), s256::bswap(h[5]), s256::bswap(h[6]), s256::bswap(h[7]));
  } else {
#pragma unroll
    for (int i = 0; i < 8; i++) state[(u64)i * a.n_cols + col] = h[i];
  }
}

hipError_t launch_sha256_leaves_range(int nl, const LeafArgs& a, uint64_t b0, uint64_t b1, uint32_t* state, hipStream_t st) {
  if (nl != 2 && nl != 4 && nl != 6 && nl != 8) return hipErrorInvalidValue;
  if (b0 > b1 || b1 > sha256_leaf_blocks(nl, a.n_rows_total)) return hipErrorInvalidValue;
  if (a.n_cols == 0 || b0 == b1) return hipSuccess;
  const dim3 grid((unsigned)((a.n_cols + 255) / 256));
#define S2_CASE(NLV)                                                                                                        \
  case NLV:                                                                                                                 \
    if (a.canon_in) hipLaunchKernelGGL((sha256_leaf_range_kernel<NLV, true>), grid, dim3(256), 0, st, a, b0, b1, state);    \
    else hipLaunchKernelGGL((sha256_leaf_range_kernel<NLV, false>), grid, dim3(256), 0, st, a, b0, b1, state);              \
    break;
  switch (nl) { S2_CASE(2) S2_CASE(4) S2_CASE(6) S2_CASE(8) }
#undef S2_CASE
  return hipGetLastError();
}

// parent = SHA-256(left || right): 64 message bytes are one block, the padding a second one that is the same for every node
__device__ __forceinline__ void sha256_node(u32 o[8], const u32* l, const u32* r) {
  u32 m[16], h[8];
#pragma unroll
  for (int i = 0; i < 8; i++) { m[i] = s256::bswap(l[i]); m[8 + i] = s256::bswap(r[i]); }
  s256::init(h);
  s256::compress(h, m);
  s256::compress_pad64(h);
#pragma unroll
  for (int i = 0; i < 8; i++) o[i] = s256::bswap(h[i]);
}

// the counterpart of sha3_merkle_subtree_kernel (sha3.hip): each workgroup folds 2^lsub consecutive nodes of a level `lsub` levels
// up through LDS, one node per lane, writing every level to its slot of the flat `hashes` array (lib.rs:656-666, 747-760)
__global__ void __launch_bounds__(256) sha256_merkle_subtree_kernel(u32* hashes, u64 in_off, u64 width, u32 lsub, u32* root_out) {
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
    sha256_node(o, l, r);
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
    if (act) sha256_node(o, buf + 2 * tid * 8, buf + (2 * tid + 1) * 8);
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

hipError_t launch_sha256_merkle_tree(u32* hashes, u64 np2, hipStream_t st, u32* root_out) {
  u64 in_off = 0, width = np2;
  while (width > 1) {
    u32 lw = 0;
    while (((u64)1 << lw) < width) lw++;
    const u32 lsub = lw < 9 ? lw : 9;
    const u64 nwg = width >> lsub;
    hipLaunchKernelGGL(sha256_merkle_subtree_kernel, dim3((unsigned)nwg), dim3(256), 0, st, hashes, in_off, width, lsub,
                       lsub == lw ? root_out : (u32*)nullptr);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    for (u32 j = 0; j < lsub; j++) { in_off += width; width >>= 1; }
  }
  return hipSuccess;
}


// sha256_merkle_subtree_kernel per member (blockIdx.y): member i's hashes start i * hashes_stride words behind member 0's; root_out
// (may be null): [n_batch][8], member i's root at root_out + 8 i
__global__ void __launch_bounds__(256) sha256_merkle_subtree_batch_kernel(u32* hashes, u64 in_off, u64 width, u32 lsub, u32* root_out,
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
    sha256_node(o, l, r);
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
    if (act) sha256_node(o, buf + 2 * tid * 8, buf + (2 * tid + 1) * 8);
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

// launch_sha256_merkle_tree for every member: the same launches, each over the whole batch
hipError_t launch_sha256_merkle_tree_batch(u32* hashes, u64 np2, u32 n_batch, u64 hashes_stride, hipStream_t st, u32* root_out) {
  if (n_batch > 65535) return hipErrorInvalidValue;          // grid.y
  if (n_batch == 0) return hipSuccess;
  u64 in_off = 0, width = np2;
  while (width > 1) {
    u32 lw = 0;
    while (((u64)1 << lw) < width) lw++;
    const u32 lsub = lw < 9 ? lw : 9;
    const u64 nwg = width >> lsub;
    hipLaunchKernelGGL(sha256_merkle_subtree_batch_kernel, dim3((unsigned)nwg, n_batch), dim3(256), 0, st, hashes, in_off, width, lsub,
                       lsub == lw ? root_out : (u32*)nullptr, hashes_stride);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    for (u32 j = 0; j < lsub; j++) { in_off += width; width >>= 1; }
  }
  return hipSuccess;
}

}  // namespace lcpc

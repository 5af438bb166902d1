// lcpc_amd/csrc/blake2b.hip -- BLAKE2b-512 column hash, Merkle tree and path gather (LcCommit<Blake2b, E>) for gfx950.
//
//   leaf[c] = BLAKE2b(0^64 || to_repr(comm[0][c]) || ... || to_repr(comm[R-1][c]))   (lcpc-2d lib.rs:719-735)
//   node    = BLAKE2b(left || right)                                                (lib.rs:770-775)
//
// Output<Blake2b>::default() is 64 zero bytes, so the leaf message is 8 + L R little-endian 64-bit words, one canonical limb
// each, and every word is one BLAKE2b message word: word k goes into word k mod 16 of block k / 16.  As for SHA3 the hash is one
// serial chain per column, so the grid is one lane per column.  L blocks (16 L words) hold exactly 16 elements, so the kernel walks
// the message in groups of L blocks whose word -> (row, limb) map is a compile-time table.  A message that fills its last block
// exactly gets no extra block: the final compression is the full last block with t = the message length and f0 = ~0.
// Digests are 64 bytes = 16 u32 words: LcCommit.hashes is [2 np2 - 1][16] words for a BLAKE2b encoder.
#include "kernels.h"
#include "field_ln.h"
#include "blake2b_dev.h"

namespace lcpc {

constexpr int b2_fdiv(int a, int b) { return a >= 0 ? a / b : -((-a + b - 1) / b); }

// the message of block B (0 <= B < L) of the group starting at row 16 j: words 16 B .. 16 B + 15 of the group, word w of the
// group being limb (w - 8) mod L of row 16 j + (w - 8) div L
template <int NL, bool CANON, int B>
__device__ __forceinline__ void b2_load_block(uint64_t m[16], const LeafArgs& a, u64 col, int64_t row_g) {
  constexpr int L = NL / 2;
  constexpr int X0 = b2_fdiv(16 * B - 8, L), X1 = b2_fdiv(16 * B + 7, L), NE = X1 - X0 + 1;
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
      el[x] = fe_zero<NL>();       // the 64-byte zero prefix (rows < 0) and the zero words past the message
    }
  }
#pragma unroll
  for (int p = 0; p < 16; p++) {
    const int w = 16 * B + p - 8;
    const int x = b2_fdiv(w, L), l = w - x * L;
    m[p] = b2b::pack(el[x - X0].v[2 * l], el[x - X0].v[2 * l + 1]);
  }
}

template <int NL, bool CANON, int B>
__device__ __forceinline__ void b2_group_step(uint64_t h[8], const LeafArgs& a, u64 col, u64 j, u64 n_words, u64 n_blocks) {
  constexpr int L = NL / 2;
  const u64 blk = j * L + B;
  if (blk >= n_blocks) return;
  uint64_t m[16];
  b2_load_block<NL, CANON, B>(m, a, col, (int64_t)(16 * j));
  const bool last = blk + 1 == n_blocks;
  b2b::compress(h, m, last ? 8 * n_words : 128 * (blk + 1), last);
  if constexpr (B + 1 < L) b2_group_step<NL, CANON, B + 1>(h, a, col, j, n_words, n_blocks);
}

__device__ __forceinline__ void b2_store(u32* o, const uint64_t h[8]) {
#pragma unroll
  for (int i = 0; i < 8; i += 2)
    *reinterpret_cast<uint4*>(o + 2 * i) = make_uint4(b2b::lo32(h[i]), b2b::hi32(h[i]), b2b::lo32(h[i + 1]), b2b::hi32(h[i + 1]));
}

template <int NL, bool CANON>
__global__ void __launch_bounds__(256) blake2b_leaf_kernel(LeafArgs a) {
  const u64 col = (u64)blockIdx.x * 256 + threadIdx.x;
  if (col >= a.n_cols) return;
  constexpr int L = NL / 2;
  const u64 n_words = 8 + (u64)L * a.n_rows_total;
  const u64 n_blocks = (n_words + 15) / 16;       // no padding block: a message of 16 k words ends on a full block
  uint64_t h[8];
  b2b::init(h);
  for (u64 j = 0; j * L < n_blocks; j++) b2_group_step<NL, CANON, 0>(h, a, col, j, n_words, n_blocks);
  b2_store(a.out + col * 16, h);
}

hipError_t launch_blake2b_leaves(int nl, const LeafArgs& a, hipStream_t st) {
  if (a.n_cols == 0) return hipSuccess;
  const dim3 grid((unsigned)((a.n_cols + 255) / 256));
#define B2_CASE(NLV)                                                                                            \
  case NLV:                                                                                                     \
    if (a.canon_in) hipLaunchKernelGGL((blake2b_leaf_kernel<NLV, true>), grid, dim3(256), 0, st, a);         \
    else hipLaunchKernelGGL((blake2b_leaf_kernel<NLV, false>), grid, dim3(256), 0, st, a);                   \
    break;
  switch (nl) {
    B2_CASE(2) B2_CASE(4) B2_CASE(6) B2_CASE(8)
    default: return hipErrorInvalidValue;
  }
#undef B2_CASE
  return hipGetLastError();
}

// ---- the batch form (kernels.h: launch_blake2b_leaves_batch; batch.cpp) ----
// blake2b_leaf_kernel for n_batch equal-shape members of one encoder, the member index blockIdx.y: the same chain per column on
// member i's comm and out, which start i * comm_stride / i * out_stride words behind member 0's
// (No occupancy bound: held to the one-shot twin's 5 / 4 waves per SIMD the register allocator spills 36 .. 116 bytes per lane; left
// alone it takes 116 .. 136 VGPRs -- one wave per SIMD fewer -- and no scratch.)
template <int NL, bool CANON>
__global__ void __launch_bounds__(256) blake2b_leaf_batch_kernel(LeafArgs a, u64 comm_stride, u64 out_stride) {
  const u64 col = (u64)blockIdx.x * 256 + threadIdx.x;
  if (col >= a.n_cols) return;
  a.comm += (u64)blockIdx.y * comm_stride;
  a.out += (u64)blockIdx.y * out_stride;
  constexpr int L = NL / 2;
  const u64 n_words = 8 + (u64)L * a.n_rows_total;
  const u64 n_blocks = (n_words + 15) / 16;
  uint64_t h[8];
  b2b::init(h);
  for (u64 j = 0; j * L < n_blocks; j++) b2_group_step<NL, CANON, 0>(h, a, col, j, n_words, n_blocks);
  b2_store(a.out + col * 16, h);
}

hipError_t launch_blake2b_leaves_batch(int nl, const LeafArgs& a, u32 n_batch, u64 comm_stride, u64 out_stride, hipStream_t st) {
  if (n_batch > 65535) return hipErrorInvalidValue;          // grid.y
  if (nl != 2 && nl != 4 && nl != 6 && nl != 8) return hipErrorInvalidValue;
  if (nl == 8 && !a.canon_in) return hipErrorInvalidValue;   // Ft255's Ligero comm is canonical: the other form has no batch user
  if (a.n_cols == 0 || n_batch == 0) return hipSuccess;
  const dim3 grid((unsigned)((a.n_cols + 255) / 256), n_batch);
#define B2_CASE(NLV)                                                                                                                \
  case NLV:                                                                                                                         \
    if (a.canon_in) hipLaunchKernelGGL((blake2b_leaf_batch_kernel<NLV, true>), grid, dim3(256), 0, st, a, comm_stride, out_stride); \
    else hipLaunchKernelGGL((blake2b_leaf_batch_kernel<NLV, false>), grid, dim3(256), 0, st, a, comm_stride, out_stride);           \
    break;
  switch (nl) {
    B2_CASE(2) B2_CASE(4) B2_CASE(6)
    case 8: hipLaunchKernelGGL((blake2b_leaf_batch_kernel<8, true>), grid, dim3(256), 0, st, a, comm_stride, out_stride); break;
  }
#undef B2_CASE
  return hipGetLastError();
}

// ---- the same chain a block range at a time (kernels.h: launch_blake2b_leaves_range) ----
// b2_group_step for the blocks of group j that lie in [b0, b1): a block outside the range is neither loaded nor compressed.  The byte
// counter of a block that is not the last is 128 (blk + 1), so the chaining value is all a later launch needs
template <int NL, bool CANON, int B>
__device__ __forceinline__ void b2_range_step(uint64_t h[8], const LeafArgs& a, u64 col, u64 j, u64 n_words, u64 n_blocks, u64 b0, u64 b1) {
  constexpr int L = NL / 2;
  const u64 blk = j * L + B;
  if (blk >= b0 && blk < b1) {
    uint64_t m[16];
    b2_load_block<NL, CANON, B>(m, a, col, (int64_t)(16 * j));
    const bool last = blk + 1 == n_blocks;
    b2b::compress(h, m, last ? 8 * n_words : 128 * (blk + 1), last);
  }
  if constexpr (B + 1 < L) b2_range_step<NL, CANON, B + 1>(h, a, col, j, n_words, n_blocks, b0, b1);
}

// state: word i of column c at state[i * n_cols + c]
template <int NL, bool CANON>
__global__ void __launch_bounds__(256) blake2b_leaf_range_kernel(LeafArgs a, u64 b0, u64 b1, uint64_t* state) {
  const u64 col = (u64)blockIdx.x * 256 + threadIdx.x;
  if (col >= a.n_cols) return;
  constexpr int L = NL / 2;
  const u64 n_words = 8 + (u64)L * a.n_rows_total;
  const u64 n_blocks = (n_words + 15) / 16;
  uint64_t h[8];
  if (b0 == 0) {
    b2b::init(h);
  } else {
#pragma unroll
    for (int i = 0; i < 8; i++) h[i] = state[(u64)i * a.n_cols + col];
  }
  for (u64 j = b0 / L; j * L < b1; j++) b2_range_step<NL, CANON, 0>(h, a, col, j, n_words, n_blocks, b0, b1);
  if (b1 == n_blocks) {
    b2_store(a.out + col * 16, h);
  } else {
#pragma unroll
    for (int i = 0; i < 8; i++) state[(u64)i * a.n_cols + col] = h[i];
  }
}

hipError_t launch_blake2b_leaves_range(int nl, const LeafArgs& a, uint64_t b0, uint64_t b1, uint64_t* state, hipStream_t st) {
  if (nl != 2 && nl != 4 && nl != 6 && nl != 8) return hipErrorInvalidValue;
  if (b0 > b1 || b1 > blake2b_leaf_blocks(nl, a.n_rows_total)) return hipErrorInvalidValue;
  if (a.n_cols == 0 || b0 == b1) return hipSuccess;
  const dim3 grid((unsigned)((a.n_cols + 255) / 256));
#define B2_CASE(NLV)                                                                                                        \
  case NLV:                                                                                                                 \
    if (a.canon_in) hipLaunchKernelGGL((blake2b_leaf_range_kernel<NLV, true>), grid, dim3(256), 0, st, a, b0, b1, state);   \
    else hipLaunchKernelGGL((blake2b_leaf_range_kernel<NLV, false>), grid, dim3(256), 0, st, a, b0, b1, state);             \
    break;
  switch (nl) { B2_CASE(2) B2_CASE(4) B2_CASE(6) B2_CASE(8) }
#undef B2_CASE
  return hipGetLastError();
}

// parent = BLAKE2b(left || right): 16 words, one compression with t = 128 and the last-block flag
__device__ __forceinline__ void blake2b_node(u32 o[16], const u32* l, const u32* r) {
  uint64_t m[16], h[8];
#pragma unroll
  for (int i = 0; i < 8; i++) { m[i] = b2b::pack(l[2 * i], l[2 * i + 1]); m[8 + i] = b2b::pack(r[2 * i], r[2 * i + 1]); }
  b2b::init(h);
  b2b::compress(h, m, 128, true);
#pragma unroll
  for (int i = 0; i < 8; i++) { o[2 * i] = b2b::lo32(h[i]); o[2 * i + 1] = b2b::hi32(h[i]); }
}

// the counterpart of sha3_merkle_subtree_kernel (sha3.hip) with 16-word nodes: each workgroup folds 2^lsub consecutive nodes of a
// level `lsub` levels up through LDS, one node per lane, writing every level to its slot of the flat `hashes` array
// (lib.rs:656-666, 747-760)
__global__ void __launch_bounds__(256) blake2b_merkle_subtree_kernel(u32* hashes, u64 in_off, u64 width, u32 lsub, u32* root_out) {
  __shared__ u32 buf[256 * 16];
  const u32 tid = threadIdx.x;
  const u64 base = (u64)blockIdx.x << lsub;
  u64 layer_in = in_off, w = width, layer_out = in_off + width;
  u32 n_out = 1u << (lsub - 1);
  u32 o[16];
  if (tid < n_out) {
    const u32* gl = hashes + (layer_in + base + 2 * tid) * 16;
    u32 l[16], r[16];
#pragma unroll
    for (int i = 0; i < 16; i++) { l[i] = gl[i]; r[i] = gl[16 + i]; }
    blake2b_node(o, l, r);
    u32* d = hashes + (layer_out + (base >> 1) + tid) * 16;
#pragma unroll
    for (int i = 0; i < 16; i++) { d[i] = o[i]; buf[tid * 16 + i] = o[i]; }
  }
  for (u32 j = 2; j <= lsub; j++) {
    __syncthreads();
    layer_in = layer_out;
    w >>= 1;
    layer_out = layer_in + w;
    n_out >>= 1;
    const bool act = tid < n_out;
    if (act) blake2b_node(o, buf + 2 * tid * 16, buf + (2 * tid + 1) * 16);
    __syncthreads();
    if (act) {
      u32* d = hashes + (layer_out + (base >> j) + tid) * 16;
#pragma unroll
      for (int i = 0; i < 16; i++) { d[i] = o[i]; buf[tid * 16 + i] = o[i]; }
    }
  }
  if (root_out != nullptr) {
    __syncthreads();
    if (tid < 16) root_out[tid] = buf[tid];
  }
}

hipError_t launch_blake2b_merkle_tree(u32* hashes, u64 np2, hipStream_t st, u32* root_out) {
  u64 in_off = 0, width = np2;
  while (width > 1) {
    u32 lw = 0;
    while (((u64)1 << lw) < width) lw++;
    const u32 lsub = lw < 9 ? lw : 9;
    const u64 nwg = width >> lsub;
    hipLaunchKernelGGL(blake2b_merkle_subtree_kernel, dim3((unsigned)nwg), dim3(256), 0, st, hashes, in_off, width, lsub,
                       lsub == lw ? root_out : (u32*)nullptr);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    for (u32 j = 0; j < lsub; j++) { in_off += width; width >>= 1; }
  }
  return hipSuccess;
}

// blake2b_merkle_subtree_kernel per member (blockIdx.y): member i's hashes start i * hashes_stride words behind member 0's; root_out
// (may be null): [n_batch][16], member i's root at root_out + 16 i
__global__ void __launch_bounds__(256) blake2b_merkle_subtree_batch_kernel(u32* hashes, u64 in_off, u64 width, u32 lsub, u32* root_out,
                                                                           u64 hashes_stride) {
  __shared__ u32 buf[256 * 16];
  hashes += (u64)blockIdx.y * hashes_stride;
  const u32 tid = threadIdx.x;
  const u64 base = (u64)blockIdx.x << lsub;
  u64 layer_in = in_off, w = width, layer_out = in_off + width;
  u32 n_out = 1u << (lsub - 1);
  u32 o[16];
  if (tid < n_out) {
    const u32* gl = hashes + (layer_in + base + 2 * tid) * 16;
    u32 l[16], r[16];
#pragma unroll
    for (int i = 0; i < 16; i++) { l[i] = gl[i]; r[i] = gl[16 + i]; }
    blake2b_node(o, l, r);
    u32* d = hashes + (layer_out + (base >> 1) + tid) * 16;
#pragma unroll
    for (int i = 0; i < 16; i++) { d[i] = o[i]; buf[tid * 16 + i] = o[i]; }
  }
  for (u32 j = 2; j <= lsub; j++) {
    __syncthreads();
    layer_in = layer_out;
    w >>= 1;
    layer_out = layer_in + w;
    n_out >>= 1;
    const bool act = tid < n_out;
    if (act) blake2b_node(o, buf + 2 * tid * 16, buf + (2 * tid + 1) * 16);
    __syncthreads();
    if (act) {
      u32* d = hashes + (layer_out + (base >> j) + tid) * 16;
#pragma unroll
      for (int i = 0; i < 16; i++) { d[i] = o[i]; buf[tid * 16 + i] = o[i]; }
    }
  }
  if (root_out != nullptr) {
    __syncthreads();
    if (tid < 16) root_out[(u64)blockIdx.y * 16 + tid] = buf[tid];
  }
}

// launch_blake2b_merkle_tree for every member: the same launches, each over the whole batch
hipError_t launch_blake2b_merkle_tree_batch(u32* hashes, u64 np2, u32 n_batch, u64 hashes_stride, hipStream_t st, u32* root_out) {
  if (n_batch > 65535) return hipErrorInvalidValue;          // grid.y
  if (n_batch == 0) return hipSuccess;
  u64 in_off = 0, width = np2;
  while (width > 1) {
    u32 lw = 0;
    while (((u64)1 << lw) < width) lw++;
    const u32 lsub = lw < 9 ? lw : 9;
    const u64 nwg = width >> lsub;
    hipLaunchKernelGGL(blake2b_merkle_subtree_batch_kernel, dim3((unsigned)nwg, n_batch), dim3(256), 0, st, hashes, in_off, width, lsub,
                       lsub == lw ? root_out : (u32*)nullptr, hashes_stride);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    for (u32 j = 0; j < lsub; j++) { in_off += width; width >>= 1; }
  }
  return hipSuccess;
}

// open_column's paths for 64-byte digests: paths[k][lvl] = the sibling of column cols[k] at level lvl (gather_paths_kernel of
// kernels.hip with 16-word entries)
__global__ void __launch_bounds__(256) blake2b_gather_paths_kernel(const u32* hashes, u64 np2, u32 path_len, const u64* cols, u32 n,
                                                                   u32* paths) {
  const u64 id = (u64)blockIdx.x * 256 + threadIdx.x;
  if (id >= (u64)n * path_len) return;
  const u32 k = (u32)(id / path_len), lvl = (u32)(id % path_len);
  u64 base = 0, w = np2;
  for (u32 i = 0; i < lvl; i++) { base += w; w >>= 1; }
  const u64 node = (cols[k] >> lvl) ^ 1;
  const uint4* s = reinterpret_cast<const uint4*>(hashes + (base + node) * 16);
  uint4* d = reinterpret_cast<uint4*>(paths + id * 16);
#pragma unroll
  for (int i = 0; i < 4; i++) d[i] = s[i];
}

hipError_t launch_blake2b_gather_paths(const u32* hashes, u64 np2, u32 path_len, const u64* cols, u32 n, u32* paths, hipStream_t st) {
  const u64 tot = (u64)n * path_len;
  if (tot == 0) return hipSuccess;
  hipLaunchKernelGGL(blake2b_gather_paths_kernel, dim3((unsigned)((tot + 255) / 256)), dim3(256), 0, st, hashes, np2, path_len, cols, n,
                     paths);
  return hipGetLastError();
}

}  // namespace lcpc

// lcpc_amd/csrc/batch_kernels.hip -- gfx950 kernels of the batched commit (batch.cpp, include/lcpc_hip_batch.h): the BLAKE3 batch forms
// of leaf_chunk_kernel, leaf_tree_kernel, leaf_finish_kernel and merkle_subtree_kernel (kernels.hip), and the placement of strided /
// ragged polynomials into the padded coeffs rows (every digest).  The batch forms of the SHA3-256 / Keccak-256 / SHA-256 / BLAKE2b
// leaf and subtree kernels are chain_dev.h's.
// Launchers: kernels.h.
#include "kernels.h"
#include "field_dev.h"
#include "blake3_dev.h"
#include "leaf_dev.h"
#include "fold_dev.h"

namespace lcpc {

// =================================================================================================
// K3b / K4b: the column hash and the tree of a BATCH of equal-shape commitments of one encoder (batch.cpp).  Each kernel is its
// namesake of kernels.hip (K3 / K4) with the member index as one more grid dimension: member i's comm, chaining values and hashes sit at a fixed
// word stride behind member 0's, and the per-member work is the same code on shifted pointers -- so one launch holds n_batch
// times as many workgroups, where a small commitment's own launch leaves most of the chip idle.  Digests are bit for bit those of
// the single kernels (the lane-per-column and the quad form of a chunk give the same chaining value).
// =================================================================================================
template <int NL, bool CANON, bool QUAD>
__global__ void __launch_bounds__(256) leaf_chunk_batch_kernel(LeafArgs a, u64 comm_stride, u64 out_stride) {
  const u64 col = QUAD ? (u64)blockIdx.x * 64 + (threadIdx.x >> 2) : (u64)blockIdx.x * 256 + threadIdx.x;
  const u32 q = threadIdx.x & 3u;
  if (col >= a.n_cols) return;
  a.comm += (u64)blockIdx.z * comm_stride;
  const u32 chunk = a.chunk_begin + blockIdx.y;
  u32 cv[8];
  u32 cv_lo, cv_hi;
  leaf_chunk_cv<NL, CANON, QUAD>(a, col, chunk, q, cv, cv_lo, cv_hi);
  u32* o = a.out + (u64)blockIdx.z * out_stride + ((u64)blockIdx.y * a.n_cols + col) * 8;
  if constexpr (QUAD) {
    o[q] = cv_lo;
    o[4 + q] = cv_hi;
  } else {
    *reinterpret_cast<uint4*>(o) = make_uint4(cv[0], cv[1], cv[2], cv[3]);
    *reinterpret_cast<uint4*>(o + 4) = make_uint4(cv[4], cv[5], cv[6], cv[7]);
  }
}
template <int NL> static void launch_leaf_chunks_batch_nl(const LeafArgs& a, u32 n_batch, u64 comm_stride, u64 out_stride, hipStream_t st) {
  // Four lanes per column (latency) while the WHOLE BATCH has few (column, chunk) pairs, one lane per column (throughput) above.
  // launch_leaf_chunks_nl's threshold was measured on single commits; counting the pairs of all members against the same number
  // is an assumption that no measurement backs yet (tools/bench_batch.py is where to check it).  A batch may therefore run the
  // other form of the kernel than a single commit of its shape does -- both give the same chaining values.
  const bool quad = (u64)a.n_cols * a.n_chunks_local * n_batch <= 65536;
  const dim3 grid((unsigned)((a.n_cols + (quad ? 63 : 255)) / (quad ? 64 : 256)), a.n_chunks_local, n_batch);
  if (a.canon_in) {
    if (quad) hipLaunchKernelGGL((leaf_chunk_batch_kernel<NL, true, true>), grid, dim3(256), 0, st, a, comm_stride, out_stride);
    else hipLaunchKernelGGL((leaf_chunk_batch_kernel<NL, true, false>), grid, dim3(256), 0, st, a, comm_stride, out_stride);
  } else {
    if (quad) hipLaunchKernelGGL((leaf_chunk_batch_kernel<NL, false, true>), grid, dim3(256), 0, st, a, comm_stride, out_stride);
    else hipLaunchKernelGGL((leaf_chunk_batch_kernel<NL, false, false>), grid, dim3(256), 0, st, a, comm_stride, out_stride);
  }
}
hipError_t launch_leaf_chunks_batch(int nl, const LeafArgs& a, u32 n_batch, u64 comm_stride, u64 out_stride, hipStream_t st) {
  if (a.n_chunks_local == 0 || a.n_cols == 0 || n_batch == 0) return hipSuccess;
  if (n_batch > 65535) return hipErrorInvalidValue;          // grid.z
  constexpr u32 SLICE = 32768;                               // grid.y, as in launch_leaf_chunks
  for (u32 s0 = 0; s0 < a.n_chunks_local; s0 += SLICE) {
    LeafArgs b = a;
    b.chunk_begin = a.chunk_begin + s0;
    b.n_chunks_local = a.n_chunks_local - s0 < SLICE ? a.n_chunks_local - s0 : SLICE;
    b.out = a.out + (u64)s0 * a.n_cols * 8;
    switch (nl) {
      case 2: launch_leaf_chunks_batch_nl<2>(b, n_batch, comm_stride, out_stride, st); break;
      case 4: launch_leaf_chunks_batch_nl<4>(b, n_batch, comm_stride, out_stride, st); break;
      case 6: launch_leaf_chunks_batch_nl<6>(b, n_batch, comm_stride, out_stride, st); break;
      case 8: launch_leaf_chunks_batch_nl<8>(b, n_batch, comm_stride, out_stride, st); break;
      default: return hipErrorInvalidValue;
    }
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
  }
  return hipSuccess;
}

// leaf_tree_kernel per member (blockIdx.y): leaf digests and the first six tree levels of every member in one launch
template <int NL, bool CANON>
__global__ void __launch_bounds__(256) leaf_tree_batch_kernel(LeafArgs a, u32* hashes, u64 np2, u64 comm_stride, u64 hashes_stride) {
  __shared__ u32 buf[64 * 8];
  a.comm += (u64)blockIdx.y * comm_stride;
  hashes += (u64)blockIdx.y * hashes_stride;
  const u32 tid = threadIdx.x, qd = tid >> 2, q = tid & 3u;
  const u64 base = (u64)blockIdx.x * 64;
  const u64 col = base + qd;
  u32 cv[8];
  u32 lo, hi;
  leaf_chunk_cv<NL, CANON, true>(a, col, 0, q, cv, lo, hi);
  if (a.n_chunks_total == 2) {
    u32 lo1, hi1, l[8], r[8];
    leaf_chunk_cv<NL, CANON, true>(a, col, 1, q, cv, lo1, hi1);
#pragma unroll
    for (int i = 0; i < 4; i++) {
      l[i] = (u32)__shfl((int)lo, i, 4); l[4 + i] = (u32)__shfl((int)hi, i, 4);
      r[i] = (u32)__shfl((int)lo1, i, 4); r[4 + i] = (u32)__shfl((int)hi1, i, 4);
    }
    b3_hash64_quad(q, lo, hi, l, r, B3_PARENT | B3_ROOT);
  }
  {
    u32* g = hashes + col * 8;
    g[q] = lo; g[4 + q] = hi;
    buf[qd * 8 + q] = lo; buf[qd * 8 + 4 + q] = hi;
  }
  constexpr u32 FL = B3_CHUNK_START | B3_CHUNK_END | B3_ROOT;
  u64 w = np2, layer_out = np2;
  u32 n_out = 32;
#pragma unroll 1
  for (u32 j = 1; j <= 6; j++) {
    __syncthreads();
    const bool act = qd < n_out;
    u32 o_lo = 0, o_hi = 0;
    if (act) {
      u32 l[8], r[8];
      ld8(l, buf + (2 * qd) * 8);
      ld8(r, buf + (2 * qd + 1) * 8);
      b3_hash64_quad(q, o_lo, o_hi, l, r, FL);
    }
    __syncthreads();
    if (act) {
      buf[qd * 8 + q] = o_lo; buf[qd * 8 + 4 + q] = o_hi;
      u32* g = hashes + (layer_out + (base >> j) + qd) * 8;
      g[q] = o_lo; g[4 + q] = o_hi;
    }
    w >>= 1;
    layer_out += w;
    n_out >>= 1;
  }
}
hipError_t launch_leaf_tree_batch(int nl, const LeafArgs& a, u32* hashes, u64 np2, u32 n_batch, u64 comm_stride, u64 hashes_stride, hipStream_t st) {
  if (!leaf_tree_supported(a, np2) || n_batch == 0 || n_batch > 65535) return hipErrorInvalidValue;
  const dim3 grid((unsigned)(a.n_cols / 64), n_batch);
#define LTB_CASE(NLV) case NLV: if (a.canon_in) hipLaunchKernelGGL((leaf_tree_batch_kernel<NLV, true>), grid, dim3(256), 0, st, a, hashes, np2, comm_stride, hashes_stride); \
                                else hipLaunchKernelGGL((leaf_tree_batch_kernel<NLV, false>), grid, dim3(256), 0, st, a, hashes, np2, comm_stride, hashes_stride); break;
  switch (nl) {
    LTB_CASE(2) LTB_CASE(4) LTB_CASE(6) LTB_CASE(8)
    default: return hipErrorInvalidValue;
  }
#undef LTB_CASE
  return hipGetLastError();
}

// leaf_finish_kernel per member (blockIdx.y), for whole leaf messages (chunk j's CV in slot j, ROOT at the top): the incremental
// stack of single chunks -- after chunk j, merge while the running chunk count is even
__global__ void __launch_bounds__(256) leaf_finish_batch_kernel(u32* cvs, u32 n_chunks, u64 n_cols, u32* out, u64 cvs_stride, u64 out_stride) {
  const u64 col = (u64)blockIdx.x * 256 + threadIdx.x;
  if (col >= n_cols) return;
  cvs += (u64)blockIdx.y * cvs_stride;
  out += (u64)blockIdx.y * out_stride;
  u32 cv[8], left[8];
  u32 len = 0;
  for (u32 j = 0; j < n_chunks; j++) {
    ld8(cv, cvs + ((u64)j * n_cols + col) * 8);
    if (j == n_chunks - 1) break;
    u64 t = (u64)j + 1;
    while ((t & 1) == 0) {
      --len;
      ld8(left, cvs + ((u64)len * n_cols + col) * 8);
      u32 o[8];
      b3_hash64(o, left, cv, B3_PARENT);
#pragma unroll
      for (int i = 0; i < 8; i++) cv[i] = o[i];
      t >>= 1;
    }
    st8(cvs + ((u64)len * n_cols + col) * 8, cv);
    ++len;
  }
  while (len > 0) {
    --len;
    ld8(left, cvs + ((u64)len * n_cols + col) * 8);
    u32 o[8];
    b3_hash64(o, left, cv, B3_PARENT | (len == 0 ? (u32)B3_ROOT : 0u));
#pragma unroll
    for (int i = 0; i < 8; i++) cv[i] = o[i];
  }
  st8(out + col * 8, cv);
}
hipError_t launch_leaf_finish_batch(u32* cvs, u32 n_chunks, u64 n_cols, u32* digests, u32 n_batch, u64 cvs_stride, u64 digests_stride, hipStream_t st) {
  if (n_chunks == 0 || n_cols == 0 || n_batch == 0 || n_batch > 65535) return hipErrorInvalidValue;
  hipLaunchKernelGGL(leaf_finish_batch_kernel, dim3((unsigned)((n_cols + 255) / 256), n_batch), dim3(256), 0, st, cvs, n_chunks, n_cols, digests,
                     cvs_stride, digests_stride);
  return hipGetLastError();
}

// merkle_subtree_kernel per member (blockIdx.y); root_out (may be null): [n_batch][8], member i's root at root_out + 8 i
template <u32 BS>
__global__ void __launch_bounds__(BS) merkle_subtree_batch_kernel(u32* hashes, u64 in_off, u64 width, u32 lsub, u32* root_out, u64 hashes_stride) {
  __shared__ u32 buf[BS * 8];
  hashes += (u64)blockIdx.y * hashes_stride;
  constexpr u32 NQ = BS / 4;
  const u32 tid = threadIdx.x;
  const u64 sub = (u64)1 << lsub;
  const u64 base = (u64)blockIdx.x * sub;
  constexpr u32 FL = B3_CHUNK_START | B3_CHUNK_END | B3_ROOT;
  u32 l[8], r[8], o[8];
  u64 layer_in = in_off, w = width;
  u64 layer_out = in_off + w;
  u32 n_out = (u32)(sub / 2);
  const u32 qd = tid >> 2, q = tid & 3u;
  u32 o_lo = 0, o_hi = 0;
  if (n_out > NQ) {
    if (tid < n_out) {
      ld8(l, hashes + (layer_in + base + 2 * tid) * 8);
      ld8(r, hashes + (layer_in + base + 2 * tid + 1) * 8);
      b3_hash64(o, l, r, FL);
      st8(hashes + (layer_out + (base >> 1) + tid) * 8, o);
      st8(buf + tid * 8, o);
    }
  } else if (qd < n_out) {
    ld8(l, hashes + (layer_in + base + 2 * qd) * 8);
    ld8(r, hashes + (layer_in + base + 2 * qd + 1) * 8);
    b3_hash64_quad(q, o_lo, o_hi, l, r, FL);
    u32* g = hashes + (layer_out + (base >> 1) + qd) * 8;
    g[q] = o_lo; g[4 + q] = o_hi;
    buf[qd * 8 + q] = o_lo; buf[qd * 8 + 4 + q] = o_hi;
  }
  for (u32 j = 2; j <= lsub; j++) {
    __syncthreads();
    layer_in = layer_out;
    w >>= 1;
    layer_out = layer_in + w;
    n_out >>= 1;
    if (n_out > NQ) {
      const bool act = tid < n_out;
      if (act) {
        ld8(l, buf + (2 * tid) * 8);
        ld8(r, buf + (2 * tid + 1) * 8);
        b3_hash64(o, l, r, FL);
      }
      __syncthreads();
      if (act) {
        st8(buf + tid * 8, o);
        st8(hashes + (layer_out + (base >> j) + tid) * 8, o);
      }
    } else {
      const bool act = qd < n_out;
      if (act) {
        ld8(l, buf + (2 * qd) * 8);
        ld8(r, buf + (2 * qd + 1) * 8);
        b3_hash64_quad(q, o_lo, o_hi, l, r, FL);
      }
      __syncthreads();
      if (act) {
        buf[qd * 8 + q] = o_lo; buf[qd * 8 + 4 + q] = o_hi;
        u32* g = hashes + (layer_out + (base >> j) + qd) * 8;
        g[q] = o_lo; g[4 + q] = o_hi;
      }
    }
  }
  if (root_out != nullptr) {
    __syncthreads();
    if (tid < 8) root_out[(u64)blockIdx.y * 8 + tid] = buf[tid];
  }
}
// launch_merkle_tree_from for every member: the same launches, each over the whole batch
hipError_t launch_merkle_tree_from_batch(u32* hashes, u64 np2, u32 levels_done, u32 n_batch, u64 hashes_stride, hipStream_t st, u32* root_out) {
  if (n_batch == 0 || n_batch > 65535) return hipErrorInvalidValue;
  u64 in_off = 0, width = np2;
  for (u32 j = 0; j < levels_done; j++) { in_off += width; width >>= 1; }
  while (width > 1) {
    u32 lw = 0;
    while (((u64)1 << lw) < width) lw++;
    if (lw <= 9) {
      hipLaunchKernelGGL(merkle_subtree_batch_kernel<1024>, dim3(1, n_batch), dim3(1024), 0, st, hashes, in_off, width, lw, root_out, hashes_stride);
      return hipGetLastError();
    }
    const u32 lsub = 9;
    const u64 nwg = width >> lsub;
    hipLaunchKernelGGL(merkle_subtree_batch_kernel<256>, dim3((unsigned)nwg, n_batch), dim3(256), 0, st, hashes, in_off, width, lsub, (u32*)nullptr,
                       hashes_stride);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    for (u32 j = 0; j < lsub; j++) { in_off += width; width >>= 1; }
  }
  return hipSuccess;
}

// K8b under BLAKE3 (kernels.h FoldPathsArgs, fold_dev.h): a tree node is the 64-byte message left || right hashed as one whole chunk, with
// the flags merkle_subtree_batch_kernel passes
struct B3Node {
  static constexpr int DIGEST_WORDS = 8;
  static __device__ __forceinline__ void node(u32 o[8], const u32* l, const u32* r) { b3_hash64(o, l, r, B3_CHUNK_START | B3_CHUNK_END | B3_ROOT); }
};
__global__ void __launch_bounds__(256) fold_paths_b3_kernel(FoldPathsArgs a) {
  fold_path_lane<B3Node>(a);
}
hipError_t launch_fold_paths_b3(const FoldPathsArgs& a, hipStream_t st) {
  const int job = fold_paths_job(a);
  if (job <= 0) return job ? hipErrorInvalidValue : hipSuccess;
  hipLaunchKernelGGL(fold_paths_b3_kernel, dim3((a.n_open + 255) / 256, a.n_batch), dim3(256), 0, st, a);
  return hipGetLastError();
}

// the polynomials of a batch into the padded coeffs rows of the slab: member i's n_valid 64-bit words from src + i * src_stride to
// dst + i * dst_stride, the rest of its dst_stride words zero (a ragged last row; poison between strided polynomials is not read)
__global__ void __launch_bounds__(256) batch_place_kernel(const uint2* src, u64 src_stride, u64 n_valid, uint2* dst, u64 dst_stride) {
  const uint2* s = src + (u64)blockIdx.y * src_stride;
  uint2* d = dst + (u64)blockIdx.y * dst_stride;
  for (u64 i = (u64)blockIdx.x * 256 + threadIdx.x; i < dst_stride; i += (u64)gridDim.x * 256)
    d[i] = i < n_valid ? s[i] : make_uint2(0u, 0u);
}
hipError_t launch_batch_place(const uint64_t* src, u64 src_stride, u64 n_valid, uint64_t* dst, u64 dst_stride, u32 n_batch, hipStream_t st) {
  if (n_batch == 0 || n_batch > 65535 || n_valid > dst_stride || n_valid > src_stride) return hipErrorInvalidValue;
  if (dst_stride == 0) return hipSuccess;
  const u64 blocks = (dst_stride + 255) / 256;
  hipLaunchKernelGGL(batch_place_kernel, dim3((unsigned)(blocks < 4096 ? blocks : 4096), n_batch), dim3(256), 0, st,
                     reinterpret_cast<const uint2*>(src), src_stride, n_valid, reinterpret_cast<uint2*>(dst), dst_stride);
  return hipGetLastError();
}

}  // namespace lcpc

// tests/native/k3_harness.cpp -- test-only C entry points over the BLAKE3 column-hash (K3), Merkle-tree (K4) and path-gather launchers of
// lcpc_amd/csrc/kernels.h and their batch forms (kernels.hip, BATCH = true), so that a test can hand a kernel a commitment matrix, a chunk range,
// a node table or a leaf layer of its own making (tests/k3_harness.py, tests/test_gpu_k3_kernels.py, tests/test_gpu_k3_batch.py).  Built by
// lcpc_amd/csrc/Makefile into lcpc_amd/lib/liblcpc_k3_harness.so and linked against the product library, which gains nothing by it.
//
// Every wrapper takes HOST pointers, checks that every index the kernel will form stays inside the buffers it was given (a refused call
// returns H_BAD_ARGS and launches nothing), allocates device buffers, copies in, launches on the null stream, synchronises, copies
// the in/out buffers back and frees.  The return value is the first hipError_t.  Buffers a kernel writes are copied in first and back
// whole, so the caller sees what was written outside the expected region too (sentinel fill).
#include <vector>

#include "harness.h"
#include "../../lcpc_amd/csrc/kernels.h"

namespace {

constexpr uint64_t MAX_DIM = (uint64_t)1 << 28;      // rows, columns, strides: far above any test, far below 64-bit overflow of a product

bool pow2(uint64_t v) { return v && !(v & (v - 1)); }
uint32_t log2u(uint64_t v) { uint32_t l = 0; while (((uint64_t)1 << l) < v) l++; return l; }

// the leaf message of a column is 32 + 4 nl n_rows_total bytes in chunks of 1024; a launch hashes chunks [chunk_begin, chunk_begin +
// n_chunks_local) and loads every element that overlaps those bytes: they must be rows of [row_base, row_base + n_rows_local), and the
// furthest element of them inside comm (comm_elems elements)
bool leaf_ok(int nl, uint64_t comm_elems, uint64_t row_stride, uint64_t col_stride, uint64_t n_cols, int64_t row_base, uint64_t n_rows_local,
             uint64_t n_rows_total, uint32_t chunk_begin, uint32_t n_chunks_local, uint32_t n_chunks_total) {
  if (!nl_ok(nl) || !n_cols || !n_chunks_local) return false;
  if (n_cols > MAX_DIM || row_stride > MAX_DIM || col_stride > MAX_DIM || n_rows_total > MAX_DIM || n_rows_local > MAX_DIM) return false;
  if (row_base < 0 || (uint64_t)row_base > MAX_DIM) return false;
  const uint64_t eb = (uint64_t)nl * 4, total = 32 + eb * n_rows_total;
  if ((uint64_t)n_chunks_total != (total + 1023) / 1024) return false;
  if ((uint64_t)chunk_begin + n_chunks_local > n_chunks_total) return false;
  const uint64_t b0 = (uint64_t)chunk_begin * 1024;
  uint64_t b1 = ((uint64_t)chunk_begin + n_chunks_local) * 1024;
  if (b1 > total) b1 = total;
  if (b1 <= 32) return true;                                  // the zero prefix only: nothing is loaded
  const uint64_t first = b0 > 32 ? (b0 - 32) / eb : 0, last = (b1 - 32 - 1) / eb;      // (last < n_rows_total since b1 <= total)
  if (first < (uint64_t)row_base || last >= (uint64_t)row_base + n_rows_local) return false;
  return (last - (uint64_t)row_base) * row_stride + (n_cols - 1) * col_stride < comm_elems;
}

lcpc::LeafArgs leaf_args(const uint32_t* d_comm, uint64_t row_stride, uint64_t col_stride, uint64_t n_cols, int64_t row_base,
                         uint64_t n_rows_total, uint32_t chunk_begin, uint32_t n_chunks_local, uint32_t n_chunks_total, int canon_in,
                         uint32_t* d_out) {
  lcpc::LeafArgs a{};
  a.comm = d_comm; a.row_stride = row_stride; a.col_stride = col_stride; a.n_cols = n_cols; a.row_base = row_base;
  a.n_rows_total = n_rows_total; a.chunk_begin = chunk_begin; a.n_chunks_local = n_chunks_local; a.n_chunks_total = n_chunks_total;
  a.out = d_out; a.canon_in = canon_in ? 1u : 0u;
  return a;
}

}  // namespace

H_DEVICE_COUNT(k3h_)

// launch_leaf_chunks: comm of comm_elems elements (element (r, c) at (r - row_base) row_stride + c col_stride); out (in / out) is a
// buffer of out_slots x n_cols x 8 words, of which the launch writes slots [out_slot0, out_slot0 + n_chunks_local) (one chunk in all:
// the digests; else the chaining values)
H_EXPORT int k3h_leaf_chunks(int nl, const uint32_t* comm, uint64_t comm_elems, uint64_t row_stride, uint64_t col_stride,
                             uint64_t n_cols, int64_t row_base, uint64_t n_rows_local, uint64_t n_rows_total, uint32_t chunk_begin,
                             uint32_t n_chunks_local, uint32_t n_chunks_total, int canon_in, uint32_t* out, uint64_t out_slots,
                             uint64_t out_slot0) {
  if (!leaf_ok(nl, comm_elems, row_stride, col_stride, n_cols, row_base, n_rows_local, n_rows_total, chunk_begin, n_chunks_local,
               n_chunks_total)) return H_BAD_ARGS;
  if (out_slots > MAX_DIM || out_slot0 + n_chunks_local > out_slots) return H_BAD_ARGS;
  DevBuf d_comm, d_out;
  const size_t out_bytes = (size_t)out_slots * n_cols * 32;
  H_TRY(d_comm.put(comm, (size_t)comm_elems * nl * 4));
  H_TRY(d_out.put(out, out_bytes));
  const lcpc::LeafArgs a = leaf_args(d_comm.p, row_stride, col_stride, n_cols, row_base, n_rows_total, chunk_begin, n_chunks_local,
                                     n_chunks_total, canon_in, d_out.p + out_slot0 * n_cols * 8);
  H_TRY(lcpc::launch_leaf_chunks(nl, a, nullptr));
  H_TRY(hipDeviceSynchronize());
  return (int)d_out.get(out, out_bytes);
}

// launch_leaf_finish: cvs (n_chunks x n_cols x 8 words, in / out: the kernel keeps its stack there), digests (dig_cols >= n_cols columns
// of 8 words, in / out)
H_EXPORT int k3h_leaf_finish(uint32_t* cvs, uint32_t n_chunks, uint64_t n_cols, uint32_t* digests, uint64_t dig_cols) {
  if (!n_chunks || !n_cols || n_cols > MAX_DIM || n_chunks > MAX_DIM || dig_cols < n_cols || dig_cols > MAX_DIM) return H_BAD_ARGS;
  DevBuf d_cvs, d_dig;
  const size_t cv_bytes = (size_t)n_chunks * n_cols * 32, dig_bytes = (size_t)dig_cols * 32;
  H_TRY(d_cvs.put(cvs, cv_bytes));
  H_TRY(d_dig.put(digests, dig_bytes));
  H_TRY(lcpc::launch_leaf_finish(d_cvs.p, n_chunks, n_cols, d_dig.p, nullptr));
  H_TRY(hipDeviceSynchronize());
  H_TRY(d_cvs.get(cvs, cv_bytes));
  return (int)d_dig.get(digests, dig_bytes);
}

// launch_leaf_finish_nodes: cvs (n_slots x n_cols x 8 words, in / out); node j is the subtree of 2^node_log[j] chunks whose chaining
// value sits in slot node_slot[j] (null tables: slot j, one chunk each).  The nodes must tile chunks [chunk0, chunk0 + n_chunks) in
// order, each starting at a multiple of its size, in distinct slots below n_slots; root: chunk0 == 0 (the whole message); a pre-merge
// (root == 0) covers one aligned subtree
H_EXPORT int k3h_leaf_finish_nodes(uint32_t* cvs, uint64_t n_slots, const uint32_t* node_slot, const uint32_t* node_log,
                                   uint32_t n_nodes, uint64_t chunk0, uint64_t n_chunks, uint64_t n_cols, uint32_t* out,
                                   uint64_t out_cols, int root) {
  if (!n_nodes || !n_cols || n_cols > MAX_DIM || n_slots > MAX_DIM || n_nodes > n_slots || out_cols < n_cols || out_cols > MAX_DIM ||
      chunk0 > MAX_DIM || n_chunks > MAX_DIM) return H_BAD_ARGS;
  if (root ? chunk0 != 0 : (!pow2(n_chunks) || chunk0 % n_chunks)) return H_BAD_ARGS;
  std::vector<bool> used(n_slots, false);
  uint64_t at = chunk0;
  for (uint32_t j = 0; j < n_nodes; j++) {
    const uint64_t s = node_slot ? node_slot[j] : j;
    const uint32_t l = node_log ? node_log[j] : 0;
    if (s >= n_slots || used[s] || l > 28 || at % ((uint64_t)1 << l)) return H_BAD_ARGS;
    used[s] = true;
    at += (uint64_t)1 << l;
  }
  if (at != chunk0 + n_chunks) return H_BAD_ARGS;
  DevBuf d_cvs, d_out, d_slot, d_log;
  const size_t cv_bytes = (size_t)n_slots * n_cols * 32, out_bytes = (size_t)out_cols * 32;
  H_TRY(d_cvs.put(cvs, cv_bytes));
  H_TRY(d_out.put(out, out_bytes));
  if (node_slot) H_TRY(d_slot.put(node_slot, (size_t)n_nodes * 4));
  if (node_log) H_TRY(d_log.put(node_log, (size_t)n_nodes * 4));
  H_TRY(lcpc::launch_leaf_finish_nodes(d_cvs.p, node_slot ? d_slot.p : nullptr, node_log ? d_log.p : nullptr, n_nodes, n_cols, d_out.p,
                                         root != 0, nullptr));
  H_TRY(hipDeviceSynchronize());
  H_TRY(d_cvs.get(cvs, cv_bytes));
  return (int)d_out.get(out, out_bytes);
}

// leaf_tree_supported on the fields it reads: 1 / 0
H_EXPORT int k3h_leaf_tree_supported(uint64_t n_cols, uint64_t np2, uint32_t chunk_begin, uint32_t n_chunks_local, uint32_t n_chunks_total) {
  lcpc::LeafArgs a{};
  a.n_cols = n_cols; a.chunk_begin = chunk_begin; a.n_chunks_local = n_chunks_local; a.n_chunks_total = n_chunks_total;
  return lcpc::leaf_tree_supported(a, np2) ? 1 : 0;
}

// launch_leaf_tree: the leaf arguments as for k3h_leaf_chunks; hashes (2 np2 - 1 slots of 8 words, in / out).  What the launcher does
// not support it refuses itself (hipErrorInvalidValue, nothing launched); what it supports writes leaves and six levels, which a tree
// of np2 >= 128 leaves has
H_EXPORT int k3h_leaf_tree(int nl, const uint32_t* comm, uint64_t comm_elems, uint64_t row_stride, uint64_t col_stride, uint64_t n_cols,
                           int64_t row_base, uint64_t n_rows_local, uint64_t n_rows_total, uint32_t chunk_begin,
                           uint32_t n_chunks_local, uint32_t n_chunks_total, int canon_in, uint32_t* hashes, uint64_t np2) {
  if (!leaf_ok(nl, comm_elems, row_stride, col_stride, n_cols, row_base, n_rows_local, n_rows_total, chunk_begin, n_chunks_local,
               n_chunks_total)) return H_BAD_ARGS;
  if (!pow2(np2) || np2 < 2 || np2 > MAX_DIM) return H_BAD_ARGS;
  const lcpc::LeafArgs probe = leaf_args(nullptr, row_stride, col_stride, n_cols, row_base, n_rows_total, chunk_begin, n_chunks_local,
                                         n_chunks_total, canon_in, nullptr);
  // (supported implies the whole chunk range, np2 == n_cols >= 128 and a multiple of 64: every column of every workgroup exists)
  if (lcpc::leaf_tree_supported(probe, np2) && (np2 != n_cols || n_cols < 128 || n_cols % 64 || n_chunks_total > 2)) return H_BAD_ARGS;
  DevBuf d_comm, d_hashes;
  const size_t h_bytes = (size_t)(2 * np2 - 1) * 32;
  H_TRY(d_comm.put(comm, (size_t)comm_elems * nl * 4));
  H_TRY(d_hashes.put(hashes, h_bytes));
  const lcpc::LeafArgs a = leaf_args(d_comm.p, row_stride, col_stride, n_cols, row_base, n_rows_total, chunk_begin, n_chunks_local,
                                     n_chunks_total, canon_in, d_hashes.p);
  H_TRY(lcpc::launch_leaf_tree(nl, a, d_hashes.p, np2, nullptr));
  H_TRY(hipDeviceSynchronize());
  return (int)d_hashes.get(hashes, h_bytes);
}

// launch_merkle_tree_from: hashes (2 np2 - 1 slots, in / out) with the first levels_done levels above the leaves already there; at
// least one level is left to do (2^levels_done < np2), so a launch writes the root; root_out (16 words, in / out; the launcher gets
// its first 8) or null
H_EXPORT int k3h_merkle_tree_from(uint32_t* hashes, uint64_t np2, uint32_t levels_done, uint32_t* root_out) {
  if (!pow2(np2) || np2 < 2 || np2 > ((uint64_t)1 << 24) || levels_done >= log2u(np2)) return H_BAD_ARGS;
  DevBuf d_hashes, d_root;
  const size_t h_bytes = (size_t)(2 * np2 - 1) * 32;
  H_TRY(d_hashes.put(hashes, h_bytes));
  if (root_out) H_TRY(d_root.put(root_out, 64));
  H_TRY(lcpc::launch_merkle_tree_from(d_hashes.p, np2, levels_done, nullptr, root_out ? d_root.p : nullptr));
  H_TRY(hipDeviceSynchronize());
  H_TRY(d_hashes.get(hashes, h_bytes));
  return (int)(root_out ? d_root.get(root_out, 64) : hipSuccess);
}

// launch_gather_paths: hashes (2 np2 - 1 slots), cols (n, each < np2), paths (n x path_len x 8 words, in / out); a path has at most
// log2 np2 levels
H_EXPORT int k3h_gather_paths(const uint32_t* hashes, uint64_t np2, uint32_t path_len, const uint64_t* cols, uint32_t n, uint32_t* paths) {
  if (!pow2(np2) || np2 < 2 || np2 > ((uint64_t)1 << 24) || !path_len || path_len > log2u(np2) || !n || n > (1u << 20)) return H_BAD_ARGS;
  for (uint32_t k = 0; k < n; k++) if (cols[k] >= np2) return H_BAD_ARGS;
  DevBuf d_hashes, d_cols, d_paths;
  const size_t p_bytes = (size_t)n * path_len * 32;
  H_TRY(d_hashes.put(hashes, (size_t)(2 * np2 - 1) * 32));
  H_TRY(d_cols.put(cols, (size_t)n * 8));
  H_TRY(d_paths.put(paths, p_bytes));
  H_TRY(lcpc::launch_gather_paths(d_hashes.p, np2, path_len, reinterpret_cast<const uint64_t*>(d_cols.p), n, d_paths.p, 8, nullptr));
  H_TRY(hipDeviceSynchronize());
  return (int)d_paths.get(paths, p_bytes);
}

// ---- the batch forms (lcpc_amd/csrc/kernels.hip, BATCH = true): member i of a buffer starts i * stride 32-bit words behind member 0 and the
// buffer is n_batch * stride words, so every member -- the last one too -- is followed by its gap.  Refused before anything is launched:
// n_batch outside 1 .. 65535 (a grid dimension), a stride smaller than one member (a member's region would reach into the next), and a
// stride that is no multiple of 4 words (kernels.h: the kernels load and store 16 bytes at a time at member offsets).
namespace {

bool batch_ok(uint32_t n_batch) { return n_batch >= 1 && n_batch <= 65535; }
bool stride_ok(uint64_t stride, uint64_t member_words) { return stride >= member_words && stride % 4 == 0 && stride <= MAX_DIM; }

}  // namespace

// launch_leaf_chunks_batch: every member as for k3h_leaf_chunks -- a comm of comm_elems elements and an out of out_slots x n_cols x 8
// words, of which slots [out_slot0, out_slot0 + n_chunks_local) are written -- comm_stride / out_stride words apart
H_EXPORT int k3h_leaf_chunks_batch(int nl, const uint32_t* comm, uint64_t comm_elems, uint64_t row_stride, uint64_t col_stride,
                                   uint64_t n_cols, int64_t row_base, uint64_t n_rows_local, uint64_t n_rows_total, uint32_t chunk_begin,
                                   uint32_t n_chunks_local, uint32_t n_chunks_total, int canon_in, uint32_t* out, uint64_t out_slots,
                                   uint64_t out_slot0, uint32_t n_batch, uint64_t comm_stride, uint64_t out_stride) {
  if (!leaf_ok(nl, comm_elems, row_stride, col_stride, n_cols, row_base, n_rows_local, n_rows_total, chunk_begin, n_chunks_local,
               n_chunks_total)) return H_BAD_ARGS;       // (the same indices in every member: one check holds for all)
  if (out_slots > MAX_DIM || out_slot0 + n_chunks_local > out_slots || comm_elems > MAX_DIM) return H_BAD_ARGS;
  if (!batch_ok(n_batch) || !stride_ok(comm_stride, comm_elems * nl) || !stride_ok(out_stride, out_slots * n_cols * 8)) return H_BAD_ARGS;
  DevBuf d_comm, d_out;
  const size_t out_bytes = (size_t)n_batch * out_stride * 4;
  H_TRY(d_comm.put(comm, (size_t)n_batch * comm_stride * 4));
  H_TRY(d_out.put(out, out_bytes));
  const lcpc::LeafArgs a = leaf_args(d_comm.p, row_stride, col_stride, n_cols, row_base, n_rows_total, chunk_begin, n_chunks_local,
                                     n_chunks_total, canon_in, d_out.p + out_slot0 * n_cols * 8);
  H_TRY(lcpc::launch_leaf_chunks_batch(nl, a, n_batch, comm_stride, out_stride, nullptr));
  H_TRY(hipDeviceSynchronize());
  return (int)d_out.get(out, out_bytes);
}

// launch_leaf_tree_batch: every member as for k3h_leaf_tree, hashes (2 np2 - 1 slots per member) hashes_stride words apart.  The buffers
// hold n_batch members; the launcher is told n_batch_told members, which is n_batch or a count the launcher must refuse without a launch
// (0, or above 65535: no grid takes it either) -- so that its own answer to those is seen on buffers it must leave alone
H_EXPORT int k3h_leaf_tree_batch(int nl, const uint32_t* comm, uint64_t comm_elems, uint64_t row_stride, uint64_t col_stride,
                                 uint64_t n_cols, int64_t row_base, uint64_t n_rows_local, uint64_t n_rows_total, uint32_t chunk_begin,
                                 uint32_t n_chunks_local, uint32_t n_chunks_total, int canon_in, uint32_t* hashes, uint64_t np2,
                                 uint32_t n_batch, uint64_t comm_stride, uint64_t hashes_stride, uint32_t n_batch_told) {
  if (!leaf_ok(nl, comm_elems, row_stride, col_stride, n_cols, row_base, n_rows_local, n_rows_total, chunk_begin, n_chunks_local,
               n_chunks_total)) return H_BAD_ARGS;
  if (!pow2(np2) || np2 < 2 || np2 > MAX_DIM || comm_elems > MAX_DIM) return H_BAD_ARGS;
  if (!batch_ok(n_batch) || !stride_ok(comm_stride, comm_elems * nl) || !stride_ok(hashes_stride, (2 * np2 - 1) * 8)) return H_BAD_ARGS;
  if (n_batch_told != n_batch && n_batch_told != 0 && n_batch_told <= 65535) return H_BAD_ARGS;
  const lcpc::LeafArgs probe = leaf_args(nullptr, row_stride, col_stride, n_cols, row_base, n_rows_total, chunk_begin, n_chunks_local,
                                         n_chunks_total, canon_in, nullptr);
  if (lcpc::leaf_tree_supported(probe, np2) && (np2 != n_cols || n_cols < 128 || n_cols % 64 || n_chunks_total > 2)) return H_BAD_ARGS;
  DevBuf d_comm, d_hashes;
  const size_t h_bytes = (size_t)n_batch * hashes_stride * 4;
  H_TRY(d_comm.put(comm, (size_t)n_batch * comm_stride * 4));
  H_TRY(d_hashes.put(hashes, h_bytes));
  const lcpc::LeafArgs a = leaf_args(d_comm.p, row_stride, col_stride, n_cols, row_base, n_rows_total, chunk_begin, n_chunks_local,
                                     n_chunks_total, canon_in, d_hashes.p);
  const hipError_t e = lcpc::launch_leaf_tree_batch(nl, a, d_hashes.p, np2, n_batch_told, comm_stride, hashes_stride, nullptr);
  H_TRY(hipDeviceSynchronize());
  H_TRY(d_hashes.get(hashes, h_bytes));                    // (copied back after a refusal too: the caller sees that nothing was written)
  return (int)e;
}

// launch_leaf_finish_batch: every member as for k3h_leaf_finish -- cvs of n_chunks x n_cols x 8 words (in / out), digests of
// dig_cols >= n_cols columns (in / out) -- cvs_stride / digests_stride words apart
H_EXPORT int k3h_leaf_finish_batch(uint32_t* cvs, uint32_t n_chunks, uint64_t n_cols, uint64_t cvs_stride, uint32_t* digests,
                                   uint64_t dig_cols, uint64_t digests_stride, uint32_t n_batch) {
  if (!n_chunks || !n_cols || n_cols > MAX_DIM || n_chunks > MAX_DIM || dig_cols < n_cols || dig_cols > MAX_DIM) return H_BAD_ARGS;
  if (!batch_ok(n_batch) || !stride_ok(cvs_stride, (uint64_t)n_chunks * n_cols * 8) || !stride_ok(digests_stride, dig_cols * 8)) return H_BAD_ARGS;
  DevBuf d_cvs, d_dig;
  const size_t cv_bytes = (size_t)n_batch * cvs_stride * 4, dig_bytes = (size_t)n_batch * digests_stride * 4;
  H_TRY(d_cvs.put(cvs, cv_bytes));
  H_TRY(d_dig.put(digests, dig_bytes));
  H_TRY(lcpc::launch_leaf_finish_batch(d_cvs.p, n_chunks, n_cols, d_dig.p, n_batch, cvs_stride, digests_stride, nullptr));
  H_TRY(hipDeviceSynchronize());
  H_TRY(d_cvs.get(cvs, cv_bytes));
  return (int)d_dig.get(digests, dig_bytes);
}

// launch_merkle_tree_from_batch: every member as for k3h_merkle_tree_from, hashes_stride words apart; root_out (n_batch x 8 words and 8
// more that no member owns, in / out) or null
H_EXPORT int k3h_merkle_tree_from_batch(uint32_t* hashes, uint64_t np2, uint32_t levels_done, uint32_t n_batch, uint64_t hashes_stride,
                                        uint32_t* root_out) {
  if (!pow2(np2) || np2 < 2 || np2 > ((uint64_t)1 << 24) || levels_done >= log2u(np2)) return H_BAD_ARGS;
  if (!batch_ok(n_batch) || !stride_ok(hashes_stride, (2 * np2 - 1) * 8)) return H_BAD_ARGS;
  DevBuf d_hashes, d_root;
  const size_t h_bytes = (size_t)n_batch * hashes_stride * 4, r_bytes = ((size_t)n_batch + 1) * 32;
  H_TRY(d_hashes.put(hashes, h_bytes));
  if (root_out) H_TRY(d_root.put(root_out, r_bytes));
  H_TRY(lcpc::launch_merkle_tree_from_batch(d_hashes.p, np2, levels_done, n_batch, hashes_stride, nullptr, root_out ? d_root.p : nullptr));
  H_TRY(hipDeviceSynchronize());
  H_TRY(d_hashes.get(hashes, h_bytes));
  return (int)(root_out ? d_root.get(root_out, r_bytes) : hipSuccess);
}

// launch_batch_place: src (n_batch x src_stride 64-bit words), dst (dst_words >= n_batch x dst_stride 64-bit words, in / out: the
// words behind the last member belong to nobody); member i's first n_valid words are copied, the rest of its dst_stride words zeroed.
// Strides are in 64-bit words here (any count: the kernel moves one such word at a time); a stride below n_valid is one smaller than a member
H_EXPORT int k3h_batch_place(const uint64_t* src, uint64_t src_stride, uint64_t n_valid, uint64_t* dst, uint64_t dst_stride,
                             uint64_t dst_words, uint32_t n_batch) {
  if (!batch_ok(n_batch) || !dst_stride || src_stride > MAX_DIM || dst_stride > MAX_DIM) return H_BAD_ARGS;
  if (n_valid > src_stride || n_valid > dst_stride || dst_words < (uint64_t)n_batch * dst_stride || dst_words > ((uint64_t)1 << 32)) return H_BAD_ARGS;
  DevBuf d_src, d_dst;
  H_TRY(d_src.put(src, (size_t)n_batch * src_stride * 8));
  H_TRY(d_dst.put(dst, (size_t)dst_words * 8));
  H_TRY(lcpc::launch_batch_place(reinterpret_cast<const uint64_t*>(d_src.p), src_stride, n_valid, reinterpret_cast<uint64_t*>(d_dst.p),
                                   dst_stride, n_batch, nullptr));
  H_TRY(hipDeviceSynchronize());
  return (int)d_dst.get(dst, (size_t)dst_words * 8);
}

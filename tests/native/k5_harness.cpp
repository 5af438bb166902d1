// tests/native/k5_harness.cpp -- test-only C entry points over the prover's kernels (K5 / K6 of lcpc_amd/csrc/kernels.h: launch_collapse in
// both forms, launch_to_r29, launch_field_sum(_batch), launch_to_mont / launch_to_canon, launch_gather_columns(_batch),
// launch_gather_paths(_batch), launch_assemble_columns), in the manner of k7_harness.cpp: built by lcpc_amd/csrc/Makefile into
// lcpc_amd/lib/liblcpc_k5_harness.so and linked against the product library, which gains nothing by it (tests/k5_harness.py,
// tests/test_k5_cases.py, tests/test_gpu_k5_kernels.py).
//
// Every k5h_* entry takes HOST pointers, checks that every index the kernel will form stays inside the buffers it was given (a refused
// call returns H_BAD_ARGS and launches nothing), allocates device buffers, copies in, launches on the null stream, synchronises and
// copies the outputs back.  Outputs are in / out: a test pre-fills them and sees what was written.  For the batch forms the harness
// builds the ProveMember descriptors itself from per-member element offsets into ONE buffer, so that members sit wherever a test puts
// them, in any order, with poison between them.  The k5h_refuse_* entries hand a launcher arguments it must settle BEFORE any launch,
// with null buffers: they touch no device.
#include <vector>

#include "harness.h"
#include "../../lcpc_amd/csrc/kernels.h"

namespace {

constexpr uint64_t MAX_ELEMS = (uint64_t)1 << 24;   // what a test may ask for here (the launchers take far more)
bool batch_ok(uint32_t n_batch, int batch_form) { return batch_form ? (n_batch >= 1 && n_batch <= 65535) : n_batch == 1; }

}  // namespace

H_DEVICE_COUNT(k5h_)

// K5 / K5b.  coeffs: ONE buffer of coeffs_elems elements, member m's n_rows x n_per_row coefficients at element coeff_off[m]; tensors
// [n_batch][n_tensors][n_rows]; out: out_elems elements, in / out.  j0, j1, out_stride reach the launcher as given (0 = its defaults).
// batch_form == 0: the single launch on member 0 (n_batch must be 1); else CollapseArgs.members, and CollapseArgs.coeffs is null.
// limb_form (Ft255 only): the tensors go through launch_to_r29 and are passed as tensors29; else tensors29 is null
H_EXPORT int k5h_collapse(int nl, const uint32_t* coeffs, uint64_t coeffs_elems, const uint64_t* coeff_off, const uint32_t* tensors,
                          uint32_t* out, uint64_t out_elems, uint64_t n_rows, uint64_t n_per_row, uint32_t n_tensors, uint32_t n_splits,
                          uint64_t j0, uint64_t j1, uint64_t out_stride, uint32_t n_batch, int batch_form, int limb_form) {
  if (!nl_ok(nl) || !batch_ok(n_batch, batch_form) || (n_tensors != 1 && n_tensors != 2) || !n_splits || n_splits > 65535) return H_BAD_ARGS;
  if (!n_rows || !n_per_row || n_rows > MAX_ELEMS || n_per_row > MAX_ELEMS || n_rows * n_per_row > MAX_ELEMS) return H_BAD_ARGS;
  if (limb_form && nl != 8) return H_BAD_ARGS;
  if (coeffs_elems > MAX_ELEMS || out_elems > MAX_ELEMS || out_stride > MAX_ELEMS) return H_BAD_ARGS;
  const uint64_t ej0 = j1 ? j0 : 0, ej1 = j1 ? j1 : n_per_row, es = out_stride ? out_stride : n_per_row;   // the launcher's defaults
  if (ej1 > n_per_row || ej0 >= ej1 || es < ej1 - ej0) return H_BAD_ARGS;
  for (uint32_t m = 0; m < n_batch; m++)
    if (coeff_off[m] > coeffs_elems || n_rows * n_per_row > coeffs_elems - coeff_off[m]) return H_BAD_ARGS;
  const uint64_t n_tens = (uint64_t)n_batch * n_tensors * n_rows;
  if (n_tens > MAX_ELEMS || (uint64_t)n_batch * n_splits * n_tensors * es > out_elems) return H_BAD_ARGS;
  DevBuf d_coeffs, d_t, d_t29, d_out, d_members;
  H_TRY(d_coeffs.put(coeffs, (size_t)coeffs_elems * nl * 4));
  H_TRY(d_t.put(tensors, (size_t)n_tens * nl * 4));
  H_TRY(d_out.put(out, (size_t)out_elems * nl * 4));
  lcpc::CollapseArgs a{};
  a.tensors = d_t.p; a.out = d_out.p; a.n_rows = n_rows; a.n_per_row = n_per_row; a.n_tensors = n_tensors; a.n_splits = n_splits;
  a.j0 = j0; a.j1 = j1; a.out_stride = out_stride;
  if (batch_form) {
    std::vector<lcpc::ProveMember> mem(n_batch);
    for (uint32_t m = 0; m < n_batch; m++) { mem[m] = lcpc::ProveMember{}; mem[m].coeffs = d_coeffs.p + coeff_off[m] * nl; }
    H_TRY(d_members.put(mem.data(), mem.size() * sizeof(lcpc::ProveMember)));
    a.members = reinterpret_cast<const lcpc::ProveMember*>(d_members.p); a.n_batch = n_batch;
  } else {
    a.coeffs = d_coeffs.p + coeff_off[0] * nl;
  }
  if (limb_form) {
    H_TRY(d_t29.alloc((size_t)n_tens * 48));
    H_TRY(lcpc::launch_to_r29(d_t.p, n_tens, d_t29.p, nullptr));
    a.tensors29 = d_t29.p;
  }
  H_TRY(lcpc::launch_collapse(nl, a, nullptr));
  H_TRY(hipDeviceSynchronize());
  return (int)d_out.get(out, (size_t)out_elems * nl * 4);
}

// in: n Ft255 elements; out: out_entries entries of 12 words, in / out
H_EXPORT int k5h_to_r29(const uint32_t* in, uint64_t n, uint32_t* out, uint64_t out_entries) {
  if (!n || n > out_entries || out_entries > MAX_ELEMS) return H_BAD_ARGS;
  DevBuf d_in, d_out;
  H_TRY(d_in.put(in, (size_t)n * 32));
  H_TRY(d_out.put(out, (size_t)out_entries * 48));
  H_TRY(lcpc::launch_to_r29(d_in.p, n, d_out.p, nullptr));
  H_TRY(hipDeviceSynchronize());
  return (int)d_out.get(out, (size_t)out_entries * 48);
}

// buf: buf_elems elements, in / out: parts [n_batch][n_parts][n_elems], then the sums [n_batch][n_elems] right behind them, then
// whatever a test left there.  batch_form == 0: launch_field_sum (n_batch must be 1)
H_EXPORT int k5h_field_sum(int nl, uint32_t* buf, uint64_t buf_elems, uint32_t n_parts, uint64_t n_elems, uint32_t n_batch, int batch_form) {
  if (!nl_ok(nl) || !batch_ok(n_batch, batch_form) || !n_parts || !n_elems || n_elems > MAX_ELEMS || buf_elems > MAX_ELEMS) return H_BAD_ARGS;
  const uint64_t n_in = (uint64_t)n_batch * n_parts * n_elems;
  if (n_in > MAX_ELEMS || n_in + (uint64_t)n_batch * n_elems > buf_elems) return H_BAD_ARGS;
  DevBuf d;
  H_TRY(d.put(buf, (size_t)buf_elems * nl * 4));
  uint32_t* d_out = d.p + n_in * nl;
  if (batch_form) H_TRY(lcpc::launch_field_sum_batch(nl, d.p, n_parts, n_elems, d_out, n_batch, nullptr));
  else H_TRY(lcpc::launch_field_sum(nl, d.p, n_parts, n_elems, d_out, nullptr));
  H_TRY(hipDeviceSynchronize());
  return (int)d.get(buf, (size_t)buf_elems * nl * 4);
}

// to_mont != 0: launch_to_mont with r2 (one element), else launch_to_canon.  out: out_elems elements, in / out.  in_place: `in` is not
// read, the first n elements of out are the input and the launcher gets in == out
H_EXPORT int k5h_convert(int nl, int to_mont, const uint32_t* in, uint64_t n, const uint32_t* r2, uint32_t* out, uint64_t out_elems,
                         int in_place) {
  if (!nl_ok(nl) || !n || n > out_elems || out_elems > MAX_ELEMS || (to_mont && !r2) || (!in_place && !in)) return H_BAD_ARGS;
  DevBuf d_in, d_r2, d_out;
  if (!in_place) H_TRY(d_in.put(in, (size_t)n * nl * 4));
  if (to_mont) H_TRY(d_r2.put(r2, (size_t)nl * 4));
  H_TRY(d_out.put(out, (size_t)out_elems * nl * 4));
  const uint32_t* src = in_place ? d_out.p : d_in.p;
  if (to_mont) H_TRY(lcpc::launch_to_mont(nl, src, n, d_r2.p, d_out.p, nullptr));
  else H_TRY(lcpc::launch_to_canon(nl, src, n, d_out.p, nullptr));
  H_TRY(hipDeviceSynchronize());
  return (int)d_out.get(out, (size_t)out_elems * nl * 4);
}

// K6 / K6b.  comm: ONE buffer of comm_elems elements; member m's matrix starts at element comm_off[m], its element (r, c) at
// comm_off[m] + r * row_stride[m] + c * col_stride[m]; canon[m]: the member's values are canonical.  cols [n_batch][n_open], each
// < n_cols; r2: one element or null; vals: vals_elems elements, in / out.  batch_form == 0: launch_gather_columns on member 0 (n_batch
// must be 1), with r2 when canon[0] and null otherwise; else launch_gather_columns_batch with r2 as given
H_EXPORT int k5h_gather_columns(int nl, const uint32_t* comm, uint64_t comm_elems, const uint64_t* comm_off, const uint64_t* row_stride,
                                const uint64_t* col_stride, const uint32_t* canon, uint64_t n_rows, uint64_t n_cols, const uint64_t* cols,
                                uint32_t n_open, const uint32_t* r2, uint32_t* vals, uint64_t vals_elems, uint32_t n_batch, int batch_form) {
  if (!nl_ok(nl) || !batch_ok(n_batch, batch_form) || !n_rows || !n_cols || !n_open) return H_BAD_ARGS;
  if (n_rows > MAX_ELEMS || n_cols > MAX_ELEMS || comm_elems > MAX_ELEMS || vals_elems > MAX_ELEMS) return H_BAD_ARGS;
  for (uint32_t m = 0; m < n_batch; m++) {
    if (row_stride[m] > MAX_ELEMS || col_stride[m] > MAX_ELEMS || comm_off[m] > MAX_ELEMS) return H_BAD_ARGS;
    if (comm_off[m] + (n_rows - 1) * row_stride[m] + (n_cols - 1) * col_stride[m] >= comm_elems) return H_BAD_ARGS;   // < 2^49: no wrap
    if (canon[m] && !r2) return H_BAD_ARGS;
  }
  const uint64_t n_c = (uint64_t)n_batch * n_open;
  if (n_c > MAX_ELEMS || n_c * n_rows > vals_elems) return H_BAD_ARGS;
  for (uint64_t i = 0; i < n_c; i++)
    if (cols[i] >= n_cols) return H_BAD_ARGS;
  DevBuf d_comm, d_cols, d_r2, d_vals, d_members;
  H_TRY(d_comm.put(comm, (size_t)comm_elems * nl * 4));
  H_TRY(d_cols.put(cols, (size_t)n_c * 8));
  if (r2) H_TRY(d_r2.put(r2, (size_t)nl * 4));
  H_TRY(d_vals.put(vals, (size_t)vals_elems * nl * 4));
  const uint64_t* dc = reinterpret_cast<const uint64_t*>(d_cols.p);
  if (batch_form) {
    std::vector<lcpc::ProveMember> mem(n_batch);
    for (uint32_t m = 0; m < n_batch; m++) {
      mem[m] = lcpc::ProveMember{};
      mem[m].comm = d_comm.p + comm_off[m] * nl; mem[m].comm_row_stride = row_stride[m]; mem[m].comm_col_stride = col_stride[m];
      mem[m].comm_canon = canon[m];
    }
    H_TRY(d_members.put(mem.data(), mem.size() * sizeof(lcpc::ProveMember)));
    H_TRY(lcpc::launch_gather_columns_batch(nl, reinterpret_cast<const lcpc::ProveMember*>(d_members.p), n_batch, n_rows, dc, n_open, d_vals.p,
                                              r2 ? d_r2.p : nullptr, nullptr));
  } else {
    H_TRY(lcpc::launch_gather_columns(nl, d_comm.p + comm_off[0] * nl, n_rows, row_stride[0], col_stride[0], dc, n_open, d_vals.p,
                                        canon[0] ? d_r2.p : nullptr, nullptr));
  }
  H_TRY(hipDeviceSynchronize());
  return (int)d_vals.get(vals, (size_t)vals_elems * nl * 4);
}

// hashes: ONE buffer of hashes_digests digests of digest_words words; member m's 2 np2 - 1 digests start at digest hash_off[m].  cols
// [n_batch][n_open], each < np2; paths: paths_digests digests, in / out.  batch_form == 0: launch_gather_paths on member 0
H_EXPORT int k5h_gather_paths(const uint32_t* hashes, uint64_t hashes_digests, const uint64_t* hash_off, uint64_t np2, uint32_t path_len,
                              const uint64_t* cols, uint32_t n_open, uint32_t* paths, uint64_t paths_digests, uint32_t digest_words,
                              uint32_t n_batch, int batch_form) {
  if ((digest_words != 8 && digest_words != 16) || !batch_ok(n_batch, batch_form) || !n_open) return H_BAD_ARGS;
  if (np2 < 2 || np2 > ((uint64_t)1 << 20) || (np2 & (np2 - 1))) return H_BAD_ARGS;
  uint32_t depth = 0;
  while (((uint64_t)1 << depth) < np2) depth++;
  if (path_len > depth) return H_BAD_ARGS;        // level lvl < depth has np2 >> lvl >= 2 nodes: the sibling exists
  if (hashes_digests > MAX_ELEMS || paths_digests > MAX_ELEMS) return H_BAD_ARGS;
  for (uint32_t m = 0; m < n_batch; m++)
    if (hash_off[m] > hashes_digests || 2 * np2 - 1 > hashes_digests - hash_off[m]) return H_BAD_ARGS;
  const uint64_t n_c = (uint64_t)n_batch * n_open;
  if (n_c > MAX_ELEMS || n_c * path_len > paths_digests) return H_BAD_ARGS;
  for (uint64_t i = 0; i < n_c; i++)
    if (cols[i] >= np2) return H_BAD_ARGS;
  DevBuf d_h, d_cols, d_paths, d_members;
  H_TRY(d_h.put(hashes, (size_t)hashes_digests * digest_words * 4));
  H_TRY(d_cols.put(cols, (size_t)n_c * 8));
  H_TRY(d_paths.put(paths, (size_t)paths_digests * digest_words * 4));
  const uint64_t* dc = reinterpret_cast<const uint64_t*>(d_cols.p);
  if (batch_form) {
    std::vector<lcpc::ProveMember> mem(n_batch);
    for (uint32_t m = 0; m < n_batch; m++) { mem[m] = lcpc::ProveMember{}; mem[m].hashes = d_h.p + hash_off[m] * digest_words; }
    H_TRY(d_members.put(mem.data(), mem.size() * sizeof(lcpc::ProveMember)));
    H_TRY(lcpc::launch_gather_paths_batch(reinterpret_cast<const lcpc::ProveMember*>(d_members.p), n_batch, np2, path_len, dc, n_open, d_paths.p,
                                            digest_words, nullptr));
  } else {
    H_TRY(lcpc::launch_gather_paths(d_h.p + hash_off[0] * digest_words, np2, path_len, dc, n_open, d_paths.p, digest_words, nullptr));
  }
  H_TRY(hipDeviceSynchronize());
  return (int)d_paths.get(paths, (size_t)paths_digests * digest_words * 4);
}

// recv: G blocks of block_words words, rank g's the n opened columns of its rb[g + 1] - rb[g] rows; rb: G + 1 row boundaries; out:
// out_elems elements, in / out
H_EXPORT int k5h_assemble_columns(int nl, const uint32_t* recv, uint64_t block_words, const uint64_t* rb, uint32_t G, uint32_t n,
                                  uint64_t n_rows, uint32_t* out, uint64_t out_elems) {
  if (!nl_ok(nl) || !G || G > 4096 || !n || !n_rows || n_rows > MAX_ELEMS || out_elems > MAX_ELEMS) return H_BAD_ARGS;
  if ((block_words & 1) || block_words > MAX_ELEMS * 2 || (uint64_t)G * block_words > MAX_ELEMS * 8) return H_BAD_ARGS;   // 8-byte moves
  if (rb[0] != 0 || rb[G] != n_rows || (uint64_t)n * n_rows > out_elems) return H_BAD_ARGS;
  for (uint32_t g = 0; g < G; g++) {
    if (rb[g + 1] < rb[g] || rb[g + 1] > n_rows) return H_BAD_ARGS;
    if ((uint64_t)n * (rb[g + 1] - rb[g]) * nl > block_words) return H_BAD_ARGS;
  }
  DevBuf d_recv, d_rb, d_out;
  H_TRY(d_recv.put(recv, (size_t)G * block_words * 4));
  H_TRY(d_rb.put(rb, (size_t)(G + 1) * 8));
  H_TRY(d_out.put(out, (size_t)out_elems * nl * 4));
  H_TRY(lcpc::launch_assemble_columns(nl, d_recv.p, block_words, reinterpret_cast<const uint64_t*>(d_rb.p), G, n, n_rows, d_out.p, nullptr));
  H_TRY(hipDeviceSynchronize());
  return (int)d_out.get(out, (size_t)out_elems * nl * 4);
}

// ---- what a launcher answers to a job it must settle before any launch, on NULL buffers.  Each entry refuses (H_BAD_ARGS) every job
// a correct launcher would launch, and returns the launcher's hipError_t otherwise. ----------------------------------------------------

H_EXPORT int k5h_refuse_collapse(int nl, uint64_t n_per_row, uint32_t n_tensors, uint32_t n_splits, uint64_t j0, uint64_t j1, int batch_form,
                                 uint32_t n_batch, int limb_form) {
  const uint64_t ej0 = j1 ? j0 : 0, ej1 = j1 ? j1 : n_per_row;
  const bool settled = !nl_ok(nl) || (n_tensors != 1 && n_tensors != 2) || !n_splits || n_splits > 65535 || ej1 > n_per_row || ej0 >= ej1 ||
                       (batch_form && (!n_batch || n_batch > 65535));
  if (!settled) return H_BAD_ARGS;
  static uint32_t dummy[16];                 // a non-null tensors29 that nothing reads
  static lcpc::ProveMember none[1];          // a non-null members that nothing reads
  lcpc::CollapseArgs a{};
  a.n_rows = 1; a.n_per_row = n_per_row; a.n_tensors = n_tensors; a.n_splits = n_splits; a.j0 = j0; a.j1 = j1;
  a.tensors29 = limb_form ? dummy : nullptr;
  if (batch_form) { a.members = none; a.n_batch = n_batch; }
  return (int)lcpc::launch_collapse(nl, a, nullptr);
}

H_EXPORT int k5h_refuse_field_sum(int nl, uint32_t n_parts, uint64_t n_elems, int batch_form, uint32_t n_batch) {
  const bool settled = !n_elems || !n_parts || !nl_ok(nl) || (batch_form && (!n_batch || n_batch > 65535));
  if (!settled) return H_BAD_ARGS;
  if (batch_form) return (int)lcpc::launch_field_sum_batch(nl, nullptr, n_parts, n_elems, nullptr, n_batch, nullptr);
  return (int)lcpc::launch_field_sum(nl, nullptr, n_parts, n_elems, nullptr, nullptr);
}

H_EXPORT int k5h_refuse_gather_columns(int nl, uint64_t n_rows, uint32_t n_open, int batch_form, uint32_t n_batch) {
  const bool settled = !n_rows || !n_open || !nl_ok(nl) || (batch_form && (!n_batch || n_batch > 65535));
  if (!settled) return H_BAD_ARGS;
  if (batch_form) return (int)lcpc::launch_gather_columns_batch(nl, nullptr, n_batch, n_rows, nullptr, n_open, nullptr, nullptr, nullptr);
  return (int)lcpc::launch_gather_columns(nl, nullptr, n_rows, 1, 1, nullptr, n_open, nullptr, nullptr, nullptr);
}

H_EXPORT int k5h_refuse_gather_paths(uint32_t digest_words, uint32_t path_len, uint32_t n_open, int batch_form, uint32_t n_batch) {
  const bool settled = (digest_words != 8 && digest_words != 16) || !path_len || !n_open || (batch_form && !n_batch);
  if (!settled) return H_BAD_ARGS;
  if (batch_form) return (int)lcpc::launch_gather_paths_batch(nullptr, n_batch, 2, path_len, nullptr, n_open, nullptr, digest_words, nullptr);
  return (int)lcpc::launch_gather_paths(nullptr, 2, path_len, nullptr, n_open, nullptr, digest_words, nullptr);
}

// which: 0 = launch_to_canon, 1 = launch_to_mont, 2 = launch_to_r29 (nl is not its argument)
H_EXPORT int k5h_refuse_convert(int nl, int which, uint64_t n) {
  if (which < 0 || which > 2) return H_BAD_ARGS;
  const bool settled = !n || (which != 2 && !nl_ok(nl));
  if (!settled) return H_BAD_ARGS;
  if (which == 2) return (int)lcpc::launch_to_r29(nullptr, n, nullptr, nullptr);
  if (which == 1) return (int)lcpc::launch_to_mont(nl, nullptr, n, nullptr, nullptr, nullptr);
  return (int)lcpc::launch_to_canon(nl, nullptr, n, nullptr, nullptr);
}

H_EXPORT int k5h_refuse_assemble_columns(int nl, uint32_t n, uint64_t n_rows) {
  const bool settled = !n || !n_rows || !nl_ok(nl);
  if (!settled) return H_BAD_ARGS;
  return (int)lcpc::launch_assemble_columns(nl, nullptr, 0, nullptr, 1, n, n_rows, nullptr, nullptr);
}

// tests/native/k2_harness.cpp -- test-only C entry points over the Brakedown (K2) launchers of lcpc_amd/csrc/kernels.h, so that a test
// can hand a kernel a matrix and operands of its own making (tests/k2_harness.py, tests/test_gpu_k2_kernels.py).  Built by
// lcpc_amd/csrc/Makefile into lcpc_amd/lib/liblcpc_k2_harness.so and linked against the product library, which gains nothing by it.
//
// Every wrapper takes HOST pointers and element counts (an element is nl 32-bit words), checks that every index the kernel will form
// stays inside the buffers it was given (a refused call returns H_BAD_ARGS and launches nothing), allocates device buffers, copies
// in, launches on the null stream, synchronises, copies the in/out buffers back and frees.  The return value is the first hipError_t.
// Buffers a kernel writes are copied in first and back whole, so the caller sees what was written outside the expected region too.
#include <vector>

#include "harness.h"
#include "../../lcpc_amd/csrc/kernels.h"

namespace {

// the CSR-by-output matrix: monotone rowptr ending at nnz, every column below n_in
bool csr_ok(const uint32_t* rowptr, const uint32_t* colidx, uint64_t m, uint64_t nnz, uint64_t n_in) {
  if (rowptr[0] != 0 || rowptr[m] != nnz) return false;
  for (uint64_t o = 0; o < m; o++) if (rowptr[o] > rowptr[o + 1]) return false;
  for (uint64_t k = 0; k < nnz; k++) if (colidx[k] >= n_in) return false;
  return true;
}

// the matrix on the device the way ctx.cpp's upload lambda leaves it: rowptr, colidx, values, and (limb_form) the limb form derived on
// the device with one zeroed entry of slack behind it
struct DevCsr {
  DevBuf rowptr, colidx, vals, vals29, rprime;
  hipError_t upload(int nl, const uint32_t* h_rowptr, const uint32_t* h_colidx, const uint32_t* h_vals, uint64_t m, uint64_t nnz,
                    bool limb_form, const uint32_t* h_rprime) {
    hipError_t e;
    if ((e = rowptr.put(h_rowptr, (m + 1) * 4)) != hipSuccess) return e;
    if ((e = colidx.put(h_colidx, nnz * 4)) != hipSuccess) return e;
    if ((e = vals.put(h_vals, nnz * nl * 4)) != hipSuccess) return e;
    if (!limb_form) return hipSuccess;
    const size_t stride = (size_t)lcpc::ntt_lns_stride(nl);
    if ((e = vals29.alloc((nnz + 1) * stride * 4)) != hipSuccess) return e;
    if ((e = hipMemset(vals29.p, 0, (nnz + 1) * stride * 4)) != hipSuccess) return e;
    if (!nnz) return hipSuccess;
    if (nl == 8) return lcpc::launch_to_r29(vals.p, nnz, vals29.p, nullptr);
    if ((e = rprime.put(h_rprime, (size_t)nl * 4)) != hipSuccess) return e;
    return lcpc::launch_ntt_lns_roots(nl, vals.p, nnz, rprime.p, vals29.p, nullptr);
  }
};

}  // namespace

H_DEVICE_COUNT(k2h_)

// the limb form of n stored values (Ft255: launch_to_r29; Ft127 / Ft191: launch_ntt_lns_roots with R' mod p): out[n][stride] words
H_EXPORT int k2h_limb_form(int nl, const uint32_t* vals, uint64_t n, const uint32_t* rprime, uint32_t* out) {
  if ((nl != 4 && nl != 6 && nl != 8) || !n || (nl != 8 && !rprime)) return H_BAD_ARGS;
  const size_t stride = (size_t)lcpc::ntt_lns_stride(nl);
  DevBuf d_in, d_out, d_rp;
  H_TRY(d_in.put(vals, n * nl * 4));
  H_TRY(d_out.alloc(n * stride * 4));
  if (nl == 8) H_TRY(lcpc::launch_to_r29(d_in.p, n, d_out.p, nullptr));
  else {
    H_TRY(d_rp.put(rprime, (size_t)nl * 4));
    H_TRY(lcpc::launch_ntt_lns_roots(nl, d_in.p, n, d_rp.p, d_out.p, nullptr));
  }
  H_TRY(hipDeviceSynchronize());
  return (int)d_out.get(out, n * stride * 4);
}

// launch_spmv on a row-major matrix of n_rows x stride elements (in / out): inputs at [in_off, in_off + n_in), outputs at
// [out_off, out_off + m) of every row, or in out_alt (n_rows x out_alt_stride, in / out) when that is non-null
H_EXPORT int k2h_spmv(int nl, uint32_t* mat, uint64_t stride, uint64_t n_rows, uint64_t in_off, uint64_t n_in, uint64_t out_off,
                      uint32_t* out_alt, uint64_t out_alt_stride, const uint32_t* rowptr, const uint32_t* colidx,
                      const uint32_t* vals, uint64_t m, uint64_t nnz, int limb_form, const uint32_t* rprime) {
  if (!nl_ok(nl) || !m || !n_rows || n_rows > 65535 || in_off + n_in > stride) return H_BAD_ARGS;
  if (out_alt ? out_alt_stride < m : out_off + m > stride) return H_BAD_ARGS;
  if (!out_alt && !(out_off >= in_off + n_in || out_off + m <= in_off)) return H_BAD_ARGS;   // in and out segments are disjoint
  if (limb_form && (nl == 2 || (nl != 8 && !rprime))) return H_BAD_ARGS;
  if (!csr_ok(rowptr, colidx, m, nnz, n_in)) return H_BAD_ARGS;
  DevCsr csr;
  DevBuf d_mat, d_alt;
  H_TRY(csr.upload(nl, rowptr, colidx, vals, m, nnz, limb_form != 0, rprime));
  const size_t mat_bytes = (size_t)n_rows * stride * nl * 4, alt_bytes = out_alt ? (size_t)n_rows * out_alt_stride * nl * 4 : 0;
  H_TRY(d_mat.put(mat, mat_bytes));
  if (out_alt) H_TRY(d_alt.put(out_alt, alt_bytes));
  lcpc::SpmvArgs a{};
  a.mat = d_mat.p; a.out_alt = out_alt ? d_alt.p : nullptr; a.stride = stride; a.out_alt_stride = out_alt_stride;
  a.in_off = in_off; a.out_off = out_off; a.rowptr = csr.rowptr.p; a.colidx = csr.colidx.p; a.vals = csr.vals.p;
  a.vals29 = limb_form ? csr.vals29.p : nullptr; a.m = m; a.n_rows = n_rows;
  H_TRY(lcpc::launch_spmv(nl, a, nullptr));
  H_TRY(hipDeviceSynchronize());
  H_TRY(d_mat.get(mat, mat_bytes));
  return (int)(out_alt ? d_alt.get(out_alt, alt_bytes) : hipSuccess);
}

// launch_spmm_t on a position-major T of n_pos x n_rows elements (in / out): inputs at positions [in_off, in_off + n_in), outputs at
// [out_off, out_off + m), or in out_alt (m x n_rows, in / out) when that is non-null
H_EXPORT int k2h_spmm_t(int nl, uint32_t* t, uint64_t n_pos, uint64_t n_rows, uint64_t in_off, uint64_t n_in, uint64_t out_off,
                        uint32_t* out_alt, const uint32_t* rowptr, const uint32_t* colidx, const uint32_t* vals, uint64_t m,
                        uint64_t nnz, int limb_form, const uint32_t* rprime) {
  if (!nl_ok(nl) || !m || !n_rows || n_rows > (1u << 20) || in_off + n_in > n_pos) return H_BAD_ARGS;
  if (!out_alt && (out_off + m > n_pos || !(out_off >= in_off + n_in || out_off + m <= in_off))) return H_BAD_ARGS;
  if (limb_form && (nl == 2 || (nl != 8 && !rprime))) return H_BAD_ARGS;
  if (!csr_ok(rowptr, colidx, m, nnz, n_in)) return H_BAD_ARGS;
  DevCsr csr;
  DevBuf d_t, d_alt;
  H_TRY(csr.upload(nl, rowptr, colidx, vals, m, nnz, limb_form != 0, rprime));
  const size_t t_bytes = (size_t)n_pos * n_rows * nl * 4, alt_bytes = out_alt ? (size_t)m * n_rows * nl * 4 : 0;
  H_TRY(d_t.put(t, t_bytes));
  if (out_alt) H_TRY(d_alt.put(out_alt, alt_bytes));
  lcpc::SpmmTArgs a{};
  a.t = d_t.p; a.out_alt = out_alt ? d_alt.p : nullptr; a.n_rows = n_rows; a.in_off = in_off; a.out_off = out_off;
  a.rowptr = csr.rowptr.p; a.colidx = csr.colidx.p; a.vals = csr.vals.p; a.vals29 = limb_form ? csr.vals29.p : nullptr; a.m = m;
  H_TRY(lcpc::launch_spmm_t(nl, a, nullptr));     // (Ft255 without the limb form: the launcher refuses, nothing runs)
  H_TRY(hipDeviceSynchronize());
  H_TRY(d_t.get(t, t_bytes));
  return (int)(out_alt ? d_alt.get(out_alt, alt_bytes) : hipSuccess);
}

// launch_sdig_rs: in (n_rows x in_stride), mat (n_rows x stride, in / out), outputs at [out_off, out_off + n_out); r2 = R^2 mod p
H_EXPORT int k2h_sdig_rs(int nl, const uint32_t* in, uint64_t in_stride, uint32_t n_in, uint32_t* mat, uint64_t stride,
                         uint64_t out_off, uint32_t n_out, uint64_t n_rows, const uint32_t* r2) {
  if (!nl_ok(nl) || !n_out || !n_rows || n_rows > 65535 || n_in > in_stride || out_off + n_out > stride) return H_BAD_ARGS;
  DevBuf d_in, d_mat, d_r2;
  const size_t mat_bytes = (size_t)n_rows * stride * nl * 4;
  H_TRY(d_in.put(in, (size_t)n_rows * in_stride * nl * 4));
  H_TRY(d_mat.put(mat, mat_bytes));
  H_TRY(d_r2.put(r2, (size_t)nl * 4));
  H_TRY(lcpc::launch_sdig_rs(nl, d_in.p, in_stride, n_in, d_mat.p, stride, out_off, n_out, n_rows, d_r2.p, nullptr));
  H_TRY(hipDeviceSynchronize());
  return (int)d_mat.get(mat, mat_bytes);
}

// launch_sdig_rs_t: in_t (n_in x n_rows), t (n_pos x n_rows, in / out), outputs at positions [out_off, out_off + n_out)
H_EXPORT int k2h_sdig_rs_t(int nl, const uint32_t* in_t, uint32_t n_in, uint32_t* t, uint64_t n_pos, uint64_t out_off,
                           uint32_t n_out, uint64_t n_rows, const uint32_t* r2) {
  if (!nl_ok(nl) || !n_out || !n_rows || n_rows > (1u << 20) || out_off + n_out > n_pos) return H_BAD_ARGS;
  DevBuf d_in, d_t, d_r2;
  const size_t t_bytes = (size_t)n_pos * n_rows * nl * 4;
  H_TRY(d_in.put(in_t, (size_t)n_in * n_rows * nl * 4));
  H_TRY(d_t.put(t, t_bytes));
  H_TRY(d_r2.put(r2, (size_t)nl * 4));
  H_TRY(lcpc::launch_sdig_rs_t(nl, d_in.p, n_in, d_t.p, out_off, n_out, n_rows, d_r2.p, nullptr));
  H_TRY(hipDeviceSynchronize());
  return (int)d_t.get(t, t_bytes);
}

// launch_transpose_to_t: src of src_elems elements (rows of src_stride), t (n_valid x n_rows, in / out), copy_dst (may be null; as
// large as src, in / out)
H_EXPORT int k2h_transpose_to_t(int nl, const uint32_t* src, uint64_t src_elems, uint64_t src_stride, uint64_t n_valid,
                                uint64_t n_rows, uint32_t* t, uint64_t n_src_total, uint32_t* copy_dst, int canon) {
  if (!nl_ok(nl) || !n_valid || !n_rows || n_valid > src_stride) return H_BAD_ARGS;
  const uint64_t span = (n_rows - 1) * src_stride + n_valid;          // one past the last flat element the kernel can touch
  if ((span < n_src_total ? span : n_src_total) > src_elems) return H_BAD_ARGS;
  if (copy_dst && span > src_elems) return H_BAD_ARGS;
  DevBuf d_src, d_t, d_copy;
  const size_t t_bytes = (size_t)n_valid * n_rows * nl * 4, src_bytes = (size_t)src_elems * nl * 4;
  H_TRY(d_src.put(src, src_bytes));
  H_TRY(d_t.put(t, t_bytes));
  if (copy_dst) H_TRY(d_copy.put(copy_dst, src_bytes));
  H_TRY(lcpc::launch_transpose_to_t(nl, d_src.p, src_stride, n_valid, n_rows, d_t.p, nullptr, n_src_total,
                                      copy_dst ? d_copy.p : nullptr, canon != 0));
  H_TRY(hipDeviceSynchronize());
  H_TRY(d_t.get(t, t_bytes));
  return (int)(copy_dst ? d_copy.get(copy_dst, src_bytes) : hipSuccess);
}

// launch_transpose_from_t: t (n_pos x n_rows), dst (n_rows x dst_stride, in / out)
H_EXPORT int k2h_transpose_from_t(int nl, const uint32_t* t, uint64_t n_pos, uint64_t n_rows, uint32_t* dst, uint64_t dst_stride) {
  if (!nl_ok(nl) || !n_pos || !n_rows || n_pos > dst_stride) return H_BAD_ARGS;
  DevBuf d_t, d_dst;
  const size_t dst_bytes = (size_t)n_rows * dst_stride * nl * 4;
  H_TRY(d_t.put(t, (size_t)n_pos * n_rows * nl * 4));
  H_TRY(d_dst.put(dst, dst_bytes));
  H_TRY(lcpc::launch_transpose_from_t(nl, d_t.p, n_pos, n_rows, d_dst.p, dst_stride, nullptr));
  H_TRY(hipDeviceSynchronize());
  return (int)d_dst.get(dst, dst_bytes);
}

// launch_pad_rows: src (n_rows x src_stride), dst (n_rows x dst_stride, in / out)
H_EXPORT int k2h_pad_rows(int nl, const uint32_t* src, uint64_t src_stride, uint32_t* dst, uint64_t dst_stride, uint64_t n_valid,
                          uint64_t n_rows) {
  if (!nl_ok(nl) || !n_valid || !n_rows || n_rows > 65535 || n_valid > src_stride || n_valid > dst_stride) return H_BAD_ARGS;
  DevBuf d_src, d_dst;
  const size_t dst_bytes = (size_t)n_rows * dst_stride * nl * 4;
  H_TRY(d_src.put(src, (size_t)n_rows * src_stride * nl * 4));
  H_TRY(d_dst.put(dst, dst_bytes));
  H_TRY(lcpc::launch_pad_rows(nl, d_src.p, src_stride, d_dst.p, dst_stride, n_valid, n_rows, nullptr));
  H_TRY(hipDeviceSynchronize());
  return (int)d_dst.get(dst, dst_bytes);
}

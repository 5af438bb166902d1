// tests/native/k2b_harness.cpp -- test-only C entry points over the BATCH forms of the position-major Brakedown launchers of
// lcpc_amd/csrc/kernels.h (launch_transpose_to_t_batch, launch_spmm_t_batch, launch_sdig_rs_t_batch), in the manner of k2_harness.cpp:
// built by lcpc_amd/csrc/Makefile into lcpc_amd/lib/liblcpc_k2b_harness.so and linked against the product library, which gains nothing
// by it (tests/k2b_harness.py, tests/test_gpu_k2_batch.py).
//
// Every wrapper takes HOST pointers, checks that every index the kernel will form stays inside the buffers it was given (a refused
// call returns H_BAD_ARGS and launches nothing), allocates device buffers, copies in, launches on the null stream, synchronises,
// copies the in / out buffers back whole and frees.  Member strides are in 32-bit words, as at the launchers.  k2bh_refusal hands a
// launcher arguments it must refuse (or an empty job it must accept) BEFORE any launch, with null buffers: it touches no device.
#include "harness.h"
#include "../../lcpc_amd/csrc/kernels.h"

namespace {

constexpr uint64_t MAX_BATCH_ROWS = 1u << 16;       // what a test may ask for here (the launchers take far more)

// members of `extent` words at `stride` words: no overlap, elements aligned as member 0's
bool stride_ok(uint64_t stride, uint64_t extent) { return stride >= extent && stride % 4 == 0; }
bool batch_ok(uint32_t n_batch, uint64_t n_rows) { return n_batch && n_batch <= 65535 && n_rows && (uint64_t)n_batch * n_rows <= MAX_BATCH_ROWS; }

bool csr_ok(const uint32_t* rowptr, const uint32_t* colidx, uint64_t m, uint64_t nnz, uint64_t n_in) {
  if (rowptr[0] != 0 || rowptr[m] != nnz) return false;
  for (uint64_t o = 0; o < m; o++) if (rowptr[o] > rowptr[o + 1]) return false;
  for (uint64_t k = 0; k < nnz; k++) if (colidx[k] >= n_in) return false;
  return true;
}

// the matrix on the device the way ctx.cpp's upload leaves it (k2_harness.cpp DevCsr)
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

H_DEVICE_COUNT(k2bh_)

// launch_spmm_t_batch: t = n_batch members of t_stride words, each a position-major T of n_pos x n_rows elements (in / out): inputs
// at positions [in_off, in_off + n_in), outputs at [out_off, out_off + m), or in out_alt (n_batch members of alt_stride words, each
// m x n_rows, in / out) when that is non-null
H_EXPORT int k2bh_spmm_t(int nl, uint32_t* t, uint32_t n_batch, uint64_t t_stride, uint64_t n_pos, uint64_t n_rows, uint64_t in_off,
                         uint64_t n_in, uint64_t out_off, uint32_t* out_alt, uint64_t alt_stride, const uint32_t* rowptr,
                         const uint32_t* colidx, const uint32_t* vals, uint64_t m, uint64_t nnz, int limb_form, const uint32_t* rprime) {
  if (!nl_ok(nl) || !m || !batch_ok(n_batch, n_rows) || in_off + n_in > n_pos) return H_BAD_ARGS;
  if (!stride_ok(t_stride, n_pos * n_rows * nl)) return H_BAD_ARGS;
  if (out_alt ? !stride_ok(alt_stride, m * n_rows * nl) : (out_off + m > n_pos || !(out_off >= in_off + n_in || out_off + m <= in_off)))
    return H_BAD_ARGS;
  if (limb_form && (nl == 2 || (nl != 8 && !rprime))) return H_BAD_ARGS;
  if (!csr_ok(rowptr, colidx, m, nnz, n_in)) return H_BAD_ARGS;
  DevCsr csr;
  DevBuf d_t, d_alt;
  H_TRY(csr.upload(nl, rowptr, colidx, vals, m, nnz, limb_form != 0, rprime));
  const size_t t_bytes = (size_t)n_batch * t_stride * 4, alt_bytes = out_alt ? (size_t)n_batch * alt_stride * 4 : 0;
  H_TRY(d_t.put(t, t_bytes));
  if (out_alt) H_TRY(d_alt.put(out_alt, alt_bytes));
  lcpc::SpmmTArgs a{};
  a.t = d_t.p; a.out_alt = out_alt ? d_alt.p : nullptr; a.n_rows = n_rows; a.in_off = in_off; a.out_off = out_off;
  a.rowptr = csr.rowptr.p; a.colidx = csr.colidx.p; a.vals = csr.vals.p; a.vals29 = limb_form ? csr.vals29.p : nullptr; a.m = m;
  H_TRY(lcpc::launch_spmm_t_batch(nl, a, n_batch, t_stride, alt_stride, nullptr));     // (Ft255 without the limb form: refused, nothing runs)
  H_TRY(hipDeviceSynchronize());
  H_TRY(d_t.get(t, t_bytes));
  return (int)(out_alt ? d_alt.get(out_alt, alt_bytes) : hipSuccess);
}

// launch_sdig_rs_t_batch: in_t = n_batch members of in_stride words (each n_in x n_rows), t = n_batch members of t_stride words (each
// n_pos x n_rows, in / out), outputs at positions [out_off, out_off + n_out); r2 = R^2 mod p
H_EXPORT int k2bh_sdig_rs_t(int nl, const uint32_t* in_t, uint64_t in_stride, uint32_t n_in, uint32_t* t, uint64_t t_stride,
                            uint64_t n_pos, uint64_t out_off, uint32_t n_out, uint64_t n_rows, const uint32_t* r2, uint32_t n_batch) {
  if (!nl_ok(nl) || !n_out || !batch_ok(n_batch, n_rows) || out_off + n_out > n_pos) return H_BAD_ARGS;
  if (!stride_ok(in_stride, (uint64_t)n_in * n_rows * nl) || !stride_ok(t_stride, n_pos * n_rows * nl)) return H_BAD_ARGS;
  DevBuf d_in, d_t, d_r2;
  const size_t t_bytes = (size_t)n_batch * t_stride * 4;
  H_TRY(d_in.put(in_t, (size_t)n_batch * in_stride * 4));
  H_TRY(d_t.put(t, t_bytes));
  H_TRY(d_r2.put(r2, (size_t)nl * 4));
  H_TRY(lcpc::launch_sdig_rs_t_batch(nl, d_in.p, n_in, d_t.p, out_off, n_out, n_rows, d_r2.p, n_batch, in_stride, t_stride, nullptr));
  H_TRY(hipDeviceSynchronize());
  return (int)d_t.get(t, t_bytes);
}

// launch_transpose_to_t_batch: src of src_elems elements (the members' rows stacked, src_stride elements per row), t = n_batch
// members of t_stride words (each n_valid x n_rows, in / out), copy_dst (may be null; as large as src, in / out)
H_EXPORT int k2bh_transpose_to_t(int nl, const uint32_t* src, uint64_t src_elems, uint64_t src_stride, uint64_t n_valid,
                                 uint64_t n_rows, uint32_t* t, uint64_t t_stride, uint32_t n_batch, uint64_t n_src_total,
                                 uint32_t* copy_dst, int canon) {
  if (!nl_ok(nl) || !n_valid || !batch_ok(n_batch, n_rows) || n_valid > src_stride) return H_BAD_ARGS;
  if (!stride_ok(t_stride, n_valid * n_rows * nl)) return H_BAD_ARGS;
  // one past the last flat element the kernel can touch (n_src_total masks inside a member only: the whole span must be there)
  if (((uint64_t)n_batch * n_rows - 1) * src_stride + n_valid > src_elems) return H_BAD_ARGS;
  DevBuf d_src, d_t, d_copy;
  const size_t t_bytes = (size_t)n_batch * t_stride * 4, src_bytes = (size_t)src_elems * nl * 4;
  H_TRY(d_src.put(src, src_bytes));
  H_TRY(d_t.put(t, t_bytes));
  if (copy_dst) H_TRY(d_copy.put(copy_dst, src_bytes));
  H_TRY(lcpc::launch_transpose_to_t_batch(nl, d_src.p, src_stride, n_valid, n_rows, d_t.p, n_batch, t_stride, nullptr, n_src_total,
                                             copy_dst ? d_copy.p : nullptr, canon != 0));
  H_TRY(hipDeviceSynchronize());
  H_TRY(d_t.get(t, t_bytes));
  return (int)(copy_dst ? d_copy.get(copy_dst, src_bytes) : hipSuccess);
}

// What a launcher answers to a job it must settle before any launch: which = 0 transpose, 1 spmm, 2 sdig_rs.  The job is n_batch
// members of n_rows rows with `work` outputs / valid positions, on NULL buffers -- so this refuses (H_BAD_ARGS) every job a correct
// launcher would launch: only n_batch == 0 or > 65535, more batch rows than the launcher's grid carries (rows_per_block x 65535),
// Ft255 without the limb form (spmm), and empty work get through.  Returns the launcher's hipError_t.
H_EXPORT int k2bh_refusal(int which, int nl, uint32_t n_batch, uint64_t n_rows, uint64_t work, int limb_form) {
  if (!nl_ok(nl) || which < 0 || which > 2) return H_BAD_ARGS;
  const uint64_t per_block = which == 0 ? 32 : 128;
  const bool settled = n_batch == 0 || n_batch > 65535 || (uint64_t)n_batch * n_rows > 65535 * per_block ||
                       (which == 1 && nl == 8 && !limb_form) || work == 0 || n_rows == 0;
  if (!settled) return H_BAD_ARGS;
  static uint32_t dummy[16];        // a non-null vals29 that nothing reads
  if (which == 0) return (int)lcpc::launch_transpose_to_t_batch(nl, nullptr, work, work, n_rows, nullptr, n_batch, 0, nullptr);
  if (which == 2) return (int)lcpc::launch_sdig_rs_t_batch(nl, nullptr, 1, nullptr, 0, (uint32_t)work, n_rows, nullptr, n_batch, 0, 0, nullptr);
  lcpc::SpmmTArgs a{};
  a.n_rows = n_rows; a.m = work; a.vals29 = limb_form ? dummy : nullptr;
  return (int)lcpc::launch_spmm_t_batch(nl, a, n_batch, 0, 0, nullptr);
}

// tests/native/k7_harness.cpp -- test-only C entry points over the column check of the batched verify (K7b: launch_verify_columns_batch
// of lcpc_amd/csrc/kernels.h), in the manner of k2b_harness.cpp: built by lcpc_amd/csrc/Makefile into lcpc_amd/lib/liblcpc_k7_harness.so
// and linked against the product library, which gains nothing by it (tests/k7_harness.py, tests/test_gpu_k7_kernels.py).
//
// k7h_verify_columns takes HOST pointers, checks that every index the kernel will form stays inside the buffers it was given (a refused
// call returns H_BAD_ARGS and launches nothing), allocates device buffers, copies in, converts the tensors to the 29-bit-limb form for
// Ft255 as verify_batch.cpp does, launches on the null stream, synchronises and copies the status words back.  k7h_refusal hands the
// launcher arguments it must settle BEFORE any launch, with null buffers: it touches no device.
#include "harness.h"
#include "../../lcpc_amd/csrc/kernels.h"

namespace {

constexpr uint64_t MAX_ELEMS = (uint64_t)1 << 24;   // what a test may ask for here (the launcher takes far more)

}  // namespace

H_DEVICE_COUNT(k7h_)

// cols: n_batch members of cols_stride elements (the first n_open * n_rows of each are its columns); tensors [n_batch][n_t][n_rows];
// enc [n_batch][n_t][n_cols]; drawn [n_batch][n_open] (any value: the kernel must not read enc for one >= n_cols);
// status [n_batch][n_open], in / out (a test pre-fills it to see what is written)
H_EXPORT int k7h_verify_columns(int nl, const uint32_t* cols, uint64_t cols_stride, const uint32_t* tensors, const uint32_t* enc,
                                const uint64_t* drawn, uint32_t* status, uint64_t n_rows, uint64_t n_cols, uint32_t n_open, uint32_t n_t,
                                uint32_t n_batch) {
  if (!nl_ok(nl) || !n_batch || n_batch > 65535 || !n_open || !n_t || !n_rows || !n_cols) return H_BAD_ARGS;
  if (cols_stride < (uint64_t)n_open * n_rows) return H_BAD_ARGS;
  if ((uint64_t)n_batch * cols_stride > MAX_ELEMS || (uint64_t)n_batch * n_t * n_rows > MAX_ELEMS || (uint64_t)n_batch * n_t * n_cols > MAX_ELEMS)
    return H_BAD_ARGS;
  DevBuf d_cols, d_t, d_t29, d_enc, d_drawn, d_status;
  const size_t n_tens = (size_t)n_batch * n_t * n_rows, st_bytes = (size_t)n_batch * n_open * 4;
  H_TRY(d_cols.put(cols, (size_t)n_batch * cols_stride * nl * 4));
  H_TRY(d_t.put(tensors, n_tens * nl * 4));
  H_TRY(d_enc.put(enc, (size_t)n_batch * n_t * n_cols * nl * 4));
  H_TRY(d_drawn.put(drawn, (size_t)n_batch * n_open * 8));
  H_TRY(d_status.put(status, st_bytes));
  lcpc::VerifyColsArgs a{};
  a.cols = d_cols.p; a.cols_stride = cols_stride; a.tensors = d_t.p; a.enc = d_enc.p;
  a.drawn = reinterpret_cast<const uint64_t*>(d_drawn.p); a.status = d_status.p;
  a.n_rows = n_rows; a.n_cols = n_cols; a.n_open = n_open; a.n_t = n_t; a.n_batch = n_batch;
  if (nl == 8) {
    H_TRY(d_t29.alloc(n_tens * 48));
    H_TRY(lcpc::launch_to_r29(d_t.p, n_tens, d_t29.p, nullptr));
    a.tensors29 = d_t29.p;
  }
  H_TRY(lcpc::launch_verify_columns_batch(nl, a, nullptr));
  H_TRY(hipDeviceSynchronize());
  return (int)d_status.get(status, st_bytes);
}

// What the launcher answers to a job it must settle before any launch, on NULL buffers -- so this refuses (H_BAD_ARGS) every job a
// correct launcher would launch: only n_batch == 0 or > 65535, n_open == 0, n_t == 0 and Ft255 without the limb form get through.
// Returns the launcher's hipError_t.
H_EXPORT int k7h_refusal(int nl, uint32_t n_batch, uint32_t n_open, uint32_t n_t, int limb_form) {
  if (!nl_ok(nl)) return H_BAD_ARGS;
  const bool settled = n_batch == 0 || n_batch > 65535 || n_open == 0 || n_t == 0 || (nl == 8 && !limb_form);
  if (!settled) return H_BAD_ARGS;
  static uint32_t dummy[16];        // a non-null tensors29 that nothing reads
  lcpc::VerifyColsArgs a{};
  a.n_rows = 1; a.n_cols = 1; a.n_open = n_open; a.n_t = n_t; a.n_batch = n_batch; a.tensors29 = limb_form ? dummy : nullptr;
  return (int)lcpc::launch_verify_columns_batch(nl, a, nullptr);
}

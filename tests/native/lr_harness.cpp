// tests/native/lr_harness.cpp -- test-only C entry points over the resumable column-hash launchers of lcpc_amd/csrc/kernels.h
// (launch_sha3_leaves_range, launch_keccak256_leaves_range, launch_sha256_leaves_range, launch_blake2b_leaves_range), so that a test can
// hand a kernel a commitment matrix that ends where a row batch ends, a block range and a chaining-state buffer of its own making
// (tests/lr_harness.py, tests/test_gpu_leaf_range.py).  Built by lcpc_amd/csrc/Makefile into lcpc_amd/lib/liblcpc_lr_harness.so and
// linked against the product library, which gains nothing by it.
//
// The wrapper takes HOST pointers, checks that every index the kernel will form stays inside the buffers it was given (a refused call
// returns LRH_BAD_ARGS and launches nothing), allocates device buffers, copies in, launches one range on the null stream, synchronises,
// copies `state` and `out` back whole and frees.  The return value is the first hipError_t.  Both buffers are copied in first and back
// whole, so the caller sees what was written outside the expected region too (sentinel fill).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../lcpc_amd/csrc/kernels.h"

#define LRH_EXPORT extern "C" __attribute__((visibility("default")))
#define LRH_BAD_ARGS (-1)

namespace {

struct DevBuf {
  uint32_t* p = nullptr;
  ~DevBuf() { if (p) (void)hipFree(p); }
  hipError_t put(const void* src, size_t bytes) {
    hipError_t e = hipMalloc((void**)&p, bytes ? bytes : 16);
    if (e == hipSuccess && bytes) e = hipMemcpy(p, src, bytes, hipMemcpyHostToDevice);
    return e;
  }
  hipError_t get(void* dst, size_t bytes) const { return bytes ? hipMemcpy(dst, p, bytes, hipMemcpyDeviceToHost) : hipSuccess; }
};

#define LRH_TRY(expr) do { hipError_t e_ = (expr); if (e_ != hipSuccess) return (int)e_; } while (0)

constexpr uint64_t MAX_DIM = (uint64_t)1 << 28;      // rows, columns, strides: far above any test, far below 64-bit overflow of a product

enum Family { SHA3 = 0, KECCAK256 = 1, SHA256 = 2, BLAKE2B = 3 };
struct Shape { uint64_t prefix_words, block_words, state_words, digest_words, n_blocks; };   // message in 64-bit words, buffers in 32-bit words

bool shape_of(int family, int nl, uint64_t n_rows_total, Shape* s) {
  if (nl != 2 && nl != 4 && nl != 6 && nl != 8) return false;
  switch (family) {
    case SHA3: case KECCAK256: *s = {4, 17, lcpc::SHA3_STATE_WORDS, 8, lcpc::sha3_leaf_blocks(nl, n_rows_total)}; return true;
    case SHA256: *s = {4, 8, lcpc::SHA256_STATE_WORDS, 8, lcpc::sha256_leaf_blocks(nl, n_rows_total)}; return true;
    case BLAKE2B: *s = {8, 16, lcpc::BLAKE2B_STATE_WORDS, 16, lcpc::blake2b_leaf_blocks(nl, n_rows_total)}; return true;
  }
  return false;
}

}  // namespace

LRH_EXPORT int lrh_device_count() {
  int n = 0;
  return hipGetDeviceCount(&n) == hipSuccess ? n : 0;
}

// blocks of the whole leaf message (0: family or nl unknown)
LRH_EXPORT uint64_t lrh_leaf_blocks(int family, int nl, uint64_t n_rows_total) {
  Shape s;
  return n_rows_total <= MAX_DIM && shape_of(family, nl, n_rows_total, &s) ? s.n_blocks : 0;
}

// one launch of blocks [blk_begin, blk_end).  comm: comm_elems elements, element (r, c) at r row_stride + c col_stride (row 0 is the
// message's first row); it has to hold every row the range's blocks carry bytes of and nothing more.  state (in / out): state_words
// 32-bit words, the kernel's region starting at word state_off (even: the sponge and BLAKE2b states are 64-bit words); out (in / out):
// out_words words, the digests starting at word out_off (a multiple of 4: the digest stores are 16 bytes wide)
LRH_EXPORT int lrh_leaf_range(int family, int nl, const uint32_t* comm, uint64_t comm_elems, uint64_t row_stride, uint64_t col_stride,
                              uint64_t n_cols, uint64_t n_rows_total, uint64_t blk_begin, uint64_t blk_end, int canon_in, uint32_t* state,
                              uint64_t state_words, uint64_t state_off, uint32_t* out, uint64_t out_words, uint64_t out_off) {
  Shape s;
  if (!n_cols || !n_rows_total || n_cols > MAX_DIM || n_rows_total > MAX_DIM || row_stride > MAX_DIM || col_stride > MAX_DIM ||
      comm_elems > (MAX_DIM << 4) || !shape_of(family, nl, n_rows_total, &s)) return LRH_BAD_ARGS;
  if (blk_begin > blk_end || blk_end > s.n_blocks) return LRH_BAD_ARGS;
  if (!comm || !state || !out) return LRH_BAD_ARGS;
  if (state_words > (MAX_DIM << 6) || (state_off & 1) || state_off > state_words || s.state_words * n_cols > state_words - state_off) return LRH_BAD_ARGS;
  if (out_words > (MAX_DIM << 6) || (out_off & 3) || out_off > out_words || s.digest_words * n_cols > out_words - out_off) return LRH_BAD_ARGS;
  // the rows whose limbs lie in words [block_words blk_begin, block_words blk_end) of the message: the furthest element of them is the
  // furthest the launch addresses (rows >= n_rows_total are the zero words of the padding and are not loaded)
  const uint64_t L = (uint64_t)nl / 2, w1 = s.block_words * blk_end;
  if (blk_end > blk_begin && w1 > s.prefix_words) {
    uint64_t last = (w1 - s.prefix_words - 1) / L;
    if (last >= n_rows_total) last = n_rows_total - 1;
    if (last * row_stride + (n_cols - 1) * col_stride >= comm_elems) return LRH_BAD_ARGS;
  }
  DevBuf d_comm, d_state, d_out;
  LRH_TRY(d_comm.put(comm, (size_t)comm_elems * nl * 4));
  LRH_TRY(d_state.put(state, (size_t)state_words * 4));
  LRH_TRY(d_out.put(out, (size_t)out_words * 4));
  lcpc::LeafArgs a{};
  a.comm = d_comm.p; a.row_stride = row_stride; a.col_stride = col_stride; a.n_cols = n_cols; a.row_base = 0; a.n_rows_total = n_rows_total;
  a.out = d_out.p + out_off; a.canon_in = canon_in ? 1u : 0u;
  uint32_t* st = d_state.p + state_off;
  switch (family) {
    case SHA3: LRH_TRY(lcpc::launch_sha3_leaves_range(nl, a, blk_begin, blk_end, reinterpret_cast<uint64_t*>(st), nullptr)); break;
    case KECCAK256: LRH_TRY(lcpc::launch_keccak256_leaves_range(nl, a, blk_begin, blk_end, reinterpret_cast<uint64_t*>(st), nullptr)); break;
    case SHA256: LRH_TRY(lcpc::launch_sha256_leaves_range(nl, a, blk_begin, blk_end, st, nullptr)); break;
    default: LRH_TRY(lcpc::launch_blake2b_leaves_range(nl, a, blk_begin, blk_end, reinterpret_cast<uint64_t*>(st), nullptr)); break;
  }
  LRH_TRY(hipDeviceSynchronize());
  LRH_TRY(d_state.get(state, (size_t)state_words * 4));
  return (int)d_out.get(out, (size_t)out_words * 4);
}

// tests/native/lr_harness.cpp -- test-only C entry points over the launchers of the serial-chain digests in lcpc_amd/csrc/kernels.h
// (launch_chain_leaves, launch_chain_leaves_batch, launch_chain_leaves_range, launch_chain_merkle_tree[_batch]), so that a test can hand a
// kernel a commitment matrix that ends where a row batch ends, a block range, a chaining-state buffer, member strides and a hashes array
// of its own making (tests/lr_harness.py, tests/test_gpu_leaf_range.py, tests/test_gpu_chain_direct.py).  Built by lcpc_amd/csrc/Makefile
// into lcpc_amd/lib/liblcpc_lr_harness.so and linked against the product library, which gains nothing by it.
//
// A wrapper takes HOST pointers, checks that every index the kernel will form stays inside the buffers it was given (a refused call
// returns H_BAD_ARGS and launches nothing), allocates device buffers, copies in, launches on the null stream, synchronises, copies the
// output buffers back whole and frees.  The return value is the first hipError_t.  Output buffers are copied in first and back whole, so
// the caller sees what was written outside the expected region too (sentinel fill).
#include "harness.h"
#include "../../lcpc_amd/csrc/kernels.h"

namespace {

constexpr uint64_t MAX_DIM = (uint64_t)1 << 28;      // rows, columns, strides: far above any test, far below 64-bit overflow of a product

// family: 0 SHA3-256, 1 Keccak-256, 2 SHA-256, 3 BLAKE2b
bool shape_of(int family, int nl, uint64_t n_rows_total, lcpc::ChainHash* h, lcpc::ChainShape* s) {
  if (family < 0 || family > 3 || !nl_ok(nl)) return false;
  *h = static_cast<lcpc::ChainHash>(family);
  *s = lcpc::chain_shape(*h, nl, n_rows_total);
  return true;
}
static_assert((int)lcpc::ChainHash::Sha3_256 == 0 && (int)lcpc::ChainHash::Keccak256 == 1 && (int)lcpc::ChainHash::Sha256 == 2 &&
              (int)lcpc::ChainHash::Blake2b == 3, "tests/lr_harness.py FAMILY");

// the furthest element a launch over the whole message addresses lies inside comm_elems
bool comm_holds(uint64_t comm_elems, uint64_t row_stride, uint64_t col_stride, uint64_t n_cols, uint64_t last_row) {
  return last_row * row_stride + (n_cols - 1) * col_stride < comm_elems;
}

}  // namespace

H_DEVICE_COUNT(lrh_)

// blocks of the whole leaf message (0: family or nl unknown)
H_EXPORT uint64_t lrh_leaf_blocks(int family, int nl, uint64_t n_rows_total) {
  lcpc::ChainHash h;
  lcpc::ChainShape s;
  return n_rows_total <= MAX_DIM && shape_of(family, nl, n_rows_total, &h, &s) ? s.n_blocks : 0;
}

// one launch of blocks [blk_begin, blk_end).  comm: comm_elems elements, element (r, c) at r row_stride + c col_stride (row 0 is the
// message's first row); it has to hold every row the range's blocks carry bytes of and nothing more.  state (in / out): state_words
// 32-bit words, the kernel's region starting at word state_off (even: the sponge and BLAKE2b states are 64-bit words); out (in / out):
// out_words words, the digests starting at word out_off (a multiple of 4: the digest stores are 16 bytes wide)
H_EXPORT int lrh_leaf_range(int family, int nl, const uint32_t* comm, uint64_t comm_elems, uint64_t row_stride, uint64_t col_stride,
                            uint64_t n_cols, uint64_t n_rows_total, uint64_t blk_begin, uint64_t blk_end, int canon_in, uint32_t* state,
                            uint64_t state_words, uint64_t state_off, uint32_t* out, uint64_t out_words, uint64_t out_off) {
  lcpc::ChainHash h;
  lcpc::ChainShape s;
  if (!n_cols || !n_rows_total || n_cols > MAX_DIM || n_rows_total > MAX_DIM || row_stride > MAX_DIM || col_stride > MAX_DIM ||
      comm_elems > (MAX_DIM << 4) || !shape_of(family, nl, n_rows_total, &h, &s)) return H_BAD_ARGS;
  if (blk_begin > blk_end || blk_end > s.n_blocks) return H_BAD_ARGS;
  if (!comm || !state || !out) return H_BAD_ARGS;
  if (state_words > (MAX_DIM << 6) || (state_off & 1) || state_off > state_words || (uint64_t)s.state_words * n_cols > state_words - state_off) return H_BAD_ARGS;
  if (out_words > (MAX_DIM << 6) || (out_off & 3) || out_off > out_words || (uint64_t)s.digest_words * n_cols > out_words - out_off) return H_BAD_ARGS;
  // the rows whose limbs lie in words [block_words blk_begin, block_words blk_end) of the message: the furthest element of them is the
  // furthest the launch addresses (rows >= n_rows_total are the zero words of the padding and are not loaded)
  const uint64_t L = (uint64_t)nl / 2, w1 = (uint64_t)s.block_words * blk_end;
  if (blk_end > blk_begin && w1 > s.prefix_words) {
    uint64_t last = (w1 - s.prefix_words - 1) / L;
    if (last >= n_rows_total) last = n_rows_total - 1;
    if (!comm_holds(comm_elems, row_stride, col_stride, n_cols, last)) return H_BAD_ARGS;
  }
  DevBuf d_comm, d_state, d_out;
  H_TRY(d_comm.put(comm, (size_t)comm_elems * nl * 4));
  H_TRY(d_state.put(state, (size_t)state_words * 4));
  H_TRY(d_out.put(out, (size_t)out_words * 4));
  lcpc::LeafArgs a{};
  a.comm = d_comm.p; a.row_stride = row_stride; a.col_stride = col_stride; a.n_cols = n_cols; a.row_base = 0; a.n_rows_total = n_rows_total;
  a.out = d_out.p + out_off; a.canon_in = canon_in ? 1u : 0u;
  H_TRY(lcpc::launch_chain_leaves_range(h, nl, a, blk_begin, blk_end, d_state.p + state_off, nullptr));
  H_TRY(hipDeviceSynchronize());
  H_TRY(d_state.get(state, (size_t)state_words * 4));
  return (int)d_out.get(out, (size_t)out_words * 4);
}

// the one-shot column hash (n_batch == 0: launch_chain_leaves) or its batch form (n_batch >= 1: launch_chain_leaves_batch) over the
// whole message.  Member i's comm starts i * comm_stride 32-bit words behind member 0's (a multiple of 4), its digests at word
// out_off + i * out_stride of out (both multiples of 4); comm: comm_words 32-bit words in all, a member's element (r, c) at
// r row_stride + c col_stride elements.  Members may not overlap.  A call the launcher refuses (nl == 8, canon_in == 0 in batch form)
// comes back as its hipError_t, with out copied back as it then is
H_EXPORT int lrh_leaves(int family, int nl, const uint32_t* comm, uint64_t comm_words, uint64_t row_stride, uint64_t col_stride, uint64_t n_cols,
                        uint64_t n_rows_total, int canon_in, uint32_t n_batch, uint64_t comm_stride, uint64_t out_stride, uint32_t* out,
                        uint64_t out_words, uint64_t out_off) {
  lcpc::ChainHash h;
  lcpc::ChainShape s;
  if (!n_cols || !n_rows_total || n_cols > MAX_DIM || n_rows_total > MAX_DIM || row_stride > MAX_DIM || col_stride > MAX_DIM ||
      comm_words > (MAX_DIM << 6) || out_words > (MAX_DIM << 6) || n_batch > 1024 || comm_stride > (MAX_DIM << 6) || out_stride > (MAX_DIM << 6) ||
      !shape_of(family, nl, n_rows_total, &h, &s) || !comm || !out) return H_BAD_ARGS;
  const uint64_t members = n_batch ? n_batch : 1;
  const uint64_t ext_comm = ((n_rows_total - 1) * row_stride + (n_cols - 1) * col_stride + 1) * (uint64_t)nl, ext_out = (uint64_t)s.digest_words * n_cols;
  if ((comm_stride & 3) || (out_stride & 3) || (out_off & 3) || out_off > out_words) return H_BAD_ARGS;
  if (members > 1 && (comm_stride < ext_comm || out_stride < ext_out)) return H_BAD_ARGS;
  if ((members - 1) * comm_stride + ext_comm > comm_words || (members - 1) * out_stride + ext_out > out_words - out_off) return H_BAD_ARGS;
  DevBuf d_comm, d_out;
  H_TRY(d_comm.put(comm, (size_t)comm_words * 4));
  H_TRY(d_out.put(out, (size_t)out_words * 4));
  lcpc::LeafArgs a{};
  a.comm = d_comm.p; a.row_stride = row_stride; a.col_stride = col_stride; a.n_cols = n_cols; a.row_base = 0; a.n_rows_total = n_rows_total;
  a.out = d_out.p + out_off; a.canon_in = canon_in ? 1u : 0u;
  const hipError_t e = n_batch ? lcpc::launch_chain_leaves_batch(h, nl, a, n_batch, comm_stride, out_stride, nullptr) : lcpc::launch_chain_leaves(h, nl, a, nullptr);
  H_TRY(hipDeviceSynchronize());
  H_TRY(d_out.get(out, (size_t)out_words * 4));
  return (int)e;
}

// the tree above np2 leaf digests (n_batch == 0: launch_chain_merkle_tree; n_batch >= 1: launch_chain_merkle_tree_batch).  hashes (in /
// out): hashes_words words, member i's [2 np2 - 1][digest_words] array starting at word hashes_off + i * hashes_stride (multiples of 4);
// root (in / out, may be null: the launcher gets a null root_out): root_words words, member i's root at word root_off + i digest_words
H_EXPORT int lrh_merkle_tree(int family, uint64_t np2, uint32_t n_batch, uint64_t hashes_stride, uint32_t* hashes, uint64_t hashes_words,
                             uint64_t hashes_off, uint32_t* root, uint64_t root_words, uint64_t root_off) {
  lcpc::ChainHash h;
  lcpc::ChainShape s;
  if (!shape_of(family, 2, 1, &h, &s) || !hashes || np2 < 2 || np2 > ((uint64_t)1 << 20) || (np2 & (np2 - 1)) || n_batch > 1024 ||
      hashes_words > (MAX_DIM << 6) || hashes_stride > (MAX_DIM << 6) || root_words > (MAX_DIM << 6)) return H_BAD_ARGS;
  const uint64_t members = n_batch ? n_batch : 1, ext = (2 * np2 - 1) * s.digest_words;
  if ((hashes_stride & 3) || (hashes_off & 3) || hashes_off > hashes_words || (members > 1 && hashes_stride < ext)) return H_BAD_ARGS;
  if ((members - 1) * hashes_stride + ext > hashes_words - hashes_off) return H_BAD_ARGS;
  if (root && (root_off > root_words || members * s.digest_words > root_words - root_off)) return H_BAD_ARGS;
  DevBuf d_hashes, d_root;
  H_TRY(d_hashes.put(hashes, (size_t)hashes_words * 4));
  if (root) H_TRY(d_root.put(root, (size_t)root_words * 4));
  uint32_t* r = root ? d_root.p + root_off : nullptr;
  const hipError_t e = n_batch ? lcpc::launch_chain_merkle_tree_batch(h, d_hashes.p + hashes_off, np2, n_batch, hashes_stride, nullptr, r)
                               : lcpc::launch_chain_merkle_tree(h, d_hashes.p + hashes_off, np2, nullptr, r);
  H_TRY(hipDeviceSynchronize());
  H_TRY(d_hashes.get(hashes, (size_t)hashes_words * 4));
  if (root) H_TRY(d_root.get(root, (size_t)root_words * 4));
  return (int)e;
}

// tests/native/k8_harness.cpp -- test-only C entry points over the Merkle path folds of the batched verify and the column check (K8b:
// launch_fold_paths_b3 / launch_chain_fold_paths of lcpc_amd/csrc/kernels.h), in the manner of k7_harness.cpp: built by
// lcpc_amd/csrc/Makefile into lcpc_amd/lib/liblcpc_k8_harness.so and linked against the product library, which gains nothing by it
// (tests/k8_harness.py, tests/test_gpu_k8_kernels.py).
//
// k8h_fold_paths takes HOST pointers and the sizes of the buffers behind them, checks that every index the kernel will form stays
// inside them (a refused call returns H_BAD_ARGS and launches nothing), allocates device buffers, copies in, launches on the null
// stream, synchronises and copies the status words back.  k8h_refusal hands the launcher arguments it must settle BEFORE any launch,
// with null or never-read buffers: it touches no device.
#include "harness.h"
#include "../../lcpc_amd/csrc/kernels.h"

namespace {

// a cap of its own, a quarter of harness.h's MAX_WORDS: it bounds the strides too, which the index checks below multiply by the batch
constexpr uint64_t MAX_FOLD_WORDS = (uint64_t)1 << 26;

// digest: 0 BLAKE3, 1 SHA3-256, 2 Keccak-256, 3 SHA-256, 4 BLAKE2b
bool digest_ok(int d) { return d >= 0 && d <= 4; }
uint32_t digest_words(int d) { return d == 4 ? 16 : 8; }
hipError_t launch(int d, const lcpc::FoldPathsArgs& a) {
  switch (d) {
    case 0: return lcpc::launch_fold_paths_b3(a, nullptr);
    case 1: return lcpc::launch_chain_fold_paths(lcpc::ChainHash::Sha3_256, a, nullptr);
    case 2: return lcpc::launch_chain_fold_paths(lcpc::ChainHash::Keccak256, a, nullptr);
    case 3: return lcpc::launch_chain_fold_paths(lcpc::ChainHash::Sha256, a, nullptr);
    default: return lcpc::launch_chain_fold_paths(lcpc::ChainHash::Blake2b, a, nullptr);
  }
}

}  // namespace

H_DEVICE_COUNT(k8h_)

// leaves: leaves_words words, member m's digests at m * leaves_stride; drawn [n_batch][n_open]; sibs: sibs_words words, the sibling of
// (m, k, lvl) at m * sib_member + k * sib_col + lvl * sib_lvl; roots [n_batch][DW]; status: status_words words, in / out, member m's
// at m * status_stride (a test pre-fills it to see what is written)
H_EXPORT int k8h_fold_paths(int digest, const uint32_t* leaves, uint64_t leaves_words, uint64_t leaves_stride, const uint64_t* drawn,
                            const uint32_t* sibs, uint64_t sibs_words, uint64_t sib_member, uint64_t sib_col, uint64_t sib_lvl,
                            const uint32_t* roots, uint32_t* status, uint64_t status_words, uint64_t status_stride, uint32_t n_open,
                            uint32_t depth, uint32_t n_batch) {
  if (!digest_ok(digest) || !n_batch || n_batch > 65535 || !n_open || depth > 63) return H_BAD_ARGS;
  if (!leaves || !drawn || !sibs || !roots || !status) return H_BAD_ARGS;
  const uint64_t dw = digest_words(digest);
  if (leaves_words > MAX_FOLD_WORDS || sibs_words > MAX_FOLD_WORDS || status_words > MAX_FOLD_WORDS) return H_BAD_ARGS;
  if (leaves_stride > MAX_FOLD_WORDS || sib_member > MAX_FOLD_WORDS || sib_col > MAX_FOLD_WORDS || sib_lvl > MAX_FOLD_WORDS || status_stride > MAX_FOLD_WORDS) return H_BAD_ARGS;
  // the kernel moves digests as uint4
  if (leaves_stride % 4 || sib_member % 4 || sib_col % 4 || sib_lvl % 4) return H_BAD_ARGS;
  // the last word of every kind the kernel forms
  const uint64_t mb = n_batch - 1, kb = n_open - 1;
  if (mb * leaves_stride + kb * dw + dw > leaves_words) return H_BAD_ARGS;
  if (mb * status_stride + kb + 1 > status_words) return H_BAD_ARGS;
  if (depth && mb * sib_member + kb * sib_col + (uint64_t)(depth - 1) * sib_lvl + dw > sibs_words) return H_BAD_ARGS;
  DevBuf d_leaves, d_drawn, d_sibs, d_roots, d_status;
  H_TRY(d_leaves.put(leaves, leaves_words * 4));
  H_TRY(d_drawn.put(drawn, (size_t)n_batch * n_open * 8));
  H_TRY(d_sibs.put(sibs, sibs_words * 4));
  H_TRY(d_roots.put(roots, (size_t)n_batch * dw * 4));
  H_TRY(d_status.put(status, status_words * 4));
  lcpc::FoldPathsArgs a{};
  a.leaves = d_leaves.p; a.leaves_stride = leaves_stride; a.drawn = reinterpret_cast<const uint64_t*>(d_drawn.p);
  a.sibs = d_sibs.p; a.sib_member = sib_member; a.sib_col = sib_col; a.sib_lvl = sib_lvl;
  a.roots = d_roots.p; a.status = d_status.p; a.status_stride = status_stride;
  a.n_open = n_open; a.depth = depth; a.n_batch = n_batch;
  H_TRY(launch(digest, a));
  H_TRY(hipDeviceSynchronize());
  return (int)d_status.get(status, status_words * 4);
}

// What the launcher answers to a job it must settle before any launch -- so this refuses (H_BAD_ARGS) every job a correct launcher
// would launch: only n_batch == 0 or > 65535, depth > 63, n_open == 0 and a null buffer get through.  null_mask: bit 0 leaves, 1 drawn,
// 2 sibs, 3 roots, 4 status are NULL; the others point at words nothing reads.  Returns the launcher's hipError_t.
H_EXPORT int k8h_refusal(int digest, uint32_t n_batch, uint32_t n_open, uint32_t depth, uint32_t null_mask) {
  if (!digest_ok(digest)) return H_BAD_ARGS;
  const bool settled = n_batch == 0 || n_batch > 65535 || depth > 63 || n_open == 0 || (null_mask & 31u) != 0;
  if (!settled) return H_BAD_ARGS;
  alignas(16) static uint32_t dummy[16];
  lcpc::FoldPathsArgs a{};
  a.leaves = (null_mask & 1u) ? nullptr : dummy;
  a.drawn = (null_mask & 2u) ? nullptr : reinterpret_cast<const uint64_t*>(dummy);
  a.sibs = (null_mask & 4u) ? nullptr : dummy;
  a.roots = (null_mask & 8u) ? nullptr : dummy;
  a.status = (null_mask & 16u) ? nullptr : dummy;
  a.n_open = n_open; a.depth = depth; a.n_batch = n_batch;
  return (int)launch(digest, a);
}

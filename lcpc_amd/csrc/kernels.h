// lcpc_amd/csrc/kernels.h -- host-callable launchers for the gfx950 kernels (kernels.hip).
// Element pointers are `const uint32_t*` views of the L x u64 Montgomery limbs (NL = 2L words).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace lcpc {

// an element width the launchers know (NL = 2, 4, 6 or 8 words), and what those of eval.hip, fft.hip, domain.hip and quot.hip ask of an
// element pointer: aligned for the widest load of an element
inline bool nl_ok(int nl) { return nl == 2 || nl == 4 || nl == 6 || nl == 8; }
inline bool elem_aligned(const void* p, int nl) { return reinterpret_cast<uintptr_t>(p) % (nl % 4 == 0 ? 16 : 8) == 0; }

struct NttPassArgs {
  const uint32_t* src;     // row-major, src_stride elements per row
  uint32_t* dst;           // row-major, dst_stride elements per row (may alias src when strides match)
  const uint32_t* roots;   // roots[i] = w^i (Montgomery), i < n/2
  const uint32_t* roots29; // Ft255 only: w^i * 2^261 mod p as 9 x 29-bit limbs, 12-word stride (fe_mul_r29)
  const uint32_t* qp29;    // Ft255 only: q*p (q < 32) as 9 x 29-bit limbs, 12-word stride; non-null selects the lazy-limb kernel
  const uint32_t* roots29c;// lazy-limb kernel only, may be null: w^i * 2^5 mod p, same layout.  Non-null = "canonical output":
                           // src is in Montgomery form, dst of the final pass holds canonical values (see ntt_pass_l9_kernel)
  uint32_t mont_prefix;    // canonical output, final pass: elements [0, mont_prefix) of a row never met a multiplier and are
                           // converted at the store
  uint64_t src_stride, dst_stride;
  uint64_t n_valid;        // elements >= n_valid of every src row read as zero (fused zero padding)
  uint64_t n_src_total;    // flat src elements >= n_src_total read as zero (ragged last row)
  uint32_t* copy_dst;      // if non-null (first pass): padded copy of src, same strides (LcCommit.coeffs)
  uint64_t n_rows;
  uint32_t log_n, t0, s, log_tj;   // stages [t0, t0+s) on tiles of 2^s x 2^log_tj elements
  uint32_t* mid = nullptr; // shape-specialised two-pass kernel only, may be null: the 29-bit-limb intermediate between the passes
                           // (n_rows x n_cols x 36 bytes, layout in ntt_l9s.hip); the first pass writes it instead of dst, the
                           // last pass reads it instead of src
  uint32_t canon_row_mask = 0; // canonical output (roots29c != null) applies to the rows r with (r & canon_row_mask) == 0 only: the
                           // three-pass plan runs its last two passes on n_rows << s0 sub-rows of 2^20 elements, of which only every
                           // 2^s0-th still holds never-multiplied elements (ntt_l9s.hip)
  uint32_t blk0_gone = 0;  // shape-specialised kernel, canonical output: an earlier pass converted the last never-multiplied elements
                           // (the round before its uniform round): this pass sees canonical values only
  const uint32_t* wq_w = nullptr;  // shape-specialised last pass (ntt_l9s.hip): the shifted multiples of w^(n/4) (81 words, ctx.cpp wmul_table), the
                           // one wave-uniform twiddle of the transform (stages k-2, k-1); null: the Montgomery-form table entry
  uint32_t tile_group = 0; // shape-specialised first pass (ntt_l9s.hip, ntt_lns.hip): 2^tile_group neighbouring tiles of a row are
                           // consecutive workgroups of one XCD (short strided runs then meet in that L2); needs
                           // tiles_per_row >= 8 << tile_group
  uint32_t form = 0;       // K1s two-pass plans (ntt_l9s.hip): 0 = DIF with the twist on the first pass, 1 = pure first pass and coset-form
                           // last pass; the packs differ (launch_ntt_l9s_form_pack), the results do not
};
hipError_t launch_ntt_pass(int nl, int log_tile, const NttPassArgs& a, hipStream_t st);

// ---- shape-specialised Ft255 NTT for two-pass plans on 1024-element tiles (ntt_l9s.hip) ----
// twiddle pack of one pass: per tile class, per round, the table entries in lane order (layout: ntt_ln_dev.h; built by
// launch_ntt_lns_pack for all four fields)
struct NttPackInfo {
  uint32_t round_off[8];    // word offset of round slot r inside a class block
  uint32_t class_words;     // words per tile class
  uint32_t u_off;           // passes with a uniform round (ntt_ln_dev.h Shape::RU): word offset of its 4 x 3 shifted-multiples tables
  uint32_t mul2;            // K1s pure / coset form only: 1 = every lane-varying slot holds the two-table pair of ln::mul2 (twice the
                            // variants: b0 of variant v at v, b1 at NV + v) and the pass kernel multiplies by it; 0 = ln::mul entries
};
bool ntt_l9s_supported(uint32_t log_n, uint32_t n_passes, int log_tile);
// three passes for 2^21 .. 2^26 columns: s0 = log_n - 20 stages with the first-pass kernel on the whole rows (element stride 2^20),
// then the two-pass plan of a 2^20-point transform on each of the 2^s0 contiguous blocks of every row (DIF: after s0 stages the
// blocks are independent transforms with the root w^(2^s0)), from a sub-sampled twiddle table
bool ntt_l9s3_supported(uint32_t log_n);
hipError_t launch_ntt_pass_l9s(const NttPassArgs& a, bool first, const uint32_t* pack, const NttPackInfo& pi, hipStream_t st);
// the packs of the pure / coset form (NttPassArgs.form == 1; built in ntt_lns.hip beside the other packs).  First pass: one class;
// last pass: one class per tile position, 2^(log_n - 10).  a: log_n, s, roots29, roots29c
NttPackInfo ntt_l9s_form_pack_info(uint32_t s, bool first, bool mul2);
// mul2 (NttPackInfo.mul2, ln::mul2 on two-table packs) exists for these passes of the pure / coset form only: the coset pass, and the
// pure passes but S = 2 (2^12 columns: no lane-varying round, I alone) and S = 7, 9 (2^17, 2^19 columns), which are not built: with 18
// words per twiddle the ln::mul2 builds of <7, 3, first, packed intermediate> and of both <9, 1, first> need 12 / 12 / 20 bytes of scratch
// per lane at 128 VGPRs, where every other ln::mul2 build needs none.  (The ln::mul builds of <9, 1, first, packed intermediate> carry 12 /
// 20 bytes as well, DIF / pure form: those are what the plan ran before and runs still; they are not a reason to add spilling kernels.)
// One predicate for the launcher's instantiations (ntt_l9s.hip) and the plan (ctx.cpp)
constexpr bool ntt_l9s_mul2_supported(uint32_t s, bool first) { return !first ? s == 10 : (s >= 1 && s <= 10 && s != 2 && s != 7 && s != 9); }
hipError_t launch_ntt_l9s_form_pack(const NttPassArgs& a, bool first, const NttPackInfo& pi, uint32_t n_classes, uint32_t* pack, hipStream_t st);

// ---- shape-specialised lazy-limb NTT for Ft63 / Ft127 / Ft191, two-pass plans on 1024-element tiles (ntt_lns.hip) ----
// nl = 2 / 4 / 6.  a.roots29 = the limb-form twiddle table (w^i R' mod p, ntt_lns_stride words per entry), a.qp29 = the
// (i - 24) p table (64 rows, same stride)
bool ntt_lns_supported(int nl, uint32_t log_n);
// three passes for 2^21 .. 2^26 columns, built like ntt_l9s3_supported's plan (first-pass kernel over the whole rows, then the
// 2^20-point two-pass plan per block from sub-sampled tables)
bool ntt_lns3_supported(int nl, uint32_t log_n);
hipError_t launch_ntt_pass_lns(int nl, const NttPassArgs& a, bool first, const uint32_t* pack, const NttPackInfo& pi, hipStream_t st);
// the table side of both plan families, nl = 2 / 4 / 6 / 8 (Ft255: N = 9, W = 29, 12-word entries):
int ntt_lns_limbs(int nl);          // N
int ntt_lns_limb_bits(int nl);      // W
int ntt_lns_stride(int nl);         // words per table entry
// sub[i] = tab[i << shift], i < n
hipError_t launch_ntt_lns_subtable(int nl, const uint32_t* tab, uint32_t shift, uint64_t n, uint32_t* sub, hipStream_t st);
NttPackInfo ntt_lns_pack_info(int nl, uint32_t s, bool first);
hipError_t launch_ntt_lns_roots(int nl, const uint32_t* roots, uint64_t n, const uint32_t* rprime, uint32_t* out, hipStream_t st);
// a: the pass (log_n, t0, s, log_tj, roots29, roots29c); first pass: n_classes = tiles per row, last pass: 1
hipError_t launch_ntt_lns_pack(int nl, const NttPassArgs& a, bool first, const NttPackInfo& pi, uint32_t n_classes, uint32_t* pack, hipStream_t st);

// device-side precomp_fft: roots[i] = w^i (i < 2^log_half) from pw[j] = w^(2^j); roots29 (Ft255) may be null
hipError_t launch_roots(int nl, const uint32_t* pw, uint32_t log_half, const uint32_t* one, uint32_t* roots, uint32_t* roots29,
                        uint32_t* roots29c, hipStream_t st);

struct LeafArgs {
  const uint32_t* comm;        // local rows, row-major
  uint64_t row_stride;         // elements between consecutive rows of a column (n_cols for the row-major comm)
  uint64_t col_stride;         // elements between consecutive columns of a row (1 for row-major; n_rows for a position-major copy)
  uint64_t n_cols;
  int64_t  row_base;           // global index of local row 0
  uint64_t n_rows_total;
  uint32_t chunk_begin, n_chunks_local, n_chunks_total;
  uint32_t* out;               // n_chunks_total == 1: digests [n_cols][8]; else CVs [n_chunks_local][n_cols][8]
  uint32_t canon_in;           // comm already holds canonical values (Ft255 Ligero commit): no Montgomery reduction here
};
hipError_t launch_leaf_chunks(int nl, const LeafArgs& a, hipStream_t st);
// cvs [n_chunks][n_cols][8] (clobbered: used as the BLAKE3 CV stack) -> digests [n_cols][8]
hipError_t launch_leaf_finish(uint32_t* cvs, uint32_t n_chunks, uint64_t n_cols, uint32_t* digests, hipStream_t st);
// general form: node j = aligned subtree of 2^node_log[j] chunks, CV at cvs[node_slot[j]][col] (tables on the device,
// nullptr = identity / all zero); root = false only pre-merges (no ROOT flag) into one subtree CV per column
hipError_t launch_leaf_finish_nodes(uint32_t* cvs, const uint32_t* node_slot, const uint32_t* node_log, uint32_t n_nodes,
                                    uint64_t n_cols, uint32_t* out, bool root, hipStream_t st);
// whole tree above the leaf layer in as few launches as possible (hashes = LcCommit.hashes, np2 leaves)
// root_out (may be null): 8 more words the root is written to by the launch that produces it (host-mapped memory)
hipError_t launch_merkle_tree(uint32_t* hashes, uint64_t np2, hipStream_t st, uint32_t* root_out);
hipError_t launch_merkle_tree_from(uint32_t* hashes, uint64_t np2, uint32_t levels_done, hipStream_t st, uint32_t* root_out);
// small commitments: leaf digests (<= 2 chunks per leaf message) AND the first six tree levels in one launch (np2 == n_cols,
// n_cols % 64 == 0, n_cols >= 128, n_cols * n_chunks <= 65536); follow with launch_merkle_tree_from(.., 6, ..)
bool leaf_tree_supported(const LeafArgs& a, uint64_t np2);
hipError_t launch_leaf_tree(int nl, const LeafArgs& a, uint32_t* hashes, uint64_t np2, hipStream_t st);

// ---- batched BLAKE3 column hash and tree (kernels.hip K3b / K4b: the K3 / K4 kernels' BATCH = true forms): n_batch <= 65535 equal-shape commitments of one encoder in one
// launch each, the member index a grid dimension.  `a`, `hashes`, `cvs`, `digests` describe member 0; member i's comm, a.out, hashes,
// cvs and digests start i * (the given stride, in 32-bit words) behind it.  Same digests as the single launchers, bit for bit.
// Alignment: every stride must be a multiple of 4 words (16 bytes), and member 0's pointers 16-byte aligned as for the single launchers --
// the kernels move chaining values and digests as uint4 and load elements 8 or 16 bytes at a time (fe_load), at the member's offset.
// A stride must be at least one member's extent: nothing here checks that members do not overlap.
hipError_t launch_leaf_chunks_batch(int nl, const LeafArgs& a, uint32_t n_batch, uint64_t comm_stride, uint64_t out_stride, hipStream_t st);
hipError_t launch_leaf_finish_batch(uint32_t* cvs, uint32_t n_chunks, uint64_t n_cols, uint32_t* digests, uint32_t n_batch, uint64_t cvs_stride,
                                    uint64_t digests_stride, hipStream_t st);
hipError_t launch_leaf_tree_batch(int nl, const LeafArgs& a, uint32_t* hashes, uint64_t np2, uint32_t n_batch, uint64_t comm_stride,
                                  uint64_t hashes_stride, hipStream_t st);
// root_out (may be null): [n_batch][8] words, member i's root written by the launch that produces it (host-mapped memory)
hipError_t launch_merkle_tree_from_batch(uint32_t* hashes, uint64_t np2, uint32_t levels_done, uint32_t n_batch, uint64_t hashes_stride,
                                         hipStream_t st, uint32_t* root_out);
// member i: n_valid 64-bit words from src + i * src_stride -> dst + i * dst_stride, the rest of its dst_stride words zero (strides in
// 64-bit words; n_valid <= both)
hipError_t launch_batch_place(const uint64_t* src, uint64_t src_stride, uint64_t n_valid, uint64_t* dst, uint64_t dst_stride, uint32_t n_batch,
                              hipStream_t st);

// ---- the serial-chain digests SHA3-256, Keccak-256, SHA-256 and BLAKE2b (chain.hip; kernels: chain_dev.h over the traits of keccak_dev.h,
// sha256_dev.h, blake2b_dev.h; instantiated in sha3.hip, sha256.hip, blake2b.hip): the same leaves and tree for an encoder built with
// LCPC_HASH_SHA3_256 / _KECCAK256 / _SHA256 / _BLAKE2B.  Keccak-256 is SHA3-256 with the padding's first byte 0x01 instead of 0x06.
enum class ChainHash { Sha3_256, Keccak256, Sha256, Blake2b };
// the leaf message of n_rows_total rows: zero prefix and block in 64-bit words, a column's chaining value and a digest (a hashes slot, a
// root, a path entry) in 32-bit words, the blocks of the whole message, padding blocks included.  nl = 2 / 4 / 6 / 8
struct ChainShape { uint32_t prefix_words, block_words, state_words, digest_words; uint64_t n_blocks; };
constexpr ChainShape chain_shape(ChainHash h, int nl, uint64_t n_rows_total) {
  const uint64_t L = (uint64_t)(nl / 2);
  switch (h) {
    case ChainHash::Sha256: { const uint64_t w = 4 + L * n_rows_total; return {4, 8, 8, 8, w / 8 + 1 + ((w & 7) == 7 ? 1 : 0)}; }
    case ChainHash::Blake2b: return {8, 16, 16, 16, (8 + L * n_rows_total + 15) / 16};
    default: return {4, 17, 50, 8, (4 + L * n_rows_total) / 17 + 1};          // the two sponges
  }
}
// leaf digests [n_cols][digest_words] of the whole column (a.n_chunks_* unused: a chain is not split); a.out = LcCommit.hashes
hipError_t launch_chain_leaves(ChainHash h, int nl, const LeafArgs& a, hipStream_t st);
// the whole tree above the np2 leaf digests; root_out (may be null): digest_words more words the root is written to by the launch that
// produces it (host-mapped memory)
hipError_t launch_chain_merkle_tree(ChainHash h, uint32_t* hashes, uint64_t np2, hipStream_t st, uint32_t* root_out);

// The batch forms: n_batch <= 65535 members with the member index a grid dimension.  `a` and `hashes` describe member 0; member i's comm,
// a.out and hashes start i * (the given stride, in 32-bit words) behind it.  Same digests as the single launchers, bit for bit; alignment
// and stride rules as for the BLAKE3 batch launchers above.  Empty work (n_batch == 0, no columns) is hipSuccess; nl == 8 with
// a.canon_in == 0 is hipErrorInvalidValue (a Ligero comm over Ft255 is always canonical, so that kernel is not instantiated).
hipError_t launch_chain_leaves_batch(ChainHash h, int nl, const LeafArgs& a, uint32_t n_batch, uint64_t comm_stride, uint64_t out_stride,
                                     hipStream_t st);
// root_out (may be null): [n_batch][digest_words] words, member i's root written by the launch that produces it
hipError_t launch_chain_merkle_tree_batch(ChainHash h, uint32_t* hashes, uint64_t np2, uint32_t n_batch, uint64_t hashes_stride, hipStream_t st,
                                          uint32_t* root_out);

// The resumable column hash.  The same leaf message hashed a block range at a time: a launch runs blocks [blk_begin, blk_end) of every
// column's chain.  It starts from the IV / the zero sponge when blk_begin == 0 and from `state` otherwise; it leaves the chaining value in
// `state` when blk_end is not the message's last block and the digest in a.out (the one-shot layout) when it is.  An empty range launches
// nothing; a range past the last block is hipErrorInvalidValue.  A launch loads only the rows its blocks hold bytes of, so comm
// needs nothing behind them yet (the host-memory commit hashes behind each row batch: commit.cpp).
// state: the chaining value alone, state_words * n_cols words, 8-byte aligned, word-major so that consecutive columns are consecutive
// addresses -- word i of column c at state[i * n_cols + c]: 25 x u64 lanes (sponges), 8 x u32 (SHA-256), 8 x u64 (BLAKE2b; its byte
// counter is 128 (blk + 1)).
hipError_t launch_chain_leaves_range(ChainHash h, int nl, const LeafArgs& a, uint64_t blk_begin, uint64_t blk_end, uint32_t* state, hipStream_t st);

// ---- K5b / K6b: the batch forms for the batched prove (batch.cpp): the member index is a grid dimension ------------------------
// What differs between the members of a batch, one record per member in device memory: a member's coefficients and commitment
// matrix wherever they live.  Element (r, c) of comm at comm + (r * comm_row_stride + c * comm_col_stride) elements.
struct ProveMember {
  const uint32_t* coeffs;      // n_rows x n_per_row
  const uint32_t* comm;
  uint64_t comm_row_stride, comm_col_stride;   // row-major: n_cols, 1; position-major: 1, n_rows
  const uint32_t* hashes;      // 2 np2 - 1 digests
  uint32_t comm_canon;         // comm holds canonical values: open multiplies by R^2
};
struct CollapseArgs {
  const uint32_t* coeffs;      // local rows x n_per_row
  const uint32_t* tensors;     // [n_tensors][n_rows_local]
  const uint32_t* tensors29;   // Ft255: the same tensors as 9 x 29-bit limbs of t * 2^261 (12-word stride), or null
  uint32_t* out;               // n_splits == 1: polys [n_tensors][n_per_row]; else partial [n_splits][n_tensors][n_per_row]
  uint64_t n_rows, n_per_row;
  uint32_t n_tensors, n_splits;
  // column range [j0, j1) of this launch (j1 == 0: all of them) and the element stride between the output rows: a range's outputs sit
  // at out + ((split * n_tensors + tensor) * out_stride + (j - j0)) elements (prove collapses p_random in two ranges: commit.cpp)
  uint64_t j0 = 0, j1 = 0, out_stride = 0;
  // the batch form (K5b): members non-null -> grid z = member (n_batch <= 65535).  Member z reads members[z].coeffs (`coeffs` is not
  // read), its tensors at tensors / tensors29 + z * n_tensors * n_rows elements, and writes at out + z * n_splits * n_tensors * out_stride
  const ProveMember* members = nullptr;
  uint32_t n_batch = 0;
};
// Every launcher of K5 / K6 below settles what it will not run BEFORE any launch: empty work is hipSuccess with nothing launched, a
// job no grid can carry (or no kernel is built for) is hipErrorInvalidValue with nothing launched.  Each states its own cases.
//
// nl = 2 / 4 / 6 / 8, n_tensors = 1 or 2, 1 <= n_splits <= 65535 (grid y), j0 < j1 <= n_per_row after the defaults, and with members
// non-null 1 <= n_batch <= 65535 (grid z): anything else is hipErrorInvalidValue, checked before any launch.  A split that holds no
// row (ceil(n_rows / n_splits) * split >= n_rows) writes zeros.  Ft255 with tensors29 == null runs the Montgomery-word kernel of the
// other fields: same values, slower.
hipError_t launch_collapse(int nl, const CollapseArgs& a, hipStream_t st);
// Ft255 tensors (Montgomery) -> the 29-bit-limb / 2^261 form used by the lazy dot-product kernels: nine 29-bit limbs of 32 t mod p and
// three zero words per entry.  n == 0 is hipSuccess, nothing launched
hipError_t launch_to_r29(const uint32_t* in, uint64_t n, uint32_t* out, hipStream_t st);
// out[e] = sum_p parts[p][e] mod p.  n_elems == 0 is hipSuccess, nothing launched; otherwise n_parts == 0 or a bad nl is
// hipErrorInvalidValue, checked before any launch
hipError_t launch_field_sum(int nl, const uint32_t* parts, uint32_t n_parts, uint64_t n_elems, uint32_t* out, hipStream_t st);

// open_column: vals[k][r] = comm[r][cols[k]]; paths[k][lvl] = sibling digest.  r2 non-null: comm holds canonical
// values, multiply by R^2 on the way out so that vals are Montgomery-form elements like everything else at the ABI
// element (r, c) at comm + (r * row_stride + c * col_stride) elements (row-major comm: n_cols, 1; position-major: 1, n_rows)
// n == 0 or n_rows == 0 is hipSuccess, nothing launched; otherwise a bad nl is hipErrorInvalidValue, checked before any launch.
// n in slices of 32768 (grid y); more than 16384 rows: a grid-stride loop over 64 row blocks
hipError_t launch_gather_columns(int nl, const uint32_t* comm, uint64_t n_rows, uint64_t row_stride, uint64_t col_stride,
                                 const uint64_t* cols, uint32_t n, uint32_t* vals, const uint32_t* r2, hipStream_t st);
// elementwise representation change of n elements (in may equal out): to_mont = x * R (r2 = R^2 mod p, Montgomery
// multiply), to_canon = x * R^-1 (Montgomery reduction = PrimeField::to_repr without the byte dump)
// n == 0 is hipSuccess, nothing launched; otherwise a bad nl is hipErrorInvalidValue, checked before any launch
hipError_t launch_to_mont(int nl, const uint32_t* in, uint64_t n, const uint32_t* r2, uint32_t* out, hipStream_t st);
hipError_t launch_to_canon(int nl, const uint32_t* in, uint64_t n, uint32_t* out, hipStream_t st);
// sharded open_column: [rank][k][rows of rank] (blocks of block_words) -> [k][all rows]; rb: G + 1 row boundaries on the device
// (rb[0] = 0, non-decreasing, rb[G] = n_rows: a rank may hold no row).  n == 0 or n_rows == 0 is hipSuccess, nothing launched;
// otherwise a bad nl is hipErrorInvalidValue, checked before any launch
hipError_t launch_assemble_columns(int nl, const uint32_t* recv, uint64_t block_words, const uint64_t* rb, uint32_t G, uint32_t n,
                                   uint64_t n_rows, uint32_t* out, hipStream_t st);
// digest_words = 8 or 16 (ChainShape.digest_words; BLAKE3: 8): paths [n][path_len][digest_words]
// digest_words other than 8 or 16 is hipErrorInvalidValue, whatever else is asked; otherwise n == 0 or path_len == 0 is hipSuccess,
// nothing launched
hipError_t launch_gather_paths(const uint32_t* hashes, uint64_t np2, uint32_t path_len, const uint64_t* cols, uint32_t n,
                               uint32_t* paths, uint32_t digest_words, hipStream_t st);

// ---- K5b / K6b: the batch forms of the split sum and the gathers (the batch form of collapse: CollapseArgs.members) -------------
// out[member][e] = sum_p parts[member][p][e] mod p (member = blockIdx.y)
// n_batch == 0 or n_elems == 0 is hipSuccess, nothing launched; otherwise n_batch > 65535, n_parts == 0 or a bad nl is
// hipErrorInvalidValue, checked before any launch
hipError_t launch_field_sum_batch(int nl, const uint32_t* parts, uint32_t n_parts, uint64_t n_elems, uint32_t* out, uint32_t n_batch,
                                  hipStream_t st);
// vals[member][k][r] = comm_member[r][cols[member][k]]; grid (row blocks, opened column, member), n_open in slices of 32768.
// r2 is applied to the members whose descriptor says comm_canon
// n_batch == 0, n_open == 0 or n_rows == 0 is hipSuccess, nothing launched; otherwise n_batch > 65535 or a bad nl is
// hipErrorInvalidValue, checked before any launch
hipError_t launch_gather_columns_batch(int nl, const ProveMember* members, uint32_t n_batch, uint64_t n_rows, const uint64_t* cols,
                                       uint32_t n_open, uint32_t* vals, const uint32_t* r2, hipStream_t st);
// paths[member][k][lvl][digest_words]: one flat launch over n_batch * n_open * path_len entries
// digest_words other than 8 or 16 is hipErrorInvalidValue, whatever else is asked; otherwise an empty product is hipSuccess, nothing
// launched
hipError_t launch_gather_paths_batch(const ProveMember* members, uint32_t n_batch, uint64_t np2, uint32_t path_len, const uint64_t* cols,
                                     uint32_t n_open, uint32_t* paths, uint32_t digest_words, hipStream_t st);

// ---- K7b: the column check of the batched verify (verify_batch.cpp): verify_column_value (lib.rs:985-1000) for every opened column of
// every member and every tensor in one launch.  acc_d = sum_k tensors[d][k] * cols[i][k] mod p is compared, as a fully reduced
// Montgomery element, with enc[d][drawn[i]].  One wave per (member, opened column): the lanes run over consecutive rows of the column,
// every column element is loaded once and multiplied with up to 4 tensors (n_t > 4: again for every further 4), the lanes' partial
// sums are combined across the wave.  The member is grid dimension y; n_open is sliced at the grid limit of x.
// Alignment: cols, tensors and enc are aligned as elements are (fe_load: 16 bytes for Ft127 / Ft255, 8 for Ft63 / Ft191), tensors29 to
// 16 bytes; cols_stride counts whole elements, so every member's are.  A drawn column number >= n_cols reads nothing of enc and sets
// every bit the launch can set.
struct VerifyColsArgs {
  const uint32_t* cols;        // [member][n_open][n_rows] Montgomery elements; member stride in elements
  uint64_t cols_stride;
  const uint32_t* tensors;     // [member][n_t][n_rows]
  const uint32_t* tensors29;   // Ft255: the 29-bit-limb form (launch_to_r29), else null
  const uint32_t* enc;         // [member][n_t][n_cols] encoded rows
  const uint64_t* drawn;       // [member][n_open] column numbers
  uint32_t* status;            // [member][n_open]: bit 0 = some degree-test row differs, bit 1 = the eval row differs
  uint64_t n_rows, n_cols;
  uint32_t n_open, n_t, n_batch;   // n_t = n_deg + 1, the LAST tensor is the outer tensor
};
// nl = 2 / 4 / 6 / 8; Ft255 needs tensors29.  n_batch > 65535 or n_t == 0 with work to do is hipErrorInvalidValue, checked before
// any launch; empty work (n_batch == 0 or n_open == 0) is hipSuccess
hipError_t launch_verify_columns_batch(int nl, const VerifyColsArgs& a, hipStream_t st);

// ---- K8b: the Merkle path folds of the batched verify and of the column check (fold.cpp): verify_column_path (lib.rs:955-982) for every
// opened column of every member in one launch.  One lane per (member, opened column): h = the column's leaf digest; for lvl = 0 ..
// depth - 1: h = node(cc even ? h || sib : sib || h), cc >>= 1, cc starting at the drawn column number; h is then compared with the
// member's root.  On a mismatch the lane ORs FOLD_PATH_BIT into ITS status word (plain load, OR, store: one lane owns one word), otherwise
// the word is neither read nor written.  depth is uniform for a launch; depth == 0 compares the leaf digest with the root.  Grid: x =
// columns in blocks of 256, y = member; no LDS.
// The sibling of (member m, opened column k, level lvl) is the digest at sibs + m * sib_member + k * sib_col + lvl * sib_lvl words, so
// both layouts run without a transposition: level-major [lvl][column] (sib_col = DW, sib_lvl = n_open * DW: consecutive lanes read
// consecutive digests; what verify_batch.cpp stages) and column-major [column][lvl] (sib_col = depth * DW, sib_lvl = DW: what the core
// header's open-columns call returns).  DW = digest words, 8 or 16 (Blake2b).
// Alignment: digests move as uint4 -- every base pointer is 16-byte aligned and every stride a multiple of 4 words.  Nothing checks that
// members do not overlap.
constexpr uint32_t FOLD_PATH_BIT = 4;    // beside K7b's 1 = degree, 2 = eval
struct FoldPathsArgs {
  const uint32_t* leaves;      // [member][n_open][DW] leaf digests; member stride in words
  uint64_t leaves_stride;
  const uint64_t* drawn;       // [member][n_open] column numbers (member stride n_open)
  const uint32_t* sibs;        // the sibling base and its three word strides
  uint64_t sib_member, sib_col, sib_lvl;
  const uint32_t* roots;       // [member][DW]
  uint32_t* status;            // [member][n_open] at member stride status_stride words
  uint64_t status_stride;
  uint32_t n_open, depth, n_batch;
};
// n_batch == 0 or > 65535, depth > 63, or a null leaves / drawn / sibs / roots / status with n_open > 0 (sibs is not read when depth ==
// 0, and must still be a pointer) is hipErrorInvalidValue, checked before any launch; n_open == 0 is hipSuccess, nothing launched
hipError_t launch_fold_paths_b3(const FoldPathsArgs& a, hipStream_t st);                    // BLAKE3 (kernels.hip)
hipError_t launch_chain_fold_paths(ChainHash h, const FoldPathsArgs& a, hipStream_t st);    // the chain digests (chain_dev.h)
// what both settle before a launch: -1 = refuse, 0 = nothing to do, 1 = launch
constexpr int fold_paths_job(const FoldPathsArgs& a) {
  if (a.n_batch == 0 || a.n_batch > 65535 || a.depth > 63) return -1;
  if (a.n_open == 0) return 0;
  if (!a.leaves || !a.drawn || !a.sibs || !a.roots || !a.status) return -1;
  return 1;
}

// Brakedown: y[row][out_off + o] = sum_k vals[k] * x[row][in_off + colidx[k]], k in [rowptr[o], rowptr[o+1])
struct SpmvArgs {
  uint32_t* mat;                // comm (row-major, stride elements per row); in and out segments are disjoint
  uint32_t* out_alt;            // if non-null: write to out_alt[row][o] (stride out_alt_stride) instead of mat
  uint64_t stride, out_alt_stride;
  uint64_t in_off, out_off;
  const uint32_t* rowptr;       // [m+1]
  const uint32_t* colidx;       // [nnz]
  const uint32_t* vals;         // [nnz][NL]
  const uint32_t* vals29;       // Ft255: [nnz][12], the 29-bit-limb / 2^261 form (may be null)
  uint64_t m, n_rows;
};
hipError_t launch_spmv(int nl, const SpmvArgs& a, hipStream_t st);
// ---- position-major ("transposed") Brakedown path: T[pos][row], row fastest -----------------------
// rows x n_valid block of a row-major matrix -> T (leading dimension n_rows); and back
hipError_t launch_transpose_to_t(int nl, const uint32_t* src, uint64_t src_stride, uint64_t n_valid, uint64_t n_rows,
                                 uint32_t* t, hipStream_t st, uint64_t n_src_total = ~(uint64_t)0, uint32_t* copy_dst = nullptr,
                                 bool canon = false);   // canon: T receives canonical values (x R^-1); copy_dst the values as read
hipError_t launch_transpose_from_t(int nl, const uint32_t* t, uint64_t n_pos, uint64_t n_rows, uint32_t* dst,
                                   uint64_t dst_stride, hipStream_t st);
struct SpmmTArgs {
  uint32_t* t;                  // T[pos][row]
  uint32_t* out_alt;            // if non-null: outputs go to out_alt[o][row] instead of t[out_off + o][row]
  uint64_t n_rows;
  uint64_t in_off, out_off;
  const uint32_t* rowptr;       // [m+1]
  const uint32_t* colidx;       // [nnz]
  const uint32_t* vals;         // [nnz][NL]  Montgomery (R = 2^(32 NL))
  const uint32_t* vals29;       // Ft255: [nnz][12]  value * 2^261 mod p as 9 x 29-bit limbs (required: null is refused); Ft127 / Ft191:
                                // [nnz][8] value * R' mod p as 5 / 7 limbs, or null for the Wide<NL> path
  uint64_t m;
};
hipError_t launch_spmm_t(int nl, const SpmmTArgs& a, hipStream_t st);
hipError_t launch_sdig_rs_t(int nl, const uint32_t* in_t, uint32_t n_in, uint32_t* t, uint64_t out_off, uint32_t n_out,
                            uint64_t n_rows, const uint32_t* r2, hipStream_t st);
// ---- the same for a batch of n_batch equal-shape members (kernels.hip K2b): lane = batch row R = member * n_rows + row.  The
// arguments of the one-shot launcher describe member 0; member i's T (leading dimension n_rows, as a single commit's) starts
// i * t_stride words behind it, its out_alt / in_t i * out_alt_stride / in_stride words.  Same values as the one-shot launchers run
// member by member, bit for bit.  A stride must be at least one member's extent and keep the members' elements aligned as member
// 0's are; nothing here checks that members do not overlap.  n_batch == 0 or > 65535, or more batch rows than the grid's second
// dimension carries (65535 x 32 for the transpose, 65535 x 128 for the others), is hipErrorInvalidValue, checked before any launch;
// Ft255 with null vals29 likewise; otherwise empty work is hipSuccess.
// transpose: src is the members' rows STACKED (batch row R at src + R * src_stride elements; copy_dst likewise); n_src_total
// counts a member's own flat elements
hipError_t launch_transpose_to_t_batch(int nl, const uint32_t* src, uint64_t src_stride, uint64_t n_valid, uint64_t n_rows, uint32_t* t,
                                       uint32_t n_batch, uint64_t t_stride, hipStream_t st, uint64_t n_src_total = ~(uint64_t)0,
                                       uint32_t* copy_dst = nullptr, bool canon = false);
// launch_spmm_t's selection by m, without the packed-tail kernel: the whole batch has at most one partial wave
hipError_t launch_spmm_t_batch(int nl, const SpmmTArgs& a, uint32_t n_batch, uint64_t t_stride, uint64_t out_alt_stride, hipStream_t st);
hipError_t launch_sdig_rs_t_batch(int nl, const uint32_t* in_t, uint32_t n_in, uint32_t* t, uint64_t out_off, uint32_t n_out,
                                  uint64_t n_rows, const uint32_t* r2, uint32_t n_batch, uint64_t in_stride, uint64_t t_stride,
                                  hipStream_t st);

// Reed-Solomon base case (encode.rs:97-110): out[row][out_off + k] = sum_j in[row][j] (k+1)^j
hipError_t launch_sdig_rs(int nl, const uint32_t* in, uint64_t in_stride, uint32_t n_in, uint32_t* mat, uint64_t stride,
                          uint64_t out_off, uint32_t n_out, uint64_t n_rows, const uint32_t* r2, hipStream_t st);
// copy rows: dst[row][0..n_valid) = src[row][..]; the rest of a dst row is not written (Brakedown row setup: the encode fills it)
hipError_t launch_pad_rows(int nl, const uint32_t* src, uint64_t src_stride, uint32_t* dst, uint64_t dst_stride,
                           uint64_t n_valid, uint64_t n_rows, hipStream_t st);

// K9 (ints.hip): n plain integers of `kind` -> out[n][nl], the Montgomery forms of v mod p (r2 = R^2 mod p on the device).  The kinds
// are lcpci_kind's values (include/lcpc_hip_ints.h); an element of the input is ints_elem_bytes wide and needs that alignment only
// (WIDE: 8), `out` that of an element array (16 bytes; 8 where nl is 2 or 6).  One element per lane, the grid sized to n.  in == out
// is allowed where the two element sizes are equal (a lane reads its element before it writes it).
// n == 0 is hipSuccess, nothing launched; otherwise a bad nl or kind, a misaligned pointer or n >= 2^39 is hipErrorInvalidValue,
// checked before the launch
enum : int { INTS_U32 = 0, INTS_I32 = 1, INTS_U64 = 2, INTS_I64 = 3, INTS_WIDE = 4 };
inline size_t ints_elem_bytes(int kind, int L) { return kind <= INTS_I32 ? 4 : kind <= INTS_I64 ? 8 : (size_t)8 * L; }
hipError_t launch_from_ints(int nl, int kind, const void* in, uint64_t n, const uint32_t* r2, uint32_t* out, hipStream_t st);

// K10 (eval.hip): the tensors of an opening from points.  The bases are lcpce_basis's values (include/lcpc_hip_eval.h); every basis is
// out[i] = product over k < n_bits of (bit k of i * stride ? hi_k : lo_k).  `one` is R mod p as nl words in HOST memory (it travels
// as a kernel argument); points, the table and the outputs are device arrays of elements, aligned as such (16 bytes; 8 where nl is
// 2 or 6).  Points must be fully reduced; the outputs then are.
// Step 1, one lane per point: tab[n_points][n_bits][2][nl] = the pairs (lo_k, hi_k) of every point, the points n_point elements
// apart.  EVAL_POWERS: (1, x^(2^k)), n_point == 1; EVAL_ML_MONOMIAL: (1, z_k); EVAL_ML_LAGRANGE: (1 - z_k, z_k), n_point >= n_bits.
// n_points == 0 or n_bits == 0 is hipSuccess, nothing launched; otherwise a bad nl or basis, n_bits > 64, an n_point that does not
// fit, a NULL or misaligned pointer is hipErrorInvalidValue, checked before the launch
enum : int { EVAL_POWERS = 0, EVAL_ML_MONOMIAL = 1, EVAL_ML_LAGRANGE = 2 };
hipError_t launch_eval_pairs(int nl, int basis, const uint32_t* points, uint32_t n_point, uint32_t n_points, uint32_t n_bits,
                             const uint32_t* one, uint32_t* tab, hipStream_t st);
// Step 2, one output element per lane, the point as the grid's second dimension: out[n_points][n] from n_bits pairs of every point,
// the points' pairs tab_bits pairs apart -- `tab` is step 1's table or, for a tensor over the variables from z_a on, that table from
// its pair a (n_bits == 0: no table is read, every out[t][0] is 1).  n == 0 or n_points == 0 is hipSuccess, nothing launched; otherwise a bad nl or
// basis, n_bits > 64 or > tab_bits, n_points > 65535, n >= 2^39, stride == 0, a largest index (n - 1) * stride that overflows 64 bits or has a bit
// at or above n_bits, a NULL or misaligned pointer is hipErrorInvalidValue, checked before the launch
hipError_t launch_eval_expand(int nl, int basis, const uint32_t* tab, uint32_t tab_bits, uint32_t n_bits, uint64_t n, uint64_t stride, uint32_t n_points,
                              const uint32_t* one, uint32_t* out, hipStream_t st);
// K11 (eval.hip): out[t] = sum_{i < n} a[t * a_stride + i] * b[t * b_stride + i] mod p for t < n_pairs; strides in elements, 0 shares
// one vector.  Operands fully reduced Montgomery forms; so is the result (n == 0: zero).  parts == nullptr: one workgroup per pair.
// Otherwise parts has room for field_dot_chunks(n, n_pairs) * n_pairs elements: a pair is cut into that many chunks, one workgroup
// each, whose sums launch_field_sum adds in a second launch (one chunk: parts is not touched, one launch).  Same result either way.
// n_pairs == 0 is hipSuccess, nothing launched; otherwise a bad nl, n_pairs > 65535, a NULL a / b / out or a misaligned pointer is
// hipErrorInvalidValue, checked before any launch
uint32_t field_dot_chunks(uint64_t n, uint32_t n_pairs);
hipError_t launch_field_dot(int nl, const uint32_t* a, uint64_t a_stride, const uint32_t* b, uint64_t b_stride, uint64_t n,
                            uint32_t n_pairs, uint32_t* out, uint32_t* parts, hipStream_t st);

// K12 / K13 (fft.hip): the transform of n_vecs whole vectors of n = 2^log_n elements, the vectors n elements apart.  The forms are
// lcpcf_form's values (include/lcpc_hip_fft.h): X[k] = sum_j x[j] w^(jk), the inverse with w^-1 and n^-1; the two letters give the
// order of input and output, I natural, O bit-reversed.
// fft_plan: the stage split of a transform in decimation-in-frequency order, ceil(log_n / log_tile) passes of log_tile stages of
// which the last takes the remainder; s[] has room for FFT_MAX_PASSES entries.  Returns the number of passes (0 for log_n == 0),
// -1 for log_tile == 0, log_tile > FFT_MAX_LOG_TILE or log_n > FFT_MAX_LOG_N.  A pure host function: launch_fft runs exactly this plan
// (the natural-output forms run it from its last pass to its first).
// Twiddles come from a two-level table `tab` on the device, for the root v = w (forward) or w^-1 (inverse):
//   tab[i] = v^i for i < 2^h, tab[2^h + i] = v^(i 2^h) for i < 2^(log_n - h), h = fft_tab_split(log_n); fft_tab_elems(log_n) elements
// in all, at most 2^(ceil(log_n / 2) + 1).  n_inv: n^-1 mod p as nl words in HOST memory (a kernel argument), read by the inverse
// forms only.  in == out runs in place; otherwise the two ranges must not overlap, and `in` is only read.  Inputs fully reduced; every
// stored element then is.  *n_launches (may be null) receives the number of kernels launched: the passes, plus K13 for the II forms.
// log_n == 0 copies (no launch).  A bad nl, form, log_tile or log_n, n_vecs == 0 or > 65535, n_vecs * n >= 2^39, a NULL or
// misaligned pointer, ranges that overlap without being the same is hipErrorInvalidValue, checked before any launch
enum : int { FFT_FFT_II = 0, FFT_FFT_IO = 1, FFT_FFT_OI = 2, FFT_IFFT_II = 3, FFT_IFFT_IO = 4, FFT_IFFT_OI = 5 };
constexpr uint32_t FFT_MAX_LOG_TILE = 10, FFT_MAX_LOG_N = 32, FFT_MAX_PASSES = 32;
inline uint32_t fft_tab_split(uint32_t log_n) { return log_n / 2; }
inline uint64_t fft_tab_elems(uint32_t log_n) { return ((uint64_t)1 << fft_tab_split(log_n)) + ((uint64_t)1 << (log_n - fft_tab_split(log_n))); }
int fft_plan(uint32_t log_n, uint32_t log_tile, uint32_t s[]);
hipError_t launch_fft(int nl, int form, uint32_t log_n, uint32_t log_tile, uint32_t n_vecs, const uint32_t* in, uint32_t* out,
                      const uint32_t* tab, const uint32_t* n_inv, hipStream_t st, uint32_t* n_launches);
// K13 alone: out[v n + rev(i)] = in[v n + i] over total = n_vecs << log_n elements, log_n >= 1; in == out swaps in place
hipError_t launch_fft_bitrev(int nl, const uint32_t* in, uint32_t* out, uint32_t log_n, uint64_t total, hipStream_t st);

// K14 (domain.hip; include/lcpc_hip_domain.h): the coset forms of the transform above and the low-degree extension.
// launch_coset_fft: X[k] = sum_j x[j] s^j w^(jk) and its inverse x[j] = s^-j n^-1 sum_k X[k] w^(-jk), launch_fft's forms, plan, vectors,
// in-place rule and refusals.  tab as for launch_fft.  stab: the two-level table of the shift for this size and direction,
//   stab[i] = t^i for i < 2^h, stab[2^h + i] = c t^(i 2^h) for i < 2^(log_n - h), h = fft_tab_split(log_n),
// with t = s, c = 1 forward and t = s^-1, c = n^-1 inverse (there is no n_inv argument).  The scale is fused into the pass that loads
// the input (forward) or stores the output (inverse): the launches are launch_fft's.
// launch_extend: Y[k] = sum_{j < n_coeffs} x[j] s^j w_m^(jk) for k < m = 2^log_m, stored at out[k] (natural) or out[rev_m(k)].  Source
// vectors lie 2^ext_src_log(n_coeffs) elements apart and are read up to n_coeffs; output vectors lie m apart; the two ranges must
// not overlap.  It runs the plan of ext_log_n(n_coeffs, log_m) points on n_vecs << (log_m - that) blocks -- the launches of an FFT_IO of
// that length, plus K13 in place for the natural order.  tab_m: the FORWARD table of launch_fft for log_m; stab: the forward shift table
// for ext_log_n points.  hipErrorInvalidValue before any launch for n_coeffs == 0 or > m, log_m > FFT_MAX_LOG_N, n_vecs == 0,
// n_vecs << (log_m - ext_src_log) > 65535, n_vecs * m >= 2^39, a NULL or misaligned pointer, overlapping ranges.  log_m == 0 copies.
inline uint32_t ext_src_log(uint64_t n_coeffs) {
  uint32_t l = 0;
  while (l < 63 && ((uint64_t)1 << l) < n_coeffs) l++;
  return l;
}
// the transform length of a block: the source length, but two points where one coefficient spreads over more than one value
inline uint32_t ext_log_n(uint64_t n_coeffs, uint32_t log_m) {
  const uint32_t l = ext_src_log(n_coeffs);
  return l == 0 && log_m ? 1 : l;
}
// the source elements the extension may read: n_vecs vectors 2^ext_src_log apart, the last up to n_coeffs
inline uint64_t ext_src_elems(uint64_t n_coeffs, uint32_t n_vecs) { return (((uint64_t)n_vecs - 1) << ext_src_log(n_coeffs)) + n_coeffs; }
hipError_t launch_coset_fft(int nl, int form, uint32_t log_n, uint32_t log_tile, uint32_t n_vecs, const uint32_t* in, uint32_t* out,
                            const uint32_t* tab, const uint32_t* stab, hipStream_t st, uint32_t* n_launches);
hipError_t launch_extend(int nl, uint64_t n_coeffs, uint32_t log_m, int natural, uint32_t log_tile, uint32_t n_vecs, const uint32_t* coeffs,
                         uint32_t* out, const uint32_t* tab_m, const uint32_t* stab, hipStream_t st, uint32_t* n_launches);

// K15 / K16 (quot.hip; include/lcpc_hip_quot.h): inverses, pointwise arithmetic and quotients on a domain.  One launch each.  A
// workgroup inverts a tile of quot_tile(nl) elements with one exponentiation per lane of ONE wave (quot.hip describes it).  Inputs fully
// reduced; every stored element then is.  An input may BE the output; ranges that overlap otherwise, a bad nl, op or kind, a NULL or
// misaligned pointer, n == 0 or n >= 2^39 are hipErrorInvalidValue, checked before the launch.
// launch_batch_inverse: out[i] = in[i]^-1, zero for zero.
// launch_pointwise: out[i] = a[i] op b[i]; QUOT_DIV is a[i] b[i]^-1, zero where b[i] is zero.
// launch_domain_quotient: n_vecs vectors of m = 2^log_m values at x_k = s w_m^k, value k at [k] or (bitrev) at [rev_m(k)];
//   QUOT_LINEAR: out_v[k] = (in_v[k] - y[v]) / (x_k - z), s = *shift (NULL: one), z: nl words in HOST memory, y: n_vecs elements on the
//   device that must not meet the output.  The caller guarantees that z is no point of the domain.
//   QUOT_VANISH: out_v[k] = in_v[k] / (x_k^n - 1), n = 2^log_n <= m; `shift` holds s^n (not NULL), z and y are not read.  The caller
//   guarantees s^m != 1.
//   tab_m: the FORWARD table of launch_fft for log_m (not read for log_m == 0); shift and z are kernel arguments.  Further refusals:
//   log_m > FFT_MAX_LOG_N, n_vecs == 0 or > 65535, n_vecs * m >= 2^39, log_n > log_m.
enum : int { QUOT_ADD = 0, QUOT_SUB = 1, QUOT_MUL = 2, QUOT_DIV = 3 };
enum : int { QUOT_LINEAR = 0, QUOT_VANISH = 1 };
constexpr uint32_t quot_tile(int nl) { return nl >= 6 ? 2048 : 4096; }      // elements of a workgroup's tile
hipError_t launch_batch_inverse(int nl, const uint32_t* in, uint32_t* out, uint64_t n, hipStream_t st);
hipError_t launch_pointwise(int nl, int op, const uint32_t* a, const uint32_t* b, uint32_t* out, uint64_t n, hipStream_t st);
hipError_t launch_domain_quotient(int nl, int kind, int bitrev, uint32_t log_m, uint32_t log_n, uint32_t n_vecs, const uint32_t* in, uint32_t* out,
                                  const uint32_t* tab_m, const uint32_t* shift, const uint32_t* z, const uint32_t* y, hipStream_t st);

// K17 (scan.hip; include/lcpc_hip_scan.h): prefix sums and products of n_vecs vectors of n elements, the vectors n elements apart,
// each scanned on its own.  out_v[k] = c_v (+) in_v[0] (+) ... (+) in_v[k] (SCAN_INCLUSIVE) or ... (+) in_v[k - 1] (SCAN_EXCLUSIVE),
// total[v] = c_v (+) all of in_v, with c_v = init[v], or the identity where init is NULL; total may be NULL.  `one` is R mod p as nl
// words in HOST memory (a kernel argument).  A workgroup owns a tile of scan_tile(nl) consecutive elements, scan_lane_elems(nl)
// consecutive ones per lane.  A vector of one tile is ONE launch (K17c seeded with c_v; work is not touched).  Otherwise K17a writes
// the tile totals to work[v * tiles + t]; K17b turns them into the tiles' exclusive prefixes in place and writes total -- it is this
// very scan, exclusive and in place, of n_vecs runs of `tiles` elements, with the rest of `work` as its workspace: one launch while
// tiles <= scan_mid_chunk(nl), three up to its square --; K17c applies them.  Three launches up to scan_tile(nl)^2 elements per
// vector, five beyond.  No workgroup waits for another.  in == out runs in place (both modes); *n_launches (may be null) receives
// the number of kernels.  work has room for work_elems >= scan_work_elems(nl, n, n_vecs) elements: the totals of every level, the
// last (one per vector) included.  Inputs fully reduced; every stored element then is.
// hipErrorInvalidValue before any launch: a bad nl, op or mode, n == 0, n_vecs == 0 or > 65535, n * n_vecs >= 2^39, a NULL in, out,
// one or work, a misaligned pointer, too small a work_elems, in and out overlapping without being the same, init, total or work
// meeting another buffer or each other; and a vector of SCAN_MAX_TILES tiles or more (2^35 elements, 2^36 for nl <= 4 -- more than
// any device holds): the tiles of a vector are the grid's x dimension, which times the 256 lanes must stay below 2^32
enum : int { SCAN_SUM = 0, SCAN_PRODUCT = 1 };
enum : int { SCAN_INCLUSIVE = 0, SCAN_EXCLUSIVE = 1 };
constexpr uint32_t SCAN_LANES = 256;
constexpr uint64_t SCAN_MAX_TILES = (uint64_t)1 << 24;
constexpr uint32_t scan_lane_elems(int nl) { return nl >= 6 ? 8 : 16; }
constexpr uint32_t scan_tile(int nl) { return SCAN_LANES * scan_lane_elems(nl); }
constexpr uint32_t scan_mid_chunk(int nl) { return scan_tile(nl); }
inline uint64_t scan_tiles(int nl, uint64_t n) { return (n + scan_tile(nl) - 1) / scan_tile(nl); }
inline uint64_t scan_work_elems(int nl, uint64_t n, uint32_t n_vecs) {
  uint64_t t = n, sum = 0;
  do { t = scan_tiles(nl, t); sum += t; } while (t > 1);
  return sum * n_vecs;
}
hipError_t launch_scan(int nl, int op, int mode, const uint32_t* in, uint32_t* out, uint64_t n, uint32_t n_vecs, const uint32_t* init,
                       uint32_t* total, const uint32_t* one, uint32_t* work, uint64_t work_elems, hipStream_t st, uint32_t* n_launches);

// K18 / K19 (sumcheck.hip; include/lcpc_hip_sumcheck.h): the round sums of a composition of tables and the binding of a variable.  A
// table is n = 2^v elements; pair i < n / 2 is (t[2i], t[2i+1]) (SUMCHECK_LOW_FIRST) or (t[i], t[i + n/2]) (SUMCHECK_HIGH_FIRST), and
// ext(t, i, x) = lo + x (hi - lo).  `in`, `out`, `tables` are HOST arrays of n_tables device pointers; r, coeffs ([n_terms][nl], null: all
// one) and one (R mod p) are nl-word elements in HOST memory that travel as kernel arguments.
// launch_sumcheck_bind (K19): out[j][i] = ext(in[j], i, r), i < n / 2, one launch, the table as the grid's second dimension.
// launch_sumcheck_round (K18): evals[x] = sum_i sum_m c_m prod_k ext(tables[terms[m].table[k]], i, x), x = 0 .. d = max n_factors.  A
// workgroup of SUMCHECK_LANES lanes takes tiles of sumcheck_tile_pairs pairs in a grid-stride loop over sumcheck_groups(pairs,
// max_groups) workgroups and leaves its sums, one per term and x, in work[(group * n_terms + m) * (d + 1) + x]; a second launch of d + 1
// workgroups adds them and applies c_m.  One workgroup does both itself: one launch, work untouched.
// launch_sumcheck_bind_round (K18f), n >= 4: lane i < n / 4 binds its two pairs of every table, stores them, and adds the round of the
// BOUND tables (n / 2 elements, pair i) to its sums: the stores of the bind and the evals of the round on its output, bit for bit.
// *n_launches (may be null) receives the kernels launched.  Inputs fully reduced; every stored element then is.  No workgroup waits
// for another.
// hipErrorInvalidValue before any launch, for everything sumcheck_job_ok refuses: a bad nl or order; n no power of two, below 2 (4 for
// the fused form) or >= 2^39; n_tables, n_terms, an n_factors of 0 or above its limit, a table index >= n_tables; a NULL or misaligned
// pointer (coeffs may be null); max_groups == 0; work_elems < sumcheck_work_elems(pairs, n_terms, max_groups); an output that meets an
// input without BEING it under SUMCHECK_HIGH_FIRST with the same table number (and that input listed once); outputs meeting each
// other; evals or work meeting anything else.
enum : int { SUMCHECK_LOW_FIRST = 0, SUMCHECK_HIGH_FIRST = 1 };
constexpr uint32_t SUMCHECK_MAX_TABLES = 8, SUMCHECK_MAX_TERMS = 4, SUMCHECK_MAX_FACTORS = 4;
constexpr uint32_t SUMCHECK_LANES = 256;
constexpr uint32_t SUMCHECK_GROUPS = 1024;          // the product's max_groups: four workgroups for each of 256 compute units
struct SumcheckTerm { uint32_t n_factors; uint32_t table[SUMCHECK_MAX_FACTORS]; };
constexpr uint32_t sumcheck_tile_pairs(int) { return SUMCHECK_LANES; }      // one pair per lane and stride, every field
inline uint32_t sumcheck_groups(uint64_t pairs, uint32_t max_groups) {
  const uint64_t tiles = (pairs + SUMCHECK_LANES - 1) / SUMCHECK_LANES;
  return (uint32_t)(tiles < max_groups ? tiles : max_groups);
}
// (every workgroup has room for MAX_FACTORS + 1 sums per term, whatever the degree)
inline uint64_t sumcheck_work_elems(uint64_t pairs, uint32_t n_terms, uint32_t max_groups) {
  return (uint64_t)sumcheck_groups(pairs, max_groups) * n_terms * (SUMCHECK_MAX_FACTORS + 1);
}
// the degree of a composition, 0 where it is refused
inline uint32_t sumcheck_degree(uint32_t n_tables, const SumcheckTerm* terms, uint32_t n_terms) {
  if (n_tables == 0 || n_tables > SUMCHECK_MAX_TABLES || !terms || n_terms == 0 || n_terms > SUMCHECK_MAX_TERMS) return 0;
  uint32_t d = 0;
  for (uint32_t m = 0; m < n_terms; m++) {
    if (terms[m].n_factors == 0 || terms[m].n_factors > SUMCHECK_MAX_FACTORS) return 0;
    for (uint32_t k = 0; k < terms[m].n_factors; k++)
      if (terms[m].table[k] >= n_tables) return 0;
    if (terms[m].n_factors > d) d = terms[m].n_factors;
  }
  return d;
}
// one call of the three launchers: bind (out used), round (terms, evals, work used) or both (the fused form).  A pure host function
// that reads none of the buffers: the launchers and the entry points of sumcheck.cpp settle their refusals with it
struct SumcheckJob {
  int nl, order;
  bool bind, round;
  const uint32_t* const* in;
  uint32_t* const* out;
  uint32_t n_tables;
  const SumcheckTerm* terms;
  uint32_t n_terms;
  uint64_t n;
  const uint32_t* evals;
  const uint32_t* work;
  uint64_t work_elems;
  uint32_t max_groups;
};
inline uint64_t sumcheck_pairs(const SumcheckJob& j) { return j.bind && j.round ? j.n / 4 : j.n / 2; }
inline bool sumcheck_job_ok(const SumcheckJob& j) {
  auto meet = [](const void* a, uint64_t na, const void* b, uint64_t nb) {
    const uintptr_t x = reinterpret_cast<uintptr_t>(a), y = reinterpret_cast<uintptr_t>(b);
    return x < y + nb && y < x + na;
  };
  if (!nl_ok(j.nl) || (j.order != SUMCHECK_LOW_FIRST && j.order != SUMCHECK_HIGH_FIRST) || !j.in) return false;
  if (j.n_tables == 0 || j.n_tables > SUMCHECK_MAX_TABLES) return false;
  if (j.n < (j.bind && j.round ? 4u : 2u) || j.n >= ((uint64_t)1 << 39) || (j.n & (j.n - 1))) return false;
  const uint64_t eb = (uint64_t)j.nl * 4, in_b = j.n * eb, out_b = in_b / 2;
  for (uint32_t t = 0; t < j.n_tables; t++)
    if (!j.in[t] || !elem_aligned(j.in[t], j.nl)) return false;
  uint64_t ev_b = 0, work_b = 0;
  if (j.round) {
    const uint32_t d = sumcheck_degree(j.n_tables, j.terms, j.n_terms);
    if (d == 0 || !j.evals || !j.work || !elem_aligned(j.evals, j.nl) || !elem_aligned(j.work, j.nl) || j.max_groups == 0) return false;
    const uint64_t need = sumcheck_work_elems(sumcheck_pairs(j), j.n_terms, j.max_groups);
    if (j.work_elems < need) return false;
    ev_b = (d + 1) * eb; work_b = need * eb;
    if (meet(j.evals, ev_b, j.work, work_b)) return false;
    for (uint32_t t = 0; t < j.n_tables; t++)
      if (meet(j.evals, ev_b, j.in[t], in_b) || meet(j.work, work_b, j.in[t], in_b)) return false;
  }
  if (j.bind) {
    if (!j.out) return false;
    for (uint32_t t = 0; t < j.n_tables; t++) {
      if (!j.out[t] || !elem_aligned(j.out[t], j.nl)) return false;
      if (j.round && (meet(j.evals, ev_b, j.out[t], out_b) || meet(j.work, work_b, j.out[t], out_b))) return false;
      for (uint32_t u = 0; u < j.n_tables; u++) {
        if (u != t && meet(j.out[t], out_b, j.out[u], out_b)) return false;
        if (!meet(j.out[t], out_b, j.in[u], in_b)) continue;
        if (j.order != SUMCHECK_HIGH_FIRST || u != t || j.out[t] != j.in[t]) return false;     // in place: this table's own input only
      }
    }
  }
  return true;
}
hipError_t launch_sumcheck_bind(int nl, int order, const uint32_t* const* in, uint32_t* const* out, uint32_t n_tables, uint64_t n,
                                const uint32_t* r, hipStream_t st);
hipError_t launch_sumcheck_round(int nl, int order, const uint32_t* const* tables, uint32_t n_tables, const SumcheckTerm* terms, uint32_t n_terms,
                                 const uint32_t* coeffs, const uint32_t* one, uint64_t n, uint32_t* evals, uint32_t* work, uint64_t work_elems,
                                 uint32_t max_groups, hipStream_t st, uint32_t* n_launches);
hipError_t launch_sumcheck_bind_round(int nl, int order, const uint32_t* const* in, uint32_t* const* out, uint32_t n_tables,
                                      const SumcheckTerm* terms, uint32_t n_terms, const uint32_t* coeffs, const uint32_t* one, uint64_t n,
                                      const uint32_t* r, uint32_t* evals, uint32_t* work, uint64_t work_elems, uint32_t max_groups,
                                      hipStream_t st, uint32_t* n_launches);

}  // namespace lcpc

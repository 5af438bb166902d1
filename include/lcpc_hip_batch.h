/*
 * include/lcpc_hip_batch.h -- extension of the C ABI of lcpc_hip.h: one commit call for MANY equal-shape polynomials.
 *
 * A prover commits to dozens of witness polynomials of one shape under one encoder.  One by one, each small commit is a chain of
 * short kernels on a nearly empty chip; this entry point runs the whole batch through one pipeline instead.
 *
 * The extension has its own prefix (lcpcx_) and its own version.  Its symbols are exported by the same liblcpc_hip.so; nothing of
 * lcpc_hip.h changes, LCPC_ABI_VERSION stays what it is, and a caller built against that header alone is unaffected.  A caller of
 * this header checks lcpcx_batch_version() == LCPCX_BATCH_VERSION (and the core version as before).
 *
 * Contract of the batch commit
 *  - cms[0 .. n_batch) are distinct commitment objects (made by the core header's commit-create call) of ONE unsharded encoder.
 *    Polynomial i is the n_coeffs elements at coeffs_dev + i * poly_stride * L (L = 64-bit limbs per element; poly_stride counts
 *    elements, is >= n_coeffs, and 0 means n_coeffs: the polynomials back to back).  What lies between strided polynomials is
 *    never read.
 *  - After the call member cms[i] is in the state the core header's device commit of polynomial i alone (same stream, same flags)
 *    would have left it in: the same comm, coeffs, hashes, root and dims, bit for bit.  Every reader of the core header -- prove,
 *    open_columns, collapse and its device form, the getters, the bincode writer -- works on it unchanged and concurrently, as that
 *    header documents.
 *  - The members are independent afterwards: any of them may be destroyed, in any order; any of them may be refilled alone through
 *    any commit entry point of the core header, at other dims too; any of them may be refilled by another batch call, with the same
 *    or other partners.  (Members of a batched commit share one device allocation; the last of them to be destroyed or refilled
 *    elsewhere frees it.  A batch call into the same members, in the same order, at the same shape reuses it.)
 *  - flags: LCPC_COMMIT_BORROW_COEFFS means what it means in the core header -- honoured when n_coeffs fills whole rows; member i
 *    then keeps reading its slice of the caller's buffer, which must outlive it.  LCPC_COMMIT_ASYNC_TAIL is ignored, as by the
 *    single device commit.
 *  - roots: n_batch * D bytes (D = the encoder's digest length), root i at roots + i * D; or NULL.  A non-NULL roots synchronises
 *    `stream` ONCE, for the whole batch.  With NULL the call only enqueues work on `stream`; every member records its completion
 *    event, so readers and refills on other streams wait for the batch exactly as they wait for a single commit.
 *  - errors: LCPC_ERR_ARG for a NULL cms / member / coeffs_dev, n_batch == 0 or > 65535, n_coeffs == 0, 0 < poly_stride < n_coeffs,
 *    a member listed twice, members of different encoders; LCPC_ERR_STATE on a sharded encoder; device errors as usual (the detail
 *    text is on cms[0]).  After a failure EVERY member is un-committed, as after a failed single commit.
 *  - threads: the call is a fill of every member.  It takes the members' fill locks in one global order (by address), so batches
 *    that overlap in members, issued from several threads, do not deadlock; readers in flight on any member are waited for.
 *
 * Which encoders are batched
 *  - Ligero encoders, all four fields, all five digests: ONE row encode over n_batch * n_rows rows (the row NTT is row-independent),
 *    then batched column-hash and tree kernels, the member index a grid dimension.  BLAKE3: kernels.hip (K3b / K4b).  SHA3-256,
 *    Keccak-256, SHA-256 and BLAKE2b -- one serial chain per column -- run the batch forms of their leaf and subtree kernels (sha3.hip,
 *    sha256.hip, blake2b.hip): one leaf launch and one tree call for the whole batch, roots and hashes slots of D bytes.
 *    The hash and tree of the whole batch cost as many launches as one member's; the encode costs one member's when n_coeffs fills
 *    whole rows and the polynomials are back to back, and one more (a strided placement that also zero-fills ragged tails) otherwise.
 *  - Brakedown encoders: the expander matrices are the same for every row of every member, so the encode is ONE pass over the
 *    n_batch * n_rows stacked rows, in the launches of one commit (one more when a placement is needed, as above).  By the member's
 *    n_rows, at the threshold of the single commit (24), so that each member holds what it would hold alone:
 *      n_rows < 24   the members keep row-major comm matrices in the shared allocation, as Ligero members do.  From 24 STACKED rows on
 *                    the encode runs the position-major kernels on a working copy and transposes back; below, the row-major kernels.
 *      n_rows >= 24  every member keeps its own position-major matrix, written by the batch forms of the position-major kernels
 *                    (kernels.hip K2b: one lane per stacked row, full waves).  The row-major copy lcpc_get_comm makes on demand is
 *                    the member's own allocation; reading it leaves the shared one and the other members alone.
 *    BLAKE3: the batched column-hash and tree kernels, as for Ligero -- hash and tree cost one commit's launches.
 *    LIMITATION -- SHA3-256, Keccak-256, SHA-256, BLAKE2b: the encode is batched as above, the hash and the tree run member by member
 *    with the single-commit launchers, n_batch times one commit's launches (pinned by
 *    tests/test_gpu_commit_batch_digests.py::test_brakedown_under_a_chained_digest); the roots are then copied out member by member
 *    behind the one synchronisation.
 *    LIMITATION -- a batch of more than 65535 * 32 stacked rows (the grid of the batch transposes) runs the single-commit pipeline for
 *    each member in turn on `stream`: same results.
 *
 * Timing: if lcpc_set_timing is on for cms[0], the call measures the BATCH -- phase times and launch counts of all members
 * together -- and stores those figures in every member's lcpc_timings.  They are the batch's, not one member's share.  For Brakedown
 * under BLAKE3 all of them are the batch's; under the four chained digests encode_ms and encode_launches are the batch's, hash_ms /
 * merkle_ms and their launch counts are sums over the members (the members' hashes and trees alternate on the stream).  On the
 * member-by-member path every figure is the sum over the members.
 *
 * Contract of the batch prove (version 2)
 *  The prover that committed a batch opens all of it.  One call runs the core header's prove for every member in lockstep: all members
 *  draw their degree-test tensors, ONE launch chain collapses for all, all members absorb side by side on the host pool, all draw
 *  their columns, ONE launch chain opens for all.  Every proof is byte for byte what the core header's prove call returns for that
 *  member alone, and every transcript is left in exactly the state that call leaves it in.
 *  - members: cms[0 .. n_batch) are distinct, committed, unsharded commitments of ONE encoder with the same n_rows.  They need not come
 *    from one batch commit, or from a batch commit at all: slab members, single device / host / from_parts / from_bincode commits,
 *    borrowed coefficients and position-major Brakedown members may be mixed in any order.  The kernels reach every member through a
 *    per-member descriptor (coeffs, comm and its two strides, hashes), never through a slab stride.
 *  - outer tensor: member i's is the n_outer elements at outer_tensors + i * outer_stride * L.  outer_stride == 0 means ONE tensor
 *    shared by all members (all polynomials opened at one point); a nonzero stride must be >= n_outer.
 *  - transcripts and proofs: trs[i] is member i's transcript; the transcripts are distinct objects.  proofs[i] / proof_lens[i]
 *    receive the bincode bytes, each released with lcpc_free like a single proof.  cols_opened: NULL, or [n_batch][n_col_opens].
 *  - errors: LCPC_ERR_ARG for a NULL cms / member / trs / transcript / outer_tensors / proofs / proof_lens, n_batch == 0 or > 65535, a
 *    member or a transcript listed twice, members of different encoders or different n_rows, 0 < outer_stride < n_outer;
 *    LCPC_ERR_STATE for an uncommitted member or a sharded encoder; LCPC_ERR_OUTER_TENSOR for n_outer != n_rows; LCPC_ERR_COMMIT where
 *    the single prove returns it; device errors as usual (the detail text is on cms[0]).  After a failure no proof is returned --
 *    every proofs[i] is NULL, nothing leaks -- and the transcripts are in an unspecified state, as after a failed single prove.
 *  - threads: the call is a READER of every member.  It holds every member's fill lock shared for its duration, taken in address
 *    order as the batch commit takes its exclusive locks, so it runs next to single proves, other batch proves that overlap in
 *    members, collapses and opens; a refill of any member waits for it.  It works in ONE working set of cms[0] (stream, pinned arena,
 *    device scratch, sized for a group); the stream is ordered behind every member's commit.
 *  - stats (may be NULL): how the call ran.  Within one group the launch and synchronisation counts do not depend on n_batch.
 *  - groups: the pinned arena per member is
 *        A = (2 n_rows + 4 n_per_row) F + n_col_opens (8 + n_rows F + path_len D)   bytes  (F = 8 L, D = the digest length)
 *    -- tensors, polynomials and their canonical forms; the drawn columns and the opened columns and paths, which are staged.
 *    LIMITATION -- the arena is bounded by LCPCX_PROVE_ARENA_BUDGET (64 MiB): a batch runs in consecutive groups of
 *    max(1, floor(budget / A)) members, ceil(n_batch / that) groups in all, each a lockstep pipeline of its own.  Same results;
 *    stats.groups says how many.  (The arena stays with cms[0]'s working set until that object is destroyed.)
 *  - timing: with LCPC_DEBUG_TIMING set when the encoder was created the call prints one line for the batch to stderr.
 *  Out of scope: sharded encoders (LCPC_ERR_STATE); the batched verify, which is lcpc_hip_verify.h's; any change to proof format or protocol, such as a random linear
 *  combination of the members into one proof -- the reference has none, and byte parity would have nothing to stand on.
 */
#ifndef LCPC_HIP_BATCH_H
#define LCPC_HIP_BATCH_H
#include "lcpc_hip.h"
#ifdef __cplusplus
extern "C" {
#endif

#define LCPCX_BATCH_VERSION 2
int lcpcx_batch_version(void);
/* cms[0..n_batch): distinct LcCommit objects of ONE unsharded encoder.  Polynomial i = n_coeffs elements at
 * coeffs_dev + i * poly_stride * L  (poly_stride in elements, >= n_coeffs; 0 means n_coeffs).
 * roots: n_batch * D bytes (D = the encoder's digest length) or NULL; non-NULL synchronises `stream` once. */
int lcpcx_commit_batch_device(lcpc_commit_t *const *cms, uint32_t n_batch, const uint64_t *coeffs_dev,
                              uint64_t n_coeffs, uint64_t poly_stride, void *stream, uint32_t flags, uint8_t *roots);

#define LCPCX_PROVE_ARENA_BUDGET ((uint64_t)64 << 20)
typedef struct {
  uint32_t groups;            /* lockstep groups the batch was cut into */
  uint32_t collapse_launches; /* kernel launches of all collapse rounds: to_r29 + collapse + split sum + to_canon */
  uint32_t open_launches;     /* column + path gather launches */
  uint32_t host_syncs;        /* stream / event synchronisations the call made */
} lcpcx_prove_stats;
/* cms[0..n_batch): distinct committed LcCommit objects of ONE unsharded encoder, equal n_rows; trs[0..n_batch): distinct transcripts.
 * Member i's outer tensor: n_outer elements at outer_tensors + i * outer_stride * L (0: one tensor for all).
 * proofs / proof_lens: [n_batch]; cols_opened: [n_batch][n_col_opens] or NULL; stats: NULL or filled on success. */
int lcpcx_prove_batch(lcpc_commit_t *const *cms, uint32_t n_batch, const uint64_t *outer_tensors, uint64_t n_outer,
                      uint64_t outer_stride, lcpc_transcript *const *trs, uint8_t **proofs, uint64_t *proof_lens,
                      uint64_t *cols_opened, lcpcx_prove_stats *stats);

#ifdef __cplusplus
}
#endif
#endif

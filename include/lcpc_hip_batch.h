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
 *    then batched column-hash and tree kernels, the member index a grid dimension.  BLAKE3: batch_kernels.hip (K3b / K4b).  SHA3-256,
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
 */
#ifndef LCPC_HIP_BATCH_H
#define LCPC_HIP_BATCH_H
#include "lcpc_hip.h"
#ifdef __cplusplus
extern "C" {
#endif

#define LCPCX_BATCH_VERSION 1
int lcpcx_batch_version(void);
/* cms[0..n_batch): distinct LcCommit objects of ONE unsharded encoder.  Polynomial i = n_coeffs elements at
 * coeffs_dev + i * poly_stride * L  (poly_stride in elements, >= n_coeffs; 0 means n_coeffs).
 * roots: n_batch * D bytes (D = the encoder's digest length) or NULL; non-NULL synchronises `stream` once. */
int lcpcx_commit_batch_device(lcpc_commit_t *const *cms, uint32_t n_batch, const uint64_t *coeffs_dev,
                              uint64_t n_coeffs, uint64_t poly_stride, void *stream, uint32_t flags, uint8_t *roots);

#ifdef __cplusplus
}
#endif
#endif

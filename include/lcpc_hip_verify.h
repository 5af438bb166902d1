/*
 * include/lcpc_hip_verify.h -- verifier-side extension of the C ABI of lcpc_hip.h: one verify call for MANY proofs under one encoder.
 *
 * A verifier that receives the proofs of a batch of equal-shape polynomials (lcpc_hip_batch.h commits and opens such a batch in one
 * pipeline each) checks all of them here in one lockstep pipeline, in place of one single-proof verify call of the core header per
 * proof.  Each of those starts two helper threads, takes the encoder's lock for a row encode of 1 + n_degree_tests rows on a nearly
 * empty chip, brings the encoded rows back whole, and computes the tensor . column dot products and the leaf hashes on the host.
 *
 * The extension has its own prefix (lcpcv_) and its own version.  Its symbols are exported by the same liblcpc_hip.so; nothing of
 * lcpc_hip.h or lcpc_hip_batch.h changes, and a caller built against those headers alone is unaffected: a verifier links neither the
 * batch commit nor the batch prove.  A caller of this header checks lcpcv_version() == LCPCV_VERSION (and the core version as before).
 *
 * Contract of the batch verify
 *  - members: member i has a root at roots + i * D (D = the encoder's digest length), a proof of proof_lens[i] bytes at proofs[i], at any
 *    alignment, and a transcript trs[i].  Its outer tensor is the n_outer elements at outer_tensors + i * outer_stride * L (L = 64-bit
 *    limbs per element), its inner tensor the n_inner elements at inner_tensors + i * inner_stride * L.  A stride of 0 means ONE tensor
 *    shared by all members; a nonzero stride must be >= the count.  What lies between strided tensors is never read.  The transcripts are
 *    distinct objects.
 *  - verdicts are per member: status[i] is exactly what the core header's verify call returns for member i alone with the same
 *    arguments -- 0 or an LCPC_VERR_* code, with its precedence: the first failing column decides, and within a column degree > eval >
 *    path.  evals + i * L receives member i's evaluation when status[i] == 0 and is left alone otherwise.  After a member with status 0
 *    its transcript is in the state the single verify leaves it in; after a failed member its state is unspecified.  A member that fails
 *    -- malformed bytes, a tensor of the wrong length for ITS proof, a limb >= p, a bad column -- drops out and does not disturb the
 *    others: its slots of the device work are zero-filled and never read as data.
 *  - return value: 0 when every member was judged, whatever the verdicts.  LCPC_ERR_ARG for a NULL ctx / roots / outer_tensors /
 *    inner_tensors / proofs / proof_lens / trs / evals / status, a NULL member proof or transcript, n_batch == 0 or > 65535, a transcript
 *    listed twice, 0 < outer_stride < n_outer or 0 < inner_stride < n_inner: all of it checked before a device is touched.
 *    LCPC_ERR_STATE on a sharded encoder.  Device and allocation errors as usual, the detail text on the context.  After any failure
 *    but LCPC_ERR_ARG, EVERY status[i] is that error code; an argument error writes nothing.
 *  - threads: the call runs beside single verifies, beside other batch verifies and beside commits and proves under the same encoder.
 *    It takes one working set from the context (stream, pinned arena, device buffers, sized for a group), as a single verify takes its
 *    pinned set.  The row encode shares the encoder's encode workspace with the single verifies: the call takes the encoder's lock
 *    around it and holds it until the encode has run -- not while the hashes and the column check run, and never across a transcript.
 *  - the pipeline, per group: every member is parsed, checked and staged on the host pool; ONE upload; ONE row encode of all
 *    members' 1 + n_degree_tests polynomials, whose result stays on the device; the leaf digests of all opened columns (the batch forms
 *    of the column-hash kernels; under SHA3-256 / Keccak-256 / SHA-256 / BLAKE2b over Ft255, one representation change in front of them);
 *    beside that the members' transcripts on the host pool; ONE upload of tensors and drawn columns; the column check (all dot products
 *    and their comparison with the encoded rows, one kernel); the Merkle path folds (one more kernel, below); ONE download of the status words and leaf
 *    digests; the verdicts on the host pool.
 *  - stats (may be NULL, filled when the call returns 0): how the call ran.  host_syncs is 2 per group: one event wait behind the row
 *    encode, for which the encoder's lock is held, and one stream synchronisation at the end.  Within one group the launch and
 *    synchronisation counts do not depend on n_batch for a Ligero encoder; a Brakedown row encode changes kernels at 24 stacked rows, as
 *    it does in a commit, and encode_launches with it.
 *  - groups: the pinned arena per member is
 *        A = 2 (n_deg + 1) n_per_row F + (n_deg + 1) n_rows F + n_col_opens (8 + 4 + D) + even(n_col_opens n_rows) F   bytes
 *    (n_rows = n_outer, F = 8 L; even(x) = x rounded up to an even number for Ft63 and Ft191, x itself for Ft127 and Ft255: the
 *    column-hash kernels want member strides of 16 bytes, in whole elements) -- the polynomials and their canonical forms; the tensors;
 *    the drawn column numbers, the status words and the leaf digests that come back; the staged columns.  The arena is bounded by LCPCV_ARENA_BUDGET
 *    (64 MiB): a batch runs in consecutive groups of max(1, floor(budget / A)) members, ceil(n_batch / that) groups in all, each a
 *    pipeline of its own.  Same verdicts; stats.groups says how many.  (The seven segments of a group start at multiples of 256 bytes;
 *    that slack, under 2 KiB, is not counted.  The arena stays with the working set until the encoder is destroyed.)
 *    n_outer == 0 fits no honest proof (a column has at least one row): such a call is judged member by member by the single verify,
 *    and stats is all zero.
 *  - timing: with LCPC_DEBUG_TIMING set when the encoder was created the call prints one line to stderr: parse + stage, transcripts,
 *    device, path folds (the host's share), and how many columns folded on the device and how many on the host.
 *  - path folds: the Merkle path of every opened column is folded on the device, by one more kernel behind the column check (one lane per
 *    opened column: the leaf digest, path_len node hashes, the comparison with the member's root; a mismatch sets bit 4 of the
 *    column's status word, beside the column check's 1 = degree and 2 = eval).  The siblings are staged level-major in a second pinned
 *    buffer of the working set and cross the bus behind the polynomials; they are P = n_col_opens * path_len * D bytes per member
 *    (path_len = the encoder's tree depth) and are NOT part of A.  They are bounded by LCPCV_PATH_BUDGET (64 MiB): the first
 *    min(g, max(1, floor(budget / P))) members of a group of g fold on the device, the rest of that group on the host pool (one task per
 *    opened column, from the downloaded leaf digest).  A column whose path has another number of entries than path_len (the parser
 *    accepts any count) is folded on the host as well.  Same verdicts either way.
 *  Out of scope: sharded encoders (LCPC_ERR_STATE); any change to the proof format or the protocol, such as a random linear combination
 *  of the proofs -- the reference has none.
 */
#ifndef LCPC_HIP_VERIFY_H
#define LCPC_HIP_VERIFY_H
#include "lcpc_hip.h"
#ifdef __cplusplus
extern "C" {
#endif

#define LCPCV_VERSION 1
int lcpcv_version(void);

#define LCPCV_ARENA_BUDGET ((uint64_t)64 << 20)
#define LCPCV_PATH_BUDGET ((uint64_t)64 << 20)
typedef struct {
  uint32_t groups;           /* lockstep groups the batch was cut into */
  uint32_t encode_launches;  /* kernel launches of the row encode(s) */
  uint32_t hash_launches;    /* leaf-digest launches (and representation changes in front of them), and the path-fold launch */
  uint32_t check_launches;   /* tensor conversions + the column-check kernel */
  uint32_t host_syncs;       /* stream / event synchronisations the call made */
} lcpcv_verify_stats;
/* roots: n_batch * D bytes; member i's tensors at outer_tensors + i * outer_stride * L / inner_tensors + i * inner_stride * L (stride 0:
 * one tensor for all); proofs / proof_lens / trs / status: [n_batch]; evals: [n_batch][L]; stats: NULL or filled on success. */
int lcpcv_verify_batch(lcpc_ctx *ctx, uint32_t n_batch, const uint8_t *roots,
                       const uint64_t *outer_tensors, uint64_t n_outer, uint64_t outer_stride,
                       const uint64_t *inner_tensors, uint64_t n_inner, uint64_t inner_stride,
                       const uint8_t *const *proofs, const uint64_t *proof_lens,
                       lcpc_transcript *const *trs,
                       uint64_t *evals, int32_t *status, lcpcv_verify_stats *stats);

#ifdef __cplusplus
}
#endif
#endif

/*
 * include/lcpc_hip_columns.h -- column-check extension of the C ABI of lcpc_hip.h: the verifier's side of an opening made OUTSIDE a proof.
 *
 * The core header's open-columns call lets a prover open columns of a commitment on request: per column its n_rows values and the
 * Merkle path of its leaf.  This header is the other side: given a root, it says for each such opening whether the column's leaf digest
 * folds up that path to the root -- verify_column_path of the reference (lcpc-2d lib.rs:955-982), which until now ran only inside the
 * verify calls.  It runs on the device: the leaf digests by the batch forms of the column-hash kernels, the folds by the path-fold
 * kernel the batched verify of lcpc_hip_verify.h runs (one lane per column).
 *
 * The extension has its own prefix (lcpcp_) and its own version.  Its symbols are exported by the same liblcpc_hip.so; nothing of
 * lcpc_hip.h, lcpc_hip_batch.h or lcpc_hip_verify.h changes.  A caller of this header checks lcpcp_version() == LCPCP_VERSION (and the
 * core version as before).
 *
 * Contract of the column check
 *  - arguments, as the open-columns call of the core header returns them: cols[n] column numbers; col_vals[n][n_rows][L] stored limbs
 *    (L = 64-bit limbs per element); paths[n][path_len][D] sibling digests, level 0 first (path_len = log2 of the encoder's n_cols
 *    rounded up to a power of two, D = the encoder's digest length); root: D bytes.  ok[n] receives 1 where the column's leaf digest
 *    folds to root and 0 where it does not.  A column number may be listed more than once.
 *  - return value: 0 when every column was judged, whatever the verdicts.  LCPC_ERR_ARG for a NULL ctx / root / cols / col_vals /
 *    paths / ok or n_rows == 0, settled before a device is touched.  n == 0 returns 0 and writes nothing (it is looked at after the
 *    pointers).  LCPC_ERR_COLUMN_NUMBER if any cols[i] >= n_cols: nothing is judged and ok is left alone.  LCPC_ERR_STATE on a sharded
 *    encoder.  Device and allocation errors as usual, the detail text on the context; ok is then unspecified.
 *  - untrusted limbs: a column with a limb >= p gets ok = 0 -- no honest opening has one.  Its slot of the device work is zero-filled
 *    and never reaches device arithmetic.
 *  - threads: the call does not take the encoder's lock.  It takes one working set from the context, as the batched verify does, and
 *    runs beside verifies, commits and proves under the same encoder.
 *  - slices: the columns run in consecutive slices.  A slice's values fit the arena budget of lcpc_hip_verify.h (64 MiB) and its
 *    siblings the path budget (64 MiB), with at least one column per slice.  Per slice: ONE upload, the leaf digests, the path folds,
 *    ONE download, one synchronisation.
 *  Out of scope: sharded encoders; a check of the values against an evaluation (that is the verify calls' column check).
 */
#ifndef LCPC_HIP_COLUMNS_H
#define LCPC_HIP_COLUMNS_H
#include "lcpc_hip.h"
#ifdef __cplusplus
extern "C" {
#endif

#define LCPCP_VERSION 1
int lcpcp_version(void);

/* cols[n]; col_vals[n][n_rows][L] stored limbs; paths[n][path_len][D]; ok[n] = 1 where the column's leaf digest folds to root */
int lcpcp_check_columns(lcpc_ctx *ctx, const uint8_t *root, const uint64_t *cols, uint32_t n, uint64_t n_rows,
                        const uint64_t *col_vals, const uint8_t *paths, uint8_t *ok);

#ifdef __cplusplus
}
#endif
#endif

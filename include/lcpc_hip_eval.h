/*
 * include/lcpc_hip_eval.h -- evaluation extension of the C ABI of lcpc_hip.h: from a point to the two tensors of an opening, and
 * the value of the committed polynomial at that point, computed where the coefficients are.
 *
 * The core header proves and verifies with an outer tensor and an inner tensor; this header makes them from a point, and gives
 * the prover the claimed value without a round trip of a collapsed polynomial through the host.  The reference's univariate and
 * multilinear openings differ only in how the two tensors are computed from the point, and so do the bases below.
 *
 * The extension has its own prefix (lcpce_) and its own version.  Its symbols are exported by the same liblcpc_hip.so; nothing of
 * lcpc_hip.h or of the other extension headers changes.  A caller of this header checks lcpce_version() == LCPCE_VERSION (and the
 * core version as before).
 *
 * Elements are L little-endian 64-bit limbs in Montgomery form, fully reduced (< p), as everywhere at the ABI.
 *
 * Bases.  Coefficient e of a commitment is the element at row r = e / n_per_row, column j = e % n_per_row.  A basis gives each
 * coefficient the weight w(e) = outer[r] * inner[j]; the evaluation is the sum over e of coeffs[e] * w(e).
 *    LCPCE_POWERS        the point is ONE element x (n_point == 1).  inner[j] = x^j, outer[r] = x^(r * n_per_row), so w(e) = x^e:
 *                        the univariate polynomial with coefficients coeffs, at x.  Any n_rows, n_per_row >= 1 whose largest
 *                        exponent (n_rows - 1) * n_per_row fits 64 bits; the row count need not be a power of two.  The limbs
 *                        are those of a sequential chain of multiplications by x: field products are exact and the outputs fully
 *                        reduced, so every multiplication order gives the same limbs.
 *    LCPCE_ML_MONOMIAL   n_per_row = 2^a, n_rows = 2^b, n_point == a + b.  w(e) = the product of z_k over the set bits k of e.
 *    LCPCE_ML_LAGRANGE   the same shape rule.  w(e) = the product over k of (bit k of e set ? z_k : 1 - z_k), the equality basis:
 *                        the coefficients are the polynomial's values on the hypercube.
 *  - variable order, both multilinear bases: variable k is bit k of e, variable 0 the least significant bit.  inner is built from
 *    z_0 .. z_(a-1), outer from z_a .. z_(a+b-1).  a + b == 0 is legal: n_point == 0, both tensors are [1], and `point` may be NULL.
 *  - all three are one formula, out[i] = product over k of (bit k of i ? hi_k : lo_k), with i = j for the inner tensor and
 *    i = r * n_per_row for the outer one, and (lo_k, hi_k) = (1, x^(2^k)), (1, z_k), (1 - z_k, z_k).
 *
 * Status codes are lcpc_hip.h's.  Every error below is settled before any launch, and nothing is written on an error.
 *
 * Host call (no device, no context, no HIP call: it works on a machine without a GPU)
 *    the tensors call: point[n_point] -> outer[n_rows], inner[n_per_row]; field = LCPC_FT*.  Either output may be NULL, so a
 *    verifier that needs one tensor asks for one (both NULL is LCPC_ERR_ARG).  One multiplication per element (two for
 *    LCPCE_ML_LAGRANGE), one thread.  LCPC_ERR_ARG for an unknown field or basis, a NULL point with n_point > 0, n_rows or n_per_row
 *    of 0, an n_point that does not fit the basis and the shape, a multilinear basis on a dimension that is not a power of two, and a
 *    point whose limb pattern is >= p.
 *
 * Device calls.  A device array of elements is 16-byte aligned (8 bytes do for Ft63 and Ft191), as every device allocation is; a
 * pointer that is not is LCPC_ERR_ARG.  The device forms cannot look at their points without a synchronisation: points, and the
 * operands of the dot product, MUST be fully reduced (< p), or the results are unspecified.  n_points == 0 or n_points > 65535 is
 * LCPC_ERR_ARG.  Inputs and outputs must not overlap.
 *  - the device tensors call: n_points points at a stride of n_point elements -> outer_dev[n_points][n_rows],
 *    inner_dev[n_points][n_per_row] under the field of ctx, with the shape rules of the host call.  Either output may be NULL.
 *    Only enqueues on `stream`.  The table of (lo_k, hi_k) lives in the context's evaluation scratch; calls that use it on several
 *    streams are ordered behind each other by the library.
 *  - the dot call: out_dev[t] = the sum over i < n of a_dev[t * a_stride + i] * b_dev[t * b_stride + i] mod p for t < n_pairs
 *    (strides in elements; 0 shares one vector among all pairs), fully reduced Montgomery form.  Only enqueues; long vectors are
 *    summed in chunks through the context's evaluation scratch, as above.  n == 0, n_pairs == 0 or n_pairs > 65535 is LCPC_ERR_ARG.
 *  - evaluation with the caller's tensors: outer_dev[n_points][n_rows], inner_dev[n_points][n_per_row] of a committed object ->
 *    evals_dev[n_points].  The commitment is collapsed with each outer tensor -- two tensors per pass over the coefficients, the
 *    collapse of lcpc_collapse_device -- and each polynomial dotted with its inner tensor.  Only enqueues on `stream`.
 *  - evaluation at points: the device tensors step followed by the evaluation step, with n_rows and n_per_row taken from the
 *    commitment; nothing returns to the host in between.  Only enqueues on `stream`.
 *  - both take the locks of lcpc_collapse_device and are ordered behind the commit that filled the object.  Their scratch is the
 *    commitment's own, grown as needed (a growth waits for the device): as with lcpc_collapse_device, calls that use it on
 *    DIFFERENT streams must be ordered by the caller.  LCPC_ERR_STATE when nothing is committed and on a sharded encoder.
 *  - the host evaluation: points_host[n_points][n_point] -> evals_host[n_points].  One upload of the points, one download of
 *    n_points * L limbs, one synchronisation; complete on return.  It runs in a working set of the commitment as lcpc_collapse
 *    does, so any number of host threads may call it beside each other and beside a prove on the same commitment.  Points with a
 *    limb pattern >= p are LCPC_ERR_ARG.
 *  Round trip: prove with the outer tensor of a point, verify with both tensors -- lcpc_verify's eval_out holds the very limbs the
 *  evaluation calls return for that point.
 *  Out of scope: sharded encoders; batch forms over several commitments; a collapse of more than two tensors per pass.
 */
#ifndef LCPC_HIP_EVAL_H
#define LCPC_HIP_EVAL_H
#include "lcpc_hip.h"
#ifdef __cplusplus
extern "C" {
#endif

#define LCPCE_VERSION 1
int lcpce_version(void);

enum lcpce_basis { LCPCE_POWERS = 0, LCPCE_ML_MONOMIAL = 1, LCPCE_ML_LAGRANGE = 2 };

/* host: point[n_point][L] -> outer[n_rows][L], inner[n_per_row][L] (either may be NULL); field = LCPC_FT* */
int lcpce_tensors(uint32_t field, uint32_t basis, const uint64_t *point, uint32_t n_point, uint64_t n_rows, uint64_t n_per_row,
                  uint64_t *outer, uint64_t *inner);

/* device: points_dev[n_points][n_point] -> outer_dev[n_points][n_rows], inner_dev[n_points][n_per_row] (either may be NULL) on
 * `stream` (hipStream_t); enqueue only */
int lcpce_tensors_device(lcpc_ctx *ctx, uint32_t basis, const uint64_t *points_dev, uint32_t n_point, uint32_t n_points,
                         uint64_t n_rows, uint64_t n_per_row, uint64_t *outer_dev, uint64_t *inner_dev, void *stream);

/* device: out_dev[t] = sum_i a_dev[t * a_stride + i] * b_dev[t * b_stride + i], t < n_pairs, i < n; enqueue only */
int lcpce_dot_device(lcpc_ctx *ctx, const uint64_t *a_dev, uint64_t a_stride, const uint64_t *b_dev, uint64_t b_stride, uint64_t n,
                     uint32_t n_pairs, uint64_t *out_dev, void *stream);

/* device: evals_dev[t] = sum_e coeffs[e] * outer_dev[t][e / n_per_row] * inner_dev[t][e % n_per_row]; enqueue only */
int lcpce_eval_tensors_device(lcpc_commit_t *cm, const uint64_t *outer_dev, const uint64_t *inner_dev, uint32_t n_points, void *stream,
                              uint64_t *evals_dev);
/* device: the polynomial at points_dev[n_points][n_point] under `basis` -> evals_dev[n_points]; enqueue only */
int lcpce_eval_device(lcpc_commit_t *cm, uint32_t basis, const uint64_t *points_dev, uint32_t n_point, uint32_t n_points, void *stream,
                      uint64_t *evals_dev);
/* the same from host memory into host memory; complete on return */
int lcpce_eval(lcpc_commit_t *cm, uint32_t basis, const uint64_t *points_host, uint32_t n_point, uint32_t n_points,
               uint64_t *evals_host);

#ifdef __cplusplus
}
#endif
#endif

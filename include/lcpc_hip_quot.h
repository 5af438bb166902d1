/*
 * include/lcpc_hip_quot.h -- quotient extension of the C ABI of lcpc_hip.h: field inverses of whole vectors, pointwise arithmetic on
 * element vectors, and the division of columns of values on a domain by X - z or by the vanishing polynomial X^n - 1 -- all where the
 * data is.
 *
 * lcpc_hip_domain.h takes the columns of a univariate prover out to a coset g H_m and commits to a quotient from its values there.
 * The step between the two -- the constraint arithmetic on the values and the division by a denominator that is known in closed
 * form -- used to leave the device: there was no field inverse on it.  With this header the chain
 *    low-degree extension -> pointwise arithmetic -> quotient -> commit from coset values
 * and the opening chain
 *    values of a commitment -> its evaluation y = p(z) -> (p(X) - y) / (X - z) -> commit
 * stay in device memory.
 *
 * The extension has its own prefix (lcpcq_) and its own version.  Its symbols are exported by the same liblcpc_hip.so; nothing of
 * lcpc_hip.h or of the other extension headers changes.  A caller checks lcpcq_version() == LCPCQ_VERSION (and the core version).
 *
 * Conventions.  An element is L Montgomery limbs, fully reduced (< p).  Device arrays are aligned, vectors lie one after the other
 * (n_vecs vectors of m = 2^log_m elements), and lcpcd_order says where value k lies (LCPCD_NATURAL at [k], LCPCD_BITREV at
 * [rev_m(k)]) exactly as in lcpc_hip_domain.h, whose status codes these calls return.  Every error is settled before any launch and
 * nothing is written on an error.  Device calls only enqueue on `stream`; their inputs MUST be reduced, or the results are
 * unspecified.  Host calls touch no device and run on a machine without one, on one thread; an input element with a limb pattern
 * >= p is LCPC_ERR_ARG there, and they work on copies (LCPC_ERR_NOMEM when the host cannot hold them).  Everywhere an input array may
 * BE the output array (out == in, out == a, out == b); any other overlap of an input with the output is LCPC_ERR_ARG.  Common
 * LCPC_ERR_ARG: a NULL pointer (where NULL has no meaning of its own), an unknown field, op or order, a misaligned device pointer.
 *
 *  - batch inverse: out[i] = in[i]^-1, and zero for a zero input (as ff's batch_invert leaves zeros alone).  1 <= n < 2^39.  The
 *    host form is Montgomery's trick: one inversion and 3 (n - 1) multiplies.
 *  - pointwise: out[i] = a[i] op b[i] with op LCPCQ_ADD, LCPCQ_SUB, LCPCQ_MUL, or LCPCQ_DIV = a[i] b[i]^-1, which is zero where b[i]
 *    is zero.  1 <= n < 2^39.
 *  - division by X - z: vector v holds the values of a column at the points x_k = shift w_m^k, k < m.
 *        out_v[k] = (in_v[k] - y_v) / (x_k - z)
 *    shift and z are elements behind HOST pointers, read during the call; shift == NULL means the subgroup itself (shift = 1),
 *    otherwise it is nonzero and reduced.  y_dev holds n_vecs elements in DEVICE memory -- where lcpce_eval_device leaves p(z) -- and
 *    must not overlap the output; the host form takes one vector and one y behind a host pointer.  If z is a point of the domain a
 *    denominator vanishes: LCPC_ERR_ARG, decided on the host by (z / shift)^m == 1.  Bounds as for lcpcd_coset_fft_device: log_m at
 *    most S (host) or min(S, 32) (device), 1 <= n_vecs <= 65535, n_vecs * m < 2^39.
 *  - division by X^n - 1, n = 2^log_n, log_n <= log_m (LCPC_ERR_ARG otherwise):
 *        out_v[k] = in_v[k] / (x_k^n - 1)
 *    A denominator vanishes exactly when shift^m == 1: LCPC_ERR_ARG, and so is shift == NULL, the subgroup itself.  The
 *    denominators have period m / n in k; the bounds are those above.
 *
 * Each device call is ONE kernel launch, allocates nothing and caches no table of its own: the two divisions read the context's
 * forward twiddle table of m points, the one the transforms of that size use (its first use builds and uploads it, which waits for
 * that copy).  An inverse costs about 1.4 multiplies per bit of p; a workgroup gathers the inversions of a tile of 2048 or 4096
 * elements into the 64 lanes of one wave, and the two divisions invert once per POSITION and then walk the n_vecs vectors at it.
 *
 * Out of scope: a Rust binding; sharded encoders; z and shifts held in device memory; division of a polynomial in coefficient form.
 */
#ifndef LCPC_HIP_QUOT_H
#define LCPC_HIP_QUOT_H
#include "lcpc_hip.h"
#ifdef __cplusplus
extern "C" {
#endif

#define LCPCQ_VERSION 1
int lcpcq_version(void);

enum lcpcq_op { LCPCQ_ADD = 0, LCPCQ_SUB = 1, LCPCQ_MUL = 2, LCPCQ_DIV = 3 };

/* host: out[n][L] = in[n][L]^-1, zero for zero; out == in allowed */
int lcpcq_batch_inverse(uint32_t field, const uint64_t *in, uint64_t *out, uint64_t n);
/* device; enqueue only */
int lcpcq_batch_inverse_device(lcpc_ctx *ctx, const uint64_t *in_dev, uint64_t *out_dev, uint64_t n, void *stream);

/* host: out[i] = a[i] op b[i]; out may be a or b */
int lcpcq_pointwise(uint32_t field, uint32_t op, const uint64_t *a, const uint64_t *b, uint64_t *out, uint64_t n);
/* device; enqueue only */
int lcpcq_pointwise_device(lcpc_ctx *ctx, uint32_t op, const uint64_t *a_dev, const uint64_t *b_dev, uint64_t *out_dev, uint64_t n,
                           void *stream);

/* host: out[k] = (in[k] - y) / (shift w_m^k - z) over one vector of 2^log_m values; shift == NULL: the subgroup */
int lcpcq_divide_linear(uint32_t field, const uint64_t *shift, uint32_t order, const uint64_t *in, uint32_t log_m, const uint64_t *z,
                        const uint64_t *y, uint64_t *out);
/* device: n_vecs vectors, y_dev[n_vecs] in device memory, shift and z in host memory; enqueue only */
int lcpcq_divide_linear_device(lcpc_ctx *ctx, const uint64_t *shift, uint32_t order, const uint64_t *in_dev, uint32_t log_m,
                               uint32_t n_vecs, const uint64_t *z, const uint64_t *y_dev, uint64_t *out_dev, void *stream);

/* host: out[k] = in[k] / ((shift w_m^k)^n - 1), n = 2^log_n */
int lcpcq_divide_vanishing(uint32_t field, const uint64_t *shift, uint32_t order, const uint64_t *in, uint32_t log_m, uint32_t log_n,
                           uint64_t *out);
/* device: n_vecs vectors; enqueue only */
int lcpcq_divide_vanishing_device(lcpc_ctx *ctx, const uint64_t *shift, uint32_t order, const uint64_t *in_dev, uint32_t log_m,
                                  uint32_t log_n, uint32_t n_vecs, uint64_t *out_dev, void *stream);

#ifdef __cplusplus
}
#endif
#endif

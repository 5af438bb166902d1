/*
 * include/lcpc_hip_sumcheck.h -- sumcheck extension of the C ABI of lcpc_hip.h: the prover's two steps of a sumcheck round, the round
 * sums and the binding of a variable, where the tables are.
 *
 * The library commits to a multilinear polynomial (lcpc_static_get_dims_ml) and opens the commitment at a multilinear point
 * (lcpc_hip_eval.h, LCPCE_ML_LAGRANGE).  Between the two a multilinear prover runs sumcheck: v rounds over tables of 2^v elements,
 * each of which sums a product of tables over the hypercube at a few values of the current variable and then folds every table by
 * the verifier's challenge.  With this header both steps run on the tables in device memory; per round d + 1 elements come down.
 *
 * The extension has its own prefix (lcpcm_) and its own version.  Its symbols are exported by the same liblcpc_hip.so; nothing of
 * lcpc_hip.h or of the other extension headers changes.  A caller checks lcpcm_version() == LCPCM_VERSION (and the core version).
 *
 * Conventions.  An element is L Montgomery limbs, fully reduced (< p); every stored element is fully reduced.  The status codes are
 * those of lcpc_hip_domain.h.  Every error is settled on the host before anything is enqueued and nothing is written on an error.
 * Device calls only enqueue on `stream`, allocate nothing and cache nothing in the context; their inputs MUST be reduced, or the
 * results are unspecified.  Host calls touch no device and run on a machine without one, on one thread; an element, r or a
 * coefficient with a limb pattern >= p is LCPC_ERR_ARG there.  r and the coefficients are HOST limbs in the device calls too, checked
 * the same way.
 *
 * Definitions.  A table is n = 2^v elements, v >= 1: the values of a multilinear polynomial on the hypercube; variable k is bit k of
 * the index, exactly as for LCPCE_ML_LAGRANGE.  Let h = n / 2.  An order says which variable a round binds:
 *    LCPCM_LOW_FIRST    the lowest remaining variable:   (lo, hi)_i = (f[2i], f[2i+1])
 *    LCPCM_HIGH_FIRST   the highest remaining variable:  (lo, hi)_i = (f[i], f[i+h])
 *    ext(f, i, t) = lo_i + t (hi_i - lo_i)       for a field element t
 *    bind:          out[i] = ext(f, i, r), i < h: a table of h elements in the same order convention.
 * After v binds by r_0 ... r_(v-1) the one remaining value is the polynomial at the point z with z_k = r_k (low first) or
 * z_(v-1-k) = r_k (high first): the dot product of the table with the LCPCE_ML_LAGRANGE tensor of z.
 *
 * Composition.  Up to LCPCM_MAX_TABLES tables of one length and up to LCPCM_MAX_TERMS terms; a term is a product of 1 ...
 * LCPCM_MAX_FACTORS table indices (a repeated index, a square, is allowed) with one coefficient c_m.  Coefficients are host limbs
 * [n_terms][L]; NULL means all one.  The degree is d = max n_factors.
 *    round:  evals[t] = sum_{i<h} sum_m c_m prod_k ext(table[m][k], i, t)     for t = 0 ... d, d + 1 elements;
 * terms of lower degree are evaluated at every t too.  evals[0] + evals[1] is the sum of the composition over the whole tables.
 *
 * lcpcm_bind_round_device takes n >= 4, binds every table by r, writes the n / 2 bound elements of each, and in the same pass produces
 * the round evaluations of the BOUND tables: its stores and its evals_dev are byte for byte those of lcpcm_bind_device followed by
 * lcpcm_round_device on n / 2.  Its workspace is that of the round it replaces, lcpcm_round_work_bytes(ctx, n / 2, n_terms) (the
 * value for n is never smaller).
 *
 * Overlap.  On the device, under LCPCM_HIGH_FIRST out_dev[j] == in_dev[j] is allowed (a lane writes only positions it alone reads);
 * under LCPCM_LOW_FIRST any overlap of an output with an input is LCPC_ERR_ARG (lane i would write what lane i / 2 reads).  Any partial
 * overlap, outputs meeting each other, evals_dev or work_dev meeting anything else of the call is LCPC_ERR_ARG.  Inputs may repeat.
 * On the host out == in is allowed for both orders (one thread walks upward); any other overlap is LCPC_ERR_ARG.
 *
 * Further LCPC_ERR_ARG: n not a power of two, n < 2 (n < 4 for the fused form), n >= 2^39; n_tables, n_terms or an n_factors of 0 or
 * beyond its limit; a table index >= n_tables; an unknown field or order; a NULL or misaligned pointer (coeffs may be NULL);
 * work_bytes short of lcpcm_round_work_bytes; r or a coefficient >= p.
 *
 * The device calls: the round is one kernel over at most a fixed number of workgroups, each of which leaves one partial sum per
 * term and t in work_dev, and a second kernel that adds them and applies c_m -- a round that fits one workgroup (256 pairs) is one
 * launch.  The bind is one launch for all tables.  No workgroup waits for another, and field sums are exact: the limbs do not depend
 * on the grid.  work_dev is aligned like an element array; its contents after the call are unspecified.
 *
 * Out of scope: a Rust binding; sharded encoders; a C driver that owns the transcript (the reference defines no sumcheck wire
 * format); skipping g(1) by the claim; special forms for the eq polynomial; tables of unequal length; batches of instances.
 */
#ifndef LCPC_HIP_SUMCHECK_H
#define LCPC_HIP_SUMCHECK_H
#include "lcpc_hip.h"
#ifdef __cplusplus
extern "C" {
#endif

#define LCPCM_VERSION 1
int lcpcm_version(void);

enum lcpcm_order { LCPCM_LOW_FIRST = 0, LCPCM_HIGH_FIRST = 1 };

#define LCPCM_MAX_TABLES 8
#define LCPCM_MAX_TERMS 4
#define LCPCM_MAX_FACTORS 4
typedef struct { uint32_t n_factors; uint32_t table[LCPCM_MAX_FACTORS]; } lcpcm_term;

/* host, one table of n elements -> n / 2; out == in allowed */
int lcpcm_bind(uint32_t field, uint32_t order, const uint64_t *in, uint64_t *out, uint64_t n, const uint64_t *r);
/* host: evals[0 .. d] of the composition over n_tables tables of n elements */
int lcpcm_round(uint32_t field, uint32_t order, const uint64_t *const *tables, uint32_t n_tables, const lcpcm_term *terms,
                uint32_t n_terms, const uint64_t *coeffs, uint64_t n, uint64_t *evals);

/* the bytes of work_dev for a round over tables of n elements; 0 for arguments the round refuses and for a NULL context.  A pure host
 * function */
uint64_t lcpcm_round_work_bytes(const lcpc_ctx *ctx, uint64_t n, uint32_t n_terms);
/* device; enqueue only.  in_dev, out_dev, tables_dev: HOST arrays of n_tables device pointers */
int lcpcm_bind_device(lcpc_ctx *ctx, uint32_t order, const uint64_t *const *in_dev, uint64_t *const *out_dev, uint32_t n_tables,
                      uint64_t n, const uint64_t *r, void *stream);
int lcpcm_round_device(lcpc_ctx *ctx, uint32_t order, const uint64_t *const *tables_dev, uint32_t n_tables, const lcpcm_term *terms,
                       uint32_t n_terms, const uint64_t *coeffs, uint64_t n, uint64_t *evals_dev, void *work_dev, uint64_t work_bytes,
                       void *stream);
int lcpcm_bind_round_device(lcpc_ctx *ctx, uint32_t order, const uint64_t *const *in_dev, uint64_t *const *out_dev, uint32_t n_tables,
                            const lcpcm_term *terms, uint32_t n_terms, const uint64_t *coeffs, uint64_t n, const uint64_t *r,
                            uint64_t *evals_dev, void *work_dev, uint64_t work_bytes, void *stream);

#ifdef __cplusplus
}
#endif
#endif

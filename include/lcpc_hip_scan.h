/*
 * include/lcpc_hip_scan.h -- scan extension of the C ABI of lcpc_hip.h: prefix sums and prefix products of element vectors, where
 * the data is.
 *
 * lcpc_hip_quot.h keeps the chain low-degree extension -> constraint arithmetic -> quotient -> commit on the device.  One column of
 * a univariate prover is not a map of its inputs: the running accumulator,
 *    z[k+1] = z[k] num[k] / den[k]        the grand product of a permutation argument,
 *    s[k+1] = s[k] + m[k] / d[k]          the running sum of a log-derivative lookup,
 * carries a value from position k to k + 1.  With this header that column is built in device memory too: lcpcq_pointwise_device for
 * the terms, the scan here, lcpcf_commit_evals_device to commit to it.
 *
 * The extension has its own prefix (lcpcs_) and its own version.  Its symbols are exported by the same liblcpc_hip.so; nothing of
 * lcpc_hip.h or of the other extension headers changes.  A caller checks lcpcs_version() == LCPCS_VERSION (and the core version).
 *
 * Conventions.  An element is L Montgomery limbs, fully reduced (< p); every stored element is fully reduced.  The status codes are
 * those of lcpc_hip_domain.h.  Every error is settled on the host before anything is enqueued and nothing is written on an error.
 * Device calls only enqueue on `stream`; their inputs MUST be reduced, or the results are unspecified.  Host calls touch no device
 * and run on a machine without one, on one thread, in O(n); an input element with a limb pattern >= p is LCPC_ERR_ARG there.
 *
 * The scan.  (+) is + (LCPCS_SUM) or * (LCPCS_PRODUCT) in the field and e its identity.  There are n_vecs vectors of n elements, one
 * after the other, each scanned on its own (the host forms take one vector); n is any count, not a power of two.  With
 * c_v = init[v], or e where init is NULL,
 *    inclusive:  out_v[k] = c_v (+) in_v[0] (+) ... (+) in_v[k]
 *    exclusive:  out_v[k] = c_v (+) in_v[0] (+) ... (+) in_v[k-1], so out_v[0] = c_v
 *    both:       total[v] = c_v (+) in_v[0] (+) ... (+) in_v[n-1]            (total may be NULL)
 * A zero in a product scan is a value like any other: everything after it is zero, and no inverse is involved.  init_dev and
 * total_dev hold n_vecs elements in device memory, and the total_dev of one call may be the init_dev of the next, so a long column
 * can be scanned in pieces.
 *
 * The ratio forms scan the terms num[k] den[k]^-1, a zero term where den[k] is zero (LCPCQ_DIV's convention).  LCPCS_PRODUCT with
 * LCPCS_EXCLUSIVE is the accumulator of a permutation argument, whose total must be one; LCPCS_SUM is the log-derivative sum.  On the
 * device they are lcpcq_pointwise_device(LCPCQ_DIV) into out_dev followed by the scan in place.
 *
 * LCPC_ERR_ARG: n == 0, n_vecs == 0, n_vecs > 65535, n * n_vecs >= 2^39; an unknown field, op or mode; a NULL pointer other than
 * init and total, a misaligned device pointer; work_bytes < lcpcs_scan_work_bytes(ctx, n, n_vecs); an input that overlaps the output
 * without BEING it (out == in, out == num and out == den are allowed, for exclusive scans too); on the device, init_dev, total_dev
 * or work_dev meeting any other buffer of the call or each other.  On the host init and total may lie anywhere: init is read before
 * and total written after everything else.  The ratio forms on the host work on a copy (LCPC_ERR_NOMEM when the host cannot hold
 * it).
 *
 * The device calls allocate nothing and cache nothing in the context: work_dev, of lcpcs_scan_work_bytes bytes and aligned like an
 * element array, is the caller's, and its contents after the call are unspecified.  A vector that fits one tile of 2048 (L >= 3) or
 * 4096 elements is one kernel launch, n_vecs of them one launch still; longer vectors take three launches, and five beyond the
 * square of that tile (2^22 or 2^24 elements).  No workgroup of these kernels waits for another.  On the device one more bound
 * holds: a single vector of 2^35 elements or more (2^36 for L <= 2) is LCPC_ERR_ARG, and lcpcs_scan_work_bytes is 0 for it -- the
 * tiles of a vector are one dimension of the launch grid; no device holds such a vector.
 *
 * Out of scope: a Rust binding; sharded encoders; vectors of unequal length (segmented scans); bit-reversed order.
 */
#ifndef LCPC_HIP_SCAN_H
#define LCPC_HIP_SCAN_H
#include "lcpc_hip.h"
#ifdef __cplusplus
extern "C" {
#endif

#define LCPCS_VERSION 1
int lcpcs_version(void);

enum lcpcs_op { LCPCS_SUM = 0, LCPCS_PRODUCT = 1 };
enum lcpcs_mode { LCPCS_INCLUSIVE = 0, LCPCS_EXCLUSIVE = 1 };

/* host, one vector: init and total are one element each, or NULL; out == in allowed */
int lcpcs_scan(uint32_t field, uint32_t op, uint32_t mode, const uint64_t *in, uint64_t *out, uint64_t n, const uint64_t *init,
               uint64_t *total);
/* host, one vector: the scan of num[k] / den[k]; out may be num or den */
int lcpcs_scan_ratio(uint32_t field, uint32_t op, uint32_t mode, const uint64_t *num, const uint64_t *den, uint64_t *out, uint64_t n,
                     const uint64_t *init, uint64_t *total);

/* the bytes of work_dev for n_vecs vectors of n elements; 0 for arguments the scan refuses.  A pure host function */
uint64_t lcpcs_scan_work_bytes(const lcpc_ctx *ctx, uint64_t n, uint32_t n_vecs);
/* device; enqueue only */
int lcpcs_scan_device(lcpc_ctx *ctx, uint32_t op, uint32_t mode, const uint64_t *in_dev, uint64_t *out_dev, uint64_t n,
                      uint32_t n_vecs, const uint64_t *init_dev, uint64_t *total_dev, void *work_dev, uint64_t work_bytes,
                      void *stream);
int lcpcs_scan_ratio_device(lcpc_ctx *ctx, uint32_t op, uint32_t mode, const uint64_t *num_dev, const uint64_t *den_dev,
                            uint64_t *out_dev, uint64_t n, uint32_t n_vecs, const uint64_t *init_dev, uint64_t *total_dev,
                            void *work_dev, uint64_t work_bytes, void *stream);

#ifdef __cplusplus
}
#endif
#endif

/*
 * include/lcpc_hip_fft.h -- transform extension of the C ABI of lcpc_hip.h: the FieldFFT of a whole vector, on the host and on the
 * device, and a commit that reads the VALUES of a polynomial on a power-of-two subgroup instead of its coefficients.
 *
 * The core header commits to coefficients.  A caller of a univariate commitment often holds evaluations -- a trace column, a
 * quotient, whatever pointwise arithmetic left behind -- and the reference's users get from one to the other with the six
 * transforms of fffft's FieldFFT trait, the crate and the root of unity the Ligero encoder itself uses.  This header is that trait
 * where the data is, and the commit entry points run the inverse transform straight into the commitment's own coefficients.
 *
 * The extension has its own prefix (lcpcf_) and its own version.  Its symbols are exported by the same liblcpc_hip.so; nothing of
 * lcpc_hip.h or of the other extension headers changes.  A caller of this header checks lcpcf_version() == LCPCF_VERSION (and the
 * core version as before).
 *
 * Definitions.
 *    n = 2^log_n.  S is the field's two-adicity (lcpcf_max_log_n: 41, 40, 41, 41 for Ft63, Ft127, Ft191, Ft255).
 *    w = ROOT_OF_UNITY^(2^(S - log_n)) with ROOT_OF_UNITY = GENERATOR^((p - 1) / 2^S): fffft's root, and the encoder's -- a
 *    transform of length n_cols IS the Ligero encoder's transform.
 *    rev is bit reversal over log_n bits.
 *    Forward:  X[k] = sum_j x[j] w^(jk).          Inverse:  x[j] = n^-1 sum_k X[k] w^(-jk).
 *    The six forms carry fffft's names; the two letters give the order of input and output, i natural, o bit-reversed:
 *    LCPCF_FFT_IO stores X[k] at out[rev(k)]; LCPCF_IFFT_OI reads X[k] from in[rev(k)] and stores x[j] at out[j]; LCPCF_FFT_OI reads
 *    x[j] from in[rev(j)]; the II forms read and write in natural order.  log_n == 0 copies the element.
 *    Elements are L little-endian 64-bit limbs in Montgomery form, fully reduced (< p), as everywhere at the ABI.  Field arithmetic
 *    is exact and every output is fully reduced, so every decomposition and every twiddle scheme gives the same limbs: the host
 *    form, the device form at any size and fffft agree limb for limb.
 *
 * Status codes are lcpc_hip.h's.  Every error below is settled before any launch, and nothing is written on an error.
 *
 * Host call (no device, no context, no HIP call: it works on a machine without a GPU)
 *    the transform of in[n] into out[n] on one thread in O(n log n); field = LCPC_FT*.  in == out is allowed.  LCPC_ERR_ARG for
 *    an unknown field or form, a NULL pointer, log_n > S, an element whose limb pattern is >= p, and ranges that overlap without
 *    being equal.  (It works on a copy of n elements and a table of n / 2: LCPC_ERR_NOMEM when the host cannot hold them.)
 *
 * Device calls.  A device array of elements is 16-byte aligned (8 bytes do for Ft63 and Ft191), as every device allocation is; a
 * pointer that is not is LCPC_ERR_ARG.  The device forms cannot look at their input without a synchronisation: it MUST be fully
 * reduced (< p), or the results are unspecified.
 *  - the device transform: n_vecs vectors that lie one after the other at a stride of n elements, each transformed on its own,
 *    under the field of ctx.  Only enqueues on `stream`.  in_dev == out_dev means in place; otherwise the two ranges must not
 *    overlap, and in_dev is only read.  LCPC_ERR_ARG for a NULL or misaligned pointer, an unknown form, log_n > min(S, 32),
 *    n_vecs == 0 or n_vecs > 65535, n_vecs * n >= 2^39 (the kernels' grids), and ranges that overlap without being equal.
 *    A transform runs ceil(log_n / 10) passes over the data (one more for the II forms, whose permutation is a pass of its own) and
 *    needs no scratch.  Its twiddles are a two-level table of 2^floor(log_n / 2) + 2^ceil(log_n / 2) elements per size and
 *    direction -- never n / 2 -- which lives in the context and is freed with it; the tables of the last four (size, direction)
 *    pairs stay cached.  The first call for a pair builds its table on the host and uploads it, which waits for that copy; a
 *    table is read-only afterwards, so calls on several streams need no order among each other.  A context that never calls the
 *    extension allocates nothing for it.
 *  - commit from evaluations: after the call the object is in exactly the state lcpc_commit_device leaves for the 2^log_n
 *    coefficients of the interpolating polynomial -- dims, coeffs, comm, hashes and root -- so prove, collapse, open, the
 *    evaluation extension, the getters, bincode and the batch prove work unchanged.  `order` says where the caller keeps p(w^i):
 *    LCPCF_NATURAL evals[i] = p(w^i), LCPCF_BITREV evals[rev(i)] = p(w^i).  The caller's buffer is only read: the first step of the
 *    inverse transform writes into the commitment's own coeffs, the rest runs there in place, and the encode reads coeffs where they
 *    lie; no further buffer is taken.  root == NULL only enqueues and records the commitment's event; otherwise the call waits for
 *    the root as lcpc_commit_device does.  Any encoder (Ligero, Brakedown) and any digest.  Locks, the order behind the previous
 *    fill and the un-commit on failure are lcpc_commit_device's.  LCPC_ERR_ARG for a NULL or misaligned evals_dev, an unknown order,
 *    log_n > min(S, 32); LCPC_ERR_STATE on a sharded encoder; both leave a committed object as it was.
 *  - the host form: one upload of the evaluations into coeffs, then the device form in place; complete on return.  Elements with
 *    a limb pattern >= p are LCPC_ERR_ARG.
 *  Out of scope: sharded encoders; batch forms of the commit.  Coset transforms, the low-degree extension and the values of a
 *  commitment on a domain are lcpc_hip_domain.h's.
 */
#ifndef LCPC_HIP_FFT_H
#define LCPC_HIP_FFT_H
#include "lcpc_hip.h"
#ifdef __cplusplus
extern "C" {
#endif

#define LCPCF_VERSION 1
int lcpcf_version(void);

enum lcpcf_form { LCPCF_FFT_II = 0, LCPCF_FFT_IO = 1, LCPCF_FFT_OI = 2, LCPCF_IFFT_II = 3, LCPCF_IFFT_IO = 4, LCPCF_IFFT_OI = 5 };
enum lcpcf_order { LCPCF_NATURAL = 0, LCPCF_BITREV = 1 };

/* S, the largest log_n of `field` (LCPC_FT*); 0 for an unknown field */
uint32_t lcpcf_max_log_n(uint32_t field);

/* host: in[2^log_n][L] -> out[2^log_n][L] under `form`; in == out allowed */
int lcpcf_fft(uint32_t field, uint32_t form, const uint64_t *in, uint64_t *out, uint32_t log_n);

/* device: n_vecs vectors of 2^log_n elements, one after the other, on `stream` (hipStream_t); enqueue only */
int lcpcf_fft_device(lcpc_ctx *ctx, uint32_t form, const uint64_t *in_dev, uint64_t *out_dev, uint32_t log_n, uint32_t n_vecs,
                     void *stream);

/* commit to the polynomial of degree < 2^log_n with the given values on the subgroup; evaluations in HBM, read only */
int lcpcf_commit_evals_device(lcpc_commit_t *cm, uint32_t order, const uint64_t *evals_dev, uint32_t log_n, void *stream,
                              uint8_t *root);
/* the same from host memory; complete on return */
int lcpcf_commit_evals(lcpc_commit_t *cm, uint32_t order, const uint64_t *evals_host, uint32_t log_n, uint8_t *root);

#ifdef __cplusplus
}
#endif
#endif

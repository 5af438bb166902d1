/*
 * include/lcpc_hip_domain.h -- domain extension of the C ABI of lcpc_hip.h: transforms on a COSET s H of a power-of-two subgroup, the
 * low-degree extension of columns from one domain to a larger one, a commit that reads values on a coset, and the values of a
 * committed polynomial on a domain of the caller's choice -- all where the data is.
 *
 * lcpc_hip_fft.h is fffft's FieldFFT on the subgroup H_n.  A univariate prover works one step further out: a quotient is computed
 * pointwise on g H_m with m = 2^b n, because on H_n its denominator vanishes.  To get there it needs the low-degree extension of its
 * columns -- values on H_n to values on g H_m -- and to come back it commits to the quotient from its values on the coset.  Both used
 * to take a trip through the host, or three device steps (inverse transform, copy into a zeroed buffer of m elements, forward
 * transform of length m) that could not apply a shift at all.
 *
 * The extension has its own prefix (lcpcd_) and its own version.  Its symbols are exported by the same liblcpc_hip.so; nothing of
 * lcpc_hip.h or of the other extension headers changes.  A caller checks lcpcd_version() == LCPCD_VERSION (and the core version).
 *
 * Definitions.
 *    n = 2^log_n.  S, the root w_n of the subgroup of n points, bit reversal rev and the six form names are exactly lcpc_hip_fft.h's.
 *    A shift s is any NONZERO element: L Montgomery limbs behind a HOST pointer, fully reduced (< p), read during the call.
 *    lcpcd_generator gives the shift everybody uses, ff's multiplicative_generator(): 10, 3, 5, 5 for Ft63, Ft127, Ft191, Ft255.
 *    D(s, n) = { s w_n^k : k < n }.
 *    Coset forward:  X[k] = p(s w_n^k) = sum_j x[j] s^j w_n^(jk).      Coset inverse:  x[j] = s^-j n^-1 sum_k X[k] w_n^(-jk).
 *    The two letters of a form give the order of input and output as in lcpcf_: LCPCD_FFT_IO stores X[k] at out[rev(k)], and so on.
 *    s = 1 gives lcpcf_'s limbs exactly.  All arithmetic is exact and every stored element is fully reduced, so every decomposition
 *    agrees limb for limb: the host forms, the device forms at any size, and a plain transform of a vector scaled beforehand.
 *    Extension:  Y[k] = sum_{j < n_coeffs} x[j] s^j w_m^(jk) for k < m = 2^log_m -- the values on D(s, m) of the polynomial with the
 *    coefficients x.  n_coeffs is any number with 1 <= n_coeffs <= m, not necessarily a power of two.  With order LCPCD_NATURAL Y[k]
 *    is stored at out[k], with LCPCD_BITREV at out[rev_m(k)].
 *
 * Status codes are lcpc_hip.h's.  Every error below is settled before any launch, and nothing is written on an error.  Common to all
 * calls, LCPC_ERR_ARG: a NULL pointer (where NULL has no meaning of its own), an unknown field, form or order, a shift that is zero
 * or whose limb pattern is >= p, log_n or log_m above S (host) or above min(S, 32) (device).
 *
 * Host calls (no device, no context, no HIP call: they work on a machine without a GPU), one thread, O(m log m):
 *  - the coset transform of in[n] into out[n]; in == out is allowed, ranges that overlap otherwise are LCPC_ERR_ARG, and so is an
 *    input element with a limb pattern >= p.
 *  - the extension of coeffs[n_coeffs] into out[m]: LCPC_ERR_ARG for n_coeffs == 0 or n_coeffs > m, an input element >= p, and
 *    ranges that overlap unless coeffs == out.
 *    (Both work on a copy: LCPC_ERR_NOMEM when the host cannot hold it.)
 *
 * Device calls.  A device array of elements is 16-byte aligned (8 bytes do for Ft63 and Ft191); a pointer that is not is
 * LCPC_ERR_ARG.  Device inputs MUST be fully reduced, or the results are unspecified.  All of them only enqueue on `stream`.
 *  - the coset transform: n_vecs vectors at a stride of n elements under the field of ctx, in place (in_dev == out_dev) or into a
 *    range that does not overlap the input, which is then only read.  LCPC_ERR_ARG as for the device transform of lcpc_hip_fft.h:
 *    n_vecs == 0 or > 65535, n_vecs * n >= 2^39, ranges that overlap without being equal.  It takes exactly the kernel launches of the
 *    plain transform of its form and size: the multiplication by s^j (forward) or s^-j n^-1 (inverse) happens in the pass that loads
 *    the input or stores the output, with j the element's natural index whatever the storage order.  No pass over memory scales.
 *  - the extension: source vector v starts at coeffs_dev + v 2^ceil(log2 n_coeffs) elements and only its first n_coeffs elements are
 *    read; output vector v starts at out_dev + v m.  Source and output must not overlap.  LCPC_ERR_ARG for n_coeffs == 0 or > m,
 *    n_vecs == 0, n_vecs 2^(log_m - ceil(log2 n_coeffs)) > 65535, n_vecs * m >= 2^39.  With nb = 2^ceil(log2 n_coeffs) and m = 2^b nb,
 *    block c of the bit-reversed output -- out[c nb .. (c + 1) nb) -- is the LCPCD_FFT_IO coset transform of the zero-padded
 *    coefficients with the shift s w_m^rev_b(c).  The kernels compute it that way: 2^b transforms of nb points that all read the same
 *    coefficients, never a padded buffer of m elements, and log nb stages instead of log m.  LCPCD_BITREV takes exactly the launches of
 *    an FFT_IO of nb points whatever b is (one launch where a single coefficient spreads over m > 1 values); LCPCD_NATURAL takes
 *    one more, the bit-reversal permutation in place on the output.
 *  - the low-degree extension: values on D(shift_in, n) -> values on D(shift_out, m), log_m >= log_n, n_vecs columns.  shift_in ==
 *    NULL means the subgroup itself.  in_order / out_order say where value k lies (LCPCD_NATURAL at [k], LCPCD_BITREV at [rev(k)]).
 *    It is the coset inverse into work_dev followed by the extension from there.  work_dev holds n_vecs * n elements and holds the
 *    COEFFICIENTS afterwards (natural order), which callers want anyway; it may equal in_dev, which is then overwritten, and
 *    otherwise must not overlap it; neither may overlap out_dev (n_vecs * m elements).  log_m == log_n is the pure change of coset.
 *    The library allocates nothing for data.  LCPC_ERR_ARG: n_vecs == 0, n_vecs 2^(log_m - log_n) > 65535, n_vecs * m >= 2^39,
 *    log_m < log_n, forbidden overlaps.
 *  - commit from values on a coset: the polynomial of degree < n with the given values on D(shift, n).  After the call the object is
 *    in exactly the state the device commit of the core header leaves for the interpolated coefficients -- dims, coeffs, comm, hashes
 *    and root.  `order` as above.  The inverse transform writes straight into the commitment's own coeffs and the caller's buffer is
 *    only read; root == NULL only enqueues.  Locks, the order behind the previous fill and the un-commit on failure are those of
 *    lcpcf_commit_evals_device.  The host form uploads the values into coeffs, runs the device form in place and is complete on
 *    return; values with a limb pattern >= p are LCPC_ERR_ARG.  LCPC_ERR_STATE on a sharded encoder.
 *  - the values of a commitment: Y[k] = sum_i coeffs[i] (shift w_m^k)^i into the caller's out_dev[m], i over the n_rows * n_per_row
 *    padded coefficients of the object, which are read where they lie.  2^log_m must be at least that number (LCPC_ERR_ARG), and
 *    out_dev must not overlap the object's buffers.  A reader of the object like the device collapse of the core header: ordered
 *    behind the commitment's event, no lock beyond what readers take, enqueue only.  LCPC_ERR_STATE on an object that holds no
 *    commitment and on a sharded encoder.
 *
 * Shift tables.  A power of a shift is the product of two entries of a table of 2^floor(log_n / 2) + 2^ceil(log_n / 2) elements per
 * (shift, size, direction) -- never n.  The tables live in the context beside the twiddle tables and are freed with it; the last eight
 * stay cached.  The first call for a key builds its table on the host and uploads it, which waits for that copy; a table is
 * read-only afterwards, so calls on several streams need no order among each other, and a table is evicted only after everything
 * that reads it has finished.
 *
 * Out of scope: a Rust binding; batch forms; sharded encoders; shifts held in device memory.
 */
#ifndef LCPC_HIP_DOMAIN_H
#define LCPC_HIP_DOMAIN_H
#include "lcpc_hip.h"
#ifdef __cplusplus
extern "C" {
#endif

#define LCPCD_VERSION 1
int lcpcd_version(void);

/* lcpcf_form's numbering */
enum lcpcd_form { LCPCD_FFT_II = 0, LCPCD_FFT_IO = 1, LCPCD_FFT_OI = 2, LCPCD_IFFT_II = 3, LCPCD_IFFT_IO = 4, LCPCD_IFFT_OI = 5 };
enum lcpcd_order { LCPCD_NATURAL = 0, LCPCD_BITREV = 1 };

/* out[L]: multiplicative_generator() of `field` (LCPC_FT*) in Montgomery limbs */
int lcpcd_generator(uint32_t field, uint64_t *out);

/* host: in[2^log_n][L] -> out[2^log_n][L] on the coset of `shift`; in == out allowed */
int lcpcd_coset_fft(uint32_t field, uint32_t form, const uint64_t *shift, const uint64_t *in, uint64_t *out, uint32_t log_n);

/* device: n_vecs vectors of 2^log_n elements, one after the other; enqueue only */
int lcpcd_coset_fft_device(lcpc_ctx *ctx, uint32_t form, const uint64_t *shift, const uint64_t *in_dev, uint64_t *out_dev,
                           uint32_t log_n, uint32_t n_vecs, void *stream);

/* host: coeffs[n_coeffs][L] -> out[2^log_m][L], the values on D(shift, 2^log_m) */
int lcpcd_extend(uint32_t field, const uint64_t *shift, const uint64_t *coeffs, uint64_t n_coeffs, uint32_t log_m, uint32_t order,
                 uint64_t *out);

/* device: n_vecs coefficient vectors 2^ceil(log2 n_coeffs) apart -> n_vecs value vectors 2^log_m apart; enqueue only */
int lcpcd_extend_device(lcpc_ctx *ctx, const uint64_t *shift, const uint64_t *coeffs_dev, uint64_t n_coeffs, uint32_t log_m,
                        uint32_t order, uint64_t *out_dev, uint32_t n_vecs, void *stream);

/* device: values on D(shift_in, 2^log_n) -> values on D(shift_out, 2^log_m); work_dev keeps the coefficients; enqueue only */
int lcpcd_lde_device(lcpc_ctx *ctx, uint32_t in_order, const uint64_t *shift_in, const uint64_t *in_dev, uint32_t log_n,
                     const uint64_t *shift_out, uint32_t log_m, uint32_t out_order, uint64_t *out_dev, uint64_t *work_dev,
                     uint32_t n_vecs, void *stream);

/* commit to the polynomial of degree < 2^log_n with the given values on D(shift, 2^log_n); values in HBM, read only */
int lcpcd_commit_coset_evals_device(lcpc_commit_t *cm, uint32_t order, const uint64_t *shift, const uint64_t *evals_dev,
                                    uint32_t log_n, void *stream, uint8_t *root);
/* the same from host memory; complete on return */
int lcpcd_commit_coset_evals(lcpc_commit_t *cm, uint32_t order, const uint64_t *shift, const uint64_t *evals_host, uint32_t log_n,
                             uint8_t *root);

/* the values of the committed polynomial on D(shift, 2^log_m) into out_dev; a reader of cm; enqueue only */
int lcpcd_commit_values_device(lcpc_commit_t *cm, const uint64_t *shift, uint32_t log_m, uint32_t order, uint64_t *out_dev,
                               void *stream);

#ifdef __cplusplus
}
#endif
#endif

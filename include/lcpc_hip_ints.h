/*
 * include/lcpc_hip_ints.h -- plain-integer extension of the C ABI of lcpc_hip.h: for callers who do not hold ff elements.
 *
 * Every element that crosses the core header is L little-endian 64-bit limbs in ff_derive's Montgomery form.  A C, C++ or Python
 * caller whose witness is a vector of uint32_t or int64_t has no such limbs.  This header turns integers into field elements -- on the
 * host for the handful of elements of a tensor, a point or an evaluation, on the device for a witness -- and commits straight from
 * the integers: they cross the bus as they are (4 or 8 bytes each instead of 8 L) and are widened and converted in HBM.
 *
 * The extension has its own prefix (lcpci_) and its own version.  Its symbols are exported by the same liblcpc_hip.so; nothing of
 * lcpc_hip.h, lcpc_hip_batch.h, lcpc_hip_verify.h or lcpc_hip_columns.h changes.  A caller of this header checks
 * lcpci_version() == LCPCI_VERSION (and the core version as before).
 *
 * Integer kinds.  ONE rule for all of them: the input is an integer v and denotes the field element v mod p in the mathematical
 * sense -- for a negative v that is p - (|v| mod p), and 0 stays 0.
 *    LCPCI_U32, LCPCI_I32    4 bytes per element, unsigned / two's complement
 *    LCPCI_U64, LCPCI_I64    8 bytes per element
 *    LCPCI_WIDE              L x uint64_t per element, little-endian limbs: an unsigned integer of 64 L bits
 *  - the output is always the fully reduced Montgomery form (< p): bit for bit the Montgomery product of v mod p and R^2.
 *  - there is NO error path for values >= p.  LCPCI_WIDE is an integer input, not a checked representation: 2^(64 L) - 1 is as
 *    good an input as 1 and is reduced like any other.  (The rest of the library refuses stored limbs >= p; those are representations.
 *    This header never reads stored limbs except in the canonical-value call below, whose input is a Montgomery form < p.)  The
 *    rule needs no flag and no synchronisation, so the device forms only enqueue.
 *  - alignment: an input needs the natural alignment of its element only (4 or 8 bytes; LCPCI_WIDE: 8) -- a slice of a larger array
 *    may start at any element.  An output of field elements on the device is 16-byte aligned (8 bytes do for Ft63 and Ft191), as every
 *    device allocation is.  A pointer that is not is LCPC_ERR_ARG.
 *  - output and input must not overlap.
 *
 * Host calls (no device, no context, no HIP call: they work on a machine without a GPU)
 *    the from-integers call: n integers of `kind` -> out_mont[n][L].  The canonical-value call: in_mont[n][L] (Montgomery forms < p)
 *    -> out_canon[n][L], the canonical integers as L limbs (PrimeField::to_repr's limbs).  Meant for tensors, points and evaluations
 *    (thousands of elements, one thread).  An unknown field or kind, or a NULL pointer with n > 0, is LCPC_ERR_ARG; n == 0 returns 0.
 *
 * Device conversion
 *    n integers at in_dev -> out_dev[n][L] on `stream` under the field of ctx.  Only enqueues.  One element per lane, the grid sized
 *    to n.  LCPC_ERR_ARG for a NULL ctx / in_dev / out_dev, n == 0, an unknown kind or a misaligned pointer.
 *
 * Commit from integers
 *    After either commit call the object is in exactly the state the core device commit would leave it in for the Montgomery forms
 *    of the same values with the same n: dims, coeffs (with the zero tail of a ragged last row), comm, hashes, root.  Every reader works
 *    on it unchanged -- prove, collapse, open, the getters, the bincode writer, the batch prove.  The object owns its coeffs.
 *  - device form: vals_dev holds n integers.  With root == NULL the call only enqueues on `stream` and records the commitment's
 *    event, as the core device commit does; the caller's buffer is read until the stream reaches that point.  With a root it returns
 *    after the root is on the host.
 *  - host form: vals_host may be pageable or pinned.  Small inputs, Brakedown encoders and timing runs: one upload of the integers,
 *    the widening kernel, the resident pipeline.  Large Ligero inputs take the row-batch pipeline of the core host commit, the
 *    integers of a batch uploaded on the copy stream and widened on the compute stream in front of that batch's encode.  The switch
 *    is at the same n as the core host commit's (64 MiB of Montgomery limbs, 16 rows).  Pageable sources go through the encoder's
 *    ring of pinned bounce buffers.  The call returns after the work is complete: the caller's buffer is free on return.
 *  - locks, ordering behind the previous fill and the un-commit on failure are those of the core commit entry points: a failed call
 *    leaves the object uncommitted.  LCPC_ERR_ARG for a NULL object / pointer, n == 0 or an unknown kind (nothing is touched);
 *    LCPC_ERR_STATE on a sharded encoder.
 *  Out of scope: batch forms; sharded encoders; any check that an input is < p.
 */
#ifndef LCPC_HIP_INTS_H
#define LCPC_HIP_INTS_H
#include "lcpc_hip.h"
#ifdef __cplusplus
extern "C" {
#endif

#define LCPCI_VERSION 1
int lcpci_version(void);

enum lcpci_kind { LCPCI_U32 = 0, LCPCI_I32 = 1, LCPCI_U64 = 2, LCPCI_I64 = 3, LCPCI_WIDE = 4 };

/* host: in[n] integers of `kind` -> out_mont[n][L]; field = LCPC_FT* */
int lcpci_from_ints(uint32_t field, uint32_t kind, const void *in, uint64_t n, uint64_t *out_mont);
/* host: in_mont[n][L] -> out_canon[n][L], the canonical integers */
int lcpci_to_canon(uint32_t field, const uint64_t *in_mont, uint64_t n, uint64_t *out_canon);

/* device: in_dev[n] integers of `kind` -> out_dev[n][L] on `stream` (hipStream_t); enqueue only */
int lcpci_from_ints_device(lcpc_ctx *ctx, uint32_t kind, const void *in_dev, uint64_t n, uint64_t *out_dev, void *stream);

/* commit n integers in HBM; root (optional): the digest on the host, after a synchronisation of `stream` */
int lcpci_commit_ints_device(lcpc_commit_t *cm, uint32_t kind, const void *vals_dev, uint64_t n, void *stream, uint8_t *root);
/* commit n integers in host memory (pageable or pinned); complete on return */
int lcpci_commit_ints(lcpc_commit_t *cm, uint32_t kind, const void *vals_host, uint64_t n, uint8_t *root);

#ifdef __cplusplus
}
#endif
#endif

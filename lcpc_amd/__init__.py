"""lcpc_amd -- host-side mirror of conroi/lcpc's LcEncoding / LcCommit / prove / verify API over the
MI355X-native C ABI (include/lcpc_hip.h).  The reference's toolchain (Rust) is absent from this image, so
the host side above the C ABI is Python + ctypes with the reference's names, argument meaning and error
behaviour; INTEGRATION.md shows the Rust `extern "C"` binding a maintainer would add instead.

Field elements are numpy uint64 arrays of shape (n, L): ff_derive's Montgomery limbs, exactly what a Rust
`&[FtN]` is in memory.  (/root/reference citations: see include/lcpc_hip.h.)"""
import ctypes as C

import numpy as np

from . import _lib
from ._lib import LcpcParams, LcpcTimings

FT63, FT127, FT191, FT255 = 0, 1, 2, 3
FIELD_LIMBS = {FT63: 1, FT127: 2, FT191: 3, FT255: 4}
ENC_LIGERO, ENC_SDIG = 0, 1
# D of LcCommit<D, E>: LCPC_HASH_BLAKE3 / LCPC_HASH_SHA3_256 (include/lcpc_hip.h)
DIGESTS = {"blake3": 0, "sha3_256": 1}
# every digest `digest=` accepts: DIGESTS plus LCPC_HASH_BLAKE2B (BLAKE2b-512), and the bytes of one Output<D> of each -- a root,
# a `hashes` slot, a path entry
ALL_DIGESTS = dict(DIGESTS, blake2b=2)
DIGEST_LEN = {"blake3": 32, "sha3_256": 32, "blake2b": 64}
# the table `digest=` is looked up in: the three above plus LCPC_HASH_KECCAK256 (Keccak-256, the pre-FIPS padding of the EVM's
# KECCAK256) and LCPC_HASH_SHA256 -- name -> (lcpc_params.hash, bytes of one Output<D>)
DIGEST_TABLE = {"blake3": (0, 32), "sha3_256": (1, 32), "blake2b": (2, 64), "keccak256": (3, 32), "sha256": (4, 32)}


class LcpcError(RuntimeError):
    """a negative lcpc_status; .code mirrors ProverError / VerifierError (lcpc-2d/src/lib.rs:111-166)."""

    def __init__(self, code, detail=""):
        self.code = code
        msg = _lib.lib().lcpc_strerror(code).decode()
        super().__init__("%s (%d)%s" % (msg, code, (": " + detail) if detail else ""))


ERR_TOO_BIG, ERR_ENCODE, ERR_COMMIT, ERR_COLUMN_NUMBER, ERR_OUTER_TENSOR, ERR_DIMS, ERR_ARG, ERR_STATE = -1, -2, -3, -4, -5, -6, -7, -8
VERR_NUM_COL_OPENS, VERR_COLUMN_PATH, VERR_COLUMN_EVAL, VERR_COLUMN_DEGREE = -32, -33, -34, -35
VERR_OUTER_TENSOR, VERR_INNER_TENSOR, VERR_ENCODING_DIMS, VERR_ENCODE, VERR_MALFORMED = -36, -37, -38, -39, -40


def _ptr(a):
    return a.ctypes.data_as(C.c_void_p)


def _elems(a, L):
    a = np.ascontiguousarray(a, dtype=np.uint64)
    if a.size % L:
        raise ValueError("element array size is not a multiple of L")
    return a


# the four moduli (lcpc-test-fields/src/lib.rs:13-59), for the plain-integer calls (include/lcpc_hip_ints.h): Python ints are reduced here
FIELD_MODULUS = {FT63: 0x46d0760000000001, FT127: 0x6e754097ba20e0bf7f2bd90000000001,
                 FT191: 0x453708aa3fbc8dda936888270ceecbcdd246820000000001,
                 FT255: 0x663c799b6e4d2900fda9df04b9575969ef73c79086595f3002a4f20000000001}
_INT_BYTES = {"u32": 4, "i32": 4, "u64": 8, "i64": 8}
_INT_DTYPE_KIND = {"uint32": "u32", "int32": "i32", "uint64": "u64", "int64": "i64"}


def _int_kind(dtype, shape, L, kind):
    """(lcpci_kind, element count) of an integer array of `dtype` (numpy's or torch's, by name) and `shape`; kind=None goes by the
    dtype, "wide" reads (n, L) 64-bit limbs, and a kind of the dtype's width re-reads its storage (int64 storage as "u64")."""
    name = str(dtype).replace("torch.", "")
    if name not in _INT_DTYPE_KIND:
        raise ValueError("integer values must be uint32 / int32 / uint64 / int64, not %s" % name)
    n = 1
    for d in shape:
        n *= int(d)
    if kind is None:
        kind = _INT_DTYPE_KIND[name]
    if kind not in _lib.INTS_KINDS:
        raise ValueError("kind must be one of %s, not %r" % (sorted(_lib.INTS_KINDS), kind))
    if kind == "wide":
        if _INT_BYTES[_INT_DTYPE_KIND[name]] != 8 or len(shape) != 2 or shape[1] != L:
            raise ValueError('kind="wide" takes an (n, L) array of 64-bit limbs')
        n //= L
    elif _INT_BYTES[kind] != _INT_BYTES[_INT_DTYPE_KIND[name]]:
        raise ValueError("kind %r does not have the width of %s" % (kind, name))
    return _lib.INTS_KINDS[kind], n


def _basis(basis):
    if basis not in _lib.EVAL_BASES:
        raise ValueError("basis must be one of %s, not %r" % (sorted(_lib.EVAL_BASES), basis))
    return _lib.EVAL_BASES[basis]


def _n_point(basis, n_rows, n_per_row):
    """elements per point (include/lcpc_hip_eval.h): one for "powers", one per variable for the multilinear bases"""
    return 1 if basis == "powers" else (n_rows * n_per_row).bit_length() - 1


def tensors(field, point, n_rows, n_per_row, basis="powers"):
    """lcpce_tensors (include/lcpc_hip_eval.h): the (outer (n_rows, L), inner (n_per_row, L)) tensors that open a polynomial of
    n_rows x n_per_row coefficients at `point`.  basis="powers": point is one element x, outer[r] = x^(r n_per_row), inner[j] = x^j;
    "ml_monomial" / "ml_lagrange": point is (n_vars, L), variable k = bit k of the coefficient index.  A host call: no device."""
    L = FIELD_LIMBS[field]
    p = _elems(point, L)
    outer, inner = np.zeros((n_rows, L), np.uint64), np.zeros((n_per_row, L), np.uint64)
    rc = _lib.lib().lcpce_tensors(field, _basis(basis), _ptr(p) if p.size else None, p.size // L, n_rows, n_per_row, _ptr(outer), _ptr(inner))
    if rc:
        raise LcpcError(rc)
    return outer, inner


def _form(form):
    if form not in _lib.FFT_FORMS:
        raise ValueError("form must be one of %s, not %r" % (sorted(_lib.FFT_FORMS), form))
    return _lib.FFT_FORMS[form]


def _log_n(n):
    if n < 1 or n & (n - 1):
        raise ValueError("a transform takes a power-of-two number of elements, not %d" % n)
    return n.bit_length() - 1


def fft(field, x, form="fft_io"):
    """lcpcf_fft (include/lcpc_hip_fft.h): fffft's FieldFFT of the (n, L) elements x, n a power of two, under the encoder's own root of
    unity.  form: "fft_ii" / "fft_io" / "fft_oi" / "ifft_ii" / "ifft_io" / "ifft_oi", the two letters the order of input and output
    (i natural, o bit-reversed).  A host call: no device."""
    L = FIELD_LIMBS[field]
    a = _elems(x, L).reshape(-1, L)
    out = np.zeros_like(a)
    rc = _lib.lib().lcpcf_fft(field, _form(form), _ptr(a), _ptr(out), _log_n(a.shape[0]))
    if rc:
        raise LcpcError(rc)
    return out


def _order(order):
    if order not in _lib.DOMAIN_ORDERS:
        raise ValueError("order must be one of %s, not %r" % (sorted(_lib.DOMAIN_ORDERS), order))
    return _lib.DOMAIN_ORDERS[order]


def _shift(shift, L):
    """one element: the L limbs of a shift, in host memory"""
    s = np.ascontiguousarray(shift, dtype=np.uint64).reshape(-1)
    if s.size != L:
        raise ValueError("a shift is one element of %d limbs" % L)
    return s


def generator(field):
    """lcpcd_generator (include/lcpc_hip_domain.h): ff's multiplicative_generator() of the field as (L,) Montgomery limbs -- the
    coset shift everybody uses."""
    out = np.zeros(FIELD_LIMBS[field], np.uint64)
    rc = _lib.lib().lcpcd_generator(field, _ptr(out))
    if rc:
        raise LcpcError(rc)
    return out


def coset_fft(field, x, shift, form="fft_io"):
    """lcpcd_coset_fft (include/lcpc_hip_domain.h): the transform of the (n, L) elements x on the coset shift * H_n -- forward
    X[k] = p(shift w^k), inverse back to the coefficients; forms as lcpc_amd.fft.  A host call: no device."""
    L = FIELD_LIMBS[field]
    a = _elems(x, L).reshape(-1, L)
    out = np.zeros_like(a)
    rc = _lib.lib().lcpcd_coset_fft(field, _form(form), _ptr(_shift(shift, L)), _ptr(a), _ptr(out), _log_n(a.shape[0]))
    if rc:
        raise LcpcError(rc)
    return out


def extend(field, coeffs, shift, log_m, order="natural"):
    """lcpcd_extend (include/lcpc_hip_domain.h): the values of the polynomial with the (n_coeffs, L) coefficients on the 2^log_m
    points shift * w_m^k; order="natural" stores value k at [k], "bitrev" at [rev(k)].  A host call: no device."""
    L = FIELD_LIMBS[field]
    a = _elems(coeffs, L).reshape(-1, L)
    out = np.zeros((1 << log_m if log_m < 48 else 0, L), np.uint64)
    rc = _lib.lib().lcpcd_extend(field, _ptr(_shift(shift, L)), _ptr(a), a.shape[0], log_m, _order(order), _ptr(out))
    if rc:
        raise LcpcError(rc)
    return out


def _op(op):
    if op not in _lib.QUOT_OPS:
        raise ValueError("op must be one of %s, not %r" % (sorted(_lib.QUOT_OPS), op))
    return _lib.QUOT_OPS[op]


def batch_inverse(field, x):
    """lcpcq_batch_inverse (include/lcpc_hip_quot.h): the inverses of the (n, L) elements x, zero for a zero.  A host call: no
    device."""
    L = FIELD_LIMBS[field]
    a = _elems(x, L).reshape(-1, L)
    out = np.zeros_like(a)
    rc = _lib.lib().lcpcq_batch_inverse(field, _ptr(a), _ptr(out), a.shape[0])
    if rc:
        raise LcpcError(rc)
    return out


def pointwise(field, op, a, b):
    """lcpcq_pointwise: a[i] op b[i] over two (n, L) element arrays, op "add" / "sub" / "mul" / "div" (a[i] / b[i], zero where b[i]
    is zero).  A host call: no device."""
    L = FIELD_LIMBS[field]
    x, y = _elems(a, L).reshape(-1, L), _elems(b, L).reshape(-1, L)
    if x.shape != y.shape:
        raise ValueError("a and b hold the same number of elements")
    out = np.zeros_like(x)
    rc = _lib.lib().lcpcq_pointwise(field, _op(op), _ptr(x), _ptr(y), _ptr(out), x.shape[0])
    if rc:
        raise LcpcError(rc)
    return out


def divide_linear(field, vals, shift, z, y, order="natural"):
    """lcpcq_divide_linear: (vals[k] - y) / (shift w_m^k - z) over the (m, L) values of a column on shift * H_m (shift=None: on H_m);
    z and y are one element each.  order as lcpc_amd.extend.  A host call: no device."""
    L = FIELD_LIMBS[field]
    a = _elems(vals, L).reshape(-1, L)
    out = np.zeros_like(a)
    s = None if shift is None else _ptr(_shift(shift, L))
    rc = _lib.lib().lcpcq_divide_linear(field, s, _order(order), _ptr(a), _log_n(a.shape[0]), _ptr(_shift(z, L)), _ptr(_shift(y, L)), _ptr(out))
    if rc:
        raise LcpcError(rc)
    return out


def divide_vanishing(field, vals, shift, log_n, order="natural"):
    """lcpcq_divide_vanishing: vals[k] / ((shift w_m^k)^n - 1), n = 2^log_n, over the (m, L) values of a column on shift * H_m, a
    coset off the subgroup.  A host call: no device."""
    L = FIELD_LIMBS[field]
    a = _elems(vals, L).reshape(-1, L)
    out = np.zeros_like(a)
    rc = _lib.lib().lcpcq_divide_vanishing(field, _ptr(_shift(shift, L)), _order(order), _ptr(a), _log_n(a.shape[0]), log_n, _ptr(out))
    if rc:
        raise LcpcError(rc)
    return out

def _scan_op(op):
    if op not in _lib.SCAN_OPS:
        raise ValueError("op must be one of %s, not %r" % (sorted(_lib.SCAN_OPS), op))
    return _lib.SCAN_OPS[op]


def scan(field, x, op, exclusive=False, init=None):
    """lcpcs_scan (include/lcpc_hip_scan.h): the prefix sums (op "sum") or products ("product") of the (n, L) elements x, starting
    from init (one element; None: the identity) -- out[k] takes in x[0..k], or x[0..k-1] with exclusive=True.  Returns (out, total),
    total the one element init (+) all of x.  A host call: no device."""
    L = FIELD_LIMBS[field]
    a = _elems(x, L).reshape(-1, L)
    out, total = np.zeros_like(a), np.zeros(L, np.uint64)
    c = None if init is None else _ptr(_shift(init, L))
    rc = _lib.lib().lcpcs_scan(field, _scan_op(op), int(bool(exclusive)), _ptr(a), _ptr(out), a.shape[0], c, _ptr(total))
    if rc:
        raise LcpcError(rc)
    return out, total


def scan_ratio(field, num, den, op, exclusive=False, init=None):
    """lcpcs_scan_ratio: lcpc_amd.scan of the terms num[k] / den[k], zero where den[k] is zero.  op "product" with exclusive=True is
    the accumulator of a permutation argument (total is one for a valid one), op "sum" a log-derivative sum.  A host call."""
    L = FIELD_LIMBS[field]
    x, y = _elems(num, L).reshape(-1, L), _elems(den, L).reshape(-1, L)
    if x.shape != y.shape:
        raise ValueError("num and den hold the same number of elements")
    out, total = np.zeros_like(x), np.zeros(L, np.uint64)
    c = None if init is None else _ptr(_shift(init, L))
    rc = _lib.lib().lcpcs_scan_ratio(field, _scan_op(op), int(bool(exclusive)), _ptr(x), _ptr(y), _ptr(out), x.shape[0], c, _ptr(total))
    if rc:
        raise LcpcError(rc)
    return out, total


def _sc_order(order):
    if order not in _lib.SUMCHECK_ORDERS:
        raise ValueError("order must be one of %s, not %r" % (sorted(_lib.SUMCHECK_ORDERS), order))
    return _lib.SUMCHECK_ORDERS[order]


def _sc_terms(terms, L):
    """a list of (coeff_or_None, [table indices]) -> (lcpcm_term array, n_terms, the coefficients as (n_terms, L) limbs or None when
    every one is None, the degree).  A coefficient left None beside given ones has no limbs to stand for it: give all or none"""
    terms = list(terms)
    if not 1 <= len(terms) <= _lib.SUMCHECK_MAX_TERMS:
        raise ValueError("a composition has 1 .. %d terms" % _lib.SUMCHECK_MAX_TERMS)
    arr = (_lib.LcpcmTerm * len(terms))()
    coeffs = []
    for m, (c, idx) in enumerate(terms):
        idx = list(idx)
        if not 1 <= len(idx) <= _lib.SUMCHECK_MAX_FACTORS:
            raise ValueError("a term has 1 .. %d factors" % _lib.SUMCHECK_MAX_FACTORS)
        arr[m].n_factors = len(idx)
        for k, t in enumerate(idx):
            arr[m].table[k] = t
        coeffs.append(c)
    given = [c is not None for c in coeffs]
    if any(given) and not all(given):
        raise ValueError("give a coefficient for every term or for none")
    cs = np.stack([_shift(c, L) for c in coeffs]) if all(given) else None
    return arr, len(terms), cs, max(t.n_factors for t in arr)


def sumcheck_bind(field, table, r, order="low"):
    """lcpcm_bind (include/lcpc_hip_sumcheck.h): binds one variable of the (n, L) table to r -- out[i] = lo + r (hi - lo) with
    (lo, hi) = (t[2i], t[2i+1]) (order "low") or (t[i], t[i + n/2]) ("high").  Returns the (n / 2, L) table.  A host call: no device."""
    L = FIELD_LIMBS[field]
    a = _elems(table, L).reshape(-1, L)
    out = np.zeros((a.shape[0] // 2, L), np.uint64)
    rc = _lib.lib().lcpcm_bind(field, _sc_order(order), _ptr(a), _ptr(out), a.shape[0], _ptr(_shift(r, L)))
    if rc:
        raise LcpcError(rc)
    return out


def sumcheck_round(field, tables, terms, order="low"):
    """lcpcm_round: the round polynomial of sum_i sum_m c_m prod_k tables[idx_mk] at t = 0 .. d, as (d + 1, L) limbs.  tables: a list of
    (n, L) tables of one length; terms: a list of (coeff_or_None, [table indices]).  A host call."""
    L = FIELD_LIMBS[field]
    tabs = [_elems(t, L).reshape(-1, L) for t in tables]
    if not tabs or any(t.shape != tabs[0].shape for t in tabs):
        raise ValueError("the tables hold one number of elements")
    arr, n_terms, cs, d = _sc_terms(terms, L)
    ptrs = (C.c_void_p * len(tabs))(*[t.ctypes.data for t in tabs])
    evals = np.zeros((d + 1, L), np.uint64)
    rc = _lib.lib().lcpcm_round(field, _sc_order(order), ptrs, len(tabs), arr, n_terms, None if cs is None else _ptr(cs), tabs[0].shape[0], _ptr(evals))
    if rc:
        raise LcpcError(rc)
    return evals


class Transcript:
    """merlin::Transcript (the `tr: &mut Transcript` of prove/verify)."""

    def __init__(self, label=b"", _h=None):
        self._h = _h if _h is not None else _lib.lib().lcpc_transcript_new(label, len(label))

    def append_message(self, label, message):
        _lib.lib().lcpc_transcript_append_message(self._h, label, len(label), bytes(message), len(message))

    def append_messages(self, label, messages, mlen):
        """append_message(label, m) for every mlen-byte slice m of `messages`."""
        messages = bytes(messages)
        _lib.lib().lcpc_transcript_append_messages(self._h, label, len(label), messages, mlen, len(messages) // mlen)

    def challenge_bytes(self, label, n):
        out = C.create_string_buffer(n)
        _lib.lib().lcpc_transcript_challenge_bytes(self._h, label, len(label), out, n)
        return out.raw

    def clone(self):
        return Transcript(_h=_lib.lib().lcpc_transcript_clone(self._h))

    def __del__(self):
        try:
            _lib.lib().lcpc_transcript_free(self._h)
        except Exception:
            pass


class _Encoding:
    """common part of the two LcEncoding implementors; owns one lcpc_ctx (encoder tables on the GPU)."""

    def __init__(self, params):
        self.params = params
        h = C.c_void_p()
        rc = _lib.lib().lcpc_ctx_create(C.byref(params), C.byref(h))
        if rc:
            raise LcpcError(rc)
        self._h = h
        self.field = params.field
        self.digest = {v[0]: k for k, v in DIGEST_TABLE.items()}[params.hash]
        self.digest_len = DIGEST_TABLE[self.digest][1]
        self.L = FIELD_LIMBS[params.field]
        a, b, c = C.c_uint64(), C.c_uint64(), C.c_uint64()
        _lib.lib().lcpc_get_dims(self._h, 1, C.byref(a), C.byref(b), C.byref(c))
        self.n_per_row, self.n_cols = b.value, c.value

    def _check(self, rc):
        if rc:
            raise LcpcError(rc, _lib.lib().lcpc_last_error(self._h).decode())

    # LcEncoding trait, lcpc-2d/src/lib.rs:74-104
    def get_dims(self, length):
        a, b, c = C.c_uint64(), C.c_uint64(), C.c_uint64()
        self._check(_lib.lib().lcpc_get_dims(self._h, length, C.byref(a), C.byref(b), C.byref(c)))
        return a.value, b.value, c.value

    def dims_ok(self, n_per_row, n_cols):
        return bool(_lib.lib().lcpc_dims_ok(self._h, n_per_row, n_cols))

    def get_n_col_opens(self):
        return _lib.lib().lcpc_get_n_col_opens(self._h)

    def get_n_degree_tests(self):
        return _lib.lib().lcpc_get_n_degree_tests(self._h)

    def encode(self, rows):
        """in place on a copy: rows of n_cols elements, message in the first n_per_row, rest zero."""
        rows = _elems(rows, self.L).copy()
        n = rows.size // (self.L * self.n_cols)
        if n * self.L * self.n_cols != rows.size:
            raise LcpcError(ERR_ENCODE, "row length != n_cols")
        self._check(_lib.lib().lcpc_encode_rows(self._h, _ptr(rows), n))
        return rows

    def random_coeffs_device(self, n, seed=0, stream_id=0, out_ptr=None, stream=0):
        """lcpc_test_fields::random_coeffs (lcpc-test-fields/src/lib.rs:75-97) with a fixed generator, on the device: n elements by
        Field::random from ChaCha20Rng::from_seed([seed; 32]), stream `stream_id` (lcpc_random_coeffs_device) -- element for
        element the vector the same rule gives on a host.  Returns a torch int64 tensor [n, L] on the encoder's device, or
        fills `out_ptr` (a device address with room for n * L u64) and returns None."""
        key = (C.c_uint8 * 32)(*([seed & 0xFF] * 32))
        t = None
        if out_ptr is None:
            import torch
            t = torch.empty((n, self.L), dtype=torch.int64, device=torch.device("cuda", self.params.device))
            out_ptr = t.data_ptr()
        self._check(_lib.lib().lcpc_random_coeffs_device(self._h, key, stream_id, n, C.c_void_p(out_ptr), C.c_void_p(stream)))
        return t

    # plain integers <-> field elements on the host (include/lcpc_hip_ints.h): tensors, points, evaluations
    def from_ints(self, values, kind=None):
        """the (n, L) Montgomery limbs of `values` mod p.  values: a numpy array of uint32 / int32 / uint64 / int64 (kind="wide": (n, L)
        uint64 limbs of unsigned 64 L-bit integers), or any sequence of Python ints of any size and sign -- those are reduced here and
        sent as "wide".  A negative v is p - (|v| mod p)."""
        if isinstance(values, np.ndarray) and values.dtype.kind in "iu":
            a = np.ascontiguousarray(values)
        else:
            p = FIELD_MODULUS[self.field]
            red = [int(v) % p for v in values]
            a = np.array([[(v >> (64 * i)) & 0xFFFFFFFFFFFFFFFF for i in range(self.L)] for v in red], np.uint64).reshape(len(red), self.L)
            kind = "wide"
        k, n = _int_kind(a.dtype, a.shape, self.L, kind)
        out = np.zeros((n, self.L), np.uint64)
        rc = _lib.lib().lcpci_from_ints(self.field, k, _ptr(a), n, _ptr(out))
        if rc:
            raise LcpcError(rc)
        return out

    def to_ints(self, elems):
        """the canonical values of (n, L) Montgomery limbs as a list of Python ints in [0, p)"""
        e = _elems(elems, self.L).reshape(-1, self.L)
        out = np.zeros_like(e)
        rc = _lib.lib().lcpci_to_canon(self.field, _ptr(e), e.shape[0], _ptr(out))
        if rc:
            raise LcpcError(rc)
        return [sum(int(w) << (64 * i) for i, w in enumerate(row)) for row in out]

    def tensors(self, point, n_rows, basis="powers"):
        """tensors(field, point, n_rows, n_per_row, basis) with the field and n_per_row of this encoder: what prove (outer) and
        verify (outer, inner) take for a commitment of n_rows rows under it"""
        return tensors(self.field, point, n_rows, self.n_per_row, basis)

    def fft(self, t, form="fft_io", out=None, stream=0):
        """lcpcf_fft_device (include/lcpc_hip_fft.h): the transform of a torch tensor of 64-bit limbs on the encoder's device, (n, L)
        or (n_vecs, n, L) with every vector transformed on its own; forms as lcpc_amd.fft.  out=None returns a new tensor, out=t runs
        in place, any other tensor of t's shape must not overlap it.  Only enqueues on `stream`."""
        import torch
        if not torch.is_tensor(t) or t.device != torch.device("cuda", self.params.device) or not t.is_contiguous() or t.element_size() != 8:
            raise ValueError("a tensor of elements must be contiguous 64-bit limbs on the encoder's device")
        if t.dim() not in (2, 3) or t.shape[-1] != self.L:
            raise ValueError("the transform takes (n, L) or (n_vecs, n, L) limbs")
        if out is None:
            out = torch.empty_like(t)
        elif not torch.is_tensor(out) or out.shape != t.shape or out.dtype != t.dtype or out.device != t.device or not out.is_contiguous():
            raise ValueError("out must be a contiguous tensor of the input's shape, dtype and device")
        n_vecs = t.shape[0] if t.dim() == 3 else 1
        self._check(_lib.lib().lcpcf_fft_device(self._h, _form(form), C.c_void_p(t.data_ptr()), C.c_void_p(out.data_ptr()),
                                                _log_n(t.shape[-2]), n_vecs, C.c_void_p(stream)))
        return out

    def _elem_tensor(self, t, what="the transform"):
        import torch
        if not torch.is_tensor(t) or t.device != torch.device("cuda", self.params.device) or not t.is_contiguous() or t.element_size() != 8:
            raise ValueError("a tensor of elements must be contiguous 64-bit limbs on the encoder's device")
        if t.dim() not in (2, 3) or t.shape[-1] != self.L:
            raise ValueError("%s takes (n, L) or (n_vecs, n, L) limbs" % what)
        return t.shape[0] if t.dim() == 3 else 1

    def _out_tensor(self, t, out, shape):
        import torch
        if out is None:
            return torch.empty(shape, dtype=t.dtype, device=t.device)
        if not torch.is_tensor(out) or tuple(out.shape) != tuple(shape) or out.dtype != t.dtype or out.device != t.device or not out.is_contiguous():
            raise ValueError("out must be a contiguous tensor of shape %s with the input's dtype and device" % (tuple(shape),))
        return out

    def coset_fft(self, t, shift, form="fft_io", out=None, stream=0):
        """lcpcd_coset_fft_device (include/lcpc_hip_domain.h): enc.fft on the coset shift * H_n; shift is one element of host limbs
        (lcpc_amd.generator).  out=None returns a new tensor, out=t runs in place.  Only enqueues on `stream`."""
        n_vecs = self._elem_tensor(t)
        out = self._out_tensor(t, out, t.shape)
        self._check(_lib.lib().lcpcd_coset_fft_device(self._h, _form(form), _ptr(_shift(shift, self.L)), C.c_void_p(t.data_ptr()),
                                                      C.c_void_p(out.data_ptr()), _log_n(t.shape[-2]), n_vecs, C.c_void_p(stream)))
        return out

    def extend(self, coeffs, shift, log_m, order="natural", n_coeffs=None, out=None, stream=0):
        """lcpcd_extend_device: the values on the 2^log_m points shift * w_m^k of the polynomials whose coefficients are the vectors
        of `coeffs`, (n, L) or (n_vecs, n, L) with n a power of two; n_coeffs <= n says how many of each vector are read (the rest
        counts as zero; n must then be the next power of two).  Returns (2^log_m, L) or (n_vecs, 2^log_m, L).  Only enqueues."""
        n_vecs = self._elem_tensor(coeffs, "the extension")
        n = coeffs.shape[-2]
        _log_n(n)
        if n_coeffs is None:
            n_coeffs = n
        if not 0 < n_coeffs <= n or 2 * n_coeffs <= n > 1:
            raise ValueError("the coefficient vectors lie 2^ceil(log2 n_coeffs) elements apart")
        out = self._out_tensor(coeffs, out, tuple(coeffs.shape[:-2]) + (1 << log_m if log_m < 40 else 0, self.L))
        self._check(_lib.lib().lcpcd_extend_device(self._h, _ptr(_shift(shift, self.L)), C.c_void_p(coeffs.data_ptr()), n_coeffs, log_m,
                                                   _order(order), C.c_void_p(out.data_ptr()), n_vecs, C.c_void_p(stream)))
        return out

    def lde(self, t, log_m, shift_out, shift_in=None, in_order="natural", out_order="natural", work=None, out=None, stream=0):
        """lcpcd_lde_device: values on shift_in * H_n (shift_in=None: on H_n) -> values on shift_out * H_m, m = 2^log_m >= n, for (n, L)
        or (n_vecs, n, L) columns.  Returns (out, work): work, of t's shape, holds the coefficients; work=t overwrites the input.
        Only enqueues on `stream`."""
        n_vecs = self._elem_tensor(t, "the low-degree extension")
        work = self._out_tensor(t, work, t.shape)
        out = self._out_tensor(t, out, tuple(t.shape[:-2]) + (1 << log_m if log_m < 40 else 0, self.L))
        si = None if shift_in is None else _ptr(_shift(shift_in, self.L))
        self._check(_lib.lib().lcpcd_lde_device(self._h, _order(in_order), si, C.c_void_p(t.data_ptr()), _log_n(t.shape[-2]),
                                                _ptr(_shift(shift_out, self.L)), log_m, _order(out_order), C.c_void_p(out.data_ptr()),
                                                C.c_void_p(work.data_ptr()), n_vecs, C.c_void_p(stream)))
        return out, work

    def batch_inverse(self, t, out=None, stream=0):
        """lcpcq_batch_inverse_device (include/lcpc_hip_quot.h): the inverse of every element of an (n, L) or (n_vecs, n, L) tensor on
        the encoder's device, zero for a zero.  out=None returns a new tensor, out=t runs in place.  Only enqueues on `stream`."""
        n_vecs = self._elem_tensor(t, "the inversion")
        out = self._out_tensor(t, out, t.shape)
        self._check(_lib.lib().lcpcq_batch_inverse_device(self._h, C.c_void_p(t.data_ptr()), C.c_void_p(out.data_ptr()),
                                                          n_vecs * t.shape[-2], C.c_void_p(stream)))
        return out

    def pointwise(self, op, a, b, out=None, stream=0):
        """lcpcq_pointwise_device: a[i] op b[i] over two tensors of one shape, op "add" / "sub" / "mul" / "div" (zero where b[i] is
        zero).  out may be a or b.  Only enqueues on `stream`."""
        n_vecs = self._elem_tensor(a, "a pointwise operation")
        if self._elem_tensor(b, "a pointwise operation") != n_vecs or a.shape != b.shape:
            raise ValueError("a and b are tensors of one shape")
        out = self._out_tensor(a, out, a.shape)
        self._check(_lib.lib().lcpcq_pointwise_device(self._h, _op(op), C.c_void_p(a.data_ptr()), C.c_void_p(b.data_ptr()),
                                                      C.c_void_p(out.data_ptr()), n_vecs * a.shape[-2], C.c_void_p(stream)))
        return out

    def divide_linear(self, vals, shift, z, y, order="natural", out=None, stream=0):
        """lcpcq_divide_linear_device: (vals_v[k] - y_v) / (shift w_m^k - z) over (m, L) or (n_vecs, m, L) values on shift * H_m
        (shift=None: on H_m).  shift and z are host limbs; y is a tensor of n_vecs elements on the device, where LcCommit.eval leaves
        them.  Only enqueues on `stream`."""
        import torch
        n_vecs = self._elem_tensor(vals, "the division")
        if not torch.is_tensor(y) or y.device != vals.device or not y.is_contiguous() or y.element_size() != 8 or y.numel() != n_vecs * self.L:
            raise ValueError("y holds one element per vector, contiguous 64-bit limbs on the encoder's device")
        out = self._out_tensor(vals, out, vals.shape)
        s = None if shift is None else _ptr(_shift(shift, self.L))
        self._check(_lib.lib().lcpcq_divide_linear_device(self._h, s, _order(order), C.c_void_p(vals.data_ptr()), _log_n(vals.shape[-2]), n_vecs,
                                                          _ptr(_shift(z, self.L)), C.c_void_p(y.data_ptr()), C.c_void_p(out.data_ptr()),
                                                          C.c_void_p(stream)))
        return out

    def divide_vanishing(self, vals, shift, log_n, order="natural", out=None, stream=0):
        """lcpcq_divide_vanishing_device: vals_v[k] / ((shift w_m^k)^n - 1), n = 2^log_n, over (m, L) or (n_vecs, m, L) values on the
        coset shift * H_m.  Only enqueues on `stream`."""
        n_vecs = self._elem_tensor(vals, "the division")
        out = self._out_tensor(vals, out, vals.shape)
        self._check(_lib.lib().lcpcq_divide_vanishing_device(self._h, _ptr(_shift(shift, self.L)), _order(order), C.c_void_p(vals.data_ptr()),
                                                             _log_n(vals.shape[-2]), log_n, n_vecs, C.c_void_p(out.data_ptr()), C.c_void_p(stream)))
        return out

    def _scan_ends(self, t, n_vecs, op, init, total, stream):
        """what enc.scan and enc.scan_ratio share: the op, init and total as tensors of n_vecs elements, and the work buffer"""
        import torch
        for name, e in (("init", init), ("total", total)):
            if e is not None and (not torch.is_tensor(e) or e.device != t.device or not e.is_contiguous() or e.dtype != t.dtype or
                                  e.numel() != n_vecs * self.L):
                raise ValueError("%s holds one element per vector, contiguous limbs of the input's dtype on the encoder's device" % name)
        need = _lib.lib().lcpcs_scan_work_bytes(self._h, t.shape[-2], n_vecs)
        work = torch.empty(max(need, 16) // 8, dtype=torch.int64, device=t.device)
        if stream:                                   # freed on return, while the scan may still run on a stream torch does not know
            work.record_stream(torch.cuda.ExternalStream(stream, device=t.device))
        return _scan_op(op), None if init is None else C.c_void_p(init.data_ptr()), None if total is None else C.c_void_p(total.data_ptr()), work, need

    def scan(self, x, op, exclusive=False, init=None, out=None, total=None, stream=None):
        """lcpcs_scan_device (include/lcpc_hip_scan.h): the prefix sums (op "sum") or products ("product") of every vector of an (n, L)
        or (n_vecs, n, L) tensor, each starting from its element of init (None: the identity); exclusive=True leaves init itself at
        [0].  total, a tensor of n_vecs elements, receives init (+) the whole vector, and may be the init of the next call.  out=None
        returns a new tensor, out=x runs in place.  The work buffer is a torch allocation.  Returns out, or (out, total) when total is
        given.  Only enqueues on `stream`."""
        stream = stream or 0
        n_vecs = self._elem_tensor(x, "the scan")
        out = self._out_tensor(x, out, x.shape)
        o, c, tot, work, need = self._scan_ends(x, n_vecs, op, init, total, stream)
        self._check(_lib.lib().lcpcs_scan_device(self._h, o, int(bool(exclusive)), C.c_void_p(x.data_ptr()), C.c_void_p(out.data_ptr()), x.shape[-2],
                                                 n_vecs, c, tot, C.c_void_p(work.data_ptr()), need, C.c_void_p(stream)))
        return out if total is None else (out, total)

    def scan_ratio(self, num, den, op, exclusive=False, init=None, out=None, total=None, stream=None):
        """lcpcs_scan_ratio_device: enc.scan of the terms num[k] / den[k] (zero where den[k] is zero) of two tensors of one shape; out
        may be num or den.  op "product" with exclusive=True is the accumulator of a permutation argument, whose total is one."""
        stream = stream or 0
        n_vecs = self._elem_tensor(num, "the scan")
        if self._elem_tensor(den, "the scan") != n_vecs or num.shape != den.shape:
            raise ValueError("num and den are tensors of one shape")
        out = self._out_tensor(num, out, num.shape)
        o, c, tot, work, need = self._scan_ends(num, n_vecs, op, init, total, stream)
        self._check(_lib.lib().lcpcs_scan_ratio_device(self._h, o, int(bool(exclusive)), C.c_void_p(num.data_ptr()), C.c_void_p(den.data_ptr()),
                                                       C.c_void_p(out.data_ptr()), num.shape[-2], n_vecs, c, tot, C.c_void_p(work.data_ptr()),
                                                       need, C.c_void_p(stream)))
        return out if total is None else (out, total)

    def _sc_tables(self, tables, what):
        """the tables of a sumcheck call: a list of (n, L) tensors of one length -> (pointer array, n)"""
        tables = list(tables)
        if not tables:
            raise ValueError("%s takes at least one table" % what)
        for t in tables:
            if self._elem_tensor(t, what) != 1 or t.dim() != 2 or t.shape != tables[0].shape or t.dtype != tables[0].dtype:
                raise ValueError("%s takes (n, L) tables of one length and dtype" % what)
        return (C.c_void_p * len(tables))(*[t.data_ptr() for t in tables]), tables[0].shape[0]

    def _sc_out(self, tables, out):
        """out=None: new tensors of half the length; otherwise a list of as many tensors; out[j] is tables[j] binds in place -- the
        result is then the first half of that tensor, which is what is returned for it"""
        import torch
        h = tables[0].shape[0] // 2
        if out is None:
            outs = [torch.empty((h, self.L), dtype=t.dtype, device=t.device) for t in tables]
            return outs, outs
        out = list(out)
        if len(out) != len(tables):
            raise ValueError("out holds one tensor per table")
        ret = []
        for o, t in zip(out, tables):
            if o is t:
                ret.append(t[:h])
                continue
            if not torch.is_tensor(o) or tuple(o.shape) != (h, self.L) or o.dtype != t.dtype or o.device != t.device or not o.is_contiguous():
                raise ValueError("an output is the table itself or a contiguous (n / 2, L) tensor of its dtype and device")
            ret.append(o)
        return out, ret

    def _sc_work(self, n, n_terms, like, stream):
        import torch
        need = _lib.lib().lcpcm_round_work_bytes(self._h, n, n_terms)
        work = torch.empty(max(need, 16) // 8, dtype=torch.int64, device=like.device)
        if stream:                                   # freed on return, while the round may still run on a stream torch does not know
            work.record_stream(torch.cuda.ExternalStream(stream, device=like.device))
        return work, need

    def sumcheck_bind(self, tables, r, order="low", out=None, stream=None):
        """lcpcm_bind_device (include/lcpc_hip_sumcheck.h): binds one variable of every (n, L) tensor of the list `tables` to r (one
        element of host limbs) in one launch.  out=None returns new (n / 2, L) tensors, out=tables binds in place (order "high" only)
        and returns views of the first halves.  Only enqueues on `stream`."""
        stream = stream or 0
        tables = list(tables)
        ins, n = self._sc_tables(tables, "the bind")
        outs, ret = self._sc_out(tables, out)
        op = (C.c_void_p * len(outs))(*[o.data_ptr() for o in outs])
        self._check(_lib.lib().lcpcm_bind_device(self._h, _sc_order(order), ins, op, len(tables), n, _ptr(_shift(r, self.L)), C.c_void_p(stream)))
        return ret

    def sumcheck_round(self, tables, terms, order="low", evals=None, stream=None):
        """lcpcm_round_device: the round polynomial of the composition `terms` (a list of (coeff_or_None, [table indices])) over the
        tensors `tables` at t = 0 .. d, as a (d + 1, L) tensor (evals=None: a new one).  The work buffer is a torch allocation.  Only
        enqueues on `stream`."""
        stream = stream or 0
        tables = list(tables)
        ins, n = self._sc_tables(tables, "the round")
        arr, n_terms, cs, d = _sc_terms(terms, self.L)
        evals = self._out_tensor(tables[0], evals, (d + 1, self.L))
        work, need = self._sc_work(n, n_terms, tables[0], stream)
        self._check(_lib.lib().lcpcm_round_device(self._h, _sc_order(order), ins, len(tables), arr, n_terms, None if cs is None else _ptr(cs), n,
                                                  C.c_void_p(evals.data_ptr()), C.c_void_p(work.data_ptr()), need, C.c_void_p(stream)))
        return evals

    def sumcheck_bind_round(self, tables, terms, r, order="low", out=None, evals=None, stream=None):
        """lcpcm_bind_round_device: enc.sumcheck_bind by r followed by enc.sumcheck_round on the bound tables, in one pass over the
        tables (n >= 4).  Returns (bound tables, evals), byte for byte those of the two calls."""
        stream = stream or 0
        tables = list(tables)
        ins, n = self._sc_tables(tables, "the bind")
        outs, ret = self._sc_out(tables, out)
        op = (C.c_void_p * len(outs))(*[o.data_ptr() for o in outs])
        arr, n_terms, cs, d = _sc_terms(terms, self.L)
        evals = self._out_tensor(tables[0], evals, (d + 1, self.L))
        work, need = self._sc_work(n, n_terms, tables[0], stream)
        self._check(_lib.lib().lcpcm_bind_round_device(self._h, _sc_order(order), ins, op, len(tables), arr, n_terms, None if cs is None else _ptr(cs), n,
                                                       _ptr(_shift(r, self.L)), C.c_void_p(evals.data_ptr()), C.c_void_p(work.data_ptr()), need,
                                                       C.c_void_p(stream)))
        return ret, evals

    def __del__(self):
        try:
            _lib.lib().lcpc_ctx_destroy(self._h)     # commitments made with it keep the tables alive (refcount)
        except Exception:
            pass


def _digest_id(digest):
    if digest not in DIGEST_TABLE:
        raise ValueError("digest must be one of %s, not %r" % (sorted(DIGEST_TABLE), digest))
    return DIGEST_TABLE[digest][0]


def _params(field, encoding, device, **kw):
    p = LcpcParams()
    p.field, p.encoding, p.hash, p.device = field, encoding, _digest_id(kw.get("digest", "blake3")), device
    p.rho_num, p.rho_den = kw.get("rho", (1, 2))
    p.sdig_code, p.seed = kw.get("code", 3), kw.get("seed", 0)
    p.n_coeffs, p.n_per_row, p.n_cols = kw.get("n_coeffs", 0), kw.get("n_per_row", 0), kw.get("n_cols", 0)
    p.shard_rank, p.shard_count = kw.get("shard", (0, 1))
    return p


def static_get_dims(field, encoding, length, rho=(1, 2), code=3):
    """LigeroEncodingRho::_get_dims (ligero lib.rs:70-112) / SdigEncodingS::new's shape (brakedown lib.rs:69-110)."""
    p = _params(field, encoding, 0, n_coeffs=length, rho=rho, code=code)
    a, b, c = C.c_uint64(), C.c_uint64(), C.c_uint64()
    rc = _lib.lib().lcpc_static_get_dims(C.byref(p), C.byref(a), C.byref(b), C.byref(c))
    if rc:
        raise LcpcError(rc)
    return a.value, b.value, c.value


def static_get_dims_ml(field, encoding, n_vars, rho=(1, 2), code=3):
    """the dims new_ml(n_vars) picks (ligero lib.rs:128-135, brakedown lib.rs:114-123); LcpcError(ERR_DIMS) where the
    reference's assert!s fire."""
    p = _params(field, encoding, 0, n_coeffs=1, rho=rho, code=code)
    a, b, c = C.c_uint64(), C.c_uint64(), C.c_uint64()
    rc = _lib.lib().lcpc_static_get_dims_ml(C.byref(p), n_vars, C.byref(a), C.byref(b), C.byref(c))
    if rc:
        raise LcpcError(rc)
    return a.value, b.value, c.value


class LigeroEncoding(_Encoding):
    """LigeroEncodingRho<Ft, Rn, Rd> (lcpc-ligero-pc/src/lib.rs:31-186); default rate 1/2 (lib.rs:189)."""

    def __init__(self, field, length=None, rho=(1, 2), device=0, shard=(0, 1), _dims=None, digest="blake3"):
        kw = dict(rho=rho, shard=shard, digest=digest)
        if _dims is not None:
            kw.update(n_per_row=_dims[0], n_cols=_dims[1])
        else:
            kw.update(n_coeffs=length)
        super().__init__(_params(field, ENC_LIGERO, device, **kw))

    @classmethod
    def new(cls, field, length, rho=(1, 2), device=0, shard=(0, 1), digest="blake3"):
        return cls(field, length, rho, device, shard, digest=digest)

    @classmethod
    def new_ml(cls, field, n_vars, rho=(1, 2), device=0, digest="blake3"):
        """LigeroEncodingRho::new_ml (lib.rs:128-135)."""
        _, n_per_row, n_cols = static_get_dims_ml(field, ENC_LIGERO, n_vars, rho)
        return cls.new_from_dims(field, n_per_row, n_cols, rho, device, digest=digest)

    @classmethod
    def new_from_dims(cls, field, n_per_row, n_cols, rho=(1, 2), device=0, shard=(0, 1), digest="blake3"):
        return cls(field, None, rho, device, shard, _dims=(n_per_row, n_cols), digest=digest)


class SdigEncoding(_Encoding):
    """SdigEncodingS<Ft, S> (lcpc-brakedown-pc/src/lib.rs:41-176); default code SdigCode3 (lib.rs:19)."""

    def __init__(self, field, length=None, seed=0, code=3, device=0, shard=(0, 1), _dims=None, digest="blake3"):
        kw = dict(seed=seed, code=code, shard=shard, digest=digest)
        if _dims is not None:
            kw.update(n_per_row=_dims[0], n_cols=_dims[1])
        else:
            kw.update(n_coeffs=length)
        super().__init__(_params(field, ENC_SDIG, device, **kw))

    @classmethod
    def new(cls, field, length, seed, code=3, device=0, digest="blake3"):
        return cls(field, length, seed, code, device, digest=digest)

    @classmethod
    def new_ml(cls, field, n_vars, seed, code=3, device=0, digest="blake3"):
        """SdigEncodingS::new_ml (lib.rs:114-123)."""
        _, n_per_row, n_cols = static_get_dims_ml(field, ENC_SDIG, n_vars, code=code)
        return cls.new_from_dims(field, n_per_row, n_cols, seed, code, device, digest=digest)

    @classmethod
    def new_from_dims(cls, field, n_per_row, n_cols, seed, code=3, device=0, digest="blake3"):
        return cls(field, None, seed, code, device, _dims=(n_per_row, n_cols), digest=digest)


BORROW_COEFFS = 1      # LCPC_COMMIT_BORROW_COEFFS
ASYNC_TAIL = 2         # LCPC_COMMIT_ASYNC_TAIL (lcpc_commit_sharded_device)


class LcCommit:
    """LcCommit<D, E> (lcpc-2d/src/lib.rs:172-184, 270-312) with D = the encoder's digest (BLAKE3, SHA3-256, BLAKE2b, Keccak-256 or SHA-256): one lcpc_commit_t -- comm / coeffs / hashes
    of ONE commitment, resident in HBM.  Any number of them may be live under one encoding object (lib.rs:299-311)."""

    def __init__(self, enc):
        """an empty commitment bound to `enc` (lcpc_commit_create); the commit constructors below fill it."""
        self.enc = enc
        h = C.c_void_p()
        rc = _lib.lib().lcpc_commit_create(enc._h, C.byref(h))
        if rc:
            raise LcpcError(rc)
        self._h = h
        self.n_rows = self.n_per_row = self.n_cols = self.n_hashes = 0

    def _check(self, rc):
        if rc:
            raise LcpcError(rc, _lib.lib().lcpc_commit_last_error(self._h).decode())

    def _refresh(self):
        a, b, c, d = (C.c_uint64() for _ in range(4))
        self._check(_lib.lib().lcpc_commit_dims(self._h, C.byref(a), C.byref(b), C.byref(c), C.byref(d)))
        self.n_rows, self.n_per_row, self.n_cols, self.n_hashes = a.value, b.value, c.value, d.value
        return self

    @classmethod
    def commit(cls, coeffs, enc, into=None):
        """LcCommit::commit(&coeffs, &enc) (lib.rs:299-301) from host memory.  `into`: refill that object (buffers reused)."""
        coeffs = _elems(coeffs, enc.L)
        cm = into if into is not None else cls(enc)
        cm._check(_lib.lib().lcpc_commit(cm._h, _ptr(coeffs), coeffs.size // enc.L, None))
        return cm._refresh()

    @classmethod
    def commit_device(cls, coeffs_ptr, n_coeffs, enc, stream=0, sync=True, borrow=False, into=None):
        """same, coefficients already in HBM (`coeffs_ptr` = device address, e.g. torch tensor .data_ptr()).
        borrow: LCPC_COMMIT_BORROW_COEFFS -- the commitment keeps reading the caller's buffer instead of copying it."""
        cm = into if into is not None else cls(enc)
        root = (C.c_uint8 * enc.digest_len)() if sync else None
        cm._check(_lib.lib().lcpc_commit_device(cm._h, C.c_void_p(coeffs_ptr), n_coeffs, C.c_void_p(stream),
                                                BORROW_COEFFS if borrow else 0, root))
        return cm._refresh()

    @classmethod
    def commit_ints(cls, values, enc, kind=None, into=None, stream=0, sync=True):
        """commit to plain integers (include/lcpc_hip_ints.h): element i of the polynomial is values[i] mod p; the integers cross the
        bus as they are and are widened on the device.  A numpy array (uint32 / int32 / uint64 / int64, or (n, L) uint64 with
        kind="wide") takes the host call, which is complete on return.  A torch tensor on the encoder's device takes the device call
        (kind="u64" reads int64 storage as unsigned); sync=False only enqueues on `stream`, and the object keeps the tensor alive
        until its next fill."""
        cm = into if into is not None else cls(enc)
        if isinstance(values, np.ndarray):
            a = np.ascontiguousarray(values)
            k, n = _int_kind(a.dtype, a.shape, enc.L, kind)
            cm._check(_lib.lib().lcpci_commit_ints(cm._h, k, _ptr(a), n, None))
            cm._coeffs_ref = None
            return cm._refresh()
        import torch
        if not torch.is_tensor(values):
            raise TypeError("values must be a numpy array or a torch tensor")
        if values.device != torch.device("cuda", enc.params.device) or not values.is_contiguous():
            raise ValueError("a tensor of integers must be contiguous and on the encoder's device")
        k, n = _int_kind(values.dtype, tuple(values.shape), enc.L, kind)
        root = (C.c_uint8 * enc.digest_len)() if sync else None
        cm._check(_lib.lib().lcpci_commit_ints_device(cm._h, k, C.c_void_p(values.data_ptr()), n, C.c_void_p(stream), root))
        cm._coeffs_ref = None if sync else values
        return cm._refresh()

    @classmethod
    def commit_evals(cls, evals, enc, order="natural", into=None, stream=0, sync=True):
        """commit to the polynomial of degree < n that takes the values `evals` -- (n, L) elements, n a power of two -- on the subgroup
        of order n (include/lcpc_hip_fft.h): order="natural" evals[i] = p(w^i), "bitrev" evals[rev(i)] = p(w^i), w the encoder's root
        of unity.  The object ends up as LcCommit.commit of the interpolated coefficients leaves it.  A numpy array takes the host
        call, which is complete on return.  A torch tensor on the encoder's device takes the device call and is only read;
        sync=False only enqueues on `stream`, and the object keeps the tensor alive until its next fill."""
        if order not in _lib.FFT_ORDERS:
            raise ValueError("order must be one of %s, not %r" % (sorted(_lib.FFT_ORDERS), order))
        cm = into if into is not None else cls(enc)
        if isinstance(evals, np.ndarray):
            a = _elems(evals, enc.L).reshape(-1, enc.L)
            cm._check(_lib.lib().lcpcf_commit_evals(cm._h, _lib.FFT_ORDERS[order], _ptr(a), _log_n(a.shape[0]), None))
            cm._coeffs_ref = None
            return cm._refresh()
        import torch
        if not torch.is_tensor(evals):
            raise TypeError("evals must be a numpy array or a torch tensor")
        if evals.device != torch.device("cuda", enc.params.device) or not evals.is_contiguous() or evals.element_size() != 8:
            raise ValueError("a tensor of elements must be contiguous 64-bit limbs on the encoder's device")
        if evals.numel() % enc.L:
            raise ValueError("element array size is not a multiple of L")
        root = (C.c_uint8 * enc.digest_len)() if sync else None
        cm._check(_lib.lib().lcpcf_commit_evals_device(cm._h, _lib.FFT_ORDERS[order], C.c_void_p(evals.data_ptr()),
                                                       _log_n(evals.numel() // enc.L), C.c_void_p(stream), root))
        cm._coeffs_ref = None if sync else evals
        return cm._refresh()

    @classmethod
    def commit_coset_evals(cls, evals, shift, enc, order="natural", into=None, stream=0, sync=True):
        """commit_evals for values on the coset shift * H_n (include/lcpc_hip_domain.h): order="natural" evals[i] = p(shift w^i),
        "bitrev" evals[rev(i)] = p(shift w^i); shift is one element of host limbs (lcpc_amd.generator).  numpy takes the host call,
        a torch tensor on the encoder's device the device call, as commit_evals."""
        o, sh = _order(order), _shift(shift, enc.L)
        cm = into if into is not None else cls(enc)
        if isinstance(evals, np.ndarray):
            a = _elems(evals, enc.L).reshape(-1, enc.L)
            cm._check(_lib.lib().lcpcd_commit_coset_evals(cm._h, o, _ptr(sh), _ptr(a), _log_n(a.shape[0]), None))
            cm._coeffs_ref = None
            return cm._refresh()
        import torch
        if not torch.is_tensor(evals):
            raise TypeError("evals must be a numpy array or a torch tensor")
        if evals.device != torch.device("cuda", enc.params.device) or not evals.is_contiguous() or evals.element_size() != 8:
            raise ValueError("a tensor of elements must be contiguous 64-bit limbs on the encoder's device")
        if evals.numel() % enc.L:
            raise ValueError("element array size is not a multiple of L")
        root = (C.c_uint8 * enc.digest_len)() if sync else None
        cm._check(_lib.lib().lcpcd_commit_coset_evals_device(cm._h, o, _ptr(sh), C.c_void_p(evals.data_ptr()),
                                                             _log_n(evals.numel() // enc.L), C.c_void_p(stream), root))
        cm._coeffs_ref = None if sync else evals
        return cm._refresh()

    def values(self, shift, log_m, order="natural", out=None, stream=0):
        """lcpcd_commit_values_device: the values of the committed polynomial sum_i coeffs[i] X^i on the 2^log_m points shift * w_m^k
        as a (2^log_m, L) torch tensor on the encoder's device (out: written there).  2^log_m must be at least n_rows * n_per_row.
        A reader of the object; only enqueues on `stream`."""
        import torch
        shape = (1 << log_m if log_m < 40 else 0, self.enc.L)
        if out is None:
            out = torch.empty(shape, dtype=torch.int64, device=torch.device("cuda", self.enc.params.device))
        elif not torch.is_tensor(out) or tuple(out.shape) != shape or out.element_size() != 8 or not out.is_contiguous() or \
                out.device != torch.device("cuda", self.enc.params.device):
            raise ValueError("out must be a contiguous (2^log_m, L) tensor of 64-bit limbs on the encoder's device")
        self._check(_lib.lib().lcpcd_commit_values_device(self._h, _ptr(_shift(shift, self.enc.L)), log_m, _order(order),
                                                          C.c_void_p(out.data_ptr()), C.c_void_p(stream)))
        return out

    @classmethod
    def from_parts(cls, enc, comm, coeffs, n_rows, into=None):
        """test hook = lcpc-2d/src/tests.rs:435-466 random_comm + merkleize."""
        comm = _elems(comm, enc.L)
        cp = _ptr(_elems(coeffs, enc.L)) if coeffs is not None else None
        cm = into if into is not None else cls(enc)
        cm._check(_lib.lib().lcpc_commit_from_parts(cm._h, _ptr(comm), cp, n_rows, None))
        return cm._refresh()

    # ---- serde of LcCommit (lcpc-2d/src/lib.rs:186-268), bincode 1.3, streamed ----
    def bincode_size(self):
        return int(_lib.lib().lcpc_commit_bincode_size(self._h))

    def to_bincode(self, fileobj):
        """bincode::serialize_into(fileobj, &commit): the bytes the reference's `Deserialize for LcCommit` takes."""
        err = []

        def wr(_user, data, n):
            try:
                fileobj.write(C.string_at(data, n))
                return 0
            except Exception as e:      # never unwind through the C frame
                err.append(e)
                return 1

        rc = _lib.lib().lcpc_commit_bincode_write(self._h, _lib.WRITE_FN(wr), None)
        if err:
            raise err[0]
        self._check(rc)

    @classmethod
    def from_bincode(cls, enc, fileobj):
        """bincode::deserialize_from(fileobj) of a commitment the reference (or to_bincode) serialised, into HBM."""
        cm = cls(enc)
        err = []

        def rd(_user, data, n):
            try:
                b = fileobj.read(n)
                if len(b) != n:
                    return 1
                C.memmove(data, b, n)
                return 0
            except Exception as e:
                err.append(e)
                return 1

        rc = _lib.lib().lcpc_commit_from_bincode(cm._h, _lib.WRITE_FN(rd), None, None)
        if err:
            raise err[0]
        cm._check(rc)
        return cm._refresh()

    def get_root(self):
        out = (C.c_uint8 * self.enc.digest_len)()
        self._check(_lib.lib().lcpc_get_root(self._h, out))
        return bytes(out)

    def get_n_rows(self):
        return self.n_rows

    def get_n_cols(self):
        return self.n_cols

    def get_n_per_row(self):
        return self.n_per_row

    def hashes(self):
        out = np.zeros((self.n_hashes, self.enc.digest_len), np.uint8)
        self._check(_lib.lib().lcpc_get_hashes(self._h, _ptr(out)))
        return out

    def comm(self, row0=0, n_rows=None):
        n_rows = self.n_rows - row0 if n_rows is None else n_rows
        out = np.zeros((n_rows * self.n_cols, self.enc.L), np.uint64)
        self._check(_lib.lib().lcpc_get_comm(self._h, row0, n_rows, _ptr(out)))
        return out

    def coeffs(self, row0=0, n_rows=None):
        n_rows = self.n_rows - row0 if n_rows is None else n_rows
        out = np.zeros((n_rows * self.n_per_row, self.enc.L), np.uint64)
        self._check(_lib.lib().lcpc_get_coeffs(self._h, row0, n_rows, _ptr(out)))
        return out

    def eval_outer(self, tensors):
        """collapse_columns (lib.rs:1095-1123) for one (n_rows, L) or several (k, n_rows, L) tensors."""
        t = _elems(tensors, self.enc.L)
        k = t.size // (self.n_rows * self.enc.L) if self.n_rows else 0
        if k == 0 or k * self.n_rows * self.enc.L != t.size:
            raise LcpcError(ERR_OUTER_TENSOR)
        out = np.zeros((k, self.n_per_row, self.enc.L), np.uint64)
        self._check(_lib.lib().lcpc_collapse(self._h, _ptr(t), k, _ptr(out)))
        return out[0] if k == 1 and np.ndim(tensors) <= 2 else out

    # ---- evaluation (include/lcpc_hip_eval.h) ----
    def _on_device(self, t):
        import torch
        if not torch.is_tensor(t):
            return False
        if t.device != torch.device("cuda", self.enc.params.device) or not t.is_contiguous() or t.element_size() != 8:
            raise ValueError("a tensor of elements must be contiguous 64-bit limbs on the encoder's device")
        return True

    def eval(self, points, basis="powers"):
        """the committed polynomial at `points`: (n_points, L) elements.  basis="powers": points is (n_points, L) (or one (L,) element)
        and the value is sum_e coeffs[e] x^e; "ml_monomial" / "ml_lagrange": points is (n_points, n_vars, L), variable k = bit k of the
        coefficient index.  A numpy array takes the host call (lcpce_eval: complete on return, any number of threads); a torch tensor
        on the encoder's device takes lcpce_eval_device on torch's current stream and returns a tensor there, without a
        synchronisation.  The limbs are those LcEvalProof.verify returns for the tensors of the same point."""
        b, L = _basis(basis), self.enc.L
        n_point = _n_point(basis, self.n_rows, self.n_per_row)
        if self._on_device(points):
            import torch
            if points.numel() % (max(n_point, 1) * L):
                raise LcpcError(ERR_ARG)
            n_points = points.numel() // (n_point * L) if n_point else 1         # (no variables: the one empty point)
            out = torch.empty((n_points, L), dtype=torch.int64, device=points.device)
            st = torch.cuda.current_stream(points.device).cuda_stream
            self._check(_lib.lib().lcpce_eval_device(self._h, b, C.c_void_p(points.data_ptr()), n_point, n_points, C.c_void_p(st),
                                                     C.c_void_p(out.data_ptr())))
            return out
        p = _elems(points, L)
        if p.size % (max(n_point, 1) * L):
            raise LcpcError(ERR_ARG)
        n_points = p.size // (n_point * L) if n_point else 1
        out = np.zeros((n_points, L), np.uint64)
        self._check(_lib.lib().lcpce_eval(self._h, b, _ptr(p), n_point, n_points, _ptr(out)))
        return out

    def eval_tensors(self, outer, inner):
        """evaluation with the caller's own tensors: outer (k, n_rows, L) and inner (k, n_per_row, L) (or one pair without the
        leading axis) -> (k, L) elements, sum_e coeffs[e] outer[e / n_per_row] inner[e % n_per_row].  numpy arrays are uploaded and
        the result comes back as numpy; torch tensors on the encoder's device stay there (lcpce_eval_tensors_device on torch's
        current stream, no synchronisation)."""
        import torch
        L = self.enc.L
        dev = self._on_device(outer)
        if dev != self._on_device(inner):
            raise ValueError("outer and inner must both be numpy arrays or both device tensors")
        if not dev:
            device = torch.device("cuda", self.enc.params.device)
            outer = torch.from_numpy(_elems(outer, L).view(np.int64)).to(device)
            inner = torch.from_numpy(_elems(inner, L).view(np.int64)).to(device)
        k = outer.numel() // (self.n_rows * L) if self.n_rows else 0
        if k == 0 or k * self.n_rows * L != outer.numel() or k * self.n_per_row * L != inner.numel():
            raise LcpcError(ERR_ARG)
        out = torch.empty((k, L), dtype=torch.int64, device=outer.device)
        st = torch.cuda.current_stream(outer.device).cuda_stream
        self._check(_lib.lib().lcpce_eval_tensors_device(self._h, C.c_void_p(outer.data_ptr()), C.c_void_p(inner.data_ptr()), k,
                                                         C.c_void_p(st), C.c_void_p(out.data_ptr())))
        return out if dev else out.cpu().numpy().view(np.uint64)

    def open_columns(self, cols):
        cols = np.ascontiguousarray(cols, np.uint64)
        n = cols.size
        path_len = max(0, (self.n_cols - 1).bit_length())
        vals = np.zeros((n, self.n_rows, self.enc.L), np.uint64)
        paths = np.zeros((n, max(path_len, 1), self.enc.digest_len), np.uint8)
        self._check(_lib.lib().lcpc_open_columns(self._h, _ptr(cols), n, _ptr(vals), _ptr(paths)))
        return vals, paths[:, :path_len]

    def open_column(self, col):
        v, p = self.open_columns([col])
        return v[0], p[0]

    def prove(self, outer_tensor, enc, tr):
        """LcCommit::prove (lib.rs:304-311): returns an LcEvalProof (bincode bytes + parsed header)."""
        if enc is not self.enc:
            raise LcpcError(ERR_COMMIT)
        t = _elems(outer_tensor, enc.L)
        pp, plen = C.c_void_p(), C.c_uint64()
        cols = np.zeros(enc.get_n_col_opens(), np.uint64)
        self._check(_lib.lib().lcpc_prove(self._h, _ptr(t), t.size // enc.L, tr._h, C.byref(pp), C.byref(plen), _ptr(cols)))
        return LcEvalProof(_OwnedBuffer(pp, plen.value), enc.L, cols)

    def set_timing(self, on=True):
        self._check(_lib.lib().lcpc_set_timing(self._h, 1 if on else 0))

    def timings(self):
        t = LcpcTimings()
        self._check(_lib.lib().lcpc_get_timings(self._h, C.byref(t)))
        return t

    def __del__(self):
        try:
            _lib.lib().lcpc_commit_destroy(self._h)
        except Exception:
            pass


def commit_batch(enc, coeffs, n_coeffs=None, stream=0, sync=True, borrow=False, into=None, return_roots=False):
    """lcpcx_commit_batch_device (include/lcpc_hip_batch.h): every row of `coeffs` committed under `enc` in one pipeline.
    coeffs: a device tensor [n_batch, W] of 64-bit limbs (W = n_coeffs * L), or a list of equal-length device tensors, which is
    stacked.  n_coeffs: elements per polynomial when a row holds more than the polynomial (poly_stride = W / L; the rest of a row is
    never read).  borrow: LCPC_COMMIT_BORROW_COEFFS -- the members keep reading the tensor, which they keep alive.  into: the
    LcCommit objects to refill.  sync=False only enqueues on `stream`.  Ligero encoders run the batched pipeline under every digest
    (BLAKE3, SHA3-256, Keccak-256, SHA-256, BLAKE2b: roots of enc.digest_len bytes); Brakedown encoders run one expander encode over
    the stacked rows of all members, the batched hash and tree under BLAKE3 and the hash and tree member by member under the other
    four digests.  Returns the list of commitment objects (return_roots: and
    the list of roots the call itself reported; needs sync)."""
    import torch
    if isinstance(coeffs, (list, tuple)):
        coeffs = torch.stack([t.reshape(-1) for t in coeffs])
    if coeffs.dim() != 2 or coeffs.element_size() != 8 or not coeffs.is_contiguous() or coeffs.shape[1] % enc.L:
        raise ValueError("coeffs must be a contiguous [n_batch, n * L] tensor of 64-bit limbs")
    n_batch, stride = coeffs.shape[0], coeffs.shape[1] // enc.L
    n_coeffs = stride if n_coeffs is None else n_coeffs
    cms = list(into) if into is not None else [LcCommit(enc) for _ in range(n_batch)]
    if len(cms) != n_batch:
        raise ValueError("`into` must hold one LcCommit per polynomial")
    handles = (C.c_void_p * max(n_batch, 1))(*[cm._h for cm in cms])
    roots = (C.c_uint8 * (enc.digest_len * max(n_batch, 1)))() if sync else None
    rc = _lib.lib().lcpcx_commit_batch_device(handles, n_batch, C.c_void_p(coeffs.data_ptr()), n_coeffs, stride, C.c_void_p(stream),
                                              BORROW_COEFFS if borrow else 0, roots)
    if rc:
        raise LcpcError(rc, _lib.lib().lcpc_commit_last_error(cms[0]._h).decode() if cms else "")
    for cm in cms:
        # borrow: the members read the tensor for as long as they live.  sync=False: the encode that reads it is only enqueued, and
        # a stacked temporary has no other owner -- the members keep it until their next fill
        cm._coeffs_ref = coeffs if (borrow or not sync) else None
        cm._refresh()
    if return_roots:
        if not sync:
            raise ValueError("return_roots needs sync=True")
        return cms, [bytes(roots[i * enc.digest_len:(i + 1) * enc.digest_len]) for i in range(n_batch)]
    return cms


def prove_batch(cms, outer_tensor, trs, return_stats=False):
    """lcpcx_prove_batch (include/lcpc_hip_batch.h): LcCommit::prove for every member of `cms` in one lockstep pipeline -- the
    collapse and the open of all members in the launches of one prove, the members' transcript absorbs side by side on the host
    pool.  cms: committed LcCommit objects of ONE encoder with the same n_rows, of any origin; trs: one Transcript per member.
    outer_tensor: (n_rows, L) -- one tensor for all members -- or (n_batch, n_rows, L), one per member.  Returns the list of
    LcEvalProof, each byte for byte what cms[i].prove(outer_i, enc, trs[i]) returns (return_stats: and the call's
    LcpcxProveStats: groups, collapse_launches, open_launches, host_syncs)."""
    cms, trs = list(cms), list(trs)
    n_batch = len(cms)
    if n_batch == 0 or len(trs) != n_batch:
        raise LcpcError(ERR_ARG)
    enc = cms[0].enc
    t = np.ascontiguousarray(outer_tensor, dtype=np.uint64)
    if t.ndim == 3:
        if t.shape[0] != n_batch or t.shape[2] != enc.L:
            raise LcpcError(ERR_OUTER_TENSOR)
        n_outer = stride = t.shape[1]
    else:
        t = _elems(t, enc.L)
        n_outer, stride = t.size // enc.L, 0
    handles = (C.c_void_p * n_batch)(*[cm._h for cm in cms])
    th = (C.c_void_p * n_batch)(*[tr._h for tr in trs])
    pp, plen = (C.c_void_p * n_batch)(), (C.c_uint64 * n_batch)()
    n_open = enc.get_n_col_opens()
    cols = np.zeros((n_batch, n_open), np.uint64)
    stats = _lib.LcpcxProveStats()
    rc = _lib.lib().lcpcx_prove_batch(handles, n_batch, _ptr(t), n_outer, stride, th, pp, plen, _ptr(cols), C.byref(stats))
    if rc:
        raise LcpcError(rc, _lib.lib().lcpc_commit_last_error(cms[0]._h).decode())
    pfs = [LcEvalProof(_OwnedBuffer(C.c_void_p(pp[i]), plen[i]), enc.L, cols[i]) for i in range(n_batch)]
    return (pfs, stats) if return_stats else pfs


class _OwnedBuffer:
    """a malloc'ed buffer handed out by the library (lcpc_prove): viewed in place, released with lcpc_free"""

    def __init__(self, ptr, n):
        self.ptr, self.n = ptr, n
        self.view = (C.c_uint8 * n).from_address(ptr.value)

    def __del__(self):
        try:
            _lib.lib().lcpc_free(self.ptr)
        except Exception:
            pass


class LcEvalProof:
    """LcEvalProof<D, E> (lib.rs:490-500) held in the reference's bincode wire layout (lib.rs:550-609)."""

    def __init__(self, data, L, cols_opened=None):
        self._own = data if isinstance(data, _OwnedBuffer) else None
        self._bytes = None if self._own else bytes(data)
        self.L, self.cols_opened = L, cols_opened
        buf = self._own.view if self._own else self._bytes
        if len(buf) < 16:         # bincode::deserialize fails on a buffer that ends inside the header (io::UnexpectedEof)
            raise LcpcError(VERR_MALFORMED, "proof shorter than its header")
        hdr = np.frombuffer(buf, np.uint64, 2)
        self.n_cols, self._n_per_row = int(hdr[0]), int(hdr[1])

    @property
    def data(self):
        if self._bytes is None:
            self._bytes = bytes(self._own.view)
        return self._bytes

    def get_n_cols(self):
        return self.n_cols

    def get_n_per_row(self):
        return self._n_per_row

    def to_bytes(self):           # bincode::serialize(&pf)
        return self.data

    @classmethod
    def from_bytes(cls, data, L):  # bincode::deserialize
        return cls(data, L)

    def verify(self, root, outer_tensor, inner_tensor, enc, tr):
        """LcEvalProof::verify (lib.rs:518-527); returns the evaluation (L limbs) or raises LcpcError(VERR_*)."""
        o, i = _elems(outer_tensor, enc.L), _elems(inner_tensor, enc.L)
        out = np.zeros(enc.L, np.uint64)
        buf = np.frombuffer(self._own.view if self._own else self._bytes, np.uint8)
        # the library reads the encoder's digest length: a shorter root is zero-filled (it cannot match), a longer one cut
        rootb = np.zeros(enc.digest_len, np.uint8)
        rb = bytes(root)[:enc.digest_len]
        rootb[:len(rb)] = np.frombuffer(rb, np.uint8)
        rc = _lib.lib().lcpc_verify(enc._h, _ptr(rootb), _ptr(o), o.size // enc.L, _ptr(i), i.size // enc.L,
                                    _ptr(buf), buf.size, tr._h, _ptr(out))
        if rc:
            raise LcpcError(rc)
        return out


def verify_batch(enc, roots, outer_tensor, inner_tensor, proofs, trs, return_stats=False):
    """lcpcv_verify_batch (include/lcpc_hip_verify.h): LcEvalProof::verify for every proof of a batch in one lockstep pipeline -- one
    row encode, one column-hash launch chain and one column-check kernel for all members, their transcripts side by side on the host
    pool.  roots: one root per member; proofs: LcEvalProof objects or bytes; trs: one Transcript per member.  outer_tensor /
    inner_tensor: (n, L) -- one tensor for all members -- or (n_batch, n, L), one per member.  Returns (evals (n_batch, L) uint64,
    status (n_batch,) int32): status[i] is 0 or the VERR_* code proofs[i].verify(roots[i], outer_i, inner_i, enc, trs[i]) raises, and
    evals[i] its evaluation when status[i] == 0 (return_stats: and the call's LcpcvVerifyStats).  Raises LcpcError only when the call
    itself fails (arguments, device)."""
    roots, proofs, trs = list(roots), list(proofs), list(trs)
    n_batch = len(proofs)
    if n_batch == 0 or len(trs) != n_batch or len(roots) != n_batch:
        raise LcpcError(ERR_ARG)

    def tensor(t):
        t = np.ascontiguousarray(t, dtype=np.uint64)
        if t.ndim == 3:
            if t.shape[0] != n_batch or t.shape[2] != enc.L:
                raise LcpcError(ERR_ARG)
            return t, t.shape[1], t.shape[1]
        t = _elems(t, enc.L)
        return t, t.size // enc.L, 0

    o, n_outer, o_stride = tensor(outer_tensor)
    i, n_inner, i_stride = tensor(inner_tensor)
    # the library reads the encoder's digest length of every root: a shorter one is zero-filled (it cannot match), a longer one cut
    rootb = np.zeros((n_batch, enc.digest_len), np.uint8)
    for k, r in enumerate(roots):
        rb = bytes(r)[:enc.digest_len]
        rootb[k, :len(rb)] = np.frombuffer(rb, np.uint8)
    bufs = []
    for pf in proofs:
        if isinstance(pf, LcEvalProof):
            bufs.append(np.frombuffer(pf._own.view if pf._own else pf._bytes, np.uint8))
        else:
            bufs.append(np.frombuffer(pf, np.uint8))
    empty = np.zeros(8, np.uint8)             # (an empty proof is a member's VERR_MALFORMED, not a NULL argument)
    pp = (C.c_void_p * n_batch)(*[b.ctypes.data if b.size else empty.ctypes.data for b in bufs])
    plen = (C.c_uint64 * n_batch)(*[b.size for b in bufs])
    th = (C.c_void_p * n_batch)(*[tr._h for tr in trs])
    evals = np.zeros((n_batch, enc.L), np.uint64)
    status = np.zeros(n_batch, np.int32)
    stats = _lib.LcpcvVerifyStats()
    rc = _lib.lib().lcpcv_verify_batch(enc._h, n_batch, _ptr(rootb), _ptr(o), n_outer, o_stride, _ptr(i), n_inner, i_stride, pp, plen, th,
                                       _ptr(evals), _ptr(status), C.byref(stats))
    if rc:
        raise LcpcError(rc, _lib.lib().lcpc_last_error(enc._h).decode())
    return (evals, status, stats) if return_stats else (evals, status)


def check_columns(enc, root, cols, col_vals, paths, out=None):
    """lcpcp_check_columns (include/lcpc_hip_columns.h): verify_column_path for columns opened outside a proof -- what
    LcCommit.open_columns(cols) returns, checked against a root on the device.  cols: (n,) column numbers; col_vals: (n, n_rows, L)
    stored limbs; paths: (n, path_len, digest_len) bytes.  Returns an (n,) bool array: True where the column's leaf digest folds to
    root (out: an (n,) uint8 array the library writes instead, returned as it is).  Raises LcpcError when the call itself fails
    (ERR_COLUMN_NUMBER for a column number >= n_cols: nothing is judged)."""
    cols = np.ascontiguousarray(cols, np.uint64).reshape(-1)
    n = cols.size
    vals = np.ascontiguousarray(col_vals, np.uint64)
    pth = np.ascontiguousarray(paths, np.uint8)
    if vals.ndim != 3 or vals.shape[0] != n or vals.shape[2] != enc.L or pth.ndim != 3 or pth.shape[0] != n or pth.shape[2] != enc.digest_len:
        raise LcpcError(ERR_ARG)
    path_len = max(0, (enc.n_cols - 1).bit_length())
    if pth.shape[1] != path_len:
        raise LcpcError(ERR_ARG)
    rootb = np.zeros(enc.digest_len, np.uint8)
    rb = bytes(root)[:enc.digest_len]
    rootb[:len(rb)] = np.frombuffer(rb, np.uint8)
    ok = np.zeros(n, np.uint8) if out is None else out
    if ok.dtype != np.uint8 or ok.shape != (n,) or not ok.flags.c_contiguous:
        raise LcpcError(ERR_ARG)
    if n == 0:
        return ok.astype(bool) if out is None else ok
    if pth.size == 0:
        pth = np.zeros(1, np.uint8)           # (a tree of one leaf has no siblings; the library still wants a pointer)
    rc = _lib.lib().lcpcp_check_columns(enc._h, _ptr(rootb), _ptr(cols), n, vals.shape[1], _ptr(vals), _ptr(pth), _ptr(ok))
    if rc:
        raise LcpcError(rc, _lib.lib().lcpc_last_error(enc._h).decode())
    return ok.astype(bool) if out is None else ok


def root_bincode(root):
    """bincode of LcRoot (lib.rs:373-384): u64 len | the digest (40 bytes; 72 for a 64-byte BLAKE2b root)"""
    if len(root) == 64:
        return np.uint64(64).tobytes() + bytes(root)
    out = (C.c_uint8 * 40)()
    _lib.lib().lcpc_root_bincode(bytes(root), out)
    return bytes(out)

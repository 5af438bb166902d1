"""ctypes loader for lcpc_amd/lib/liblcpc_hip.so (the product: HIP kernels + C ABI of include/lcpc_hip.h).

There is deliberately NO fallback: if the shared library is missing or no HIP device is usable, every
entry point raises.  Nothing in this package touches the CPU restatement the tests check it against."""
import ctypes as C
import os
import subprocess

ABI_VERSION = 5
_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "lib", "liblcpc_hip.so")
CSRC = os.path.join(_HERE, "csrc")


class LcpcParams(C.Structure):
    _fields_ = [("field", C.c_uint32), ("encoding", C.c_uint32), ("hash", C.c_uint32),
                ("rho_num", C.c_uint32), ("rho_den", C.c_uint32), ("sdig_code", C.c_uint32),
                ("seed", C.c_uint64), ("n_coeffs", C.c_uint64), ("n_per_row", C.c_uint64), ("n_cols", C.c_uint64),
                ("device", C.c_int32), ("shard_rank", C.c_uint32), ("shard_count", C.c_uint32)]


class LcpcTimings(C.Structure):
    _fields_ = [("encode_ms", C.c_float), ("hash_ms", C.c_float), ("merkle_ms", C.c_float), ("total_ms", C.c_float),
                ("encode_launches", C.c_uint32), ("hash_launches", C.c_uint32), ("merkle_launches", C.c_uint32),
                ("exchange_exposed_ms", C.c_float), ("staged_slices", C.c_uint32), ("exchange_wire_ms", C.c_float)]


# every symbol include/lcpc_hip.h declares: name -> (restype, argtypes)
_vp, _u64, _u32, _i32, _sz = C.c_void_p, C.c_uint64, C.c_uint32, C.c_int, C.c_size_t
ALLGATHER_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_uint64)      # lcpc_allgather_fn (include/lcpc_hip.h)
WRITE_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, C.c_uint64)   # lcpc_write_fn / lcpc_read_fn

SYMBOLS = {
    "lcpc_abi_version": (_i32, []),
    "lcpc_ctx_create": (_i32, [C.POINTER(LcpcParams), C.POINTER(_vp)]),
    "lcpc_ctx_destroy": (None, [_vp]),
    "lcpc_strerror": (C.c_char_p, [_i32]),
    "lcpc_last_error": (C.c_char_p, [_vp]),
    "lcpc_get_dims": (_i32, [_vp, _u64, _vp, _vp, _vp]),
    "lcpc_dims_ok": (_i32, [_vp, _u64, _u64]),
    "lcpc_get_n_col_opens": (_u64, [_vp]),
    "lcpc_get_n_degree_tests": (_u64, [_vp]),
    "lcpc_field_limbs": (_u32, [_vp]),
    "lcpc_static_get_dims": (_i32, [C.POINTER(LcpcParams), _vp, _vp, _vp]),
    "lcpc_static_get_dims_ml": (_i32, [_vp, _u32, _vp, _vp, _vp]),
    "lcpc_random_coeffs_device": (_i32, [_vp, _vp, _u64, _u64, _vp, _vp]),
    "lcpc_encode_rows": (_i32, [_vp, _vp, _u64]),
    "lcpc_commit_create": (_i32, [_vp, C.POINTER(_vp)]),
    "lcpc_commit_destroy": (None, [_vp]),
    "lcpc_commit_last_error": (C.c_char_p, [_vp]),
    "lcpc_commit": (_i32, [_vp, _vp, _u64, _vp]),
    "lcpc_commit_device": (_i32, [_vp, _vp, _u64, _vp, _u32, _vp]),
    "lcpc_commit_from_parts": (_i32, [_vp, _vp, _vp, _u64, _vp]),
    "lcpc_commit_bincode_size": (_u64, [_vp]),
    "lcpc_commit_bincode_write": (_i32, [_vp, WRITE_FN, _vp]),
    "lcpc_commit_from_bincode": (_i32, [_vp, WRITE_FN, _vp, _vp]),
    "lcpc_get_root": (_i32, [_vp, _vp]),
    "lcpc_commit_dims": (_i32, [_vp, _vp, _vp, _vp, _vp]),
    "lcpc_get_hashes": (_i32, [_vp, _vp]),
    "lcpc_get_comm": (_i32, [_vp, _u64, _u64, _vp]),
    "lcpc_get_coeffs": (_i32, [_vp, _u64, _u64, _vp]),
    "lcpc_collapse": (_i32, [_vp, _vp, _u32, _vp]),
    "lcpc_open_columns": (_i32, [_vp, _vp, _u32, _vp, _vp]),
    "lcpc_transcript_new": (_vp, [C.c_char_p, _sz]),
    "lcpc_transcript_clone": (_vp, [_vp]),
    "lcpc_transcript_append_message": (None, [_vp, C.c_char_p, _sz, C.c_char_p, _sz]),
    "lcpc_transcript_append_messages": (None, [_vp, C.c_char_p, _sz, C.c_char_p, _sz, _sz]),
    "lcpc_transcript_challenge_bytes": (None, [_vp, C.c_char_p, _sz, _vp, _sz]),
    "lcpc_transcript_free": (None, [_vp]),
    "lcpc_prove": (_i32, [_vp, _vp, _u64, _vp, _vp, _vp, _vp]),
    "lcpc_verify": (_i32, [_vp, _vp, _vp, _u64, _vp, _u64, _vp, _u64, _vp, _vp]),
    "lcpc_root_bincode": (None, [_vp, _vp]),
    "lcpc_free": (None, [_vp]),
    "lcpc_shard_layout": (_i32, [_vp, _u64, _vp, _vp, _vp, _vp, _vp]),
    "lcpc_shard_nodes": (_i32, [_u64, _u32, _u32, _vp, _vp, _vp]),
    "lcpc_shard_nodes_field": (_i32, [_u32, _u64, _u32, _u32, _vp, _vp, _vp]),
    "lcpc_comm_unique_id": (_i32, [_vp]),
    "lcpc_comm_init": (_i32, [_vp, _vp, _u32, _u32]),
    "lcpc_comm_destroy": (_i32, [_vp]),
    "lcpc_commit_sharded_device": (_i32, [_vp, _vp, _u64, _vp, _u32, _vp]),
    "lcpc_prove_sharded_rccl": (_i32, [_vp, _vp, _u64, _vp, _vp, _vp, _vp]),
    "lcpc_commit_shard_device": (_i32, [_vp, _vp, _u64, _vp, _u32, _vp]),
    "lcpc_commit_finish_device": (_i32, [_vp, _vp, _u64, _u32, _vp, _vp]),
    "lcpc_collapse_device": (_i32, [_vp, _vp, _u32, _vp, _vp]),
    "lcpc_field_sum_device": (_i32, [_vp, _vp, _u32, _u64, _vp, _vp]),
    "lcpc_prove_sharded_bytes": (_u64, [_vp, _u64]),
    "lcpc_prove_sharded": (_i32, [_vp, _vp, _u64, _vp, _vp, _vp, _u64, ALLGATHER_FN, _vp, _vp, _vp, _vp]),
    "lcpc_shard_exchange_probe": (_i32, [_vp, _vp, C.POINTER(_u64)]),
    "lcpc_comm_rccl_version": (_i32, [C.POINTER(_i32)]),
    "lcpc_set_timing": (_i32, [_vp, _i32]),
    "lcpc_get_timings": (_i32, [_vp, C.POINTER(LcpcTimings)]),
}

# the batch extension (include/lcpc_hip_batch.h): its own prefix, table and version -- SYMBOLS and ABI_VERSION above are the core header's
BATCH_VERSION = 2


class LcpcxProveStats(C.Structure):
    _fields_ = [("groups", C.c_uint32), ("collapse_launches", C.c_uint32), ("open_launches", C.c_uint32), ("host_syncs", C.c_uint32)]


PROVE_ARENA_BUDGET = 64 << 20      # LCPCX_PROVE_ARENA_BUDGET
BATCH_SYMBOLS = {
    "lcpcx_batch_version": (_i32, []),
    "lcpcx_commit_batch_device": (_i32, [C.POINTER(_vp), _u32, _vp, _u64, _u64, _vp, _u32, _vp]),
    "lcpcx_prove_batch": (_i32, [C.POINTER(_vp), _u32, _vp, _u64, _u64, C.POINTER(_vp), C.POINTER(_vp), C.POINTER(_u64), _vp,
                                 C.POINTER(LcpcxProveStats)]),
}

# the verifier-side extension (include/lcpc_hip_verify.h): again its own prefix, table and version
VERIFY_VERSION = 1


class LcpcvVerifyStats(C.Structure):
    _fields_ = [("groups", C.c_uint32), ("encode_launches", C.c_uint32), ("hash_launches", C.c_uint32), ("check_launches", C.c_uint32),
                ("host_syncs", C.c_uint32)]


VERIFY_ARENA_BUDGET = 64 << 20     # LCPCV_ARENA_BUDGET
VERIFY_PATH_BUDGET = 64 << 20      # LCPCV_PATH_BUDGET
VERIFY_SYMBOLS = {
    "lcpcv_version": (_i32, []),
    "lcpcv_verify_batch": (_i32, [_vp, _u32, _vp, _vp, _u64, _u64, _vp, _u64, _u64, C.POINTER(_vp), C.POINTER(_u64), C.POINTER(_vp), _vp,
                                  _vp, C.POINTER(LcpcvVerifyStats)]),
}

# the column-check extension (include/lcpc_hip_columns.h): again its own prefix, table and version
COLUMNS_VERSION = 1
COLUMNS_SYMBOLS = {
    "lcpcp_version": (_i32, []),
    "lcpcp_check_columns": (_i32, [_vp, _vp, _vp, _u32, _u64, _vp, _vp, _vp]),
}

# the plain-integer extension (include/lcpc_hip_ints.h): again its own prefix, table and version
INTS_VERSION = 1
INTS_KINDS = {"u32": 0, "i32": 1, "u64": 2, "i64": 3, "wide": 4}      # lcpci_kind
INTS_SYMBOLS = {
    "lcpci_version": (_i32, []),
    "lcpci_from_ints": (_i32, [_u32, _u32, _vp, _u64, _vp]),
    "lcpci_to_canon": (_i32, [_u32, _vp, _u64, _vp]),
    "lcpci_from_ints_device": (_i32, [_vp, _u32, _vp, _u64, _vp, _vp]),
    "lcpci_commit_ints_device": (_i32, [_vp, _u32, _vp, _u64, _vp, _vp]),
    "lcpci_commit_ints": (_i32, [_vp, _u32, _vp, _u64, _vp]),
}

# the evaluation extension (include/lcpc_hip_eval.h): again its own prefix, table and version
EVAL_VERSION = 1
EVAL_BASES = {"powers": 0, "ml_monomial": 1, "ml_lagrange": 2}      # lcpce_basis
EVAL_SYMBOLS = {
    "lcpce_version": (_i32, []),
    "lcpce_tensors": (_i32, [_u32, _u32, _vp, _u32, _u64, _u64, _vp, _vp]),
    "lcpce_tensors_device": (_i32, [_vp, _u32, _vp, _u32, _u32, _u64, _u64, _vp, _vp, _vp]),
    "lcpce_dot_device": (_i32, [_vp, _vp, _u64, _vp, _u64, _u64, _u32, _vp, _vp]),
    "lcpce_eval_tensors_device": (_i32, [_vp, _vp, _vp, _u32, _vp, _vp]),
    "lcpce_eval_device": (_i32, [_vp, _u32, _vp, _u32, _u32, _vp, _vp]),
    "lcpce_eval": (_i32, [_vp, _u32, _vp, _u32, _u32, _vp]),
}

# the transform extension (include/lcpc_hip_fft.h): again its own prefix, table and version
FFT_VERSION = 1
FFT_FORMS = {"fft_ii": 0, "fft_io": 1, "fft_oi": 2, "ifft_ii": 3, "ifft_io": 4, "ifft_oi": 5}      # lcpcf_form
FFT_ORDERS = {"natural": 0, "bitrev": 1}                                                          # lcpcf_order
FFT_SYMBOLS = {
    "lcpcf_version": (_i32, []),
    "lcpcf_max_log_n": (_u32, [_u32]),
    "lcpcf_fft": (_i32, [_u32, _u32, _vp, _vp, _u32]),
    "lcpcf_fft_device": (_i32, [_vp, _u32, _vp, _vp, _u32, _u32, _vp]),
    "lcpcf_commit_evals_device": (_i32, [_vp, _u32, _vp, _u32, _vp, _vp]),
    "lcpcf_commit_evals": (_i32, [_vp, _u32, _vp, _u32, _vp]),
}

# the domain extension (include/lcpc_hip_domain.h): again its own prefix, table and version; its forms are FFT_FORMS
DOMAIN_VERSION = 1
DOMAIN_ORDERS = {"natural": 0, "bitrev": 1}                                                       # lcpcd_order
DOMAIN_SYMBOLS = {
    "lcpcd_version": (_i32, []),
    "lcpcd_generator": (_i32, [_u32, _vp]),
    "lcpcd_coset_fft": (_i32, [_u32, _u32, _vp, _vp, _vp, _u32]),
    "lcpcd_coset_fft_device": (_i32, [_vp, _u32, _vp, _vp, _vp, _u32, _u32, _vp]),
    "lcpcd_extend": (_i32, [_u32, _vp, _vp, _u64, _u32, _u32, _vp]),
    "lcpcd_extend_device": (_i32, [_vp, _vp, _vp, _u64, _u32, _u32, _vp, _u32, _vp]),
    "lcpcd_lde_device": (_i32, [_vp, _u32, _vp, _vp, _u32, _vp, _u32, _u32, _vp, _vp, _u32, _vp]),
    "lcpcd_commit_coset_evals_device": (_i32, [_vp, _u32, _vp, _vp, _u32, _vp, _vp]),
    "lcpcd_commit_coset_evals": (_i32, [_vp, _u32, _vp, _vp, _u32, _vp]),
    "lcpcd_commit_values_device": (_i32, [_vp, _vp, _u32, _u32, _vp, _vp]),
}

# the quotient extension (include/lcpc_hip_quot.h): again its own prefix, table and version; its orders are DOMAIN_ORDERS
QUOT_VERSION = 1
QUOT_OPS = {"add": 0, "sub": 1, "mul": 2, "div": 3}                                               # lcpcq_op
QUOT_SYMBOLS = {
    "lcpcq_version": (_i32, []),
    "lcpcq_batch_inverse": (_i32, [_u32, _vp, _vp, _u64]),
    "lcpcq_batch_inverse_device": (_i32, [_vp, _vp, _vp, _u64, _vp]),
    "lcpcq_pointwise": (_i32, [_u32, _u32, _vp, _vp, _vp, _u64]),
    "lcpcq_pointwise_device": (_i32, [_vp, _u32, _vp, _vp, _vp, _u64, _vp]),
    "lcpcq_divide_linear": (_i32, [_u32, _vp, _u32, _vp, _u32, _vp, _vp, _vp]),
    "lcpcq_divide_linear_device": (_i32, [_vp, _vp, _u32, _vp, _u32, _u32, _vp, _vp, _vp, _vp]),
    "lcpcq_divide_vanishing": (_i32, [_u32, _vp, _u32, _vp, _u32, _u32, _vp]),
    "lcpcq_divide_vanishing_device": (_i32, [_vp, _vp, _u32, _vp, _u32, _u32, _u32, _vp, _vp]),
}

# the scan extension (include/lcpc_hip_scan.h): again its own prefix, table and version
SCAN_VERSION = 1
SCAN_OPS = {"sum": 0, "product": 1}                                                               # lcpcs_op
SCAN_MODES = {"inclusive": 0, "exclusive": 1}                                                     # lcpcs_mode
SCAN_SYMBOLS = {
    "lcpcs_version": (_i32, []),
    "lcpcs_scan": (_i32, [_u32, _u32, _u32, _vp, _vp, _u64, _vp, _vp]),
    "lcpcs_scan_ratio": (_i32, [_u32, _u32, _u32, _vp, _vp, _vp, _u64, _vp, _vp]),
    "lcpcs_scan_work_bytes": (_u64, [_vp, _u64, _u32]),
    "lcpcs_scan_device": (_i32, [_vp, _u32, _u32, _vp, _vp, _u64, _u32, _vp, _vp, _vp, _u64, _vp]),
    "lcpcs_scan_ratio_device": (_i32, [_vp, _u32, _u32, _vp, _vp, _vp, _u64, _u32, _vp, _vp, _vp, _u64, _vp]),
}

# the sumcheck extension (include/lcpc_hip_sumcheck.h): again its own prefix, table and version
SUMCHECK_VERSION = 1
SUMCHECK_ORDERS = {"low": 0, "high": 1}                                                           # lcpcm_order
SUMCHECK_MAX_TABLES, SUMCHECK_MAX_TERMS, SUMCHECK_MAX_FACTORS = 8, 4, 4


class LcpcmTerm(C.Structure):
    _fields_ = [("n_factors", C.c_uint32), ("table", C.c_uint32 * SUMCHECK_MAX_FACTORS)]


SUMCHECK_SYMBOLS = {
    "lcpcm_version": (_i32, []),
    "lcpcm_bind": (_i32, [_u32, _u32, _vp, _vp, _u64, _vp]),
    "lcpcm_round": (_i32, [_u32, _u32, _vp, _u32, _vp, _u32, _vp, _u64, _vp]),
    "lcpcm_round_work_bytes": (_u64, [_vp, _u64, _u32]),
    "lcpcm_bind_device": (_i32, [_vp, _u32, _vp, _vp, _u32, _u64, _vp, _vp]),
    "lcpcm_round_device": (_i32, [_vp, _u32, _vp, _u32, _vp, _u32, _vp, _u64, _vp, _vp, _u64, _vp]),
    "lcpcm_bind_round_device": (_i32, [_vp, _u32, _vp, _vp, _u32, _vp, _u32, _vp, _u64, _vp, _vp, _vp, _u64, _vp]),
}


def build(force=False):
    """compile lcpc_amd/lib/liblcpc_hip.so for gfx950 (hipcc cross-compiles without a GPU)."""
    if force:
        subprocess.check_call(["make", "-C", CSRC, "-s", "clean"])
    subprocess.check_call(["make", "-C", CSRC, "-s", "-j4"])
    return LIB_PATH


_lib = None


def lib():
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise RuntimeError("lcpc_amd: %s is missing -- run `python -c 'import __graft_entry__ as g; g.build()'` "
                               "(there is no CPU fallback)" % LIB_PATH)
        try:
            # when torch shares the process (tests, bench.py) its bundled HIP runtime must be the one that gets
            # loaded first; loading ROCm's copy first leaves torch unable to see the GPU ("No HIP GPUs are available")
            import torch  # noqa: F401
        except ImportError:
            pass
        L = C.CDLL(LIB_PATH)
        for name, (res, args) in SYMBOLS.items():
            fn = getattr(L, name)          # AttributeError here = header/library mismatch
            fn.restype = res
            fn.argtypes = args
        if L.lcpc_abi_version() != ABI_VERSION:
            raise RuntimeError("lcpc_amd: ABI version mismatch")
        for name, (res, args) in BATCH_SYMBOLS.items():
            fn = getattr(L, name)
            fn.restype = res
            fn.argtypes = args
        if L.lcpcx_batch_version() != BATCH_VERSION:
            raise RuntimeError("lcpc_amd: batch extension version mismatch")
        for name, (res, args) in VERIFY_SYMBOLS.items():
            fn = getattr(L, name)
            fn.restype = res
            fn.argtypes = args
        if L.lcpcv_version() != VERIFY_VERSION:
            raise RuntimeError("lcpc_amd: verify extension version mismatch")
        for name, (res, args) in COLUMNS_SYMBOLS.items():
            fn = getattr(L, name)
            fn.restype = res
            fn.argtypes = args
        if L.lcpcp_version() != COLUMNS_VERSION:
            raise RuntimeError("lcpc_amd: column-check extension version mismatch")
        for name, (res, args) in INTS_SYMBOLS.items():
            fn = getattr(L, name)
            fn.restype = res
            fn.argtypes = args
        if L.lcpci_version() != INTS_VERSION:
            raise RuntimeError("lcpc_amd: integer extension version mismatch")
        for name, (res, args) in EVAL_SYMBOLS.items():
            fn = getattr(L, name)
            fn.restype = res
            fn.argtypes = args
        if L.lcpce_version() != EVAL_VERSION:
            raise RuntimeError("lcpc_amd: evaluation extension version mismatch")
        for name, (res, args) in FFT_SYMBOLS.items():
            fn = getattr(L, name)
            fn.restype = res
            fn.argtypes = args
        if L.lcpcf_version() != FFT_VERSION:
            raise RuntimeError("lcpc_amd: transform extension version mismatch")
        for name, (res, args) in DOMAIN_SYMBOLS.items():
            fn = getattr(L, name)
            fn.restype = res
            fn.argtypes = args
        if L.lcpcd_version() != DOMAIN_VERSION:
            raise RuntimeError("lcpc_amd: domain extension version mismatch")
        for name, (res, args) in QUOT_SYMBOLS.items():
            fn = getattr(L, name)
            fn.restype = res
            fn.argtypes = args
        if L.lcpcq_version() != QUOT_VERSION:
            raise RuntimeError("lcpc_amd: quotient extension version mismatch")
        for name, (res, args) in SCAN_SYMBOLS.items():
            fn = getattr(L, name)
            fn.restype = res
            fn.argtypes = args
        if L.lcpcs_version() != SCAN_VERSION:
            raise RuntimeError("lcpc_amd: scan extension version mismatch")
        for name, (res, args) in SUMCHECK_SYMBOLS.items():
            fn = getattr(L, name)
            fn.restype = res
            fn.argtypes = args
        if L.lcpcm_version() != SUMCHECK_VERSION:
            raise RuntimeError("lcpc_amd: sumcheck extension version mismatch")
        _lib = L
    return _lib

"""What the ctypes sides of the native test harnesses share (tests/*_harness.py over tests/native/*_harness.cpp): the two error
classes, the pointer and return-code helpers, the loader of lcpc_amd/lib/liblcpc_<stem>_harness.so, and the canary-padded output
buffers of k12 .. k18.  Every call of a harness returns after the device has finished; BadArgs means the harness refused the call
before touching the device, HipError carries the hipError_t of anything else that went wrong."""
import ctypes as C
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CANARY = 0x5A5A5A5A5A5A5A5A                         # fft_cases.CANARY
PAD = 8                                             # canary elements in front of and behind an output


class BadArgs(ValueError):
    pass


class HipError(RuntimeError):
    def __init__(self, what, code):
        RuntimeError.__init__(self, "%s: hipError_t %d" % (what, code))
        self.code = code


def ptr(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def check(what, rc):
    if rc == -1:
        raise BadArgs(what)
    if rc:
        raise HipError(what, rc)


def lib_path(stem):
    return os.path.join(ROOT, "lcpc_amd", "lib", "liblcpc_%s_harness.so" % stem)


_libs = {}


def load(stem, symbols):
    """liblcpc_<stem>_harness.so with the restype / argtypes of `symbols`: name -> argtypes (the result is an int) or name ->
    (restype, argtypes).  Loaded once"""
    if stem not in _libs:
        path = lib_path(stem)
        if not os.path.exists(path):
            raise RuntimeError("%s is missing -- `make -C lcpc_amd/csrc` (or __graft_entry__.build()) builds it beside the product" % path)
        try:
            import torch  # noqa: F401  (its bundled HIP runtime must be the first one loaded: lcpc_amd/_lib.py)
        except ImportError:
            pass
        L = C.CDLL(path)
        for name, sig in symbols.items():
            fn = getattr(L, name)
            fn.restype, fn.argtypes = sig if isinstance(sig, tuple) else (C.c_int, sig)
        _libs[stem] = L
    return _libs[stem]


def padded(n, L):
    """n elements of L limbs for a harness to write, with PAD canary elements in front of and behind them"""
    return np.full((PAD + n + PAD, L), CANARY, np.uint64)


def inner(buf, what="the output"):
    """the n elements of a padded() buffer, whose canaries must have come back untouched"""
    assert (buf[:PAD] == CANARY).all() and (buf[-PAD:] == CANARY).all(), "elements around %s were written" % what
    return buf[PAD:-PAD]

"""Binding of include/zkv_diag_primitive.h: the known-answer harness of the arithmetic primitives (TEST ONLY; the case layouts are
documented in that header, the case bodies are csrc/zkv_selftest.h)."""
import ctypes as C

from . import _lib

MAX_CASES = 65536               # ZKV_DIAG_PRIMITIVE_MAX_CASES

# the entry points of include/zkv_diag_primitive.h (not in zkv.h: _lib.SYMBOLS mirrors zkv.h alone)
SYMBOLS = {
    'zkv_diag_primitive': (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_size_t, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)]),
}

_bound = None


def lib():
    """The library with the harness's symbols bound (AttributeError when one is not exported)."""
    global _bound
    L = _lib.lib()
    if _bound is not L:
        for name, (res, args) in SYMBOLS.items():
            fn = getattr(L, name)
            fn.restype = res
            fn.argtypes = args
        _bound = L
    return L

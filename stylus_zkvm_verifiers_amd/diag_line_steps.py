"""Binding of include/zkv_diag_line_steps.h: the known-answer harness of the tangent and chord steps of k_miller2 as fused column sums
(TEST ONLY; the case layout is documented in that header, the case body is selftest_line_sums in csrc/zkv_selftest.h)."""
import ctypes as C

from . import _lib

IN_WORDS, OUT_WORDS = 192, 624  # ZKV_DIAG_LINE_STEPS_IN, ZKV_DIAG_LINE_STEPS_OUT

# the entry point of include/zkv_diag_line_steps.h (not in zkv.h: _lib.SYMBOLS mirrors zkv.h alone)
SYMBOLS = {
    'zkv_diag_line_steps': (C.c_int, [C.c_int, C.c_size_t, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)]),
}

_bound = None


def lib():
    """The library with the harness's symbol bound (AttributeError when it is not exported)."""
    global _bound
    L = _lib.lib()
    if _bound is not L:
        for name, (res, args) in SYMBOLS.items():
            fn = getattr(L, name)
            fn.restype = res
            fn.argtypes = args
        _bound = L
    return L

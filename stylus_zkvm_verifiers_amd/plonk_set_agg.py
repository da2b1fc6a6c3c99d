"""Aggregate check on PLONK key sets (include/zkv_plonk_set_agg.h): the SRS classes of a set -- keys whose [1]_2 | [tau]_2 bytes are equal
share sub-batches when PlonkVerifierSet.set_aggregate_check is on.  PARITY UNPINNED BY CONSTRUCTION: the reference holds no PLONK code."""
import ctypes as C

from . import _lib, plonk_set

_P = C.c_void_p
# declared in include/zkv_plonk_set_agg.h (plonk_set.SYMBOLS mirrors zkv_plonk_set.h alone)
SYMBOLS = {
    'zkv_plonk_set_srs_classes': (C.c_int, [_P, C.POINTER(C.c_uint32), C.POINTER(C.c_size_t)]),
}

_bound = None


def lib():
    """The library with the PLONK-set symbols and this header's bound (AttributeError when one is not exported)."""
    global _bound
    L = plonk_set.lib()
    if _bound is not L:
        for name, (res, args) in SYMBOLS.items():
            fn = getattr(L, name)
            fn.restype = res
            fn.argtypes = args
        _bound = L
    return L


def srs_classes(handle, n_keys):
    """(class of every key, number of classes) of the PLONK set behind `handle`; classes are numbered by first appearance in key order."""
    out = (C.c_uint32 * max(n_keys, 1))()
    n = C.c_size_t(0)
    _lib.check(lib().zkv_plonk_set_srs_classes(handle, out, C.byref(n)), 'zkv_plonk_set_srs_classes')
    return list(out[:n_keys]), n.value

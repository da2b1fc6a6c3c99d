"""Binding of include/zkv_diag_gt.h: read-back of the fixed-base GT tables of an SP1 / RISC Zero context and of the product the final
exponentiation kernel forms from them (TEST ONLY)."""
import ctypes as C

import numpy as np

from . import _lib

P = 21888242871839275222246405745257275088696311157297823662689037894645226208583
_RINV = pow(1 << 261, -1, P)

# the entry points of include/zkv_diag_gt.h (not in zkv.h: _lib.SYMBOLS mirrors zkv.h alone)
SYMBOLS = {
    'zkv_diag_gt_info': (C.c_int, [C.c_void_p, C.c_void_p]),
    'zkv_diag_gt_read': (C.c_int, [C.c_void_p, C.c_int, C.c_uint32, C.c_uint32, C.c_void_p]),
    'zkv_diag_gt_product': (C.c_int, [C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p]),
    'zkv_diag_gt_cache': (C.c_int, [C.c_void_p, C.c_void_p]),
}

_bound = None


def lib():
    global _bound
    L = _lib.lib()
    if _bound is not L:
        for name, (res, args) in SYMBOLS.items():
            fn = getattr(L, name)
            fn.restype = res
            fn.argtypes = args
        _bound = L
    return L


def info(handle):
    """dict(built, windows, bytes, build_ms, tried) of the context `handle` (a zkv_ctx*, e.g. verifier._h)."""
    out = np.zeros(6, dtype=np.uint64)
    _lib.check(lib().zkv_diag_gt_info(handle, out.ctypes.data), 'zkv_diag_gt_info')
    return dict(built=bool(out[0]), windows=(int(out[1]), int(out[2])), bytes=int(out[3]), build_ms=int(out[4]) / 1000.0, tried=bool(out[5]))


def cache(handle):
    """dict(valid, fills, entries) of the walk-prefix cache of the context `handle`; all 0 for a context without one."""
    out = np.zeros(3, dtype=np.uint64)
    _lib.check(lib().zkv_diag_gt_cache(handle, out.ctypes.data), 'zkv_diag_gt_cache')
    return dict(valid=int(out[0]), fills=int(out[1]), entries=int(out[2]))


def _coeffs(w):
    fp = [sum(int(w[8 * i + k]) << (32 * k) for k in range(8)) * _RINV % P for i in range(12)]
    return [(fp[2 * i], fp[2 * i + 1]) for i in range(6)]


def read(handle, signal, window=0, d=1):
    """One stored Fp12 as six (re, im) pairs of canonical integers, order g0 g1 g2 h0 h1 h2; signal < 0: the folded Miller constant."""
    w = np.zeros(96, dtype=np.uint32)
    _lib.check(lib().zkv_diag_gt_read(handle, signal, window, d, w.ctypes.data), 'zkv_diag_gt_read')
    return _coeffs(w)


def product(handle, signal_pairs):
    """The product M the lane-pair final exponentiation kernel forms for each (s0, s1) of `signal_pairs` (integers), one proof per lane
    pair in the order given: a list of Fp12 values in the form `read` returns."""
    n = len(signal_pairs)
    sc = np.array([[(s >> (32 * k)) & 0xFFFFFFFF for s in pair for k in range(8)] for pair in signal_pairs], dtype=np.uint32)
    out = np.zeros((n, 96), dtype=np.uint32)
    _lib.check(lib().zkv_diag_gt_product(handle, n, sc.ctypes.data, out.ctypes.data), 'zkv_diag_gt_product')
    return [_coeffs(out[i]) for i in range(n)]

"""Binding of include/zkv_diag_prep.h: read-back of the public signals the PREP stage derived (TEST ONLY; layout in that header)."""
import ctypes as C

import numpy as np

from . import _lib

SIGNALS = 5                     # ZKV_DIAG_PREP_SIGNALS

# the entry point of include/zkv_diag_prep.h (not in zkv.h: _lib.SYMBOLS mirrors zkv.h alone)
SYMBOLS = {
    'zkv_diag_prep_signals': (C.c_int, [C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p]),
}

_bound = None


def lib():
    """The library with the reader's symbol bound (AttributeError when it is not exported)."""
    global _bound
    L = _lib.lib()
    if _bound is not L:
        for name, (res, args) in SYMBOLS.items():
            fn = getattr(L, name)
            fn.restype = res
            fn.argtypes = args
        _bound = L
    return L


def prep_signals(handle, n):
    """(signals, flags) of the first n proofs of the most recent chunk of the context `handle` (a zkv_ctx*, e.g. verifier._h):
    signals[j][b] is signal b of proof j as a Python int, flags[j] the proof's flags word (0: no signals were stored for it)."""
    sig = np.zeros((n, SIGNALS, 8), dtype=np.uint32)
    fl = np.zeros(n, dtype=np.uint32)
    _lib.check(lib().zkv_diag_prep_signals(handle, n, sig.ctypes.data, fl.ctypes.data), 'zkv_diag_prep_signals')
    vals = [[sum(int(sig[j, b, k]) << (32 * k) for k in range(8)) for b in range(SIGNALS)] for j in range(n)]
    return vals, [int(x) for x in fl]

"""eth_call batches and a method per seal on a RISC Zero router WITH a set route (include/zkv_risc0_router_set_wire.h): raw `verify` /
`verifyIntegrity` calldata whose seal may be a set-inclusion seal of any length, decoded, routed, hashed and grouped on the device.  The
functions take any router handle: without a set route they answer what risc0_router_wire's answer.  RiscZeroSetRouter's
verify_call_batch / eth_call_batch / eth_call_batch_dev / last_call_counts are the front of this module.  PARITY UNPINNED: the reference
holds no router and no set verifier."""
import ctypes as C

import numpy as np

from . import _lib, risc0_router_set, risc0_router_wire
from .risc0 import _blob, _cat32, _same_len
from .risc0_router_wire import RETURNDATA_STRIDE

_P, _SZ = C.c_void_p, C.c_size_t
# declared in include/zkv_risc0_router_set_wire.h
SYMBOLS = {
    'zkv_risc0_router_verify_call_ragged_dev': (C.c_int, [_P, _SZ, _P, _P, _P, C.c_uint64, _P, _P, _P, _P, _P]),
    'zkv_risc0_router_verify_call_ragged': (C.c_int, [_P, _SZ, _P, _P, _P, _P, _P, _P, _P]),
    'zkv_risc0_router_eth_call_ragged_dev': (C.c_int, [_P, _SZ, _P, _P, C.c_uint64, _P, _P, _P, _P]),
    'zkv_risc0_router_eth_call_ragged': (C.c_int, [_P, _SZ, _P, _P, _P, _P, _P, _P]),
    'zkv_risc0_router_last_ragged_call_counts': (C.c_int, [_P, C.POINTER(C.c_uint64)]),
}

_bound = None


def lib():
    """The library with the neighbouring headers' symbols and this header's bound (AttributeError when one is not exported)."""
    global _bound
    risc0_router_wire.lib()
    L = risc0_router_set.lib()
    if _bound is not L:
        for name, (res, args) in SYMBOLS.items():
            fn = getattr(L, name)
            fn.restype = res
            fn.argtypes = args
        _bound = L
    return L


def verify_call_ragged(handle, methods, seals, in_a, in_b):
    """Ragged host buffers with a method per seal (None: all verify) -> (status uint8[n], received selector uint8[n, 4])."""
    n = len(seals)
    _same_len(n, in_a=in_a, in_b=in_b)
    if methods is not None:
        _same_len(n, methods=methods)
        methods = np.ascontiguousarray(methods, dtype=np.uint8)
    blob, off = _blob(seals)
    st = np.zeros(n, dtype=np.uint8); rv = np.zeros((n, 4), dtype=np.uint8)
    _lib.check(lib().zkv_risc0_router_verify_call_ragged(handle, n, methods.ctypes.data if methods is not None and n else None, blob, off.ctypes.data,
                                                         _cat32(in_a, 'in_a'), _cat32(in_b, 'in_b'), st.ctypes.data, rv.ctypes.data),
               'zkv_risc0_router_verify_call_ragged')
    return st, rv


def verify_call_ragged_dev(handle, n, d_method, d_seal_blob, d_seal_off, blob_bytes, d_in_a, d_in_b, d_status, d_recv=0, stream=0):
    """Device-resident: n method bytes (0: all verify), the blob (any alignment) and its n + 1 uint64 offsets, two rows of n x 32 bytes,
    n status bytes and n x 4 received selectors (0: none); enqueued on `stream`."""
    _lib.check(lib().zkv_risc0_router_verify_call_ragged_dev(handle, n, d_method or None, d_seal_blob or None, d_seal_off, blob_bytes, d_in_a, d_in_b,
                                                             d_status, d_recv or None, stream or None), 'zkv_risc0_router_verify_call_ragged_dev')


def eth_call_ragged(handle, calls):
    """calls: list of calldata byte strings -> (reverted uint8[n], [return / revert data], status uint8[n])."""
    n = len(calls)
    off = np.zeros(n + 1, dtype=np.uint64)
    if n:
        off[1:] = np.cumsum([len(c) for c in calls], dtype=np.uint64)
    blob = b''.join(bytes(c) for c in calls) + b'\0'
    rev = np.zeros(n, dtype=np.uint8); st = np.zeros(n, dtype=np.uint8)
    ret = np.zeros((n, RETURNDATA_STRIDE), dtype=np.uint8); ln = np.zeros(n, dtype=np.uint32)
    _lib.check(lib().zkv_risc0_router_eth_call_ragged(handle, n, blob, off.ctypes.data, rev.ctypes.data, ret.ctypes.data, ln.ctypes.data, st.ctypes.data),
               'zkv_risc0_router_eth_call_ragged')
    return rev, [ret[i, :ln[i]].tobytes() for i in range(n)], st


def eth_call_ragged_dev(handle, n, d_calldata, d_calldata_off, calldata_bytes, d_status, d_recv=0, d_call_kind=0, stream=0):
    _lib.check(lib().zkv_risc0_router_eth_call_ragged_dev(handle, n, d_calldata, d_calldata_off, calldata_bytes, d_status, d_recv or None,
                                                          d_call_kind or None, stream or None), 'zkv_risc0_router_eth_call_ragged_dev')


def last_ragged_call_counts(handle, route_count):
    """Seals of the most recent call per route (the set route under its own index), unknown selector, short, bad calldata."""
    out = (C.c_uint64 * (route_count + 3))()
    _lib.check(lib().zkv_risc0_router_last_ragged_call_counts(handle, out), 'zkv_risc0_router_last_ragged_call_counts')
    return list(out)

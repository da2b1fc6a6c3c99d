"""eth_call batches on a RISC Zero router (include/zkv_risc0_router_wire.h): raw `verify` / `verifyIntegrity` calldata in either form --
uint8[] arrays, as a Stylus shell sees `Vec<u8>`, or packed `bytes`, IRiscZeroVerifier's Solidity ABI -- decoded and routed on the device,
and the decoded-input call with a method per seal.  RiscZeroRouter's verify_call_batch / eth_call_batch / encode_* methods are the front
of this module.  PARITY UNPINNED: the reference holds no router."""
import ctypes as C

import numpy as np

from . import _lib, risc0_router
from .risc0 import _blob, _cat32, _same_len

FORM_UINT8_ARRAY, FORM_BYTES = 0, 1         # ZKV_CALLDATA_FORM_*
METHOD_VERIFY, METHOD_VERIFY_INTEGRITY = 0, 1   # ZKV_METHOD_*
CALL_KIND_BAD = 255                         # ZKV_RISC0_ROUTER_CALL_KIND_BAD; a decoded call has kind 2 * form + method
SIGNATURES = {0: b'verify(uint8[],bytes32,bytes32)', 1: b'verifyIntegrity(uint8[],bytes32)',
              2: b'verify(bytes,bytes32,bytes32)', 3: b'verifyIntegrity((bytes,bytes32))'}      # by call kind
RETURNDATA_STRIDE = 96                      # ZKV_RETURNDATA_STRIDE
STATUS_BAD_CALLDATA = 6                     # ZKV_STATUS_BAD_CALLDATA

_P, _SZ = C.c_void_p, C.c_size_t
# declared in include/zkv_risc0_router_wire.h (risc0_router.SYMBOLS mirrors zkv_risc0_router.h alone)
SYMBOLS = {
    'zkv_risc0_router_verify_call_batch': (C.c_int, [_P, _SZ, _P, _P, _P, _P, _P, _P, _P]),
    'zkv_risc0_router_verify_call_batch_dev': (C.c_int, [_P, _SZ, _P, _P, _P, _P, _P, _P, _P]),
    'zkv_risc0_router_encode_verify_call': (C.c_size_t, [C.c_int, C.c_char_p, _SZ, C.c_char_p, C.c_char_p, C.c_char_p, _SZ]),
    'zkv_risc0_router_encode_verify_integrity_call': (C.c_size_t, [C.c_int, C.c_char_p, _SZ, C.c_char_p, C.c_char_p, _SZ]),
    'zkv_risc0_router_eth_call_batch': (C.c_int, [_P, _SZ, _P, _P, _P, _P, _P, _P]),
    'zkv_risc0_router_eth_call_batch_dev': (C.c_int, [_P, _SZ, _P, _P, C.c_uint64, _P, _P, _P, _P]),
    'zkv_risc0_router_eth_call_returndata': (C.c_int, [_P, C.c_uint8, C.c_char_p, C.c_uint8, C.c_char_p, C.POINTER(C.c_uint32), C.POINTER(C.c_uint8)]),
    'zkv_risc0_router_last_call_counts': (C.c_int, [_P, C.POINTER(C.c_uint64)]),
}

_bound = None


def lib():
    """The library with the router's symbols and this header's bound (AttributeError when one is not exported)."""
    global _bound
    L = risc0_router.lib()
    if _bound is not L:
        for name, (res, args) in SYMBOLS.items():
            fn = getattr(L, name)
            fn.restype = res
            fn.argtypes = args
        _bound = L
    return L


def selector(form, method):
    """The 4-byte function selector of a call kind (keccak-256 of its signature)."""
    o = C.create_string_buffer(4)
    _lib.check(_lib.lib().zkv_abi_function_selector(SIGNATURES[2 * form + method], o), 'zkv_abi_function_selector')
    return o.raw


def _encode(fn, form, *args):
    if form not in (FORM_UINT8_ARRAY, FORM_BYTES):
        raise ValueError('form must be FORM_UINT8_ARRAY or FORM_BYTES')
    n = fn(form, *args, None, 0)
    o = C.create_string_buffer(max(n, 1))
    fn(form, *args, o, n)
    return o.raw[:n]


def encode_verify_call(seal, image_id, journal_digest, form=FORM_BYTES):
    """Canonical calldata of verify(seal, image_id, journal_digest) in `form`."""
    seal, image_id, journal_digest = bytes(seal), bytes(image_id), bytes(journal_digest)
    if len(image_id) != 32 or len(journal_digest) != 32:
        raise ValueError('image_id and journal_digest must be 32 bytes')
    return _encode(lib().zkv_risc0_router_encode_verify_call, form, seal, len(seal), image_id, journal_digest)


def encode_verify_integrity_call(seal, claim_digest, form=FORM_BYTES):
    """Canonical calldata of verifyIntegrity(Receipt(seal, claim_digest)) in `form`."""
    seal, claim_digest = bytes(seal), bytes(claim_digest)
    if len(claim_digest) != 32:
        raise ValueError('claim_digest must be 32 bytes')
    return _encode(lib().zkv_risc0_router_encode_verify_integrity_call, form, seal, len(seal), claim_digest)


def verify_call_batch(handle, methods, seals, in_a, in_b):
    """Ragged host buffers with a method per seal (None: all verify) -> (status uint8[n], received selector uint8[n, 4])."""
    n = len(seals)
    _same_len(n, in_a=in_a, in_b=in_b)
    if methods is not None:
        _same_len(n, methods=methods)
        methods = np.ascontiguousarray(methods, dtype=np.uint8)
    blob, off = _blob(seals)
    st = np.zeros(n, dtype=np.uint8); rv = np.zeros((n, 4), dtype=np.uint8)
    _lib.check(lib().zkv_risc0_router_verify_call_batch(handle, n, methods.ctypes.data if methods is not None and n else None, blob, off.ctypes.data,
                                                        _cat32(in_a, 'in_a'), _cat32(in_b, 'in_b'), st.ctypes.data, rv.ctypes.data),
               'zkv_risc0_router_verify_call_batch')
    return st, rv


def verify_call_batch_dev(handle, n, d_method, d_seals, d_in_a, d_in_b, d_status, d_recv=0, stream=0):
    _lib.check(lib().zkv_risc0_router_verify_call_batch_dev(handle, n, d_method or None, d_seals, d_in_a, d_in_b, d_status, d_recv or None, stream or None),
               'zkv_risc0_router_verify_call_batch_dev')


def eth_call_batch(handle, calls):
    """calls: list of calldata byte strings -> (reverted uint8[n], [return / revert data], status uint8[n])."""
    n = len(calls)
    off = np.zeros(n + 1, dtype=np.uint64)
    if n:
        off[1:] = np.cumsum([len(c) for c in calls], dtype=np.uint64)
    blob = b''.join(bytes(c) for c in calls) + b'\0'
    rev = np.zeros(n, dtype=np.uint8); st = np.zeros(n, dtype=np.uint8)
    ret = np.zeros((n, RETURNDATA_STRIDE), dtype=np.uint8); ln = np.zeros(n, dtype=np.uint32)
    _lib.check(lib().zkv_risc0_router_eth_call_batch(handle, n, blob, off.ctypes.data, rev.ctypes.data, ret.ctypes.data, ln.ctypes.data, st.ctypes.data),
               'zkv_risc0_router_eth_call_batch')
    return rev, [ret[i, :ln[i]].tobytes() for i in range(n)], st


def eth_call_batch_dev(handle, n, d_calldata, d_calldata_off, calldata_bytes, d_status, d_recv=0, d_call_kind=0, stream=0):
    _lib.check(lib().zkv_risc0_router_eth_call_batch_dev(handle, n, d_calldata, d_calldata_off, calldata_bytes, d_status, d_recv or None,
                                                         d_call_kind or None, stream or None), 'zkv_risc0_router_eth_call_batch_dev')


def eth_call_returndata(handle, status, received=bytes(4), call_kind=CALL_KIND_BAD):
    """(reverted, return / revert data) of one status of an eth_call batch; the data of a success depends on the call kind."""
    o = C.create_string_buffer(RETURNDATA_STRIDE); n = C.c_uint32(0); rev = C.c_uint8(0)
    _lib.check(lib().zkv_risc0_router_eth_call_returndata(handle, status, bytes(received), call_kind, o, C.byref(n), C.byref(rev)),
               'zkv_risc0_router_eth_call_returndata')
    return bool(rev.value), o.raw[:n.value]


def last_call_counts(handle, route_count):
    out = (C.c_uint64 * (route_count + 3))()
    _lib.check(lib().zkv_risc0_router_last_call_counts(handle, out), 'zkv_risc0_router_last_call_counts')
    return list(out)

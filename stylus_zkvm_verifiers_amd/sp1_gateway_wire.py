"""eth_call batches on an SP1 gateway (include/zkv_sp1_gateway_wire.h): raw `verifyProof` calldata in either form -- uint8[] arrays, as a
Stylus shell sees `Vec<u8>`, or packed `bytes`, ISP1Verifier's Solidity ABI -- decoded and routed on the device.  Sp1Gateway's
eth_call_batch / eth_call_batch_dev / encode_verify_proof_call are the front of this module.  PARITY UNPINNED: the reference holds no
gateway, no PLONK code and no router."""
import ctypes as C

import numpy as np

from . import _lib, sp1_gateway

FORM_UINT8_ARRAY, FORM_BYTES = 0, 1         # ZKV_CALLDATA_FORM_*
SIGNATURES = {FORM_UINT8_ARRAY: b'verifyProof(bytes32,uint8[],uint8[])', FORM_BYTES: b'verifyProof(bytes32,bytes,bytes)'}
RETURNDATA_STRIDE = 96                      # ZKV_RETURNDATA_STRIDE
STATUS_BAD_CALLDATA = 6                     # ZKV_STATUS_BAD_CALLDATA

_P, _SZ = C.c_void_p, C.c_size_t
# declared in include/zkv_sp1_gateway_wire.h (sp1_gateway.SYMBOLS mirrors zkv_sp1_gateway.h alone)
SYMBOLS = {
    'zkv_sp1_gateway_encode_verify_proof_call': (C.c_size_t, [C.c_int, C.c_char_p, C.c_char_p, _SZ, C.c_char_p, _SZ, C.c_char_p, _SZ]),
    'zkv_sp1_gateway_eth_call_batch': (C.c_int, [_P, _SZ, _P, _P, _P, _P, _P, _P]),
    'zkv_sp1_gateway_eth_call_batch_dev': (C.c_int, [_P, _SZ, _P, _P, C.c_uint64, _P, _P, _P]),
    'zkv_sp1_gateway_eth_call_returndata': (C.c_int, [_P, C.c_uint8, C.c_char_p, C.c_char_p, C.POINTER(C.c_uint32), C.POINTER(C.c_uint8)]),
    'zkv_sp1_gateway_last_call_counts': (C.c_int, [_P, C.POINTER(C.c_uint64)]),
}

_bound = None


def lib():
    """The library with the gateway symbols and this header's bound (AttributeError when one is not exported)."""
    global _bound
    L = sp1_gateway.lib()
    if _bound is not L:
        for name, (res, args) in SYMBOLS.items():
            fn = getattr(L, name)
            fn.restype = res
            fn.argtypes = args
        _bound = L
    return L


def selector(form):
    """The 4-byte function selector of a calldata form (keccak-256 of its signature)."""
    o = C.create_string_buffer(4)
    _lib.check(_lib.lib().zkv_abi_function_selector(SIGNATURES[form], o), 'zkv_abi_function_selector')
    return o.raw


def encode_verify_proof_call(program_vkey, public_values, proof_bytes, form=FORM_BYTES):
    """Canonical calldata of verifyProof(program_vkey, public_values, proof_bytes) in `form`."""
    if form not in SIGNATURES:
        raise ValueError('form must be FORM_UINT8_ARRAY or FORM_BYTES')
    vkey, pv, proof = bytes(program_vkey), bytes(public_values), bytes(proof_bytes)
    if len(vkey) != 32:
        raise ValueError('program_vkey must be 32 bytes')
    L = lib()
    n = L.zkv_sp1_gateway_encode_verify_proof_call(form, vkey, pv, len(pv), proof, len(proof), None, 0)
    o = C.create_string_buffer(max(n, 1))
    L.zkv_sp1_gateway_encode_verify_proof_call(form, vkey, pv, len(pv), proof, len(proof), o, n)
    return o.raw[:n]


def eth_call_batch(handle, calls):
    """calls: list of calldata byte strings -> (reverted uint8[n], [return / revert data], status uint8[n])."""
    n = len(calls)
    off = np.zeros(n + 1, dtype=np.uint64)
    if n:
        off[1:] = np.cumsum([len(c) for c in calls], dtype=np.uint64)
    blob = b''.join(bytes(c) for c in calls) + b'\0'
    rev = np.zeros(n, dtype=np.uint8); st = np.zeros(n, dtype=np.uint8)
    ret = np.zeros((n, RETURNDATA_STRIDE), dtype=np.uint8); ln = np.zeros(n, dtype=np.uint32)
    _lib.check(lib().zkv_sp1_gateway_eth_call_batch(handle, n, blob, off.ctypes.data, rev.ctypes.data, ret.ctypes.data, ln.ctypes.data, st.ctypes.data),
               'zkv_sp1_gateway_eth_call_batch')
    return rev, [ret[i, :ln[i]].tobytes() for i in range(n)], st


def eth_call_batch_dev(handle, n, d_calldata, d_calldata_off, calldata_bytes, d_status, d_recv=0, stream=0):
    _lib.check(lib().zkv_sp1_gateway_eth_call_batch_dev(handle, n, d_calldata, d_calldata_off, calldata_bytes, d_status, d_recv or None, stream or None),
               'zkv_sp1_gateway_eth_call_batch_dev')


def eth_call_returndata(handle, status, received=bytes(4)):
    """(reverted, return / revert data) of one status of an eth_call batch."""
    o = C.create_string_buffer(RETURNDATA_STRIDE); n = C.c_uint32(0); rev = C.c_uint8(0)
    _lib.check(lib().zkv_sp1_gateway_eth_call_returndata(handle, status, bytes(received), o, C.byref(n), C.byref(rev)), 'zkv_sp1_gateway_eth_call_returndata')
    return bool(rev.value), o.raw[:n.value]


def last_call_counts(handle, route_count):
    out = (C.c_uint64 * (route_count + 3))()
    _lib.check(lib().zkv_sp1_gateway_last_call_counts(handle, out), 'zkv_sp1_gateway_last_call_counts')
    return list(out)

"""eth_call batches on a Groth16 key set whose keys are deployed verifier contracts (include/zkv_groth16_set_wire.h): raw `verifyProof`
calldata of the Solidity verifiers snarkjs and gnark export, each request addressed to a contract, resolved, decoded and verified on the
device.  PARITY UNPINNED: the reference holds no generic contract shell."""
import ctypes as C

import numpy as np

from . import _lib, groth16_set
from .errors import VM_RISC0, VM_SP1
from .groth16 import MAX_IC

FORM_SNARKJS, FORM_GNARK = 0, 1             # ZKV_G16_FORM_*
SIGNATURES = {FORM_SNARKJS: 'verifyProof(uint256[2],uint256[2][2],uint256[2],uint256[%d])', FORM_GNARK: 'verifyProof(uint256[8],uint256[%d])'}
RETURNDATA_STRIDE = 96                      # ZKV_RETURNDATA_STRIDE
STATUS_BAD_CALLDATA = 6                     # ZKV_STATUS_BAD_CALLDATA
STATUS_NO_CONTRACT = 9                      # ZKV_STATUS_NO_CONTRACT
STATUS_INPUT_NOT_IN_FIELD = 10              # ZKV_STATUS_INPUT_NOT_IN_FIELD
NO_KEY = 0xFFFFFFFF

_P, _SZ = C.c_void_p, C.c_size_t
# declared in include/zkv_groth16_set_wire.h (groth16_set.SYMBOLS mirrors zkv_groth16_set.h alone)
SYMBOLS = {
    'zkv_groth16_set_create_deployed': (C.c_void_p, [_SZ, C.POINTER(C.c_char_p), C.POINTER(C.c_size_t), C.POINTER(C.c_int), C.c_char_p, C.c_char_p, C.c_int]),
    'zkv_groth16_set_call_selector': (C.c_int, [C.c_int, _SZ, C.c_char_p]),
    'zkv_groth16_set_eth_call_batch': (C.c_int, [_P, _SZ, _P, _P, _P, _P, _P, _P, _P]),
    'zkv_groth16_set_eth_call_batch_dev': (C.c_int, [_P, _SZ, _P, _P, _P, C.c_uint64, _P, _P, _P]),
    'zkv_groth16_set_eth_call_returndata': (C.c_int, [_P, C.c_uint32, C.c_uint8, C.c_char_p, C.POINTER(C.c_uint32), C.POINTER(C.c_uint8)]),
    'zkv_groth16_set_last_call_counts': (C.c_int, [_P, C.POINTER(C.c_uint64)]),
}

_bound = None


def lib():
    """The library with the key-set symbols and this header's bound (AttributeError when one is not exported)."""
    global _bound
    L = groth16_set.lib()
    if _bound is not L:
        for name, (res, args) in SYMBOLS.items():
            fn = getattr(L, name)
            fn.restype = res
            fn.argtypes = args
        _bound = L
    return L


def selector(form, n_signals):
    """The 4-byte selector of a form's verifyProof with n_signals public signals (keccak-256 of the signature, derived in the library)."""
    o = C.create_string_buffer(4)
    if lib().zkv_groth16_set_call_selector(form, n_signals, o) != 0:
        raise ValueError('form must be FORM_SNARKJS or FORM_GNARK and n_signals 1 .. %d' % (MAX_IC - 1))
    return o.raw


def encode_call(form, proof_words, signals):
    """Canonical calldata of verifyProof: the selector, the 256 proof bytes (the precompiles' word order), then the 32-byte signals."""
    proof, sig = bytes(proof_words), [bytes(s) for s in signals]
    if len(proof) != 256 or any(len(s) != 32 for s in sig):
        raise ValueError('a proof is 256 bytes and a signal 32')
    return selector(form, len(sig)) + proof + b''.join(sig)


class Groth16DeployedSet(groth16_set.Groth16VerifierSet):
    """keys: list of (vk_bytes, n_ic, vm_type, address, form): Groth16VerifierSet's triple, the contract's 20-byte address and
    FORM_SNARKJS / FORM_GNARK.  Every Groth16VerifierSet call works on it."""

    def __init__(self, keys, device=0):
        keys = list(keys)
        if not 1 <= len(keys) <= groth16_set.MAX_KEYS:
            raise ValueError('a key set holds 1 .. %d keys' % groth16_set.MAX_KEYS)
        for vk, n_ic, vm, addr, form in keys:
            if not 1 <= n_ic <= MAX_IC:
                raise ValueError('n_ic must be 1 .. %d' % MAX_IC)
            if len(vk) != 448 + 64 * n_ic:
                raise ValueError('verification key must be 448 + 64 * n_ic bytes')
            if vm not in (VM_RISC0, VM_SP1):
                raise ValueError('vm_type must be VM_RISC0 or VM_SP1')
            if len(addr) != 20:
                raise ValueError('an address is 20 bytes')
            if form not in SIGNATURES:
                raise ValueError('form must be FORM_SNARKJS or FORM_GNARK')
        self._L = lib()
        k = len(keys)
        self._vk = [bytes(key[0]) for key in keys]                   # alive for the call; the library copies them
        words = (C.c_char_p * k)(*self._vk)
        n_ic = (C.c_size_t * k)(*[key[1] for key in keys])
        vms = (C.c_int * k)(*[key[2] for key in keys])
        self._h = self._L.zkv_groth16_set_create_deployed(k, words, n_ic, vms, b''.join(bytes(key[3]) for key in keys), bytes(key[4] for key in keys), device)
        if not self._h:
            raise ValueError('zkv_groth16_set_create_deployed rejected the arguments (two keys with one address?)')
        self.n_ic = [key[1] for key in keys]
        self.addresses = [bytes(key[3]) for key in keys]
        self.forms = [key[4] for key in keys]

    selector = staticmethod(selector)
    encode_call = staticmethod(encode_call)

    def eth_call_batch(self, to, calls, offsets=None):
        """to: one 20-byte address per request; calls: one calldata byte string per request -- or, with `offsets` (n + 1 byte offsets), one
        blob that the offsets cut, which may then run backwards or past its end (offsets[n]).
        -> (reverted uint8[n], [return / revert data], status uint8[n])."""
        n = len(to)
        if offsets is None:
            if len(calls) != n:
                raise ValueError('one address per request')
            off = np.zeros(n + 1, dtype=np.uint64)
            if n:
                off[1:] = np.cumsum([len(c) for c in calls], dtype=np.uint64)
            blob = b''.join(bytes(c) for c in calls) + b'\0'
        else:
            off = np.ascontiguousarray(offsets, dtype=np.uint64)
            if off.shape != (n + 1,) or int(off[n]) > len(calls):
                raise ValueError('offsets must be n + 1 byte offsets, the last one inside the blob')
            blob = bytes(calls) + b'\0'
        if any(len(a) != 20 for a in to):
            raise ValueError('an address is 20 bytes')
        rev = np.zeros(n, dtype=np.uint8); st = np.zeros(n, dtype=np.uint8)
        ret = np.zeros((n, RETURNDATA_STRIDE), dtype=np.uint8); ln = np.zeros(n, dtype=np.uint32)
        _lib.check(self._L.zkv_groth16_set_eth_call_batch(self._h, n, b''.join(bytes(a) for a in to) + b'\0', blob, off.ctypes.data, rev.ctypes.data, ret.ctypes.data,
                                                          ln.ctypes.data, st.ctypes.data), 'zkv_groth16_set_eth_call_batch')
        return rev, [ret[i, :ln[i]].tobytes() for i in range(n)], st

    def eth_call_batch_dev(self, n, d_to, d_calldata, d_calldata_off, calldata_bytes, d_status, d_key=0, stream=0):
        """Device-resident batch: device pointers to n x 20 address bytes, the calldata, its n + 1 uint64 offsets, n status bytes and
        (optional) n uint32 resolved keys; enqueued on `stream` (0 = the context's stream)."""
        _lib.check(self._L.zkv_groth16_set_eth_call_batch_dev(self._h, n, d_to, d_calldata, d_calldata_off, calldata_bytes, d_status, d_key or None, stream or None),
                   'zkv_groth16_set_eth_call_batch_dev')

    def eth_call_returndata(self, key, status):
        """(reverted, return / revert data) of one status of a request that resolved to `key`."""
        o = C.create_string_buffer(RETURNDATA_STRIDE); n = C.c_uint32(0); rev = C.c_uint8(0)
        _lib.check(self._L.zkv_groth16_set_eth_call_returndata(self._h, key, status, o, C.byref(n), C.byref(rev)), 'zkv_groth16_set_eth_call_returndata')
        return bool(rev.value), o.raw[:n.value]

    def last_call_counts(self):
        """[placed, no contract, bad calldata, signal not in field] of the most recent eth_call batch."""
        out = (C.c_uint64 * 4)()
        _lib.check(self._L.zkv_groth16_set_last_call_counts(self._h, out), 'zkv_groth16_set_last_call_counts')
        return list(out)

    def last_wire_ms(self):
        f = C.c_float(0)
        _lib.check(_lib.lib().zkv_ctx_last_wire_ms(self._h, C.byref(f)), 'zkv_ctx_last_wire_ms')
        return f.value

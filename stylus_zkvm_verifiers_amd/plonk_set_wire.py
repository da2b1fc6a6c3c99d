"""eth_call batches on a PLONK key set whose keys are deployed gnark verifier contracts (include/zkv_plonk_set_wire.h): raw
`Verify(bytes,uint256[])` calldata, each request addressed to a contract, resolved, decoded, classified and verified on the device, and
answered with the contract's own return or revert data.  PARITY UNPINNED: the reference holds no PLONK code and no contract shell."""
import ctypes as C

import numpy as np

from . import _lib, plonk_set

SIGNATURE = 'Verify(bytes,uint256[])'
RETURNDATA_STRIDE = 128                     # ZKV_PLONK_RETURNDATA_STRIDE
STATUS_INVALID_PROOF_DATA = 4               # ZKV_STATUS_INVALID_PROOF_DATA
STATUS_BAD_CALLDATA = 6                     # ZKV_STATUS_BAD_CALLDATA
STATUS_NO_CONTRACT = 9                      # ZKV_STATUS_NO_CONTRACT
STATUS_INPUT_NOT_IN_FIELD = 10              # ZKV_STATUS_INPUT_NOT_IN_FIELD
# ZKV_PLONK_REVERT_*
REVERT_NONE, REVERT_INPUT_COUNT, REVERT_INPUT_RANGE, REVERT_PROOF_SIZE, REVERT_OPENING_RANGE, REVERT_EC_OPERATION = range(6)
NO_KEY = 0xFFFFFFFF

_P, _SZ = C.c_void_p, C.c_size_t
# declared in include/zkv_plonk_set_wire.h (plonk_set.SYMBOLS mirrors zkv_plonk_set.h alone)
SYMBOLS = {
    'zkv_plonk_set_create_deployed': (C.c_void_p, [_SZ, C.POINTER(C.c_char_p), C.POINTER(C.c_size_t), C.c_char_p, C.c_int]),
    'zkv_plonk_set_call_selector': (C.c_int, [C.c_char_p]),
    'zkv_plonk_set_eth_call_batch': (C.c_int, [_P, _SZ, _P, _P, _P, _P, _P, _P, _P, _P]),
    'zkv_plonk_set_eth_call_batch_dev': (C.c_int, [_P, _SZ, _P, _P, _P, C.c_uint64, _P, _P, _P, _P]),
    'zkv_plonk_set_eth_call_returndata': (C.c_int, [C.c_uint8, C.c_uint8, C.c_char_p, C.POINTER(C.c_uint32), C.POINTER(C.c_uint8)]),
    'zkv_plonk_set_last_call_counts': (C.c_int, [_P, C.POINTER(C.c_uint64)]),
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


def selector():
    """The 4-byte selector of Verify(bytes,uint256[]) (keccak-256 of the signature, derived in the library)."""
    o = C.create_string_buffer(4)
    _lib.check(lib().zkv_plonk_set_call_selector(o), 'zkv_plonk_set_call_selector')
    return o.raw


def encode_call(proof, public_inputs):
    """Canonical calldata of Verify: the selector, the two offsets, the proof as `bytes` (zero padded to 32), then the 32-byte inputs."""
    proof = bytes(proof)
    pub = [x.to_bytes(32, 'big') if isinstance(x, int) else bytes(x) for x in public_inputs]
    if any(len(x) != 32 for x in pub):
        raise ValueError('a public input is 32 bytes')
    pad = -len(proof) % 32
    word = lambda v: v.to_bytes(32, 'big')
    return selector() + word(0x40) + word(0x60 + len(proof) + pad) + word(len(proof)) + proof + bytes(pad) + word(len(pub)) + b''.join(pub)


def returndata(status, reason):
    """(reverted, return / revert data) of one (status, reason) pair; ValueError for a pair a deployed PLONK set never reports."""
    o = C.create_string_buffer(RETURNDATA_STRIDE); n = C.c_uint32(0); rev = C.c_uint8(0)
    if lib().zkv_plonk_set_eth_call_returndata(status, reason, o, C.byref(n), C.byref(rev)) != 0:
        raise ValueError('a deployed PLONK set never reports status %d with reason %d' % (status, reason))
    return bool(rev.value), o.raw[:n.value]


class PlonkDeployedSet(plonk_set.PlonkVerifierSet):
    """keys: list of (vk_bytes, address): PlonkVerifierSet's key bytes and the contract's 20-byte address.  Every PlonkVerifierSet call
    works on it."""

    def __init__(self, keys, device=0):
        keys = [(bytes(vk), bytes(addr)) for vk, addr in keys]
        if not 1 <= len(keys) <= plonk_set.MAX_KEYS:
            raise ValueError('a PLONK key set holds 1 .. %d keys' % plonk_set.MAX_KEYS)
        if any(len(addr) != 20 for _, addr in keys):
            raise ValueError('an address is 20 bytes')
        self._L = lib()
        k = len(keys)
        self._vk = [vk for vk, _ in keys]                            # alive for the call; the library copies them
        self._h = self._L.zkv_plonk_set_create_deployed(k, (C.c_char_p * k)(*self._vk), (C.c_size_t * k)(*[len(v) for v in self._vk]),
                                                        b''.join(addr for _, addr in keys), device)
        if not self._h:
            raise ValueError('zkv_plonk_set_create_deployed rejected the arguments (a key zkv_plonk_set_create refuses, or two keys with one address)')
        self.shapes = [self.key_shape(j) for j in range(k)]
        self.addresses = [addr for _, addr in keys]

    selector = staticmethod(selector)
    encode_call = staticmethod(encode_call)
    eth_call_returndata = staticmethod(returndata)

    def eth_call_batch(self, to, calls, offsets=None):
        """to: one 20-byte address per request; calls: one calldata byte string per request -- or, with `offsets` (n + 1 byte offsets), one
        blob that the offsets cut, which may then run backwards or past its end (offsets[n]).
        -> (reverted uint8[n], [return / revert data], status uint8[n], reason uint8[n])."""
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
        rev = np.zeros(n, dtype=np.uint8); st = np.zeros(n, dtype=np.uint8); rs = np.zeros(n, dtype=np.uint8)
        ret = np.zeros((n, RETURNDATA_STRIDE), dtype=np.uint8); ln = np.zeros(n, dtype=np.uint32)
        _lib.check(self._L.zkv_plonk_set_eth_call_batch(self._h, n, b''.join(bytes(a) for a in to) + b'\0', blob, off.ctypes.data, rev.ctypes.data, ret.ctypes.data,
                                                        ln.ctypes.data, st.ctypes.data, rs.ctypes.data), 'zkv_plonk_set_eth_call_batch')
        return rev, [ret[i, :ln[i]].tobytes() for i in range(n)], st, rs

    def eth_call_batch_dev(self, n, d_to, d_calldata, d_calldata_off, calldata_bytes, d_status, d_reason=0, d_key=0, stream=0):
        """Device-resident batch: device pointers to n x 20 address bytes, the calldata, its n + 1 uint64 offsets, n status bytes and
        (optional) n reason bytes and n uint32 resolved keys; enqueued on `stream` (0 = the context's stream)."""
        _lib.check(self._L.zkv_plonk_set_eth_call_batch_dev(self._h, n, d_to, d_calldata, d_calldata_off, calldata_bytes, d_status, d_reason or None,
                                                            d_key or None, stream or None), 'zkv_plonk_set_eth_call_batch_dev')

    def last_call_counts(self):
        """[placed, no contract, bad calldata, reason 1, reason 2, reason 3, reason 4, reason 5] of the most recent eth_call batch."""
        out = (C.c_uint64 * 8)()
        _lib.check(self._L.zkv_plonk_set_last_call_counts(self._h, out), 'zkv_plonk_set_last_call_counts')
        return list(out)

    def last_wire_ms(self):
        """Device time of the decode and point kernels of the most recent eth_call batch."""
        f = C.c_float(0)
        _lib.check(_lib.lib().zkv_ctx_last_wire_ms(self._h, C.byref(f)), 'zkv_ctx_last_wire_ms')
        return f.value

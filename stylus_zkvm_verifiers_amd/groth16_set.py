"""Groth16 key sets (include/zkv_groth16_set.h): many verification keys behind one context, the key chosen per proof -- the batch form
of `Groth16Verifier::verify_proof_with_key(vm_type, &vk, ...)` (common/groth16.rs:23-49) with proof i verified against key keys[i]."""
import ctypes as C

import numpy as np

from . import _lib
from .errors import VM_RISC0, VM_SP1
from .groth16 import MAX_IC

VM_GROTH16_SET = 7      # ZKV_VM_GROTH16_SET
MAX_KEYS = 1024         # ZKV_GROTH16_SET_MAX_KEYS

_P, _SZ, _U32P = C.c_void_p, C.c_size_t, C.c_void_p
# the set's own entry points (declared in include/zkv_groth16_set.h, not in zkv.h: _lib.SYMBOLS mirrors zkv.h alone)
SYMBOLS = {
    'zkv_groth16_set_create': (C.c_void_p, [_SZ, C.POINTER(C.c_char_p), C.POINTER(C.c_size_t), C.POINTER(C.c_int), C.c_int]),
    'zkv_groth16_set_size': (C.c_size_t, [_P]),
    'zkv_groth16_set_signal_stride': (C.c_size_t, [_P]),
    'zkv_groth16_set_key_n_ic': (C.c_int, [_P, _SZ]),
    'zkv_groth16_set_verify_batch': (C.c_int, [_P, _SZ, _U32P, _P, _P, _P]),
    'zkv_groth16_set_verify_batch_dev': (C.c_int, [_P, _SZ, _P, _P, _P, _P, _P]),
    'zkv_groth16_set_vk_x_batch': (C.c_int, [_P, _SZ, _U32P, _P, _P]),
}

_bound = None


def lib():
    """The library with the key-set symbols bound (AttributeError when one is not exported)."""
    global _bound
    L = _lib.lib()
    if _bound is not L:
        for name, (res, args) in SYMBOLS.items():
            fn = getattr(L, name)
            fn.restype = res
            fn.argtypes = args
        _bound = L
    return L


class Groth16VerifierSet:
    """keys: list of (vk_bytes, n_ic, vm_type) with vk_bytes in Groth16Verifier's layout (groth16.vk_words)."""

    def __init__(self, keys, device=0):
        keys = list(keys)
        if not 1 <= len(keys) <= MAX_KEYS:
            raise ValueError('a key set holds 1 .. %d keys' % MAX_KEYS)
        for vk, n_ic, vm in keys:
            if not 1 <= n_ic <= MAX_IC:
                raise ValueError('n_ic must be 1 .. %d' % MAX_IC)
            if len(vk) != 448 + 64 * n_ic:
                raise ValueError('verification key must be 448 + 64 * n_ic bytes')
            if vm not in (VM_RISC0, VM_SP1):
                raise ValueError('vm_type must be VM_RISC0 or VM_SP1')
        self._L = lib()
        k = len(keys)
        self._vk = [bytes(vk) for vk, _, _ in keys]                  # alive for the call; the library copies them
        words = (C.c_char_p * k)(*self._vk)
        n_ic = (C.c_size_t * k)(*[n for _, n, _ in keys])
        vms = (C.c_int * k)(*[vm for _, _, vm in keys])
        self._h = self._L.zkv_groth16_set_create(k, words, n_ic, vms, device)
        if not self._h:
            raise ValueError('zkv_groth16_set_create rejected the arguments')
        self.n_ic = [n for _, n, _ in keys]

    def close(self):
        if getattr(self, '_h', None):
            self._L.zkv_ctx_destroy(self._h)
            self._h = None

    __del__ = close

    def size(self):
        return self._L.zkv_groth16_set_size(self._h)

    def signal_stride(self):
        """Bytes per proof in the signal rows: 32 * (max n_ic - 1)."""
        return self._L.zkv_groth16_set_signal_stride(self._h)

    def key_n_ic(self, key):
        r = self._L.zkv_groth16_set_key_n_ic(self._h, key)
        if r < 0:
            raise IndexError('key %d is not in the set' % key)
        return r

    def _keys(self, keys):
        a = np.asarray(keys, dtype=np.int64)
        if a.ndim != 1 or (a < 0).any():
            raise ValueError('keys must be one non-negative key index per proof')
        return np.ascontiguousarray(np.minimum(a, 0xFFFFFFFF).astype(np.uint32))

    def _proofs(self, proofs, n):
        if isinstance(proofs, np.ndarray):
            if proofs.dtype != np.uint8 or proofs.shape != (n, 256):
                raise ValueError('proofs must be a uint8 array of shape (n, 256)')
            return np.ascontiguousarray(proofs)
        if len(proofs) != n or any(len(p) != 256 for p in proofs):
            raise ValueError('one 256-byte proof per key index')
        return np.frombuffer(b''.join(bytes(p) for p in proofs), dtype=np.uint8).reshape(n, 256) if n else np.zeros((0, 256), np.uint8)

    def _signals(self, signals, n):
        """Rows of signal_stride() bytes; a short row (list form, or an array of fewer words) is padded with zero words."""
        k = self.signal_stride() // 32
        out = np.zeros((max(n, 1), max(k, 1), 32), dtype=np.uint8)
        if isinstance(signals, np.ndarray):
            if signals.dtype != np.uint8 or signals.ndim != 3 or signals.shape[0] != n or signals.shape[2] != 32 or signals.shape[1] > k:
                raise ValueError('signals must be a uint8 array of shape (n, <= %d, 32)' % k)
            if signals.shape[1]:
                out[:n, :signals.shape[1]] = signals
            return out
        if len(signals) != n:
            raise ValueError('signals has %d rows for a batch of %d proofs' % (len(signals), n))
        for i, row in enumerate(signals):
            if len(row) > k:
                raise ValueError('row %d has more than %d signals' % (i, k))
            for b, s in enumerate(row):
                if len(s) != 32:
                    raise ValueError('a signal is 32 bytes')
                out[i, b] = np.frombuffer(bytes(s), dtype=np.uint8)
        return out

    def verify_batch(self, keys, proofs, signals):
        """keys: key index per proof (numpy or list; an index past the set gives False); proofs: n x 256 bytes; signals: per proof the
        key's n_ic - 1 32-byte big-endian values (rows may be padded to signal_stride() bytes) -> bool array."""
        ka = self._keys(keys)
        n = len(ka)
        pa, sa = self._proofs(proofs, n), self._signals(signals, n)
        out = np.zeros(max(n, 1), dtype=np.uint8)
        _lib.check(self._L.zkv_groth16_set_verify_batch(self._h, n, ka.ctypes.data if n else None, pa.ctypes.data if n else None,
                                                        sa.ctypes.data, out.ctypes.data), 'zkv_groth16_set_verify_batch')
        return out[:n].astype(bool)

    def verify_batch_dev(self, n, d_keys, d_proofs, d_signals, d_verified, stream=0):
        """Device-resident batch: device pointers to n uint32 key indices, n x 256 proof bytes, n x signal_stride() signal bytes and
        n verdict bytes (1 / 0); enqueued on `stream` (0 = the context's stream)."""
        _lib.check(self._L.zkv_groth16_set_verify_batch_dev(self._h, n, d_keys, d_proofs, d_signals or None, d_verified, stream or None),
                   'zkv_groth16_set_verify_batch_dev')

    def vk_x_batch(self, keys, signals):
        """compute_vk_x (groth16.rs:51-58) of each row under its key -> list of 64-byte affine points ((0, 0) = infinity)."""
        ka = self._keys(keys)
        n = len(ka)
        sa = self._signals(signals, n)
        out = np.zeros(max(64 * n, 1), dtype=np.uint8)
        _lib.check(self._L.zkv_groth16_set_vk_x_batch(self._h, n, ka.ctypes.data if n else None, sa.ctypes.data, out.ctypes.data),
                   'zkv_groth16_set_vk_x_batch')
        return [out[64 * i:64 * i + 64].tobytes() for i in range(n)]

    def synchronize(self):
        _lib.check(self._L.zkv_ctx_synchronize(self._h), 'zkv_ctx_synchronize')

    def reserve(self, n):
        """Device set-up (every key's tables) and buffers for batches of up to n proofs, ahead of the first batch (optional)."""
        _lib.check(self._L.zkv_ctx_reserve(self._h, n), 'zkv_ctx_reserve')

    def set_aggregate_check(self, enable=True, seed=None, sub_batch=None):
        """Opt-in aggregate check (include/zkv_groth16_set.h): proofs of capable keys are checked in key-uniform sub-batches of 16 ... 256
        (None: chosen by the failure rate seen) when a call places at least ZKV_AGG_MIN proofs; the verdicts stay the per-proof ones."""
        if sub_batch is not None and sub_batch not in (16, 32, 64, 128, 256):
            raise ValueError('sub_batch must be None, 16, 32, 64, 128 or 256')
        from .risc0 import _set_aggregate_check
        _set_aggregate_check(self._L, self._h, enable, seed, sub_batch)

    def aggregate_counters(self):
        """(sub-batches checked in aggregate, sub-batches that failed and were verified proof by proof)."""
        from .risc0 import _aggregate_counters
        return _aggregate_counters(self._L, self._h)

    def set_lanes_per_proof(self, lanes):
        """Miller-loop mapping (0 = automatic, 2, 16, 64, 128), kept even where it pads key groups more than 1.25x.  Same results."""
        _lib.check(self._L.zkv_ctx_set_lanes_per_proof(self._h, lanes), 'zkv_ctx_set_lanes_per_proof')

    def last_stage_ms(self):
        out = (C.c_float * 5)()
        _lib.check(self._L.zkv_ctx_last_stage_ms(self._h, out), 'zkv_ctx_last_stage_ms')
        return list(out)

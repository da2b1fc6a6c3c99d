"""PLONK key sets (include/zkv_plonk_set.h): many gnark BN254 PLONK keys behind one context, the key chosen per proof -- the batch form of
PlonkVerifier with proof i verified against key keys[i].  PARITY UNPINNED BY CONSTRUCTION: the reference holds no PLONK code; verdicts
follow gnark's published verifier as restated in oracle/plonk_model.py."""
import ctypes as C

import numpy as np

from . import _lib

VM_PLONK_SET = 10       # ZKV_VM_PLONK_SET
MAX_KEYS = 256          # ZKV_PLONK_SET_MAX_KEYS

_P, _SZ = C.c_void_p, C.c_size_t
# the set's own entry points (declared in include/zkv_plonk_set.h, not in zkv.h: _lib.SYMBOLS mirrors zkv.h alone)
SYMBOLS = {
    'zkv_plonk_set_create': (C.c_void_p, [_SZ, C.POINTER(C.c_char_p), C.POINTER(C.c_size_t), C.c_int]),
    'zkv_plonk_set_size': (C.c_size_t, [_P]),
    'zkv_plonk_set_proof_stride': (C.c_size_t, [_P]),
    'zkv_plonk_set_input_stride': (C.c_size_t, [_P]),
    'zkv_plonk_set_key_shape': (C.c_int, [_P, _SZ, C.POINTER(C.c_size_t), C.POINTER(C.c_size_t), C.POINTER(C.c_size_t)]),
    'zkv_plonk_set_verify_batch': (C.c_int, [_P, _SZ, _P, _P, _P, _P]),
    'zkv_plonk_set_verify_batch_dev': (C.c_int, [_P, _SZ, _P, _P, _P, _P, _P]),
}

_bound = None


def lib():
    """The library with the PLONK-set symbols bound (AttributeError when one is not exported)."""
    global _bound
    L = _lib.lib()
    if _bound is not L:
        for name, (res, args) in SYMBOLS.items():
            fn = getattr(L, name)
            fn.restype = res
            fn.argtypes = args
        _bound = L
    return L


class PlonkVerifierSet:
    """keys: list of key bytes, each in PlonkVerifier's layout (plonk_keys.vk_bytes)."""

    def __init__(self, keys, device=0):
        keys = [bytes(vk) for vk in keys]
        if not 1 <= len(keys) <= MAX_KEYS:
            raise ValueError('a PLONK key set holds 1 .. %d keys' % MAX_KEYS)
        self._L = lib()
        k = len(keys)
        self._vk = keys                                              # alive for the call; the library copies them
        self._h = self._L.zkv_plonk_set_create(k, (C.c_char_p * k)(*keys), (C.c_size_t * k)(*[len(v) for v in keys]), device)
        if not self._h:
            raise ValueError('zkv_plonk_set_create rejected a key (length, n_c > 1, nb_public > 128 or an oversized header word)')
        self.shapes = [self.key_shape(j) for j in range(k)]

    def close(self):
        if getattr(self, '_h', None):
            self._L.zkv_ctx_destroy(self._h)
            self._h = None

    __del__ = close

    def size(self):
        return self._L.zkv_plonk_set_size(self._h)

    def proof_stride(self):
        """Bytes per proof row: 32 (24 + 3 max n_c)."""
        return self._L.zkv_plonk_set_proof_stride(self._h)

    def input_stride(self):
        """Bytes per public-input row: 32 max nb_public (may be 0)."""
        return self._L.zkv_plonk_set_input_stride(self._h)

    def key_shape(self, key):
        """(nb_public, n_c, proof_bytes) of key `key`."""
        a, b, c = C.c_size_t(), C.c_size_t(), C.c_size_t()
        r = self._L.zkv_plonk_set_key_shape(self._h, key, C.byref(a), C.byref(b), C.byref(c))
        if r < 0:
            raise IndexError('key %d is not in the set' % key)
        return a.value, b.value, c.value

    @staticmethod
    def _keys(keys):
        a = np.asarray(keys, dtype=np.int64)
        if a.ndim != 1 or (a < 0).any():
            raise ValueError('keys must be one non-negative key index per proof')
        return np.ascontiguousarray(np.minimum(a, 0xFFFFFFFF).astype(np.uint32))

    def _proofs(self, proofs, n):
        """Rows of proof_stride() bytes; a shorter proof (list form, or an array of fewer columns) is padded with zero bytes."""
        ps = self.proof_stride()
        if isinstance(proofs, np.ndarray):
            if proofs.dtype != np.uint8 or proofs.ndim != 2 or proofs.shape[0] != n or proofs.shape[1] > ps:
                raise ValueError('proofs must be a uint8 array of shape (n, <= %d)' % ps)
            if proofs.shape[1] == ps:
                return np.ascontiguousarray(proofs)
            out = np.zeros((n, ps), np.uint8)
            out[:, :proofs.shape[1]] = proofs
            return out
        if len(proofs) != n:
            raise ValueError('proofs has %d rows for a batch of %d proofs' % (len(proofs), n))
        out = np.zeros((n, ps), np.uint8)
        for i, p in enumerate(proofs):
            p = bytes(p)
            if len(p) > ps:
                raise ValueError('proof %d is longer than %d bytes' % (i, ps))
            out[i, :len(p)] = np.frombuffer(p, np.uint8)
        return out

    def _inputs(self, public_inputs, n):
        """Rows of input_stride() bytes; a short row (list form, or an array of fewer words) is padded with zero words."""
        k = self.input_stride() // 32
        out = np.zeros((max(n, 1), max(k, 1), 32), dtype=np.uint8)
        if isinstance(public_inputs, np.ndarray):
            a = public_inputs
            if a.dtype != np.uint8 or a.ndim != 3 or a.shape[0] != n or a.shape[2] != 32 or a.shape[1] > k:
                raise ValueError('public_inputs must be a uint8 array of shape (n, <= %d, 32)' % k)
            if a.shape[1]:
                out[:n, :a.shape[1]] = a
            return out
        if len(public_inputs) != n:
            raise ValueError('public_inputs has %d rows for a batch of %d proofs' % (len(public_inputs), n))
        for i, row in enumerate(public_inputs):
            if len(row) > k:
                raise ValueError('row %d has more than %d public inputs' % (i, k))
            for b, x in enumerate(row):
                x = x.to_bytes(32, 'big') if isinstance(x, int) else bytes(x)
                if len(x) != 32:
                    raise ValueError('a public input is 32 bytes')
                out[i, b] = np.frombuffer(x, dtype=np.uint8)
        return out

    def verify_batch(self, keys, proofs, public_inputs):
        """keys: key index per proof (an index past the set gives 0); proofs: per proof its key's proof bytes (rows may be padded to
        proof_stride()); public_inputs: per proof its key's nb_public 32-byte big-endian values (rows may be padded to input_stride()
        bytes) -> uint8 array of verdicts (1 / 0)."""
        ka = self._keys(keys)
        n = len(ka)
        pa, ia = self._proofs(proofs, n), self._inputs(public_inputs, n)
        out = np.zeros(max(n, 1), dtype=np.uint8)
        _lib.check(self._L.zkv_plonk_set_verify_batch(self._h, n, ka.ctypes.data if n else None, pa.ctypes.data if n else None,
                                                      ia.ctypes.data, out.ctypes.data), 'zkv_plonk_set_verify_batch')
        return out[:n]

    def verify_batch_dev(self, n, d_keys, d_proofs, d_public_inputs, d_verified, stream=0):
        """Device-resident batch: device pointers to n uint32 key indices, n x proof_stride() proof bytes, n x input_stride() input bytes
        (may be 0 when the stride is 0) and n verdict bytes (1 / 0); enqueued on `stream` (0 = the context's stream)."""
        _lib.check(self._L.zkv_plonk_set_verify_batch_dev(self._h, n, d_keys, d_proofs, d_public_inputs or None, d_verified, stream or None),
                   'zkv_plonk_set_verify_batch_dev')

    def synchronize(self):
        _lib.check(self._L.zkv_ctx_synchronize(self._h), 'zkv_ctx_synchronize')

    def reserve(self, n):
        """Device set-up (every key's tables, about 24 MB per key) and buffers for batches of up to n proofs, ahead of the first batch."""
        _lib.check(self._L.zkv_ctx_reserve(self._h, n), 'zkv_ctx_reserve')

    def set_aggregate_check(self, enable=True, seed=None, sub_batch=None):
        """Opt-in aggregate check (include/zkv_plonk_set_agg.h): the pairing equation is checked per sub-batch of 16 ... 256 slots (None:
        chosen by the failure rate seen), sub-batches running across the keys of one SRS class, when the mapping is automatic and a call
        places at least ZKV_AGG_MIN proofs; the verdicts stay the per-proof ones."""
        if sub_batch is not None and sub_batch not in (16, 32, 64, 128, 256):
            raise ValueError('sub_batch must be None, 16, 32, 64, 128 or 256')
        from .risc0 import _set_aggregate_check
        _set_aggregate_check(self._L, self._h, enable, seed, sub_batch)

    def aggregate_counters(self):
        """(sub-batches checked in aggregate, sub-batches that failed and were verified proof by proof)."""
        from .risc0 import _aggregate_counters
        return _aggregate_counters(self._L, self._h)

    def srs_classes(self):
        """(class of every key, number of classes): keys with equal [1]_2 | [tau]_2 bytes are one SRS class and share sub-batches."""
        from . import plonk_set_agg
        return plonk_set_agg.srs_classes(self._h, self.size())

    def set_lanes_per_proof(self, lanes):
        """Miller-loop mapping (0 = automatic, 2, 16, 64; 128 runs as 64: PLONK has no variable pair).  Same results."""
        _lib.check(self._L.zkv_ctx_set_lanes_per_proof(self._h, lanes), 'zkv_ctx_set_lanes_per_proof')

    def last_stage_ms(self):
        out = (C.c_float * 5)()
        _lib.check(self._L.zkv_ctx_last_stage_ms(self._h, out), 'zkv_ctx_last_stage_ms')
        return list(out)

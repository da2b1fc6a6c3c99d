"""PLONK core for any gnark BN254 verifying key (include/zkv_plonk_keys.h): up to 128 public inputs, with or without one BSB22
commitment, a verdict per proof.  The PLONK counterpart of Groth16Verifier.  PARITY UNPINNED BY CONSTRUCTION: the reference holds no
PLONK code; verdicts follow gnark's published verifier as restated in oracle/plonk_model.py."""
import ctypes as C

import numpy as np

from . import _lib
from .risc0 import _aggregate_counters, _set_aggregate_check

VM_PLONK = 9                    # ZKV_VM_PLONK
MAX_PUBLIC = 128                # ZKV_PLONK_MAX_PUBLIC

_P, _SZ = C.c_void_p, C.c_size_t
# the entry points of include/zkv_plonk_keys.h (not in zkv.h: _lib.SYMBOLS mirrors zkv.h alone)
SYMBOLS = {
    'zkv_plonk_ctx_create': (C.c_void_p, [C.c_char_p, _SZ, C.c_int]),
    'zkv_plonk_key_shape': (C.c_int, [_P, C.POINTER(C.c_size_t), C.POINTER(C.c_size_t), C.POINTER(C.c_size_t)]),
    'zkv_plonk_verify_batch': (C.c_int, [_P, _SZ, _P, _P, _P]),
    'zkv_plonk_verify_batch_dev': (C.c_int, [_P, _SZ, _P, _P, _P, _P]),
}

_bound = None


def lib():
    """The library with the PLONK-key symbols bound (AttributeError when one is not exported)."""
    global _bound
    L = _lib.lib()
    if _bound is not L:
        for name, (res, args) in SYMBOLS.items():
            fn = getattr(L, name)
            fn.restype = res
            fn.argtypes = args
        _bound = L
    return L


def vk_bytes(size, size_inv, generator, coset_shift, nb_public, s1, s2, s3, ql, qr, qm, qo, qk, g2, g2_tau, qcp=None, cci=0):
    """Serialise a key given as integers: G1 points as (x, y) ((0, 0) = infinity); g2 / g2_tau as ((x_im, x_re), (y_im, y_re)) in
    EIP-197 order; qcp = None for a circuit without BSB22 commitment (n_c = 0), else the commitment's selector point."""
    be = lambda v: int(v).to_bytes(32, 'big')
    out = b''.join(be(v) for v in (size, size_inv, generator, coset_shift, nb_public, 0 if qcp is None else 1, cci))
    for p in (s1, s2, s3, ql, qr, qm, qo, qk) + (() if qcp is None else (qcp,)):
        out += be(p[0]) + be(p[1])
    for (x0, x1), (y0, y1) in (g2, g2_tau):
        out += be(x0) + be(x1) + be(y0) + be(y1)
    return out


class PlonkVerifier:
    def __init__(self, vk_bytes, device=0):
        self._L = lib()
        self._h = self._L.zkv_plonk_ctx_create(bytes(vk_bytes), len(vk_bytes), device)
        if not self._h:
            raise ValueError('zkv_plonk_ctx_create rejected the key (length, n_c > 1, nb_public > %d or an oversized header word)' % MAX_PUBLIC)
        a, b, c = C.c_size_t(), C.c_size_t(), C.c_size_t()
        _lib.check(self._L.zkv_plonk_key_shape(self._h, C.byref(a), C.byref(b), C.byref(c)), 'zkv_plonk_key_shape')
        self.nb_public, self.n_commitments, self.proof_bytes = a.value, b.value, c.value

    def close(self):
        if getattr(self, '_h', None):
            self._L.zkv_ctx_destroy(self._h)
            self._h = None

    __del__ = close

    def _proof_blob(self, proofs):
        pb = self.proof_bytes
        if isinstance(proofs, np.ndarray):
            if proofs.dtype != np.uint8 or proofs.ndim != 2 or proofs.shape[1] != pb:
                raise ValueError('proofs must be a uint8 array of shape (n, %d)' % pb)
            return len(proofs), np.ascontiguousarray(proofs)
        for p in proofs:
            if len(p) != pb:
                raise ValueError('a proof is %d bytes for this key' % pb)
        return len(proofs), b''.join(bytes(p) for p in proofs) + b'\0'

    def _input_blob(self, public_inputs, n):
        k = self.nb_public
        if isinstance(public_inputs, np.ndarray):
            if public_inputs.dtype != np.uint8 or public_inputs.ndim != 3 or public_inputs.shape[1:] != (k, 32):
                raise ValueError('public_inputs must be a uint8 array of shape (n, %d, 32)' % k)
            m = len(public_inputs)
            blob = np.ascontiguousarray(public_inputs) if public_inputs.size else np.zeros(1, np.uint8)
        else:
            m = len(public_inputs)
            for s in public_inputs:
                if len(s) != k or any(len(x) != 32 for x in s):
                    raise ValueError('expected %d public inputs of 32 bytes per proof' % k)
            blob = b''.join(b''.join(bytes(x) for x in s) for s in public_inputs) + b'\0'
        if m != n:
            raise ValueError('public_inputs has %d entries for a batch of %d proofs' % (m, n))
        return blob

    @staticmethod
    def _ptr(blob):
        return blob.ctypes.data if isinstance(blob, np.ndarray) else blob

    def verify_batch(self, proofs, public_inputs):
        """proofs: list of proof_bytes-byte proofs or uint8 array (n, proof_bytes); public_inputs: list of nb_public 32-byte big-endian
        values per proof or uint8 array (n, nb_public, 32) -> uint8 array of verdicts (1 / 0)."""
        n, pb = self._proof_blob(proofs)
        ib = self._input_blob(public_inputs, n)
        out = np.zeros(max(n, 1), dtype=np.uint8)
        _lib.check(self._L.zkv_plonk_verify_batch(self._h, n, self._ptr(pb), self._ptr(ib), out.ctypes.data), 'zkv_plonk_verify_batch')
        return out[:n]

    def verify_proof(self, proof, public_inputs):
        """One proof; public_inputs: nb_public 32-byte big-endian values or ints."""
        pub = [x.to_bytes(32, 'big') if isinstance(x, int) else bytes(x) for x in public_inputs]
        return bool(self.verify_batch([bytes(proof)], [pub])[0])

    def verify_batch_dev(self, n, d_proofs, d_public_inputs, d_verified, stream=0):
        """Device-resident batch (zkv_plonk_verify_batch_dev): device pointers to n x proof_bytes proof bytes, n x nb_public x 32 input
        bytes and n verdict bytes (1 / 0); asynchronous on `stream` (0 = the context's stream)."""
        _lib.check(self._L.zkv_plonk_verify_batch_dev(self._h, n, d_proofs, d_public_inputs or None, d_verified, stream or None),
                   'zkv_plonk_verify_batch_dev')

    def synchronize(self):
        _lib.check(self._L.zkv_ctx_synchronize(self._h), 'zkv_ctx_synchronize')

    def reserve(self, n):
        """Device set-up and per-chunk buffers for batches of up to n proofs, ahead of the first batch (optional)."""
        _lib.check(self._L.zkv_ctx_reserve(self._h, n), 'zkv_ctx_reserve')

    def set_lanes_per_proof(self, lanes):
        """Kernel mapping of the pairing stages (0 = automatic, 2, 16, 64, 128; include/zkv.h).  Same results."""
        _lib.check(self._L.zkv_ctx_set_lanes_per_proof(self._h, lanes), 'zkv_ctx_set_lanes_per_proof')

    def set_aggregate_check(self, enable=True, seed=None, sub_batch=None):
        """Opt-in: share the pairing check among sub-batches of a large chunk (include/zkv.h); the answers stay the deterministic ones."""
        _set_aggregate_check(self._L, self._h, enable, seed, sub_batch)

    def aggregate_counters(self):
        return _aggregate_counters(self._L, self._h)

    def last_stage_ms(self):
        out = (C.c_float * 5)()
        _lib.check(self._L.zkv_ctx_last_stage_ms(self._h, out), 'zkv_ctx_last_stage_ms')
        return list(out)

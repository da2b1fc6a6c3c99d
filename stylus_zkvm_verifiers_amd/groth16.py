"""Host-side mirror of `Groth16Verifier::verify_proof_with_key` (/root/reference/contracts/src/common/groth16.rs:23-49) for an
arbitrary verification key (`VerificationKey`, common/types.rs:17-23)."""
import ctypes as C

import numpy as np

from . import _lib
from .errors import VM_RISC0, VM_SP1
from .risc0 import _aggregate_counters, _set_aggregate_check

MAX_IC = 129        # ZKV_GROTH16_MAX_IC (include/zkv.h): up to 128 per-proof signals; keys with n_ic > 6 take the long-key path


def vk_words(alpha1, beta2, gamma2, delta2, ic):
    """Serialise a key given as integers in the reference's layout: alpha1 (x, y); beta2/gamma2/delta2 ((x0, x1), (y0, y1)) with
    index 0 = imaginary, 1 = real; ic list of (x, y)."""
    be = lambda v: int(v).to_bytes(32, 'big')
    out = be(alpha1[0]) + be(alpha1[1])
    for q in (beta2, gamma2, delta2):
        out += be(q[0][0]) + be(q[0][1]) + be(q[1][0]) + be(q[1][1])
    for x, y in ic:
        out += be(x) + be(y)
    return out


class Groth16Verifier:
    def __init__(self, vk_bytes, n_ic, vm_type=VM_SP1, device=0):
        if not 1 <= n_ic <= MAX_IC:
            raise ValueError('n_ic must be 1 .. %d' % MAX_IC)
        if len(vk_bytes) != 448 + 64 * n_ic:
            raise ValueError('verification key must be 448 + 64 * n_ic bytes')
        self._L = _lib.lib()
        self.n_ic = n_ic
        self._h = self._L.zkv_groth16_ctx_create(bytes(vk_bytes), n_ic, vm_type, device)
        if not self._h:
            raise ValueError('zkv_groth16_ctx_create rejected the arguments')

    def close(self):
        if getattr(self, '_h', None):
            self._L.zkv_ctx_destroy(self._h)
            self._h = None

    __del__ = close

    def _proof_blob(self, proofs):
        if isinstance(proofs, np.ndarray):
            if proofs.dtype != np.uint8 or proofs.ndim != 2 or proofs.shape[1] != 256:
                raise ValueError('proofs must be a uint8 array of shape (n, 256)')
            return len(proofs), np.ascontiguousarray(proofs)
        for p in proofs:
            if len(p) != 256:
                raise ValueError('a proof is 8 x 32 bytes')
        return len(proofs), b''.join(bytes(p) for p in proofs) + b'\0'

    def _signal_blob(self, signals, n=None):
        k = self.n_ic - 1
        if isinstance(signals, np.ndarray):
            if signals.dtype != np.uint8 or signals.ndim != 3 or signals.shape[1:] != (k, 32):
                raise ValueError('signals must be a uint8 array of shape (n, %d, 32)' % k)
            m = len(signals)
            blob = np.ascontiguousarray(signals) if signals.size else np.zeros(1, np.uint8)
        else:
            m = len(signals)
            for s in signals:
                if len(s) != k:
                    raise ValueError('expected %d signals per proof' % k)   # groth16.rs:32 length check
            blob = b''.join(b''.join(bytes(x) for x in s) for s in signals) + b'\0'
        if n is not None and m != n:
            raise ValueError('signals has %d entries for a batch of %d proofs' % (m, n))
        return m, blob

    @staticmethod
    def _ptr(blob):
        return blob.ctypes.data if isinstance(blob, np.ndarray) else blob

    def verify_batch(self, proofs, signals):
        """proofs: list of 256-byte (a, b, c) word blocks or uint8 array (n, 256); signals: list of lists of n_ic - 1 32-byte big-endian
        values or uint8 array (n, n_ic - 1, 32) -> bool array."""
        n, pb = self._proof_blob(proofs)
        _, sb = self._signal_blob(signals, n)
        out = np.zeros(max(n, 1), dtype=np.uint8)
        _lib.check(self._L.zkv_groth16_verify_batch(self._h, n, self._ptr(pb), self._ptr(sb), out.ctypes.data), 'zkv_groth16_verify_batch')
        return out[:n].astype(bool)

    def verify_batch_dev(self, n, d_proofs, d_signals, d_verified, stream=0):
        """Device-resident batch (zkv_groth16_verify_batch_dev): device pointers to n x 256 proof bytes, n x (n_ic - 1) x 32 signal bytes
        and n verdict bytes (1 / 0); asynchronous on `stream` (0 = the context's stream)."""
        _lib.check(self._L.zkv_groth16_verify_batch_dev(self._h, n, d_proofs, d_signals or None, d_verified, stream or None),
                   'zkv_groth16_verify_batch_dev')

    def synchronize(self):
        _lib.check(self._L.zkv_ctx_synchronize(self._h), 'zkv_ctx_synchronize')

    def reserve(self, n):
        """Device set-up and per-chunk buffers for batches of up to n proofs, ahead of the first batch (optional)."""
        _lib.check(self._L.zkv_ctx_reserve(self._h, n), 'zkv_ctx_reserve')

    def set_lanes_per_proof(self, lanes):
        """Kernel mapping (0 = automatic, 2, 16, 64, 128; include/zkv.h); on a long key it also fixes the lanes per proof of the vk_x
        stage (2 -> 1, 16 -> 16, 64 / 128 -> 64).  Same results."""
        _lib.check(self._L.zkv_ctx_set_lanes_per_proof(self._h, lanes), 'zkv_ctx_set_lanes_per_proof')

    def last_stage_ms(self):
        out = (C.c_float * 5)()
        _lib.check(self._L.zkv_ctx_last_stage_ms(self._h, out), 'zkv_ctx_last_stage_ms')
        return list(out)

    def set_aggregate_check(self, enable=True, seed=None, sub_batch=None):
        """Opt-in: share the pairing check among sub-batches of a large chunk (include/zkv.h); the answers stay the deterministic ones."""
        _set_aggregate_check(self._L, self._h, enable, seed, sub_batch)

    def aggregate_counters(self):
        return _aggregate_counters(self._L, self._h)

    def vk_x_batch(self, signals):
        """Groth16Verifier::compute_vk_x (common/groth16.rs:51-58): signals = list of n_ic - 1 32-byte big-endian values per proof
        (each < R) or uint8 array (n, n_ic - 1, 32); returns the 64-byte affine vk_x per proof ((0,0) = infinity)."""
        n, sb = self._signal_blob(signals)
        out = np.zeros(max(64 * n, 1), dtype=np.uint8)
        _lib.check(self._L.zkv_ctx_vk_x_batch(self._h, n, self._ptr(sb), out.ctypes.data), 'zkv_ctx_vk_x_batch')
        return [out[64 * i:64 * i + 64].tobytes() for i in range(n)]

    def verify_proof_with_key(self, a, b, c, public_signals):
        """Single call with the reference's argument shapes: a [x, y], b [[x0, x1], [y0, y1]], c [x, y], signals as ints."""
        be = lambda v: int(v).to_bytes(32, 'big')
        proof = b''.join(be(v) for v in (a[0], a[1], b[0][0], b[0][1], b[1][0], b[1][1], c[0], c[1]))
        if len(public_signals) + 1 != self.n_ic or any(int(s) >= (1 << 256) for s in public_signals):
            return False
        return bool(self.verify_batch([proof], [[be(s) for s in public_signals]])[0])

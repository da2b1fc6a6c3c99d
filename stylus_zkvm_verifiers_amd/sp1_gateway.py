"""SP1 gateway (include/zkv_sp1_gateway.h): one context that sends every proof of a batch, on the device, to the SP1 verifier whose
4-byte selector begins it -- the built-in SP1 v5.0.0 Groth16 verifier and / or SP1 PLONK verifiers -- as SP1's on-chain gateway
forwards `ISp1Verifier::verify_proof`.  The gateway itself has no reference counterpart: ROUTE_NOT_FOUND and everything PLONK are
PARITY UNPINNED; a proof routed to the Groth16 route gets the pinned SP1 statuses."""
import ctypes as C

import numpy as np

from . import _lib
from .errors import STATUS_OK, VM_SP1, VerifierError
from .risc0 import _aggregate_counters, _blob, _cat32, _same_len, _set_aggregate_check

VM_SP1_GATEWAY = 8              # ZKV_VM_SP1_GATEWAY
VM_SP1_PLONK = 6                # ZKV_VM_SP1_PLONK
MAX_ROUTES = 8                  # ZKV_SP1_GATEWAY_MAX_ROUTES
STATUS_ROUTE_NOT_FOUND = 8      # ZKV_STATUS_ROUTE_NOT_FOUND

_P, _SZ = C.c_void_p, C.c_size_t
# the gateway's own entry points (declared in include/zkv_sp1_gateway.h, not in zkv.h: _lib.SYMBOLS mirrors zkv.h alone)
SYMBOLS = {
    'zkv_sp1_gateway_create': (C.c_void_p, [C.c_int, _SZ, C.POINTER(C.c_char_p), C.POINTER(C.c_size_t), C.c_char_p, C.c_int]),
    'zkv_sp1_gateway_route_count': (C.c_size_t, [_P]),
    'zkv_sp1_gateway_route': (C.c_int, [_P, _SZ, C.c_char_p, C.POINTER(C.c_int)]),
    'zkv_sp1_gateway_route_ctx': (C.c_void_p, [_P, _SZ]),
    'zkv_sp1_gateway_verify_proof': (C.c_int, [_P, C.c_char_p, C.c_char_p, _SZ, C.c_char_p, _SZ, C.POINTER(C.c_uint8), C.c_char_p]),
    'zkv_sp1_gateway_verify_batch': (C.c_int, [_P, _SZ, _P, _P, _P, _P, _P, _P, _P]),
    'zkv_sp1_gateway_verify_batch_dev': (C.c_int, [_P, _SZ, _P, _P, _SZ, _P, _P, C.c_uint64, _P, _P, _P]),
    'zkv_sp1_gateway_last_route_counts': (C.c_int, [_P, C.POINTER(C.c_uint64)]),
    'zkv_sp1_gateway_status_abi_encode': (C.c_int, [_P, C.c_uint8, C.c_char_p, C.c_char_p]),
}

_bound = None


class RouteNotFound(VerifierError):
    """No route has the proof's selector (SP1VerifierGateway's RouteNotFound(bytes4); unpinned).  `.received`: the proof's 4 bytes."""

    def __init__(self, received, revert):
        Exception.__init__(self, 'RouteNotFound(%s)' % received.hex())
        self.vm, self.status, self.received, self.expected, self.revert = VM_SP1, STATUS_ROUTE_NOT_FOUND, received, None, revert


def lib():
    """The library with the gateway symbols bound (AttributeError when one is not exported)."""
    global _bound
    L = _lib.lib()
    if _bound is not L:
        for name, (res, args) in SYMBOLS.items():
            fn = getattr(L, name)
            fn.restype = res
            fn.argtypes = args
        _bound = L
    return L


class Sp1Gateway:
    """groth16: include the built-in SP1 v5.0.0 Groth16 verifier as route 0; plonk: list of (vk_bytes, verifier_hash) in
    Sp1PlonkVerifier's layout, one route each, in order; groth16_keys: list of (vk_words, verifier_hash), Groth16 keys of other SP1
    releases in Groth16Verifier's layout with n_ic = 3 and SP1's sign convention (include/zkv_sp1_gateway_keys.h), one route each, in
    order, between the built-in route and the PLONK routes.  At most MAX_ROUTES routes, selectors pairwise distinct."""

    def __init__(self, groth16=True, plonk=(), device=0, groth16_keys=()):
        plonk = [(bytes(vk), bytes(h)) for vk, h in plonk]
        groth16_keys = [(bytes(vk), bytes(h)) for vk, h in groth16_keys]
        if not 1 <= int(bool(groth16)) + len(groth16_keys) + len(plonk) <= MAX_ROUTES:
            raise ValueError('a gateway holds 1 .. %d routes' % MAX_ROUTES)
        if any(len(h) != 32 for _, h in plonk):
            raise ValueError('verifier_hash must be 32 bytes')
        self._L = lib()
        k = len(plonk)
        self._vk = [vk for vk, _ in plonk]                          # alive for the call; the library copies them
        vks = (C.c_char_p * max(k, 1))(*self._vk)
        lens = (C.c_size_t * max(k, 1))(*[len(v) for v in self._vk])
        hashes = b''.join(h for _, h in plonk) + b'\0'
        if groth16_keys:
            from . import sp1_gateway_keys
            self._h = sp1_gateway_keys.create(groth16, groth16_keys, plonk, device)
        else:
            self._h = self._L.zkv_sp1_gateway_create(1 if groth16 else 0, k, vks, lens, hashes, device)
        if not self._h:
            raise ValueError('zkv_sp1_gateway_create rejected the routes (bad PLONK key, or two routes with one selector)')
        self._hashes = ([self.groth16_verifier_hash()] if groth16 else []) + [h for _, h in groth16_keys] + [h for _, h in plonk]

    def close(self):
        if getattr(self, '_h', None):
            self._L.zkv_ctx_destroy(self._h)
            self._h = None

    __del__ = close

    @staticmethod
    def groth16_verifier_hash():
        o = C.create_string_buffer(32); _lib.lib().zkv_sp1_verifier_hash(o); return o.raw

    def routes(self):
        """[(selector (4 bytes), vm (errors.VM_SP1 for Groth16, VM_SP1_PLONK), verifier hash (32 bytes))] in route order."""
        out = []
        for r in range(self._L.zkv_sp1_gateway_route_count(self._h)):
            sel = C.create_string_buffer(4); vm = C.c_int(-1)
            _lib.check(self._L.zkv_sp1_gateway_route(self._h, r, sel, C.byref(vm)), 'zkv_sp1_gateway_route')
            out.append((sel.raw, vm.value, self._hashes[r]))
        return out

    def verify_proof(self, program_vkey, public_values, proof_bytes):
        """Returns None or raises VerifierError (status ROUTE_NOT_FOUND: `received` holds the proof's selector)."""
        st = C.c_uint8(0); rv = C.create_string_buffer(4)
        _lib.check(self._L.zkv_sp1_gateway_verify_proof(self._h, bytes(program_vkey), bytes(public_values), len(public_values),
                                                        bytes(proof_bytes), len(proof_bytes), C.byref(st), rv), 'zkv_sp1_gateway_verify_proof')
        if st.value == STATUS_OK:
            return None
        if st.value == STATUS_ROUTE_NOT_FOUND:
            raise RouteNotFound(rv.raw, self.status_abi_encode(st.value, rv.raw))
        raise VerifierError(VM_SP1, st.value)           # (never SELECTOR_MISMATCH: the route picked has the proof's selector)

    def verify_batch(self, program_vkeys, public_values, proofs):
        """Ragged host buffers -> (status uint8[n], received selector uint8[n, 4])."""
        n = len(proofs)
        _same_len(n, program_vkeys=program_vkeys, public_values=public_values)
        pblob, poff = _blob(proofs)
        vblob, voff = _blob(public_values)
        st = np.zeros(n, dtype=np.uint8); rv = np.zeros((n, 4), dtype=np.uint8)
        _lib.check(self._L.zkv_sp1_gateway_verify_batch(self._h, n, _cat32(program_vkeys, 'program_vkey'), vblob, voff.ctypes.data,
                                                        pblob, poff.ctypes.data, st.ctypes.data, rv.ctypes.data), 'zkv_sp1_gateway_verify_batch')
        return st, rv

    def verify_batch_dev(self, n, d_vkeys, d_public_values, pv_len, d_proofs, d_proof_off, proof_bytes, d_status, d_recv=0, stream=0):
        """Device-resident batch: n x 32 program vkeys, public values at a fixed pv_len stride, ragged proofs (n + 1 uint64 offsets in device
        memory, proof_bytes = size of the proof buffer), n status bytes and n x 4 received selectors (0: none); enqueued on `stream`."""
        _lib.check(self._L.zkv_sp1_gateway_verify_batch_dev(self._h, n, d_vkeys, d_public_values, pv_len, d_proofs, d_proof_off, proof_bytes,
                                                            d_status, d_recv or None, stream or None), 'zkv_sp1_gateway_verify_batch_dev')

    def last_route_counts(self):
        """Proofs of the most recent call per route, then not found, then shorter than 4 bytes (or unreadable)."""
        k = self._L.zkv_sp1_gateway_route_count(self._h)
        out = (C.c_uint64 * (k + 2))()
        _lib.check(self._L.zkv_sp1_gateway_last_route_counts(self._h, out), 'zkv_sp1_gateway_last_route_counts')
        return list(out)

    def last_call_counts(self):
        """last_route_counts with one more column: requests of the most recent eth_call batch that were not canonical calldata."""
        from . import sp1_gateway_wire as w
        return w.last_call_counts(self._h, self._L.zkv_sp1_gateway_route_count(self._h))

    # eth_call batches (include/zkv_sp1_gateway_wire.h, sp1_gateway_wire.py): raw verifyProof calldata, decoded and routed on the device
    @staticmethod
    def encode_verify_proof_call(program_vkey, public_values, proof_bytes, form=1):
        """Canonical calldata in `form`: 0 = verifyProof(bytes32,uint8[],uint8[]), 1 = verifyProof(bytes32,bytes,bytes)."""
        from . import sp1_gateway_wire as w
        return w.encode_verify_proof_call(program_vkey, public_values, proof_bytes, form)

    def eth_call_batch(self, calls):
        """calls: calldata byte strings, either form, Groth16 and PLONK proofs mixed -> (reverted uint8[n], [return / revert data],
        status uint8[n]).  Success returns nothing; anything but a canonical verifyProof call is BAD_CALLDATA with empty revert data."""
        from . import sp1_gateway_wire as w
        return w.eth_call_batch(self._h, calls)

    def eth_call_batch_dev(self, n, d_calldata, d_calldata_off, calldata_bytes, d_status, d_recv=0, stream=0):
        """Device-resident calldata blob and its n + 1 uint64 offsets; n status bytes and n x 4 received selectors (0: none) stay on the
        device (eth_call_returndata turns one into return / revert data)."""
        from . import sp1_gateway_wire as w
        w.eth_call_batch_dev(self._h, n, d_calldata, d_calldata_off, calldata_bytes, d_status, d_recv, stream)

    def eth_call_returndata(self, status, received=bytes(4)):
        from . import sp1_gateway_wire as w
        return w.eth_call_returndata(self._h, status, received)

    def last_wire_ms(self):
        """Decode time of the most recent eth_call batch."""
        out = C.c_float(0)
        _lib.check(self._L.zkv_ctx_last_wire_ms(self._h, C.byref(out)), 'zkv_ctx_last_wire_ms')
        return out.value

    def status_abi_encode(self, status, received=bytes(4)):
        """Revert data of a gateway status (RouteNotFound(bytes4) for ROUTE_NOT_FOUND; unpinned)."""
        o = C.create_string_buffer(68)
        r = self._L.zkv_sp1_gateway_status_abi_encode(self._h, status, bytes(received), o)
        _lib.check(min(r, 0), 'zkv_sp1_gateway_status_abi_encode')
        return o.raw[:r]

    def set_lanes_per_proof(self, lanes):
        _lib.check(self._L.zkv_ctx_set_lanes_per_proof(self._h, lanes), 'zkv_ctx_set_lanes_per_proof')

    def reserve(self, n):
        """Device set-up of every route and buffers for batches of up to n proofs (optional)."""
        _lib.check(self._L.zkv_ctx_reserve(self._h, n), 'zkv_ctx_reserve')

    def set_aggregate_check(self, enable=True, seed=None, sub_batch=None):
        """Opt-in aggregate check on every route (include/zkv.h), each route with its own secret; statuses stay the per-proof ones.  The
        routes with caller keys take it together, under the key sets' rules (a call with at least ZKV_AGG_MIN proofs on them, the automatic
        mapping, keys with alpha and beta finite), with one secret of their own."""
        _set_aggregate_check(self._L, self._h, enable, seed, sub_batch)

    def aggregate_counters(self):
        """(sub-batches checked in aggregate, sub-batches that failed), summed over the routes, the group of keyed routes included."""
        return _aggregate_counters(self._L, self._h)

    def synchronize(self):
        _lib.check(self._L.zkv_ctx_synchronize(self._h), 'zkv_ctx_synchronize')

    def last_stage_ms(self):
        out = (C.c_float * 5)()
        _lib.check(self._L.zkv_ctx_last_stage_ms(self._h, out), 'zkv_ctx_last_stage_ms')
        return list(out)

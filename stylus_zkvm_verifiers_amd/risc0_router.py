"""RISC Zero verifier router (include/zkv_risc0_router.h): one context that sends every seal of a batch, on the device, to the Groth16
verifier whose 4-byte selector begins it -- built-in-key routes (a (control_root, bn254_control_id) pair on the key of risc0/crypto.rs)
and keyed routes (a caller's key with its own pair, the selector derived from the key's digest) -- as RISC Zero's on-chain
RiscZeroVerifierRouter forwards `verify` / `verifyIntegrity`.  The routing has no reference counterpart: ROUTE_NOT_FOUND is PARITY
UNPINNED; a seal routed to a built-in route gets the pinned RISC Zero statuses."""
import ctypes as C

import numpy as np

from . import _lib
from .errors import STATUS_OK, VM_RISC0, VerifierError
from .risc0 import _aggregate_counters, _blob, _cat32, _same_len, _set_aggregate_check

VM_RISC0_ROUTER = 12            # ZKV_VM_RISC0_ROUTER
MAX_ROUTES = 32                 # ZKV_RISC0_ROUTER_MAX_ROUTES
MAX_KEYED = 8                   # ZKV_RISC0_ROUTER_MAX_KEYED
KEY_BYTES = 832                 # ZKV_RISC0_KEY_BYTES: zkv_groth16_ctx_create's layout with n_ic = 6
SEAL_BYTES = 260                # ZKV_SEAL_BYTES
STATUS_ROUTE_NOT_FOUND = 8      # ZKV_STATUS_ROUTE_NOT_FOUND

_P, _SZ = C.c_void_p, C.c_size_t
# the router's own entry points (declared in include/zkv_risc0_router.h, not in zkv.h: _lib.SYMBOLS mirrors zkv.h alone)
SYMBOLS = {
    'zkv_risc0_router_create': (C.c_void_p, [_SZ, C.c_char_p, C.c_char_p, _SZ, C.POINTER(C.c_char_p), C.c_char_p, C.c_char_p, C.c_int]),
    'zkv_risc0_router_route_count': (C.c_size_t, [_P]),
    'zkv_risc0_router_route': (C.c_int, [_P, _SZ, C.c_char_p, C.POINTER(C.c_int)]),
    'zkv_risc0_router_route_verifier_key_digest': (C.c_int, [_P, _SZ, C.c_char_p]),
    'zkv_risc0_router_verify': (C.c_int, [_P, C.c_char_p, _SZ, C.c_char_p, C.c_char_p, C.POINTER(C.c_uint8), C.c_char_p]),
    'zkv_risc0_router_verify_integrity': (C.c_int, [_P, C.c_char_p, _SZ, C.c_char_p, C.POINTER(C.c_uint8), C.c_char_p]),
    'zkv_risc0_router_verify_batch': (C.c_int, [_P, _SZ, _P, _P, _P, _P, _P, _P]),
    'zkv_risc0_router_verify_integrity_batch': (C.c_int, [_P, _SZ, _P, _P, _P, _P, _P]),
    'zkv_risc0_router_verify_batch_dev': (C.c_int, [_P, _SZ, _P, _P, _P, _P, _P, _P]),
    'zkv_risc0_router_last_route_counts': (C.c_int, [_P, C.POINTER(C.c_uint64)]),
    'zkv_risc0_router_status_abi_encode': (C.c_int, [_P, C.c_uint8, C.c_char_p, C.c_char_p]),
}

_bound = None


class SelectorUnknown(VerifierError):
    """No route has the seal's selector (RiscZeroVerifierRouter's SelectorUnknown(bytes4); unpinned).  `.received`: the seal's 4 bytes."""

    def __init__(self, received, revert):
        Exception.__init__(self, 'SelectorUnknown(%s)' % received.hex())
        self.vm, self.status, self.received, self.expected, self.revert = VM_RISC0, STATUS_ROUTE_NOT_FOUND, received, None, revert


def lib():
    """The library with the router's symbols bound (AttributeError when one is not exported)."""
    global _bound
    L = _lib.lib()
    if _bound is not L:
        for name, (res, args) in SYMBOLS.items():
            fn = getattr(L, name)
            fn.restype = res
            fn.argtypes = args
        _bound = L
    return L


class RiscZeroRouter:
    """routes: list of (control_root, bn254_control_id), one built-in-key route each, in order; keyed: list of (vk_words, control_root,
    bn254_control_id), Groth16 keys of other releases in Groth16Verifier's layout with n_ic = 6 and RISC Zero's convention, one route
    each, in order, behind the built-in routes.  At most MAX_ROUTES routes, MAX_KEYED of them keyed, selectors pairwise distinct."""

    def __init__(self, routes=(), keyed=(), device=0):
        routes = [(bytes(r), bytes(i)) for r, i in routes]
        keyed = [(bytes(vk), bytes(r), bytes(i)) for vk, r, i in keyed]
        if not 1 <= len(routes) + len(keyed) <= MAX_ROUTES or len(keyed) > MAX_KEYED:
            raise ValueError('a router holds 1 .. %d routes, at most %d of them keyed' % (MAX_ROUTES, MAX_KEYED))
        for vk, _, _ in keyed:
            if len(vk) != KEY_BYTES:
                raise ValueError('a keyed route takes a %d-byte key (n_ic = 6)' % KEY_BYTES)
        self._L = lib()
        self._vk = [vk for vk, _, _ in keyed]                       # alive for the call; the library copies them
        vks = (C.c_char_p * max(len(keyed), 1))(*self._vk)
        self._h = self._L.zkv_risc0_router_create(len(routes), _cat32([r for r, _ in routes], 'control_root'),
                                                  _cat32([i for _, i in routes], 'bn254_control_id'), len(keyed), vks,
                                                  _cat32([r for _, r, _ in keyed], 'control_root'),
                                                  _cat32([i for _, _, i in keyed], 'bn254_control_id'), device)
        if not self._h:
            raise ValueError('zkv_risc0_router_create rejected the routes (two routes with one selector)')

    def close(self):
        if getattr(self, '_h', None):
            self._L.zkv_ctx_destroy(self._h)
            self._h = None

    __del__ = close

    def routes(self):
        """[(selector (4 bytes), keyed (bool), verifier key digest (32 bytes))] in route order."""
        out = []
        for r in range(self._L.zkv_risc0_router_route_count(self._h)):
            sel = C.create_string_buffer(4); keyed = C.c_int(-1); dig = C.create_string_buffer(32)
            _lib.check(self._L.zkv_risc0_router_route(self._h, r, sel, C.byref(keyed)), 'zkv_risc0_router_route')
            _lib.check(self._L.zkv_risc0_router_route_verifier_key_digest(self._h, r, dig), 'zkv_risc0_router_route_verifier_key_digest')
            out.append((sel.raw, bool(keyed.value), dig.raw))
        return out

    def _result(self, status, recv):
        if status == STATUS_OK:
            return True
        if status == STATUS_ROUTE_NOT_FOUND:
            raise SelectorUnknown(recv, self.status_revert(status, recv))
        raise VerifierError(VM_RISC0, status)              # (never SELECTOR_MISMATCH: the route picked has the seal's selector)

    # ---- IRiscZeroVerifier, as the router forwards it
    def verify(self, seal, image_id, journal_digest):
        """Returns True or raises VerifierError (status ROUTE_NOT_FOUND: `received` holds the seal's selector)."""
        st = C.c_uint8(0); rv = C.create_string_buffer(4)
        _lib.check(self._L.zkv_risc0_router_verify(self._h, bytes(seal), len(seal), bytes(image_id), bytes(journal_digest), C.byref(st), rv),
                   'zkv_risc0_router_verify')
        return self._result(st.value, rv.raw)

    def verify_integrity(self, receipt_seal, receipt_claim_digest):
        st = C.c_uint8(0); rv = C.create_string_buffer(4)
        _lib.check(self._L.zkv_risc0_router_verify_integrity(self._h, bytes(receipt_seal), len(receipt_seal), bytes(receipt_claim_digest),
                                                             C.byref(st), rv), 'zkv_risc0_router_verify_integrity')
        return self._result(st.value, rv.raw)

    # ---- batches
    def verify_batch(self, seals, image_ids, journal_digests):
        """Ragged host buffers -> (status uint8[n], received selector uint8[n, 4])."""
        n = len(seals)
        _same_len(n, image_ids=image_ids, journal_digests=journal_digests)
        blob, off = _blob(seals)
        st = np.zeros(n, dtype=np.uint8); rv = np.zeros((n, 4), dtype=np.uint8)
        _lib.check(self._L.zkv_risc0_router_verify_batch(self._h, n, blob, off.ctypes.data, _cat32(image_ids, 'image_id'),
                                                         _cat32(journal_digests, 'journal_digest'), st.ctypes.data, rv.ctypes.data),
                   'zkv_risc0_router_verify_batch')
        return st, rv

    def verify_integrity_batch(self, seals, claim_digests):
        n = len(seals)
        _same_len(n, claim_digests=claim_digests)
        blob, off = _blob(seals)
        st = np.zeros(n, dtype=np.uint8); rv = np.zeros((n, 4), dtype=np.uint8)
        _lib.check(self._L.zkv_risc0_router_verify_integrity_batch(self._h, n, blob, off.ctypes.data, _cat32(claim_digests, 'claim_digest'),
                                                                   st.ctypes.data, rv.ctypes.data), 'zkv_risc0_router_verify_integrity_batch')
        return st, rv

    def verify_batch_dev(self, n, d_seals, d_image_ids, d_journal_digests, d_status, d_recv=0, stream=0):
        """Device-resident batch: n x SEAL_BYTES seals, n x 32 image ids, n x 32 journal digests (0: verify_integrity, the first row then
        holds claim digests), n status bytes and n x 4 received selectors (0: none); enqueued on `stream`."""
        _lib.check(self._L.zkv_risc0_router_verify_batch_dev(self._h, n, d_seals, d_image_ids, d_journal_digests or None, d_status,
                                                             d_recv or None, stream or None), 'zkv_risc0_router_verify_batch_dev')

    def verify_ragged_dev(self, n, d_seal_blob, d_seal_off, blob_bytes, d_image_ids, d_journal_digests, d_status, d_recv=0, stream=0):
        """verify_batch_dev on seals of any length: a device blob (any alignment) and its n + 1 uint64 offsets, none followed beyond
        blob_bytes (include/zkv_risc0_router_set.h, risc0_router_set.py)."""
        from . import risc0_router_set as rs
        rs.verify_ragged_dev(self._h, n, d_seal_blob, d_seal_off, blob_bytes, d_image_ids, d_journal_digests, d_status, d_recv, stream)

    def last_route_counts(self):
        """Seals of the most recent call per route, then selector unknown, then shorter than 4 bytes."""
        k = self._L.zkv_risc0_router_route_count(self._h)
        out = (C.c_uint64 * (k + 2))()
        _lib.check(self._L.zkv_risc0_router_last_route_counts(self._h, out), 'zkv_risc0_router_last_route_counts')
        return list(out)

    # ---- a method per seal, and eth_call batches (include/zkv_risc0_router_wire.h, risc0_router_wire.py)
    def verify_call_batch(self, methods, seals, in_a, in_b):
        """methods[i]: 0 = verify (in_a image id, in_b journal digest), 1 = verifyIntegrity (in_a claim digest, in_b not read); None: all
        verify.  Any other method byte is BAD_CALLDATA.  -> (status uint8[n], received selector uint8[n, 4])."""
        from . import risc0_router_wire as w
        return w.verify_call_batch(self._h, methods, seals, in_a, in_b)

    def verify_call_batch_dev(self, n, d_method, d_seals, d_in_a, d_in_b, d_status, d_recv=0, stream=0):
        """verify_batch_dev with n method bytes on the device (0: all verify); d_in_b is always a row of n x 32 bytes."""
        from . import risc0_router_wire as w
        w.verify_call_batch_dev(self._h, n, d_method, d_seals, d_in_a, d_in_b, d_status, d_recv, stream)

    @staticmethod
    def encode_verify_call(seal, image_id, journal_digest, form=1):
        """Canonical calldata in `form`: 0 = verify(uint8[],bytes32,bytes32), 1 = verify(bytes,bytes32,bytes32)."""
        from . import risc0_router_wire as w
        return w.encode_verify_call(seal, image_id, journal_digest, form)

    @staticmethod
    def encode_verify_integrity_call(seal, claim_digest, form=1):
        """Canonical calldata in `form`: 0 = verifyIntegrity(uint8[],bytes32), 1 = verifyIntegrity((bytes,bytes32))."""
        from . import risc0_router_wire as w
        return w.encode_verify_integrity_call(seal, claim_digest, form)

    def eth_call_batch(self, calls):
        """calls: calldata byte strings, both methods, both forms and seals of every route mixed -> (reverted uint8[n], [return / revert
        data], status uint8[n]).  Anything but a canonical verify / verifyIntegrity call is BAD_CALLDATA with empty revert data."""
        from . import risc0_router_wire as w
        return w.eth_call_batch(self._h, calls)

    def eth_call_batch_dev(self, n, d_calldata, d_calldata_off, calldata_bytes, d_status, d_recv=0, d_call_kind=0, stream=0):
        """Device-resident calldata blob and its n + 1 uint64 offsets; n status bytes, n x 4 received selectors (0: none) and n call kinds
        (0: none) stay on the device (eth_call_returndata turns one into return / revert data)."""
        from . import risc0_router_wire as w
        w.eth_call_batch_dev(self._h, n, d_calldata, d_calldata_off, calldata_bytes, d_status, d_recv, d_call_kind, stream)

    def eth_call_returndata(self, status, received=bytes(4), call_kind=255):
        from . import risc0_router_wire as w
        return w.eth_call_returndata(self._h, status, received, call_kind)

    def last_call_counts(self):
        """last_route_counts with one more column: seals of the most recent call that were bad calldata."""
        from . import risc0_router_wire as w
        return w.last_call_counts(self._h, self._L.zkv_risc0_router_route_count(self._h))

    def last_wire_ms(self):
        """Decode time of the most recent eth_call batch."""
        out = C.c_float(0)
        _lib.check(self._L.zkv_ctx_last_wire_ms(self._h, C.byref(out)), 'zkv_ctx_last_wire_ms')
        return out.value

    def status_revert(self, status, received=bytes(4)):
        """Revert data of a router status (SelectorUnknown(bytes4) for ROUTE_NOT_FOUND; unpinned)."""
        o = C.create_string_buffer(68)
        r = self._L.zkv_risc0_router_status_abi_encode(self._h, status, bytes(received), o)
        _lib.check(min(r, 0), 'zkv_risc0_router_status_abi_encode')
        return o.raw[:r]

    def set_lanes_per_proof(self, lanes):
        _lib.check(self._L.zkv_ctx_set_lanes_per_proof(self._h, lanes), 'zkv_ctx_set_lanes_per_proof')

    def reserve(self, n):
        """Device set-up of both groups and buffers for batches of up to n seals (optional)."""
        _lib.check(self._L.zkv_ctx_reserve(self._h, n), 'zkv_ctx_reserve')

    def set_aggregate_check(self, enable=True, seed=None, sub_batch=None):
        """Opt-in aggregate check (include/zkv.h) on the built-in routes and, under the key sets' rules, on the keyed routes (a call with at
        least ZKV_AGG_MIN seals on them, the automatic mapping, keys with alpha and beta finite); statuses stay the per-proof ones."""
        _set_aggregate_check(self._L, self._h, enable, seed, sub_batch)

    def aggregate_counters(self):
        """(sub-batches checked in aggregate, sub-batches that failed), summed over the built-in and the keyed group."""
        return _aggregate_counters(self._L, self._h)

    def synchronize(self):
        _lib.check(self._L.zkv_ctx_synchronize(self._h), 'zkv_ctx_synchronize')

    def last_stage_ms(self):
        out = (C.c_float * 5)()
        _lib.check(self._L.zkv_ctx_last_stage_ms(self._h, out), 'zkv_ctx_last_stage_ms')
        return list(out)

"""RISC Zero verifier router with a set route (include/zkv_risc0_router_set.h): the routes of RiscZeroRouter plus the RiscZeroSetVerifier
of one set-builder image id, registered under its own selector with the router itself as its inner verifier -- as on chain.  A
set-inclusion seal arrives like any other seal; its Merkle path is hashed on the device and its root seal is verified by whichever route
the root seal's own selector names, once per distinct root seal.  PARITY UNPINNED: the reference holds no router and no set verifier."""
import ctypes as C

import numpy as np

from . import _lib, risc0_router
from .risc0 import _cat32
from .risc0_router import KEY_BYTES, MAX_KEYED, MAX_ROUTES, RiscZeroRouter

ROUTE_BUILTIN, ROUTE_KEYED, ROUTE_SET = 0, 1, 2     # `keyed` of zkv_risc0_router_route
MAX_DEPTH = 64                                      # ZKV_SETINCL_MAX_DEPTH
MAX_ROOTS = 4096                                    # ZKV_SETINCL_MAX_ROOTS

_P, _SZ = C.c_void_p, C.c_size_t
# declared in include/zkv_risc0_router_set.h (risc0_router.SYMBOLS mirrors zkv_risc0_router.h alone)
SYMBOLS = {
    'zkv_risc0_router_create_with_set': (C.c_void_p, [_SZ, C.c_char_p, C.c_char_p, _SZ, C.POINTER(C.c_char_p), C.c_char_p, C.c_char_p, C.c_char_p, C.c_int]),
    'zkv_risc0_router_set_selector': (C.c_int, [_P, C.c_char_p]),
    'zkv_risc0_router_verify_ragged_dev': (C.c_int, [_P, _SZ, _P, _P, C.c_uint64, _P, _P, _P, _P, _P]),
    'zkv_risc0_router_set_submit_root': (C.c_int, [_P, C.c_char_p, C.c_char_p, _SZ, C.POINTER(C.c_uint8), C.c_char_p]),
    'zkv_risc0_router_set_has_root': (C.c_int, [_P, C.c_char_p]),
    'zkv_risc0_router_set_last_counts': (C.c_int, [_P, C.POINTER(C.c_uint64)]),
    'zkv_diag_rzset_groups': (C.c_int, [_P, _SZ, _P, _P, _SZ, C.c_uint32, _P]),
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


def verify_ragged_dev(handle, n, d_seal_blob, d_seal_off, blob_bytes, d_image_ids, d_journal_digests, d_status, d_recv=0, stream=0):
    """Device-resident batch of seals of any length on ANY router: the blob (any alignment), its n + 1 uint64 offsets, n x 32 image ids,
    n x 32 journal digests (0: verify_integrity, the first row then holds claim digests), n status bytes and n x 4 received selectors
    (0: none); enqueued on `stream`."""
    _lib.check(lib().zkv_risc0_router_verify_ragged_dev(handle, n, d_seal_blob or None, d_seal_off, blob_bytes, d_image_ids, d_journal_digests or None,
                                                        d_status, d_recv or None, stream or None), 'zkv_risc0_router_verify_ragged_dev')


def abi_encode_seal(path, root_seal):
    """abi.encode(Seal{bytes32[] path; bytes rootSeal}), the canonical body of a set-inclusion seal."""
    path, root_seal = [bytes(p) for p in path], bytes(root_seal)
    if any(len(p) != 32 for p in path):
        raise ValueError('a path element is 32 bytes')
    word = lambda v: int(v).to_bytes(32, 'big')
    return (word(0x20) + word(0x40) + word(0x60 + 32 * len(path)) + word(len(path)) + b''.join(path) + word(len(root_seal)) + root_seal +
            bytes(-len(root_seal) % 32))


class RiscZeroSetRouter(RiscZeroRouter):
    """RiscZeroRouter(routes, keyed) plus the set route of `set_builder_image_id`: the last route, at most MAX_ROUTES routes in all.
    verify / verify_integrity / verify_batch / verify_integrity_batch take set-inclusion seals beside Groth16 seals, and so do
    verify_call_batch / verify_call_ragged_dev / eth_call_batch / eth_call_batch_dev, which go through the entry points of
    include/zkv_risc0_router_set_wire.h (risc0_router_set_wire.py); only the fixed-stride calls verify_batch_dev and
    verify_call_batch_dev are out of scope on such a router (ZKV_ERR_WRONG_CTX)."""

    def __init__(self, set_builder_image_id, routes=(), keyed=(), device=0):
        set_id = bytes(set_builder_image_id)
        if len(set_id) != 32:
            raise ValueError('set_builder_image_id must be 32 bytes')
        routes = [(bytes(r), bytes(i)) for r, i in routes]
        keyed = [(bytes(vk), bytes(r), bytes(i)) for vk, r, i in keyed]
        if not 1 <= len(routes) + len(keyed) <= MAX_ROUTES - 1 or len(keyed) > MAX_KEYED:
            raise ValueError('a set router holds 1 .. %d Groth16 routes, at most %d of them keyed' % (MAX_ROUTES - 1, MAX_KEYED))
        for vk, _, _ in keyed:
            if len(vk) != KEY_BYTES:
                raise ValueError('a keyed route takes a %d-byte key (n_ic = 6)' % KEY_BYTES)
        self._L = lib()
        self._vk = [vk for vk, _, _ in keyed]                       # alive for the call; the library copies them
        vks = (C.c_char_p * max(len(keyed), 1))(*self._vk)
        self.set_builder_image_id = set_id
        self._h = self._L.zkv_risc0_router_create_with_set(len(routes), _cat32([r for r, _ in routes], 'control_root'),
                                                           _cat32([i for _, i in routes], 'bn254_control_id'), len(keyed), vks,
                                                           _cat32([r for _, r, _ in keyed], 'control_root'),
                                                           _cat32([i for _, _, i in keyed], 'bn254_control_id'), set_id, device)
        if not self._h:
            raise ValueError('zkv_risc0_router_create_with_set rejected the routes (two routes with one selector)')

    def routes(self):
        """[(selector (4 bytes), kind (ROUTE_BUILTIN / ROUTE_KEYED / ROUTE_SET), verifier key digest (32 bytes; None for the set route))]."""
        out = []
        for r in range(self._L.zkv_risc0_router_route_count(self._h)):
            sel = C.create_string_buffer(4); kind = C.c_int(-1); dig = C.create_string_buffer(32)
            _lib.check(self._L.zkv_risc0_router_route(self._h, r, sel, C.byref(kind)), 'zkv_risc0_router_route')
            if kind.value == ROUTE_SET:
                out.append((sel.raw, ROUTE_SET, None))
                continue
            _lib.check(self._L.zkv_risc0_router_route_verifier_key_digest(self._h, r, dig), 'zkv_risc0_router_route_verifier_key_digest')
            out.append((sel.raw, kind.value, dig.raw))
        return out

    def set_selector(self):
        o = C.create_string_buffer(4)
        _lib.check(self._L.zkv_risc0_router_set_selector(self._h, o), 'zkv_risc0_router_set_selector')
        return o.raw

    def encode_seal(self, path, root_seal=b''):
        """The on-chain form of one set-inclusion seal: set selector || abi.encode(Seal{path, rootSeal})."""
        return self.set_selector() + abi_encode_seal(path, root_seal)

    def verify_ragged_dev(self, n, d_seal_blob, d_seal_off, blob_bytes, d_image_ids, d_journal_digests, d_status, d_recv=0, stream=0):
        verify_ragged_dev(self._h, n, d_seal_blob, d_seal_off, blob_bytes, d_image_ids, d_journal_digests, d_status, d_recv, stream)

    # ---- a method per seal, and eth_call batches: RiscZeroRouter's methods and return shapes on seals of any length
    def verify_call_batch(self, methods, seals, in_a, in_b):
        from . import risc0_router_set_wire as w
        return w.verify_call_ragged(self._h, methods, seals, in_a, in_b)

    def verify_call_ragged_dev(self, n, d_method, d_seal_blob, d_seal_off, blob_bytes, d_in_a, d_in_b, d_status, d_recv=0, stream=0):
        """verify_ragged_dev with n method bytes on the device (0: all verify); d_in_b is always a row of n x 32 bytes."""
        from . import risc0_router_set_wire as w
        w.verify_call_ragged_dev(self._h, n, d_method, d_seal_blob, d_seal_off, blob_bytes, d_in_a, d_in_b, d_status, d_recv, stream)

    def eth_call_batch(self, calls):
        from . import risc0_router_set_wire as w
        return w.eth_call_ragged(self._h, calls)

    def eth_call_batch_dev(self, n, d_calldata, d_calldata_off, calldata_bytes, d_status, d_recv=0, d_call_kind=0, stream=0):
        from . import risc0_router_set_wire as w
        w.eth_call_ragged_dev(self._h, n, d_calldata, d_calldata_off, calldata_bytes, d_status, d_recv, d_call_kind, stream)

    def last_call_counts(self):
        """last_route_counts (the set route under its own index) with one more column: bad calldata."""
        from . import risc0_router_set_wire as w
        return w.last_ragged_call_counts(self._h, self._L.zkv_risc0_router_route_count(self._h))

    def submit_root(self, root, seal):
        """(status, received selector) of the router's verify(seal, ID, sha256(ID || root)); the root is remembered when that is OK."""
        st = C.c_uint8(0); rv = C.create_string_buffer(4)
        _lib.check(self._L.zkv_risc0_router_set_submit_root(self._h, bytes(root), bytes(seal), len(seal), C.byref(st), rv),
                   'zkv_risc0_router_set_submit_root')
        return st.value, rv.raw

    def has_root(self, root):
        r = self._L.zkv_risc0_router_set_has_root(self._h, bytes(root))
        _lib.check(min(r, 0), 'zkv_risc0_router_set_has_root')
        return bool(r)

    def set_last_counts(self):
        """(set seals, distinct root seals, root jobs run, stored-root lookups) of the most recent call."""
        out = (C.c_uint64 * 4)()
        _lib.check(self._L.zkv_risc0_router_set_last_counts(self._h, out), 'zkv_risc0_router_set_last_counts')
        return tuple(out)

    def diag_groups(self, seals, fp_mask=0xFFFFFFFF, blob_shift=0):
        """Test only: every seal's representative from the front and identity kernels alone (zkv_diag_rzset_groups)."""
        n = len(seals)
        blob = np.frombuffer(b''.join(bytes(s) for s in seals) + b'\0', dtype=np.uint8).copy()
        off = np.zeros(n + 1, dtype=np.uint64)
        off[1:] = np.cumsum([len(s) for s in seals], dtype=np.uint64)
        out = np.zeros(n, dtype=np.uint32)
        _lib.check(self._L.zkv_diag_rzset_groups(self._h, n, blob.ctypes.data, off.ctypes.data, blob_shift, fp_mask, out.ctypes.data), 'zkv_diag_rzset_groups')
        return out

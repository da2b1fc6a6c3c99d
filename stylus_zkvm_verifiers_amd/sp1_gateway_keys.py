"""SP1 gateway, Groth16 routes with caller-supplied keys (include/zkv_sp1_gateway_keys.h): one route per SP1 release's Groth16 key and
VERIFIER_HASH beside the built-in v5.0.0 route and the PLONK routes, all keyed routes verified in one pass on the device.
Sp1Gateway(groth16_keys=...) is the front of this module.  A keyed route holding the reference's own SP1 key and hash gives the pinned
SP1 statuses; PARITY UNPINNED for every other key."""
import ctypes as C

from . import _lib, sp1_gateway

KEY_BYTES = 640                 # ZKV_SP1_GROTH16_KEY_BYTES: zkv_groth16_ctx_create's layout with n_ic = 3

_P, _SZ = C.c_void_p, C.c_size_t
# declared in include/zkv_sp1_gateway_keys.h (sp1_gateway.SYMBOLS mirrors zkv_sp1_gateway.h alone)
SYMBOLS = {
    'zkv_sp1_gateway_create_keyed': (C.c_void_p, [C.c_int, _SZ, C.POINTER(C.c_char_p), C.c_char_p,
                                                  _SZ, C.POINTER(C.c_char_p), C.POINTER(C.c_size_t), C.c_char_p, C.c_int]),
    'zkv_sp1_gateway_route_verifier_hash': (C.c_int, [_P, _SZ, C.c_char_p]),
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


def create(groth16, groth16_keys, plonk, device):
    """zkv_sp1_gateway_create_keyed -> handle (0 when the library refuses the routes).  groth16_keys: [(vk_words, verifier_hash)],
    plonk: [(vk_bytes, verifier_hash)], both already bytes."""
    for vk, h in groth16_keys:
        if len(vk) != KEY_BYTES:
            raise ValueError('a keyed Groth16 route takes a %d-byte key (n_ic = 3)' % KEY_BYTES)
        if len(h) != 32:
            raise ValueError('verifier_hash must be 32 bytes')
    k, p = len(groth16_keys), len(plonk)
    keys = (C.c_char_p * max(k, 1))(*[vk for vk, _ in groth16_keys])
    vks = (C.c_char_p * max(p, 1))(*[vk for vk, _ in plonk])
    lens = (C.c_size_t * max(p, 1))(*[len(vk) for vk, _ in plonk])
    return lib().zkv_sp1_gateway_create_keyed(1 if groth16 else 0, k, keys, b''.join(h for _, h in groth16_keys) + b'\0',
                                              p, vks, lens, b''.join(h for _, h in plonk) + b'\0', device)


def route_verifier_hash(handle, r):
    o = C.create_string_buffer(32)
    _lib.check(lib().zkv_sp1_gateway_route_verifier_hash(handle, r, o), 'zkv_sp1_gateway_route_verifier_hash')
    return o.raw

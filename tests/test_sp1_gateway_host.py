"""SP1 gateway (include/zkv_sp1_gateway.h) without a device: the header against the library's exports, creation
and argument checks, context-wide calls, the RouteNotFound encoding, and the numpy routing model (tests/gateway_model.py) against a
direct per-proof rule.  Parity unpinned: the reference holds no gateway and no PLONK code."""
import ctypes as C
import hashlib
import json
import os
import re

import numpy as np
import pytest

import gateway_model as gm

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
H = bytes.fromhex
NEW = ['zkv_sp1_gateway_create', 'zkv_sp1_gateway_route_count', 'zkv_sp1_gateway_route', 'zkv_sp1_gateway_route_ctx',
       'zkv_sp1_gateway_verify_proof', 'zkv_sp1_gateway_verify_batch', 'zkv_sp1_gateway_verify_batch_dev',
       'zkv_sp1_gateway_last_route_counts', 'zkv_sp1_gateway_status_abi_encode']
WRONG_CTX, INVALID_ARG = -5, -1


def _names(path):
    return set(re.findall(r'\b(zkv_[a-z0-9_]+)\s*\(', re.sub(r'/\*.*?\*/', '', open(path).read(), flags=re.S)))


@pytest.fixture(scope='module')
def L():
    from stylus_zkvm_verifiers_amd import sp1_gateway
    return sp1_gateway.lib()


@pytest.fixture(scope='module')
def plonk():
    d = json.load(open(os.path.join(HERE, 'golden', 'plonk_cases.json')))
    return H(d['vk']), H(d['verifier_hash'])


def _hash(prefix):
    return bytes(prefix) + hashlib.sha256(bytes(prefix)).digest()[:28]


def _create(L, groth16, keys):
    k = len(keys)
    vks = (C.c_char_p * max(k, 1))(*[vk for vk, _ in keys])
    lens = (C.c_size_t * max(k, 1))(*[len(vk) for vk, _ in keys])
    return L.zkv_sp1_gateway_create(groth16, k, vks, lens, b''.join(h for _, h in keys) + b'\0', 0)


def test_header_declares_exactly_the_new_symbols_and_the_library_exports_them(L):
    hdr = os.path.join(ROOT, 'include', 'zkv_sp1_gateway.h')
    assert _names(hdr) == set(NEW)
    text = open(hdr).read()
    for d in ('#include "zkv.h"', '#define ZKV_VM_SP1_GATEWAY 8', '#define ZKV_SP1_GATEWAY_MAX_ROUTES 8', '#define ZKV_STATUS_ROUTE_NOT_FOUND 8'):
        assert d in text, d
    assert 'PARITY UNPINNED' in text
    from stylus_zkvm_verifiers_amd import _lib, sp1_gateway
    assert set(sp1_gateway.SYMBOLS) == set(NEW) and not set(NEW) & set(_lib.SYMBOLS)
    for name in NEW:
        assert hasattr(L, name), name
    main = _names(os.path.join(ROOT, 'include', 'zkv.h'))
    assert len(main) == 83 and not main & set(NEW)


def test_create_refuses_bad_route_sets(L, plonk):
    vk, vh = plonk
    from stylus_zkvm_verifiers_amd import Sp1Gateway
    sp1_sel = Sp1Gateway.groth16_verifier_hash()[:4]
    assert not _create(L, 0, [])                                                   # no route
    assert not _create(L, 1, [(vk, _hash(bytes([1, 2, 3, k]))) for k in range(8)])  # 9 routes
    assert not _create(L, 0, [(vk, _hash(bytes([1, 2, 3, k]))) for k in range(9)])
    assert not _create(L, 0, [(vk, _hash(b'\x01\x02\x03\x04')), (vk, _hash(b'\x01\x02\x03\x04'))])    # equal selectors
    assert not _create(L, 1, [(vk, _hash(sp1_sel))])                               # a PLONK hash with the Groth16 selector
    assert not _create(L, 1, [(vk[:-1], vh)])                                      # 1,055-byte key
    assert not _create(L, 1, [(vk + b'\0', vh)])
    assert not _create(L, 2, [(vk, vh)])                                           # groth16 must be 0 / 1
    assert not L.zkv_sp1_gateway_create(1, 1, None, (C.c_size_t * 1)(len(vk)), vh, 0)
    assert not L.zkv_sp1_gateway_create(1, 1, (C.c_char_p * 1)(vk), None, vh, 0)
    assert not L.zkv_sp1_gateway_create(1, 1, (C.c_char_p * 1)(vk), (C.c_size_t * 1)(len(vk)), None, 0)
    assert not L.zkv_sp1_gateway_create(1, 2, (C.c_char_p * 2)(vk, None), (C.c_size_t * 2)(len(vk), len(vk)), vh + _hash(b'\x09\x09\x09\x09'), 0)
    assert len(vk) == 1056
    # the largest gateways: 8 PLONK routes, or Groth16 + 7
    for groth16, k in ((0, 8), (1, 7)):
        h = _create(L, groth16, [(vk, _hash(bytes([7, 7, 7, j]))) for j in range(k)])
        assert h and L.zkv_sp1_gateway_route_count(h) == 8
        L.zkv_ctx_destroy(h)
    with pytest.raises(ValueError):
        Sp1Gateway(False, [])
    with pytest.raises(ValueError):
        Sp1Gateway(True, [(vk, vh[:31])])
    with pytest.raises(ValueError):
        Sp1Gateway(True, [(vk, _hash(sp1_sel))])


def test_routes_getters_and_context_wide_calls_without_a_device(L, plonk):
    vk, vh = plonk
    from stylus_zkvm_verifiers_amd import Sp1Gateway, _lib
    raw = _lib.lib()
    vh2 = _hash(b'\x5e\xc0\x4d\x00')
    gw = Sp1Gateway(True, [(vk, vh), (vk, vh2)])
    sp1_hash = Sp1Gateway.groth16_verifier_hash()
    assert gw.routes() == [(sp1_hash[:4], 1, sp1_hash), (vh[:4], 6, vh), (vh2[:4], 6, vh2)]
    assert raw.zkv_ctx_vm(gw._h) == 8
    o = C.create_string_buffer(32)
    for r, want in ((1, vh), (2, vh2)):
        k = L.zkv_sp1_gateway_route_ctx(gw._h, r)
        assert k and raw.zkv_ctx_vm(k) == 6 and raw.zkv_sp1_plonk_verifier_hash(k, o) == 0 and o.raw == want
    k0 = L.zkv_sp1_gateway_route_ctx(gw._h, 0)
    assert raw.zkv_ctx_vm(k0) == 1
    assert not L.zkv_sp1_gateway_route_ctx(gw._h, 3)
    sel = C.create_string_buffer(4); vm = C.c_int()
    assert L.zkv_sp1_gateway_route(gw._h, 3, sel, C.byref(vm)) == INVALID_ARG
    # context-wide calls forward (nothing is set up yet, so nothing runs)
    assert raw.zkv_ctx_set_lanes_per_proof(gw._h, 16) == 0 and raw.zkv_ctx_set_lanes_per_proof(gw._h, 3) == INVALID_ARG
    assert raw.zkv_ctx_set_aggregate_check(gw._h, 64, bytes(32)) == 0
    assert raw.zkv_ctx_set_aggregate_check(gw._h, 0, None) == 0
    assert gw.aggregate_counters() == (0, 0)
    assert raw.zkv_ctx_synchronize(gw._h) == 0
    # single-device: no shards, no vk_x, no SP1 / PLONK entry point of zkv.h
    arr = (C.c_void_p * 2)(gw._h, None)
    assert not raw.zkv_ctx_create_sharded(arr, 1)
    assert raw.zkv_ctx_vk_x_batch(gw._h, 1, bytes(64), C.create_string_buffer(64)) == WRONG_CTX
    st = C.c_uint8(0)
    assert raw.zkv_sp1_verify_batch(gw._h, 0, None, None, None, None, None, None, None) == WRONG_CTX
    assert raw.zkv_sp1_verify_batch_dev(gw._h, 0, None, None, 0, None, None, None, None) == WRONG_CTX
    assert raw.zkv_sp1_verify_proof(gw._h, bytes(32), b'', 0, b'abcd', 4, C.byref(st), None) == WRONG_CTX
    assert raw.zkv_sp1_plonk_verify_batch(gw._h, 0, None, None, None, None, None, None, None) == WRONG_CTX
    assert raw.zkv_sp1_plonk_verify_batch_dev(gw._h, 0, None, None, 0, None, None, None, None) == WRONG_CTX
    assert raw.zkv_sp1_plonk_verify_proof(gw._h, bytes(32), b'', 0, b'abcd', 4, C.byref(st), None) == WRONG_CTX
    assert raw.zkv_sp1_plonk_verifier_hash(gw._h, o) == WRONG_CTX
    assert raw.zkv_sp1_eth_call_batch(gw._h, 0, None, None, None, None, None, None) == WRONG_CTX
    assert raw.zkv_eth_call_batch_dev(gw._h, 0, None, None, 0, None, None, None) == WRONG_CTX
    assert raw.zkv_mixed_ctx_sp1(gw._h) is None
    gw.close()


def test_gateway_entry_points_refuse_wrong_contexts_and_bad_arguments(L, plonk):
    vk, vh = plonk
    from stylus_zkvm_verifiers_amd import _lib
    raw = _lib.lib()
    sp = raw.zkv_sp1_ctx_create(0)
    pk = raw.zkv_sp1_plonk_ctx_create(vk, len(vk), vh, 0)
    st = C.c_uint8(0); rv = C.create_string_buffer(4); out = C.create_string_buffer(68); cnt = (C.c_uint64 * 10)()
    for h in (None, sp, pk):
        assert L.zkv_sp1_gateway_route_count(h) == 0 and not L.zkv_sp1_gateway_route_ctx(h, 0)
        assert L.zkv_sp1_gateway_route(h, 0, rv, None) == WRONG_CTX
        assert L.zkv_sp1_gateway_verify_proof(h, bytes(32), b'', 0, b'ab', 2, C.byref(st), rv) == WRONG_CTX
        assert L.zkv_sp1_gateway_verify_batch(h, 0, None, None, None, None, None, None, None) == WRONG_CTX
        assert L.zkv_sp1_gateway_verify_batch_dev(h, 0, None, None, 0, None, None, 0, None, None, None) == WRONG_CTX
        assert L.zkv_sp1_gateway_last_route_counts(h, cnt) == WRONG_CTX
        assert L.zkv_sp1_gateway_status_abi_encode(h, 8, b'abcd', out) == WRONG_CTX
    g = _create(L, 1, [(vk, vh)])
    assert g
    assert L.zkv_sp1_gateway_verify_proof(g, None, b'', 0, b'ab', 2, C.byref(st), rv) == INVALID_ARG
    assert L.zkv_sp1_gateway_verify_proof(g, bytes(32), None, 3, b'ab', 2, C.byref(st), rv) == INVALID_ARG
    assert L.zkv_sp1_gateway_verify_proof(g, bytes(32), b'', 0, None, 2, C.byref(st), rv) == INVALID_ARG
    assert L.zkv_sp1_gateway_verify_proof(g, bytes(32), b'', 0, b'ab', 2, None, rv) == INVALID_ARG
    assert L.zkv_sp1_gateway_verify_batch(g, 1, None, b'', None, b'', None, None, None) == INVALID_ARG
    off_bad = np.array([8, 4], dtype=np.uint64); off_ok = np.array([0, 4], dtype=np.uint64)
    s1 = np.zeros(1, np.uint8)
    assert L.zkv_sp1_gateway_verify_batch(g, 1, bytes(32), b'\0', off_ok.ctypes.data, bytes(9), off_bad.ctypes.data, s1.ctypes.data, None) == INVALID_ARG
    assert L.zkv_sp1_gateway_verify_batch(g, 1, bytes(32), b'\0', off_bad.ctypes.data, bytes(9), off_ok.ctypes.data, s1.ctypes.data, None) == INVALID_ARG
    assert L.zkv_sp1_gateway_verify_batch_dev(g, 1, None, None, 0, None, None, 0, None, None, None) == INVALID_ARG
    assert L.zkv_sp1_gateway_verify_batch(g, 0, None, None, None, None, None, None, None) == 0          # empty batch: nothing to do
    assert L.zkv_sp1_gateway_verify_batch_dev(g, 0, None, None, 0, None, None, 0, None, None, None) == 0
    assert L.zkv_sp1_gateway_last_route_counts(g, None) == INVALID_ARG
    assert L.zkv_sp1_gateway_status_abi_encode(g, 8, None, out) == INVALID_ARG
    assert L.zkv_sp1_gateway_status_abi_encode(g, 8, b'abcd', None) == INVALID_ARG
    assert L.zkv_sp1_gateway_status_abi_encode(g, 9, b'abcd', out) == INVALID_ARG
    for h in (sp, pk, g):
        raw.zkv_ctx_destroy(h)


def test_host_routing_of_single_proofs_that_reach_no_verifier(L, plonk):
    """Short proofs and unknown selectors never reach a route, so verify_proof answers them without a device."""
    vk, vh = plonk
    from stylus_zkvm_verifiers_amd import Sp1Gateway, VerifierError
    from stylus_zkvm_verifiers_amd.sp1_gateway import RouteNotFound
    gw = Sp1Gateway(True, [(vk, vh)])
    for p in (b'', b'\x01', b'\xa4\x59\x4c'):
        with pytest.raises(VerifierError) as ei:
            gw.verify_proof(bytes(32), b'', p)
        assert ei.value.status == 4
        assert gw.last_route_counts() == [0, 0, 0, 1]
    with pytest.raises(RouteNotFound) as ei:
        gw.verify_proof(bytes(32), b'pv', b'\x50\x45\xf5\x26' + bytes(256))          # the RISC Zero selector: no SP1 route
    assert ei.value.received == b'\x50\x45\xf5\x26' and ei.value.revert == gw.status_abi_encode(8, b'\x50\x45\xf5\x26')
    assert gw.last_route_counts() == [0, 0, 1, 0]
    gw.close()


def test_route_not_found_encoding_and_other_statuses(L, plonk):
    vk, vh = plonk
    from stylus_zkvm_verifiers_amd import Sp1Gateway, _lib
    raw = _lib.lib()
    for groth16, keys in ((True, [(vk, vh)]), (False, [(vk, vh)])):
        gw = Sp1Gateway(groth16, keys)
        sel = C.create_string_buffer(4)
        assert raw.zkv_abi_function_selector(b'RouteNotFound(bytes4)', sel) == 0
        rng = np.random.default_rng(7)
        for _ in range(8):
            recv = rng.integers(0, 256, 4, dtype=np.uint8).tobytes()
            assert gw.status_abi_encode(8, recv) == sel.raw + recv + bytes(28)
            exp = gw.routes()[0][0]
            for st in range(6):
                o = C.create_string_buffer(68)
                n = raw.zkv_status_abi_encode(1, st, recv, exp, o)
                assert gw.status_abi_encode(st, recv) == o.raw[:n], st
        o = C.create_string_buffer(68)
        assert raw.zkv_status_abi_encode(1, 8, b'abcd', b'abcd', o) == INVALID_ARG       # unchanged: status 8 is the gateway's alone
        gw.close()


def _direct(blob, off, sels):
    """The rule of include/zkv_sp1_gateway.h, proof by proof."""
    out = []
    for i in range(len(off) - 1):
        p = bytes(blob[int(off[i]):int(off[i + 1])])
        if len(p) < 4:
            out.append(gm.SHORT)
            continue
        out.append(next((r for r, s in enumerate(sels) if p[:4] == bytes(s)), gm.NOT_FOUND))
    return np.array(out, dtype=np.int64)


@pytest.mark.parametrize('seed', [1, 2, 3, 4])
def test_numpy_routing_model_equals_the_direct_rule(seed):
    rng = np.random.default_rng(seed)
    R = int(rng.integers(1, 9))
    sels = [rng.integers(0, 256, 4, dtype=np.uint8).tobytes() for _ in range(R)]
    n = int(rng.integers(1, 3000))
    lens = rng.choice([0, 1, 2, 3, 4, 5, 260, 868, 1000], n)
    off = np.zeros(n + 1, dtype=np.uint64); off[1:] = np.cumsum(lens)
    blob = rng.integers(0, 256, int(off[-1]), dtype=np.uint8)
    for i in range(n):
        if lens[i] >= 4 and rng.random() < 0.8:
            blob[int(off[i]):int(off[i]) + 4] = np.frombuffer(sels[int(rng.integers(0, R))], dtype=np.uint8)
    route = gm.routes(blob, off, sels)
    assert (route == _direct(blob, off, sels)).all()
    assert {gm.SHORT, gm.NOT_FOUND} <= set(route.tolist()) or n < 50
    parts = gm.partition(route, R)
    for r in range(R):
        assert parts[r].tolist() == [i for i in range(n) if route[i] == r]        # stable: caller order within a route
    c = gm.counts(route, R)
    assert sum(c) == n and c[R] == int((route == gm.NOT_FOUND).sum()) and c[R + 1] == int((lens < 4).sum())
    # expected(): in-place answers and per-route statuses scattered back to the caller's order
    per = [(np.full(len(parts[r]), r, np.uint8), np.tile(np.frombuffer(sels[r], np.uint8), (len(parts[r]), 1))) for r in range(R)]
    st, rv = gm.expected(route, blob, off, per)
    for i in range(n):
        p = bytes(blob[int(off[i]):int(off[i + 1])])
        if route[i] == gm.SHORT:
            assert st[i] == 4 and bytes(rv[i]) == bytes(4)
        elif route[i] == gm.NOT_FOUND:
            assert st[i] == 8 and bytes(rv[i]) == p[:4]
        else:
            assert st[i] == route[i] and bytes(rv[i]) == sels[route[i]]


def test_synth_interleaves_both_pools():
    from stylus_zkvm_verifiers_amd import synth
    rng = np.random.default_rng(3)
    g = (rng.integers(0, 256, (5, 260), dtype=np.uint8), rng.integers(0, 256, (5, 32), dtype=np.uint8), rng.integers(0, 256, (5, 96), dtype=np.uint8))
    p = (rng.integers(0, 256, (3, 868), dtype=np.uint8), rng.integers(0, 256, (3, 32), dtype=np.uint8), rng.integers(0, 256, (3, 96), dtype=np.uint8))
    blob, off, vk, pv, kind, row, spliced = synth.make_sp1_gateway_batch(g, p, 1000, 0.75, 11, splice_every=10, splice_selectors=[b'\xde\xad\xbe\xef'])
    assert len(off) == 1001 and 0.65 < (kind == 0).mean() < 0.85 and spliced.sum() == 100
    for i in range(1000):
        P, V, W = g if kind[i] == 0 else p
        want = bytearray(P[row[i]].tobytes())
        if spliced[i]:
            want[:4] = b'\xde\xad\xbe\xef'
        assert blob[int(off[i]):int(off[i + 1])].tobytes() == bytes(want)
        assert vk[i].tobytes() == V[row[i]].tobytes() and pv[i].tobytes() == W[row[i]].tobytes()
    b2 = synth.make_sp1_gateway_batch(g, p, 1000, 0.75, 11, splice_every=10, splice_selectors=[b'\xde\xad\xbe\xef'])[0]
    assert (b2 == blob).all()

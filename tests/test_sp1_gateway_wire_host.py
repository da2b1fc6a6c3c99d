"""eth_call batches on the SP1 gateway (include/zkv_sp1_gateway_wire.h) without a device: the header against the
library's exports, the C encoder against the model's (tests/gateway_wire_model.py), the header arithmetic the kernel runs
(csrc/zkv_wire_gateway.h, compiled for the host) against the model's strict decoder, the model against the oracle where the two overlap,
and argument handling.  PARITY UNPINNED: the reference holds no gateway, no PLONK code and no router."""
import ctypes as C
import json
import os
import random
import re
import subprocess

import numpy as np
import pytest

import gateway_wire_model as gwm
import oracle_lib as ol
from wire_util import apply_ops

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
H = bytes.fromhex
NEW = ['zkv_sp1_gateway_encode_verify_proof_call', 'zkv_sp1_gateway_eth_call_batch', 'zkv_sp1_gateway_eth_call_batch_dev',
       'zkv_sp1_gateway_eth_call_returndata', 'zkv_sp1_gateway_last_call_counts']
WRONG_CTX, INVALID_ARG = -5, -1


@pytest.fixture(scope='module')
def L():
    from stylus_zkvm_verifiers_amd import sp1_gateway_wire
    return sp1_gateway_wire.lib()


@pytest.fixture(scope='module')
def fx():
    return json.load(open(os.path.join(HERE, 'golden', 'gateway_wire_cases.json')))


@pytest.fixture(scope='module')
def model(fx):
    return gwm.Gateway(True, [(H(r['vk']), H(r['verifier_hash'])) for r in fx['routes']])


@pytest.fixture(scope='module')
def hs():
    src = os.path.join(HERE, 'host_sim', 'host_sim_gateway_wire.cpp')
    lib = os.path.join(HERE, 'host_sim', 'libhost_sim_gateway_wire.so')
    csrc = os.path.join(HERE, '..', 'stylus_zkvm_verifiers_amd', 'csrc')
    deps = [src] + [os.path.join(csrc, f) for f in os.listdir(csrc) if f.endswith('.h')]
    if not os.path.exists(lib) or os.path.getmtime(lib) < max(os.path.getmtime(d) for d in deps):
        subprocess.check_call(['g++', '-O2', '-std=c++17', '-fPIC', '-shared', '-Wno-unknown-pragmas', '-o', lib, src])
    S = C.CDLL(lib)
    S.hsgw_parse.argtypes = [C.c_char_p, C.c_uint64, C.c_uint32, C.c_uint32, C.c_uint32, C.POINTER(C.c_uint64)]
    return S


def calldata(fx, case):
    it = fx['items'][case['item']]
    cd = apply_ops(gwm.encode(case['form'], H(it['vkey']), H(it['pv']), H(it['proof'])), case['ops'])
    assert len(cd) == case['calldata_len'], case['name']
    return cd


def _c_encode(L, form, vkey, pv, proof):
    n = L.zkv_sp1_gateway_encode_verify_proof_call(form, vkey, pv, len(pv), proof, len(proof), None, 0)
    o = C.create_string_buffer(n + 1)
    o.raw = b'\xee' * (n + 1)
    assert L.zkv_sp1_gateway_encode_verify_proof_call(form, vkey, pv, len(pv), proof, len(proof), o, n) == n
    assert o.raw[n:] == b'\xee'                                  # nothing past the needed length
    short = C.create_string_buffer(n)
    short.raw = b'\xee' * n
    assert L.zkv_sp1_gateway_encode_verify_proof_call(form, vkey, pv, len(pv), proof, len(proof), short, n - 1) == n
    assert short.raw == b'\xee' * n                              # too small: untouched
    return o.raw[:n]


def _names(path):
    return set(re.findall(r'\b(zkv_[a-z0-9_]+)\s*\(', re.sub(r'/\*.*?\*/', '', open(path).read(), flags=re.S)))


def test_header_declares_the_new_symbols_and_the_library_exports_them(L):
    hdr = os.path.join(ROOT, 'include', 'zkv_sp1_gateway_wire.h')
    assert _names(hdr) == set(NEW)
    text = open(hdr).read()
    for d in ('#include "zkv_sp1_gateway.h"', '#define ZKV_CALLDATA_FORM_UINT8_ARRAY 0', '#define ZKV_CALLDATA_FORM_BYTES 1', 'PARITY UNPINNED'):
        assert d in text, d
    from stylus_zkvm_verifiers_amd import _lib, sp1_gateway, sp1_gateway_wire
    assert set(sp1_gateway_wire.SYMBOLS) == set(NEW)
    assert not set(NEW) & set(_lib.SYMBOLS) and not set(NEW) & set(sp1_gateway.SYMBOLS)
    for name in NEW:
        assert hasattr(L, name), name
    assert (sp1_gateway_wire.FORM_UINT8_ARRAY, sp1_gateway_wire.FORM_BYTES) == (gwm.FORM_U, gwm.FORM_B)


def test_selectors_are_derived_and_the_c_encoder_equals_the_models(L, fx):
    from stylus_zkvm_verifiers_amd import Sp1Gateway, _lib, sp1_gateway_wire
    raw = _lib.lib()
    for form in (gwm.FORM_U, gwm.FORM_B):
        o = C.create_string_buffer(4)
        assert raw.zkv_abi_function_selector(gwm.SIGNATURES[form], o) == 0
        assert o.raw == gwm.selector(form) == sp1_gateway_wire.selector(form)
    print('selector of %s: %s' % (gwm.SIGNATURES[gwm.FORM_B].decode(), gwm.selector(gwm.FORM_B).hex()))
    assert gwm.selector(gwm.FORM_U) != gwm.selector(gwm.FORM_B)
    assert {len(H(it['pv'])) for it in fx['items']} >= {0, 1, 31, 32, 33, 96}
    assert {len(H(it['proof'])) for it in fx['items']} >= {0, 1, 2, 3, 4, 259, 260, 261, 867, 868, 869}
    for it in fx['items']:
        vkey, pv, proof = H(it['vkey']), H(it['pv']), H(it['proof'])
        for form in (gwm.FORM_U, gwm.FORM_B):
            want = gwm.encode(form, vkey, pv, proof)
            assert _c_encode(L, form, vkey, pv, proof) == want, (it['name'], form)
            assert gwm.decode(want) == (form, vkey, pv, proof)
        assert gwm.encode(gwm.FORM_U, vkey, pv, proof) == ol.sp1_encode_call(vkey, pv, proof)      # form U is the single verifier's encoding
        assert len(gwm.encode(gwm.FORM_B, vkey, pv, proof)) == 4 + 96 + 32 + gwm.pad32(len(pv)) + 32 + gwm.pad32(len(proof))
    it = fx['items'][0]
    assert Sp1Gateway.encode_verify_proof_call(H(it['vkey']), H(it['pv']), H(it['proof']), form=0) == gwm.encode(0, H(it['vkey']), H(it['pv']), H(it['proof']))
    assert Sp1Gateway.encode_verify_proof_call(H(it['vkey']), H(it['pv']), H(it['proof'])) == gwm.encode(1, H(it['vkey']), H(it['pv']), H(it['proof']))
    assert L.zkv_sp1_gateway_encode_verify_proof_call(2, bytes(32), b'', 0, b'', 0, None, 0) == 0     # no such form
    with pytest.raises(ValueError):
        Sp1Gateway.encode_verify_proof_call(bytes(32), b'', b'', form=2)


def test_fixture_holds_the_models_answers_and_covers_the_ground(fx, model):
    cols = set()
    for c in fx['cases']:
        rev, data, st, rv, col = model.eth_call(calldata(fx, c))
        assert (int(rev), data.hex(), st, rv.hex(), col) == (c['reverted'], c['returndata'], c['status'], c['received'], c['column']), c['name']
        assert len(data) <= 96 and (st == 0) == (not rev)
        cols.add((c['form'], col))
    assert cols == {(f, k) for f in (0, 1) for k in (0, 1, 2, -1, -2, gwm.BAD)}
    for form in (0, 1):
        ok = {c['column'] for c in fx['cases'] if c['form'] == form and c['status'] == 0}
        assert ok == {0, 1, 2}                                   # a valid proof through every route, in either form
        assert {c['status'] for c in fx['cases'] if c['form'] == form} == {0, 1, 4, 6, 8}


def _parse(hs, cd, shift=0):
    out = (C.c_uint64 * 6)()
    su, sb = (int.from_bytes(gwm.selector(f), 'big') for f in (gwm.FORM_U, gwm.FORM_B))
    assert hs.hsgw_parse(bytes(cd) + b'\0', len(cd), shift, su, sb, out) == 0
    return None if not out[0] else (out[1], out[4], out[2], out[5], out[3])      # the model's order: form, pv_at, pv_len, proof_at, proof_len


def test_kernel_header_arithmetic_equals_the_model_decoder(hs, fx):
    """The function k_wire_gateway calls, on every golden case and on seeded single-word mutations of canonical headers (length words
    near 2^32 and 2^64 included), from an aligned and from an unaligned start."""
    n_bad = 0
    for c in fx['cases']:
        cd = calldata(fx, c)
        want = gwm.parse_header(cd)
        for shift in (0, 1, 2, 3):
            assert _parse(hs, cd, shift) == want, (c['name'], shift)
        if want is None:
            assert c['status'] == 6
        n_bad += want is None
    assert n_bad > 50
    rng = random.Random(0x6A7E7174)
    seen = {True: 0, False: 0}
    for trial in range(4000):
        form = rng.randrange(2)
        pv = bytes(rng.randrange(256) for _ in range(rng.choice([0, 1, 5, 31, 32, 33, 40])))
        proof = bytes(rng.randrange(256) for _ in range(rng.choice([0, 3, 4, 31, 32, 33, 64, 70])))
        cd = bytearray(gwm.encode(form, bytes(32), pv, proof))
        second = 132 + (32 * len(pv) if form == 0 else gwm.pad32(len(pv)))
        at = rng.choice([36, 68, 100, second])
        cur = int.from_bytes(cd[at:at + 32], 'big')
        val = rng.choice([0, 1, 31, 32, 33, 0x60, 0x80, cur, cur + 1, cur - 1, cur + 32, cur - 32, cur + (1 << 32), cur + (1 << 64), cur + (1 << 248), (1 << 32) - 1, 1 << 32,
                          (1 << 32) + 1, (1 << 32) - 32, (1 << 37) - 32, (1 << 59), (1 << 63), (1 << 64) - 1, 1 << 64, (1 << 64) - 32, (1 << 64) + 0x60,
                          (1 << 256) - 1, (1 << 256) - 32, rng.randrange(200), rng.randrange(1 << 256)]) % (1 << 256)
        cd[at:at + 32] = val.to_bytes(32, 'big')
        edit = rng.randrange(8)
        if edit == 0:
            del cd[len(cd) - rng.choice([1, 31, 32, 33]):]
        elif edit == 1:
            cd += bytes(rng.choice([1, 31, 32, 33]))
        want = gwm.parse_header(cd)
        assert _parse(hs, cd, trial & 3) == want, (trial, form, at, hex(val))
        seen[want is None] += 1
    assert seen[True] > 3000 and seen[False] > 100


def test_model_equals_the_oracle_on_form_u_calls_with_the_groth16_selector(fx, model):
    """Where the unpinned model and the oracle overlap: a form U call is the single SP1 verifier's calldata, and a proof that carries the
    Groth16 selector reaches, on the gateway, the verifier the oracle's shell holds."""
    sel_u, n, statuses = gwm.selector(gwm.FORM_U), 0, set()
    for c in fx['cases']:
        it = fx['items'][c['item']]
        if c['form'] != gwm.FORM_U or H(it['proof'])[:4] != model.selectors[0]:
            continue
        cd = calldata(fx, c)
        if cd[:4] != sel_u:                                      # another method: the shell has getters, the gateway has none
            continue
        rev, data, st = ol.sp1_eth_call(cd)
        assert st == c['status'], c['name']
        assert (int(rev), data.hex()) == (c['reverted'], c['returndata']), c['name']
        n += 1; statuses.add(st)
    assert n >= 40 and statuses >= {0, 1, 4, 6}


def test_wrong_contexts_bad_arguments_and_empty_batches(L, fx):
    from stylus_zkvm_verifiers_amd import _lib
    raw = _lib.lib()
    r = fx['routes'][0]
    vk, vh = H(r['vk']), H(r['verifier_hash'])
    sp = raw.zkv_sp1_ctx_create(0)
    pk = raw.zkv_sp1_plonk_ctx_create(vk, len(vk), vh, 0)
    out = C.create_string_buffer(96); ln = C.c_uint32(7); rev = C.c_uint8(7); cnt = (C.c_uint64 * 11)()
    for h in (None, sp, pk):
        assert L.zkv_sp1_gateway_eth_call_batch(h, 0, None, None, None, None, None, None) == WRONG_CTX
        assert L.zkv_sp1_gateway_eth_call_batch_dev(h, 0, None, None, 0, None, None, None) == WRONG_CTX
        assert L.zkv_sp1_gateway_eth_call_returndata(h, 0, bytes(4), out, C.byref(ln), C.byref(rev)) == WRONG_CTX
        assert L.zkv_sp1_gateway_last_call_counts(h, cnt) == WRONG_CTX
    from stylus_zkvm_verifiers_amd import Sp1Gateway
    gw = Sp1Gateway(True, [(vk, vh)])
    g = gw._h
    # the single verifiers' calldata entry points still refuse a gateway
    assert raw.zkv_sp1_eth_call_batch(g, 0, None, None, None, None, None, None) == WRONG_CTX
    assert raw.zkv_eth_call_batch_dev(g, 0, None, None, 0, None, None, None) == WRONG_CTX
    assert L.zkv_sp1_gateway_eth_call_batch(g, 0, None, None, None, None, None, None) == 0             # empty batch: nothing to do
    assert L.zkv_sp1_gateway_eth_call_batch_dev(g, 0, None, None, 0, None, None, None) == 0
    assert gw.eth_call_batch([])[1] == []
    blob = bytes(64)
    ok = np.array([0, 8], dtype=np.uint64); back = np.array([8, 4], dtype=np.uint64)
    r1 = np.zeros(1, np.uint8); d1 = np.zeros(96, np.uint8); l1 = np.zeros(1, np.uint32); s1 = np.zeros(1, np.uint8)
    P = lambda a: a.ctypes.data
    assert L.zkv_sp1_gateway_eth_call_batch(g, 1, None, P(ok), P(r1), P(d1), P(l1), P(s1)) == INVALID_ARG
    assert L.zkv_sp1_gateway_eth_call_batch(g, 1, blob, None, P(r1), P(d1), P(l1), P(s1)) == INVALID_ARG
    assert L.zkv_sp1_gateway_eth_call_batch(g, 1, blob, P(ok), None, P(d1), P(l1), P(s1)) == INVALID_ARG
    assert L.zkv_sp1_gateway_eth_call_batch(g, 1, blob, P(ok), P(r1), None, P(l1), P(s1)) == INVALID_ARG
    assert L.zkv_sp1_gateway_eth_call_batch(g, 1, blob, P(ok), P(r1), P(d1), None, P(s1)) == INVALID_ARG
    assert L.zkv_sp1_gateway_eth_call_batch(g, 1, blob, P(back), P(r1), P(d1), P(l1), P(s1)) == INVALID_ARG      # host offsets not monotone
    assert L.zkv_sp1_gateway_eth_call_batch(g, 0xFFFFFFF1, blob, P(ok), P(r1), P(d1), P(l1), P(s1)) == INVALID_ARG
    assert L.zkv_sp1_gateway_eth_call_batch_dev(g, 1, None, 8, 64, 8, None, None) == INVALID_ARG
    assert L.zkv_sp1_gateway_eth_call_batch_dev(g, 1, 8, None, 64, 8, None, None) == INVALID_ARG
    assert L.zkv_sp1_gateway_eth_call_batch_dev(g, 1, 8, 8, 64, None, None, None) == INVALID_ARG
    assert L.zkv_sp1_gateway_eth_call_batch_dev(g, 0xFFFFFFF1, 8, 8, 64, 8, None, None) == INVALID_ARG
    assert L.zkv_sp1_gateway_last_call_counts(g, None) == INVALID_ARG
    assert L.zkv_sp1_gateway_eth_call_returndata(g, 0, bytes(4), None, C.byref(ln), C.byref(rev)) == INVALID_ARG
    assert L.zkv_sp1_gateway_eth_call_returndata(g, 0, bytes(4), out, None, C.byref(rev)) == INVALID_ARG
    assert L.zkv_sp1_gateway_eth_call_returndata(g, 0, bytes(4), out, C.byref(ln), None) == INVALID_ARG
    assert gw.last_call_counts() == [0, 0, 0, 0, 0]              # two routes, not found, short, bad calldata
    # a decoded-input call fills the old columns and leaves the new one at zero
    with pytest.raises(Exception):
        gw.verify_proof(bytes(32), b'', b'ab')
    assert gw.last_route_counts() == [0, 0, 0, 1] and gw.last_call_counts() == [0, 0, 0, 1, 0]
    f = C.c_float(0)
    assert raw.zkv_ctx_last_wire_ms(g, C.byref(f)) == -2         # no eth_call batch has run (no device was touched)
    gw.close()
    for h in (sp, pk):
        raw.zkv_ctx_destroy(h)


def test_returndata_of_every_status(L, fx, model):
    from stylus_zkvm_verifiers_amd import Sp1Gateway
    gw = Sp1Gateway(True, [(H(r['vk']), H(r['verifier_hash'])) for r in fx['routes']])
    assert [s for s, _, _ in gw.routes()] == model.selectors
    recv = b'\x12\x34\x56\x78'
    for st in range(256):
        out = C.create_string_buffer(b'\xee' * 97); ln = C.c_uint32(77); rev = C.c_uint8(77)
        rc = L.zkv_sp1_gateway_eth_call_returndata(gw._h, st, recv, out, C.byref(ln), C.byref(rev))
        assert out.raw[96:97] == b'\xee'
        if st == 0:
            assert (rc, rev.value, ln.value) == (0, 0, 0)
        elif st == 6:
            assert (rc, rev.value, ln.value) == (0, 1, 0)
        else:
            enc = C.create_string_buffer(68)
            k = L.zkv_sp1_gateway_status_abi_encode(gw._h, st, recv, enc)
            if k < 0:
                assert rc == k == INVALID_ARG, st
                continue
            assert (rc, rev.value, out.raw[:ln.value]) == (0, 1, enc.raw[:k]), st
        if st in (0, 1, 4, 6, 8):                                # what a gateway reports
            assert (bool(rev.value), out.raw[:ln.value]) == model.returndata(st, recv) == gw.eth_call_returndata(st, recv), st
    # NULL received selector: zeros
    out = C.create_string_buffer(96); ln = C.c_uint32(0); rev = C.c_uint8(0)
    assert L.zkv_sp1_gateway_eth_call_returndata(gw._h, 8, None, out, C.byref(ln), C.byref(rev)) == 0
    assert (True, out.raw[:ln.value]) == model.returndata(8, bytes(4))
    gw.close()

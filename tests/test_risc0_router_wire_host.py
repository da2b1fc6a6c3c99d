"""eth_call batches and per-seal methods on the RISC Zero router (include/zkv_risc0_router_wire.h) without a
device: the header against the library's exports, the derived selectors, the C encoders against the model's
(tests/risc0_router_wire_model.py) and against zkv.h's, the fixture against the model, return data, argument handling, and a stand-alone
host program (tests/host_sim/host_sim_rzrouter_wire.cpp, plain and under the sanitizers, as a child process) that runs the header
arithmetic of k_wire_rzrouter and the per-slot method choice of the keyed PREP body.  PARITY UNPINNED: the reference holds no router."""
import ctypes as C
import json
import os
import random
import re
import subprocess
import sys

import numpy as np
import pytest

import risc0_router_model as rm
import risc0_router_wire_model as wm
import spec_model as m
from wire_util import apply_ops

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, os.path.join(HERE, 'golden'))
import make_risc0_router_wire_cases as gen          # noqa: E402  (the item -> calldata rule of the fixture)

SRC = os.path.join(HERE, 'host_sim', 'host_sim_rzrouter_wire.cpp')
H = bytes.fromhex
NEW = ['zkv_risc0_router_verify_call_batch', 'zkv_risc0_router_verify_call_batch_dev', 'zkv_risc0_router_encode_verify_call',
       'zkv_risc0_router_encode_verify_integrity_call', 'zkv_risc0_router_eth_call_batch', 'zkv_risc0_router_eth_call_batch_dev',
       'zkv_risc0_router_eth_call_returndata', 'zkv_risc0_router_last_call_counts']
WRONG_CTX, INVALID_ARG, NO_DEVICE = -5, -1, -2
SANITIZE = ['-fsanitize=address,undefined', '-fno-sanitize-recover=all']
LENGTHS = {0, 3, 4, 256, 257, 259, 260, 261, 292}
SHAPES = [(f, t) for f in (0, 1) for t in (0, 1)]


@pytest.fixture(scope='module')
def L():
    from stylus_zkvm_verifiers_amd import risc0_router_wire
    return risc0_router_wire.lib()


@pytest.fixture(scope='module')
def fx():
    return json.load(open(os.path.join(HERE, 'golden', 'risc0_router_wire_cases.json')))


@pytest.fixture(scope='module')
def keys(fx):
    return [rm.Key(s) for s in fx['key_seeds']]


@pytest.fixture(scope='module')
def model(fx, keys):
    b = fx['builtin']
    w = wm.WireRouter(rm.Router([(H(b['control_root']), H(b['bn254_control_id']))], [k.triple() for k in keys]))
    assert [s.hex() for s in w.selectors] == fx['route_selectors']
    return w


@pytest.fixture()
def router(fx, keys):
    from stylus_zkvm_verifiers_amd import RiscZeroRouter
    b = fx['builtin']
    r = RiscZeroRouter([(H(b['control_root']), H(b['bn254_control_id']))], [k.triple() for k in keys])
    yield r
    r.close()


def calldata(fx, case):
    cd = gen.calldata_of(fx['items'][case['item']], case['form'], case['method'], case['ops'])
    assert len(cd) == case['calldata_len'], case['name']
    return cd


def _names(path):
    return set(re.findall(r'\b(zkv_[a-z0-9_]+)\s*\(', re.sub(r'/\*.*?\*/', '', open(path).read(), flags=re.S)))


def test_header_declares_the_new_symbols_and_the_library_exports_them(L):
    hdr = os.path.join(ROOT, 'include', 'zkv_risc0_router_wire.h')
    assert _names(hdr) == set(NEW)
    text = open(hdr).read()
    for d in ('#include "zkv_risc0_router.h"', '#define ZKV_CALLDATA_FORM_UINT8_ARRAY 0', '#define ZKV_CALLDATA_FORM_BYTES 1', 'PARITY UNPINNED'):
        assert d in text, d
    from stylus_zkvm_verifiers_amd import _lib, risc0_router, risc0_router_wire
    assert set(risc0_router_wire.SYMBOLS) == set(NEW)
    assert not set(NEW) & set(_lib.SYMBOLS) and not set(NEW) & set(risc0_router.SYMBOLS)
    for name in NEW:
        assert hasattr(L, name), name
    assert (risc0_router_wire.FORM_UINT8_ARRAY, risc0_router_wire.FORM_BYTES) == (wm.FORM_U, wm.FORM_B)
    assert (risc0_router_wire.METHOD_VERIFY, risc0_router_wire.METHOD_VERIFY_INTEGRITY, risc0_router_wire.CALL_KIND_BAD) == (wm.VERIFY, wm.INTEGRITY, wm.KIND_BAD)
    # the two forms mean the same in both wire headers
    other = os.path.join(ROOT, 'include', 'zkv_sp1_gateway_wire.h')
    for first, second in ((hdr, other), (other, hdr)):
        src = '#include "%s"\n#include "%s"\nint main(void) { return ZKV_CALLDATA_FORM_BYTES - 1; }\n' % (first, second)
        subprocess.run(['gcc', '-x', 'c', '-fsyntax-only', '-Wall', '-Werror', '-'], input=src.encode(), check=True)


def test_selectors_are_derived(L):
    from stylus_zkvm_verifiers_amd import _lib, risc0_router_wire
    raw = _lib.lib()
    want = {(1, 0): 'ab750e75', (1, 1): '1599ead5', (0, 0): 'f8b3b60b', (0, 1): 'a5a5c637'}     # the first two: the public on-chain values
    for form, method in SHAPES:
        o = C.create_string_buffer(4)
        assert raw.zkv_abi_function_selector(wm.SIGNATURES[2 * form + method], o) == 0
        assert o.raw == wm.selector(form, method) == risc0_router_wire.selector(form, method) == H(want[form, method])
        assert risc0_router_wire.SIGNATURES[2 * form + method] == wm.SIGNATURES[2 * form + method]


def _c_encode(fn, *args):
    n = fn(*args, None, 0)
    o = C.create_string_buffer(n + 1)
    o.raw = b'\xee' * (n + 1)
    assert fn(*args, o, n) == n
    assert o.raw[n:] == b'\xee'                                  # nothing past the needed length
    short = C.create_string_buffer(n)
    short.raw = b'\xee' * n
    assert fn(*args, short, n - 1) == n
    assert short.raw == b'\xee' * n                              # too small: untouched
    return o.raw[:n]


def test_c_encoders_equal_the_models_and_form_u_is_the_single_verifiers(L, fx):
    from stylus_zkvm_verifiers_amd import RiscZeroRouter, _lib
    raw = _lib.lib()
    raw.zkv_risc0_encode_verify_call.restype = C.c_size_t
    raw.zkv_risc0_encode_verify_integrity_call.restype = C.c_size_t
    assert {len(H(it['seal'])) for it in fx['items']} >= LENGTHS
    for it in fx['items']:
        seal, a, b = H(it['seal']), H(it['image_id']), H(it['journal_digest'])
        claim = m.receipt_claim_ok_digest(a, b)
        for form in (wm.FORM_U, wm.FORM_B):
            want = wm.encode(form, wm.VERIFY, seal, a, b)
            assert _c_encode(L.zkv_risc0_router_encode_verify_call, form, seal, len(seal), a, b) == want, (it['name'], form)
            assert wm.decode(want) == (form, wm.VERIFY, seal, a, b)
            assert RiscZeroRouter.encode_verify_call(seal, a, b, form=form) == want
            want = wm.encode(form, wm.INTEGRITY, seal, claim)
            assert _c_encode(L.zkv_risc0_router_encode_verify_integrity_call, form, seal, len(seal), claim) == want, (it['name'], form)
            assert wm.decode(want) == (form, wm.INTEGRITY, seal, claim, None)
            assert RiscZeroRouter.encode_verify_integrity_call(seal, claim, form=form) == want
        assert wm.encode(wm.FORM_U, wm.VERIFY, seal, a, b) == _c_encode(raw.zkv_risc0_encode_verify_call, seal, len(seal), a, b)
        assert wm.encode(wm.FORM_U, wm.INTEGRITY, seal, claim) == _c_encode(raw.zkv_risc0_encode_verify_integrity_call, seal, len(seal), claim)
        assert len(wm.encode(wm.FORM_B, wm.VERIFY, seal, a, b)) == len(wm.encode(wm.FORM_B, wm.INTEGRITY, seal, claim)) == 132 + wm.pad32(len(seal))
    it = fx['items'][0]
    assert RiscZeroRouter.encode_verify_call(H(it['seal']), H(it['image_id']), H(it['journal_digest']))[:4] == H('ab750e75')     # form B is the default
    assert L.zkv_risc0_router_encode_verify_call(2, b'', 0, bytes(32), bytes(32), None, 0) == 0          # no such form
    assert L.zkv_risc0_router_encode_verify_integrity_call(-1, b'', 0, bytes(32), None, 0) == 0
    with pytest.raises(ValueError):
        RiscZeroRouter.encode_verify_call(b'', bytes(32), bytes(32), form=2)
    with pytest.raises(ValueError):
        RiscZeroRouter.encode_verify_integrity_call(b'', bytes(31))


def test_fixture_holds_the_models_answers_and_covers_the_ground(fx, model):
    """With the model alone: every case's recorded answer, and everything the fixture has to hold in every one of the four shapes."""
    cases = fx['cases']
    cols = []
    for c in cases:
        rev, data, st, rv, col, kind = model.eth_call(calldata(fx, c))
        assert (int(rev), data.hex(), st, rv.hex(), col, kind) == (c['reverted'], c['returndata'], c['status'], c['received'], c['column'], c['kind']), c['name']
        assert len(data) <= 96 and (st == 0) == (not rev) and (kind == wm.KIND_BAD) == (st == 6) == (col == wm.BAD)
        assert kind in (wm.KIND_BAD, 2 * c['form'] + c['method'])
        cols.append(col)
    assert {c['status'] for c in cases} == {0, 1, 4, 6, 8}
    assert all(x > 0 for x in model.counts(cols)) and len(model.counts(cols)) == 3 + 3
    for form, method in SHAPES:
        mine = [c for c in cases if (c['form'], c['method']) == (form, method)]
        plain = [c for c in mine if not c['ops']]
        assert {c['column'] for c in mine if c['status'] == 0} == {0, 1, 2}                  # one OK per route: the built-in group and the keyed group
        assert {len(H(fx['items'][c['item']]['seal'])) for c in plain} >= LENGTHS
        assert {c['status'] for c in mine} == {0, 1, 4, 6, 8}
        assert {(c['status'], c['column']) for c in plain} >= {(8, rm.NOT_FOUND), (4, rm.SHORT), (1, 0), (1, 2), (4, 0), (4, 1)}
        names = ' | '.join(c['name'] for c in mine if c['status'] == 6)
        need = ['unknown function selector', "the other form's selector", "the other method's selector", 'cut to 0 bytes', 'cut to 3 bytes', 'cut to 4 bytes',
                'offset 32 more', 'offset with a high byte', 'length + 2^32', 'length + 2^255', 'length more than present', 'length less than present',
                'last byte missing', 'one trailing byte', 'getVerifier(bytes4)']
        need += ['first element 256 more', 'last element 256 more', 'element 260 of 261', 'element 291 of 292'] if form == wm.FORM_U else \
                ['first padding byte set', 'last padding byte set', 'first padding byte set [built-in route, seal of 261', 'last padding byte set [keyed route 0, seal of 292']
        if (form, method) == (wm.FORM_B, wm.INTEGRITY):
            need += ['seal offset in the tuple 0x60']
        for t in need:
            assert t in names, (form, method, t)
        # every malformed case changes a call that would verify
        for c in mine:
            if c['ops'] and '[' in c['name'] and 'seal of' not in c['name']:
                assert c['status'] == 6, c['name']


def test_returndata_of_every_status_and_call_kind(L, model, router):
    assert [s for s, _, _ in router.routes()] == model.selectors
    recv = b'\x12\x34\x56\x78'
    for kind in (0, 1, 2, 3, 4, 254, 255):
        for st in range(256):
            out = C.create_string_buffer(b'\xee' * 97); ln = C.c_uint32(77); rev = C.c_uint8(77)
            rc = L.zkv_risc0_router_eth_call_returndata(router._h, st, recv, kind, out, C.byref(ln), C.byref(rev))
            assert out.raw[96:97] == b'\xee'
            if st == 6:
                assert (rc, rev.value, ln.value) == (0, 1, 0)
            elif kind > 3:
                assert rc == INVALID_ARG
                continue
            elif st == 0:
                assert (rc, rev.value, out.raw[:ln.value]) == (0, 0, (1).to_bytes(32, 'big') if kind < 2 else b''), kind
            else:
                enc = C.create_string_buffer(68)
                k = L.zkv_risc0_router_status_abi_encode(router._h, st, recv, enc)
                if k < 0:
                    assert rc == k == INVALID_ARG, st
                    continue
                assert (rc, rev.value, out.raw[:ln.value]) == (0, 1, enc.raw[:k]), st
            if st in (0, 1, 4, 6, 8):                            # what a router reports
                assert (bool(rev.value), out.raw[:ln.value]) == model.returndata(st, recv, kind) == router.eth_call_returndata(st, recv, kind), (st, kind)
    out = C.create_string_buffer(96); ln = C.c_uint32(0); rev = C.c_uint8(0)
    assert L.zkv_risc0_router_eth_call_returndata(router._h, 8, None, 2, out, C.byref(ln), C.byref(rev)) == 0      # NULL received selector: zeros
    assert (True, out.raw[:ln.value]) == model.returndata(8, bytes(4), 2)


def test_wrong_contexts_bad_arguments_and_empty_batches(L, router):
    from stylus_zkvm_verifiers_amd import _lib
    raw = _lib.lib()
    rz = raw.zkv_risc0_ctx_create(bytes(32), bytes(32), 0)
    sp = raw.zkv_sp1_ctx_create(0)
    out = C.create_string_buffer(96); ln = C.c_uint32(7); rev = C.c_uint8(7); cnt = (C.c_uint64 * 40)()
    for h in (None, rz, sp):
        assert L.zkv_risc0_router_verify_call_batch(h, 0, None, None, None, None, None, None, None) == WRONG_CTX
        assert L.zkv_risc0_router_verify_call_batch_dev(h, 0, None, None, None, None, None, None, None) == WRONG_CTX
        assert L.zkv_risc0_router_eth_call_batch(h, 0, None, None, None, None, None, None) == WRONG_CTX
        assert L.zkv_risc0_router_eth_call_batch_dev(h, 0, None, None, 0, None, None, None, None) == WRONG_CTX
        assert L.zkv_risc0_router_eth_call_returndata(h, 0, bytes(4), 0, out, C.byref(ln), C.byref(rev)) == WRONG_CTX
        assert L.zkv_risc0_router_last_call_counts(h, cnt) == WRONG_CTX
    g = router._h
    # the single verifiers' calldata entry points still refuse a router
    assert raw.zkv_risc0_eth_call_batch(g, 0, None, None, None, None, None, None) == WRONG_CTX
    assert raw.zkv_eth_call_batch_dev(g, 0, None, None, 0, None, None, None) == WRONG_CTX
    assert L.zkv_risc0_router_eth_call_batch(g, 0, None, None, None, None, None, None) == 0              # empty batches: nothing to do
    assert L.zkv_risc0_router_eth_call_batch_dev(g, 0, None, None, 0, None, None, None, None) == 0
    assert L.zkv_risc0_router_verify_call_batch(g, 0, None, None, None, None, None, None, None) == 0
    assert L.zkv_risc0_router_verify_call_batch_dev(g, 0, None, None, None, None, None, None, None) == 0
    assert router.eth_call_batch([])[1] == [] and len(router.verify_call_batch(None, [], [], [])[0]) == 0
    blob = bytes(64)
    ok = np.array([0, 8], dtype=np.uint64); back = np.array([8, 4], dtype=np.uint64)
    r1 = np.zeros(1, np.uint8); d1 = np.zeros(96, np.uint8); l1 = np.zeros(1, np.uint32); s1 = np.zeros(1, np.uint8); v1 = np.zeros(4, np.uint8)
    a32 = np.zeros(32, np.uint8)
    P = lambda a: a.ctypes.data
    assert L.zkv_risc0_router_eth_call_batch(g, 1, None, P(ok), P(r1), P(d1), P(l1), P(s1)) == INVALID_ARG
    assert L.zkv_risc0_router_eth_call_batch(g, 1, blob, None, P(r1), P(d1), P(l1), P(s1)) == INVALID_ARG
    assert L.zkv_risc0_router_eth_call_batch(g, 1, blob, P(ok), None, P(d1), P(l1), P(s1)) == INVALID_ARG
    assert L.zkv_risc0_router_eth_call_batch(g, 1, blob, P(ok), P(r1), None, P(l1), P(s1)) == INVALID_ARG
    assert L.zkv_risc0_router_eth_call_batch(g, 1, blob, P(ok), P(r1), P(d1), None, P(s1)) == INVALID_ARG
    assert L.zkv_risc0_router_eth_call_batch(g, 1, blob, P(back), P(r1), P(d1), P(l1), P(s1)) == INVALID_ARG     # host offsets not monotone
    assert L.zkv_risc0_router_eth_call_batch(g, 0xFFFFFFF1, blob, P(ok), P(r1), P(d1), P(l1), P(s1)) == INVALID_ARG
    assert L.zkv_risc0_router_eth_call_batch_dev(g, 1, None, 8, 64, 8, None, None, None) == INVALID_ARG
    assert L.zkv_risc0_router_eth_call_batch_dev(g, 1, 8, None, 64, 8, None, None, None) == INVALID_ARG
    assert L.zkv_risc0_router_eth_call_batch_dev(g, 1, 8, 8, 64, None, None, None, None) == INVALID_ARG
    assert L.zkv_risc0_router_eth_call_batch_dev(g, 0xFFFFFFF1, 8, 8, 64, 8, None, None, None) == INVALID_ARG
    for miss in range(4):                                        # seals, offsets, in_a, in_b, status: none may be NULL (the method row may)
        args = [blob, P(ok), P(a32), P(a32), P(s1)]
        args[miss] = None
        assert L.zkv_risc0_router_verify_call_batch(g, 1, None, args[0], args[1], args[2], args[3], args[4], P(v1)) == INVALID_ARG, miss
    assert L.zkv_risc0_router_verify_call_batch(g, 1, None, blob, P(ok), P(a32), P(a32), None, P(v1)) == INVALID_ARG
    assert L.zkv_risc0_router_verify_call_batch(g, 1, None, blob, P(back), P(a32), P(a32), P(s1), P(v1)) == INVALID_ARG
    for miss in range(4):
        args = [8, 8, 8, 8]
        args[miss] = None
        assert L.zkv_risc0_router_verify_call_batch_dev(g, 1, None, args[0], args[1], args[2], args[3], None, None) == INVALID_ARG, miss
    assert L.zkv_risc0_router_verify_call_batch_dev(g, 0xFFFFFFF1, None, 8, 8, 8, 8, None, None) == INVALID_ARG
    assert L.zkv_risc0_router_last_call_counts(g, None) == INVALID_ARG
    assert L.zkv_risc0_router_eth_call_returndata(g, 0, bytes(4), 0, None, C.byref(ln), C.byref(rev)) == INVALID_ARG
    assert L.zkv_risc0_router_eth_call_returndata(g, 0, bytes(4), 0, out, None, C.byref(rev)) == INVALID_ARG
    assert L.zkv_risc0_router_eth_call_returndata(g, 0, bytes(4), 0, out, C.byref(ln), None) == INVALID_ARG
    assert router.last_call_counts() == [0] * 6 and router.last_route_counts() == [0] * 5     # three routes, unknown, short(, bad calldata)
    f = C.c_float(0)
    assert raw.zkv_ctx_last_wire_ms(g, C.byref(f)) == NO_DEVICE      # no eth_call batch has run (no device was touched)
    for h in (rz, sp):
        raw.zkv_ctx_destroy(h)


# ---------------------------------------------------------------- the host program
def _program(tmp_path, flags, name):
    exe = str(tmp_path / name)
    subprocess.check_call(['g++', '-std=c++17', '-O1', '-g', '-Wno-unknown-pragmas'] + flags + ['-o', exe, SRC])
    return exe


def _run(exe, mode, lines):
    out = subprocess.run([exe, mode], input=''.join(ln + '\n' for ln in lines).encode(), stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120)
    assert out.returncode == 0, (out.returncode, out.stderr.decode()[-2000:])
    assert not out.stderr, out.stderr.decode()[-2000:]
    got = out.stdout.decode().splitlines()
    assert len(got) == len(lines)
    return got


def _mutations():
    """4,000 seeded single-word mutations of canonical headers (length and offset words near 2^32 and 2^64 included), some of them cut or
    extended, as (shift, calldata)."""
    rng = random.Random(0x7A7E7176)
    out = []
    for trial in range(4000):
        form, method = rng.randrange(2), rng.randrange(2)
        seal = bytes(rng.randrange(256) for _ in range(rng.choice([0, 3, 4, 31, 32, 33, 64, 70])))
        cd = bytearray(wm.encode(form, method, seal, bytes(32), bytes(32) if method == wm.VERIFY else None))
        l_at = 68 if (form, method) == (0, 1) else 100
        at = rng.choice([4, 36, l_at, l_at])
        cur = int.from_bytes(cd[at:at + 32], 'big')
        val = rng.choice([0, 1, 31, 32, 33, 0x20, 0x40, 0x60, 0x80, cur, cur + 1, cur - 1, cur + 32, cur - 32, cur + (1 << 32), cur + (1 << 64), cur + (1 << 248),
                          (1 << 32) - 1, 1 << 32, (1 << 32) + 1, (1 << 32) - 32, (1 << 37) - 32, (1 << 59), (1 << 63), (1 << 64) - 1, 1 << 64, (1 << 64) - 32,
                          (1 << 64) + 0x60, (1 << 256) - 1, (1 << 256) - 32, rng.randrange(200), rng.randrange(1 << 256)]) % (1 << 256)
        cd[at:at + 32] = val.to_bytes(32, 'big')
        edit = rng.randrange(8)
        if edit == 0:
            del cd[len(cd) - rng.choice([1, 31, 32, 33]):]
        elif edit == 1:
            cd += bytes(rng.choice([1, 31, 32, 33]))
        out.append((trial & 3, bytes(cd)))
    return out


@pytest.mark.parametrize('flags,name', [([], 'plain'), (SANITIZE, 'san')])
def test_kernel_header_arithmetic_equals_the_model_decoder(tmp_path, fx, flags, name):
    """The function k_wire_rzrouter calls, on every golden request (four alignments) and on the seeded mutations."""
    exe = _program(tmp_path, flags, name)
    sels = ' '.join(wm.selector(k >> 1, k & 1).hex() for k in range(4))
    reqs = [(shift, calldata(fx, c)) for c in fx['cases'] for shift in (0, 1, 2, 3)] + _mutations()
    got = _run(exe, 'parse', ['%d %s %s' % (shift, sels, cd.hex() or '-') for shift, cd in reqs])
    seen = {True: 0, False: 0}
    for (shift, cd), line in zip(reqs, got):
        h = wm.parse_header(cd)
        want = '0 0 0 0 0 0' if h is None else '1 %d %d %d %d %d' % (h[0], h[1], h[4], h[2], h[3])
        assert line == want, (shift, cd[:140].hex(), len(cd))
        seen[h is None] += 1
    assert seen[True] > 3000 and seen[False] > 400
    # a header the function accepts is a request the model decodes unless an element or a padding byte is wrong
    for c in fx['cases']:
        if wm.parse_header(calldata(fx, c)) is None:
            assert c['status'] == 6


@pytest.mark.parametrize('flags,name', [([], 'plain'), (SANITIZE, 'san')])
def test_per_slot_method_choice_of_the_keyed_prep_body_equals_the_model(tmp_path, keys, flags, name):
    """rzrouter_slot_in_b in front of rzrouter_prep_slot: a group of slots with a method row that mixes verify and verifyIntegrity, the
    same group with no method row (one method: the journal-digest row present or absent), and rows whose journal digest must not be read."""
    exe = _program(tmp_path, flags, name)
    key = keys[0]
    rng = random.Random(0x17A4)
    n = 6
    ids = [bytes(rng.randrange(256) for _ in range(32)) for _ in range(n)]
    jds = [bytes(rng.randrange(256) for _ in range(32)) for _ in range(n)]
    kinds = [0, 1, 1, 0, 1, 0]
    in_a = [ids[j] if kinds[j] == 0 else m.receipt_claim_ok_digest(ids[j], jds[j]) for j in range(n)]
    seals = [key.prove(ids[j], jds[j]) for j in range(n)]
    rt = key.route
    lines, want = [], []

    def add(kind_row, a_rows, b_rows, slot, ln, rec, in_b):
        lines.append('%s %d 1 %d %s %s %s %s %s' % (bytes(kind_row).hex() if kind_row is not None else '-', slot, ln, rt.control_root.hex(), rt.control_id.hex(),
                                                   b''.join(a_rows).hex(), b''.join(b_rows).hex() if b_rows is not None else '-', rec.hex()))
        st, fl, sig, pts = rm.prep_slot(1, rt, ln, a_rows[slot], in_b, rec)
        want.append(' '.join(['%d %d' % (st, fl)] + ['%064x' % x for x in sig + pts]))

    for j in range(n):
        add(kinds, in_a, jds, j, 260, seals[j], jds[j] if kinds[j] == 0 else None)                 # the mixed row
        add(None, ids, jds, j, 260, seals[j], jds[j])                                              # no row, journal digests: all verify
        add(None, in_a, None, j, 260, seals[j], None)                                              # no row, none: all verifyIntegrity (in_a as given)
        add([1] * n, in_a, jds, j, 260, seals[j], None)                                            # a uniform row of either method
        add([0] * n, ids, jds, j, 260, seals[j], jds[j])
        add(kinds, in_a, jds, j, 259, seals[j][:259] + b'\0', jds[j] if kinds[j] == 0 else None)   # the length is answered first
    got = _run(exe, 'slot', lines)
    assert got == want
    # the valid seal of a verify slot and of a verifyIntegrity slot give the same signals: the claim digest is the verify row's own
    assert got[0].split()[2:7] == got[1].split()[2:7] and got[6].split()[2:7] == got[7].split()[2:7]
    assert {ln.split()[0] for ln in got} == {'1', '4'} and all(ln.split()[1] == '1' for ln in got if ln.split()[0] == '1')
    # every slot has its own answer, whichever way its method is told (a row read at the wrong slot would give another one); the three
    # verify slots taken as verifyIntegrity (their image id as the claim digest) have a second one; one more for the short seals
    assert len(set(got)) == n + kinds.count(0) + 1

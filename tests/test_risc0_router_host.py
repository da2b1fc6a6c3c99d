"""RISC Zero verifier router (include/zkv_risc0_router.h) without a device: the new header against the library's
exports, the selector derivation over key words against the reference's recorded values, the creation rules, the getters, the
SelectorUnknown revert bytes, and the per-slot front end of the keyed group compiled for the host (plain and under the sanitizers)
against tests/risc0_router_model.py.  Parity unpinned for the routing; a keyed route with the reference's key derives its selector."""
import ctypes as C
import os
import random
import re
import subprocess

import pytest

import risc0_router_model as rm
import spec_model as m

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
SRC = os.path.join(HERE, 'host_cpp', 'test_rzrouter_prep.cpp')
H = bytes.fromhex
NEW = ['zkv_risc0_router_create', 'zkv_risc0_router_route_count', 'zkv_risc0_router_route', 'zkv_risc0_router_route_verifier_key_digest',
       'zkv_risc0_router_verify', 'zkv_risc0_router_verify_integrity', 'zkv_risc0_router_verify_batch', 'zkv_risc0_router_verify_integrity_batch',
       'zkv_risc0_router_verify_batch_dev', 'zkv_risc0_router_last_route_counts', 'zkv_risc0_router_status_abi_encode']
NO_DEVICE, WRONG_CTX, INVALID_ARG = -2, -5, -1
SANITIZE = ['-fsanitize=address,undefined', '-fno-sanitize-recover=all']
REF_WORDS = m.vk_to_words(m.RISC0_VK)


def _names(path):
    return set(re.findall(r'\b(zkv_[a-z0-9_]+)\s*\(', re.sub(r'/\*.*?\*/', '', open(path).read(), flags=re.S)))


@pytest.fixture(scope='module')
def L():
    from stylus_zkvm_verifiers_amd import risc0_router
    return risc0_router.lib()


@pytest.fixture(scope='module')
def real(real_proofs):
    r = real_proofs['risc0']
    return dict(root=H(r['control_root']), cid=H(r['bn254_control_id']), seal=H(r['seal']), image_id=H(r['image_id']),
                journal=H(r['journal_digest']), selector=H(r['selector']), vk_digest=H(r['vk_digest']), claim=H(r['claim_digest']))


@pytest.fixture(scope='module')
def key():
    return rm.Key(0x17A0)


def _create(L, builtin, keyed, device=0):
    vks = (C.c_char_p * max(len(keyed), 1))(*[w for w, _, _ in keyed])
    return L.zkv_risc0_router_create(len(builtin), b''.join(r for r, _ in builtin) + b'\0', b''.join(i for _, i in builtin) + b'\0', len(keyed), vks,
                                     b''.join(r for _, r, _ in keyed) + b'\0', b''.join(i for _, _, i in keyed) + b'\0', device)


# ---------------------------------------------------------------- symbol sets
def test_header_declares_exactly_the_new_symbols_and_the_library_exports_them(L):
    hdr = os.path.join(ROOT, 'include', 'zkv_risc0_router.h')
    assert _names(hdr) == set(NEW)
    text = open(hdr).read()
    assert '#include "zkv.h"' in text and 'PARITY UNPINNED' in text and 'SelectorUnknown(bytes4)' in text
    for d in ('#define ZKV_VM_RISC0_ROUTER 12', '#define ZKV_RISC0_ROUTER_MAX_ROUTES 32', '#define ZKV_RISC0_ROUTER_MAX_KEYED 8',
              '#define ZKV_RISC0_KEY_BYTES 832', '#define ZKV_STATUS_ROUTE_NOT_FOUND 8'):
        assert d in text, d
    assert 'synchronisation' in text and 'asynchronous' in text          # what zkv_risc0_router_verify_batch_dev says about its stream
    import stylus_zkvm_verifiers_amd as z
    from stylus_zkvm_verifiers_amd import _lib, risc0_router
    assert set(risc0_router.SYMBOLS) == set(NEW) and not set(NEW) & set(_lib.SYMBOLS)
    for name in NEW:
        assert hasattr(L, name), name
    main = _names(os.path.join(ROOT, 'include', 'zkv.h'))
    assert len(main) == 83 and len(_lib.SYMBOLS) == 83 and not main & set(NEW)
    assert 'RiscZeroRouter' in z.__all__ and z.RiscZeroRouter is risc0_router.RiscZeroRouter
    assert (risc0_router.VM_RISC0_ROUTER, risc0_router.MAX_ROUTES, risc0_router.MAX_KEYED, risc0_router.KEY_BYTES) == (12, 32, 8, 832)


def test_cpp_mirror_compiles(tmp_path):
    src = tmp_path / 'mirror.cpp'
    src.write_text('#include "%s"\n'
                   'int main() { std::vector<zkv::RiscZeroBuiltinRoute> b; std::vector<zkv::RiscZeroKeyedRoute> k;\n'
                   '  try { zkv::RiscZeroRouter r(b, k); return (int)r.routes().size() + (int)r.last_route_counts().size(); }\n'
                   '  catch (const std::exception&) { return 0; } }\n' % os.path.join(ROOT, 'stylus_zkvm_verifiers_amd', 'host', 'zkv_risc0_router.hpp'))
    subprocess.check_call(['g++', '-std=c++17', '-fsyntax-only', '-Wall', str(src)])


# ---------------------------------------------------------------- derivation
def test_key_digest_and_selector_over_the_reference_key_words(L, real):
    assert len(REF_WORDS) == 832
    assert rm.vk_digest_of_words(REF_WORDS) == real['vk_digest'] == m.risc0_vk_digest()
    assert rm.selector_of(real['root'], real['cid'], real['vk_digest']) == real['selector'] == m.risc0_selector(real['root'], real['cid'])
    # the library: a keyed route with the reference's key and the real proof's parameters derives the reference's selector
    h = _create(L, [], [(REF_WORDS, real['root'], real['cid'])])
    assert h and L.zkv_risc0_router_route_count(h) == 1
    sel = C.create_string_buffer(4); keyed = C.c_int(-1); dig = C.create_string_buffer(32)
    assert L.zkv_risc0_router_route(h, 0, sel, C.byref(keyed)) == 0 and (sel.raw, keyed.value) == (real['selector'], 1)
    assert L.zkv_risc0_router_route_verifier_key_digest(h, 0, dig) == 0 and dig.raw == real['vk_digest']
    L.zkv_ctx_destroy(h)
    # ... as a built-in route with them does, and as the verifier context does
    h = _create(L, [(real['root'], real['cid'])], [])
    assert L.zkv_risc0_router_route(h, 0, sel, C.byref(keyed)) == 0 and (sel.raw, keyed.value) == (real['selector'], 0)
    assert L.zkv_risc0_router_route_verifier_key_digest(h, 0, dig) == 0 and dig.raw == real['vk_digest']
    L.zkv_ctx_destroy(h)
    from stylus_zkvm_verifiers_amd import RiscZeroVerifier
    v = RiscZeroVerifier(); v.initialize(real['root'], real['cid'])
    assert v.get_selector() == real['selector'] and v.get_verifier_key_digest() == real['vk_digest']     # the generalised digest keeps the built-in one
    v.close()


def test_derived_selectors_of_other_keys_and_parameters(L, key):
    rng = random.Random(0x17A1)
    keyed = [key.triple()]
    for k in range(5):                                               # one key, other parameters: other selectors
        keyed.append((key.words, bytes(rng.randrange(256) for _ in range(32)), bytes(rng.randrange(256) for _ in range(32))))
    keyed.append((rm.off_curve_ic(key.words), key.control_root, key.control_id))          # other words: another digest
    builtin = [rm.params(t) for t in range(3)] + [(bytes(32), bytes(32)), (b'\xff' * 32, b'\xff' * 32)]    # control ids 0 and >= R included
    model = rm.Router(builtin, keyed)
    from stylus_zkvm_verifiers_amd import RiscZeroRouter
    rt = RiscZeroRouter(builtin, keyed)
    got = rt.routes()
    assert [g[0] for g in got] == model.selectors and [g[1] for g in got] == [False] * 5 + [True] * 7
    assert [g[2] for g in got] == [r.vk_digest for r in model.routes]
    assert len({g[2] for g in got}) == 3                             # built-in key, the trapdoor key, the key with the moved point
    assert rt.last_route_counts() == [0] * 14
    rt.close()


# ---------------------------------------------------------------- creation rules
def test_create_refuses_bad_route_sets(L, real, key):
    one = (real['root'], real['cid'])
    assert not _create(L, [], [])                                                                  # no route
    assert not _create(L, [one, one], [])                                                          # two identical built-in routes
    assert not _create(L, [rm.params(1), one, rm.params(2), one], [])
    assert not _create(L, [one], [(REF_WORDS, real['root'], real['cid'])])                         # keyed with the reference key against built-in
    assert not _create(L, [], [key.triple(), key.triple()])                                        # keyed against keyed
    assert not _create(L, [rm.params(k) for k in range(33)], [])                                   # 33 routes
    assert not _create(L, [rm.params(k) for k in range(25)], [(key.words,) + rm.params(100 + k) for k in range(8)])      # 25 + 8
    assert not _create(L, [], [(key.words,) + rm.params(100 + k) for k in range(9)])               # 9 keyed routes
    assert not _create(L, [one], [(key.words,) + rm.params(100 + k) for k in range(9)])
    for nb, nk in ((32, 0), (24, 8), (0, 8), (31, 1), (1, 0), (0, 1)):                             # the largest and the smallest routers
        h = _create(L, [rm.params(k) for k in range(nb)], [(key.words,) + rm.params(100 + k) for k in range(nk)])
        assert h and L.zkv_risc0_router_route_count(h) == nb + nk
        L.zkv_ctx_destroy(h)
    h = _create(L, [one], [(REF_WORDS, real['root'], rm.params(7)[1])])                            # the reference key with OTHER parameters: fine
    assert h
    L.zkv_ctx_destroy(h)
    # NULL pointers
    vks = (C.c_char_p * 1)(key.words)
    r32, i32 = key.control_root, key.control_id
    assert not L.zkv_risc0_router_create(1, None, i32, 0, None, None, None, 0)
    assert not L.zkv_risc0_router_create(1, r32, None, 0, None, None, None, 0)
    assert not L.zkv_risc0_router_create(0, None, None, 1, None, r32, i32, 0)
    assert not L.zkv_risc0_router_create(0, None, None, 1, vks, None, i32, 0)
    assert not L.zkv_risc0_router_create(0, None, None, 1, vks, r32, None, 0)
    assert not L.zkv_risc0_router_create(0, None, None, 2, (C.c_char_p * 2)(key.words, None), r32 + r32, i32 + rm.params(3)[1], 0)
    h = L.zkv_risc0_router_create(0, None, None, 1, vks, r32, i32, 0)                               # a count of zero lets its pointers be NULL
    assert h
    L.zkv_ctx_destroy(h)
    h = L.zkv_risc0_router_create(1, r32, i32, 0, None, None, None, 0)
    assert h
    L.zkv_ctx_destroy(h)
    from stylus_zkvm_verifiers_amd import RiscZeroRouter
    for bad in (dict(routes=[], keyed=[]), dict(routes=[one, one]), dict(keyed=[(key.words[:-1], r32, i32)]), dict(routes=[(r32[:31], i32)]),
                dict(keyed=[(key.words,) + rm.params(k) for k in range(9)]), dict(routes=[rm.params(k) for k in range(33)])):
        with pytest.raises(ValueError):
            RiscZeroRouter(**bad)
    for bad in (dict(builtin=[], keyed=[]), dict(builtin=[one, one]), dict(builtin=[one], keyed=[(REF_WORDS, real['root'], real['cid'])])):
        with pytest.raises(ValueError):
            rm.Router(**bad)


# ---------------------------------------------------------------- getters, context-wide calls, wrong contexts, no device
def test_getters_past_the_routes_and_context_wide_calls(L, real, key):
    from stylus_zkvm_verifiers_amd import RiscZeroRouter, _lib
    raw = _lib.lib()
    bad = rm.off_curve_ic(key.words)                                 # an invalid key is accepted: its own route fails its proofs
    rt = RiscZeroRouter([(real['root'], real['cid']), rm.params(1)], [key.triple(), (bad, key.control_root, key.control_id)])
    h = rt._h
    assert raw.zkv_ctx_vm(h) == 12 and L.zkv_risc0_router_route_count(h) == 4 and L.zkv_risc0_router_route_count(None) == 0
    sel = C.create_string_buffer(4); keyed = C.c_int(-1); dig = C.create_string_buffer(32)
    assert L.zkv_risc0_router_route(h, 3, sel, C.byref(keyed)) == 0 and keyed.value == 1
    assert L.zkv_risc0_router_route(h, 3, None, None) == 0
    assert L.zkv_risc0_router_route(h, 4, sel, C.byref(keyed)) == INVALID_ARG
    assert L.zkv_risc0_router_route(None, 0, sel, C.byref(keyed)) == WRONG_CTX
    assert L.zkv_risc0_router_route_verifier_key_digest(h, 4, dig) == INVALID_ARG
    assert L.zkv_risc0_router_route_verifier_key_digest(h, 0, None) == INVALID_ARG
    assert L.zkv_risc0_router_route_verifier_key_digest(None, 0, dig) == WRONG_CTX
    assert L.zkv_risc0_router_last_route_counts(h, None) == INVALID_ARG
    assert raw.zkv_ctx_set_lanes_per_proof(h, 16) == 0 and raw.zkv_ctx_set_lanes_per_proof(h, 3) == INVALID_ARG
    assert raw.zkv_ctx_set_lanes_per_proof(h, 0) == 0
    assert raw.zkv_ctx_set_aggregate_check(h, 64, bytes(32)) == 0 and raw.zkv_ctx_set_aggregate_check(h, 1, None) == 0
    assert raw.zkv_ctx_set_aggregate_check(h, 0, None) == 0 and raw.zkv_ctx_set_aggregate_check(h, 3, None) == INVALID_ARG
    assert rt.aggregate_counters() == (0, 0)
    assert raw.zkv_ctx_synchronize(h) == 0
    assert not raw.zkv_ctx_create_sharded((C.c_void_p * 1)(h), 1)                                 # single-device
    only = RiscZeroRouter(keyed=[key.triple()])                                                   # keyed routes alone: the same calls
    assert raw.zkv_ctx_set_aggregate_check(only._h, 1, None) == 0 and only.aggregate_counters() == (0, 0)
    assert raw.zkv_ctx_set_lanes_per_proof(only._h, 2) == 0 and raw.zkv_ctx_synchronize(only._h) == 0
    only.close()
    rt.close()


def test_selector_unknown_revert_bytes(L, real):
    from stylus_zkvm_verifiers_amd import RiscZeroRouter, _lib, errors
    rt = RiscZeroRouter([(real['root'], real['cid'])])
    raw = _lib.lib()
    s4 = C.create_string_buffer(4)
    assert raw.zkv_abi_function_selector(b'SelectorUnknown(bytes4)', s4) == 0 and s4.raw == m.keccak256(b'SelectorUnknown(bytes4)')[:4]
    for recv in (H('12345678'), bytes(4), H('ffffffff'), real['selector']):
        got = rt.status_revert(8, recv)
        assert got == rm.selector_unknown_revert(recv) and len(got) == 36 and got[:4] == s4.raw and got[4:8] == recv and got[8:] == bytes(28)
    for st in (1, 2, 3, 4):                                          # every other status: the RISC Zero verifier's bytes
        assert rt.status_revert(st) == errors.revert_bytes(errors.VM_RISC0, st) == m.revert_bytes('risc0', st)
    assert rt.status_revert(0) == b''
    assert rt.status_revert(5, H('01020304')) == errors.revert_bytes(errors.VM_RISC0, 5, H('01020304'), real['selector'])
    o = C.create_string_buffer(68)
    assert L.zkv_risc0_router_status_abi_encode(rt._h, 8, None, o) == INVALID_ARG
    assert L.zkv_risc0_router_status_abi_encode(rt._h, 8, bytes(4), None) == INVALID_ARG
    assert L.zkv_risc0_router_status_abi_encode(rt._h, 9, bytes(4), o) == INVALID_ARG
    assert L.zkv_risc0_router_status_abi_encode(None, 8, bytes(4), o) == WRONG_CTX
    assert raw.zkv_status_abi_encode(0, 8, bytes(4), bytes(4), o) == INVALID_ARG                  # zkv.h's encoder is unchanged
    rt.close()


def test_wrong_ctx_both_ways(L, real, key):
    from stylus_zkvm_verifiers_amd import RiscZeroRouter, RiscZeroVerifier, RiscZeroVerifierSet, Sp1Gateway, Sp1Verifier, _lib, sp1_gateway
    raw = _lib.lib()
    gl = sp1_gateway.lib()
    rt = RiscZeroRouter([(real['root'], real['cid'])], [key.triple()])
    h = rt._h
    st = C.c_uint8(9); rv = C.create_string_buffer(4)
    z32 = bytes(32); off = (C.c_uint64 * 2)(0, 260); seal = real['seal']
    # a router under the entry points of other kinds
    assert raw.zkv_risc0_verify(h, seal, 260, z32, z32, C.byref(st), rv) == WRONG_CTX
    assert raw.zkv_risc0_verify_integrity(h, seal, 260, z32, C.byref(st), rv) == WRONG_CTX
    assert raw.zkv_risc0_verify_batch(h, 1, seal, off, z32, z32, C.byref(st), rv) == WRONG_CTX
    assert raw.zkv_risc0_verify_batch_dev(h, 1, None, None, None, None, None, None) == WRONG_CTX
    assert raw.zkv_risc0_set_verify_batch(h, 1, (C.c_uint32 * 1)(0), seal, off, z32, z32, C.cast(C.byref(st), C.c_void_p), rv) == WRONG_CTX
    assert raw.zkv_sp1_verify_proof(h, z32, b'', 0, seal, 260, C.byref(st), rv) == WRONG_CTX
    assert raw.zkv_groth16_verify_batch(h, 1, seal, z32, C.cast(C.byref(st), C.c_void_p)) == WRONG_CTX
    assert raw.zkv_ctx_vk_x_batch(h, 1, z32 * 2, C.create_string_buffer(64)) == WRONG_CTX
    assert raw.zkv_risc0_get_selector(h, rv) == WRONG_CTX
    assert gl.zkv_sp1_gateway_route_count(h) == 0 and gl.zkv_sp1_gateway_last_route_counts(h, (C.c_uint64 * 8)()) == WRONG_CTX
    assert gl.zkv_sp1_gateway_verify_proof(h, z32, b'', 0, seal, 260, C.byref(st), rv) == WRONG_CTX
    assert st.value == 9
    # other kinds under the router's entry points
    others = [RiscZeroVerifier(), RiscZeroVerifierSet([real['root']], [real['cid']]), Sp1Verifier(), Sp1Gateway(True)]
    others[0].initialize(real['root'], real['cid'])
    cnt = (C.c_uint64 * 40)()
    o = C.create_string_buffer(68)
    for v in others + [None]:
        k = v._h if v is not None else None
        assert L.zkv_risc0_router_route_count(k) == 0
        assert L.zkv_risc0_router_verify(k, seal, 260, z32, z32, C.byref(st), rv) == WRONG_CTX
        assert L.zkv_risc0_router_verify_integrity(k, seal, 260, z32, C.byref(st), rv) == WRONG_CTX
        assert L.zkv_risc0_router_verify_batch(k, 1, seal, off, z32, z32, C.cast(C.byref(st), C.c_void_p), rv) == WRONG_CTX
        assert L.zkv_risc0_router_verify_integrity_batch(k, 1, seal, off, z32, C.cast(C.byref(st), C.c_void_p), rv) == WRONG_CTX
        assert L.zkv_risc0_router_verify_batch_dev(k, 1, None, None, None, None, None, None) == WRONG_CTX
        assert L.zkv_risc0_router_last_route_counts(k, cnt) == WRONG_CTX
        assert L.zkv_risc0_router_status_abi_encode(k, 8, bytes(4), o) == WRONG_CTX
    for v in others:
        v.close()
    rt.close()


def test_compute_entry_points_without_a_device(L, real, key):
    import stylus_zkvm_verifiers_amd as z
    rt = z.RiscZeroRouter([(real['root'], real['cid'])], [key.triple()], device=4096)              # no such device, with or without a GPU in the machine
    h = rt._h
    st = C.c_uint8(9); rv = C.create_string_buffer(4)
    off = (C.c_uint64 * 2)(0, 260)
    stp = C.cast(C.byref(st), C.c_void_p)
    assert L.zkv_risc0_router_verify(h, real['seal'], 260, real['image_id'], real['journal'], C.byref(st), rv) == NO_DEVICE
    assert L.zkv_risc0_router_verify(h, b'\x01\x02', 2, real['image_id'], real['journal'], C.byref(st), rv) == NO_DEVICE      # routed on the device
    assert L.zkv_risc0_router_verify_integrity(h, real['seal'], 260, real['claim'], C.byref(st), rv) == NO_DEVICE
    assert L.zkv_risc0_router_verify_batch(h, 1, real['seal'], off, real['image_id'], real['journal'], stp, rv) == NO_DEVICE
    assert L.zkv_risc0_router_verify_integrity_batch(h, 1, real['seal'], off, real['claim'], stp, rv) == NO_DEVICE
    assert L.zkv_risc0_router_verify_batch_dev(h, 1, 8, 8, 8, 8, None, None) == NO_DEVICE
    assert st.value == 9
    from stylus_zkvm_verifiers_amd import _lib
    assert _lib.lib().zkv_ctx_reserve(h, 64) == NO_DEVICE
    assert _lib.lib().zkv_ctx_last_stage_ms(h, (C.c_float * 5)()) == NO_DEVICE
    # argument checks come first, and an empty batch needs nothing
    assert L.zkv_risc0_router_verify_batch(h, 1, None, off, real['image_id'], real['journal'], stp, rv) == INVALID_ARG
    assert L.zkv_risc0_router_verify_batch(h, 1, real['seal'], off, real['image_id'], None, stp, rv) == INVALID_ARG
    assert L.zkv_risc0_router_verify_batch(h, 1, real['seal'], (C.c_uint64 * 2)(260, 0), real['image_id'], real['journal'], stp, rv) == INVALID_ARG
    assert L.zkv_risc0_router_verify_batch_dev(h, 1, None, 8, 8, 8, None, None) == INVALID_ARG
    assert L.zkv_risc0_router_verify(h, None, 3, real['image_id'], real['journal'], C.byref(st), rv) == INVALID_ARG
    assert L.zkv_risc0_router_verify_batch(h, 0, None, None, None, None, None, None) == 0
    assert L.zkv_risc0_router_verify_batch_dev(h, 0, None, None, None, None, None, None) == 0
    assert rt.last_route_counts() == [0, 0, 0, 0]
    rt.close()


# ---------------------------------------------------------------- the host program: per-slot front end, derivation, classifier
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


def _prep_cases(key):
    """(vk_valid, route, true length, in_a, in_b or None, 260-byte compact record)."""
    rng = random.Random(0x17A2)
    image_id = bytes(rng.randrange(256) for _ in range(32)); journal = bytes(rng.randrange(256) for _ in range(32))
    claim = m.receipt_claim_ok_digest(image_id, journal)
    good = key.prove(image_id, journal)
    w = [int.from_bytes(good[4 + 32 * i:36 + 32 * i], 'big') for i in range(8)]
    rt = key.route
    big_id = rm.Route(key.control_root, m.be32(m.R), key.words)                                   # control id = R: out of range
    top_id = rm.Route(key.control_root, b'\xff' * 32, key.words)
    zero = rm.Route(bytes(32), bytes(32), key.words)

    def rec(words):
        return key.selector + b''.join(m.be32(x) for x in words)
    cases = []
    for ln in (4, 259, 260, 261):                                   # the gatherer copies min(len, 260) bytes and pads with zeros
        cases.append((1, rt, ln, image_id, journal, good[:min(ln, 260)].ljust(260, b'\0')))
        cases.append((1, rt, ln, claim, None, good[:min(ln, 260)].ljust(260, b'\0')))
    cases.append((0, rt, 260, image_id, journal, good))                                           # a key with an invalid point
    cases.append((0, rt, 261, image_id, journal, good))                                           # ... still answers the length first
    cases.append((0, rt, 260, claim, None, good))
    for r2 in (big_id, top_id):
        cases.append((1, r2, 260, image_id, journal, good))
        cases.append((1, r2, 259, image_id, journal, good))
    cases.append((1, zero, 260, image_id, journal, good))                                         # zero constants: alive, the pairing will refuse
    for k in range(4):                                                                            # verify and integrity rows, other inputs
        a = bytes(rng.randrange(256) for _ in range(32)); b = bytes(rng.randrange(256) for _ in range(32))
        cases.append((1, rt, 260, a, b, good))
        cases.append((1, rt, 260, a, None, good))
    cases.append((1, rt, 260, b'\xff' * 32, None, good)); cases.append((1, rt, 260, bytes(32), None, good))
    cases.append((1, rt, 260, image_id, journal, rec([w[0], (w[1] + 1) % m.P] + w[2:])))          # A off the curve
    cases.append((1, rt, 260, image_id, journal, rec(w[:6] + [w[6], (w[7] + 1) % m.P])))          # C off the curve
    cases.append((1, rt, 260, image_id, journal, rec(w[:2] + [w[2], (w[3] + 1) % m.P] + w[4:])))  # B off the twist
    cases.append((1, rt, 260, image_id, journal, rec([0, m.P] + w[2:])))                          # A = (0, Q): Q - Q = 0, the point at infinity
    cases.append((1, rt, 260, claim, None, rec([0, m.P] + w[2:])))
    cases.append((1, rt, 260, image_id, journal, rec([0, 0] + w[2:])))                            # A = (0, 0): not negated
    cases.append((1, rt, 260, image_id, journal, rec([w[0], 0] + w[2:])))                         # A.y = 0: Q - 0 = Q is no coordinate
    cases.append((1, rt, 260, image_id, journal, rec([w[0], m.P + 1] + w[2:])))                   # A.y > Q: wraps mod 2^256
    cases.append((1, rt, 260, image_id, journal, rec(w[:6] + [0, 0])))                            # C = (0, 0)
    cases.append((1, rt, 260, image_id, journal, rec(w[:2] + [0, 0, 0, 0] + w[6:])))              # B = (0, 0)
    for k in (0, 2, 3, 4, 5, 6, 7):
        cases.append((1, rt, 260, image_id, journal, rec(w[:k] + [w[k] + m.P] + w[k + 1:])))      # a coordinate >= Q (w + Q < 2^256)
    return cases


@pytest.mark.parametrize('flags,name', [([], 'plain'), (SANITIZE, 'san')])
def test_per_slot_front_end_equals_the_model(tmp_path, key, flags, name):
    exe = _program(tmp_path, flags, name)
    cases = _prep_cases(key)
    got = _run(exe, 'prep', ['%d %d %s %s %s %s %s' % (v, ln, rt.control_root.hex(), rt.control_id.hex(), a.hex(), b.hex() if b is not None else '-', r.hex())
                             for v, rt, ln, a, b, r in cases])
    seen = set()
    for (v, rt, ln, a, b, r), line in zip(cases, got):
        st, fl, sig, pts = rm.prep_slot(v, rt, ln, a, b, r)
        assert line == ' '.join(['%d %d' % (st, fl)] + ['%064x' % x for x in sig + pts]), (v, ln, b is None, r.hex()[:80])
        seen.add((st, fl))
    assert {(4, 0), (1, 0), (1, 1), (1, 3), (1, 5), (1, 9)} <= seen
    # the model's front end agrees with the whole-seal model wherever that one decides before the pairing, and on the valid seal
    n_ok = 0
    for v, rt, ln, a, b, r in cases:
        if v and ln == 260:
            seal = rt.selector + r[4:]                               # (the front end runs behind the classifier: the record's own selector is not its business)
            st = (rt.verify(seal, a, b) if b is not None else rt.verify_integrity(seal, a))[0]
            fl = rm.prep_slot(v, rt, ln, a, b, r)[1]
            assert st in (0, 1) and (fl & 1 or st == 1)
            n_ok += st == 0
    assert n_ok == 2                                                 # the valid seal under verify and under verify_integrity


@pytest.mark.parametrize('flags,name', [([], 'plain'), (SANITIZE, 'san')])
def test_derivation_and_classifier_in_the_host_program(tmp_path, key, real, flags, name):
    exe = _program(tmp_path, flags, name)
    rng = random.Random(0x17A3)
    rows = [(real['root'], real['cid'], REF_WORDS), key.triple()[1:] + (key.words,), (bytes(32), b'\xff' * 32, rm.off_curve_ic(key.words))]
    rows += [(bytes(rng.randrange(256) for _ in range(32)), bytes(rng.randrange(256) for _ in range(32)), key.words) for _ in range(3)]
    got = _run(exe, 'derive', ['%s %s %s' % (r.hex(), i.hex(), w.hex()) for r, i, w in rows])
    for (r, i, w), line in zip(rows, got):
        d = rm.vk_digest_of_words(w)
        assert line == '%s %s' % (d.hex(), rm.selector_of(r, i, d).hex())
    assert got[0] == '%s %s' % (real['vk_digest'].hex(), real['selector'].hex())
    # classifier: built-in routes share column 0 and report the instance; keyed route k is column 1 + k; 9 = unknown
    lines, want = [], []
    for nb, nk in ((1, 0), (0, 1), (3, 3), (24, 8), (32, 0), (0, 8)):
        sels = [rng.randrange(1 << 32) for _ in range(nb + nk)]
        for q in list(range(nb + nk)) + [-1]:
            v = sels[q] if q >= 0 else (sels[0] ^ 1)
            lines.append('%d %d %08x %s' % (nb, nk, v, ' '.join('%08x' % s for s in sels)))
            want.append('9 0' if q < 0 or v not in sels else ('0 %d' % q if q < nb else '%d 0' % (1 + q - nb)))
    assert _run(exe, 'column', lines) == want

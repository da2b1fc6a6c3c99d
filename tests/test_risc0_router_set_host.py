"""RISC Zero router with a set route (include/zkv_risc0_router_set.h) without a device: the new header against the
library's exports and the untouched symbol sets of its neighbours, the creation rules, the getters and the wrong-context answers in both
directions, the fixture against the model (tests/risc0_router_set_model.py), and a stand-alone host program
(tests/host_sim/host_sim_rzrouter_set.cpp, plain and under the sanitizers, as a child process) that runs the header arithmetic of
k_rzset_front and the identity pair of k_rzset_ident.  PARITY UNPINNED: the reference holds no router and no set verifier."""
import ctypes as C
import json
import os
import random
import re
import subprocess

import pytest

import risc0_router_model as rm
import risc0_router_set_model as rsm
import set_inclusion_model as sm
import spec_model as m

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
SRC = os.path.join(HERE, 'host_sim', 'host_sim_rzrouter_set.cpp')
H = bytes.fromhex
NEW = ['zkv_risc0_router_create_with_set', 'zkv_risc0_router_set_selector', 'zkv_risc0_router_verify_ragged_dev', 'zkv_risc0_router_set_submit_root',
       'zkv_risc0_router_set_has_root', 'zkv_risc0_router_set_last_counts', 'zkv_diag_rzset_groups']
ROUTER = ['zkv_risc0_router_create', 'zkv_risc0_router_route_count', 'zkv_risc0_router_route', 'zkv_risc0_router_route_verifier_key_digest',
          'zkv_risc0_router_verify', 'zkv_risc0_router_verify_integrity', 'zkv_risc0_router_verify_batch', 'zkv_risc0_router_verify_integrity_batch',
          'zkv_risc0_router_verify_batch_dev', 'zkv_risc0_router_last_route_counts', 'zkv_risc0_router_status_abi_encode']
WIRE = ['zkv_risc0_router_verify_call_batch', 'zkv_risc0_router_verify_call_batch_dev', 'zkv_risc0_router_encode_verify_call',
        'zkv_risc0_router_encode_verify_integrity_call', 'zkv_risc0_router_eth_call_batch', 'zkv_risc0_router_eth_call_batch_dev',
        'zkv_risc0_router_eth_call_returndata', 'zkv_risc0_router_last_call_counts']
SETINCL = ['zkv_risc0_setincl_create', 'zkv_risc0_setincl_create_keyed', 'zkv_risc0_setincl_verify_batch', 'zkv_risc0_setincl_verify_integrity_batch',
           'zkv_risc0_setincl_verify_batch_dev', 'zkv_risc0_setincl_submit_root', 'zkv_risc0_setincl_has_root', 'zkv_risc0_setincl_get_selector',
           'zkv_risc0_setincl_last_counts', 'zkv_risc0_setincl_seal_encode', 'zkv_risc0_setincl_seal_decode', 'zkv_diag_setincl_roots']
NO_DEVICE, WRONG_CTX, INVALID_ARG = -2, -5, -1
SANITIZE = ['-fsanitize=address,undefined', '-fno-sanitize-recover=all']
SHIFTS = (0, 1, 4, 16)
NOT_SET, MALFORMED, CLAIM = 0, 1, 2              # RZS_* of csrc/zkv_rzrouter_set.h


def _names(path):
    return set(re.findall(r'\b(zkv_[a-z0-9_]+)\s*\(', re.sub(r'/\*.*?\*/', '', open(path).read(), flags=re.S)))


@pytest.fixture(scope='module')
def L():
    from stylus_zkvm_verifiers_amd import risc0_router_set
    return risc0_router_set.lib()


@pytest.fixture(scope='module')
def fx():
    return json.load(open(os.path.join(HERE, 'golden', 'risc0_router_set_cases.json')))


@pytest.fixture(scope='module')
def keys(fx):
    return [rm.Key(s) for s in fx['key_seeds']]


@pytest.fixture(scope='module')
def key():
    return rm.Key(0x17C0)


def _create(L, set_id, builtin, keyed, device=0):
    vks = (C.c_char_p * max(len(keyed), 1))(*[w for w, _, _ in keyed])
    return L.zkv_risc0_router_create_with_set(len(builtin), b''.join(r for r, _ in builtin) + b'\0', b''.join(i for _, i in builtin) + b'\0', len(keyed), vks,
                                              b''.join(r for _, r, _ in keyed) + b'\0', b''.join(i for _, _, i in keyed) + b'\0', set_id, device)


# ---------------------------------------------------------------- symbol sets
def test_header_declares_exactly_the_new_symbols_and_the_library_exports_them(L):
    inc = lambda f: os.path.join(ROOT, 'include', f)
    assert _names(inc('zkv_risc0_router_set.h')) == set(NEW)
    text = open(inc('zkv_risc0_router_set.h')).read()
    for d in ('#include "zkv_risc0_router.h"', '#include "zkv_risc0_set_inclusion.h"', 'PARITY UNPINNED', 'ZKV_ERR_WRONG_CTX', 'TWICE', 'asynchronous',
              'nested sets are not followed'):
        assert d in text, d
    import stylus_zkvm_verifiers_amd as z
    from stylus_zkvm_verifiers_amd import _lib, risc0_router, risc0_router_set, risc0_router_wire, risc0_set_inclusion
    assert set(risc0_router_set.SYMBOLS) == set(NEW)
    for name in NEW:
        assert hasattr(L, name), name
    # the neighbours' symbol sets are what they were
    assert _names(inc('zkv_risc0_router.h')) == set(ROUTER) == set(risc0_router.SYMBOLS)
    assert _names(inc('zkv_risc0_router_wire.h')) == set(WIRE) == set(risc0_router_wire.SYMBOLS)
    assert _names(inc('zkv_risc0_set_inclusion.h')) == set(SETINCL)
    main = _names(inc('zkv.h'))
    assert len(main) == 83 and len(_lib.SYMBOLS) == 83
    for other in (main, set(_lib.SYMBOLS), set(ROUTER), set(WIRE), set(SETINCL)):
        assert not other & set(NEW)
    assert 'RiscZeroSetRouter' in z.__all__ and z.RiscZeroSetRouter is risc0_router_set.RiscZeroSetRouter
    assert issubclass(z.RiscZeroSetRouter, z.RiscZeroRouter)
    assert (risc0_router_set.MAX_DEPTH, risc0_router_set.MAX_ROOTS) == (sm.MAX_DEPTH, sm.MAX_ROOTS) == (risc0_set_inclusion.MAX_DEPTH, risc0_set_inclusion.MAX_ROOTS)
    # the header compiles as C next to its neighbours, in either order
    for order in (('zkv_risc0_router_set.h', 'zkv_risc0_router_wire.h'), ('zkv_risc0_router_wire.h', 'zkv_risc0_router_set.h')):
        src = ''.join('#include "%s"\n' % inc(f) for f in order) + 'int main(void) { return ZKV_SETINCL_MAX_DEPTH - 64; }\n'
        subprocess.run(['gcc', '-x', 'c', '-fsyntax-only', '-Wall', '-Werror', '-'], input=src.encode(), check=True)


# ---------------------------------------------------------------- creation rules and getters
def test_creation_rules_and_the_set_route(L, key, real_proofs):
    r = real_proofs['risc0']
    one = (H(r['control_root']), H(r['bn254_control_id']))
    set_id = m.sha256(b'a set builder')
    assert not _create(L, set_id, [], [])                                                          # a router needs a Groth16 route
    assert not _create(L, set_id, [one, one], [])                                                  # where zkv_risc0_router_create returns NULL
    assert not _create(L, set_id, [], [key.triple(), key.triple()])
    assert not _create(L, None, [one], [])                                                         # no image id
    assert not _create(L, set_id, [rm.params(k) for k in range(32)], [])                           # 32 + the set route
    assert not _create(L, set_id, [rm.params(k) for k in range(24)], [(key.words,) + rm.params(100 + k) for k in range(8)])
    assert not _create(L, set_id, [], [(key.words,) + rm.params(100 + k) for k in range(9)])       # 9 keyed routes
    sel = C.create_string_buffer(4); keyed = C.c_int(-1); dig = C.create_string_buffer(32)
    for nb, nk in ((31, 0), (23, 8), (0, 8), (1, 0), (0, 1)):                                      # 32 routes in all, and the smallest
        h = _create(L, set_id, [rm.params(k) for k in range(nb)], [(key.words,) + rm.params(100 + k) for k in range(nk)])
        assert h and L.zkv_risc0_router_route_count(h) == nb + nk + 1
        kinds = []
        for q in range(nb + nk + 1):
            assert L.zkv_risc0_router_route(h, q, sel, C.byref(keyed)) == 0
            kinds.append(keyed.value)
            assert L.zkv_risc0_router_route_verifier_key_digest(h, q, dig) == (INVALID_ARG if q == nb + nk else 0)
        assert kinds == [0] * nb + [1] * nk + [2] and sel.raw == sm.set_selector(set_id)
        assert L.zkv_risc0_router_route(h, nb + nk + 1, sel, C.byref(keyed)) == INVALID_ARG
        L.zkv_ctx_destroy(h)
    # the set selector is the set-inclusion context's for the same image id
    from stylus_zkvm_verifiers_amd import RiscZeroSetInclusionVerifier, RiscZeroSetRouter, _lib
    raw = _lib.lib()
    rt = RiscZeroSetRouter(set_id, [one], [key.triple()])
    si = RiscZeroSetInclusionVerifier(one[0], one[1], set_id)
    o = C.create_string_buffer(4)
    assert raw.zkv_risc0_setincl_get_selector(si._h, o) == 0 and o.raw == rt.set_selector() == sm.set_selector(set_id)
    model = rsm.SetRouter(set_id, [one], [key.triple()])
    assert [x[0] for x in rt.routes()] == model.selectors and [x[1] for x in rt.routes()] == [0, 1, 2] and rt.routes()[2][2] is None
    assert raw.zkv_ctx_vm(rt._h) == 12
    assert rt.last_route_counts() == [0] * 5 and rt.set_last_counts() == (0, 0, 0, 0)
    path = [bytes([k]) * 32 for k in range(3)]
    assert rt.encode_seal(path, b'\1\2\3') == model.encode_seal(path, b'\1\2\3')
    assert not rt.has_root(bytes(32))
    si.close()
    # Python refuses what the library refuses
    for bad in (dict(routes=[], keyed=[]), dict(routes=[one, one]), dict(routes=[rm.params(k) for k in range(32)])):
        with pytest.raises(ValueError):
            RiscZeroSetRouter(set_id, **bad)
    with pytest.raises(ValueError):
        RiscZeroSetRouter(set_id[:31], [one])
    with pytest.raises(ValueError):
        rsm.SetRouter(set_id, [rm.params(k) for k in range(32)])
    rt.close()


def test_wrong_context_in_both_directions_and_argument_errors(L, key, real_proofs):
    from stylus_zkvm_verifiers_amd import RiscZeroRouter, RiscZeroSetInclusionVerifier, RiscZeroSetRouter, risc0_router_wire
    assert risc0_router_wire.lib() is L                              # (binds the argument types of zkv_risc0_router_wire.h's entry points)
    r = real_proofs['risc0']
    one = (H(r['control_root']), H(r['bn254_control_id']))
    set_id = m.sha256(b'a set builder')
    plain, with_set, si = RiscZeroRouter([one]), RiscZeroSetRouter(set_id, [one]), RiscZeroSetInclusionVerifier(one[0], one[1], set_id)
    o4 = C.create_string_buffer(4); st = C.c_uint8(0); cnt = (C.c_uint64 * 8)(); rep = (C.c_uint32 * 4)()
    off = (C.c_uint64 * 2)(0, 4)
    for h in (plain._h, si._h, None):                                # the set route's calls on a context that has none
        assert L.zkv_risc0_router_set_selector(h, o4) == WRONG_CTX
        assert L.zkv_risc0_router_set_has_root(h, bytes(32)) == WRONG_CTX
        assert L.zkv_risc0_router_set_submit_root(h, bytes(32), b'abcd', 4, C.byref(st), o4) == WRONG_CTX
        assert L.zkv_risc0_router_set_last_counts(h, cnt) == WRONG_CTX
        assert L.zkv_diag_rzset_groups(h, 1, b'abcd', off, 0, 0, rep) == WRONG_CTX
    for h in (si._h, None):                                          # the ragged call is every router's, and only a router's
        assert L.zkv_risc0_router_verify_ragged_dev(h, 1, 8, 8, 4, 8, 8, 8, None, None) == WRONG_CTX
    # the entry points that are out of scope on a router with a set route
    g = with_set._h
    assert L.zkv_risc0_router_verify_batch_dev(g, 1, 8, 8, 8, 8, None, None) == WRONG_CTX
    assert L.zkv_risc0_router_verify_call_batch_dev(g, 1, None, 8, 8, 8, 8, None, None) == WRONG_CTX
    assert L.zkv_risc0_router_verify_call_batch(g, 1, None, b'abcd', off, bytes(32), bytes(32), C.byref(st), None) == WRONG_CTX
    assert L.zkv_risc0_router_eth_call_batch_dev(g, 1, 8, 8, 4, 8, None, None, None) == WRONG_CTX
    assert L.zkv_risc0_router_eth_call_batch(g, 1, b'abcd', off, C.byref(st), C.create_string_buffer(96), (C.c_uint32 * 1)(), C.byref(st)) == WRONG_CTX
    assert L.zkv_risc0_router_last_call_counts(g, cnt) == WRONG_CTX
    # ... and are what they were on a router without one: argument errors and the device come next
    assert L.zkv_risc0_router_verify_batch_dev(plain._h, 1, None, 8, 8, 8, None, None) == INVALID_ARG
    assert L.zkv_risc0_router_last_call_counts(plain._h, cnt) == 0
    # argument errors of the new calls, before any device is touched
    for h in (plain._h, g):
        for miss in range(3):
            args = [8, 8, 8]
            args[miss] = None
            assert L.zkv_risc0_router_verify_ragged_dev(h, 1, 8, args[0], 4, args[1], None, args[2], None, None) == INVALID_ARG, miss
        assert L.zkv_risc0_router_verify_ragged_dev(h, 1, None, 8, 4, 8, None, 8, None, None) == INVALID_ARG       # bytes to read and no blob
        assert L.zkv_risc0_router_verify_ragged_dev(h, 0, None, None, 0, None, None, None, None, None) == 0
        assert L.zkv_risc0_router_verify_ragged_dev(h, 0xFFFFFFF1, 8, 8, 4, 8, None, 8, None, None) == INVALID_ARG
    assert L.zkv_risc0_router_set_selector(g, None) == INVALID_ARG
    assert L.zkv_risc0_router_set_has_root(g, None) == INVALID_ARG
    assert L.zkv_risc0_router_set_submit_root(g, None, b'abcd', 4, C.byref(st), o4) == INVALID_ARG
    assert L.zkv_risc0_router_set_submit_root(g, bytes(32), None, 4, C.byref(st), o4) == INVALID_ARG
    assert L.zkv_risc0_router_set_submit_root(g, bytes(32), b'abcd', 4, None, o4) == INVALID_ARG
    assert L.zkv_risc0_router_set_last_counts(g, None) == INVALID_ARG
    back = (C.c_uint64 * 2)(4, 0)
    assert L.zkv_diag_rzset_groups(g, 1, b'abcd', back, 0, 0, rep) == INVALID_ARG
    assert L.zkv_diag_rzset_groups(g, 1, b'abcd', off, 32, 0, rep) == INVALID_ARG
    assert L.zkv_diag_rzset_groups(g, 1, None, off, 0, 0, rep) == INVALID_ARG
    assert L.zkv_diag_rzset_groups(g, (1 << 20) + 1, b'abcd', off, 0, 0, rep) == INVALID_ARG
    for x in (plain, with_set, si):
        x.close()


# ---------------------------------------------------------------- the fixture is the model's
def test_fixture_equals_the_model(fx, keys):
    b = fx['builtin']
    model = rsm.SetRouter(H(fx['set_id']), [(H(b['control_root']), H(b['bn254_control_id']))], [k.triple() for k in keys])
    assert [s.hex() for s in model.selectors] == fx['route_selectors'] and model.set_selector.hex() == fx['set_selector']
    for s in fx['submitted_roots']:
        assert model.submit_root(H(s['root']), H(s['seal']))[0] == rsm.OK
    seen = set()
    for c in fx['cases']:
        seal, a, j = H(c['seal']), H(c['image_id']), H(c['journal_digest'])
        assert model.verify(seal, a, j) == (c['status'], H(c['received'])), c['name']
        assert model.verify_integrity(seal, m.receipt_claim_ok_digest(a, j)) == (c['status'], H(c['received'])), c['name']
        assert model.route(seal) == c['route']
        seen.add((c['status'], c['route']))
    assert seen >= {(0, rsm.SET), (1, rsm.SET), (4, rsm.SET), (8, rsm.SET), (0, 0), (0, 1), (0, 2), (8, rm.NOT_FOUND), (4, rm.SHORT)}
    # the library's own host decoder of the on-chain form agrees with the model about which bodies are canonical
    from stylus_zkvm_verifiers_amd import RiscZeroSetInclusionVerifier
    si = RiscZeroSetInclusionVerifier(H(b['control_root']), H(b['bn254_control_id']), H(fx['set_id']))
    for c in fx['cases']:
        if c['route'] == rsm.SET:
            d = sm.abi_decode_seal(H(c['seal'])[4:])
            st, _, path, root_seal = si.decode_seal(H(c['seal']))
            assert (st == 0) == (d is not None), c['name']
            if d is not None:
                assert (b''.join(bytes(p) for p in path) if isinstance(path, (list, tuple)) else bytes(path), bytes(root_seal)) == (b''.join(d[0]), d[1]), c['name']
    si.close()


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


def _want(seal, set_sel):
    """rzs_parse's answer from the model's decoder: "kind depth root_len root_at"."""
    if len(seal) < 4 or seal[:4] != set_sel:
        return '%d 0 0 0' % NOT_SET
    d = sm.abi_decode_seal(seal[4:])
    if d is None:
        return '%d 0 0 0' % MALFORMED
    return '%d %d %d %d' % (CLAIM, len(d[0]), len(d[1]), 4 + 128 + 32 * len(d[0]) + 32)


def _mutations(set_sel):
    """4,000 seeded mutations of canonical seals: an offset word, a length word, the padding, the total length by 1 or 32 either way."""
    rng = random.Random(0x5E7A7E71)
    word = lambda v: (v % (1 << 256)).to_bytes(32, 'big')
    out = []
    for trial in range(4000):
        k = rng.choice([0, 0, 1, 2, 3, 7])
        ln = rng.choice([0, 1, 3, 4, 31, 32, 33, 64, 259, 260, 261])
        seal = bytearray(set_sel + sm.abi_encode_seal([bytes(rng.randrange(256) for _ in range(32)) for _ in range(k)], bytes(rng.randrange(1, 256) for _ in range(ln))))
        l_at = 4 + 128 + 32 * k
        what = rng.randrange(8)
        if what < 5:                                                 # a header word: the three offsets, the two lengths
            at = rng.choice([4, 36, 68, 100, l_at])
            cur = int.from_bytes(seal[at:at + 32], 'big')
            val = rng.choice([0, 1, 31, 32, 33, 0x20, 0x40, 0x60, 0x80, cur, cur + 1, cur - 1, cur + 32, cur - 32, cur + (1 << 32), cur + (1 << 64), cur + (1 << 248),
                              (1 << 32) - 1, 1 << 32, (1 << 32) + 1, (1 << 32) - 32, (1 << 37) - 32, 1 << 59, 1 << 63, (1 << 64) - 1, 1 << 64, (1 << 64) - 32,
                              (1 << 64) + 0x60, (1 << 256) - 1, (1 << 256) - 32, rng.randrange(200), rng.randrange(1 << 256)])
            seal[at:at + 32] = word(val)
        elif what == 5 and -ln % 32:                                 # a padding byte
            seal[l_at + 32 + ln + rng.randrange(-ln % 32)] = rng.randrange(1, 256)
        elif what == 6:                                              # shorter
            del seal[len(seal) - rng.choice([1, 32]):]
        else:                                                        # longer
            seal += bytes(rng.choice([1, 32]))
        out.append((SHIFTS[trial & 3], bytes(seal)))
    return out


@pytest.mark.parametrize('flags,name', [([], 'plain'), (SANITIZE, 'san')])
def test_kernel_header_arithmetic_equals_the_model_decoder(tmp_path, fx, flags, name):
    """The function k_rzset_front calls, on every fixture seal (four base offsets) and on the seeded mutations, each read from a heap
    block of exactly the seal's length."""
    exe = _program(tmp_path, flags, name)
    set_sel = H(fx['set_selector'])
    reqs = [(shift, H(c['seal'])) for c in fx['cases'] for shift in SHIFTS] + _mutations(set_sel)
    got = _run(exe, 'parse', ['%d %s %s' % (shift, set_sel.hex(), seal.hex() or '-') for shift, seal in reqs])
    seen = {NOT_SET: 0, MALFORMED: 0, CLAIM: 0}
    for (shift, seal), line in zip(reqs, got):
        assert line == _want(seal, set_sel), (shift, seal[:200].hex(), len(seal))
        seen[int(line.split()[0])] += 1
    assert seen[NOT_SET] >= 36 and seen[MALFORMED] > 2000 and seen[CLAIM] > 300, seen
    # another selector in front of a canonical body is not a set seal
    other = bytes(4)
    assert _run(exe, 'parse', ['0 %s %s' % (other.hex(), H(fx['cases'][-1]['seal']).hex())]) == ['0 0 0 0']


@pytest.mark.parametrize('flags,name', [([], 'plain'), (SANITIZE, 'san')])
def test_identity_is_decided_by_the_bytes(tmp_path, flags, name):
    """Fingerprint and byte comparison: equal seals are equal at every alignment and share a fingerprint; a 259-byte seal and the 260-byte
    seal it begins, two seals that differ only in byte 259 and two that differ only in the first byte are different seals."""
    exe = _program(tmp_path, flags, name)
    rng = random.Random(0x5E7A7E72)
    s260 = bytes(rng.randrange(256) for _ in range(260))
    pairs = []
    for sa in SHIFTS:
        for sb in SHIFTS:
            pairs += [(sa, sb, s260, s260, True), (sa, sb, s260[:259], s260, False), (sa, sb, s260, s260[:259] + bytes([s260[259] ^ 1]), False),
                      (sa, sb, bytes([s260[0] ^ 0x80]) + s260[1:], s260, False), (sa, sb, s260[:259], s260[:259], True), (sa, sb, b'', b'', True),
                      (sa, sb, s260[:3], s260[:3], True), (sa, sb, s260[:3], s260[:4], False), (sa, sb, s260 + b'\1', s260 + b'\2', False),
                      (sa, sb, s260 + bytes(40), s260 + bytes(40), True), (sa, sb, s260[:259] + b'\0', s260[:259], False)]
    got = _run(exe, 'ident', ['%d %d %s %s' % (sa, sb, a.hex() or '-', b.hex() or '-') for sa, sb, a, b, _ in pairs])
    fps = set()
    for (sa, sb, a, b, same), line in zip(pairs, got):
        fa, fb, eq = line.split()
        assert (eq == '1') == same, (sa, sb, len(a), len(b))
        if same:
            assert fa == fb
        fps.add((a, fa)); fps.add((b, fb))
    assert len({a for a, _ in fps}) == len(fps)                       # a seal's fingerprint does not depend on where it lies
    # the fingerprint sees the length and the last byte (a collision is allowed, these are not): the table is not one long probe chain
    by = dict(fps)
    assert by[s260] != by[s260[:259]] and by[s260] != by[s260[:259] + bytes([s260[259] ^ 1])]

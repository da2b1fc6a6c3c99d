"""RISC Zero set-inclusion receipts (include/zkv_risc0_set_inclusion.h), everything that needs no GPU: the header and its symbols,
creation rules, the context-kind checks, the on-chain seal codec against tests/set_inclusion_model.py, the host build of the device math
(csrc/zkv_setincl.h through tests/host_cpp/test_setincl.cpp, plain and under the sanitizers) on every hash case of the fixture, and the
model against the fixture's cheap cases.  PARITY UNPINNED: the reference holds no set verifier."""
import ctypes as C
import json
import os
import re
import subprocess

import numpy as np
import pytest

import set_inclusion_model as sm
import spec_model as m

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
SRC = os.path.join(HERE, 'host_cpp', 'test_setincl.cpp')
H = bytes.fromhex
NEW = ['zkv_risc0_setincl_create', 'zkv_risc0_setincl_create_keyed', 'zkv_risc0_setincl_verify_batch', 'zkv_risc0_setincl_verify_integrity_batch',
       'zkv_risc0_setincl_verify_batch_dev', 'zkv_risc0_setincl_submit_root', 'zkv_risc0_setincl_has_root', 'zkv_risc0_setincl_get_selector',
       'zkv_risc0_setincl_last_counts', 'zkv_risc0_setincl_seal_encode', 'zkv_risc0_setincl_seal_decode', 'zkv_diag_setincl_roots']
WRONG_CTX, INVALID_ARG = -5, -1
SANITIZE = ['-fsanitize=address,undefined', '-fno-sanitize-recover=all']


def _names(path):
    return set(re.findall(r'\b(zkv_[a-z0-9_]+)\s*\(', re.sub(r'/\*.*?\*/', '', open(path).read(), flags=re.S)))


@pytest.fixture(scope='module')
def fx():
    return json.load(open(os.path.join(HERE, 'golden', 'set_inclusion_cases.json')))


@pytest.fixture(scope='module')
def L():
    from stylus_zkvm_verifiers_amd import risc0_set_inclusion
    return risc0_set_inclusion.lib()


@pytest.fixture()
def keyed(fx):
    from stylus_zkvm_verifiers_amd import RiscZeroSetInclusionVerifier
    k = fx['keyed']
    v = RiscZeroSetInclusionVerifier(H(k['control_root']), H(k['bn254_control_id']), H(fx['set_builder_image_id']), vk_words=H(k['vk_words']),
                                     root_selector=H(k['root_selector']))
    yield v
    v.close()


# ---------------------------------------------------------------- symbol sets
def test_header_declares_exactly_the_new_symbols_and_the_library_exports_them(L):
    hdr = os.path.join(ROOT, 'include', 'zkv_risc0_set_inclusion.h')
    assert _names(hdr) == set(NEW)
    text = open(hdr).read()
    assert '#include "zkv.h"' in text and 'PARITY UNPINNED' in text and 'diagnostics' in text
    assert 'SYNCHRONISES ITS STREAM' in text                        # the device-resident call reads the job count back
    for define in ('ZKV_VM_RISC0_SETINCL 11', 'ZKV_SETINCL_MAX_DEPTH 64', 'ZKV_SETINCL_STORED 0xFFFFFFFFu', 'ZKV_SETINCL_MAX_ROOTS 4096'):
        assert '#define ' + define in text
    from stylus_zkvm_verifiers_amd import _lib, risc0_set_inclusion as rs
    assert set(rs.SYMBOLS) == set(NEW) and not set(NEW) & set(_lib.SYMBOLS)
    for name in NEW:
        assert hasattr(L, name), name
    main = _names(os.path.join(ROOT, 'include', 'zkv.h'))
    assert len(main) == 83 and len(_lib.SYMBOLS) == 83 and not main & set(NEW)
    assert (rs.STORED, rs.MAX_DEPTH, rs.MAX_ROOTS, rs.KEY_BYTES) == (sm.STORED, sm.MAX_DEPTH, sm.MAX_ROOTS, 832)


def test_the_class_is_exported_next_to_the_others():
    import stylus_zkvm_verifiers_amd as z
    assert 'RiscZeroSetInclusionVerifier' in z.__all__ and z.RiscZeroSetInclusionVerifier is z.risc0_set_inclusion.RiscZeroSetInclusionVerifier


# ---------------------------------------------------------------- creation rules and context kinds
def test_creation_argument_rules(L, fx):
    from stylus_zkvm_verifiers_amd import RiscZeroSetInclusionVerifier as V
    k = fx['keyed']
    cr, cid, sid, vk, sel = H(k['control_root']), H(k['bn254_control_id']), H(fx['set_builder_image_id']), H(k['vk_words']), H(k['root_selector'])
    assert not L.zkv_risc0_setincl_create(None, cid, sid, 0) and not L.zkv_risc0_setincl_create(cr, None, sid, 0)
    assert not L.zkv_risc0_setincl_create(cr, cid, None, 0)
    for hole in range(5):
        args = [vk, sel, cr, cid, sid]
        args[hole] = None
        assert not L.zkv_risc0_setincl_create_keyed(*args, 0)
    for bad in (dict(control_root=cr[:31]), dict(bn254_control_id=cid + b'\0'), dict(set_builder_image_id=b'')):
        kw = dict(control_root=cr, bn254_control_id=cid, set_builder_image_id=sid)
        kw.update(bad)
        with pytest.raises(ValueError):
            V(**kw)
    with pytest.raises(ValueError):
        V(cr, cid, sid, vk_words=vk)                                # a key without its selector
    with pytest.raises(ValueError):
        V(cr, cid, sid, root_selector=sel)
    with pytest.raises(ValueError):
        V(cr, cid, sid, vk_words=vk[:-64], root_selector=sel)       # n_ic = 5
    with pytest.raises(ValueError):
        V(cr, cid, sid, vk_words=vk, root_selector=sel + b'\0')
    for v in (V(cr, cid, sid), V(cr, cid, sid, vk_words=vk, root_selector=sel)):
        assert v.get_selector() == H(fx['set_selector']) == sm.set_selector(sid)
        assert not v.has_root(bytes(32)) and v.last_counts() == (0, 0, 0)
        v.close()


def test_context_kind_checks(L, fx, keyed):
    from stylus_zkvm_verifiers_amd import RiscZeroVerifier, _lib
    raw = _lib.lib()
    h = keyed.handle
    assert raw.zkv_ctx_vm(h) == 11
    assert raw.zkv_ctx_synchronize(h) == 0                          # nothing set up: nothing to wait for
    assert raw.zkv_ctx_set_lanes_per_proof(h, 2) == 0 and raw.zkv_ctx_set_lanes_per_proof(h, 0) == 0
    assert raw.zkv_ctx_shard_count(h) == 0
    one = np.zeros(1, dtype=np.uint64)
    buf = bytes(260)
    # the generic batch calls of the other kinds refuse the new kind
    assert raw.zkv_risc0_verify_batch(h, 1, buf, one.ctypes.data, buf, buf, None, None) == WRONG_CTX
    assert raw.zkv_risc0_verify_integrity_batch(h, 1, buf, one.ctypes.data, buf, None, None) == WRONG_CTX
    assert raw.zkv_risc0_verify_batch_dev(h, 1, None, None, None, None, None, None) == WRONG_CTX
    assert raw.zkv_groth16_verify_batch(h, 1, buf, buf, None) == WRONG_CTX
    assert raw.zkv_ctx_vk_x_batch(h, 1, buf, None) == WRONG_CTX
    assert raw.zkv_risc0_get_selector(h, C.create_string_buffer(4)) == WRONG_CTX
    assert raw.zkv_risc0_is_initialized(h) == 0
    assert raw.zkv_ctx_set_aggregate_check(h, 1, None) == INVALID_ARG
    assert not raw.zkv_ctx_create_sharded((C.c_void_p * 1)(h), 1)  # single-device
    # ... and the new calls refuse the other kinds
    r = RiscZeroVerifier(0)
    st = C.c_uint8(0); sz = C.c_size_t(0)
    assert L.zkv_risc0_setincl_get_selector(r._h, C.create_string_buffer(4)) == WRONG_CTX
    assert L.zkv_risc0_setincl_has_root(r._h, bytes(32)) == WRONG_CTX
    assert L.zkv_risc0_setincl_last_counts(r._h, (C.c_uint64 * 3)()) == WRONG_CTX
    assert L.zkv_risc0_setincl_submit_root(r._h, bytes(32), buf, 260, C.byref(st), None) == WRONG_CTX
    assert L.zkv_risc0_setincl_verify_batch(r._h, 0, None, None, None, None, None, 0, None, None, None, None) == WRONG_CTX
    assert L.zkv_risc0_setincl_verify_integrity_batch(r._h, 0, None, None, None, None, 0, None, None, None, None) == WRONG_CTX
    assert L.zkv_risc0_setincl_verify_batch_dev(r._h, 0, None, None, None, None, 0, None, 0, None, None, None, None) == WRONG_CTX
    assert L.zkv_diag_setincl_roots(r._h, 0, None, None, None, None, 0, None) == WRONG_CTX
    assert L.zkv_risc0_setincl_seal_encode(r._h, None, 0, None, 0, None, 0) == 0
    assert L.zkv_risc0_setincl_seal_decode(r._h, buf, 260, C.byref(st), None, C.byref(sz), C.byref(sz), C.byref(sz), C.byref(sz)) == WRONG_CTX
    r.close()


def test_batch_argument_rules_without_a_device(L, keyed):
    h = keyed.handle
    off = np.array([0, 2, 1], dtype=np.uint32)                      # offsets that run backwards
    idx = np.zeros(2, dtype=np.uint32); st = np.zeros(2, dtype=np.uint8)
    so = np.array([0, 260], dtype=np.uint64)
    a = bytes(64)
    assert L.zkv_risc0_setincl_verify_batch(h, 0, None, None, None, None, None, 0, None, None, None, None) == 0
    assert L.zkv_risc0_setincl_verify_batch(h, 2, a, a, a, off.ctypes.data, idx.ctypes.data, 1, bytes(260), so.ctypes.data, st.ctypes.data, None) == INVALID_ARG
    off = np.array([0, 1, 2], dtype=np.uint32)
    assert L.zkv_risc0_setincl_verify_batch(h, 2, None, a, a, off.ctypes.data, idx.ctypes.data, 1, bytes(260), so.ctypes.data, st.ctypes.data, None) == INVALID_ARG
    assert L.zkv_risc0_setincl_verify_batch(h, 2, a, None, a, off.ctypes.data, idx.ctypes.data, 1, bytes(260), so.ctypes.data, st.ctypes.data, None) == INVALID_ARG
    assert L.zkv_risc0_setincl_verify_batch(h, 2, a, a, None, off.ctypes.data, idx.ctypes.data, 1, bytes(260), so.ctypes.data, st.ctypes.data, None) == INVALID_ARG
    assert L.zkv_risc0_setincl_verify_batch(h, 2, a, a, a, off.ctypes.data, idx.ctypes.data, 1, None, so.ctypes.data, st.ctypes.data, None) == INVALID_ARG
    assert L.zkv_risc0_setincl_verify_batch(h, 2, a, a, a, off.ctypes.data, idx.ctypes.data, 1, bytes(260), so.ctypes.data, None, None) == INVALID_ARG
    bad = np.array([260, 0], dtype=np.uint64)
    assert L.zkv_risc0_setincl_verify_batch(h, 2, a, a, a, off.ctypes.data, idx.ctypes.data, 1, bytes(260), bad.ctypes.data, st.ctypes.data, None) == INVALID_ARG
    assert L.zkv_risc0_setincl_verify_batch_dev(h, 2, None, None, None, None, 0, None, 0, None, None, None, None) == INVALID_ARG
    assert L.zkv_diag_setincl_roots(h, 2, a, a, a, off.ctypes.data, 32, st.ctypes.data) == INVALID_ARG       # blob_shift past 31
    with pytest.raises(ValueError):
        keyed.verify_batch([bytes(32)], [bytes(32)], [bytes(31)], [0], [bytes(260)])
    with pytest.raises(ValueError):
        keyed.verify_batch([bytes(32)], [bytes(32)], [b''], [0, 0], [bytes(260)])


# ---------------------------------------------------------------- the on-chain form
def _variants(body):
    """Non-canonical bodies made from a canonical one (path of k siblings, root seal of ln bytes)."""
    k = int.from_bytes(body[96:128], 'big')
    at = 128 + 32 * k
    ln = int.from_bytes(body[at:at + 32], 'big')
    w = lambda v: m.be32(v)
    out = {'wrong first word': w(0x40) + body[32:], 'first word high byte': b'\x01' + body[1:],
           'swapped offsets': body[:32] + body[64:96] + body[32:64] + body[96:],
           'path offset off by a word': body[:32] + w(0x60) + body[64:],
           'root seal offset off by a word': body[:64] + w(0x60 + 32 * k + 32) + body[96:],
           'trailing word': body + bytes(32), 'trailing byte': body + b'\0', 'cut short': body[:-32], 'cut by a byte': body[:-1],
           'path length overflow': body[:96] + w(1 << 255) + body[128:], 'path length 2^32 + k': body[:96] + w((1 << 32) + k) + body[128:],
           'path longer than the body': body[:96] + w(len(body) // 32) + body[128:],
           'root seal length overflow': body[:at] + w((1 << 256) - 32) + body[at + 32:],
           'root seal length 2^32 + len': body[:at] + w((1 << 32) + ln) + body[at + 32:],
           'root seal longer than the body': body[:at] + w(ln + 32) + body[at + 32:]}
    if ln % 32:
        out['dirty padding'] = body[:-1] + b'\x01'
        out['dirty first padding byte'] = body[:at + 32 + ln] + b'\x80' + body[at + 33 + ln:]
    return out


def test_seal_codec_round_trips_and_refuses_every_non_canonical_form(keyed, fx):
    model = sm.SetVerifier(None, H(fx['set_builder_image_id']))
    rng = sm.rng(0xC0DEC)
    sel = keyed.get_selector()
    seen = set()
    for k, ln in ((0, 0), (0, 260), (1, 260), (5, 259), (64, 260), (65, 1), (3, 32), (2, 33), (7, 31)):
        path = [bytes(rng.randrange(256) for _ in range(32)) for _ in range(k)]
        root_seal = bytes(rng.randrange(1, 256) for _ in range(ln))
        seal = keyed.encode_seal(path, root_seal)
        assert seal == model.encode_seal(path, root_seal) and seal[:4] == sel
        assert keyed.encode_seal(b''.join(path), root_seal) == seal
        assert keyed.decode_seal(seal) == (0, bytes(4), b''.join(path), root_seal)
        assert model.decode_seal(seal) == (0, None, path, root_seal)
        for name, body in _variants(seal[4:]).items():
            assert model.decode_seal(sel + body)[0] == m.INVALID_PROOF_DATA, name
            assert keyed.decode_seal(sel + body) == (m.INVALID_PROOF_DATA, bytes(4), None, None), name
            seen.add(name)
        other = b'\x00' + sel[1:]
        assert keyed.decode_seal(other + seal[4:]) == (m.SELECTOR_MISMATCH, other, None, None) == model.decode_seal(other + seal[4:])[:2] + (None, None)
        assert keyed.decode_seal(other + b'garbage') == (m.SELECTOR_MISMATCH, other, None, None)       # the selector is judged before the body
    assert {'wrong first word', 'swapped offsets', 'dirty padding', 'trailing word', 'path length overflow', 'root seal length overflow'} <= seen
    for short in (b'', sel[:3]):
        assert keyed.decode_seal(short) == (m.INVALID_PROOF_DATA, bytes(4), None, None) and model.decode_seal(short)[0] == m.INVALID_PROOF_DATA
    assert keyed.decode_seal(sel)[0] == m.INVALID_PROOF_DATA        # a selector and no body
    # the length query of the encoder writes nothing
    need = keyed._L.zkv_risc0_setincl_seal_encode(keyed.handle, bytes(64), 2, bytes(5), 5, None, 0)
    assert need == 4 + 32 * 5 + 64 + 32
    small = C.create_string_buffer(b'\xAA' * need, need)
    assert keyed._L.zkv_risc0_setincl_seal_encode(keyed.handle, bytes(64), 2, bytes(5), 5, small, need - 1) == need and small.raw == b'\xAA' * need


# ---------------------------------------------------------------- the device math, compiled for the host
def _program(tmp_path, flags, name):
    exe = str(tmp_path / name)
    subprocess.check_call(['g++', '-std=c++17', '-O1', '-g', '-Wall', '-Wno-unknown-pragmas'] + flags + ['-o', exe, SRC])
    return exe


def _run(exe, lines):
    out = subprocess.run([exe], input=''.join(ln + '\n' for ln in lines).encode(), stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120)
    assert out.returncode == 0, (out.returncode, out.stderr.decode()[-2000:])
    assert not out.stderr, out.stderr.decode()[-2000:]
    got = out.stdout.decode().splitlines()
    assert len(got) == len(lines)
    return got


def _hash_requests(fx):
    h = fx['hash']
    req = [('K %s' % (c['msg'] or '-'), c['digest']) for c in h['keccak']]
    req += [('L %s' % c['claim'], c['leaf']) for c in h['leaf']]
    req += [('N %s %s' % (c['a'], c['b']), c['node']) for c in h['node']]
    req += [('J %s %s' % (fx['set_builder_image_id'], c['root']), c['digest']) for c in h['journal']]
    req += [('W %s %s' % (c['claim'], c['path'] or '-'), c['root']) for c in h['walks']]
    # the walk at each depth of the long paths: every prefix of the depth-65 path
    deep = [c for c in h['walks'] if c['name'] == 'depth65'][0]
    for d in range(0, 66):
        path = [H(deep['path'])[32 * k:32 * k + 32] for k in range(d)]
        req.append(('W %s %s' % (deep['claim'], b''.join(path).hex() or '-'), sm.walk(H(deep['claim']), path).hex()))
    return req


@pytest.mark.parametrize('flags,name', [([], 'plain'), (SANITIZE, 'san')])
def test_host_build_of_the_device_math_gives_every_hash_case(tmp_path, fx, flags, name):
    exe = _program(tmp_path, flags, name)
    req = _hash_requests(fx)
    assert len(req) > 120
    got = _run(exe, [r for r, _ in req])
    for (r, want), g in zip(req, got):
        assert g == want, r[:80]


# ---------------------------------------------------------------- the model against the fixture (the cases that cost no pairing)
def test_model_reproduces_the_cheap_cases_of_the_fixture(fx):
    sid = H(fx['set_builder_image_id'])
    h = fx['hash']
    assert h['keccak'][0]['digest'] == 'c5d2460186f7233c927e7db2dcc703c0e500b653ca82273b7bfad8045d85a470'      # keccak256("")
    assert h['keccak'][1] == {'msg': '616263', 'digest': '4e03657aea45a94fc7d47ba826c8d667c0d1e6e33a64a036ec44f58fa12d6c45'}
    for c in h['keccak']: assert m.keccak256(H(c['msg'])).hex() == c['digest']
    for c in h['leaf']: assert sm.leaf(H(c['claim'])).hex() == c['leaf']
    assert {c['name'] for c in h['node']} >= {'a<b', 'a>b', 'a==b'}
    for c in h['node']: assert sm.node(H(c['a']), H(c['b'])).hex() == c['node'] == sm.node(H(c['b']), H(c['a'])).hex()
    for c in h['journal']: assert sm.root_journal(sid, H(c['root'])).hex() == c['digest']
    depths = set()
    for c in h['walks']:
        path = [H(c['path'])[k:k + 32] for k in range(0, len(c['path']) // 2, 32)]
        assert m.receipt_claim_ok_digest(H(c['image_id']), H(c['journal_digest'])).hex() == c['claim']
        assert sm.walk(H(c['claim']), path).hex() == c['root']
        depths.add(len(path))
    assert depths == {0, 1, 2, 3, 4, 5, 20, 64, 65}
    for size in (1, 2, 3, 5, 8, 21):                                 # every leaf of a tree walks to the tree's one root
        assert len({c['root'] for c in h['walks'] if c['name'].startswith('tree%d/' % size)}) == 1
        assert len([c for c in h['walks'] if c['name'].startswith('tree%d/' % size)]) == size
    # statuses that no pairing decides, with a model whose inner verifier must not be asked for anything but the front checks
    k = fx['keyed']
    inner = sm.KeyedRisc0Verifier(None, H(k['root_selector']), H(k['control_root']), H(k['bn254_control_id']))
    sv = sm.SetVerifier(inner, sid)
    seals = [H(s) for s in k['root_seals']]
    kinds = {}
    for c in k['claims']:
        kinds[c['kind']] = kinds.get(c['kind'], 0) + 1
        path = [H(c['path'])[q:q + 32] for q in range(0, len(c['path']) // 2, 32)]
        assert m.receipt_claim_ok_digest(H(c['image_id']), H(c['journal_digest'])).hex() == c['claim']
        if c['kind'] in ('bad_selector', 'short_seal', 'bad_index', 'deep'):
            st, recv = sv.verify(H(c['image_id']), H(c['journal_digest']), path, c['root_idx'], seals)
            assert (st, (recv or bytes(4)).hex()) == (c['status'], c['recv']) and c['status_unsubmitted'] == st
        elif c['root_idx'] == sm.STORED:
            assert c['status_unsubmitted'] == m.VERIFICATION_FAILED
            sv.roots = {H(k['stored']['root'])}
            assert sv.verify(H(c['image_id']), H(c['journal_digest']), path, sm.STORED, seals)[0] == c['status']
            sv.roots = set()
    assert len(k['claims']) == 200 and kinds['honest'] >= 180 and kinds['straggler'] == 4
    assert all(kinds[x] == 1 for x in ('wrong_seal', 'bad_selector', 'big_coordinate', 'short_seal', 'bad_index', 'deep', 'depth64'))
    assert len(H(k['vk_words'])) == 448 + 64 * 6 and len(seals[5]) == 259 and int.from_bytes(seals[4][4:36], 'big') >= m.P
    r = fx['real']
    real = json.load(open(os.path.join(HERE, 'golden', 'real_proofs.json')))['risc0']
    assert r['root_seals'][0] == real['seal'] and r['root_seals'][1][8:] == real['seal'][8:] and r['status'] == [m.VERIFICATION_FAILED, m.SELECTOR_MISMATCH]
    assert os.path.getsize(os.path.join(HERE, 'golden', 'set_inclusion_cases.json')) < 256 * 1024

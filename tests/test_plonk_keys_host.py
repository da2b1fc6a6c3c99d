"""PLONK core for any key (include/zkv_plonk_keys.h), CPU side: header and symbols, context creation rules, and the host build of the
generic pre-pairing stage (plonk_prepare with the public inputs read from the proof's row) on every case of
tests/golden/plonk_keys_cases.json.  PARITY UNPINNED BY CONSTRUCTION: the reference holds no PLONK code; expectations are the verdicts
of oracle/plonk_model.plonk_verify (and of the C oracle where it takes the key), on trapdoor keys (tests/plonk_trapdoor_keys.py)."""
import ctypes as C
import json
import os
import re
import subprocess

import pytest

import oracle_lib as ol
import plonk_trapdoor_keys as T
import spec_model as m

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
H = bytes.fromhex


@pytest.fixture(scope='module')
def fx():
    return json.load(open(os.path.join(HERE, 'golden', 'plonk_keys_cases.json')))


@pytest.fixture(scope='module')
def hspk():
    src = os.path.join(HERE, 'host_sim', 'host_sim_plonk_keys.cpp')
    lib = os.path.join(HERE, 'host_sim', 'libhost_sim_plonk_keys.so')
    csrc = os.path.join(ROOT, 'stylus_zkvm_verifiers_amd', 'csrc')
    deps = [src] + [os.path.join(csrc, f) for f in os.listdir(csrc) if f.endswith('.h')]
    if not os.path.exists(lib) or os.path.getmtime(lib) < max(os.path.getmtime(d) for d in deps):
        subprocess.check_call(['g++', '-O2', '-std=c++17', '-fPIC', '-shared', '-Wno-unknown-pragmas', '-o', lib, src])
    L = C.CDLL(lib)
    L.hspk_prepare.argtypes = [C.c_char_p, C.c_size_t, C.c_char_p, C.c_size_t, C.c_char_p, C.c_char_p]
    return L


def host_verdict(hspk, vk, proof, pub):
    """The host build's D and Q, then the 2-pair check e(D, [1]_2) e(-Q, [tau]_2) = 1 through the C oracle's ecPairing."""
    out = C.create_string_buffer(128)
    rc = hspk.hspk_prepare(vk, len(vk), proof, len(proof), b''.join(pub) + b'\0', out)
    assert rc in (0, 1)
    if rc == 0:
        return 0
    g2 = vk[-256:]
    res = ol.ecpairing(out.raw[:64] + g2[:128] + out.raw[64:] + g2[128:])
    return int(res is not None and res[-1] == 1)


# ---------------------------------------------------------------- header and symbols
def test_header_declares_exactly_the_new_symbols():
    from stylus_zkvm_verifiers_amd import _lib, plonk_keys
    hdr = open(os.path.join(ROOT, 'include', 'zkv_plonk_keys.h')).read()
    body = re.sub(r'/\*.*?\*/', '', hdr, flags=re.S)
    declared = set(re.findall(r'\b(zkv_\w+)\s*\(', body))
    assert declared == set(plonk_keys.SYMBOLS)
    assert '#include "zkv.h"' in hdr and '#define ZKV_VM_PLONK 9' in hdr and '#define ZKV_PLONK_MAX_PUBLIC 128' in hdr
    zkv_h = open(os.path.join(ROOT, 'include', 'zkv.h')).read()
    for s in declared:
        assert s not in zkv_h and s not in _lib.SYMBOLS, s
    L = plonk_keys.lib()                      # binds every symbol: AttributeError if one is not exported
    for s in declared:
        assert getattr(L, s) is not None
    import stylus_zkvm_verifiers_amd as z
    assert z.PlonkVerifier is plonk_keys.PlonkVerifier and 'PlonkVerifier' in z.__all__


# ---------------------------------------------------------------- creation without a device
def _word(v):
    return int(v).to_bytes(32, 'big')


def test_context_creation_rules_and_shape(fx):
    from stylus_zkvm_verifiers_amd import _lib, plonk_keys
    L = plonk_keys.lib()
    by = {(s['nb_public'], s['n_c']): T.vk_bytes(T.shape_key(s['nb_public'], s['n_c'])) for s in fx['shapes']}
    for (nb, nc), vk in by.items():
        assert len(vk) == (992 if nc == 0 else 1056)
        h = L.zkv_plonk_ctx_create(vk, len(vk), 0)
        assert h and L.zkv_ctx_vm(h) == plonk_keys.VM_PLONK
        a, b, c = C.c_size_t(), C.c_size_t(), C.c_size_t()
        assert L.zkv_plonk_key_shape(h, C.byref(a), C.byref(b), C.byref(c)) == 0
        assert (a.value, b.value, c.value) == (nb, nc, 32 * (24 + 3 * nc))
        assert L.zkv_plonk_key_shape(h, None, None, None) == 0
        L.zkv_ctx_destroy(h)
    vk0, vk1 = by[(3, 0)], by[(3, 1)]

    def with_word(vk, k, v):
        return vk[:32 * k] + _word(v) + vk[32 * k + 32:]
    bad = [
        (vk0[:-1], 'short'), (vk0 + b'\0', 'long'), (vk1[:-64], 'n_c = 1 length without Qcp'),
        (with_word(vk0, 5, 1), 'n_c = 1 with the n_c = 0 length'), (with_word(vk1, 5, 0), 'n_c = 0 with the n_c = 1 length'),
        (with_word(vk0, 5, 2), 'n_c = 2'), (with_word(vk0, 4, 129), 'nb_public = 129'),
        (with_word(vk0, 0, 1 << 64), 'size = 2^64'), (with_word(vk1, 6, 1 << 32), 'cci = 2^32'),
        (with_word(vk0, 4, (1 << 32) + 3), 'nb_public high limb'), (with_word(vk0, 5, 1 << 200), 'n_c high limb'),
        (with_word(vk1, 6, (1 << 255) + 1), 'cci high limb'), (b'', 'empty')]
    for vk, why in bad:
        assert L.zkv_plonk_ctx_create(vk, len(vk), 0) is None, why
    assert L.zkv_plonk_ctx_create(None, 992, 0) is None
    # accepted edge values: nb_public = 0 and 128, size just below 2^64, cci just below 2^32 (a key judged on the device, not refused)
    for vk in (by[(0, 0)], by[(128, 1)], with_word(vk0, 0, (1 << 64) - 1), with_word(vk1, 6, (1 << 32) - 1)):
        h = L.zkv_plonk_ctx_create(vk, len(vk), 0)
        assert h
        L.zkv_ctx_destroy(h)
    # wrong context, both directions (answered before any device work)
    h = L.zkv_plonk_ctx_create(vk1, len(vk1), 0)
    sp = L.zkv_sp1_ctx_create(0)
    g = L.zkv_groth16_ctx_create(bytes(448 + 64), 1, 1, 0)
    for other in (sp, g):
        assert L.zkv_plonk_verify_batch(other, 0, None, None, None) == _lib.ERR_WRONG_CTX
        assert L.zkv_plonk_verify_batch_dev(other, 0, None, None, None, None) == _lib.ERR_WRONG_CTX
        assert L.zkv_plonk_key_shape(other, None, None, None) == _lib.ERR_WRONG_CTX
    assert L.zkv_sp1_verify_batch(h, 0, None, None, None, None, None, None, None) == _lib.ERR_WRONG_CTX
    assert L.zkv_sp1_plonk_verify_batch(h, 0, None, None, None, None, None, None, None) == _lib.ERR_WRONG_CTX
    assert L.zkv_sp1_plonk_verify_batch_dev(h, 0, None, None, 0, None, None, None, None) == _lib.ERR_WRONG_CTX
    assert L.zkv_sp1_plonk_verifier_hash(h, C.create_string_buffer(32)) == _lib.ERR_WRONG_CTX
    assert L.zkv_groth16_verify_batch(h, 0, None, None, None) == _lib.ERR_WRONG_CTX
    assert L.zkv_ctx_vk_x_batch(h, 1, b'x' * 64, C.create_string_buffer(64)) == _lib.ERR_WRONG_CTX
    assert L.zkv_plonk_verify_batch(h, 1, None, None, None) == _lib.ERR_INVALID_ARG
    # shards: the same key on both, or nothing
    h2 = L.zkv_plonk_ctx_create(vk1, len(vk1), 0)
    other_key = by[(2, 1)]
    h3 = L.zkv_plonk_ctx_create(other_key, len(other_key), 0)
    assert L.zkv_ctx_create_sharded((C.c_void_p * 2)(h, h3), 2) is None
    assert L.zkv_ctx_create_sharded((C.c_void_p * 2)(h, sp), 2) is None
    s = L.zkv_ctx_create_sharded((C.c_void_p * 2)(h, h2), 2)
    assert s and L.zkv_ctx_vm(s) == plonk_keys.VM_PLONK and L.zkv_ctx_shard_count(s) == 2
    a, b, c = C.c_size_t(), C.c_size_t(), C.c_size_t()
    assert L.zkv_plonk_key_shape(s, C.byref(a), C.byref(b), C.byref(c)) == 0 and (a.value, b.value, c.value) == (3, 1, 864)
    L.zkv_ctx_destroy(s)
    for x in (h3, sp, g):
        L.zkv_ctx_destroy(x)


def test_python_wrapper_without_a_device(fx):
    from stylus_zkvm_verifiers_amd import plonk_keys
    vk = T.vk_bytes(T.shape_key(9, 0))
    v = plonk_keys.PlonkVerifier(vk)
    assert (v.nb_public, v.n_commitments, v.proof_bytes) == (9, 0, 768)
    with pytest.raises(ValueError):
        v.verify_batch([b'\0' * 767], [[b'\0' * 32] * 9])
    with pytest.raises(ValueError):
        v.verify_batch([b'\0' * 768], [[b'\0' * 32] * 8])
    v.close()
    with pytest.raises(ValueError):
        plonk_keys.PlonkVerifier(vk[:-1])


def test_vk_bytes_serialiser_matches_the_model():
    from stylus_zkvm_verifiers_amd import plonk_keys
    import plonk_model as pm
    for nc in (0, 1):
        vk = T.make_key(T.rng_for('serialiser', nc), 5, nc)
        g2w = lambda q: m.g2_words(q)
        got = plonk_keys.vk_bytes(vk['size'], vk['size_inv'], vk['generator'], vk['coset_shift'], vk['nb_public'],
                                  *[vk[k] for k in ('s1', 's2', 's3', 'ql', 'qr', 'qm', 'qo', 'qk')], g2w(vk['g2']), g2w(vk['g2_tau']),
                                  qcp=vk['qcp'][0] if nc else None, cci=vk['cci'][0] if nc else 0)
        assert got == pm.vk_bytes(T.public_key_dict(vk))


# ---------------------------------------------------------------- the host build of the generic stage
def test_generic_prepare_on_the_host_gives_every_fixture_verdict(fx, hspk):
    n = 0
    for sh in fx['shapes']:
        for name, vk, proof, pub, model, c_oracle in T.fixture_cases(sh):
            assert host_verdict(hspk, vk, proof, pub) == model, (sh['nb_public'], sh['n_c'], name)
            assert c_oracle in (None, model)
            n += 1
    assert n > 1000
    shapes = {(s['nb_public'], s['n_c']) for s in fx['shapes']}
    assert shapes == {(nb, nc) for nb in (0, 1, 2, 3, 8, 9, 31, 64, 128) for nc in (0, 1)}


def test_host_build_accepts_the_batch_pools(fx, hspk):
    for e in fx['pool']:
        vk, proofs, pub = T.pool_arrays(e)
        assert len(proofs) == T.POOL_N
        for j in range(T.POOL_N):
            assert host_verdict(hspk, vk, proofs[j].tobytes(), [x.tobytes() for x in pub[j]]) == 1, (e['nb_public'], e['n_c'], j)


def test_fixture_is_reproduced_by_the_model_and_the_forger(fx):
    """A sample re-forged from the seeds and re-verified by plonk_model, so that the fixture cannot drift from its generator."""
    import base64
    for sh in fx['shapes']:
        nb, nc = sh['nb_public'], sh['n_c']
        if nb not in (0, 3, 9) and (nb, nc) != (128, 1):
            continue
        assert base64.b64encode(T.forge_valid(nb, nc)).decode() == sh['proof']
        cases = list(T.fixture_cases(sh))
        for name, vk, proof, pub, model, _ in cases[:: max(1, len(cases) // 6)] + cases[-2:]:
            got = T.pm.plonk_verify(T.parse_vk(vk), T.pad27(proof), [int.from_bytes(x, 'big') for x in pub])
            assert int(got) == model, (nb, nc, name)
    e = fx['pool'][0]
    assert base64.b64decode(e['proofs'])[:32 * (24 + 3 * e['n_c'])] == T.forge_pool(e['nb_public'], e['n_c'], 0)


def test_sp1_golden_cases_as_two_input_generic_proofs(hspk):
    """The SP1 PLONK golden cases that reach the verifier (right selector, full length), run as nb_public = 2 generic proofs with inputs
    (program vkey, hash of the public values): the only genuinely proved proofs, tying the forged fixture to the toy circuit."""
    cases = json.load(open(os.path.join(HERE, 'golden', 'plonk_cases.json')))
    vk, vh = H(cases['vk']), H(cases['verifier_hash'])
    n = ok = 0
    for c in cases['cases']:
        proof = H(c['proof'])
        if len(proof) != 868 or proof[:4] != vh[:4]:
            continue
        pub = [H(c['vkey']), m.be32(m.sp1_hash_public_values(H(c['public_values'])))]
        got = host_verdict(hspk, vk, proof[4:], pub)
        assert got == (1 if c['status'] == 0 else 0), c['name']
        n += 1; ok += got
    assert n > 60 and ok >= 7

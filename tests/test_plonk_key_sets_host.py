"""PLONK key sets (include/zkv_plonk_set.h) without a device: the header against the library's exports, creation
rules, the getters and wrong-context answers, and the 64-slot layout (csrc/zkv_gset_layout.h pset_choose, host build) against a numpy
model.  PARITY UNPINNED BY CONSTRUCTION: the reference holds no PLONK code."""
import ctypes as C
import json
import os
import re
import subprocess

import numpy as np
import pytest

import plonk_trapdoor_keys as T

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
NEW = ['zkv_plonk_set_create', 'zkv_plonk_set_size', 'zkv_plonk_set_proof_stride', 'zkv_plonk_set_input_stride', 'zkv_plonk_set_key_shape',
       'zkv_plonk_set_verify_batch', 'zkv_plonk_set_verify_batch_dev']


@pytest.fixture(scope='module')
def fx():
    return json.load(open(os.path.join(HERE, 'golden', 'plonk_keys_cases.json')))


@pytest.fixture(scope='module')
def L():
    from stylus_zkvm_verifiers_amd import plonk_set
    return plonk_set.lib()


@pytest.fixture(scope='module')
def by(fx):
    return {(s['nb_public'], s['n_c']): T.vk_bytes(T.shape_key(s['nb_public'], s['n_c'])) for s in fx['shapes']}


def _create(L, vks, lens=None):
    k = len(vks)
    lens = [len(v) if v is not None else 992 for v in vks] if lens is None else lens
    return L.zkv_plonk_set_create(k, (C.c_char_p * max(k, 1))(*vks), (C.c_size_t * max(k, 1))(*lens), 0)


def _with_word(vk, k, v):
    return vk[:32 * k] + int(v).to_bytes(32, 'big') + vk[32 * k + 32:]


def test_header_declares_exactly_the_new_symbols_and_the_library_exports_them(L):
    hdr = open(os.path.join(ROOT, 'include', 'zkv_plonk_set.h')).read()
    body = re.sub(r'/\*.*?\*/', '', hdr, flags=re.S)
    assert set(re.findall(r'\b(zkv_[a-z0-9_]+)\s*\(', body)) == set(NEW)
    assert '#include "zkv.h"' in hdr and '#define ZKV_VM_PLONK_SET 10' in body and '#define ZKV_PLONK_SET_MAX_KEYS 256' in body
    from stylus_zkvm_verifiers_amd import _lib, plonk_set
    assert set(plonk_set.SYMBOLS) == set(NEW) and not set(NEW) & set(_lib.SYMBOLS)
    for name in NEW:
        assert getattr(L, name) is not None, name
    main = re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'zkv.h')).read(), flags=re.S)
    assert not set(re.findall(r'\b(zkv_[a-z0-9_]+)\s*\(', main)) & set(NEW)
    import stylus_zkvm_verifiers_amd as z
    assert z.PlonkVerifierSet is plonk_set.PlonkVerifierSet and 'PlonkVerifierSet' in z.__all__


def test_creation_rules_without_a_device(L, by):
    import stylus_zkvm_verifiers_amd as z
    vk0, vk1 = by[(3, 0)], by[(3, 1)]
    assert not _create(L, [])
    assert not _create(L, [vk0] * 257)
    h = _create(L, [vk0] * 256)
    assert h and L.zkv_plonk_set_size(h) == 256
    L.zkv_ctx_destroy(h)
    assert not L.zkv_plonk_set_create(1, None, (C.c_size_t * 1)(992), 0)
    assert not L.zkv_plonk_set_create(1, (C.c_char_p * 1)(vk0), None, 0)
    assert not _create(L, [vk0, None])
    assert not _create(L, [vk0, vk1], [len(vk0), len(vk1) - 1])               # bad length
    assert not _create(L, [vk0, vk0 + b'\0'])
    assert not _create(L, [vk1, _with_word(vk0, 5, 2)])                        # n_c = 2
    assert not _create(L, [vk1, _with_word(vk0, 4, 129)])                      # nb_public = 129
    assert not _create(L, [_with_word(vk0, 0, 1 << 64)])                       # size = 2^64
    # keys with an invalid point or a field element >= R are accepted (their proofs answer 0 on the device)
    bad_pt = vk0[:224] + int(T.P).to_bytes(32, 'big') + vk0[256:]
    bad_r = _with_word(vk1, 1, T.R)
    h = _create(L, [bad_pt, vk1, bad_r])
    assert h and L.zkv_plonk_set_size(h) == 3
    L.zkv_ctx_destroy(h)
    with pytest.raises(ValueError):
        z.PlonkVerifierSet([])
    with pytest.raises(ValueError):
        z.PlonkVerifierSet([vk0] * 257)
    with pytest.raises(ValueError):
        z.PlonkVerifierSet([vk0, _with_word(vk0, 5, 2)])


def test_getters_on_a_set_of_mixed_shapes(L, by):
    import stylus_zkvm_verifiers_amd as z
    from stylus_zkvm_verifiers_amd import _lib
    shapes = [(0, 0), (9, 1), (2, 0), (128, 0)]
    s = z.PlonkVerifierSet([by[sh] for sh in shapes])
    assert s.size() == 4 and s.proof_stride() == 864 and s.input_stride() == 32 * 128
    assert s.shapes == [(nb, nc, 32 * (24 + 3 * nc)) for nb, nc in shapes]
    with pytest.raises(IndexError):
        s.key_shape(4)
    assert L.zkv_plonk_set_key_shape(s._h, 4, None, None, None) == _lib.ERR_INVALID_ARG
    assert L.zkv_plonk_set_key_shape(s._h, 1, None, None, None) == 0
    raw = _lib.lib()
    assert raw.zkv_ctx_vm(s._h) == 10
    assert raw.zkv_ctx_set_aggregate_check(s._h, 1, bytes(32)) == 0           # accepted; calls run the per-proof path
    out = (C.c_uint64 * 2)(7, 7)
    assert raw.zkv_ctx_aggregate_counters(s._h, out) == 0 and list(out) == [0, 0]
    assert raw.zkv_ctx_set_lanes_per_proof(s._h, 16) == 0
    s.close()
    small = z.PlonkVerifierSet([by[(0, 0)]] * 3)
    assert small.proof_stride() == 768 and small.input_stride() == 0
    small.close()


def test_sets_are_single_device_and_other_contexts_refuse_the_set_calls(L, by):
    from stylus_zkvm_verifiers_amd import _lib, plonk_keys
    raw = _lib.lib()
    h = _create(L, [by[(2, 1)], by[(9, 0)]])
    assert h
    assert not raw.zkv_ctx_create_sharded((C.c_void_p * 1)(h), 1)
    assert raw.zkv_ctx_vk_x_batch(h, 1, bytes(64), C.create_string_buffer(64)) == _lib.ERR_WRONG_CTX
    PK = plonk_keys.lib()
    assert PK.zkv_plonk_verify_batch(h, 0, None, None, None) == _lib.ERR_WRONG_CTX
    assert PK.zkv_plonk_verify_batch_dev(h, 0, None, None, None, None) == _lib.ERR_WRONG_CTX
    assert PK.zkv_plonk_key_shape(h, None, None, None) == _lib.ERR_WRONG_CTX
    assert raw.zkv_groth16_verify_batch(h, 0, None, None, None) == _lib.ERR_WRONG_CTX
    assert raw.zkv_sp1_plonk_verify_batch(h, 0, None, None, None, None, None, None, None) == _lib.ERR_WRONG_CTX
    vk = by[(2, 1)]
    p = PK.zkv_plonk_ctx_create(vk, len(vk), 0)
    g = raw.zkv_groth16_ctx_create(bytes(448 + 64), 1, 1, 0)
    for other in (p, g):
        assert L.zkv_plonk_set_verify_batch(other, 0, None, None, None, None) == _lib.ERR_WRONG_CTX
        assert L.zkv_plonk_set_verify_batch_dev(other, 0, None, None, None, None, None) == _lib.ERR_WRONG_CTX
        assert L.zkv_plonk_set_key_shape(other, 0, None, None, None) == _lib.ERR_WRONG_CTX
        assert L.zkv_plonk_set_size(other) == 0 and L.zkv_plonk_set_proof_stride(other) == 0 and L.zkv_plonk_set_input_stride(other) == 0
    # argument checks and empty batches need no device
    assert L.zkv_plonk_set_verify_batch(h, 0, None, None, None, None) == 0
    assert L.zkv_plonk_set_verify_batch_dev(h, 0, None, None, None, None, None) == 0
    assert L.zkv_plonk_set_verify_batch(h, 1, (C.c_uint32 * 1)(0), bytes(864), None, C.create_string_buffer(1)) == _lib.ERR_INVALID_ARG
    assert L.zkv_plonk_set_verify_batch(h, 1, None, bytes(864), bytes(288), C.create_string_buffer(1)) == _lib.ERR_INVALID_ARG
    raw.zkv_ctx_destroy(p)
    raw.zkv_ctx_destroy(g)
    raw.zkv_ctx_destroy(h)


# ---------------------------------------------------------------- slot layout (zkv_gset_layout.h pset_choose) against a numpy model
@pytest.fixture(scope='module')
def hsp():
    src = os.path.join(HERE, 'host_sim', 'host_sim_pset_layout.cpp')
    lib = os.path.join(HERE, 'host_sim', 'libhost_sim_pset_layout.so')
    hdr = os.path.join(ROOT, 'stylus_zkvm_verifiers_amd', 'csrc', 'zkv_gset_layout.h')
    if not os.path.exists(lib) or os.path.getmtime(lib) < max(os.path.getmtime(src), os.path.getmtime(hdr)):
        subprocess.check_call(['g++', '-O2', '-std=c++17', '-fPIC', '-shared', '-o', lib, src])
    h = C.CDLL(lib)
    h.hsp_choose.argtypes = [C.c_void_p, C.c_uint32, C.c_int, C.c_uint64, C.c_uint64, C.c_void_p, C.c_void_p]
    h.hsp_choose.restype = C.c_int
    return h


def _model(cnt, fixed, wave_below, wide_below):
    n = int(cnt.sum())
    start = np.concatenate([[0], np.cumsum((cnt.astype(np.uint64) + 63) // 64 * 64)]).astype(np.uint64)
    if fixed in (64, 128) or (not fixed and n <= wave_below):
        lanes = 64
    elif fixed == 16 or (not fixed and n <= wide_below):
        lanes = 16
    else:
        lanes = 2
    return lanes, start, int(start[-1])


@pytest.mark.parametrize('n_keys', [1, 3, 17, 256])
def test_slot_layout_matches_the_model(hsp, n_keys):
    rng = np.random.default_rng(n_keys)
    for trial in range(40):
        scale = int(rng.choice([1, 4, 70, 2000, 40000]))
        cnt = rng.integers(0, scale + 1, n_keys).astype(np.uint32)
        cnt[rng.random(n_keys) < 0.2] = 0                      # empty groups
        for fixed in (0, 2, 16, 64, 128):
            for wave_below, wide_below in ((2048, 12288), (0, 0), (1 << 40, 1 << 40)):
                start = np.zeros(n_keys + 1, np.uint64)
                slots = C.c_uint64(0)
                got = hsp.hsp_choose(cnt.ctypes.data, n_keys, fixed, wave_below, wide_below, start.ctypes.data, C.addressof(slots))
                want, wstart, wslots = _model(cnt, fixed, wave_below, wide_below)
                assert (got, slots.value) == (want, wslots) and (start == wstart).all()
                # every 64-slot block (a PREP wavefront; a fortiori every Miller wavefront of 32, 4 or 1 proofs) holds one key, and its
                # first slot is a proof of that key
                owner = np.full(wslots // 64, -1)
                for k in range(n_keys):
                    assert start[k] % 64 == 0 and start[k + 1] - start[k] >= cnt[k] and start[k + 1] - start[k] < cnt[k] + 64
                    b0, b1 = int(start[k]) // 64, int(start[k + 1]) // 64
                    assert (owner[b0:b1] == -1).all()
                    owner[b0:b1] = k
                    assert b1 - b0 == (int(cnt[k]) + 63) // 64        # (so the last block of the group starts below its cnt[k]-th proof)
                assert (owner >= 0).all()

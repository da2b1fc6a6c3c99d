"""Groth16 key sets (include/zkv_groth16_set.h) without a device: creation and argument checks, the getters, the
header against the library's exports, and the slot layout (csrc/zkv_gset_layout.h, host build) against a numpy model."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
NEW = ['zkv_groth16_set_create', 'zkv_groth16_set_size', 'zkv_groth16_set_signal_stride', 'zkv_groth16_set_key_n_ic',
       'zkv_groth16_set_verify_batch', 'zkv_groth16_set_verify_batch_dev', 'zkv_groth16_set_vk_x_batch']


def _vk(n_ic):
    return bytes(448 + 64 * n_ic)


@pytest.fixture(scope='module')
def L():
    from stylus_zkvm_verifiers_amd import groth16_set
    return groth16_set.lib()


def _create(L, vks, n_ic, vms):
    k = len(vks)
    words = (C.c_char_p * max(k, 1))(*vks)
    return L.zkv_groth16_set_create(k, words, (C.c_size_t * max(k, 1))(*n_ic), (C.c_int * max(k, 1))(*vms), 0)


def test_create_without_a_device_and_getters(L):
    import stylus_zkvm_verifiers_amd as zkv
    n_ic = [1, 2, 6, 7, 129]
    s = zkv.Groth16VerifierSet([(_vk(n), n, zkv.errors.VM_SP1 if j % 2 else zkv.errors.VM_RISC0) for j, n in enumerate(n_ic)])
    assert s.size() == 5 and s.signal_stride() == 32 * 128
    assert [s.key_n_ic(k) for k in range(5)] == n_ic
    with pytest.raises(IndexError):
        s.key_n_ic(5)
    assert L.zkv_ctx_vm(s._h) == 7
    from stylus_zkvm_verifiers_amd import _lib
    assert _lib.lib().zkv_ctx_set_aggregate_check(s._h, 1, bytes(32)) == 0      # accepted, changes nothing
    assert _lib.lib().zkv_ctx_set_lanes_per_proof(s._h, 16) == 0
    s.close()
    ones = zkv.Groth16VerifierSet([(_vk(1), 1, zkv.errors.VM_SP1)] * 3)
    assert ones.size() == 3 and ones.signal_stride() == 0
    ones.close()


def test_bad_arguments_give_null(L):
    import stylus_zkvm_verifiers_amd as zkv
    assert not _create(L, [], [], [])
    assert not _create(L, [_vk(1)] * 1025, [1] * 1025, [1] * 1025)
    assert _create(L, [_vk(1)] * 1024, [1] * 1024, [1] * 1024)          # (leaked on purpose: a 1,024-key set without a device is a few KB)
    for n in (0, 130):
        assert not _create(L, [_vk(2), _vk(max(n, 1))], [2, n], [1, 1])
    assert not _create(L, [_vk(2)], [2], [2])
    assert not _create(L, [_vk(2)], [2], [-1])
    assert not L.zkv_groth16_set_create(1, None, (C.c_size_t * 1)(2), (C.c_int * 1)(1), 0)
    assert not L.zkv_groth16_set_create(1, (C.c_char_p * 1)(_vk(2)), None, (C.c_int * 1)(1), 0)
    assert not L.zkv_groth16_set_create(1, (C.c_char_p * 1)(_vk(2)), (C.c_size_t * 1)(2), None, 0)
    assert not L.zkv_groth16_set_create(2, (C.c_char_p * 2)(_vk(2), None), (C.c_size_t * 2)(2, 2), (C.c_int * 2)(1, 1), 0)
    with pytest.raises(ValueError):
        zkv.Groth16VerifierSet([])
    with pytest.raises(ValueError):
        zkv.Groth16VerifierSet([(_vk(1), 1, 1)] * 1025)
    for n in (0, 130):
        with pytest.raises(ValueError):
            zkv.Groth16VerifierSet([(_vk(max(n, 1)), n, 1)])
    with pytest.raises(ValueError):
        zkv.Groth16VerifierSet([(_vk(2), 2, 5)])
    with pytest.raises(ValueError):
        zkv.Groth16VerifierSet([(_vk(2), 3, 1)])


def test_sets_are_single_device_and_other_contexts_refuse_the_set_calls(L):
    from stylus_zkvm_verifiers_amd import _lib
    raw = _lib.lib()
    h = _create(L, [_vk(3), _vk(2)], [3, 2], [0, 1])
    assert h
    arr = (C.c_void_p * 2)(h, h)
    assert not raw.zkv_ctx_create_sharded(arr, 1)
    assert raw.zkv_ctx_vk_x_batch(h, 1, bytes(64), C.create_string_buffer(64)) == _lib.ERR_WRONG_CTX
    assert raw.zkv_groth16_verify_batch(h, 1, bytes(256), bytes(64), C.create_string_buffer(1)) == _lib.ERR_WRONG_CTX
    g = raw.zkv_groth16_ctx_create(_vk(3), 3, 1, 0)
    assert L.zkv_groth16_set_verify_batch(g, 1, (C.c_uint32 * 1)(0), bytes(256), bytes(64), C.create_string_buffer(1)) == _lib.ERR_WRONG_CTX
    assert L.zkv_groth16_set_size(g) == 0 and L.zkv_groth16_set_signal_stride(g) == 0
    assert L.zkv_groth16_set_key_n_ic(g, 0) == _lib.ERR_WRONG_CTX
    assert L.zkv_groth16_set_key_n_ic(h, 2) == _lib.ERR_INVALID_ARG
    # keys past the set are an argument error for vk_x (no device needed to refuse them)
    assert L.zkv_groth16_set_vk_x_batch(h, 1, (C.c_uint32 * 1)(2), bytes(64), C.create_string_buffer(64)) == _lib.ERR_INVALID_ARG
    # empty batches need no device
    assert L.zkv_groth16_set_verify_batch(h, 0, None, None, None, None) == 0
    raw.zkv_ctx_destroy(g)
    raw.zkv_ctx_destroy(h)


def test_header_declares_exactly_the_new_symbols_and_the_library_exports_them(L):
    hdr = re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'zkv_groth16_set.h')).read(), flags=re.S)
    assert set(re.findall(r'\b(zkv_[a-z0-9_]+)\s*\(', hdr)) == set(NEW)
    assert '#include "zkv.h"' in hdr and '#define ZKV_VM_GROTH16_SET 7' in hdr and '#define ZKV_GROTH16_SET_MAX_KEYS 1024' in hdr
    from stylus_zkvm_verifiers_amd import _lib, groth16_set
    assert set(groth16_set.SYMBOLS) == set(NEW) and not set(NEW) & set(_lib.SYMBOLS)
    for name in NEW:
        assert hasattr(L, name), name
    main = re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'zkv.h')).read(), flags=re.S)
    assert not set(re.findall(r'\b(zkv_[a-z0-9_]+)\s*\(', main)) & set(NEW)


# ---------------------------------------------------------------- slot layout (zkv_gset_layout.h) against a numpy model
@pytest.fixture(scope='module')
def hsg():
    src = os.path.join(HERE, 'host_sim', 'host_sim_gset_layout.cpp')
    lib = os.path.join(HERE, 'host_sim', 'libhost_sim_gset_layout.so')
    hdr = os.path.join(ROOT, 'stylus_zkvm_verifiers_amd', 'csrc', 'zkv_gset_layout.h')
    if not os.path.exists(lib) or os.path.getmtime(lib) < max(os.path.getmtime(src), os.path.getmtime(hdr)):
        subprocess.check_call(['g++', '-O2', '-std=c++17', '-fPIC', '-shared', '-o', lib, src])
    h = C.CDLL(lib)
    h.hsg_choose.argtypes = [C.c_void_p, C.c_uint32, C.c_int, C.c_int, C.c_void_p, C.c_void_p]
    h.hsg_choose.restype = C.c_int
    return h


ALIGN = {2: 32, 16: 4, 64: 1, 128: 1}


def _model(cnt, lanes, fixed):
    n = int(cnt.sum())
    while True:
        a = ALIGN[lanes]
        padded = (cnt + a - 1) // a * a
        start = np.concatenate([[0], np.cumsum(padded)]).astype(np.uint64)
        slots = int(start[-1])
        if fixed or 4 * slots <= 5 * n or a == 1:
            return lanes, start, slots
        lanes = 16 if lanes == 2 else 64


@pytest.mark.parametrize('n_keys', [1, 3, 1024])
def test_slot_layout_matches_the_model(hsg, n_keys):
    rng = np.random.default_rng(n_keys)
    for trial in range(40):
        scale = int(rng.choice([1, 4, 40, 2000]))
        cnt = rng.integers(0, scale + 1, n_keys).astype(np.uint32)
        cnt[rng.random(n_keys) < 0.2] = 0                      # empty groups
        n = int(cnt.sum())
        for lanes in (2, 16, 64, 128):
            for fixed in (0, 1):
                start = np.zeros(n_keys + 1, np.uint64)
                slots = C.c_uint64(0)
                got = hsg.hsg_choose(cnt.ctypes.data, n_keys, lanes, fixed, start.ctypes.data, C.addressof(slots))
                want, wstart, wslots = _model(cnt, lanes, fixed)
                assert (got, slots.value) == (want, wslots) and (start == wstart).all()
                a = ALIGN[got]
                assert (start[:-1] % a == 0).all() and (start[1:] - start[:-1] >= cnt).all()
                if fixed:
                    assert got == lanes
                else:
                    assert slots.value <= 1.25 * n or a == 1            # the padding bound of an automatic choice
                    if a == 1:
                        assert slots.value == n

"""Aggregate check on PLONK key sets (include/zkv_plonk_set_agg.h) without a device: the header against the Python
module and the library's exports, zkv_plonk_set_srs_classes, the class layout (csrc/zkv_gset_layout.h pset_agg_choose, host build) against
a numpy model, and the Python surface.  PARITY UNPINNED BY CONSTRUCTION: the reference holds no PLONK code."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import plonk_shared_srs as S
import plonk_trapdoor_keys as T

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
NEW = ['zkv_plonk_set_srs_classes']


@pytest.fixture(scope='module')
def L():
    from stylus_zkvm_verifiers_amd import plonk_set_agg
    return plonk_set_agg.lib()


def _names(path):
    body = re.sub(r'/\*.*?\*/', '', open(path).read(), flags=re.S)
    return set(re.findall(r'\b(zkv_[a-z0-9_]+)\s*\(', body))


def test_header_declares_exactly_the_new_symbol_and_the_library_exports_it(L):
    hdr = os.path.join(ROOT, 'include', 'zkv_plonk_set_agg.h')
    assert _names(hdr) == set(NEW)
    text = open(hdr).read()
    assert '#include "zkv_plonk_set.h"' in text and 'PARITY UNPINNED BY CONSTRUCTION' in text
    from stylus_zkvm_verifiers_amd import _lib, plonk_set, plonk_set_agg
    assert set(plonk_set_agg.SYMBOLS) == set(NEW)
    assert not set(NEW) & set(_lib.SYMBOLS) and not set(NEW) & set(plonk_set.SYMBOLS)
    for name in NEW:
        assert getattr(L, name) is not None, name
    for other in ('zkv.h', 'zkv_plonk_set.h'):
        assert not _names(os.path.join(ROOT, 'include', other)) & set(NEW), other


def _classes(L, h, k):
    out = (C.c_uint32 * k)(*([77] * k))
    n = C.c_size_t(99)
    assert L.zkv_plonk_set_srs_classes(h, out, C.byref(n)) == 0
    return list(out), n.value


def test_srs_classes_by_first_appearance(L):
    import stylus_zkvm_verifiers_amd as z
    from stylus_zkvm_verifiers_amd import _lib, plonk_keys
    a = [S.key_bytes('A', 0, 0), S.key_bytes('A', 2, 1), S.key_bytes('A', 9, 0, 1)]
    b = [S.key_bytes('B', 2, 1), S.key_bytes('B', 0, 0)]
    c = [S.key_bytes('C', 3, 0)]
    assert a[0][-256:] == a[1][-256:] == a[2][-256:] and a[0][-256:] != b[0][-256:] and a[0][-256:-128] == b[0][-256:-128]
    one = z.PlonkVerifierSet(a)
    assert one.srs_classes() == ([0, 0, 0], 1)
    assert _classes(L, one._h, 3) == ([0, 0, 0], 1)
    # either pointer may be NULL
    n = C.c_size_t(0)
    assert L.zkv_plonk_set_srs_classes(one._h, None, C.byref(n)) == 0 and n.value == 1
    assert L.zkv_plonk_set_srs_classes(one._h, (C.c_uint32 * 3)(), None) == 0
    assert L.zkv_plonk_set_srs_classes(one._h, None, None) == 0
    one.close()
    distinct = z.PlonkVerifierSet([a[0], b[0], c[0]])
    assert distinct.srs_classes() == ([0, 1, 2], 3)
    distinct.close()
    inter = z.PlonkVerifierSet([a[0], b[0], a[1], c[0], b[1]])                 # A B A C B
    assert inter.srs_classes() == ([0, 1, 0, 2, 1], 3) and inter.size() == 5
    inter.close()
    # one damaged byte of [tau]_2 is a class of its own (the set-up validation then finds it off the curve)
    off = T.apply_case('key_tau2_off_curve', a[1], b'', [])[0]
    s = z.PlonkVerifierSet([a[0], off, a[2]])
    assert s.srs_classes() == ([0, 1, 0], 2)
    # the existing contract of a fresh set: the check is accepted, nothing counted before a batch
    s.set_aggregate_check(True, bytes(32), 64)
    assert s.aggregate_counters() == (0, 0)
    s.close()
    full = z.PlonkVerifierSet([a[0]] * 255 + [b[0]])
    cls, ncls = full.srs_classes()
    assert cls == [0] * 255 + [1] and ncls == 2
    full.close()
    # wrong context
    vk = a[0]
    p = plonk_keys.lib().zkv_plonk_ctx_create(vk, len(vk), 0)
    g = _lib.lib().zkv_groth16_ctx_create(bytes(448 + 64), 1, 1, 0)
    for other in (p, g, None):
        assert L.zkv_plonk_set_srs_classes(other, None, None) == _lib.ERR_WRONG_CTX
    _lib.lib().zkv_ctx_destroy(p)
    _lib.lib().zkv_ctx_destroy(g)


def test_python_surface_without_a_device():
    import stylus_zkvm_verifiers_amd as z
    s = z.PlonkVerifierSet([S.key_bytes('A', 0, 0)])
    assert callable(s.set_aggregate_check) and callable(s.aggregate_counters) and callable(s.srs_classes)
    s.set_aggregate_check(True, bytes(32), 64)
    s.set_aggregate_check(True, None, None)
    for bad in (48, 0, 8, 512, 1):
        with pytest.raises(ValueError):
            s.set_aggregate_check(True, bytes(32), bad)
    with pytest.raises(ValueError):
        s.set_aggregate_check(True, bytes(31), 64)
    s.set_aggregate_check(False)
    assert s.aggregate_counters() == (0, 0)                                    # no device set up yet: nothing counted
    s.close()


# ---------------------------------------------------------------- the class layout against the model
@pytest.fixture(scope='module')
def hpa():
    src = os.path.join(HERE, 'host_sim', 'host_sim_pset_agg_layout.cpp')
    lib = os.path.join(HERE, 'host_sim', 'libhost_sim_pset_agg_layout.so')
    hdr = os.path.join(ROOT, 'stylus_zkvm_verifiers_amd', 'csrc', 'zkv_gset_layout.h')
    if not os.path.exists(lib) or os.path.getmtime(lib) < max(os.path.getmtime(src), os.path.getmtime(hdr)):
        subprocess.check_call(['g++', '-O2', '-std=c++17', '-fPIC', '-shared', '-o', lib, src])
    h = C.CDLL(lib)
    h.hpa_choose.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32, C.c_uint32, C.c_int, C.c_uint64, C.c_uint64] + [C.c_void_p] * 5
    h.hpa_choose.restype = C.c_int
    h.hpa_classes.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p]
    h.hpa_classes.restype = C.c_uint32
    h.hpa_chunk_slots.argtypes = [C.c_uint64, C.c_uint32]
    h.hpa_chunk_slots.restype = C.c_uint64
    return h


@pytest.mark.parametrize('seed', range(24))
def test_class_layout_matches_the_model(hpa, seed):
    rng = np.random.default_rng(seed)
    K = int(rng.choice([1, 2, 5, 16, 97, 256]))
    n_cls = int(rng.integers(1, min(K, 9) + 1))
    sub = int(rng.choice([16, 32, 64, 128, 256]))
    A = max(64, sub)
    cls = rng.integers(0, n_cls, K).astype(np.uint32)
    cls[:n_cls] = rng.permutation(n_cls)                                      # every class has a key
    cnt = rng.integers(0, int(rng.choice([8, 20, 300, 3000])), K).astype(np.uint32)
    cnt[rng.random(K) < 0.15] = 0
    capable = (rng.random(n_cls) < 0.7).astype(np.uint8)
    wave_below, wide_below = int(rng.choice([0, 2048])), int(rng.choice([0, 12288, 1 << 40]))
    start = np.zeros(K + 1, np.uint64); cbeg = np.zeros(n_cls, np.uint64); cend = np.zeros(n_cls, np.uint64)
    R, slots = C.c_uint64(0), C.c_uint64(0)
    lanes = hpa.hpa_choose(cnt.ctypes.data, cls.ctypes.data, K, capable.ctypes.data, n_cls, sub, 0, wave_below, wide_below, start.ctypes.data,
                           cbeg.ctypes.data, cend.ctypes.data, C.byref(R), C.byref(slots))
    want = S.layout(cnt, cls, capable, sub)
    assert [int(x) for x in start[:K]] == want['start'] and int(start[K]) == want['slots'] == slots.value and R.value == want['R']
    assert [int(x) for x in cbeg] == want['cbeg'] and [int(x) for x in cend] == want['cend']
    rest = int(sum(int(cnt[k]) for k in range(K) if not capable[cls[k]]))
    assert lanes == (64 if rest <= wave_below else 16 if rest <= wide_below else 2)
    # the properties the device path relies on, from the numbers the C function returned
    owner = np.full(slots.value, -1, np.int64)                                # the key of every slot that holds a proof
    for k in range(K):
        c = int(cls[k])
        assert start[k] % 64 == 0                                             # key groups on 64-slot boundaries ...
        assert cbeg[c] <= start[k] and int(start[k]) + (int(cnt[k]) + 63) // 64 * 64 <= cend[c]        # ... inside their class region
        sl = np.arange(int(start[k]), int(start[k]) + int(cnt[k]))
        assert (owner[sl] == -1).all()                                        # every proof placed exactly once
        owner[sl] = k
    assert int((owner >= 0).sum()) == int(cnt.sum())
    for c in range(n_cls):
        assert cbeg[c] % A == 0 and cend[c] % A == 0                           # class regions on multiples of A
        assert (cend[c] <= R.value) == bool(capable[c]) or cbeg[c] == cend[c]  # capable classes fill [0, R), the others [R, slots)
    regions = sorted((int(cbeg[c]), int(cend[c])) for c in range(n_cls) if cend[c] > cbeg[c])
    assert all(a[1] == b[0] for a, b in zip(regions, regions[1:])) and (not regions or (regions[0][0] == 0 and regions[-1][1] == slots.value))
    for b in range(0, slots.value, 64):                                       # a PREP wavefront holds one key, its first slot a proof (or none at all)
        ks = set(owner[b:b + 64][owner[b:b + 64] >= 0])
        assert len(ks) <= 1 and (not ks or owner[b] >= 0)
    for b in range(0, R.value, sub):                                          # no sub-batch spans two classes
        ks = owner[b:b + sub][owner[b:b + sub] >= 0]
        assert len(set(int(cls[k]) for k in ks)) <= 1
        assert all(cbeg[cls[k]] <= b and b + sub <= cend[cls[k]] for k in ks)
    # chunk ends on multiples of A whatever the workspace capacity (a multiple of 64)
    for cap in (64, 192, 4096, 4096 + 64, 12345 * 64, 1 << 20):
        capa = hpa.hpa_chunk_slots(cap, sub)
        assert capa == cap // A * A and capa % A == 0 and capa <= cap
        if capa:
            assert all(e % A == 0 for e in list(range(capa, R.value, capa)) + [R.value])


def test_host_class_formation_matches_byte_equality(hpa):
    rng = np.random.default_rng(5)
    for K in (1, 2, 7, 256):
        pool = rng.integers(0, 256, (4, 256)).astype(np.uint8)
        pick = rng.integers(0, 4, K)
        g2 = np.ascontiguousarray(pool[pick])
        if K > 2:
            g2[K - 1] = g2[0]; g2[K - 1, 255] ^= 1; pick[K - 1] = 9               # one byte off: another class
        out = np.zeros(K, np.uint32); rep = np.zeros(K, np.uint32)
        n = hpa.hpa_classes(g2.ctypes.data, K, out.ctypes.data, rep.ctypes.data)
        seen = []
        for k in range(K):
            if pick[k] not in seen:
                seen.append(pick[k])
            assert out[k] == seen.index(pick[k])
        assert n == len(seen) and [int(pick[r]) for r in rep[:n]] == [int(x) for x in seen]

"""Aggregate check on Groth16 key sets without a device: the two-region slot layout (csrc/zkv_gset_layout.h gset_agg_choose, host build)
against a model, the per-signal share loop of the scalar-sum form (csrc/zkv_gset_agg.h, host build) against the spec model's
sum_i r_i vk_x_i, and the Python surface."""
import ctypes as C
import os
import random
import subprocess

import numpy as np
import pytest

import spec_model as m

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CSRC = os.path.join(ROOT, 'stylus_zkvm_verifiers_amd', 'csrc')
ALIGN = {2: 32, 16: 4, 64: 1, 128: 1}
P32 = C.POINTER(C.c_uint32)


@pytest.fixture(scope='module')
def hga():
    src = os.path.join(HERE, 'host_sim', 'host_sim_gset_agg.cpp')
    lib = os.path.join(HERE, 'host_sim', 'libhost_sim_gset_agg.so')
    deps = [src] + [os.path.join(CSRC, h) for h in ('zkv_gset_layout.h', 'zkv_gset_agg.h', 'zkv_agg.h', 'zkv_verify.h')]
    if not os.path.exists(lib) or os.path.getmtime(lib) < max(os.path.getmtime(p) for p in deps):
        subprocess.check_call(['g++', '-O2', '-std=c++17', '-fPIC', '-shared', '-o', lib, src])
    h = C.CDLL(lib)
    h.hga_choose.argtypes = [C.c_void_p] * 2 + [C.c_uint32, C.c_uint32, C.c_int] + [C.c_void_p] * 6
    h.hga_choose.restype = C.c_int
    h.hga_slot.argtypes = [C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p]
    h.hga_slot.restype = C.c_uint64
    h.hga_u.argtypes = [C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    h.hga_u.restype = C.c_int
    h.hga_chunk_plan.argtypes = [C.c_void_p] * 3 + [C.c_uint32, C.c_uint64, C.c_uint64, C.c_uint32, C.c_int, C.c_uint64] + [C.c_void_p] * 5
    h.hga_chunk_plan.restype = C.c_int
    return h


def _choose_model(cnt, lanes):
    """gset_choose (zkv_gset_layout.h): pad to the mapping's proofs per wavefront, step finer above 1.25x."""
    n = sum(cnt)
    while True:
        a = ALIGN[lanes]
        start = np.concatenate([[0], np.cumsum([(c + a - 1) // a * a for c in cnt])]).astype(np.uint64)
        if 4 * int(start[-1]) <= 5 * n or a == 1:
            return lanes, start
        lanes = 16 if lanes == 2 else 64


@pytest.mark.parametrize('seed', range(12))
def test_layout_regions(hga, seed):
    rng = np.random.default_rng(seed)
    K = int(rng.choice([1, 2, 5, 16, 300, 1024]))
    sub = int(rng.choice([16, 32, 64, 128, 256]))
    cnt = rng.integers(0, int(rng.choice([8, 300, 3000])), K).astype(np.uint32)
    capable = (rng.random(K) < 0.8).astype(np.uint8)
    lanes_in = int(rng.choice([2, 16, 64, 128]))
    agg = np.zeros(K, np.uint32); rest = np.zeros(K, np.uint32)
    astart = np.zeros(K + 1, np.uint64); pstart = np.zeros(K + 1, np.uint64)
    R, slots = C.c_uint64(0), C.c_uint64(0)
    lanes = hga.hga_choose(cnt.ctypes.data, capable.ctypes.data, K, sub, lanes_in, agg.ctypes.data, astart.ctypes.data, rest.ctypes.data,
                           pstart.ctypes.data, C.byref(R), C.byref(slots))
    A = max(64, sub)
    assert (agg == np.where(capable == 1, cnt // A * A, 0)).all() and (agg % A == 0).all()
    assert (rest == cnt - agg).all()
    assert (astart == np.concatenate([[0], np.cumsum(agg)])).all() and R.value == int(agg.sum())
    want_lanes, want_start = _choose_model([int(x) for x in rest], lanes_in)
    assert lanes == want_lanes and (pstart == want_start + R.value).all() and slots.value == int(want_start[-1]) + R.value
    # every proof exactly one slot, ranks stable, each aggregate group key-uniform and a whole number of A
    owner = np.full(slots.value, -1, np.int64)
    for k in range(K):
        sl = [hga.hga_slot(k, r, agg.ctypes.data, astart.ctypes.data, pstart.ctypes.data) for r in range(int(cnt[k]))]
        assert sl == sorted(sl) and len(set(sl)) == len(sl)
        assert all(s < R.value for s in sl[:agg[k]]) and all(s >= R.value for s in sl[agg[k]:])
        assert not (owner[sl] >= 0).any()
        owner[sl] = k
    assert (owner[:R.value] >= 0).all()                                          # no pad slot in the aggregate region
    for b in range(0, R.value, A):
        assert len(set(owner[b:b + A])) == 1


def _regions(rng, shape, A):
    """Regions of an aggregate region [0, R): a Groth16 set's keys back to back (rep = None: the key itself), or a PLONK set's SRS classes on
    multiples of A with a class without proofs among them and a class that cannot take the check passed as an empty region behind R."""
    if shape == 'keys':
        n = int(rng.choice([1, 2, 5, 16, 300]))
        size = A * rng.integers(0, int(rng.choice([2, 4, 40])), n)
        size[rng.integers(0, n)] += A                                            # (R > 0)
        beg = np.concatenate([[0], np.cumsum(size)])[:-1]
        return beg.astype(np.uint64), (beg + size).astype(np.uint64), None, int(size.sum())
    n = int(rng.choice([3, 8, 40]))
    size = A * rng.integers(1, int(rng.choice([2, 4, 40])), n)
    size[rng.integers(0, n - 1)] = 0                                             # a class without proofs
    size[n - 1] = 0                                                              # the class that cannot take the check
    beg = np.concatenate([[0], np.cumsum(size)])[:-1]
    rep = np.sort(rng.choice(np.arange(1, 1024), n, replace=False)).astype(np.uint32)
    return beg.astype(np.uint64), (beg + size).astype(np.uint64), rep, int(size.sum())


def test_aggregate_chunk_plan(hga):
    """gset_agg_chunk_plan (zkv_gset_layout.h): where the pseudo-proof of every sub-batch of an aggregate chunk lives and which key's line
    tables its slot takes, for both kinds of set, against a model."""
    NONE = 0xFFFFFFFF
    stepped = fell_back = chunks = 0
    for seed in range(60):
        rng = np.random.default_rng(7000 + seed)
        sub = int(rng.choice([16, 32, 64, 128, 256]))
        A = max(64, sub)
        beg, end, rep, R = _regions(rng, 'keys' if seed % 2 == 0 else 'classes', A)
        n_reg = len(beg)
        rep_of = np.arange(n_reg) if rep is None else rep
        capa = A * int(rng.integers(1, 12))
        for base in range(0, R, capa):
            m = min(capa, R - base)
            n2 = m // sub
            lanes_in = int(rng.choice([2, 16, 64, 128]))
            cap = int(rng.choice([n2, n2 + n2 // 8, 1 << 20]))                    # the pseudo-workspace holds the n2 pseudo-proofs at least
            nsb = np.full(n_reg, NONE, np.uint32); pst = np.zeros(n_reg + 1, np.uint64)
            psl = np.full(n2, NONE, np.uint32); skey2 = np.full(n2 + 31 * n_reg, NONE, np.uint32)
            slots = C.c_uint64(0)
            lanes = hga.hga_chunk_plan(beg.ctypes.data, end.ctypes.data, None if rep is None else rep.ctypes.data, n_reg, base, m, sub, lanes_in,
                                       cap, nsb.ctypes.data, pst.ctypes.data, psl.ctypes.data, skey2.ctypes.data, C.byref(slots))
            lo = np.maximum(beg.astype(np.int64), base); hi = np.minimum(end.astype(np.int64), base + m)
            want_nsb = np.where(hi > lo, (hi - lo) // sub, 0)
            assert (nsb == want_nsb).all() and int(want_nsb.sum()) == n2         # (the regions tile the chunk)
            want_lanes, want_pst = _choose_model([int(x) for x in want_nsb], lanes_in)
            if int(want_pst[-1]) > cap:                                          # no room for the padding: one wavefront per pseudo-proof
                fell_back += 1
                want_lanes, want_pst = 64, np.concatenate([[0], np.cumsum(want_nsb)]).astype(np.uint64)
            elif want_lanes != lanes_in:
                stepped += 1
            a = ALIGN[want_lanes]
            assert lanes == want_lanes and (pst == want_pst).all()
            assert slots.value == sum((int(x) + a - 1) // a * a for x in want_nsb) == int(want_pst[-1])
            assert len(set(psl.tolist())) == n2                                  # injective
            for q in range(n_reg):
                t0 = (int(lo[q]) - base) // sub
                assert (psl[t0:t0 + int(want_nsb[q])] == int(pst[q]) + np.arange(int(want_nsb[q]))).all()       # in order, inside [pst[q], pst[q + 1])
                assert int(pst[q]) + int(want_nsb[q]) <= int(pst[q + 1])
                assert (skey2[int(pst[q]):int(pst[q + 1])] == rep_of[q]).all()
            assert (skey2[slots.value:] == NONE).all()                           # nothing written past the slots
            chunks += 1
    assert chunks > 100 and stepped > 0 and fell_back > 0                         # the generator reaches the 1.25x step-down and the capacity fall-back


def _limbs(v):
    return [(v >> (32 * k)) & 0xFFFFFFFF for k in range(8)]


@pytest.mark.parametrize('n_sig', [0, 1, 2, 5, 17, 128])
@pytest.mark.parametrize('sub', [16, 32, 64])
def test_scalar_sum_shares_equal_the_spec_model(hga, n_sig, sub):
    rng = random.Random(1000 * n_sig + sub)
    c = [rng.randrange(1, m.R) for _ in range(n_sig + 1)]
    ic = [m.g1_mul(m.G1_GEN, x) for x in c]
    r = [rng.randrange(1 << 128) % m.R for _ in range(sub)]
    s = [[rng.choice([0, 1, m.R - 1, rng.randrange(m.R)]) for _ in range(n_sig)] for _ in range(sub)]
    ic_l = np.array([w for (x, y) in ic for w in _limbs(x) + _limbs(y)], np.uint32)
    r_l = np.array([w for v in r for w in _limbs(v)], np.uint32)
    s_l = np.array([w for row in s for v in row for w in _limbs(v)] or [0], np.uint32)
    out = (C.c_uint8 * 64)()
    inf = hga.hga_u(n_sig, sub, ic_l.ctypes.data, r_l.ctypes.data, s_l.ctypes.data, out)
    total = sum(ri * (c[0] + sum(sib * cb for sib, cb in zip(row, c[1:]))) for ri, row in zip(r, s)) % m.R
    want = m.g1_mul(m.G1_GEN, total)
    got = (int.from_bytes(bytes(out[:32]), 'big'), int.from_bytes(bytes(out[32:]), 'big'))
    assert inf == 0 and got == tuple(want)


def test_python_surface_without_a_device():
    import stylus_zkvm_verifiers_amd as zkv
    s = zkv.Groth16VerifierSet([(bytes(448 + 64 * 3), 3, zkv.errors.VM_SP1)])
    assert callable(s.set_aggregate_check) and callable(s.aggregate_counters)
    s.set_aggregate_check(True, bytes(32), 64)
    s.set_aggregate_check(True, None, None)
    with pytest.raises(ValueError):
        s.set_aggregate_check(True, bytes(32), 48)
    s.set_aggregate_check(False)
    assert s.aggregate_counters() == (0, 0)                                    # no device set up yet: nothing counted
    s.close()

"""PLONK core for any key (include/zkv_plonk_keys.h) on the MI355X: every fixture verdict at every kernel mapping, device-resident
batches against host batches, batches across the host staging chunk, the aggregate check, two shards on one device.  PARITY UNPINNED
BY CONSTRUCTION (no PLONK in the reference): expectations are oracle/plonk_model.py's verdicts (tests/golden/plonk_keys_cases.json)."""
import ctypes as C
import json
import os

import numpy as np
import pytest

import plonk_trapdoor_keys as T

HERE = os.path.dirname(os.path.abspath(__file__))
H = bytes.fromhex
pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def fx():
    return json.load(open(os.path.join(HERE, 'golden', 'plonk_keys_cases.json')))


@pytest.fixture(scope='module')
def pk():
    import stylus_zkvm_verifiers_amd as z
    from stylus_zkvm_verifiers_amd import plonk_keys
    assert z.device_count() >= 1, 'no gfx950 device visible'
    return plonk_keys


def _pool(fx, nb, nc):
    e = next(e for e in fx['pool'] if (e['nb_public'], e['n_c']) == (nb, nc))
    vk, proofs, pub = T.pool_arrays(e)
    return vk, (proofs, pub)


def _batch(fx, nb, nc, n, bad_every, seed):
    """n proofs tiled from the pool; every bad_every-th one damaged (the claimed l(zeta) changed, or a public input + 1): the expected
    verdicts are known."""
    vk, (P, Q) = _pool(fx, nb, nc)
    idx = np.random.default_rng(seed).integers(0, len(P), n)
    proofs, pub = P[idx].copy(), Q[idx].copy()
    want = np.ones(n, np.uint8)
    bad = np.arange(bad_every - 1, n, bad_every) if bad_every else np.arange(0)
    want[bad] = 0
    for j, i in enumerate(bad):
        if nb and j % 2:
            pub[i, j % nb, 31] ^= 1
        else:
            proofs[i, 12 * 32 + 31] ^= 1
    return vk, proofs, pub, want


def _dev(pk, v, proofs, pub):
    import torch
    dp = torch.from_numpy(np.ascontiguousarray(proofs)).cuda()
    di = torch.from_numpy(np.ascontiguousarray(pub)).cuda() if pub.size else None
    out = torch.zeros(len(proofs), dtype=torch.uint8, device='cuda')
    v.verify_batch_dev(len(proofs), dp.data_ptr(), di.data_ptr() if di is not None else 0, out.data_ptr())
    v.synchronize()
    return out.cpu().numpy()


def test_every_fixture_case_at_every_mapping(fx, pk):
    n = 0
    for sh in fx['shapes']:
        groups = {}
        for name, vk, proof, pub, model, _ in T.fixture_cases(sh):
            groups.setdefault(vk, []).append((dict(name=name, model=model), proof, pub))
        for vk, cs in groups.items():
            v = pk.PlonkVerifier(vk)
            for lanes in (0, 2, 16, 64, 128):
                v.set_lanes_per_proof(lanes)
                got = v.verify_batch([p for _, p, _ in cs], [q for _, _, q in cs])
                for (c, _, _), g in zip(cs, got):
                    assert int(g) == c['model'], (sh['nb_public'], sh['n_c'], c['name'], lanes)
            v.set_lanes_per_proof(0)
            c, p, q = cs[0]
            assert v.verify_proof(p, q) == bool(c['model'])
            v.close()
            n += len(cs)
    assert n > 1000


@pytest.mark.parametrize('nb', [0, 2, 9, 128])
@pytest.mark.parametrize('nc', [0, 1])
def test_device_batch_equals_host_batch(fx, pk, nb, nc):
    vk, proofs, pub, want = _batch(fx, nb, nc, 4099, 7, 100 + nb + nc)
    v = pk.PlonkVerifier(vk)
    host = v.verify_batch(proofs, pub)
    dev = _dev(pk, v, proofs, pub)
    assert np.array_equal(host, want) and np.array_equal(dev, host)
    ms = v.last_stage_ms()
    assert len(ms) == 5 and all(x >= 0 for x in ms)
    v.close()


def test_large_batches_within_and_across_the_staging_chunk(fx, pk):
    # 2^16 device-resident proofs at 128 inputs (one chunk), then 2^17 + 5 host proofs (the staging chunk is 2^17 at 128 inputs)
    vk, proofs, pub, want = _batch(fx, 128, 1, 1 << 16, 64, 7)
    v = pk.PlonkVerifier(vk)
    assert np.array_equal(_dev(pk, v, proofs, pub), want)
    vk, proofs, pub, want = _batch(fx, 128, 1, (1 << 17) + 5, 64, 8)
    got = v.verify_batch(proofs, pub)
    assert np.array_equal(got, want)
    v.close()


def test_aggregate_check_gives_the_per_proof_verdicts(fx, pk, monkeypatch):
    monkeypatch.setenv('ZKV_AGG_MIN', '4096')          # 2^16-proof chunks take the check (default: from 2^17 on)
    vk, proofs, pub, want = _batch(fx, 9, 1, 1 << 16, 0, 11)
    _, proofs_b, pub_b, want_b = _batch(fx, 9, 1, 1 << 16, 64, 12)
    v = pk.PlonkVerifier(vk)
    off = [v.verify_batch(proofs, pub), v.verify_batch(proofs_b, pub_b)]
    assert np.array_equal(off[0], want) and np.array_equal(off[1], want_b)
    v.set_aggregate_check(True, seed=bytes(range(32)), sub_batch=32)
    c0 = v.aggregate_counters()
    on = [v.verify_batch(proofs, pub), _dev(pk, v, proofs_b, pub_b)]
    c1 = v.aggregate_counters()
    assert np.array_equal(on[0], off[0]) and np.array_equal(on[1], off[1])
    assert c1[0] > c0[0] and c1[1] > c0[1]
    v.set_aggregate_check(False)
    v.close()


def test_two_shards_on_one_device_equal_one_context(fx, pk):
    L = pk.lib()
    vk, proofs, pub, want = _batch(fx, 9, 0, 5003, 13, 21)
    one = pk.PlonkVerifier(vk)
    ref_h, ref_d = one.verify_batch(proofs, pub), _dev(pk, one, proofs, pub)
    kids = [L.zkv_plonk_ctx_create(vk, len(vk), 0) for _ in range(2)]
    s = L.zkv_ctx_create_sharded((C.c_void_p * 2)(*kids), 2)
    assert s and L.zkv_ctx_shard_count(s) == 2
    sh = pk.PlonkVerifier.__new__(pk.PlonkVerifier)
    sh._L, sh._h, sh.nb_public, sh.n_commitments, sh.proof_bytes = L, s, 9, 0, 768
    got_h, got_d = sh.verify_batch(proofs, pub), _dev(pk, sh, proofs, pub)
    assert np.array_equal(ref_h, want) and np.array_equal(ref_d, want)
    assert np.array_equal(got_h, want) and np.array_equal(got_d, want)
    sh.close()                                          # the sharded context owns its shards
    one.close()


def test_wrong_context_after_device_set_up(fx, pk):
    from stylus_zkvm_verifiers_amd import _lib
    vk, proofs, pub, want = _batch(fx, 2, 1, 64, 0, 3)
    v = pk.PlonkVerifier(vk)
    assert np.array_equal(v.verify_batch(proofs, pub), want)
    L = pk.lib()
    sp = L.zkv_sp1_ctx_create(0)
    assert L.zkv_plonk_verify_batch(sp, 1, proofs.ctypes.data, pub.ctypes.data, C.create_string_buffer(1)) == _lib.ERR_WRONG_CTX
    assert L.zkv_sp1_plonk_verify_batch(v._h, 0, None, None, None, None, None, None, None) == _lib.ERR_WRONG_CTX
    assert L.zkv_ctx_vk_x_batch(v._h, 1, b'x' * 64, C.create_string_buffer(64)) == _lib.ERR_WRONG_CTX
    L.zkv_ctx_destroy(sp)
    v.close()


def test_no_wait_faults_after_the_module(pk):
    from stylus_zkvm_verifiers_amd import _lib
    out = C.c_uint64(1)
    assert _lib.lib().zkv_diag_wait_faults(0, C.byref(out)) == 0 and out.value == 0

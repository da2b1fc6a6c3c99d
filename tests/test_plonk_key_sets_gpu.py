"""PLONK key sets (include/zkv_plonk_set.h) on the MI355X: every fixture case in one set of 117 keys at every
mapping, bytes past each key's row length ignored, proofs under another key, key indices past the set, a one-key set against PlonkVerifier,
and a large host batch across the staging chunk in a child process.  PARITY UNPINNED BY CONSTRUCTION (no PLONK in the reference):
expectations are oracle/plonk_model.py's verdicts (tests/golden/plonk_keys_cases.json, plonk_trapdoor_keys.model_verify)."""
import ctypes as C
import json
import os
import subprocess
import sys
import tempfile

import numpy as np
import pytest

import plonk_trapdoor_keys as T

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def fx():
    return json.load(open(os.path.join(HERE, 'golden', 'plonk_keys_cases.json')))


@pytest.fixture(scope='module')
def z():
    import stylus_zkvm_verifiers_amd as z
    assert z.device_count() >= 1, 'no gfx950 device visible'
    return z


@pytest.fixture(scope='module')
def cases(fx):
    """Every fixture case: the distinct keys (shape keys and tampered keys) and per case its key index, proof, inputs and model verdict."""
    keys, index, rows = [], {}, []
    for sh in fx['shapes']:
        for name, vk, proof, pub, model, _ in T.fixture_cases(sh):
            if vk not in index:
                index[vk] = len(keys)
                keys.append(vk)
            rows.append((index[vk], proof, pub, model))
    return keys, rows


def _rows(rows, perm, ps, ins, fill=0):
    n = len(perm)
    kk = np.array([rows[j][0] for j in perm], np.uint32)
    proofs = np.full((n, ps), fill, np.uint8)
    pub = np.full((n, ins // 32, 32), fill, np.uint8)
    for r, j in enumerate(perm):
        p, q = rows[j][1], rows[j][2]
        proofs[r, :len(p)] = np.frombuffer(p, np.uint8)
        if q:
            pub[r, :len(q)] = np.frombuffer(b''.join(q), np.uint8).reshape(len(q), 32)
    want = np.array([rows[j][3] for j in perm], np.uint8)
    return kk, proofs, pub, want


def _dev(s, kk, proofs, pub):
    import torch
    dk = torch.from_numpy(np.ascontiguousarray(kk).view(np.int32)).cuda()
    dp = torch.from_numpy(np.ascontiguousarray(proofs)).cuda()
    di = torch.from_numpy(np.ascontiguousarray(pub)).cuda() if pub.size else None
    out = torch.zeros(len(kk), dtype=torch.uint8, device='cuda')
    s.verify_batch_dev(len(kk), dk.data_ptr(), dp.data_ptr(), di.data_ptr() if di is not None else 0, out.data_ptr())
    s.synchronize()
    return out.cpu().numpy()


@pytest.fixture(scope='module')
def big_set(z, cases):
    keys, _ = cases
    s = z.PlonkVerifierSet(keys)
    yield s
    s.close()


def test_every_fixture_case_in_one_set_at_every_mapping(big_set, cases):
    keys, rows = cases
    s = big_set
    assert len(keys) == 117 and len(rows) == 1019
    assert s.size() == 117 and s.proof_stride() == 864 and s.input_stride() == 32 * 128
    perm = np.random.default_rng(1).permutation(len(rows))
    kk, proofs, pub, want = _rows(rows, perm, s.proof_stride(), s.input_stride())
    for lanes in (0, 2, 16, 64):
        s.set_lanes_per_proof(lanes)
        host = s.verify_batch(kk, proofs, pub)
        dev = _dev(s, kk, proofs, pub)
        bad = [(rows[perm[i]][0], i) for i in np.nonzero(host != want)[0]]
        assert np.array_equal(host, want), (lanes, bad[:8])
        assert np.array_equal(dev, host), lanes
    s.set_lanes_per_proof(0)
    ms = s.last_stage_ms()
    assert len(ms) == 5 and all(x >= 0 for x in ms)


def test_bytes_past_each_keys_row_length_are_never_read(big_set, cases):
    keys, rows = cases
    s = big_set
    perm = np.random.default_rng(2).permutation(len(rows))
    kk, proofs, pub, want = _rows(rows, perm, s.proof_stride(), s.input_stride(), fill=0xFF)
    assert (proofs == 0xFF).any() and (pub == 0xFF).any()
    assert np.array_equal(s.verify_batch(kk, proofs, pub), want)
    assert np.array_equal(_dev(s, kk, proofs, pub), want)


def _pool(fx):
    """The 8 pool keys and their valid proofs: (key bytes, trapdoor key, proofs (4, pb), inputs (4, nb, 32)) per shape."""
    out = []
    for e in fx['pool']:
        vk, proofs, pub = T.pool_arrays(e)
        out.append((vk, T.shape_key(e['nb_public'], e['n_c']), proofs, pub))
    return out


def test_valid_proofs_under_another_key_answer_0(z, fx):
    pool = _pool(fx)
    s = z.PlonkVerifierSet([p[0] for p in pool])
    ps, ins = s.proof_stride(), s.input_stride()
    kk, proofs, pub, want, src = [], [], [], [], []
    for a, (_, _, P, Q) in enumerate(pool):
        for j in range(len(P)):
            for b in range(len(pool)):
                row = np.zeros(ps, np.uint8); row[:P.shape[1]] = P[j]
                inp = np.zeros((ins // 32, 32), np.uint8); inp[:Q.shape[1]] = Q[j]
                kk.append(b); proofs.append(row); pub.append(inp); want.append(1 if a == b else 0); src.append((a, j))
    kk, proofs, pub, want = np.array(kk, np.uint32), np.stack(proofs), np.stack(pub), np.array(want, np.uint8)
    host = s.verify_batch(kk, proofs, pub)
    assert np.array_equal(host, want)
    assert np.array_equal(_dev(s, kk, proofs, pub), want)
    # the model agrees on a sample of the cross-key pairs: key b reads the first 32 (24 + 3 n_c[b]) bytes and nb_public[b] words of the row
    cross = [i for i in range(len(kk)) if want[i] == 0]
    for i in np.random.default_rng(3).choice(cross, 8, replace=False):
        b = int(kk[i])
        nb, nc, pb = s.key_shape(b)
        inputs = [int.from_bytes(pub[i, w].tobytes(), 'big') for w in range(nb)]
        assert not T.model_verify(pool[b][1], proofs[i, :pb].tobytes(), inputs), (src[i], b)
    s.close()


def test_key_indices_past_the_set_answer_0(z, fx):
    pool = _pool(fx)
    s = z.PlonkVerifierSet([p[0] for p in pool])
    ps, ins = s.proof_stride(), s.input_stride()
    rng = np.random.default_rng(4)
    n = 3000
    k = rng.integers(0, len(pool), n)
    j = rng.integers(0, 4, n)
    proofs = np.zeros((n, ps), np.uint8)
    pub = np.zeros((n, ins // 32, 32), np.uint8)
    for i in range(n):
        _, _, P, Q = pool[k[i]]
        proofs[i, :P.shape[1]] = P[j[i]]
        pub[i, :Q.shape[1]] = Q[j[i]]
    kk = k.astype(np.uint32)
    past = rng.random(n) < 0.25
    kk[past] = rng.choice([len(pool), len(pool) + 1, 1000, 0xFFFFFFFF], int(past.sum()))
    want = (~past).astype(np.uint8)
    assert np.array_equal(s.verify_batch(kk, proofs, pub), want)
    assert np.array_equal(_dev(s, kk, proofs, pub), want)
    s.close()


def _batch(fx, nb, nc, n, bad_every, seed):
    """As test_plonk_keys_gpu._batch: n proofs tiled from the pool, every bad_every-th one damaged."""
    e = next(e for e in fx['pool'] if (e['nb_public'], e['n_c']) == (nb, nc))
    vk, P, Q = T.pool_arrays(e)
    idx = np.random.default_rng(seed).integers(0, len(P), n)
    proofs, pub = P[idx].copy(), Q[idx].copy()
    want = np.ones(n, np.uint8)
    bad = np.arange(bad_every - 1, n, bad_every)
    want[bad] = 0
    for c, i in enumerate(bad):
        if nb and c % 2:
            pub[i, c % nb, 31] ^= 1
        else:
            proofs[i, 12 * 32 + 31] ^= 1
    return vk, proofs, pub, want


@pytest.mark.parametrize('nb,nc', [(2, 1), (128, 0)])
def test_one_key_set_equals_plonk_verifier(z, fx, nb, nc):
    vk, proofs, pub, want = _batch(fx, nb, nc, 1 << 16, 64, 50 + nb)
    v = z.PlonkVerifier(vk)
    s = z.PlonkVerifierSet([vk])
    kk = np.zeros(len(proofs), np.uint32)
    import torch
    dp = torch.from_numpy(proofs).cuda()
    di = torch.from_numpy(np.ascontiguousarray(pub)).cuda()
    out = torch.zeros(len(proofs), dtype=torch.uint8, device='cuda')
    v.verify_batch_dev(len(proofs), dp.data_ptr(), di.data_ptr(), out.data_ptr())
    v.synchronize()
    ref = out.cpu().numpy()
    assert np.array_equal(ref, want)
    assert np.array_equal(_dev(s, kk, proofs, pub), ref)
    assert np.array_equal(s.verify_batch(kk, proofs, pub), v.verify_batch(proofs, pub))
    s.close()
    v.close()


def _objects(xs):
    a = np.empty(len(xs), dtype=object)
    for i, x in enumerate(xs):
        a[i] = x
    return a


def test_large_host_batch_across_the_staging_chunk_in_a_child_process(z, fx):
    """2^17 + 5 proofs over the 8 pool keys through the host entry: at 128 inputs a staging chunk holds 2^17 proofs, so two chunks."""
    pool = _pool(fx)
    with tempfile.TemporaryDirectory() as d:
        f = os.path.join(d, 'pool.npz')
        np.savez(f, vk=_objects([np.frombuffer(p[0], np.uint8) for p in pool]), P=_objects([p[2] for p in pool]), Q=_objects([p[3] for p in pool]))
        code = ('import sys, numpy as np; sys.path.insert(0, %r); import stylus_zkvm_verifiers_amd as z\n'
                'd = np.load(%r, allow_pickle=True)\n'
                's = z.PlonkVerifierSet([bytes(v) for v in d["vk"]])\n'
                'ps, ins = s.proof_stride(), s.input_stride()\n'
                'n = (1 << 17) + 5\n'
                'rng = np.random.default_rng(6)\n'
                'k = rng.integers(0, 8, n); j = rng.integers(0, 4, n)\n'
                'proofs = np.zeros((n, ps), np.uint8); pub = np.zeros((n, ins // 32, 32), np.uint8)\n'
                'for b in range(8):\n'
                '    m = k == b; P, Q = d["P"][b], d["Q"][b]\n'
                '    proofs[m, :P.shape[1]] = P[j[m]]\n'
                '    if Q.shape[1]: pub[m, :Q.shape[1]] = Q[j[m]]\n'
                'want = np.ones(n, np.uint8)\n'
                'bad = np.arange(63, n, 64); want[bad] = 0; proofs[bad, 12 * 32 + 31] ^= 1\n'
                'got = s.verify_batch(k.astype(np.uint32), proofs, pub)\n'
                'assert (got == want).all(), int((got != want).sum())\n'
                'print("large ok")\n') % (ROOT, f)
        r = subprocess.run([sys.executable, '-c', code], capture_output=True, text=True, timeout=900)
        assert r.returncode == 0 and 'large ok' in r.stdout, r.stdout + r.stderr


def test_no_wait_faults_after_the_module(z):
    from stylus_zkvm_verifiers_amd import _lib
    out = C.c_uint64(1)
    assert _lib.lib().zkv_diag_wait_faults(0, C.byref(out)) == 0 and out.value == 0

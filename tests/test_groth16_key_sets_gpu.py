"""Groth16 key sets on the device (include/zkv_groth16_set.h): verdicts against the C oracle proof by proof,
equivalence with per-key Groth16Verifier contexts at scale (also over many chunks in a child process), vk_x, the device entry point on a
caller's stream, and the wait-fault counter."""
import ctypes as C
import os
import random
import subprocess
import sys
import tempfile

import numpy as np
import pytest

import oracle_lib as ol
import spec_model as m

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
VM = {'risc0': 0, 'sp1': 1}
pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def zkv():
    import stylus_zkvm_verifiers_amd as z
    if z.device_count() < 1:
        pytest.skip('no gfx950 device')
    return z


def _parity_set():
    """About ten trapdoor keys (n_ic 1 .. 129, both conventions, one key listed twice, one with IC[1] off the curve, one with gamma at
    infinity) and distinct cases (key, proof words, signals, expected from the oracle)."""
    rng = random.Random(2026)
    keys, tds = [], []
    for j, n_ic in enumerate((1, 2, 3, 6, 7, 17, 129)):
        vk, td = m.trapdoor_vk(rng, n_ic)
        keys.append((vk, n_ic, 'risc0' if j % 2 else 'sp1')); tds.append(td)
    keys.append(keys[2]); tds.append(tds[2])                                                   # the same key twice
    vk, td = m.trapdoor_vk(rng, 3)
    keys.append((dict(vk, ic=[vk['ic'][0], (vk['ic'][1][0], vk['ic'][1][1] ^ 1), vk['ic'][2]]), 3, 'sp1')); tds.append(td)   # IC[1] off the curve
    vk, td = m.trapdoor_vk(rng, 3)
    keys.append((dict(vk, gamma2=((0, 0), (0, 0))), 3, 'risc0')); tds.append(dict(td, gamma=0))                               # gamma at infinity
    cases = []
    for k, ((vk, n_ic, vm), td) in enumerate(zip(keys, tds)):
        vkb = m.vk_to_words(vk)
        for j in range(2):
            sig = [rng.randrange(m.R) for _ in range(n_ic - 1)]
            if j and sig:
                sig[0] = rng.choice([0, 1, m.R - 1])
            prf = m.trapdoor_prove(rng, td, sig, vm)
            words = m.proof_to_words(*prf)
            cases.append((k, words, sig))
            if sig:
                bad = list(sig); bad[-1] = (bad[-1] + 1) % m.R
                cases.append((k, words, bad))
                over = list(sig); over[0] = m.R
                cases.append((k, words, over))
        sig = [rng.randrange(m.R) for _ in range(n_ic - 1)]                                    # a proof made for the other convention
        cases.append((k, m.proof_to_words(*m.trapdoor_prove(rng, td, sig, 'sp1' if vm == 'risc0' else 'risc0')), sig))
    out = []
    for k, words, sig in cases:
        vk, n_ic, vm = keys[k]
        sb = [m.be32(s) for s in sig]
        want = ol.groth16_verify_vk(VM[vm], m.vk_to_words(vk), n_ic, words, sb)
        out.append((k, words, sb, want))
    return [(m.vk_to_words(vk), n_ic, VM[vm]) for vk, n_ic, vm in keys], out


@pytest.fixture(scope='module')
def parity(zkv):
    keys, cases = _parity_set()
    assert any(c[3] for c in cases) and not all(c[3] for c in cases)
    assert not any(c[3] for c in cases if c[0] == 8)                 # the key with an invalid point fails all of its proofs
    s = zkv.Groth16VerifierSet(keys)
    yield s, keys, cases
    s.close()


def _batch(cases, keys, n, seed, stride_words, n_keys):
    """n proofs drawn from the distinct cases, shuffled, with some key indices past the set and garbage in the ignored signal words."""
    rng = np.random.default_rng(seed)
    pick = rng.integers(0, len(cases), n)
    kk = np.array([cases[j][0] for j in pick], dtype=np.uint32)
    want = np.array([cases[j][3] for j in pick], dtype=bool)
    proofs = np.frombuffer(b''.join(cases[j][1] for j in pick), dtype=np.uint8).reshape(n, 256).copy()
    sigs = rng.integers(0, 256, (n, stride_words, 32), dtype=np.uint8)           # garbage everywhere, then the real signals
    for r, j in enumerate(pick):
        for b, s in enumerate(cases[j][2]):
            sigs[r, b] = np.frombuffer(s, dtype=np.uint8)
    off = rng.random(n) < 0.03
    kk[off] = rng.choice([n_keys, n_keys + 1, 0xFFFFFFFF], int(off.sum()))
    want[off] = False
    return kk, proofs, sigs, want


def _dev(zkv, s, kk, proofs, sigs, stream=0):
    import torch
    dev = torch.device('cuda', 0)
    n = len(kk)
    d_k = torch.from_numpy(kk.view(np.int32).copy()).to(dev)
    d_p = torch.from_numpy(proofs.copy()).to(dev)
    d_s = torch.from_numpy(sigs.reshape(n, -1).copy()).to(dev)
    d_v = torch.full((n,), 255, dtype=torch.uint8, device=dev)
    s.verify_batch_dev(n, d_k.data_ptr(), d_p.data_ptr(), d_s.data_ptr(), d_v.data_ptr(), stream)
    if stream:
        torch.cuda.current_stream().synchronize()
    else:
        s.synchronize()
    return d_v.cpu().numpy().astype(bool)


@pytest.mark.parametrize('lanes', [0, 2, 16, 64, 128])
def test_parity_with_the_oracle(zkv, parity, lanes):
    s, keys, cases = parity
    s.set_lanes_per_proof(lanes)
    stride = s.signal_stride() // 32
    for n in (1, 33, 3000):
        kk, proofs, sigs, want = _batch(cases, keys, n, 1000 * lanes + n, stride, len(keys))
        got = s.verify_batch(kk, proofs, sigs)
        assert (got == want).all(), (lanes, n, np.nonzero(got != want)[0][:8])
        assert (_dev(zkv, s, kk, proofs, sigs) == want).all(), (lanes, n)
    s.set_lanes_per_proof(0)


def test_parity_20000_proofs_over_8_keys(zkv, parity):
    s, keys, cases = parity
    sub = [c for c in cases if c[0] < 8 and keys[c[0]][1] <= 17]
    kk, proofs, sigs, want = _batch(sub, keys, 20000, 7, s.signal_stride() // 32, len(keys))
    for lanes in (0, 2):
        s.set_lanes_per_proof(lanes)
        assert (s.verify_batch(kk, proofs, sigs) == want).all(), lanes
    s.set_lanes_per_proof(0)


def test_short_rows_are_padded_and_list_inputs_work(zkv, parity):
    s, keys, cases = parity
    sel = cases[:12]
    got = s.verify_batch([c[0] for c in sel], [c[1] for c in sel], [c[2] for c in sel])
    assert list(got) == [c[3] for c in sel]


def test_vk_x_equals_the_oracle(zkv, parity):
    s, keys, cases = parity
    rng = random.Random(5)
    kk, rows, want = [], [], []
    for k, (vkb, n_ic, _) in enumerate(keys):
        for _ in range(3):
            sig = [m.be32(rng.choice([0, 1, m.R - 1, rng.randrange(m.R)])) for _ in range(n_ic - 1)]
            w = ol.groth16_vk_x_vk(vkb, n_ic, sig)
            if w is None:                                   # (a key whose point a precompile rejects has no vk_x)
                continue
            kk.append(k); rows.append(sig); want.append(w)
    assert len(set(kk)) >= len(keys) - 1
    for lanes in (0, 2, 16, 64):
        s.set_lanes_per_proof(lanes)
        assert s.vk_x_batch(kk, rows) == want, lanes
    s.set_lanes_per_proof(0)


def test_device_entry_on_a_caller_stream(zkv, parity):
    import torch
    s, keys, cases = parity
    kk, proofs, sigs, want = _batch(cases, keys, 5000, 11, s.signal_stride() // 32, len(keys))
    st = torch.cuda.Stream()
    with torch.cuda.stream(st):
        got = _dev(zkv, s, kk, proofs, sigs, st.cuda_stream)
    assert (got == want).all() and (got == s.verify_batch(kk, proofs, sigs)).all()
    assert len(s.last_stage_ms()) == 5


# ---------------------------------------------------------------- equivalence with per-key contexts at scale
def _scale_keys(zkv):
    from stylus_zkvm_verifiers_amd import synth
    rng = random.Random(16)
    keys, batches = [], []
    for j in range(16):
        n_ic = (2, 3, 5, 7, 9, 17)[j % 6]
        vm = 'risc0' if j % 2 else 'sp1'
        vk, td = m.trapdoor_vk(rng, n_ic)
        sig = [rng.randrange(m.R) for _ in range(n_ic - 1)]
        base = m.proof_to_words(*m.trapdoor_prove(rng, td, sig, vm))
        vkb = m.vk_to_words(vk)
        keys.append((vkb, n_ic, VM[vm]))
        batches.append(synth.make_groth16_batch(vkb, vm, base, sig, 4096, seed=100 + j, mutate_every=16)[:2])
    return keys, batches


def test_equivalence_with_per_key_contexts_at_scale(zkv):
    keys, batches = _scale_keys(zkv)
    ref = []
    for (vkb, n_ic, vm), (p, sg) in zip(keys, batches):
        v = zkv.Groth16Verifier(vkb, n_ic, vm)
        ref.append(v.verify_batch(p, sg))
        v.close()
    n = 16 * 4096
    stride = 16
    kk = np.repeat(np.arange(16, dtype=np.uint32), 4096)
    proofs = np.concatenate([b[0] for b in batches])
    sigs = np.zeros((n, stride, 32), np.uint8)
    for j, (p, sg) in enumerate(batches):
        sigs[4096 * j:4096 * (j + 1), :sg.shape[1]] = sg
    want = np.concatenate(ref)
    assert want.any() and not want.all()
    perm = np.random.default_rng(3).permutation(n)
    kk, proofs, sigs, want = kk[perm], proofs[perm], sigs[perm], want[perm]
    s = zkv.Groth16VerifierSet(keys)
    assert (s.verify_batch(kk, proofs, sigs) == want).all()
    assert (_dev(zkv, s, kk, proofs, sigs) == want).all()
    s.close()
    # many chunks: ZKV_CHUNK=4096 in a fresh child process (the chunk size is read per call, but a child keeps this process's contexts apart)
    with tempfile.TemporaryDirectory() as d:
        f = os.path.join(d, 'batch.npz')
        np.savez(f, kk=kk, proofs=proofs, sigs=sigs, want=want, vk=np.array([np.frombuffer(k[0], np.uint8) for k in keys], dtype=object),
                 n_ic=np.array([k[1] for k in keys]), vm=np.array([k[2] for k in keys]))
        code = ('import sys, numpy as np; sys.path.insert(0, %r); import stylus_zkvm_verifiers_amd as z\n'
                'd = np.load(%r, allow_pickle=True)\n'
                's = z.Groth16VerifierSet([(bytes(v), int(n), int(t)) for v, n, t in zip(d["vk"], d["n_ic"], d["vm"])])\n'
                'got = s.verify_batch(d["kk"], d["proofs"], d["sigs"])\n'
                'assert (got == d["want"]).all(), int((got != d["want"]).sum())\n'
                'print("chunked ok")\n') % (ROOT, f)
        env = dict(os.environ, ZKV_CHUNK='4096')
        r = subprocess.run([sys.executable, '-c', code], env=env, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0 and 'chunked ok' in r.stdout, r.stdout + r.stderr


def test_wait_faults_zero(zkv):
    from stylus_zkvm_verifiers_amd import _lib
    out = C.c_uint64(0)
    _lib.check(_lib.lib().zkv_diag_wait_faults(0, C.byref(out)), 'zkv_diag_wait_faults')
    assert out.value == 0

"""Aggregate check on Groth16 key sets (include/zkv_groth16_set.h) on the device: with the check on, verdicts equal
the ones with it off and the C oracle; the counters count the key-uniform sub-batches the layout predicts; cross-key and out-of-range
proofs stay rejected; the fixed mapping and the check switched off leave the counters alone; the device entry on a caller's stream;
several chunks in a child process; and the wait-fault counter."""
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
from test_groth16_key_sets_gpu import VM, _batch, _dev, _parity_set

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
pytestmark = pytest.mark.gpu
SEED = bytes(range(32))


@pytest.fixture(scope='module')
def zkv():
    import stylus_zkvm_verifiers_amd as z
    if z.device_count() < 1:
        pytest.skip('no gfx950 device')
    return z


@pytest.fixture
def low_min(monkeypatch):
    monkeypatch.setenv('ZKV_AGG_MIN', '64')


def _unit(sub):
    return max(64, sub)


def _predicted(kk, capable, sub):
    """Sub-batches the layout forms (zkv_gset_layout.h gset_agg_choose) and, per proof, its sub-batch id (-1: per-proof region)."""
    sb = np.full(len(kk), -1, np.int64)
    total = 0
    for k in np.unique(kk):
        if k >= len(capable) or not capable[k]:
            continue
        idx = np.nonzero(kk == k)[0]
        a = len(idx) // _unit(sub) * _unit(sub)
        sb[idx[:a]] = total + np.arange(a) // sub
        total += a // sub
    return total, sb


def _parity_with_alpha_inf():
    keys, cases = _parity_set()
    rng = random.Random(77)
    vk, td = m.trapdoor_vk(rng, 3)
    vk = dict(vk, alpha1=(0, 0))                                          # alpha at infinity: valid for the oracle's precompiles, not capable
    vkb = m.vk_to_words(vk)
    k = len(keys)
    keys = keys + [(vkb, 3, VM['sp1'])]
    for _ in range(3):
        sig = [rng.randrange(m.R) for _ in range(2)]
        words = m.proof_to_words(*m.trapdoor_prove(rng, td, sig, 'sp1'))
        sb = [m.be32(s) for s in sig]
        cases.append((k, words, sb, ol.groth16_verify_vk(1, vkb, 3, words, sb)))
    return keys, cases


@pytest.fixture(scope='module')
def parity(zkv):
    keys, cases = _parity_with_alpha_inf()
    s = zkv.Groth16VerifierSet(keys)
    yield s, keys, cases
    s.close()


@pytest.mark.parametrize('sub', [None, 16, 32, 64, 128, 256])
def test_parity_with_the_oracle_every_size(zkv, parity, low_min, sub):
    s, keys, cases = parity
    stride = s.signal_stride() // 32
    kk, proofs, sigs, want = _batch(cases, keys, 6000, 31 + (sub or 0), stride, len(keys))
    s.set_aggregate_check(False)
    off = s.verify_batch(kk, proofs, sigs)
    assert (off == want).all()
    c0 = s.aggregate_counters()
    s.set_aggregate_check(True, SEED, sub)
    got = s.verify_batch(kk, proofs, sigs)
    c1 = s.aggregate_counters()
    s.set_aggregate_check(False)
    assert (got == want).all(), (sub, np.nonzero(got != want)[0][:8])
    assert c1[0] > c0[0]                                                   # sub-batches were checked (a set ignored the check before)


def _two_keys(zkv, n_ics=(3, 17), n=4096, mutate_every=0, seed=5):
    from stylus_zkvm_verifiers_amd import synth
    rng = random.Random(seed)
    keys, batches = [], []
    for j, n_ic in enumerate(n_ics):
        vm = 'risc0' if j % 2 else 'sp1'
        vk, td = m.trapdoor_vk(rng, n_ic)
        sig = [rng.randrange(m.R) for _ in range(n_ic - 1)]
        base = m.proof_to_words(*m.trapdoor_prove(rng, td, sig, vm))
        vkb = m.vk_to_words(vk)
        keys.append((vkb, n_ic, VM[vm]))
        batches.append(synth.make_groth16_batch(vkb, vm, base, sig, n, seed=seed + j, mutate_every=mutate_every)[:2])
    return keys, batches


def _stack(batches, stride):
    n = sum(len(b[0]) for b in batches)
    kk = np.concatenate([np.full(len(b[0]), j, np.uint32) for j, b in enumerate(batches)])
    proofs = np.concatenate([b[0] for b in batches])
    sigs = np.zeros((n, max(stride, 1), 32), np.uint8)
    r = 0
    for b in batches:
        if b[1].shape[1]:
            sigs[r:r + len(b[0]), :b[1].shape[1]] = b[1]
        r += len(b[0])
    return kk, proofs, sigs


def test_all_valid_counts_the_predicted_sub_batches(zkv, low_min):
    keys, batches = _two_keys(zkv, (3, 17), 3000)
    s = zkv.Groth16VerifierSet(keys)
    kk, proofs, sigs = _stack(batches, s.signal_stride() // 32)
    perm = np.random.default_rng(1).permutation(len(kk))
    kk, proofs, sigs = kk[perm], proofs[perm], sigs[perm]
    for sub in (16, 64, 256):
        s.set_aggregate_check(True, SEED, sub)
        c0 = s.aggregate_counters()
        assert s.verify_batch(kk, proofs, sigs).all()
        c1 = s.aggregate_counters()
        total, _ = _predicted(kk, [1, 1], sub)
        assert (c1[0] - c0[0], c1[1] - c0[1]) == (total, 0), sub
    s.close()


def test_early_rejects_only_fail_no_sub_batch(zkv, low_min):
    """Signals out of range, C off the curve, B outside the subgroup: rejected before the pairing, so no sub-batch fails."""
    from stylus_zkvm_verifiers_amd import synth
    rng = random.Random(6)
    keys, batches = [], []
    for j, n_ic in enumerate((3, 6)):
        vm = 'risc0' if j % 2 else 'sp1'
        vk, td = m.trapdoor_vk(rng, n_ic)
        sig = [rng.randrange(m.R) for _ in range(n_ic - 1)]
        vkb = m.vk_to_words(vk)
        keys.append((vkb, n_ic, VM[vm]))
        batches.append(synth.make_groth16_batch(vkb, vm, m.proof_to_words(*m.trapdoor_prove(rng, td, sig, vm)), sig, 2048, seed=60 + j,
                                                mutate_every=16, classes=('signal_eq_r', 'c_off_curve', 'b_out_of_subgroup'))[:3])
    s = zkv.Groth16VerifierSet(keys)
    kk, proofs, sigs = _stack(batches, s.signal_stride() // 32)
    mutated = np.concatenate([b[2] for b in batches])
    s.set_aggregate_check(False)
    want = s.verify_batch(kk, proofs, sigs)
    assert (want == ~mutated).all()
    s.set_aggregate_check(True, SEED, 32)
    c0 = s.aggregate_counters()
    assert (s.verify_batch(kk, proofs, sigs) == want).all()
    c1 = s.aggregate_counters()
    assert c1[0] > c0[0] and c1[1] == c0[1]
    s.close()


@pytest.mark.parametrize('sub', [16, 64])
def test_wrong_signals_fail_exactly_their_sub_batches(zkv, low_min, sub):
    keys, batches = _two_keys(zkv, (3, 5), 1024)
    s = zkv.Groth16VerifierSet(keys)
    kk, proofs, sigs = _stack(batches, s.signal_stride() // 32)
    # failures at the end of key 0's last sub-batch and the start of key 1's first: failing sub-batches of two keys side by side
    bad = [1023, 1024, 500, 1800]
    for i in bad:
        sigs[i, 0, 31] ^= 1
    s.set_aggregate_check(False)
    want = s.verify_batch(kk, proofs, sigs)
    assert not want[bad].any() and want.sum() == len(kk) - len(bad)
    s.set_aggregate_check(True, SEED, sub)
    c0 = s.aggregate_counters()
    got = s.verify_batch(kk, proofs, sigs)
    c1 = s.aggregate_counters()
    assert (got == want).all()
    total, sb = _predicted(kk, [1, 1], sub)
    assert c1[0] - c0[0] == total
    assert c1[1] - c0[1] == len(set(int(sb[i]) for i in bad if sb[i] >= 0))
    s.close()


def test_cross_key_proofs_and_keys_past_the_set_are_rejected(zkv, low_min):
    keys, batches = _two_keys(zkv, (4, 4), 1024)
    s = zkv.Groth16VerifierSet(keys)
    kk, proofs, sigs = _stack(batches, s.signal_stride() // 32)
    swapped = (1 - kk).astype(np.uint32)                                    # every proof submitted as the other key (same n_ic)
    past = np.where(np.arange(len(kk)) % 7 == 0, np.uint32(2), kk).astype(np.uint32)
    s.set_aggregate_check(True, SEED, 16)
    assert s.verify_batch(kk, proofs, sigs).all()
    assert not s.verify_batch(swapped, proofs, sigs).any()
    got = s.verify_batch(past, proofs, sigs)
    assert (got == (past < 2)).all()
    s.close()


def test_fixed_mapping_and_check_off_leave_the_counters(zkv, low_min):
    keys, batches = _two_keys(zkv, (3, 9), 1024, mutate_every=64)
    s = zkv.Groth16VerifierSet(keys)
    kk, proofs, sigs = _stack(batches, s.signal_stride() // 32)
    s.set_aggregate_check(True, SEED, 32)
    on = s.verify_batch(kk, proofs, sigs)
    c0 = s.aggregate_counters()
    assert c0[0] > 0
    s.set_lanes_per_proof(16)
    assert (s.verify_batch(kk, proofs, sigs) == on).all()
    assert s.aggregate_counters() == c0
    s.set_lanes_per_proof(0)
    s.set_aggregate_check(False)
    assert (s.verify_batch(kk, proofs, sigs) == on).all()
    assert s.aggregate_counters() == c0
    with pytest.raises(ValueError):
        s.set_aggregate_check(True, SEED, 48)
    s.close()


def test_device_entry_on_a_caller_stream(zkv, parity, low_min):
    import torch
    s, keys, cases = parity
    kk, proofs, sigs, want = _batch(cases, keys, 5000, 12, s.signal_stride() // 32, len(keys))
    s.set_aggregate_check(True, SEED, 16)
    c0 = s.aggregate_counters()
    st = torch.cuda.Stream()
    with torch.cuda.stream(st):
        got = _dev(zkv, s, kk, proofs, sigs, st.cuda_stream)
    assert (got == want).all()
    assert s.aggregate_counters()[0] > c0[0]
    s.set_aggregate_check(False)


def test_scale_in_a_child_process(zkv):
    """Default threshold, OS-drawn secret: 2^18 proofs over 16 keys with a spread of n_ic, and a 1-key n_ic = 129 set over several
    at 2^17 + 1,000 proofs (more than the 2^17 proofs of signals one chunk stages: two aggregate chunks); verdicts equal the per-proof run."""
    from stylus_zkvm_verifiers_amd import synth
    rng = random.Random(18)
    keys, parts = [], []
    for j in range(16):
        n_ic = (2, 3, 5, 9, 17, 33)[j % 6]
        vm = 'risc0' if j % 2 else 'sp1'
        vk, td = m.trapdoor_vk(rng, n_ic)
        sig = [rng.randrange(m.R) for _ in range(n_ic - 1)]
        base = m.proof_to_words(*m.trapdoor_prove(rng, td, sig, vm))
        vkb = m.vk_to_words(vk)
        keys.append((vkb, n_ic, VM[vm]))
        parts.append(synth.make_groth16_batch(vkb, vm, base, sig, 1 << 14, seed=300 + j, mutate_every=1024)[:2])
    vk, td = m.trapdoor_vk(rng, 129)
    sig = [rng.randrange(m.R) for _ in range(128)]
    base = m.proof_to_words(*m.trapdoor_prove(rng, td, sig, 'sp1'))
    long_key = (m.vk_to_words(vk), 129, VM['sp1'])
    long_part = synth.make_groth16_batch(long_key[0], 'sp1', base, sig, 4096, seed=9, mutate_every=512)[:2]
    with tempfile.TemporaryDirectory() as d:
        f = os.path.join(d, 'batch.npz')
        kk, proofs, sigs = _stack(parts, 32)
        perm = np.random.default_rng(4).permutation(len(kk))
        np.savez(f, kk=kk[perm], proofs=proofs[perm], sigs=sigs[perm], vk=np.array([np.frombuffer(k[0], np.uint8) for k in keys], dtype=object),
                 n_ic=np.array([k[1] for k in keys]), vm=np.array([k[2] for k in keys]), lp=long_part[0], ls=long_part[1],
                 lvk=np.frombuffer(long_key[0], np.uint8))
        code = ('import os, sys, numpy as np; sys.path.insert(0, %r); import stylus_zkvm_verifiers_amd as z\n'
                'd = np.load(%r, allow_pickle=True)\n'
                's = z.Groth16VerifierSet([(bytes(v), int(n), int(t)) for v, n, t in zip(d["vk"], d["n_ic"], d["vm"])])\n'
                'want = s.verify_batch(d["kk"], d["proofs"], d["sigs"])\n'
                's.set_aggregate_check(True)\n'
                'got = s.verify_batch(d["kk"], d["proofs"], d["sigs"])\n'
                'assert (got == want).all(), int((got != want).sum())\n'
                'assert s.aggregate_counters()[0] > 0 and want.any() and not want.all()\n'
                'l = z.Groth16VerifierSet([(bytes(d["lvk"]), 129, 1)])\n'
                'n = (1 << 17) + 1000\n'
                'lp = np.resize(d["lp"], (n, 256)); ls = np.resize(d["ls"], (n, 128, 32))\n'
                'kk = np.zeros(n, np.uint32)\n'
                'want = l.verify_batch(kk, lp, ls)\n'
                'l.set_aggregate_check(True)\n'
                'got = l.verify_batch(kk, lp, ls)\n'
                'assert (got == want).all(), int((got != want).sum())\n'
                'c = l.aggregate_counters()\n'
                'assert c[0] > 0 and c[1] > 0 and want.any() and not want.all(), c\n'
                'print("scale ok")\n') % (ROOT, f)
        r = subprocess.run([sys.executable, '-c', code], capture_output=True, text=True, timeout=900)
        assert r.returncode == 0 and 'scale ok' in r.stdout, r.stdout + r.stderr


def test_wait_faults_zero(zkv):
    from stylus_zkvm_verifiers_amd import _lib
    out = C.c_uint64(0)
    _lib.check(_lib.lib().zkv_diag_wait_faults(0, C.byref(out)), 'zkv_diag_wait_faults')
    assert out.value == 0

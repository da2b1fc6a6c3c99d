"""Generic Groth16 keys with up to 128 public signals (`Groth16Verifier::verify_proof_with_key`, common/groth16.rs:23-58, takes a
key of any length): the long-key path (n_ic > 6; include/zkv.h, DESIGN.md "Long keys").  CPU tests run the kernels' own walk through a
host build (tests/host_sim/host_sim_long_key.cpp); GPU tests compare the library with the C oracle."""
import ctypes as C
import json
import os
import random
import subprocess
import sys

import numpy as np
import pytest

import oracle_lib as ol
import spec_model as m

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
VM = {'risc0': 0, 'sp1': 1}


def _sig_bytes(sig):
    return [m.be32(s) for s in sig]


def _key(rng, n_ic):
    vk, td = m.trapdoor_vk(rng, n_ic)
    return vk, td, m.vk_to_words(vk)


# ---------------------------------------------------------------- CPU
@pytest.fixture(scope='module')
def hsl():
    src = os.path.join(HERE, 'host_sim', 'host_sim_long_key.cpp')
    lib = os.path.join(HERE, 'host_sim', 'libhost_sim_long_key.so')
    csrc = os.path.join(ROOT, 'stylus_zkvm_verifiers_amd', 'csrc')
    deps = [src] + [os.path.join(csrc, f) for f in os.listdir(csrc) if f.endswith('.h')]
    if not os.path.exists(lib) or os.path.getmtime(lib) < max(os.path.getmtime(d) for d in deps):
        subprocess.check_call(['g++', '-O2', '-std=c++17', '-fPIC', '-shared', '-Wno-unknown-pragmas', '-o', lib, src])
    L = C.CDLL(lib)
    L.hsl_vk_x.argtypes = [C.c_char_p, C.c_int, C.c_char_p, C.c_int, C.c_char_p]
    L.hsl_verify.argtypes = [C.c_char_p, C.c_int, C.c_int, C.c_char_p, C.c_char_p, C.c_int]
    L.hsl_msm_mads.argtypes = [C.c_char_p, C.c_int, C.c_char_p]
    L.hsl_msm_mads.restype = C.c_ulonglong
    return L


def test_long_keys_construct_without_a_device():
    import stylus_zkvm_verifiers_amd as zkv
    for n_ic in (7, 17, 65, 129):
        vkb = m.vk_to_words(dict(alpha1=(1, 2), beta2=((0, 0), (0, 0)), gamma2=((0, 0), (0, 0)), delta2=((0, 0), (0, 0)),
                                 ic=[(1, 2)] * n_ic))
        v = zkv.Groth16Verifier(vkb, n_ic, zkv.errors.VM_SP1)      # context creation copies the key; the device is set up lazily
        assert v.n_ic == n_ic
        v.close()
    for n_ic in (0, 130):
        with pytest.raises(ValueError):
            zkv.Groth16Verifier(bytes(448 + 64 * n_ic), n_ic)
    from stylus_zkvm_verifiers_amd import _lib
    L = _lib.lib()
    assert L.zkv_groth16_ctx_create(bytes(448 + 64 * 130), 130, 1, 0) is None
    h = L.zkv_groth16_ctx_create(bytes(448 + 64 * 129), 129, 1, 0)
    assert h
    L.zkv_ctx_destroy(h)


def test_long_key_symbol_declared_and_bound():
    hdr = open(os.path.join(ROOT, 'include', 'zkv.h')).read()
    assert 'zkv_groth16_verify_batch_dev(' in hdr and '#define ZKV_GROTH16_MAX_IC 129' in hdr
    from stylus_zkvm_verifiers_amd import _lib
    assert 'zkv_groth16_verify_batch_dev' in _lib.SYMBOLS
    assert hasattr(_lib.lib(), 'zkv_groth16_verify_batch_dev')


@pytest.mark.parametrize('n_ic', [7, 8, 33, 129])
def test_host_walk_vk_x_equals_oracle(hsl, n_ic):
    """The kernels' long-key walk, sliced over 1, 16 and 64 simulated lanes and folded in butterfly order, equals the oracle's
    ecMul / ecAdd chain."""
    rng = random.Random(100 + n_ic)
    vk, _, vkb = _key(rng, n_ic)
    k = n_ic - 1
    sets = [[rng.choice([0, 1, m.R - 1, rng.randrange(m.R)]) for _ in range(k)], [0] * k, [m.R - 1] * k,
            [rng.randrange(m.R) for _ in range(k)]]
    for sig in sets:
        want = ol.groth16_vk_x_vk(vkb, n_ic, _sig_bytes(sig))
        sb = b''.join(_sig_bytes(sig)) + b'\0'
        for lanes in (1, 16, 64):
            out = C.create_string_buffer(64)
            assert hsl.hsl_vk_x(vkb, n_ic, sb, lanes, out) == 1
            assert out.raw == want, (n_ic, lanes)


def test_host_walk_verify_equals_oracle(hsl):
    """The long-key PREP / MSM functions and the unchanged pairing stages against groth16_verify_vk on trapdoor-key proofs, both VMTypes,
    valid and invalid; keys with an invalid IC point and with an IC point at infinity."""
    rng = random.Random(7)
    for n_ic, vm in ((7, 'risc0'), (17, 'sp1'), (33, 'risc0')):
        vk, td, vkb = _key(rng, n_ic)
        k = n_ic - 1
        sig = [rng.randrange(m.R) for _ in range(k)]
        sig[0] = rng.choice([0, 1, m.R - 1])
        prf = m.trapdoor_prove(rng, td, sig, vm)
        cases = [(vm, sig, prf, True), ('sp1' if vm == 'risc0' else 'risc0', sig, prf, False)]
        for j in (0, k // 2, k - 1):
            bad = list(sig); bad[j] = (bad[j] + 1) % m.R
            cases.append((vm, bad, prf, False))
        over = list(sig); over[k - 1] = m.R
        cases.append((vm, over, prf, False))
        a, b, c = prf
        cases.append((vm, sig, (a, b, (c[0], c[1] ^ 1)), False))
        for cvm, csig, (a, b, c), expect in cases:
            words = m.proof_to_words(a, b, c)
            want = ol.groth16_verify_vk(VM[cvm], vkb, n_ic, words, _sig_bytes(csig))
            assert want == expect
            for lanes in (1, 16):
                assert hsl.hsl_verify(vkb, n_ic, 1 if cvm == 'risc0' else 0, words, b''.join(_sig_bytes(csig)) + b'\0', lanes) == int(expect)
    # degenerate keys (n_ic = 9): an invalid IC point fails every proof; an IC point at infinity contributes nothing
    vk, td, _ = _key(rng, 9)
    sig = [rng.randrange(m.R) for _ in range(8)]
    prf = m.trapdoor_prove(rng, td, sig, 'sp1')
    broken = dict(vk, ic=vk['ic'][:5] + [(vk['ic'][5][0], vk['ic'][5][1] ^ 1)] + vk['ic'][6:])
    bb = m.vk_to_words(broken)
    assert not ol.groth16_verify_vk(1, bb, 9, m.proof_to_words(*prf), _sig_bytes(sig))
    assert hsl.hsl_verify(bb, 9, 0, m.proof_to_words(*prf), b''.join(_sig_bytes(sig)), 1) == 0
    vk2 = dict(vk, ic=vk['ic'][:3] + [(0, 0)] + vk['ic'][4:])
    td2 = dict(td, ic=td['ic'][:3] + [0] + td['ic'][4:])
    prf2 = m.trapdoor_prove(rng, td2, sig, 'sp1')
    b2 = m.vk_to_words(vk2)
    assert ol.groth16_verify_vk(1, b2, 9, m.proof_to_words(*prf2), _sig_bytes(sig))
    assert hsl.hsl_verify(b2, 9, 0, m.proof_to_words(*prf2), b''.join(_sig_bytes(sig)), 16) == 1


@pytest.mark.parametrize('vm', ['risc0', 'sp1'])
def test_make_groth16_batch_in_oracle(vm):
    from stylus_zkvm_verifiers_amd import synth
    rng = random.Random(11 if vm == 'risc0' else 12)
    n_ic = 9
    vk, td, vkb = _key(rng, n_ic)
    sig = [rng.randrange(m.R) for _ in range(n_ic - 1)]
    base = m.proof_to_words(*m.trapdoor_prove(rng, td, sig, vm))
    proofs, sigs, mutated, mclass = synth.make_groth16_batch(vkb, vm, base, sig, 96, seed=5, mutate_every=2)
    assert proofs.shape == (96, 256) and sigs.shape == (96, n_ic - 1, 32) and mutated.sum() == 48
    assert len(set(p.tobytes() for p in proofs)) == 96
    for i in range(96):
        got = ol.groth16_verify_vk(VM[vm], vkb, n_ic, proofs[i].tobytes(), [sigs[i, j].tobytes() for j in range(n_ic - 1)])
        assert got == (not mutated[i]), (i, mclass[i])
    assert set(mclass[mutated].tolist()) >= {0, 1, 2, 3, 4, 5}
    # the other convention's delta does not keep the pairing product
    wrong, _, _, _ = synth.make_groth16_batch(vkb, 'sp1' if vm == 'risc0' else 'risc0', base, sig, 2, seed=5, mutate_every=0)
    assert not ol.groth16_verify_vk(VM[vm], vkb, n_ic, wrong[1].tobytes(), _sig_bytes(sig))


# ---------------------------------------------------------------- GPU
@pytest.fixture(scope='module')
def zkv():
    import stylus_zkvm_verifiers_amd as z
    assert z.device_count() >= 1, 'no gfx950 device visible'
    return z


def _vmc(zkv, vm):
    return zkv.errors.VM_RISC0 if vm == 'risc0' else zkv.errors.VM_SP1


def _cases(rng, vk, td, vm):
    """(proof words, signals, expected) for one key: valid, wrong signal first / middle / last, signal = R, A / C off the curve,
    B out of the subgroup."""
    from stylus_zkvm_verifiers_amd import synth
    k = len(vk['ic']) - 1
    out = []
    for j in range(2):
        sig = [rng.choice([0, 1, m.R - 1, rng.randrange(m.R)]) for _ in range(k)]
        prf = m.trapdoor_prove(rng, td, sig, vm)
        out.append((m.proof_to_words(*prf), sig, True))
    for j in (0, k // 2, k - 1):
        bad = list(sig); bad[j] = (bad[j] + 1) % m.R
        out.append((m.proof_to_words(*prf), bad, False))
    over = list(sig); over[k // 2] = m.R
    out.append((m.proof_to_words(*prf), over, False))
    a, b, c = prf
    out.append((m.proof_to_words((a[0], a[1] ^ 1), b, c), sig, False))
    out.append((m.proof_to_words(a, b, (c[0], c[1] ^ 1)), sig, False))
    (xr, xi), (yr, yi) = synth.random_twist_point(synth.SplitMix64(k))
    out.append((m.proof_to_words(a, ((xi, xr), (yi, yr)), c), sig, False))
    return out


@pytest.mark.gpu
@pytest.mark.parametrize('n_ic', [7, 8, 17, 33, 65, 129])
@pytest.mark.parametrize('vm', ['risc0', 'sp1'])
def test_long_key_parity(zkv, n_ic, vm):
    rng = random.Random(1000 * n_ic + VM[vm])
    vk, td, vkb = _key(rng, n_ic)
    cases = _cases(rng, vk, td, vm)
    proofs = [c[0] for c in cases]
    sigs = [_sig_bytes(c[1]) for c in cases]
    want = [ol.groth16_verify_vk(VM[vm], vkb, n_ic, p, s) for p, s in zip(proofs, sigs)]
    assert want == [c[2] for c in cases]
    v = zkv.Groth16Verifier(vkb, n_ic, _vmc(zkv, vm))
    assert list(v.verify_batch(proofs, sigs)) == want
    for lanes in (2, 16, 64, 128):
        v.set_lanes_per_proof(lanes)
        assert list(v.verify_batch(proofs, sigs)) == want, lanes
    v.set_lanes_per_proof(0)
    # vk_x alone
    vsig = [_sig_bytes(c[1]) for c in cases if all(s < m.R for s in c[1])]
    assert v.vk_x_batch(vsig) == [ol.groth16_vk_x_vk(vkb, n_ic, s) for s in vsig]
    v.close()
    # the other VMType convention rejects the valid proofs
    o = zkv.Groth16Verifier(vkb, n_ic, _vmc(zkv, 'sp1' if vm == 'risc0' else 'risc0'))
    assert not any(o.verify_batch(proofs[:2], sigs[:2]))
    o.close()


@pytest.mark.gpu
def test_long_key_degenerate_keys(zkv):
    rng = random.Random(4)
    vk, td, _ = _key(rng, 17)
    sig = [rng.randrange(m.R) for _ in range(16)]
    prf = m.trapdoor_prove(rng, td, sig, 'sp1')
    broken = dict(vk, ic=vk['ic'][:9] + [(vk['ic'][9][0], vk['ic'][9][1] ^ 1)] + vk['ic'][10:])
    v = zkv.Groth16Verifier(m.vk_to_words(broken), 17, zkv.errors.VM_SP1)
    assert not v.verify_batch([m.proof_to_words(*prf)] * 3, [_sig_bytes(sig)] * 3).any()
    v.close()
    vk2 = dict(vk, ic=vk['ic'][:5] + [(0, 0)] + vk['ic'][6:])
    td2 = dict(td, ic=td['ic'][:5] + [0] + td['ic'][6:])
    prf2 = m.trapdoor_prove(rng, td2, sig, 'sp1')
    b2 = m.vk_to_words(vk2)
    bad = list(sig); bad[4] ^= 1                                    # signal 4 multiplies the point at infinity: no effect
    bad2 = list(sig); bad2[5] ^= 1
    v = zkv.Groth16Verifier(b2, 17, zkv.errors.VM_SP1)
    got = v.verify_batch([m.proof_to_words(*prf2)] * 3, [_sig_bytes(sig), _sig_bytes(bad), _sig_bytes(bad2)])
    assert list(got) == [ol.groth16_verify_vk(1, b2, 17, m.proof_to_words(*prf2), _sig_bytes(s)) for s in (sig, bad, bad2)] == [True, True, False]
    assert v.vk_x_batch([_sig_bytes(sig)]) == [ol.groth16_vk_x_vk(b2, 17, _sig_bytes(sig))]
    v.close()


def _batch(n_ic, vm, n, seed):
    from stylus_zkvm_verifiers_amd import synth
    rng = random.Random(seed)
    vk, td, vkb = _key(rng, n_ic)
    sig = [rng.randrange(m.R) for _ in range(n_ic - 1)]
    base = m.proof_to_words(*m.trapdoor_prove(rng, td, sig, vm))
    proofs, sigs, mutated, _ = synth.make_groth16_batch(vkb, vm, base, sig, n, seed=seed, mutate_every=37)
    return vkb, proofs, sigs, mutated


def _oracle_sample(vkb, n_ic, vm, proofs, sigs, got, k=24, seed=0):
    rng = random.Random(seed)
    idx = sorted(set([0, len(proofs) - 1] + [rng.randrange(len(proofs)) for _ in range(k)]))
    for i in idx:
        assert bool(got[i]) == ol.groth16_verify_vk(VM[vm], vkb, n_ic, proofs[i].tobytes(), [sigs[i, j].tobytes() for j in range(n_ic - 1)]), i


@pytest.mark.gpu
def test_long_key_batch_sizes_and_device_entry_point(zkv, monkeypatch):
    """Batches crossing every mapping (one wavefront / 16 lanes per proof in the vk_x stage, and the Miller-stage families), host and
    device entry points, a batch larger than the chunk; mutated <=> rejected on all proofs, the oracle on a sample."""
    import torch
    dev = torch.device('cuda', 0)
    vkb, proofs, sigs, mutated = _batch(17, 'sp1', 70000, 21)
    v = zkv.Groth16Verifier(vkb, 17, zkv.errors.VM_SP1)
    for n in (1, 700, 3000, 13000, 70000):
        got = v.verify_batch(proofs[:n], sigs[:n])
        assert (got == ~mutated[:n]).all(), n
        _oracle_sample(vkb, 17, 'sp1', proofs[:n], sigs[:n], got, k=8, seed=n)
    # device-resident, on the context's stream and on a caller stream
    n = 13000
    d_p, d_s = torch.from_numpy(proofs[:n].copy()).to(dev), torch.from_numpy(sigs[:n].copy()).to(dev)
    d_v = torch.full((n,), 255, dtype=torch.uint8, device=dev)
    v.verify_batch_dev(n, d_p.data_ptr(), d_s.data_ptr(), d_v.data_ptr())
    v.synchronize()
    assert (d_v.cpu().numpy() == (~mutated[:n]).astype(np.uint8)).all()
    d_v.fill_(255)
    v.verify_batch_dev(n, d_p.data_ptr(), d_s.data_ptr(), d_v.data_ptr(), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert (d_v.cpu().numpy() == (~mutated[:n]).astype(np.uint8)).all()
    assert len(v.last_stage_ms()) == 5
    v.close()
    # chunks of 4,096 proofs (ZKV_CHUNK, read per call): the 13,000-proof batch runs as four chunks
    monkeypatch.setenv('ZKV_CHUNK', '4096')
    v = zkv.Groth16Verifier(vkb, 17, zkv.errors.VM_SP1)
    v.reserve(n)
    d_v.fill_(255)
    v.verify_batch_dev(n, d_p.data_ptr(), d_s.data_ptr(), d_v.data_ptr())
    v.synchronize()
    assert (d_v.cpu().numpy() == (~mutated[:n]).astype(np.uint8)).all()
    assert (v.verify_batch(proofs[:n], sigs[:n]) == ~mutated[:n]).all()
    v.close()
    monkeypatch.delenv('ZKV_CHUNK')
    # 128 signals, risc0 convention
    vkb, proofs, sigs, mutated = _batch(129, 'risc0', 3000, 22)
    v = zkv.Groth16Verifier(vkb, 129, zkv.errors.VM_RISC0)
    got = v.verify_batch(proofs, sigs)
    assert (got == ~mutated).all()
    _oracle_sample(vkb, 129, 'risc0', proofs, sigs, got, k=8)
    for lanes in (2, 64):
        v.set_lanes_per_proof(lanes)
        assert (v.verify_batch(proofs[:700], sigs[:700]) == got[:700]).all(), lanes
    v.close()


@pytest.mark.gpu
def test_long_key_sharded_and_aggregate(zkv, monkeypatch):
    import torch
    dev = torch.device('cuda', 0)
    vkb, proofs, sigs, mutated = _batch(33, 'risc0', 3000, 23)
    single = zkv.Groth16Verifier(vkb, 33, zkv.errors.VM_RISC0)
    want = single.verify_batch(proofs, sigs)
    assert (want == ~mutated).all()
    single.close()
    sv = zkv.shard([zkv.Groth16Verifier(vkb, 33, zkv.errors.VM_RISC0, 0) for _ in range(2)])
    assert zkv.shard_count(sv) == 2
    assert (sv.verify_batch(proofs, sigs) == want).all()
    d_p, d_s = torch.from_numpy(proofs.copy()).to(dev), torch.from_numpy(sigs.copy()).to(dev)
    d_v = torch.full((len(proofs),), 255, dtype=torch.uint8, device=dev)
    sv.verify_batch_dev(len(proofs), d_p.data_ptr(), d_s.data_ptr(), d_v.data_ptr())
    sv.synchronize()
    assert (d_v.cpu().numpy() == want.astype(np.uint8)).all()
    assert sv.vk_x_batch(sigs[:4]) == [ol.groth16_vk_x_vk(vkb, 33, [sigs[i, j].tobytes() for j in range(32)]) for i in range(4)]
    sv.close()
    # aggregate check on a long key: accepted, same statuses, the chunks take the per-proof path (counters stay {0, 0})
    monkeypatch.setenv('ZKV_AGG_MIN', '64')
    v = zkv.Groth16Verifier(vkb, 33, zkv.errors.VM_RISC0)
    v.set_aggregate_check(True, seed=bytes(range(32)), sub_batch=16)
    assert (v.verify_batch(proofs, sigs) == want).all()
    assert tuple(v.aggregate_counters()) == (0, 0)
    v.close()


_CHILD = r'''
import json, random, sys
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, sys.argv[1] + '/oracle')
import spec_model as m
import stylus_zkvm_verifiers_amd as zkv
from stylus_zkvm_verifiers_amd import synth
out = {}
for n_ic in (2, 3, 6):
    for vm in ('risc0', 'sp1'):
        rng = random.Random(50 + n_ic)
        vk, td = m.trapdoor_vk(rng, n_ic)
        vkb = m.vk_to_words(vk)
        sig = [rng.randrange(m.R) for _ in range(n_ic - 1)]
        base = m.proof_to_words(*m.trapdoor_prove(rng, td, sig, vm))
        proofs, sigs, mutated, _ = synth.make_groth16_batch(vkb, vm, base, sig, 3000, seed=n_ic, mutate_every=5)
        v = zkv.Groth16Verifier(vkb, n_ic, zkv.errors.VM_RISC0 if vm == 'risc0' else zkv.errors.VM_SP1)
        res = []
        for n in (1, 700, 3000):
            res.append(v.verify_batch(proofs[:n], sigs[:n]).astype(int).tolist())
        res.append([bytes(x).hex() for x in v.vk_x_batch(sigs[:8])])
        res.append(mutated.astype(int).tolist())
        out['%d %s' % (n_ic, vm)] = res
        v.close()
print(json.dumps(out))
'''


@pytest.mark.gpu
def test_long_key_knob_matches_default_path(zkv):
    """ZKV_LONG_KEY=1 (fresh child processes, read at context creation) sends keys with n_ic = 2, 3, 6 through the long-key path: the
    same answers as the default path."""
    runs = {}
    for knob in ('0', '1'):
        env = dict(os.environ, ZKV_LONG_KEY=knob)
        r = subprocess.run([sys.executable, '-c', _CHILD, ROOT], env=env, capture_output=True, text=True, timeout=900)
        assert r.returncode == 0, r.stderr[-3000:]
        runs[knob] = json.loads(r.stdout.strip().splitlines()[-1])
    assert runs['0'] == runs['1']
    for key, res in runs['1'].items():
        mutated = res[-1]
        assert res[2] == [1 - x for x in mutated], key


@pytest.mark.gpu
def test_long_key_wait_faults_zero(zkv):
    from stylus_zkvm_verifiers_amd import _lib
    out = C.c_uint64(0)
    _lib.check(_lib.lib().zkv_diag_wait_faults(0, C.byref(out)), 'zkv_diag_wait_faults')
    assert out.value == 0

"""Aggregate check on PLONK key sets (include/zkv_plonk_set_agg.h) on the MI355X: verdicts with the check on equal
the per-proof run and the model at every sub-batch size, the counters against the model of the class layout (sub-batches run across the
keys of one SRS class), proofs under another key of the same class, early and pairing-level rejects, the conditions under which the check
stays off, the device entry on a caller's stream, and scale in a child process.  PARITY UNPINNED BY CONSTRUCTION (no PLONK in the
reference): expectations are oracle/plonk_model.py's verdicts (plonk_trapdoor_keys.model_verify)."""
import ctypes as C
import os
import subprocess
import sys
import tempfile

import numpy as np
import pytest

import plonk_shared_srs as S
import plonk_trapdoor_keys as T

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
pytestmark = pytest.mark.gpu
SEED = bytes(range(32))
SUBS = (16, 32, 64, 128, 256)


@pytest.fixture(scope='module')
def z():
    import stylus_zkvm_verifiers_amd as z
    assert z.device_count() >= 1, 'no gfx950 device visible'
    return z


@pytest.fixture
def low_min(monkeypatch):
    monkeypatch.setenv('ZKV_AGG_MIN', '64')


def _dev(s, kk, proofs, pub, stream=0):
    import torch
    dk = torch.from_numpy(np.ascontiguousarray(kk).view(np.int32)).cuda()
    dp = torch.from_numpy(np.ascontiguousarray(proofs)).cuda()
    di = torch.from_numpy(np.ascontiguousarray(pub)).cuda() if pub.size else None
    out = torch.zeros(len(kk), dtype=torch.uint8, device='cuda')
    torch.cuda.synchronize()
    s.verify_batch_dev(len(kk), dk.data_ptr(), dp.data_ptr(), di.data_ptr() if di is not None else 0, out.data_ptr(), stream)
    s.synchronize()
    return out.cpu().numpy()


# ---------------------------------------------------------------- the parity set: three classes, rejects of every kind
# class A: four keys of different shapes and a fifth whose S3 is off the curve (valid G2 points, invalid key); class B: one key;
# class C: one key whose [tau]_2 is off the curve (the class is not capable).
PARITY_KEYS = [('A', 0, 0, 0), ('A', 2, 1, 0), ('B', 2, 0, 0), ('A', 9, 0, 0), ('C', 3, 1, 0), ('A', 3, 1, 0), ('A', 2, 0, 7)]
BAD_KEY, OFF_KEY = 6, 4
REJECTS = ('eval_l+1', 'pub0+1', 'scalar12+R', 'scalar19+R', 'L.x+P', 'Z=inf', '-Hzw', 'H0.y^1', 'pub0=R')
EARLY = ('scalar12+R', 'scalar19+R', 'L.x+P', 'H0.y^1', 'pub0=R')              # rejected before the pairing equation (range, curve)


def _parity_keys():
    vks = [S.key_bytes(*k) for k in PARITY_KEYS]
    vks[BAD_KEY] = T.apply_case('key_S3_off_curve', vks[BAD_KEY], b'', [])[0]
    vks[OFF_KEY] = T.apply_case('key_tau2_off_curve', vks[OFF_KEY], b'', [])[0]
    return vks


def _parity_cases(vks):
    """The distinct cases (key index, proof bytes, 32-byte inputs, model verdict, name): per key three valid proofs and every reject of the
    first, and a valid proof of key 1 presented under key 5 (another shape of the same class)."""
    cases = []
    for k, (cls, nb, nc, tag) in enumerate(PARITY_KEYS):
        for j in range(3):
            proof, pub = S.valid(cls, nb, nc, tag, j)
            names = ('valid',) + (tuple(n for n in REJECTS if nb or not n.startswith('pub')) if j == 0 else ())
            for name in names:
                _, p, q = T.apply_case(name, vks[k], proof, list(pub))
                cases.append((k, p, [x.to_bytes(32, 'big') for x in q], name))
    proof, pub = S.valid('A', 2, 1, 0, 1)
    cases.append((5, proof, [x.to_bytes(32, 'big') for x in pub] + [bytes(32)], 'under_key5'))
    out = []
    for k, p, q, name in cases:
        nb, nc = PARITY_KEYS[k][1], PARITY_KEYS[k][2]
        model = T.pm.plonk_verify(T.parse_vk(vks[k]), T.pad27(p[:32 * (24 + 3 * nc)]), [int.from_bytes(x, 'big') for x in q[:nb]])
        out.append((k, p, q, int(bool(model)), name))
    assert all(c[3] == 0 for c in out if c[0] in (BAD_KEY, OFF_KEY) or c[4] != 'valid')
    assert all(c[3] == 1 for c in out if c[4] == 'valid' and c[0] not in (BAD_KEY, OFF_KEY))
    return out


@pytest.fixture(scope='module')
def parity(z):
    vks = _parity_keys()
    cases = _parity_cases(vks)
    s = z.PlonkVerifierSet(vks)
    yield s, cases
    s.close()


def _batch(s, cases, n, seed, past=0.02):
    rng = np.random.default_rng(seed)
    pick = rng.integers(0, len(cases), n)
    ps, ins = s.proof_stride(), s.input_stride()
    kk = np.array([cases[j][0] for j in pick], np.uint32)
    proofs = np.zeros((n, ps), np.uint8)
    pub = np.zeros((n, ins // 32, 32), np.uint8)
    for j in np.unique(pick):
        rows = np.nonzero(pick == j)[0]
        p, q = cases[j][1], cases[j][2]
        proofs[rows, :len(p)] = np.frombuffer(p, np.uint8)
        if q:
            pub[rows, :len(q)] = np.frombuffer(b''.join(q), np.uint8).reshape(len(q), 32)
    want = np.array([cases[j][3] for j in pick], np.uint8)
    gone = rng.random(n) < past                                               # key indices past the set
    kk[gone] = rng.choice([s.size(), 1000, 0xFFFFFFFF], int(gone.sum()))
    want[gone] = 0
    return kk, proofs, pub, want


@pytest.mark.parametrize('sub', (None,) + SUBS)
def test_parity_at_every_size(parity, low_min, sub):
    s, cases = parity
    assert s.srs_classes() == ([0, 0, 1, 0, 2, 0, 0], 3)
    kk, proofs, pub, want = _batch(s, cases, 5000, 10 + (sub or 0))
    s.set_aggregate_check(False)
    off = s.verify_batch(kk, proofs, pub)
    assert np.array_equal(off, want), [int(k) for k in kk[off != want]][:8]
    s.set_aggregate_check(True, SEED, sub)
    c0 = s.aggregate_counters()
    on = s.verify_batch(kk, proofs, pub)
    c1 = s.aggregate_counters()
    s.set_aggregate_check(False)
    assert np.array_equal(on, want), int((on != want).sum())
    assert c1[0] > c0[0], 'the set ignored the aggregate check'               # (fails on a library whose sets run the per-proof path only)
    assert c1[1] > c0[1]                                                       # pairing-level rejects are in the batch
    assert len(s.last_stage_ms()) == 5


# ---------------------------------------------------------------- counters against the layout
def _valid_set(z, keys, n_valid=2):
    s = z.PlonkVerifierSet([S.key_bytes(*k) for k in keys])
    ps, ins = s.proof_stride(), s.input_stride()
    return s, [S.rows_of(*k, n_valid, ps, ins) for k in keys]


def _valid_batch(pool, kk, seed):
    rng = np.random.default_rng(seed)
    j = rng.integers(0, len(pool[0][0]), len(kk))
    proofs = np.stack([pool[k][0][jj] for k, jj in zip(kk, j)])
    pub = np.stack([pool[k][1][jj] for k, jj in zip(kk, j)])
    return proofs, pub


def test_counters_equal_the_layout_model(z, low_min):
    keys = [('A', 2, 0, 0), ('B', 2, 0, 0), ('A', 0, 0, 0), ('B', 1, 1, 0), ('A', 2, 1, 0)]
    s, pool = _valid_set(z, keys)
    cls, ncls = s.srs_classes()
    assert (cls, ncls) == ([0, 1, 0, 1, 0], 2)
    rng = np.random.default_rng(3)
    kk = rng.choice(5, 3001, p=[0.4, 0.3, 0.15, 0.1, 0.05]).astype(np.uint32)
    proofs, pub = _valid_batch(pool, kk, 4)
    for sub in SUBS:
        s.set_aggregate_check(True, SEED, sub)
        c0 = s.aggregate_counters()
        got = s.verify_batch(kk, proofs, pub)
        c1 = s.aggregate_counters()
        total, _ = S.predict(kk, 5, cls, [1, 1], sub)
        assert got.all() and (c1[0] - c0[0], c1[1] - c0[1]) == (total, 0), (sub, c0, c1, total)
    s.close()


def test_sub_batches_cross_keys(z, low_min):
    """16 keys of one class with 8 proofs each: 16 key groups of 64 slots, so 16 sub-batches of 64 slots (eight live lanes each); a
    per-key layout could form none at all (no key reaches 64 proofs)."""
    keys = [('A', (0, 2)[t % 2], (t // 2) % 2, t) for t in range(16)]
    s, pool = _valid_set(z, keys, 1)
    assert s.srs_classes() == ([0] * 16, 1)
    kk = np.repeat(np.arange(16, dtype=np.uint32), 8)
    np.random.default_rng(8).shuffle(kk)
    proofs, pub = _valid_batch(pool, kk, 5)
    total, sb = S.predict(kk, 16, [0] * 16, [1], 64)
    assert total == 16 and (sb >= 0).all()
    s.set_aggregate_check(True, SEED, 64)
    c0 = s.aggregate_counters()
    got = s.verify_batch(kk, proofs, pub)
    c1 = s.aggregate_counters()
    assert got.all() and (c1[0] - c0[0], c1[1] - c0[1]) == (16, 0)
    # ... and with 256-slot sub-batches four key groups share one
    s.set_aggregate_check(True, SEED, 256)
    c0 = s.aggregate_counters()
    assert s.verify_batch(kk, proofs, pub).all()
    c1 = s.aggregate_counters()
    assert (c1[0] - c0[0], c1[1] - c0[1]) == (4, 0)
    s.close()


def test_a_proof_valid_under_another_key_of_the_class_is_rejected(z, low_min):
    """PREP binds a proof to its key through the transcript; the shared SRS must not weaken that."""
    keys = [('A', 2, 0, 0), ('A', 2, 0, 1), ('B', 2, 0, 2)]                   # same shape: two of one class, one of another
    s, pool = _valid_set(z, keys)
    assert s.srs_classes() == ([0, 0, 1], 2)
    own = np.tile(np.arange(3, dtype=np.uint32), 400)
    proofs, pub = _valid_batch(pool, own, 6)
    s.set_aggregate_check(True, SEED, 32)
    assert s.verify_batch(own, proofs, pub).all()
    for shift in (1, 2):                                                       # 0 <-> 1 is the same-class swap; the others cross classes
        kk = ((own + shift) % 3).astype(np.uint32)
        c0 = s.aggregate_counters()
        got = s.verify_batch(kk, proofs, pub)
        assert not got.any() and s.aggregate_counters()[0] > c0[0]
    swap = np.array([1, 0, 2], np.uint32)[own]
    got = s.verify_batch(swap, proofs, pub)
    assert np.array_equal(got, (own == 2).astype(np.uint8))
    i = int(np.nonzero(own == 0)[0][0])
    assert not T.model_verify(S.key(*keys[1]), proofs[i, :768].tobytes(), [int.from_bytes(pub[i, w].tobytes(), 'big') for w in range(2)])
    s.close()


def test_early_rejects_fail_no_sub_batch(parity, low_min):
    s, cases = parity
    keep = [c for c in cases if c[4] == 'valid' and c[0] not in (BAD_KEY, OFF_KEY) or c[4] in EARLY]
    assert any(c[4] in EARLY for c in keep)
    kk, proofs, pub, want = _batch(s, keep, 4000, 21)
    assert want.any() and not want.all()
    s.set_aggregate_check(True, SEED, 32)
    c0 = s.aggregate_counters()
    got = s.verify_batch(kk, proofs, pub)
    c1 = s.aggregate_counters()
    s.set_aggregate_check(False)
    assert np.array_equal(got, want) and c1[0] > c0[0] and c1[1] == c0[1]


@pytest.mark.parametrize('sub', SUBS)
def test_pairing_level_rejects_fail_exactly_their_sub_batches(z, low_min, sub):
    keys = [('A', 2, 0, 0), ('A', 0, 0, 0), ('B', 2, 0, 0), ('A', 2, 1, 0)]
    s, pool = _valid_set(z, keys)
    cls = [0, 0, 1, 0]
    cnt = [40, 100, 300, 70]
    kk = np.repeat(np.arange(4, dtype=np.uint32), cnt)
    perm = np.random.default_rng(31).permutation(len(kk))
    kk = kk[perm]
    proofs, pub = _valid_batch(pool, kk, 32)
    total, sb = S.predict(kk, 4, cls, [1, 1], sub)
    lay = S.layout(cnt, cls, [1, 1], sub)
    sl = S.slots_of(kk, 4, lay)
    at = lambda slot: int(np.nonzero(sl == slot)[0][0])
    # the last proof of key 0's group and the first of key 1's (slots 39 and 64: one sub-batch from 128 slots on), the last proof of
    # class A (key 3) next to the first of class B (key 2), two in one sub-batch, and the last proof of the region
    hit = [at(lay['start'][0] + 39), at(lay['start'][1]), at(lay['start'][3] + 69), at(lay['start'][2]), at(lay['start'][2] + 1), at(lay['start'][2] + 299)]
    S.damage_at_the_pairing(proofs, hit)
    want = np.ones(len(kk), np.uint8)
    want[hit] = 0
    s.set_aggregate_check(False)
    assert np.array_equal(s.verify_batch(kk, proofs, pub), want)
    s.set_aggregate_check(True, SEED, sub)
    c0 = s.aggregate_counters()
    got = s.verify_batch(kk, proofs, pub)
    c1 = s.aggregate_counters()
    assert np.array_equal(got, want)
    assert sb[hit[2]] != sb[hit[3]]                                            # two classes never share a sub-batch
    assert (sb[hit[0]] == sb[hit[1]]) == (sub >= 128)                          # two keys of a class do
    assert (c1[0] - c0[0], c1[1] - c0[1]) == (total, len(set(sb[hit]))), (sub, c0, c1, total, sb[hit])
    s.close()


def test_fixed_mapping_check_off_and_small_calls_leave_the_counters(parity, low_min, monkeypatch):
    s, cases = parity
    kk, proofs, pub, want = _batch(s, cases, 3000, 41)
    s.set_aggregate_check(True, SEED, 32)
    s.verify_batch(kk[:64], proofs[:64], pub[:64])                             # (counters exist from here on)
    c0 = s.aggregate_counters()
    for lanes in (2, 16, 64):                                                  # a fixed mapping
        s.set_lanes_per_proof(lanes)
        assert np.array_equal(s.verify_batch(kk, proofs, pub), want) and s.aggregate_counters() == c0
    s.set_lanes_per_proof(0)
    s.set_aggregate_check(False)                                               # the check off
    assert np.array_equal(s.verify_batch(kk, proofs, pub), want) and s.aggregate_counters() == c0
    s.set_aggregate_check(True, SEED, 32)
    monkeypatch.setenv('ZKV_AGG_MIN', '4096')                                  # a call below the threshold
    assert np.array_equal(s.verify_batch(kk, proofs, pub), want) and s.aggregate_counters() == c0
    assert np.array_equal(_dev(s, kk, proofs, pub), want) and s.aggregate_counters() == c0
    monkeypatch.setenv('ZKV_AGG_MIN', '64')
    assert np.array_equal(s.verify_batch(kk, proofs, pub), want) and s.aggregate_counters()[0] > c0[0]
    s.set_aggregate_check(False)


def test_device_entry_on_a_caller_stream(parity, low_min):
    import torch
    s, cases = parity
    kk, proofs, pub, want = _batch(s, cases, 5000, 51)
    s.set_aggregate_check(True, SEED, 16)
    c0 = s.aggregate_counters()
    st = torch.cuda.Stream()
    with torch.cuda.stream(st):
        got = _dev(s, kk, proofs, pub, st.cuda_stream)
    c1 = s.aggregate_counters()
    host = s.verify_batch(kk, proofs, pub)
    s.set_aggregate_check(False)
    assert np.array_equal(got, want) and np.array_equal(host, got) and c1[0] > c0[0]


def _objects(xs):
    a = np.empty(len(xs), dtype=object)
    for i, x in enumerate(xs):
        a[i] = x
    return a


def test_scale_in_a_child_process(z):
    """Default threshold, OS-drawn secret: 2^18 rows over 16 keys of one class with one proof in 1,024 damaged at the pairing, and a host
    batch of 2^17 + 1,000 rows of a 128-input key (a staging chunk holds 2^17 of them: two chunks, the first at the threshold)."""
    keys = [('A', (0, 2, 9, 3)[t % 4], (t // 4) % 2, t) for t in range(16)]
    vks = [S.key_bytes(*k) for k in keys]
    big = ('B', 128, 0, 0)
    with tempfile.TemporaryDirectory() as d:
        f = os.path.join(d, 'pool.npz')
        pools = [S.rows_of(*k, 2, 864, 32 * 9) for k in keys]
        bp, bq = S.rows_of(*big, 2, 768, 32 * 128)
        np.savez(f, vk=_objects([np.frombuffer(v, np.uint8) for v in vks]), P=_objects([p[0] for p in pools]), Q=_objects([p[1] for p in pools]),
                 bvk=np.frombuffer(S.key_bytes(*big), np.uint8), bp=bp, bq=bq)
        code = ('import sys, numpy as np; sys.path.insert(0, %r); import stylus_zkvm_verifiers_amd as z\n'
                'd = np.load(%r, allow_pickle=True)\n'
                'R = 21888242871839275222246405745257275088548364400416034343698204186575808495617\n'
                'def damage(P, rows):\n'
                '    for i in rows:\n'
                '        v = (int.from_bytes(P[i, 384:416].tobytes(), "big") + 1) %% R\n'
                '        P[i, 384:416] = np.frombuffer(v.to_bytes(32, "big"), np.uint8)\n'
                's = z.PlonkVerifierSet([bytes(v) for v in d["vk"]])\n'
                'assert s.srs_classes() == ([0] * 16, 1)\n'
                'n = 1 << 18\n'
                'rng = np.random.default_rng(6)\n'
                'k = rng.integers(0, 16, n); j = rng.integers(0, 2, n)\n'
                'proofs = np.zeros((n, s.proof_stride()), np.uint8); pub = np.zeros((n, s.input_stride() // 32, 32), np.uint8)\n'
                'for b in range(16):\n'
                '    m = k == b; P, Q = d["P"][b], d["Q"][b]\n'
                '    proofs[m] = P[j[m]]; pub[m] = Q[j[m]]\n'
                'bad = np.arange(1023, n, 1024); damage(proofs, bad)\n'
                'want = np.ones(n, np.uint8); want[bad] = 0\n'
                'kk = k.astype(np.uint32)\n'
                'off = s.verify_batch(kk, proofs, pub)\n'
                'assert (off == want).all(), int((off != want).sum())\n'
                's.set_aggregate_check(True)\n'
                'on = s.verify_batch(kk, proofs, pub)\n'
                'assert (on == off).all(), int((on != off).sum())\n'
                'c = s.aggregate_counters()\n'
                'assert c[0] > 0 and c[1] > 0 and on.any() and not on.all(), c\n'
                's.close()\n'
                'l = z.PlonkVerifierSet([bytes(d["bvk"])])\n'
                'n = (1 << 17) + 1000\n'
                'lp = np.resize(d["bp"], (n, 768)).copy(); lq = np.resize(d["bq"], (n, 128, 32))\n'
                'bad = np.arange(511, n, 1024); damage(lp, bad)\n'
                'kk = np.zeros(n, np.uint32)\n'
                'off = l.verify_batch(kk, lp, lq)\n'
                'want = np.ones(n, np.uint8); want[bad] = 0\n'
                'assert (off == want).all(), int((off != want).sum())\n'
                'l.set_aggregate_check(True)\n'
                'on = l.verify_batch(kk, lp, lq)\n'
                'assert (on == off).all(), int((on != off).sum())\n'
                'c = l.aggregate_counters()\n'
                'assert c[0] > 0 and c[1] > 0 and on.any() and not on.all(), c\n'
                'print("scale ok")\n') % (ROOT, f)
        r = subprocess.run([sys.executable, '-c', code], capture_output=True, text=True, timeout=900)
        assert r.returncode == 0 and 'scale ok' in r.stdout, r.stdout + r.stderr


def test_no_wait_faults_after_the_module(z):
    from stylus_zkvm_verifiers_amd import _lib
    out = C.c_uint64(1)
    assert _lib.lib().zkv_diag_wait_faults(0, C.byref(out)) == 0 and out.value == 0

"""Valid proofs that reach the point-at-infinity and zero-scalar branches (tests/degenerate_cases.py), and their one-value siblings,
through every device entry point: Groth16Verifier (short and long keys, every mapping, host and device-resident batches, the single
call), Groth16VerifierSet, PlonkVerifier, PlonkVerifierSet, Sp1PlonkVerifier and an Sp1Gateway route, and the aggregate check.  Every
status must equal the C oracle's.  Degenerate proofs sit among ordinary valid ones of the same key inside one wavefront (a branch taken
by some lanes and not by others), at lane 0, at lane 63 and at both ends of 16- and 64-proof sub-batches."""
import random

import numpy as np
import pytest

import degenerate_cases as D
import oracle_lib as ol
import plonk_trapdoor_keys as T
import spec_model as m

pytestmark = pytest.mark.gpu

N = 128                                                       # two wavefronts of one-lane-per-proof, 8 / 2 sub-batches of 16 / 64
SLOTS = [0, 63, 15, 16, 64, 127, 47, 48, 31, 32, 79, 80, 111, 112, 1, 62]     # lane 0, lane 63, both ends of sub-batches


@pytest.fixture(scope='module')
def zkv():
    import stylus_zkvm_verifiers_amd as z
    assert z.device_count() >= 1, 'no gfx950 device visible'
    return z


def _layout(cases, filler):
    """A batch of N: the cases at SLOTS (then after them), every other row an ordinary valid proof from filler(i).  Returns (rows,
    expected, index of each case)."""
    assert len(cases) <= N // 2
    at = (SLOTS + [s for s in range(N) if s not in SLOTS])[:len(cases)]
    rows, want = [None] * N, [True] * N
    for j, (row, w) in zip(at, cases):
        rows[j], want[j] = row, w
    for i in range(N):
        if rows[i] is None:
            rows[i] = filler(i)
    return rows, want, at


def _g16_groups(cases):
    groups = {}
    for c in cases:
        groups.setdefault((c[3], c[1]), []).append(c)
    return groups


def _g16_batch(key, cs, seed):
    vkb, vm = key
    rng = random.Random(seed)
    rows, want, at = _layout([((c[4], c[5]), c[6]) for c in cs], lambda i: D.ordinary_g16(vkb, vm, rng))
    sigs = [[m.be32(s) for s in sig] for _, sig in rows]
    # the oracle's verdict on every degenerate row (and on the first ordinary one)
    n_ic = len(sigs[0]) + 1
    for j in at + [next(i for i in range(N) if i not in at)]:
        assert ol.groth16_verify_vk(D.VM[vm], vkb, n_ic, rows[j][0], sigs[j]) == want[j], j
    return [w for w, _ in rows], sigs, np.array(want)


def _vmc(zkv, vm):
    return zkv.errors.VM_RISC0 if vm == 'risc0' else zkv.errors.VM_SP1


def _g16_every_entry_point(zkv, cases, lanes_list):
    import torch
    dev = torch.device('cuda', 0)
    for g, (key, cs) in enumerate(sorted(_g16_groups(cases).items(), key=lambda kv: kv[1][0][0])):
        proofs, sigs, want = _g16_batch(key, cs, g)
        n_ic = len(cs[0][2]['ic'])
        v = zkv.Groth16Verifier(key[0], n_ic, _vmc(zkv, key[1]))
        for lanes in lanes_list:
            v.set_lanes_per_proof(lanes)
            got = v.verify_batch(proofs, sigs)
            assert np.array_equal(got, want), (cs[0][0], lanes, np.nonzero(got != want)[0].tolist())
        v.set_lanes_per_proof(0)
        d_p = torch.from_numpy(np.frombuffer(b''.join(proofs), np.uint8).reshape(N, 256).copy()).to(dev)
        d_s = torch.from_numpy(np.frombuffer(b''.join(b''.join(s) for s in sigs) + b'\0', np.uint8)[:N * 32 * (n_ic - 1)].copy()).to(dev)
        d_v = torch.full((N,), 255, dtype=torch.uint8, device=dev)
        v.verify_batch_dev(N, d_p.data_ptr(), d_s.data_ptr() if n_ic > 1 else 0, d_v.data_ptr())
        v.synchronize()
        assert np.array_equal(d_v.cpu().numpy(), want.astype(np.uint8)), cs[0][0]
        for name, vm, vk, vkb, words, sig, w in cs:
            x = [int.from_bytes(words[32 * i:32 * i + 32], 'big') for i in range(8)]
            assert v.verify_proof_with_key(x[0:2], [x[2:4], x[4:6]], x[6:8], sig) == w, name
        v.close()


def test_groth16_short_keys_every_mapping_and_entry_point(zkv):
    _g16_every_entry_point(zkv, D.short_cases(), (0, 128, 64, 16, 2))


def test_groth16_long_keys_every_mapping_and_entry_point(zkv):
    _g16_every_entry_point(zkv, D.long_cases(), (0, 128, 64, 16, 2))


def _agg_ok_key(vk):
    return vk['alpha1'] != (0, 0) and vk['beta2'] != ((0, 0), (0, 0))


@pytest.mark.parametrize('sub', [16, 64])
def test_groth16_aggregate_check(zkv, monkeypatch, sub):
    """All-valid degenerate batches: every status accepts and no sub-batch fails (a key with alpha or beta at infinity, and a long key,
    take the documented per-proof fallback: counters stay {0, 0}).  Batches with the siblings: the oracle's statuses."""
    monkeypatch.setenv('ZKV_AGG_MIN', '64')
    for g, (key, cs) in enumerate(sorted(_g16_groups(D.short_cases() + D.long_cases()).items(), key=lambda kv: kv[1][0][0])):
        vk, n_ic = cs[0][2], len(cs[0][2]['ic'])
        v = zkv.Groth16Verifier(key[0], n_ic, _vmc(zkv, key[1]))
        v.set_aggregate_check(True, seed=bytes(range(32)), sub_batch=sub)
        valid = [c for c in cs if c[6]]
        proofs, sigs, want = _g16_batch(key, valid, 100 + g)
        got = v.verify_batch(proofs, sigs)
        assert got.all(), (valid[0][0], sub, np.nonzero(~got)[0].tolist())
        checked, failed = v.aggregate_counters()
        if _agg_ok_key(vk) and n_ic <= 6:
            assert checked > 0 and failed == 0, (valid[0][0], sub, checked, failed)
        else:
            assert (checked, failed) == (0, 0), valid[0][0]
        proofs, sigs, want = _g16_batch(key, cs, 200 + g)
        got = v.verify_batch(proofs, sigs)
        assert np.array_equal(got, want), (cs[0][0], sub, np.nonzero(got != want)[0].tolist())
        v.close()


def _set_rows(groups, extra_keys, seed):
    """Key set rows: degenerate keys (with their cases), then ordinary keys; proofs interleaved by key, round robin."""
    rng = random.Random(seed)
    keys = [(k[0], len(cs[0][2]['ic']), k[1]) for k, cs in groups] + extra_keys
    queues = [[(c[4], c[5], c[6]) for c in cs] for _, cs in groups]
    rows = []
    while any(queues):
        for k, q in enumerate(queues):
            if q:
                rows.append((k,) + q.pop(0))
            vkb, vm = keys[k][0], keys[k][2]
            rows.append((k,) + D.ordinary_g16(vkb, vm, rng) + (True,))
    for k in range(len(groups), len(keys)):                  # ordinary keys: ordinary proofs
        for _ in range(3):
            rows.append((k,) + D.ordinary_g16(keys[k][0], keys[k][2], rng) + (True,))
    return keys, rows


@pytest.mark.parametrize('sub', [0, 16, 64])
def test_groth16_key_set_mixes_degenerate_and_ordinary_keys(zkv, monkeypatch, sub):
    """Degenerate keys (short and n_ic = 9) beside ordinary ones, proofs interleaved by key; the same batch through the aggregate check
    (sub-batches of 16 / 64; the valid-only batch must not fail a sub-batch)."""
    groups = sorted(_g16_groups(D.short_cases() + [c for c in D.long_cases() if len(c[2]['ic']) == 9]).items(), key=lambda kv: kv[1][0][0])
    extra = []
    for n_ic, vm in ((3, 'sp1'), (5, 'risc0'), (9, 'sp1')):
        vk, td = D.g16_key(random.Random('ordinary %d' % n_ic), n_ic)
        vkb = m.vk_to_words(vk)
        D.TRAPDOORS[vkb] = td
        extra.append((vkb, n_ic, vm))
    named, rows = _set_rows(groups, extra, 7 + sub)
    keys = [(vkb, n_ic, _vmc(zkv, vm)) for vkb, n_ic, vm in named]
    s = zkv.Groth16VerifierSet(keys)
    if sub:
        monkeypatch.setenv('ZKV_AGG_MIN', '64')
        s.set_aggregate_check(True, seed=bytes(range(32)), sub_batch=sub)
        # every sub-batch holds proofs of one key, and a key takes the check in units of max(64, sub) proofs: each key's valid rows,
        # padded with ordinary proofs to a multiple of the unit, interleaved by key
        rng, unit = random.Random(sub), max(64, sub)
        per_key = [[r for r in rows if r[0] == k and r[3]] for k in range(len(named))]
        per_key = [q + [(k,) + D.ordinary_g16(named[k][0], named[k][2], rng) + (True,) for _ in range(-len(q) % unit)] for k, q in enumerate(per_key)]
        valid = [q[j] for j in range(max(map(len, per_key))) for q in per_key if j < len(q)]
        got = s.verify_batch([r[0] for r in valid], [r[1] for r in valid], [[m.be32(x) for x in r[2]] for r in valid])
        assert got.all(), np.nonzero(~got)[0].tolist()
        checked, failed = s.aggregate_counters()
        assert checked > 0 and failed == 0, (checked, failed)
    for i, (k, words, sig, w) in enumerate(rows):
        vkb, n_ic, vm = keys[k]
        assert ol.groth16_verify_vk(0 if vm == zkv.errors.VM_RISC0 else 1, vkb, n_ic, words, [m.be32(x) for x in sig]) == w, i
    want = np.array([r[3] for r in rows])
    for lanes in ((0,) if sub else (0, 128, 64, 16, 2)):      # the aggregate check runs with the automatic mapping only
        s.set_lanes_per_proof(lanes)
        got = s.verify_batch([r[0] for r in rows], [r[1] for r in rows], [[m.be32(x) for x in r[2]] for r in rows])
        assert np.array_equal(got, want), (lanes, np.nonzero(got != want)[0].tolist())
    s.close()


# ---------------------------------------------------------------- PLONK
def _plonk_groups():
    groups = {}
    for c in D.plonk_cases():
        groups.setdefault(c[4], []).append(c)
    return sorted(groups.items(), key=lambda kv: kv[1][0][0])


def _plonk_batch(cs, seed):
    rng = random.Random(seed)
    rows, want, at = _layout([((c[5], c[6]), c[7]) for c in cs], lambda i: D.ordinary_plonk(cs[0][4], rng))
    pubs = [[x.to_bytes(32, 'big') for x in pub] for _, pub in rows]
    for j in at + [next(i for i in range(N) if i not in at)]:
        assert ol.plonk_verify(cs[0][4], T.pad27(rows[j][0]), pubs[j]) == want[j], j
    return [p for p, _ in rows], pubs, np.array(want, dtype=np.uint8)


def test_plonk_every_mapping_and_device_batch(zkv):
    import torch
    dev = torch.device('cuda', 0)
    for g, (vkb, cs) in enumerate(_plonk_groups()):
        proofs, pubs, want = _plonk_batch(cs, g)
        v = zkv.PlonkVerifier(vkb)
        for lanes in (0, 2, 16, 64, 128):
            v.set_lanes_per_proof(lanes)
            got = v.verify_batch(proofs, pubs)
            assert np.array_equal(got, want), (cs[0][0], lanes, np.nonzero(got != want)[0].tolist())
        v.set_lanes_per_proof(0)
        nb = cs[0][1]
        d_p = torch.from_numpy(np.frombuffer(b''.join(proofs), np.uint8).reshape(N, -1).copy()).to(dev)
        d_i = torch.from_numpy(np.frombuffer(b''.join(b''.join(p) for p in pubs) + b'\0', np.uint8)[:N * 32 * nb].copy()).to(dev)
        d_v = torch.full((N,), 255, dtype=torch.uint8, device=dev)
        v.verify_batch_dev(N, d_p.data_ptr(), d_i.data_ptr() if nb else 0, d_v.data_ptr())
        v.synchronize()
        assert np.array_equal(d_v.cpu().numpy(), want), cs[0][0]
        v.close()


@pytest.mark.parametrize('sub', [16, 64])
def test_plonk_aggregate_check(zkv, monkeypatch, sub):
    monkeypatch.setenv('ZKV_AGG_MIN', '64')
    for g, (vkb, cs) in enumerate(_plonk_groups()):
        v = zkv.PlonkVerifier(vkb)
        v.set_aggregate_check(True, seed=bytes(range(32)), sub_batch=sub)
        proofs, pubs, _ = _plonk_batch([c for c in cs if c[7]], 100 + g)
        got = v.verify_batch(proofs, pubs)
        assert got.all(), (cs[0][0], sub, np.nonzero(got == 0)[0].tolist())
        checked, failed = v.aggregate_counters()
        assert checked > 0 and failed == 0, (cs[0][0], sub, checked, failed)
        proofs, pubs, want = _plonk_batch(cs, 200 + g)
        got = v.verify_batch(proofs, pubs)
        assert np.array_equal(got, want), (cs[0][0], sub, np.nonzero(got != want)[0].tolist())
        v.close()


def test_plonk_key_set_mixes_degenerate_and_ordinary_keys(zkv):
    groups = _plonk_groups()
    ordinary = [D.ordinary_plonk_key(nb, nc) for nb, nc in ((2, 0), (3, 1))]
    keys = [vkb for vkb, _ in groups] + [T.vk_bytes(k) for k in ordinary]
    rng = random.Random(5)
    rows, queues = [], [list(cs) for _, cs in groups]
    while any(queues):
        for k, q in enumerate(queues):
            if q:
                c = q.pop(0)
                rows.append((k, c[5], c[6], c[7]))
            rows.append((len(groups) + k % 2,) + D.ordinary_plonk(keys[len(groups) + k % 2], rng) + (True,))
    s = zkv.PlonkVerifierSet(keys)
    got = s.verify_batch([r[0] for r in rows], [r[1] for r in rows], [[x.to_bytes(32, 'big') for x in r[2]] for r in rows])
    want = np.array([ol.plonk_verify(keys[k], T.pad27(p), [x.to_bytes(32, 'big') for x in pub]) for k, p, pub, _ in rows], dtype=np.uint8)
    assert np.array_equal(want, np.array([r[3] for r in rows], dtype=np.uint8))
    assert np.array_equal(got, want), np.nonzero(got != want)[0].tolist()
    s.close()


def test_sp1_plonk_verifier_and_gateway_route(zkv):
    """SP1 PLONK keys with degenerate points / proofs behind Sp1PlonkVerifier (every mapping) and behind an Sp1Gateway route each, beside
    the built-in Groth16 route: the oracle's statuses."""
    sp = D.sp1_plonk_cases()
    routes = []
    allrows = []
    for vkb, cs in sp.items():
        h = D.sp1_verifier_hash(vkb)
        routes.append((vkb, h))
        rng = random.Random(len(routes))
        vk = cs[0][1]
        rows = []
        for name, _, vkey, pv, proof, w in cs:            # each case beside ordinary proofs of the same key
            rows.append((name, vkey, pv, proof))
            pv2 = rng.randbytes(40)
            vk2 = (rng.randrange(m.R)).to_bytes(32, 'big')
            rows.append(('ordinary', vk2, pv2, h[:4] + T.forge(vk, [int.from_bytes(vk2, 'big'), m.sp1_hash_public_values(pv2)], rng)))
        want = [ol.sp1_plonk_verify_proof(vkb, h, r[1], r[2], r[3])[0] for r in rows]
        assert want == [0 if (r[0] == 'ordinary' or not r[0].endswith('sibling')) else 1 for r in rows], want
        v = zkv.Sp1PlonkVerifier(vkb, h)
        for lanes in (0, 2, 16, 64, 128):
            v.set_lanes_per_proof(lanes)
            st, _ = v.verify_batch([r[1] for r in rows], [r[2] for r in rows], [r[3] for r in rows])
            assert [int(x) for x in st] == want, (cs[0][0], lanes)
        v.close()
        allrows += [(r, w) for r, w in zip(rows, want)]
    gw = zkv.Sp1Gateway(True, routes)
    st, _ = gw.verify_batch([r[1] for r, _ in allrows], [r[2] for r, _ in allrows], [r[3] for r, _ in allrows])
    assert [int(x) for x in st] == [w for _, w in allrows]
    gw.close()

"""Ownership of device memory (csrc/zkv_devmem.h), counted by the library itself: zkv_diag_device_memory reads {live allocations,
live bytes} of this process.  Every case reads the count, creates a context of one family, makes one host-buffer call and one
device-resident call on a small batch (with the aggregate check switched on where the family has one, so that its buffers are reserved
too), sees the count above where it was, destroys the context and finds the count EXACTLY where it was.  The statuses of both calls are
checked against the expectations the family's own tests use (corpus statuses, the C oracle, the models of tests/): a library that
verified nothing would not pass by returning its memory.  Free-memory readings of the device move with other processes' work and
are not used."""
import ctypes as C
import hashlib
import json
import os
import random

import numpy as np
import pytest

import gateway_keys_model as gk
import oracle_lib as ol
import plonk_trapdoor_keys as T
import risc0_router_model as rm
import spec_model as m

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
H = bytes.fromhex


@pytest.fixture(scope='module')
def zkv():
    import stylus_zkvm_verifiers_amd as z
    assert z.device_count() >= 1, 'no gfx950 device visible'
    return z


def live(z):
    out = (C.c_uint64 * 2)()
    assert z._lib.lib().zkv_diag_device_memory(out) == 0
    return int(out[0]), int(out[1])


def up(a):
    """Bytes or an array as a device tensor of bytes (a writable copy), with a spare byte behind."""
    import torch
    b = a if isinstance(a, (bytes, bytearray)) else np.ascontiguousarray(a).tobytes()
    return torch.from_numpy(np.frombuffer(bytes(b) + b'\0', dtype=np.uint8).copy()).cuda()


def outs(n):
    import torch
    return torch.full((n,), 255, dtype=torch.uint8, device='cuda'), torch.full((n, 4), 255, dtype=torch.uint8, device='cuda')


def stream():
    import torch
    return torch.cuda.current_stream().cuda_stream


def done(*t):
    import torch
    torch.cuda.synchronize()
    return [x.cpu().numpy() for x in t]


def load(name):
    return json.load(open(os.path.join(HERE, 'golden', name)))


def risc0_rows(verify_corpus):
    """The corpus cases with a full-length seal (the device entry points take rows of 260 bytes): 29 of them, every status."""
    rows = [(H(c['seal']), H(c['image_id']), H(c['journal_digest']), c['status']) for c in verify_corpus['cases'] if c['vm'] == 'risc0' and len(c['seal']) == 520]
    assert 3 <= len(rows) <= 80 and {0, 1, 5} <= {r[3] for r in rows}
    return rows


def sp1_rows(verify_corpus):
    rows = [(H(c['vkey']), H(c['public_values']), H(c['proof']), c['status']) for c in verify_corpus['cases']
            if c['vm'] == 'sp1' and len(c['proof']) == 520 and len(c['public_values']) == 192]
    assert 3 <= len(rows) <= 80 and {0, 1, 5} <= {r[3] for r in rows}
    return rows


def new_risc0(z, real_proofs):
    r = real_proofs['risc0']
    v = z.RiscZeroVerifier(0)
    v.initialize(H(r['control_root']), H(r['bn254_control_id']))
    return v


# ---------------------------------------------------------------- the families: each returns the contexts it created, calls made and checked
def fam_risc0(z, real_proofs, verify_corpus, make=None):
    rows = risc0_rows(verify_corpus)
    n, want = len(rows), [r[3] for r in rows]
    v = make() if make else new_risc0(z, real_proofs)
    v.set_aggregate_check(True)
    st, _ = v.verify_batch([r[0] for r in rows], [r[1] for r in rows], [r[2] for r in rows])
    assert st.tolist() == want
    d = [up(b''.join(r[k] for r in rows)) for k in range(3)]
    d_st, d_rv = outs(n)
    v.verify_batch_dev(n, d[0].data_ptr(), d[1].data_ptr(), d[2].data_ptr(), d_st.data_ptr(), d_rv.data_ptr(), stream())
    assert done(d_st)[0].tolist() == want
    return [v]


def fam_risc0_sharded(z, real_proofs, verify_corpus):
    """Two shards on one device: the second takes the staged path of the device-resident call when asked to (ZKV_SHARD_FORCE_STAGING)."""
    return fam_risc0(z, real_proofs, verify_corpus, make=lambda: z.shard([new_risc0(z, real_proofs), new_risc0(z, real_proofs)]))


def fam_risc0_set(z, real_proofs, verify_corpus):
    r = real_proofs['risc0']
    rows = risc0_rows(verify_corpus)
    n, want = len(rows), [x[3] for x in rows]
    other = hashlib.sha256(b'device memory: another control root').digest()
    v = z.RiscZeroVerifierSet([H(r['control_root']), other], [H(r['bn254_control_id']), H(r['bn254_control_id'])])
    v.set_aggregate_check(True)
    inst = np.zeros(n, dtype=np.uint32)
    st, _ = v.verify_batch(inst, [x[0] for x in rows], [x[1] for x in rows], [x[2] for x in rows])
    assert st.tolist() == want
    d = [up(b''.join(x[k] for x in rows)) for k in range(3)]
    d_inst = up(inst)
    d_st, d_rv = outs(n)
    v.verify_batch_dev(n, d_inst.data_ptr(), d[0].data_ptr(), d[1].data_ptr(), d[2].data_ptr(), d_st.data_ptr(), d_rv.data_ptr(), stream())
    assert done(d_st)[0].tolist() == want
    return [v]


def _sp1_calls(v, rows):
    n, want = len(rows), [x[3] for x in rows]
    st, _ = v.verify_batch([x[0] for x in rows], [x[1] for x in rows], [x[2] for x in rows])
    assert st.tolist() == want
    d = [up(b''.join(x[k] for x in rows)) for k in range(3)]
    d_st, d_rv = outs(n)
    v.verify_batch_dev(n, d[0].data_ptr(), d[1].data_ptr(), len(rows[0][1]), d[2].data_ptr(), d_st.data_ptr(), d_rv.data_ptr(), stream())
    assert done(d_st)[0].tolist() == want


def fam_sp1(z, real_proofs, verify_corpus):
    v = z.Sp1Verifier(0)
    v.set_aggregate_check(True)
    _sp1_calls(v, sp1_rows(verify_corpus))
    return [v]


def fam_sp1_plonk(z, real_proofs, verify_corpus):
    pk = load('plonk_cases.json')
    rows = [(H(c['vkey']), H(c['public_values']), H(c['proof']), c['status']) for c in pk['cases'] if len(c['public_values']) == 192 and len(c['proof']) == 1736]
    assert 3 <= len(rows) <= 80 and {0, 1, 5} <= {x[3] for x in rows}
    v = z.Sp1PlonkVerifier(H(pk['vk']), H(pk['verifier_hash']), 0)
    v.set_aggregate_check(True)
    _sp1_calls(v, rows)
    return [v]


def _plonk_pool(nb, nc, n):
    """n proofs of the fixture pool's key of shape (nb public inputs, nc commitments), every third one damaged (the claimed l(zeta))."""
    e = next(e for e in load('plonk_keys_cases.json')['pool'] if (e['nb_public'], e['n_c']) == (nb, nc))
    vk, P, Q = T.pool_arrays(e)
    idx = np.arange(n) % len(P)
    proofs, pub = P[idx].copy(), Q[idx].copy()
    want = np.ones(n, np.uint8)
    want[2::3] = 0
    proofs[2::3, 12 * 32 + 31] ^= 1
    return vk, proofs, pub, want


def fam_plonk_key(z, real_proofs, verify_corpus):
    from stylus_zkvm_verifiers_amd import plonk_keys
    vk, proofs, pub, want = _plonk_pool(2, 1, 12)
    v = plonk_keys.PlonkVerifier(vk)
    v.set_aggregate_check(True)
    assert np.asarray(v.verify_batch(proofs, pub)).astype(np.uint8).tolist() == want.tolist()
    d_p, d_i = up(proofs), up(pub)
    d_v, _ = outs(len(want))
    v.verify_batch_dev(len(want), d_p.data_ptr(), d_i.data_ptr(), d_v.data_ptr())
    v.synchronize()
    assert done(d_v)[0].tolist() == want.tolist()
    return [v]


def _groth16_batch(n_ic, vm, n, seed):
    """n re-randomisations of one trapdoor proof under a fresh key of n_ic IC points, every fifth one mutated: (key words, proofs, signals,
    expected verdicts) -- the construction of tests/test_groth16_long_keys.py, a sample of it checked against the C oracle."""
    from stylus_zkvm_verifiers_amd import synth
    rng = random.Random(seed)
    vk, td = m.trapdoor_vk(rng, n_ic)
    vkb = m.vk_to_words(vk)
    sig = [rng.randrange(m.R) for _ in range(n_ic - 1)]
    base = m.proof_to_words(*m.trapdoor_prove(rng, td, sig, vm))
    proofs, sigs, mutated, _ = synth.make_groth16_batch(vkb, vm, base, sig, n, seed=seed, mutate_every=5)
    assert 0 < mutated.sum() < n
    for i in (0, 4, n - 1):
        assert ol.groth16_verify_vk({'risc0': 0, 'sp1': 1}[vm], vkb, n_ic, proofs[i].tobytes(), [sigs[i, j].tobytes() for j in range(n_ic - 1)]) == (not mutated[i])
    return vkb, proofs, sigs, (~mutated).astype(np.uint8)


def _fam_groth16(z, n_ic):
    vkb, proofs, sigs, want = _groth16_batch(n_ic, 'sp1', 24, 100 + n_ic)
    v = z.Groth16Verifier(vkb, n_ic, z.errors.VM_SP1)
    v.set_aggregate_check(True)                            # (a long key takes no aggregate check: the switch is accepted, its chunks run per proof)
    assert np.asarray(v.verify_batch(proofs, sigs)).astype(np.uint8).tolist() == want.tolist()
    d_p, d_s = up(proofs), up(sigs)
    d_v, _ = outs(len(want))
    v.verify_batch_dev(len(want), d_p.data_ptr(), d_s.data_ptr(), d_v.data_ptr())
    v.synchronize()
    assert done(d_v)[0].tolist() == want.tolist()
    return [v]


def fam_groth16_short_key(z, real_proofs, verify_corpus):
    return _fam_groth16(z, 3)


def fam_groth16_long_key(z, real_proofs, verify_corpus):
    return _fam_groth16(z, 17)


def fam_groth16_key_set(z, real_proofs, verify_corpus):
    parts = [_groth16_batch(3, 'sp1', 12, 201), _groth16_batch(7, 'risc0', 12, 202)]
    s = z.Groth16VerifierSet([(parts[0][0], 3, 1), (parts[1][0], 7, 0)])
    s.set_aggregate_check(True)
    stride = s.signal_stride() // 32
    assert stride == 6
    n = 24
    kk = np.array([i % 2 for i in range(n)], dtype=np.uint32)
    proofs = np.zeros((n, 256), np.uint8); sigs = np.zeros((n, stride, 32), np.uint8); want = np.zeros(n, np.uint8)
    for i in range(n):
        _, P, S, W = parts[i % 2]
        proofs[i] = P[i // 2]; sigs[i, :S.shape[1]] = S[i // 2]; want[i] = W[i // 2]
    assert np.asarray(s.verify_batch(kk, proofs, sigs)).astype(np.uint8).tolist() == want.tolist()
    d_k, d_p, d_s = up(kk), up(proofs), up(sigs)
    d_v, _ = outs(n)
    s.verify_batch_dev(n, d_k.data_ptr(), d_p.data_ptr(), d_s.data_ptr(), d_v.data_ptr())
    s.synchronize()
    assert done(d_v)[0].tolist() == want.tolist()
    return [s]


def fam_plonk_key_set(z, real_proofs, verify_corpus):
    from stylus_zkvm_verifiers_amd import plonk_set
    parts = [_plonk_pool(2, 1, 12), _plonk_pool(9, 0, 12)]
    s = plonk_set.PlonkVerifierSet([parts[0][0], parts[1][0]])
    s.set_aggregate_check(True)
    ps, ins = s.proof_stride(), s.input_stride()
    n = 24
    kk = np.array([i % 2 for i in range(n)], dtype=np.uint32)
    proofs = np.zeros((n, ps), np.uint8); pub = np.zeros((n, ins // 32, 32), np.uint8); want = np.zeros(n, np.uint8)
    for i in range(n):
        _, P, Q, W = parts[i % 2]
        proofs[i, :P.shape[1]] = P[i // 2]; pub[i, :Q.shape[1]] = Q[i // 2]; want[i] = W[i // 2]
    assert np.asarray(s.verify_batch(kk, proofs, pub)).astype(np.uint8).tolist() == want.tolist()
    d_k, d_p, d_i = up(kk), up(proofs), up(pub)
    d_v, _ = outs(n)
    s.verify_batch_dev(n, d_k.data_ptr(), d_p.data_ptr(), d_i.data_ptr(), d_v.data_ptr())
    s.synchronize()
    assert done(d_v)[0].tolist() == want.tolist()
    return [s]


def fam_mixed(z, real_proofs, verify_corpus):
    r = real_proofs['risc0']
    r0, s1 = risc0_rows(verify_corpus)[:20], sp1_rows(verify_corpus)[:20]
    vm = [0] * len(r0) + [1] * len(s1)
    order = list(range(len(vm)))
    random.Random(5).shuffle(order)
    rows = r0 + s1
    vm, rows = [vm[i] for i in order], [rows[i] for i in order]
    n, want = len(rows), [x[3] for x in rows]
    mx = z.MixedVerifier(H(r['control_root']), H(r['bn254_control_id']), 0)
    mx.set_aggregate_check(True)
    # (RISC Zero: seal, image id, journal digest; SP1: proof, vkey, public values)
    seals = [x[0] if t == 0 else x[2] for t, x in zip(vm, rows)]
    in_a = [x[1] if t == 0 else x[0] for t, x in zip(vm, rows)]
    in_b = [x[2] if t == 0 else x[1] for t, x in zip(vm, rows)]
    st, _ = mx.verify_batch(vm, seals, in_a, in_b)
    assert st.tolist() == want
    d_vm, d_s, d_a = up(np.array(vm, dtype=np.uint8)), up(b''.join(seals)), up(b''.join(in_a))
    d_b = up(b''.join(x.ljust(96, b'\0') for x in in_b))
    d_st, d_rv = outs(n)
    mx.verify_batch_dev(n, d_vm.data_ptr(), d_s.data_ptr(), d_a.data_ptr(), d_b.data_ptr(), 96, 96, d_st.data_ptr(), d_rv.data_ptr(), stream())
    assert done(d_st)[0].tolist() == want
    return [mx]


def fam_sp1_gateway_keyed(z, real_proofs, verify_corpus):
    """The built-in Groth16 route and a keyed route (a trapdoor key of tests/gateway_keys_model.py) in one batch: corpus statuses on the
    first (no route instead of a selector mismatch), the model's on the second; then the eth_call entry points on the same rows as
    calldata."""
    key = gk.Key(0xD3A1)
    gw = z.Sp1Gateway(True, groth16_keys=[(key.words, key.hash)])
    gw.set_aggregate_check(True)
    rows = [(x[0], x[1], x[2], 8 if x[3] == 5 else x[3]) for x in sp1_rows(verify_corpus)]
    vkey, pv = rows[0][0], rows[0][1]
    for j in range(6):
        p = key.prove(vkey, pv)
        if j % 3 == 2:
            p = p[:-1] + bytes([p[-1] ^ 1])
        rows.insert(3 * j, (vkey, pv, p, key.verify(vkey, pv, p)[0]))
    n, want = len(rows), [x[3] for x in rows]
    assert want.count(0) >= 5 and 8 in want
    st, _ = gw.verify_batch([x[0] for x in rows], [x[1] for x in rows], [x[2] for x in rows])
    assert st.tolist() == want
    off = np.arange(n + 1, dtype=np.uint64) * 260
    d_vk, d_pv, d_p, d_off = up(b''.join(x[0] for x in rows)), up(b''.join(x[1] for x in rows)), up(b''.join(x[2] for x in rows)), up(off)
    d_st, d_rv = outs(n)
    gw.verify_batch_dev(n, d_vk.data_ptr(), d_pv.data_ptr(), 96, d_p.data_ptr(), d_off.data_ptr(), int(off[-1]), d_st.data_ptr(), d_rv.data_ptr(), stream())
    assert done(d_st)[0].tolist() == want
    calls = [gw.encode_verify_proof_call(*x[:3]) for x in rows]
    rev, _, st = gw.eth_call_batch(calls)
    assert st.tolist() == want and rev.tolist() == [int(w != 0) for w in want]
    off = np.zeros(n + 1, dtype=np.uint64); off[1:] = np.cumsum([len(c) for c in calls])
    d_cd, d_off = up(b''.join(calls)), up(off)
    d_st, d_rv = outs(n)
    gw.eth_call_batch_dev(n, d_cd.data_ptr(), d_off.data_ptr(), int(off[-1]), d_st.data_ptr(), d_rv.data_ptr(), stream())
    assert done(d_st)[0].tolist() == want
    return [gw]


def fam_risc0_router_keyed(z, real_proofs, verify_corpus):
    """A built-in route and a keyed route (tests/risc0_router_model.py), through verify_batch / verify_batch_dev and through the eth_call
    entry points on the same seals as calldata: the model's statuses everywhere."""
    r = real_proofs['risc0']
    key = rm.Key(0xD3A2)
    builtin = [(H(r['control_root']), H(r['bn254_control_id']))]
    rt = z.RiscZeroRouter(builtin, [key.triple()])
    rt.set_aggregate_check(True)
    rows = [x[:3] for x in risc0_rows(verify_corpus)]
    iid, jd = rows[0][1], rows[0][2]
    for j in range(6):
        s = key.prove(iid, jd)
        if j % 3 == 2:
            s = s[:-1] + bytes([s[-1] ^ 1])
        rows.insert(3 * j, (s, iid, jd))
    n = len(rows)
    seals, ids, jds = [x[0] for x in rows], [x[1] for x in rows], [x[2] for x in rows]
    want = rm.Router(builtin, [key.triple()]).expect(seals, ids, jds)[0].tolist()
    assert want.count(0) >= 5 and 8 in want and 1 in want
    st, _ = rt.verify_batch(seals, ids, jds)
    assert st.tolist() == want
    d = [up(b''.join(x)) for x in (seals, ids, jds)]
    d_st, d_rv = outs(n)
    rt.verify_batch_dev(n, d[0].data_ptr(), d[1].data_ptr(), d[2].data_ptr(), d_st.data_ptr(), d_rv.data_ptr(), stream())
    assert done(d_st)[0].tolist() == want
    calls = [rt.encode_verify_call(*x) for x in rows]
    rev, _, st = rt.eth_call_batch(calls)
    assert st.tolist() == want and rev.tolist() == [int(w != 0) for w in want]
    off = np.zeros(n + 1, dtype=np.uint64); off[1:] = np.cumsum([len(c) for c in calls])
    d_cd, d_off = up(b''.join(calls)), up(off)
    d_st, d_rv = outs(n)
    rt.eth_call_batch_dev(n, d_cd.data_ptr(), d_off.data_ptr(), int(off[-1]), d_st.data_ptr(), d_rv.data_ptr(), 0, stream())
    assert done(d_st)[0].tolist() == want
    return [rt]


def fam_risc0_router_set(z, real_proofs, verify_corpus):
    """A router with a set route on the first seals of tests/golden/risc0_router_set_cases.json -- Groth16 seals of every route, set seals
    whose root seals the keyed routes verify, malformed ones -- through verify_batch and verify_ragged_dev: the fixture's statuses (those
    of tests/risc0_router_set_model.py), and root jobs were run, so their rows are held too."""
    rs = load('risc0_router_set_cases.json')
    rt = z.RiscZeroSetRouter(H(rs['set_id']), [(H(rs['builtin']['control_root']), H(rs['builtin']['bn254_control_id']))],
                             [(H(k['vk_words']), H(k['control_root']), H(k['bn254_control_id'])) for k in rs['keyed']])
    rt.set_aggregate_check(True)
    for x in rs['submitted_roots']:
        assert rt.submit_root(H(x['root']), H(x['seal']))[0] == 0
    cases = rs['cases'][:48]
    n, want = len(cases), [c['status'] for c in cases]
    seals, ids, jds = [H(c['seal']) for c in cases], [H(c['image_id']) for c in cases], [H(c['journal_digest']) for c in cases]
    assert {0, 1, 4, 8} <= set(want)
    st, _ = rt.verify_batch(seals, ids, jds)
    assert st.tolist() == want and rt.set_last_counts()[2] >= 1
    off = np.zeros(n + 1, dtype=np.uint64); off[1:] = np.cumsum([len(s) for s in seals])
    d_s, d_off, d_a, d_b = up(b''.join(seals)), up(off), up(b''.join(ids)), up(b''.join(jds))
    d_st, d_rv = outs(n)
    rt.verify_ragged_dev(n, d_s.data_ptr(), d_off.data_ptr(), int(off[-1]), d_a.data_ptr(), d_b.data_ptr(), d_st.data_ptr(), d_rv.data_ptr(), stream())
    assert done(d_st)[0].tolist() == want and rt.set_last_counts()[2] >= 1
    return [rt]


def fam_set_inclusion(z, real_proofs, verify_corpus):
    si = load('set_inclusion_cases.json')
    k = si['keyed']
    v = z.RiscZeroSetInclusionVerifier(H(k['control_root']), H(k['bn254_control_id']), H(si['set_builder_image_id']), vk_words=H(k['vk_words']),
                                       root_selector=H(k['root_selector']))
    claims = k['claims'][:32]
    seals = [H(x) for x in k['root_seals']]
    n, want = len(claims), [c['status'] for c in claims]
    assert 0 in want and 1 in want
    st, _ = v.verify_batch([H(c['image_id']) for c in claims], [H(c['journal_digest']) for c in claims], [H(c['path']) for c in claims],
                           [c['root_idx'] for c in claims], seals)
    assert st.tolist() == want
    # the device-resident call takes root seals as rows of 260 bytes: the claims behind the seals of that length, renumbered
    full = [j for j, s in enumerate(seals) if len(s) == 260]
    claims = [dict(c, root_idx=full.index(c['root_idx'])) for c in claims if c['root_idx'] in full]
    seals = [seals[j] for j in full]
    n, want = len(claims), [c['status'] for c in claims]
    assert n >= 3 and 0 in want and 1 in want
    off = np.zeros(n + 1, dtype=np.uint32); off[1:] = np.cumsum([len(c['path']) // 64 for c in claims])
    d_a, d_b = up(b''.join(H(c['image_id']) for c in claims)), up(b''.join(H(c['journal_digest']) for c in claims))
    d_blob, d_off = up(b''.join(H(c['path']) for c in claims) + bytes(64)), up(off)
    d_idx, d_seals = up(np.array([c['root_idx'] for c in claims], dtype=np.uint32)), up(b''.join(seals) + bytes(4))
    d_st, d_rv = outs(n)
    v.verify_batch_dev(n, d_a.data_ptr(), d_b.data_ptr(), d_blob.data_ptr(), d_off.data_ptr(), int(off[-1]), d_idx.data_ptr(), len(seals), d_seals.data_ptr(),
                       d_st.data_ptr(), d_rv.data_ptr(), stream())
    v.synchronize()
    assert done(d_st)[0].tolist() == want
    return [v]


def fam_bn254_precompiles(z, real_proofs, verify_corpus):
    rng = random.Random(9)
    g = lambda: m.be32(1) + m.be32(2)
    adds = [g() + g(), g() + bytes(64), bytes(128), g() + m.be32(1) + m.be32(3)] + [m.be32(rng.randrange(m.P)) * 4 for _ in range(4)]
    pc = z.Bn254Precompiles()
    assert pc.ecadd(adds) == [ol.ecadd(a) for a in adds] and pc.ecadd(adds)[0] is not None and pc.ecadd(adds)[3] is None
    r = real_proofs['risc0']
    seal = H(r['seal'])
    w = [seal[4 + 32 * i:36 + 32 * i] for i in range(8)]
    ax, ay = m.negate_g1_words(int.from_bytes(w[0], 'big'), int.from_bytes(w[1], 'big'))
    vk = m.RISC0_VK
    g2 = lambda q: b''.join(m.be32(v) for v in (q[0][0], q[0][1], q[1][0], q[1][1]))
    data = (m.be32(ax) + m.be32(ay) + b''.join(w[2:6]) + m.be32(vk['alpha1'][0]) + m.be32(vk['alpha1'][1]) + g2(vk['beta2'])
            + H(r['vk_x'][0]) + H(r['vk_x'][1]) + g2(vk['gamma2']) + w[6] + w[7] + g2(vk['delta2']))
    bad = bytearray(data); bad[100] ^= 1
    calls = [data, bytes(bad), bytes(64) + data[64:], data]
    want = [(lambda x: None if x is None else bool(x[-1]))(ol.ecpairing(x)) for x in calls]
    assert want[0] is True and want[3] is True and want[1] is None
    n = len(calls)
    d_in = up(b''.join(calls))
    d_res, _ = outs(n); d_ok, _ = outs(n)
    pc.pairing_dev(n, 4, d_in.data_ptr(), d_res.data_ptr(), d_ok.data_ptr(), stream())
    res, ok = done(d_res, d_ok)
    assert [bool(res[i]) if ok[i] else None for i in range(n)] == want
    return [pc]


def _fam_sp1_lane_pairs(z, real_proofs, built):
    """80 proofs with lane pairs forced (make_sp1 of tests/test_gt_tables_gpu.py): the GT tables and the walk cache are built, or refused."""
    from stylus_zkvm_verifiers_amd import diag_gt
    s = real_proofs['sp1']
    good = (H(s['vkey']), H(s['public_values']), H(s['proof']), 0)
    bad = (H(s['vkey']), H(s['public_values'])[:-1] + bytes([H(s['public_values'])[-1] ^ 1]), H(s['proof']), 1)
    rows = [good if i % 5 else bad for i in range(80)]
    assert [ol.sp1_verify_proof(*x[:3])[0] for x in (good, bad)] == [0, 1]
    v = z.Sp1Verifier(0)
    v.set_lanes_per_proof(2)
    _sp1_calls(v, rows)
    info = diag_gt.info(v._h)
    assert bool(info['built']) == built and info['tried']
    return [v]


def fam_sp1_gt_tables(z, real_proofs, verify_corpus):
    return _fam_sp1_lane_pairs(z, real_proofs, True)


def fam_sp1_gt_tables_refused(z, real_proofs, verify_corpus):
    return _fam_sp1_lane_pairs(z, real_proofs, False)


FAMILIES = {f.__name__[4:]: f for f in (fam_risc0, fam_risc0_set, fam_sp1, fam_sp1_plonk, fam_plonk_key, fam_groth16_short_key, fam_groth16_long_key,
                                         fam_groth16_key_set, fam_plonk_key_set, fam_mixed, fam_sp1_gateway_keyed, fam_risc0_router_keyed,
                                         fam_risc0_router_set, fam_set_inclusion, fam_bn254_precompiles, fam_risc0_sharded, fam_sp1_gt_tables, fam_sp1_gt_tables_refused)}


def cycle(z, name, real_proofs, verify_corpus):
    """One create / call / destroy round of a family: (count before, count while the context lives, count after)."""
    before = live(z)
    ctxs = FAMILIES[name](z, real_proofs, verify_corpus)
    during = live(z)
    for c in ctxs:
        c.close()
    return before, during, live(z)


@pytest.mark.parametrize('name', sorted(FAMILIES))
def test_context_returns_what_it_took(zkv, monkeypatch, real_proofs, verify_corpus, name):
    if name == 'sp1_gt_tables_refused':
        monkeypatch.setenv('ZKV_GT_MAX_BYTES', '1')
    if name == 'risc0_sharded':
        monkeypatch.setenv('ZKV_SHARD_FORCE_STAGING', '1')
    before, during, after = cycle(zkv, name, real_proofs, verify_corpus)
    print(name, 'allocations / bytes before, during, after:', before, during, after)
    assert during[0] > before[0] and during[1] > before[1]
    assert after == before


def test_three_rounds_leave_the_same_count(zkv, real_proofs, verify_corpus):
    ends = [cycle(zkv, 'risc0_router_keyed', real_proofs, verify_corpus)[2] for _ in range(3)]
    assert ends[0] == ends[2] == ends[1]

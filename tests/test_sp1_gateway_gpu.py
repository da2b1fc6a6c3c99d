"""SP1 gateway on the GPU (include/zkv_sp1_gateway.h): statuses and received selectors of every proof equal the
oracle of the route its selector picks (oracle_lib's SP1 Groth16 and PLONK verifiers) or the routing rule (tests/gateway_model.py),
through the host, device-resident and single-proof entry points; at scale they equal the per-route contexts' own device calls.
Parity unpinned for ROUTE_NOT_FOUND and everything PLONK (no gateway or PLONK code in the reference)."""
import ctypes as C
import hashlib
import json
import os
import random

import numpy as np
import pytest

import gateway_model as gm
import oracle_lib as ol

HERE = os.path.dirname(os.path.abspath(__file__))
H = bytes.fromhex
RISC0_SELECTOR = None        # filled from the real RISC Zero seal


@pytest.fixture(scope='module')
def zkv():
    import stylus_zkvm_verifiers_amd as z
    assert z.device_count() >= 1, 'no gfx950 device visible'
    return z


@pytest.fixture(scope='module')
def keys():
    """(vk, verifier hash) of the golden PLONK key and of a second trapdoor key (oracle/plonk_model.ToyCircuit, fixed seed), and a prover
    for the second key."""
    import plonk_model as pm
    import spec_model as m
    d = json.load(open(os.path.join(HERE, 'golden', 'plonk_cases.json')))
    circ = pm.ToyCircuit(random.Random(0x6A7E5EED))
    vh2 = b'\x5e\xc0\x4d\x02' + hashlib.sha256(b'second toy PLONK key').digest()[:28]

    def prove2(vkey, pv, tamper=None):
        return vh2[:4] + circ.prove(int.from_bytes(vkey, 'big'), m.sp1_hash_public_values(pv), tamper=tamper)
    return (H(d['vk']), H(d['verifier_hash'])), (pm.vk_bytes(circ.vk), vh2), prove2


def _oracle(route, keys, vkey, pv, proof):
    if route == 0:
        st, rv = ol.sp1_verify_proof(vkey, pv, proof)
    else:
        vk, vh = keys[route - 1]
        st, rv = ol.sp1_plonk_verify_proof(vk, vh, vkey, pv, proof)
    return st, bytes(rv or bytes(4))


def _dev_call(zkv, gw, vkeys, pvs, proofs, recv=True):
    """Device-resident call on one batch whose public values share one length."""
    import torch
    dev = torch.device('cuda', 0)
    n = len(proofs)
    lens = [len(p) for p in proofs]
    off = np.zeros(n + 1, dtype=np.uint64); off[1:] = np.cumsum(lens)
    blob = np.frombuffer(b''.join(proofs) + b'\0', dtype=np.uint8)
    pv_len = len(pvs[0])
    d_vk = torch.from_numpy(np.frombuffer(b''.join(vkeys), dtype=np.uint8).copy()).to(dev)
    d_pv = torch.from_numpy(np.frombuffer(b''.join(pvs) + b'\0', dtype=np.uint8).copy()).to(dev)
    d_p = torch.from_numpy(blob.copy()).to(dev)
    d_off = torch.from_numpy(off.view(np.int64).copy()).to(dev)
    d_st = torch.full((n,), 255, dtype=torch.uint8, device=dev)
    d_rv = torch.full((n, 4), 255, dtype=torch.uint8, device=dev)
    gw.verify_batch_dev(n, d_vk.data_ptr(), d_pv.data_ptr(), pv_len, d_p.data_ptr(), d_off.data_ptr(), int(off[-1]), d_st.data_ptr(),
                        d_rv.data_ptr() if recv else 0, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return d_st.cpu().numpy(), d_rv.cpu().numpy()


def _case_batch(keys, real, corpus):
    (vk1, vh1), (vk2, vh2), prove2 = keys
    d = json.load(open(os.path.join(HERE, 'golden', 'plonk_cases.json')))
    s = real['sp1']
    items = [(H(c['vkey']), H(c['public_values']), H(c['proof'])) for c in d['cases']]
    items += [(H(c['vkey']), H(c['public_values']), H(c['proof'])) for c in corpus['cases'] if c['vm'] == 'sp1']
    sp1 = (H(s['vkey']), H(s['public_values']), H(s['proof']))
    items.append(sp1)
    rng = random.Random(0x6A7E)
    for k in range(4):
        items.append((sp1[0], sp1[1], sp1[2][:k]))                                  # 0 .. 3 bytes
    for k in range(6):                                                              # unknown selectors, Groth16 and PLONK lengths
        items.append((sp1[0], sp1[1], bytes(rng.randrange(256) for _ in range(4)) + (sp1[2][4:] if k % 2 else items[0][2][4:])))
    items.append((sp1[0], sp1[1], H(real['risc0']['seal'])))                        # the RISC Zero selector
    items.append((sp1[0], sp1[1], vh1[:4] + sp1[2][4:]))                            # a Groth16 proof under a PLONK route's selector
    items.append((sp1[0], sp1[1], vh2[:4] + sp1[2][4:]))
    plonk_ok = next(c for c in d['cases'] if c['status'] == 0)
    items.append((H(plonk_ok['vkey']), H(plonk_ok['public_values']), vh2[:4] + H(plonk_ok['proof'])[4:]))    # PLONK proof, second route's selector
    items.append((H(plonk_ok['vkey']), H(plonk_ok['public_values']), b'\xa4\x59\x4c\x59' + H(plonk_ok['proof'])[4:]))   # ... the Groth16 selector
    for k in range(3):                                                              # proofs of the second key, one tampered
        vkey = int(rng.randrange(1 << 250)).to_bytes(32, 'big')
        pv = bytes(rng.randrange(256) for _ in range(96))
        items.append((vkey, pv, prove2(vkey, pv, tamper='o5' if k == 2 else None)))
    items.append((items[-2][0], items[-2][1][:-1] + b'\x00', items[-2][2]))          # second key, wrong public values
    rng.shuffle(items)
    return items


@pytest.mark.gpu
def test_case_parity_through_every_entry_point(zkv, keys, real_proofs, verify_corpus):
    (vk1, vh1), (vk2, vh2), _ = keys
    items = _case_batch(keys, real_proofs, verify_corpus)
    gw = zkv.Sp1Gateway(True, [(vk1, vh1), (vk2, vh2)])
    sels = [r[0] for r in gw.routes()]
    assert sels[0] == b'\xa4\x59\x4c\x59'
    proofs = [p for _, _, p in items]
    off = np.zeros(len(items) + 1, dtype=np.uint64); off[1:] = np.cumsum([len(p) for p in proofs])
    blob = np.frombuffer(b''.join(proofs) + b'\0', dtype=np.uint8)
    route = gm.routes(blob, off, sels)
    assert {0, 1, 2, gm.NOT_FOUND, gm.SHORT} <= set(route.tolist())
    want_st, want_rv = [], []
    for (vkey, pv, proof), r in zip(items, route):
        if r >= 0:
            st, rv = _oracle(int(r), [(vk1, vh1), (vk2, vh2)], vkey, pv, proof)
        elif r == gm.NOT_FOUND:
            st, rv = 8, proof[:4]
        else:
            st, rv = 4, bytes(4)
        want_st.append(st); want_rv.append(rv)
    want_st = np.array(want_st, dtype=np.uint8)
    assert {0, 1, 4, 8} <= set(want_st.tolist())
    assert want_st[[i for i, (_, _, p) in enumerate(items) if p[:4] == vh2[:4] and len(p) == 260]].tolist() == [4]     # spliced Groth16: PLONK's length check
    # host buffers
    st, rv = gw.verify_batch([v for v, _, _ in items], [w for _, w, _ in items], proofs)
    assert st.tolist() == want_st.tolist() and [bytes(x) for x in rv] == want_rv
    assert gw.last_route_counts() == gm.counts(route, 3)
    assert sum(gw.last_stage_ms()) > 0
    # device-resident, one call per public-values length (fixed stride); one call without received selectors
    for L_ in sorted({len(w) for _, w, _ in items}):
        idx = [i for i, (_, w, _) in enumerate(items) if len(w) == L_]
        dst, drv = _dev_call(zkv, gw, [items[i][0] for i in idx], [items[i][1] for i in idx], [items[i][2] for i in idx])
        assert dst.tolist() == want_st[idx].tolist(), L_
        assert [bytes(x) for x in drv] == [want_rv[i] for i in idx], L_
        sub = gm.routes(np.frombuffer(b''.join(items[i][2] for i in idx) + b'\0', np.uint8),
                        np.concatenate([[0], np.cumsum([len(items[i][2]) for i in idx])]).astype(np.uint64), sels)
        assert gw.last_route_counts() == gm.counts(sub, 3)
    idx = [i for i, (_, w, _) in enumerate(items) if len(w) == 96]
    dst, _ = _dev_call(zkv, gw, [items[i][0] for i in idx], [items[i][1] for i in idx], [items[i][2] for i in idx], recv=False)
    assert dst.tolist() == want_st[idx].tolist()
    # single proofs, routed on the host
    L = gw._L
    for (vkey, pv, proof), ws, wr in zip(items, want_st, want_rv):
        s = C.c_uint8(255); r = C.create_string_buffer(4)
        assert L.zkv_sp1_gateway_verify_proof(gw._h, vkey, pv, len(pv), proof, len(proof), C.byref(s), r) == 0
        assert (s.value, r.raw) == (int(ws), wr)
    real = real_proofs['sp1']
    assert gw.verify_proof(H(real['vkey']), H(real['public_values']), H(real['proof'])) is None
    gw.close()


@pytest.mark.gpu
def test_without_the_groth16_route_sp1_groth16_proofs_find_no_route(zkv, keys, real_proofs, verify_corpus):
    (vk1, vh1), _, _ = keys
    gw = zkv.Sp1Gateway(False, [(vk1, vh1)])
    cases = [c for c in verify_corpus['cases'] if c['vm'] == 'sp1'] + [dict(vkey=real_proofs['sp1']['vkey'], public_values=real_proofs['sp1']['public_values'],
                                                                            proof=real_proofs['sp1']['proof'])]
    proofs = [H(c['proof']) for c in cases]
    st, rv = gw.verify_batch([H(c['vkey']) for c in cases], [H(c['public_values']) for c in cases], proofs)
    for p, s, r in zip(proofs, st, rv):
        if len(p) < 4:
            assert int(s) == 4 and bytes(r) == bytes(4)
        elif p[:4] == vh1[:4]:
            continue
        else:
            assert int(s) == 8 and bytes(r) == p[:4], p[:8].hex()
    assert int(st[-1]) == 8 and bytes(rv[-1]) == b'\xa4\x59\x4c\x59'
    with pytest.raises(zkv.VerifierError) as ei:
        gw.verify_proof(H(real_proofs['sp1']['vkey']), H(real_proofs['sp1']['public_values']), H(real_proofs['sp1']['proof']))
    assert ei.value.status == 8
    gw.close()


def _pools(keys, real, n_g=1024):
    """Groth16 pool (re-randomised real SP1 proof, 1 in 64 damaged), golden PLONK pool (key 1), a few model proofs of key 2."""
    from stylus_zkvm_verifiers_amd import synth
    (vk1, vh1), (vk2, vh2), prove2 = keys
    s = real['sp1']
    seals, _, _, flip = synth.make_batch('sp1', H(s['proof']), n_g, 0x6A7E01)
    pv = np.tile(np.frombuffer(H(s['public_values']), np.uint8), (n_g, 1))
    pv[flip, -1] ^= 1
    g = (seals, np.tile(np.frombuffer(H(s['vkey']), np.uint8), (n_g, 1)), pv)
    pool = json.load(open(os.path.join(HERE, 'golden', 'plonk_pool.json')))
    rows = [(H(p['proof']), H(p['vkey']), H(p['public_values'])) for p in pool['proofs']]
    rng = random.Random(0x6A7E02)
    for k in range(4):
        vkey = int(rng.randrange(1 << 250)).to_bytes(32, 'big')
        pvb = bytes(rng.randrange(256) for _ in range(96))
        rows.append((prove2(vkey, pvb, tamper='o5' if k == 3 else None), vkey, pvb))
    p = tuple(np.stack([np.frombuffer(r[j], np.uint8) for r in rows]) for j in range(3))
    p[0][5, 4 + 32 * 3 + 31] ^= 1                                                    # one damaged key-1 proof
    return g, p


def _reference(zkv, refs, blob, off, vkeys, pvs, route):
    """Every route's own context, device-resident, on its proofs sorted on the host."""
    import torch
    dev = torch.device('cuda', 0)
    per = []
    for r, idx in enumerate(gm.partition(route, len(refs))):
        m = len(idx)
        if not m:
            per.append((np.zeros(0, np.uint8), np.zeros((0, 4), np.uint8)))
            continue
        L = int(off[idx[0] + 1] - off[idx[0]])
        P = np.stack([blob[int(off[i]):int(off[i]) + L] for i in idx])
        d = [torch.from_numpy(np.ascontiguousarray(x)).to(dev) for x in (vkeys[idx], pvs[idx], P)]
        d_st = torch.full((m,), 255, dtype=torch.uint8, device=dev); d_rv = torch.full((m, 4), 255, dtype=torch.uint8, device=dev)
        refs[r].verify_batch_dev(m, d[0].data_ptr(), d[1].data_ptr(), pvs.shape[1], d[2].data_ptr(), d_st.data_ptr(), d_rv.data_ptr(),
                                 torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        per.append((d_st.cpu().numpy(), d_rv.cpu().numpy()))
    return gm.expected(route, blob, off, per)


@pytest.mark.gpu
def test_scale_against_per_route_contexts(zkv, keys, real_proofs):
    (vk1, vh1), (vk2, vh2), _ = keys
    from stylus_zkvm_verifiers_amd import synth
    g, p = _pools(keys, real_proofs)
    gw = zkv.Sp1Gateway(True, [(vk1, vh1), (vk2, vh2)])
    refs = [zkv.Sp1Verifier(), zkv.Sp1PlonkVerifier(vk1, vh1), zkv.Sp1PlonkVerifier(vk2, vh2)]
    sels = [r[0] for r in gw.routes()]
    rng = np.random.default_rng(0x6A7E03)
    for n in (1, 63, 4096, 70000, 1 << 17):
        frac = float(rng.random())
        blob, off, vkeys, pvs, kind, row, spliced = synth.make_sp1_gateway_batch(
            g, p, n, frac, int(rng.integers(1 << 30)), splice_every=97, splice_selectors=[b'\x50\x45\xf5\x26', b'\x00\x00\x00\x00', b'\xff\xff\xff\xff'])
        # about half the PLONK proofs carry the second key's selector (a key-1 proof there fails; key-2 rows are valid there)
        p_idx = np.nonzero((kind == 1) & ~spliced)[0]
        for i in p_idx[rng.random(len(p_idx)) < 0.5]:
            blob[int(off[i]):int(off[i]) + 4] = np.frombuffer(vh2[:4], np.uint8)
        route = gm.routes(blob, off, sels)
        want_st, want_rv = _reference(zkv, refs, blob, off, vkeys, pvs, route)
        import torch
        dev = torch.device('cuda', 0)
        d_vk, d_pv, d_p = (torch.from_numpy(np.ascontiguousarray(x).reshape(-1)).to(dev) for x in (vkeys, pvs, blob))
        d_off = torch.from_numpy(off.view(np.int64).copy()).to(dev)
        d_st = torch.full((n,), 255, dtype=torch.uint8, device=dev); d_rv = torch.full((n, 4), 255, dtype=torch.uint8, device=dev)
        gw.verify_batch_dev(n, d_vk.data_ptr(), d_pv.data_ptr(), pvs.shape[1], d_p.data_ptr(), d_off.data_ptr(), len(blob), d_st.data_ptr(),
                            d_rv.data_ptr(), torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        st, rv = d_st.cpu().numpy(), d_rv.cpu().numpy()
        bad = np.nonzero((st != want_st) | (rv != want_rv).any(axis=1))[0]
        assert not len(bad), (n, bad[:8], st[bad[:8]], want_st[bad[:8]])
        assert gw.last_route_counts() == gm.counts(route, 3), n
        if n >= 4096:
            assert {0, 1, 8} <= set(st.tolist()), n
    for v in refs:
        v.close()
    gw.close()


@pytest.mark.gpu
def test_aggregate_check_keeps_the_statuses(zkv, keys, real_proofs, monkeypatch):
    """Every route gets at least ZKV_AGG_MIN proofs (lowered to 64), so every route runs its aggregate check."""
    (vk1, vh1), (vk2, vh2), _ = keys
    from stylus_zkvm_verifiers_amd import synth
    monkeypatch.setenv('ZKV_AGG_MIN', '64')
    g, p = _pools(keys, real_proofs, n_g=512)
    n = 3072
    blob, off, vkeys, pvs, kind, _, _ = synth.make_sp1_gateway_batch(g, p, n, 0.5, 0x6A7E04)
    p_idx = np.nonzero(kind == 1)[0]
    for i in p_idx[::2]:
        blob[int(off[i]):int(off[i]) + 4] = np.frombuffer(vh2[:4], np.uint8)
    gw = zkv.Sp1Gateway(True, [(vk1, vh1), (vk2, vh2)])
    route = gm.routes(blob, off, [r[0] for r in gw.routes()])
    assert min(gm.counts(route, 3)[:3]) >= 64
    proofs = [blob[int(off[i]):int(off[i + 1])].tobytes() for i in range(n)]
    vk_l, pv_l = [x.tobytes() for x in vkeys], [x.tobytes() for x in pvs]
    st0, rv0 = gw.verify_batch(vk_l, pv_l, proofs)
    gw.set_aggregate_check(True, seed=bytes(range(32)), sub_batch=16)
    st1, rv1 = gw.verify_batch(vk_l, pv_l, proofs)
    gw.synchronize()
    assert (st1 == st0).all() and (rv1 == rv0).all()
    assert gw.aggregate_counters()[0] > 0
    assert {0, 1} <= set(st0.tolist())
    gw.set_aggregate_check(False)
    gw.close()


@pytest.mark.gpu
def test_hygiene_route_getters_and_no_wait_faults(zkv, keys):
    (vk1, vh1), (vk2, vh2), _ = keys
    gw = zkv.Sp1Gateway(True, [(vk1, vh1), (vk2, vh2)])
    L = gw._L
    h = C.create_string_buffer(32)
    assert L.zkv_sp1_verifier_hash(h) == 0
    assert gw.routes() == [(h.raw[:4], 1, h.raw), (vh1[:4], 6, vh1), (vh2[:4], 6, vh2)]
    for r, want in ((1, vh1), (2, vh2)):
        o = C.create_string_buffer(32)
        assert L.zkv_sp1_plonk_verifier_hash(L.zkv_sp1_gateway_route_ctx(gw._h, r), o) == 0 and o.raw == want
    gw.reserve(1024)
    gw.synchronize()
    gw.close()
    out = C.c_uint64(1)
    assert L.zkv_diag_wait_faults(0, C.byref(out)) == 0 and out.value == 0

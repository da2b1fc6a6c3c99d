"""SP1 gateway, Groth16 routes with caller-supplied keys, on the GPU (include/zkv_sp1_gateway_keys.h).  A keyed
route holding the reference's own SP1 key and hash is pinned to oracle_lib.sp1_verify_proof; every other expectation is the model of
tests/gateway_keys_model.py (sp1/verifier.rs with the route's hash and key, the pairing by the C oracle) behind the routing rule of
tests/gateway_model.py -- parity unpinned.  Batches are 100 - 200 proofs: group boundaries inside and on wavefronts, every mapping."""
import ctypes as C
import json
import os
import random

import numpy as np
import pytest

import gateway_keys_model as gk
import gateway_model as gm
import gateway_wire_model as gwm
import oracle_lib as ol
import spec_model as m

HERE = os.path.dirname(os.path.abspath(__file__))
H = bytes.fromhex


@pytest.fixture(scope='module')
def zkv():
    import stylus_zkvm_verifiers_amd as z
    assert z.device_count() >= 1, 'no gfx950 device visible'
    return z


@pytest.fixture(scope='module', autouse=True)
def no_gt_tables():
    """The built-in route of these gateways sees a few proofs per call; with the mapping fixed to lane pairs it would build its 5.2 GB of
    GT tables for them.  Same statuses without (the Miller path)."""
    old = os.environ.get('ZKV_GT_WINDOW_BITS')
    os.environ['ZKV_GT_WINDOW_BITS'] = '0'
    yield
    if old is None:
        del os.environ['ZKV_GT_WINDOW_BITS']
    else:
        os.environ['ZKV_GT_WINDOW_BITS'] = old


@pytest.fixture(scope='module')
def keys():
    return gk.Key(0x12DA), gk.Key(0x12DB), gk.Key(0x12DC)


@pytest.fixture(scope='module')
def plonk():
    d = json.load(open(os.path.join(HERE, 'golden', 'plonk_cases.json')))
    return d, (H(d['vk']), H(d['verifier_hash']))


def _blob(proofs):
    off = np.zeros(len(proofs) + 1, dtype=np.uint64); off[1:] = np.cumsum([len(p) for p in proofs])
    return np.frombuffer(b''.join(proofs) + b'\0', dtype=np.uint8), off


def _dev_call(gw, vkeys, pvs, proofs, recv=True, shift=0):
    """Device-resident call; the public values share one length.  Every buffer holds what the n proofs need and `shift` bytes in front:
    shift = 1 hands the library odd addresses for the proof and vkey buffers."""
    import torch
    dev = torch.device('cuda', 0)
    n = len(proofs)
    blob, off = _blob(proofs)
    pv_len = len(pvs[0])
    assert all(len(w) == pv_len for w in pvs)
    d_vk = torch.from_numpy(np.frombuffer(bytes(shift) + b''.join(vkeys), dtype=np.uint8).copy()).to(dev)
    d_pv = torch.from_numpy(np.frombuffer(b''.join(pvs) + b'\0', dtype=np.uint8).copy()).to(dev)
    d_p = torch.from_numpy(np.frombuffer(bytes(shift) + blob.tobytes(), dtype=np.uint8).copy()).to(dev)
    d_off = torch.from_numpy(off.view(np.int64).copy()).to(dev)
    d_st = torch.full((n,), 255, dtype=torch.uint8, device=dev)
    d_rv = torch.full((n, 4), 255, dtype=torch.uint8, device=dev)
    gw.verify_batch_dev(n, d_vk.data_ptr() + shift, d_pv.data_ptr(), pv_len, d_p.data_ptr() + shift, d_off.data_ptr(), int(off[-1]), d_st.data_ptr(),
                        d_rv.data_ptr() if recv else 0, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return d_st.cpu().numpy(), d_rv.cpu().numpy()


def _expect(items, sels, verifiers):
    """Statuses, received selectors and route of every (vkey, pv, proof): verifiers[r](vkey, pv, proof) -> (status, received)."""
    blob, off = _blob([p for _, _, p in items])
    route = gm.routes(blob, off, sels)
    st, rv = [], []
    for (vkey, pv, proof), r in zip(items, route):
        if r >= 0:
            s, v = verifiers[int(r)](vkey, pv, proof)
        elif r == gm.NOT_FOUND:
            s, v = 8, proof[:4]
        else:
            s, v = 4, bytes(4)
        st.append(int(s)); rv.append(bytes(v or bytes(4)))
    return np.array(st, dtype=np.uint8), rv, route


def _builtin(vkey, pv, proof):
    return ol.sp1_verify_proof(vkey, pv, proof)


def _tamper(proof, word, rng):
    """The proof with one coordinate word replaced by a random value (off the curve, or at least another proof)."""
    at = 4 + 32 * word
    return proof[:at] + m.be32(rng.randrange(m.P)) + proof[at + 32:]


def _merge(rng, queues):
    """One batch from per-route lists, shuffled but keeping every list's own order: the first and the last proof of a route in the batch
    are the first and the last of its list, which the stable partition makes the first and last slot of its group."""
    queues = [list(q) for q in queues if q]
    out = []
    while queues:
        q = rng.choice(queues)
        out.append(q.pop(0))
        if not q:
            queues.remove(q)
    return out


# ---------------------------------------------------------------- 1. the reference's own key behind a keyed route
@pytest.mark.gpu
def test_reference_key_on_a_keyed_route_is_pinned(zkv, real_proofs, verify_corpus):
    gw = zkv.Sp1Gateway(False, groth16_keys=[(m.vk_to_words(m.SP1_VK), m.SP1_VERIFIER_HASH)])
    assert gw.routes() == [(m.SP1_VERIFIER_HASH[:4], 1, m.SP1_VERIFIER_HASH)]
    real = real_proofs['sp1']
    sp1 = (H(real['vkey']), H(real['public_values']), H(real['proof']))
    assert gw.verify_proof(*sp1) is None                                                           # ACCEPT, reference-pinned
    items = [(H(c['vkey']), H(c['public_values']), H(c['proof'])) for c in verify_corpus['cases'] if c['vm'] == 'sp1'] + [sp1]
    want_st, want_rv = [], []
    for vkey, pv, proof in items:
        st, rv = ol.sp1_verify_proof(vkey, pv, proof)
        if st == 5:                        # the one difference between a verifier and a gateway in front of it: no route instead of a mismatch
            st = 8
        want_st.append(st); want_rv.append(bytes(rv or bytes(4)))
    assert {0, 1, 4, 8} <= set(want_st)
    st, rv = gw.verify_batch([v for v, _, _ in items], [w for _, w, _ in items], [p for _, _, p in items])
    assert st.tolist() == want_st and [bytes(x) for x in rv] == want_rv
    for L_ in sorted({len(w) for _, w, _ in items}):
        idx = [i for i, (_, w, _) in enumerate(items) if len(w) == L_]
        dst, drv = _dev_call(gw, [items[i][0] for i in idx], [items[i][1] for i in idx], [items[i][2] for i in idx])
        assert dst.tolist() == [want_st[i] for i in idx], L_
        assert [bytes(x) for x in drv] == [want_rv[i] for i in idx], L_
    for (vkey, pv, proof), ws, wr in zip(items, want_st, want_rv):
        s = C.c_uint8(255); r = C.create_string_buffer(4)
        assert gw._L.zkv_sp1_gateway_verify_proof(gw._h, vkey, pv, len(pv), proof, len(proof), C.byref(s), r) == 0
        assert (s.value, r.raw) == (ws, wr)
    assert sum(gw.last_stage_ms()) > 0
    gw.close()


# ---------------------------------------------------------------- 2. every kind of route in one shuffled batch, every mapping
@pytest.fixture(scope='module')
def mixed_batch(keys, plonk, real_proofs):
    """Built-in route, three keyed routes with 1, 33 and 31 proofs, one PLONK route, unknown selectors and short proofs."""
    A, B, Cc = keys
    d, (pvk, pvh) = plonk
    rng = random.Random(0x12DD)
    real = real_proofs['sp1']
    sp1 = (H(real['vkey']), H(real['public_values']), H(real['proof']))

    def fresh(n):
        return int(rng.randrange(m.R)).to_bytes(32, 'big'), bytes(rng.randrange(256) for _ in range(n))

    def valid(key, n_pv=96):
        vkey, pv = fresh(n_pv)
        return vkey, pv, key.prove(vkey, pv)
    qa = [valid(A)]                                                                                # a group of one slot
    vb = [valid(B, n) for n in (96, 0, 55)]
    va = valid(A)
    qb = [vb[0]]                                                                                   # first slot: valid
    qb.append((va[0], va[1], B.selector + va[2][4:]))                                              # valid for key A, under key B's selector
    qb.append((vb[1][0], vb[1][1], vb[1][2][:259]))                                                # 259 and 261 bytes under a keyed selector
    qb.append((vb[1][0], vb[1][1], vb[1][2] + b'\0'))
    qb.append((m.be32(m.R), vb[2][1], vb[2][2]))                                                   # program vkey = R
    qb.append((vb[2][0], vb[2][1] + b'\x01', vb[2][2]))                                            # other public values
    qb.append((vb[0][0], vb[0][1], B.selector + bytes(256)))                                       # A = B = C = (0, 0)
    while len(qb) < 32:
        v = vb[len(qb) % 3]
        qb.append(v if len(qb) % 4 else (v[0], v[1], _tamper(v[2], len(qb) % 8, rng)))
    qb.append(vb[1])                                                                               # last slot (the 33rd: a wavefront of its own on lane pairs): valid
    vc = [valid(Cc, n) for n in (64, 96, 120)]
    qc = [vc[0]] + [vc[k % 3] if k % 5 else (vc[k % 3][0], vc[k % 3][1], _tamper(vc[k % 3][2], k % 8, rng)) for k in range(29)] + [vc[2]]
    assert (len(qa), len(qb), len(qc)) == (1, 33, 31)
    q0 = [sp1, (sp1[0], sp1[1], _tamper(sp1[2], 6, rng)), sp1, (sp1[0], sp1[1][:-1] + b'\0', sp1[2])]
    qp = [(H(c['vkey']), H(c['public_values']), H(c['proof'])) for c in d['cases'][:6]]
    qx = [(sp1[0], sp1[1], sp1[2][:k]) for k in range(4)]                                          # shorter than 4 bytes
    qx += [(sp1[0], sp1[1], bytes(rng.randrange(256) for _ in range(4)) + sp1[2][4:]) for _ in range(5)]   # unknown selectors
    qx.append((sp1[0], sp1[1], H(real_proofs['risc0']['seal'])))
    items = _merge(rng, [q0, qa, qb, qc, qp, qx])
    hashes = [None, A.hash, B.hash, Cc.hash, pvh]
    verifiers = [_builtin, A.verify, B.verify, Cc.verify, lambda v, w, p: ol.sp1_plonk_verify_proof(pvk, pvh, v, w, p)]
    return items, hashes, verifiers


@pytest.fixture(scope='module')
def mixed_gateway(zkv, keys, plonk, mixed_batch):
    A, B, Cc = keys
    gw = zkv.Sp1Gateway(True, [plonk[1]], groth16_keys=[(k.words, k.hash) for k in (A, B, Cc)])
    sels = [r[0] for r in gw.routes()]
    assert [r[1] for r in gw.routes()] == [1, 1, 1, 1, 6] and sels[1:4] == [k.selector for k in (A, B, Cc)]
    items, _, verifiers = mixed_batch
    want = _expect(items, sels, verifiers)
    yield gw, sels, want
    gw.close()


@pytest.mark.gpu
@pytest.mark.parametrize('lanes', [0, 2, 16, 64, 128])
def test_every_kind_of_route_in_one_shuffled_batch(mixed_gateway, mixed_batch, keys, lanes):
    gw, sels, (want_st, want_rv, route) = mixed_gateway
    items = mixed_batch[0]
    assert gm.counts(route, 5)[1:4] == [1, 33, 31] and {0, 1, 2, 3, 4, gm.NOT_FOUND, gm.SHORT} <= set(route.tolist())
    for r in (1, 2, 3):                                             # first and last slot of every keyed group hold a valid proof
        idx = np.nonzero(route == r)[0]
        assert want_st[idx[0]] == 0 and want_st[idx[-1]] == 0
    assert {0, 1, 4} <= set(want_st[route == 2].tolist())
    gw.set_lanes_per_proof(lanes)
    st, rv = gw.verify_batch([v for v, _, _ in items], [w for _, w, _ in items], [p for _, _, p in items])
    bad = np.nonzero(st != want_st)[0]
    assert not len(bad), (lanes, bad.tolist(), route[bad].tolist(), st[bad].tolist(), want_st[bad].tolist())
    assert [bytes(x) for x in rv] == want_rv
    assert gw.last_route_counts() == gm.counts(route, 5)
    gw.set_lanes_per_proof(0)


@pytest.mark.gpu
def test_several_count_blocks_and_a_chunked_keyed_group(zkv, mixed_gateway, mixed_batch, keys, plonk, monkeypatch):
    """The mixed batch seven times over under a seeded permutation: 595 proofs are three 256-proof count blocks, so a slot is its route's
    first slot plus the scanned counts of the blocks in front plus the rank in its own block; the keyed groups hold 7, 231 and 217 proofs.
    Through the host entry; through the device-resident one, which takes one public-values length per call, on the proofs of the most
    common length repeated past 512 (three count blocks there too); then on a gateway created with 64-slot chunks, whose keyed group
    runs in 8 chunks."""
    gw, sels, (want_st, want_rv, route) = mixed_gateway
    items = mixed_batch[0]
    reps = 7
    perm = list(range(reps * len(items)))
    random.Random(0x12DF).shuffle(perm)
    idx = [p % len(items) for p in perm]
    big = [items[i] for i in idx]
    big_st, big_rv, big_route = want_st[idx], [want_rv[i] for i in idx], route[idx]
    counts = [reps * c for c in gm.counts(route, 5)]
    assert len(big) == 595 > 512 and counts[1:4] == [7, 231, 217] and gm.counts(big_route, 5) == counts

    def check(g, what):
        st, rv = g.verify_batch([v for v, _, _ in big], [w for _, w, _ in big], [p for _, _, p in big])
        bad = np.nonzero(st != big_st)[0]
        assert not len(bad), (what, bad.tolist(), big_route[bad].tolist(), st[bad].tolist(), big_st[bad].tolist())
        assert [bytes(x) for x in rv] == big_rv, what
        assert g.last_route_counts() == counts, what
    check(gw, 'defaults')
    lens = [len(w) for _, w, _ in items]
    common = max(sorted(set(lens)), key=lens.count)
    same = [i for i in range(len(items)) if lens[i] == common]
    sub = [same[p % len(same)] for p in perm if p < len(same) * (512 // len(same) + 1)]
    assert len(sub) > 512 and all(c > 0 for c in gm.counts(route[sub], 5)[1:4])     # every keyed route, in more than two count blocks
    dst, drv = _dev_call(gw, [items[i][0] for i in sub], [items[i][1] for i in sub], [items[i][2] for i in sub])
    assert dst.tolist() == want_st[sub].tolist()
    assert [bytes(x) for x in drv] == [want_rv[i] for i in sub]
    assert gw.last_route_counts() == gm.counts(route[sub], 5)
    monkeypatch.setenv('ZKV_CHUNK', '64')
    A, B, Cc = keys
    g64 = zkv.Sp1Gateway(True, [plonk[1]], groth16_keys=[(k.words, k.hash) for k in (A, B, Cc)])
    try:
        check(g64, '64-slot chunks')
    finally:
        g64.close()


# ---------------------------------------------------------------- 3. an invalid key fails its own route only
@pytest.mark.gpu
def test_a_key_with_an_off_curve_ic_point_fails_its_own_route_only(zkv, keys, mixed_batch, mixed_gateway, plonk):
    A, B, Cc = keys
    items = mixed_batch[0]
    _, _, (good_st, good_rv, route) = mixed_gateway
    bad_words = gk.off_curve_ic(B.words)
    gw = zkv.Sp1Gateway(True, [plonk[1]], groth16_keys=[(A.words, A.hash), (bad_words, B.hash), (Cc.words, Cc.hash)])
    st, rv = gw.verify_batch([v for v, _, _ in items], [w for _, w, _ in items], [p for _, _, p in items])
    on_b = route == 2
    # every proof of the bad key's route that reaches the key fails; its length errors stay; the model with the bad key says the same
    want_b = [gk.sp1_verify_proof(bad_words, B.hash, *items[i])[0] for i in np.nonzero(on_b)[0]]
    assert st[on_b].tolist() == want_b and set(want_b) == {1, 4} and 0 in good_st[on_b]
    assert st[~on_b].tolist() == good_st[~on_b].tolist()                                         # the other routes: unchanged
    assert [bytes(x) for x in rv] == good_rv
    gw.close()


# ---------------------------------------------------------------- 4. device-resident, fixed-stride public values at the SHA-256 padding edges
@pytest.mark.gpu
@pytest.mark.parametrize('pv_len,shift', [(0, 0), (55, 0), (56, 0), (64, 0), (64, 1)])
def test_device_resident_call_at_the_padding_edges(mixed_gateway, keys, real_proofs, pv_len, shift):
    gw, sels, _ = mixed_gateway
    A, B, Cc = keys
    rng = random.Random(0x12DE00 + pv_len)
    items = []
    for k in range(40):
        key = (A, B, Cc)[k % 3]
        vkey = int(rng.randrange(m.R)).to_bytes(32, 'big'); pv = bytes(rng.randrange(256) for _ in range(pv_len))
        proof = key.prove(vkey, pv) if k < 6 else items[k % 6][2]                                # six valid proofs, reused with other inputs
        if k >= 6:
            vkey, pv = (items[k % 6][0], items[k % 6][1]) if k % 4 else (vkey, pv)
        items.append((vkey, pv, proof))
    items.append((items[0][0], items[0][1], items[0][2][:259]))
    items.append((items[0][0], items[0][1], b'\xde\xad\xbe\xef' + items[0][2][4:]))
    items.append((items[0][0], items[0][1], b'\xa4\x59'))
    verifiers = [_builtin, A.verify, B.verify, Cc.verify, None]
    want_st, want_rv, route = _expect(items, sels, verifiers)
    assert {0, 1, 4, 8} <= set(want_st.tolist()) and (pv_len == 0 or (want_st[route >= 0] == 1).any())
    st, rv = _dev_call(gw, [v for v, _, _ in items], [w for _, w, _ in items], [p for _, _, p in items], shift=shift)
    assert st.tolist() == want_st.tolist() and [bytes(x) for x in rv] == want_rv
    assert gw.last_route_counts() == gm.counts(route, 5)
    if shift:
        st, _ = _dev_call(gw, [v for v, _, _ in items], [w for _, w, _ in items], [p for _, _, p in items], recv=False, shift=shift)
        assert st.tolist() == want_st.tolist()


# ---------------------------------------------------------------- 5. eth_call batches, both calldata forms
class _WireModel(gwm.Gateway):
    """gateway_wire_model.Gateway with the keyed routes between the built-in route and the PLONK routes."""

    def __init__(self, groth16, keyed, plonk):
        gwm.Gateway.__init__(self, groth16, plonk)
        g = int(self.groth16)
        self.keyed = list(keyed)
        self.selectors = self.selectors[:g] + [k.selector for k in self.keyed] + self.selectors[g:]

    def verify(self, vkey, pv, proof):
        off = np.array([0, len(proof)], dtype=np.uint64)
        col = int(gm.routes(np.frombuffer(bytes(proof) + b'\0', np.uint8), off, self.selectors)[0])
        g = int(self.groth16)
        if g <= col < g + len(self.keyed):
            st, rv = self.keyed[col - g].verify(vkey, pv, proof)
            return st, rv, col
        if col >= g + len(self.keyed):
            vk, vh = self.plonk[col - g - len(self.keyed)]
            st, rv = ol.sp1_plonk_verify_proof(vk, vh, vkey, pv, proof)
            return st, bytes(rv or bytes(4)), col
        return gwm.Gateway.verify(self, vkey, pv, proof)           # the built-in route, not found, short


@pytest.mark.gpu
def test_eth_call_batch_both_calldata_forms(mixed_gateway, mixed_batch, keys, plonk):
    gw, sels, _ = mixed_gateway
    model = _WireModel(True, keys, [plonk[1]])
    assert model.selectors == sels
    items = mixed_batch[0]
    calls = [gwm.encode(k % 2, *it) for k, it in enumerate(items)] + [gwm.encode((k + 1) % 2, *it) for k, it in enumerate(items[:40])]
    calls.append(calls[0][:-1]); calls.append(b'\x01\x02\x03\x04' + calls[1][4:])                 # not canonical calls
    want = [model.eth_call(c) for c in calls]
    rev, data, st = gw.eth_call_batch(calls)
    assert st.tolist() == [w[2] for w in want]
    assert rev.tolist() == [int(w[0]) for w in want] and data == [w[1] for w in want]
    assert gw.last_call_counts() == model.counts([w[4] for w in want])
    assert {0, 1, 4, 6, 8} <= set(st.tolist())
    # device-resident: statuses and received selectors stay on the device
    import torch
    dev = torch.device('cuda', 0)
    blob, off = _blob(calls)
    n = len(calls)
    d_cd = torch.from_numpy(blob.copy()).to(dev); d_off = torch.from_numpy(off.view(np.int64).copy()).to(dev)
    d_st = torch.full((n,), 255, dtype=torch.uint8, device=dev); d_rv = torch.full((n, 4), 255, dtype=torch.uint8, device=dev)
    gw.eth_call_batch_dev(n, d_cd.data_ptr(), d_off.data_ptr(), int(off[-1]), d_st.data_ptr(), d_rv.data_ptr(), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert d_st.cpu().numpy().tolist() == [w[2] for w in want]
    assert [bytes(x) for x in d_rv.cpu().numpy()] == [w[3] for w in want]


# ---------------------------------------------------------------- 6. no keys: the old constructor
@pytest.mark.gpu
def test_no_keys_equals_the_old_constructor(zkv, plonk, real_proofs, verify_corpus):
    from stylus_zkvm_verifiers_amd import sp1_gateway_keys
    d, (pvk, pvh) = plonk
    old = zkv.Sp1Gateway(True, [(pvk, pvh)])
    new = zkv.Sp1Gateway(True, [(pvk, pvh)])
    new._L.zkv_ctx_destroy(new._h)
    new._h = sp1_gateway_keys.create(True, [], [(pvk, pvh)], 0)                                  # zkv_sp1_gateway_create_keyed with n_keys = 0
    assert new._h and new.routes() == old.routes()
    items = [(H(c['vkey']), H(c['public_values']), H(c['proof'])) for c in d['cases']]
    items += [(H(c['vkey']), H(c['public_values']), H(c['proof'])) for c in verify_corpus['cases'] if c['vm'] == 'sp1']
    s = real_proofs['sp1']
    items += [(H(s['vkey']), H(s['public_values']), H(s['proof'])), (H(s['vkey']), H(s['public_values']), H(real_proofs['risc0']['seal']))]
    args = ([v for v, _, _ in items], [w for _, w, _ in items], [p for _, _, p in items])
    st0, rv0 = old.verify_batch(*args)
    st1, rv1 = new.verify_batch(*args)
    assert st1.tolist() == st0.tolist() and rv1.tolist() == rv0.tolist() and {0, 1, 4, 8} <= set(st0.tolist())
    assert new.last_route_counts() == old.last_route_counts()
    old.close(); new.close()

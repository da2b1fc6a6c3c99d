"""Aggregate check on the keyed routes of the SP1 gateway (include/zkv_sp1_gateway_keys.h) on the device: with the
check on, statuses and received selectors equal the ones with it off and the model's (tests/gateway_keys_model.py behind the routing rule
of tests/gateway_model.py -- parity unpinned); the counters count the key-uniform sub-batches the layout predicts (zkv_gset_layout.h
route_layout_agg); a failed sub-batch is verified again in place; several aggregate chunks, the device-resident and the eth_call entry; a
fixed mapping and the check switched off leave the counters alone; and the wait-fault counter.
Volume comes from one trapdoor proof per key, re-randomised (synth.make_groth16_batch): such proofs verify by construction, so the model
is asked about every damaged proof and the first eight of every route, and the run with the check off covers the rest."""
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
pytestmark = pytest.mark.gpu
SEED = bytes(range(32, 64))
PV_LEN = 96


@pytest.fixture(scope='module')
def zkv():
    import stylus_zkvm_verifiers_amd as z
    assert z.device_count() >= 1, 'no gfx950 device visible'
    return z


@pytest.fixture(scope='module', autouse=True)
def no_gt_tables():
    """The built-in route of these gateways sees a few proofs per call: no GT tables for them (same statuses on the Miller path)."""
    old = os.environ.get('ZKV_GT_WINDOW_BITS')
    os.environ['ZKV_GT_WINDOW_BITS'] = '0'
    yield
    if old is None:
        del os.environ['ZKV_GT_WINDOW_BITS']
    else:
        os.environ['ZKV_GT_WINDOW_BITS'] = old


@pytest.fixture
def low_min(monkeypatch):
    monkeypatch.setenv('ZKV_AGG_MIN', '64')


def _faults():
    from stylus_zkvm_verifiers_amd import _lib
    out = C.c_uint64(1 << 40)
    _lib.check(_lib.lib().zkv_diag_wait_faults(0, C.byref(out)), 'zkv_diag_wait_faults')
    return out.value


@pytest.fixture(scope='module')
def faults_before(zkv):
    return _faults()


class AlphaInfKey(gk.Key):
    """A trapdoor key with alpha at infinity (discrete log 0): valid, its proofs verify, but it cannot take the aggregate check."""

    def __init__(self, seed):
        gk.Key.__init__(self, seed)
        self.td = dict(self.td, alpha=0)
        self.vk = dict(self.vk, alpha1=(0, 0))
        self.words = m.vk_to_words(self.vk)


def _volume(key, n, seed):
    """n valid proofs of one route, all for one (program vkey, public values): one trapdoor proof, re-randomised."""
    from stylus_zkvm_verifiers_amd import synth
    rng = random.Random(seed)
    vkey = int(rng.randrange(m.R)).to_bytes(32, 'big')
    pv = bytes(rng.randrange(256) for _ in range(PV_LEN))
    base = key.prove(vkey, pv)
    sig = [int.from_bytes(vkey, 'big'), m.sp1_hash_public_values(pv)]
    rows = synth.make_groth16_batch(key.words, 'sp1', base[4:], sig, n, seed=seed, pool=4, mutate_every=0)[0]
    return [(vkey, pv, key.selector + bytes(r)) for r in rows]


@pytest.fixture(scope='module')
def keys():
    return gk.Key(0x12F0), gk.Key(0x12F1), gk.Key(0x12F2), gk.Key(0x12F3), AlphaInfKey(0x12F4)


@pytest.fixture(scope='module')
def volumes(keys):
    """Per key: 1,100 valid proofs (the alpha-at-infinity key: 100)."""
    return [_volume(k, 100 if isinstance(k, AlphaInfKey) else 1100, 0x12F8 + j) for j, k in enumerate(keys)]


@pytest.fixture(scope='module')
def plonk():
    d = json.load(open(os.path.join(HERE, 'golden', 'plonk_cases.json')))
    return d, (H(d['vk']), H(d['verifier_hash']))


def _flip_pv(it):
    return it[0], it[1][:-1] + bytes([it[1][-1] ^ 1]), it[2]


def _tamper(proof, word, rng):
    at = 4 + 32 * word
    return proof[:at] + m.be32(rng.randrange(m.P)) + proof[at + 32:]


def _damaged_queue(q, key, other, rng):
    """The route's valid proofs with damaged ones of every class among them; returns (queue, damaged positions)."""
    q = list(q)
    bad = {}
    bad[5] = (q[5][0], q[5][1], _tamper(q[5][2], 7, rng))                           # C off the curve (or another point): refused before or at the pairing
    bad[70] = _flip_pv(q[70])                                                        # other public values: the pairing fails
    bad[71] = (q[71][0], q[71][1], q[71][2][:259])                                   # 259 and 261 bytes under the route's selector
    bad[72] = (q[72][0], q[72][1], q[72][2] + b'\0')
    bad[130] = (m.be32(m.R), q[130][1], q[130][2])                                   # program vkey = R
    bad[200] = (other[0], other[1], key.selector + other[2][4:])                     # valid under another key, this route's selector
    bad[300] = (q[300][0], q[300][1], key.selector + bytes(256))                     # A = B = C = (0, 0)
    for k in range(333, len(q), 97):
        bad[k] = _flip_pv(q[k]) if k % 2 else (q[k][0], q[k][1], _tamper(q[k][2], k % 8, rng))
    for k, it in bad.items():
        q[k] = it
    return q, sorted(bad)


def _merge(rng, queues):
    """One batch from per-route lists, shuffled but keeping every list's own order (the stable partition keeps it in the slots)."""
    tags = [j for j, q in enumerate(queues) for _ in q]
    rng.shuffle(tags)
    at = [0] * len(queues)
    out = []
    for j in tags:
        out.append((j, at[j])); at[j] += 1
    return out


def _cols(items):
    return [v for v, _, _ in items], [w for _, w, _ in items], [p for _, _, p in items]


def _counters(gw):
    return tuple(int(x) for x in gw.aggregate_counters())


def _predicted(counts, capable, sub):
    unit = max(64, sub)
    return sum(c // unit * unit // sub for c, ok in zip(counts, capable) if ok)


# ---------------------------------------------------------------- 1. parity and engagement
@pytest.fixture(scope='module')
def mixed(zkv, keys, volumes, plonk, real_proofs):
    """Built-in route (4 proofs), three keyed routes (1,000, 900 and 1,100 proofs, damaged ones of every class among them), one PLONK
    route (6), tampered selectors and short proofs: about 3,000 proofs, shuffled."""
    A, B, Cc = keys[:3]
    d, (pvk, pvh) = plonk
    rng = random.Random(0x12FA)
    real = real_proofs['sp1']
    sp1 = (H(real['vkey']), H(real['public_values']), H(real['proof']))
    q0 = [sp1, (sp1[0], sp1[1], _tamper(sp1[2], 6, rng)), sp1, (sp1[0], sp1[1][:-1] + b'\0', sp1[2])]
    queues, damaged = [q0], [list(range(4))]
    for j, n in enumerate((1000, 900, 1100)):
        q, bad = _damaged_queue(volumes[j][:n], keys[j], volumes[(j + 1) % 3][0], rng)
        queues.append(q); damaged.append(bad)
    qp = [(H(c['vkey']), H(c['public_values']), H(c['proof'])) for c in d['cases'][:6]]
    qx = [(sp1[0], sp1[1], sp1[2][:k]) for k in range(4)]                                          # shorter than 4 bytes
    for j in range(3):                                                                            # a keyed route's selector with one bit flipped
        p = volumes[j][3][2]
        qx.append((volumes[j][3][0], volumes[j][3][1], bytes([p[0] ^ 1]) + p[1:]))
    queues += [qp, qx]; damaged += [list(range(len(qp))), list(range(len(qx)))]
    order = _merge(rng, queues)
    items = [queues[j][k] for j, k in order]
    gw = zkv.Sp1Gateway(True, [plonk[1]], groth16_keys=[(k.words, k.hash) for k in (A, B, Cc)])
    sels = [r[0] for r in gw.routes()]
    verifiers = [ol.sp1_verify_proof, A.verify, B.verify, Cc.verify, lambda v, w, p: ol.sp1_plonk_verify_proof(pvk, pvh, v, w, p)]
    blob = np.frombuffer(b''.join(p for _, _, p in items) + b'\0', dtype=np.uint8)
    off = np.zeros(len(items) + 1, dtype=np.uint64); off[1:] = np.cumsum([len(p) for _, _, p in items])
    route = gm.routes(blob, off, sels)
    want_st, want_rv = np.zeros(len(items), np.uint8), [bytes(4)] * len(items)
    for i, (j, k) in enumerate(order):
        r = int(route[i])
        if r >= 0 and (k in damaged[j] or k < 8):                  # the model; every other proof is a re-randomised valid one: status 0
            s, v = verifiers[r](*items[i])
            want_st[i], want_rv[i] = s, bytes(v or bytes(4))
        elif r == gm.NOT_FOUND:
            want_st[i], want_rv[i] = 8, items[i][2][:4]
        elif r < 0:
            want_st[i] = 4
    assert {0, 1, 4, 8} <= set(want_st.tolist()) and gm.counts(route, 5)[:5] == [4, 1000, 900, 1100, 6]
    yield gw, items, want_st, want_rv, route
    gw.close()


@pytest.mark.parametrize('sub', [None, 16, 64, 256])
def test_statuses_equal_the_per_proof_path_and_the_model(mixed, low_min, sub):
    gw, items, want_st, want_rv, route = mixed
    gw.set_aggregate_check(False)
    st0, rv0 = gw.verify_batch(*_cols(items))
    bad = np.nonzero(st0 != want_st)[0]
    assert not len(bad), ('check off', bad.tolist()[:8], route[bad].tolist()[:8], st0[bad].tolist()[:8], want_st[bad].tolist()[:8])
    assert [bytes(x) for x in rv0] == want_rv
    c0 = _counters(gw)
    gw.set_aggregate_check(True, SEED, sub)
    st1, rv1 = gw.verify_batch(*_cols(items))
    c1 = _counters(gw)
    gw.set_aggregate_check(False)
    bad = np.nonzero(st1 != want_st)[0]
    assert not len(bad), (sub, bad.tolist()[:8], route[bad].tolist()[:8], st1[bad].tolist()[:8], want_st[bad].tolist()[:8])
    assert rv1.tobytes() == rv0.tobytes()
    assert gw.last_route_counts() == gm.counts(route, 5)
    # the built-in and the PLONK route hold fewer than 64 proofs: what was checked in aggregate is the keyed group's
    s = sub or 32
    assert c1[0] - c0[0] == _predicted([1000, 900, 1100], [1, 1, 1], s) and c1[1] > c0[1]


# ---------------------------------------------------------------- 2. the predicted sub-batches, all proofs valid
@pytest.mark.parametrize('sub', [16, 64, 256])
def test_all_valid_counts_the_predicted_sub_batches(zkv, keys, volumes, low_min, sub):
    """Keyed routes only, with A - 1, A, 2A + 1 and 0 proofs, and 100 proofs of a key with alpha at infinity, which cannot take the check."""
    unit = max(64, sub)
    counts = [unit - 1, unit, 2 * unit + 1, 0, 100]
    gw = zkv.Sp1Gateway(False, groth16_keys=[(k.words, k.hash) for k in keys])
    try:
        queues = [volumes[j][:n] for j, n in enumerate(counts)]
        items = [queues[j][k] for j, k in _merge(random.Random(0x12FB + sub), queues)]
        gw.set_aggregate_check(True, SEED, sub)
        c0 = _counters(gw)
        st, rv = gw.verify_batch(*_cols(items))
        c1 = _counters(gw)
        assert not st.any() and not rv.any()
        assert gw.last_route_counts()[:5] == counts
        assert (c1[0] - c0[0], c1[1] - c0[1]) == (_predicted(counts, [1, 1, 1, 1, 0], sub), 0) and c1[0] - c0[0] == 3 * unit // sub
    finally:
        gw.close()


# ---------------------------------------------------------------- 3. failed sub-batches are verified again in place
def test_failed_sub_batches_reject_only_their_bad_proofs(zkv, keys, volumes, low_min):
    A, B = keys[:2]
    gw = zkv.Sp1Gateway(False, groth16_keys=[(A.words, A.hash), (B.words, B.hash)])
    try:
        qa, qb = list(volumes[0][:300]), list(volumes[1][:300])
        qa[77] = _flip_pv(qa[77])                                   # rank 77 of key A: sub-batch 4 of its aggregate part (256 proofs at sub 16)
        qb[255] = _flip_pv(qb[255])                                 # the last proof of key B's aggregate part
        cross = volumes[0][5]
        qb[299] = (cross[0], cross[1], B.selector + cross[2][4:])   # valid under key A, key B's selector; rank 299: key B's per-proof part
        order = _merge(random.Random(0x12FC), [qa, qb])
        items = [(qa, qb)[j][k] for j, k in order]
        assert A.verify(*qa[77])[0] == 1 and B.verify(*qb[255])[0] == 1 and B.verify(*qb[299])[0] == 1 and A.verify(*cross)[0] == 0
        want = np.array([1 if (j, k) in ((0, 77), (1, 255), (1, 299)) else 0 for j, k in order], np.uint8)
        gw.set_aggregate_check(True, SEED, 16)
        c0 = _counters(gw)
        st, rv = gw.verify_batch(*_cols(items))
        c1 = _counters(gw)
        assert st.tolist() == want.tolist() and not rv.any()
        assert (c1[0] - c0[0], c1[1] - c0[1]) == (32, 2)
        # the cross-key proof inside key B's aggregate part: one more failed sub-batch, the same verdicts
        qb[299], qb[100] = volumes[1][299], (cross[0], cross[1], B.selector + cross[2][4:])
        items = [(qa, qb)[j][k] for j, k in order]
        want = np.array([1 if (j, k) in ((0, 77), (1, 255), (1, 100)) else 0 for j, k in order], np.uint8)
        st, _ = gw.verify_batch(*_cols(items))
        c2 = _counters(gw)
        assert st.tolist() == want.tolist() and (c2[0] - c1[0], c2[1] - c1[1]) == (32, 3)
    finally:
        gw.close()


# ---------------------------------------------------------------- 4. chunks and entry points
def _dev_call(gw, items, stream, shift):
    import torch
    dev = torch.device('cuda', 0)
    n = len(items)
    vkeys, pvs, proofs = _cols(items)
    off = np.zeros(n + 1, dtype=np.uint64); off[1:] = np.cumsum([len(p) for p in proofs])
    up = lambda b: torch.from_numpy(np.frombuffer(b, dtype=np.uint8).copy()).to(dev)
    d_vk, d_pv, d_p = up(bytes(shift) + b''.join(vkeys)), up(b''.join(pvs) + b'\0'), up(bytes(shift) + b''.join(proofs) + b'\0')
    d_off = torch.from_numpy(off.view(np.int64).copy()).to(dev)
    d_st = torch.full((n,), 255, dtype=torch.uint8, device=dev)
    d_rv = torch.full((n, 4), 255, dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()
    with torch.cuda.stream(stream):
        gw.verify_batch_dev(n, d_vk.data_ptr() + shift, d_pv.data_ptr(), PV_LEN, d_p.data_ptr() + shift, d_off.data_ptr(), int(off[-1]), d_st.data_ptr(),
                            d_rv.data_ptr(), stream.cuda_stream)
    stream.synchronize()
    return d_st.cpu().numpy(), d_rv.cpu().numpy()


@pytest.fixture(scope='module')
def small(keys, volumes):
    """Two keyed routes with 200 and 150 proofs, damaged ones among them, a flipped selector and a short proof; one public-values length."""
    rng = random.Random(0x12FD)
    A, B = keys[:2]
    qa, qb = list(volumes[0][:200]), list(volumes[1][:150])
    bad = {(0, 3): _flip_pv(qa[3]), (0, 64): (qa[64][0], qa[64][1], qa[64][2][:259]), (0, 191): (m.be32(m.R), qa[191][1], qa[191][2]),
           (0, 199): _flip_pv(qa[199]), (1, 0): (qb[0][0], qb[0][1], _tamper(qb[0][2], 1, rng)), (1, 127): _flip_pv(qb[127]),
           (1, 128): (qa[0][0], qa[0][1], B.selector + qa[0][2][4:])}
    for (j, k), it in bad.items():
        (qa, qb)[j][k] = it
    p = volumes[0][1]
    qx = [(p[0], p[1], bytes([p[2][0] ^ 1]) + p[2][1:]), (p[0], p[1], p[2][:3])]
    queues = [qa, qb, qx]
    order = _merge(rng, queues)
    items = [queues[j][k] for j, k in order]
    want = np.zeros(len(items), np.uint8)
    rv = [bytes(4)] * len(items)
    for i, (j, k) in enumerate(order):
        if (j, k) in bad:
            want[i] = (A, B)[j].verify(*items[i])[0]
        elif j == 2:
            want[i], rv[i] = (8, items[i][2][:4]) if k == 0 else (4, bytes(4))
    assert {0, 1, 4, 8} <= set(want.tolist())
    return items, want, rv


def test_several_aggregate_chunks_and_every_entry_point(zkv, keys, small, low_min, monkeypatch):
    """64-slot chunks with 16-proof sub-batches: the aggregate region (192 + 128 slots) runs in five chunks, the rests in one more."""
    import torch
    items, want, want_rv = small
    A, B = keys[:2]
    monkeypatch.setenv('ZKV_CHUNK', '64')
    gw = zkv.Sp1Gateway(False, groth16_keys=[(A.words, A.hash), (B.words, B.hash)])
    try:
        gw.set_aggregate_check(True, SEED, 16)
        c0 = _counters(gw)
        st, rv = gw.verify_batch(*_cols(items))
        c1 = _counters(gw)
        assert st.tolist() == want.tolist() and [bytes(x) for x in rv] == want_rv
        # pairing failures in the aggregate region: A ranks 3 and 191 are not both (191 is refused before the pairing), B rank 127
        assert (c1[0] - c0[0], c1[1] - c0[1]) == (20, 2)
        assert sum(gw.last_stage_ms()) > 0
        # device-resident, on the caller's stream, proofs and vkeys from odd addresses
        dst, drv = _dev_call(gw, items, torch.cuda.Stream(), 1)
        c2 = _counters(gw)
        assert dst.tolist() == want.tolist() and [bytes(x) for x in drv] == want_rv and (c2[0] - c1[0], c2[1] - c1[1]) == (20, 2)
        # eth_call: the same proofs as calldata, both forms
        calls = [gwm.encode(k % 2, *it) for k, it in enumerate(items)]
        _, _, wst = gw.eth_call_batch(calls)
        c3 = _counters(gw)
        assert wst.tolist() == want.tolist() and (c3[0] - c2[0], c3[1] - c2[1]) == (20, 2)
        # a mapping fixed by the caller, and the check switched off: the per-proof path
        for lanes in (2, 16, 64):
            gw.set_lanes_per_proof(lanes)
            st, rv = gw.verify_batch(*_cols(items))
            assert st.tolist() == want.tolist() and [bytes(x) for x in rv] == want_rv and _counters(gw) == c3, lanes
        gw.set_lanes_per_proof(0)
        gw.set_aggregate_check(False)
        st, _ = gw.verify_batch(*_cols(items))
        assert st.tolist() == want.tolist() and _counters(gw) == c3
    finally:
        gw.close()


# ---------------------------------------------------------------- 5. no wavefront timed out waiting
def test_no_wait_faults_across_the_module(zkv, faults_before):
    assert _faults() == faults_before

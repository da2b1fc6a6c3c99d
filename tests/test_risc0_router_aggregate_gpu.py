"""Aggregate check on the keyed routes of the RISC Zero router (include/zkv_risc0_router.h) on the device: with
the check on, statuses and received selectors equal the ones with it off and the model's (tests/risc0_router_model.py -- parity unpinned
for the routing); the counters count the key-uniform sub-batches the layout predicts; a failed sub-batch is verified again in place;
several aggregate chunks and every entry point that reaches the keyed group; a fixed mapping and the check switched off leave the
counters alone; and the wait-fault counter.
Volume comes from one trapdoor seal per key, re-randomised (synth.make_groth16_batch): such seals verify by construction, so the model is
asked about every damaged seal and the first eight of every route, and the run with the check off covers the rest."""
import random

import numpy as np
import pytest

import risc0_router_model as rm
import spec_model as m
from test_sp1_gateway_keys_aggregate_gpu import _counters, _faults, _merge, _predicted

H = bytes.fromhex
pytestmark = pytest.mark.gpu
SEED = bytes(range(64, 96))


@pytest.fixture(scope='module')
def zkv():
    import stylus_zkvm_verifiers_amd as z
    assert z.device_count() >= 1, 'no gfx950 device visible'
    return z


@pytest.fixture(scope='module', autouse=True)
def no_gt_tables():
    """The built-in group of these routers sees a few seals per call: no GT tables for them (same statuses on the Miller path)."""
    import os
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


@pytest.fixture(scope='module')
def faults_before(zkv):
    return _faults()


@pytest.fixture(scope='module')
def real(real_proofs):
    r = real_proofs['risc0']
    return dict(root=H(r['control_root']), cid=H(r['bn254_control_id']), seal=H(r['seal']), image_id=H(r['image_id']),
                journal=H(r['journal_digest']), claim=H(r['claim_digest']))


class AlphaInfKey(rm.Key):
    """A keyed route whose key has alpha at infinity (discrete log 0): valid, its seals verify, but it cannot take the aggregate check."""

    def __init__(self, seed):
        rm.Key.__init__(self, seed)
        self.td = dict(self.td, alpha=0)
        self.vk = dict(self.vk, alpha1=(0, 0))
        self.words = m.vk_to_words(self.vk)
        self.route = rm.Route(self.control_root, self.control_id, self.words)
        self.selector = self.route.selector


def _volume(key, n, seed):
    """n valid seals of one keyed route, all for one (image id, journal digest): one trapdoor seal, re-randomised.  Items are
    (seal, image id, journal digest, claim digest)."""
    from stylus_zkvm_verifiers_amd import synth
    rng = random.Random(seed)
    image = bytes(rng.randrange(256) for _ in range(32)); journal = bytes(rng.randrange(256) for _ in range(32))
    claim = m.receipt_claim_ok_digest(image, journal)
    base = key.prove(image, journal)
    rows = synth.make_groth16_batch(key.words, 'risc0', base[4:], key.route.verifier.signals(claim), n, seed=seed, pool=4, mutate_every=0)[0]
    return [(key.selector + bytes(r), image, journal, claim) for r in rows]


@pytest.fixture(scope='module')
def keys():
    return rm.Key(0x17F0), rm.Key(0x17F1), rm.Key(0x17F2), rm.Key(0x17F3), AlphaInfKey(0x17F4)


@pytest.fixture(scope='module')
def volumes(keys):
    """Per key: 1,100 valid seals (the alpha-at-infinity key: 100)."""
    return [_volume(k, 100 if isinstance(k, AlphaInfKey) else 1100, 0x17F8 + j) for j, k in enumerate(keys)]


def _flip(it):
    """The seal with another image id: the pairing fails (the claim digest of the item no longer belongs to it either)."""
    a = it[1][:-1] + bytes([it[1][-1] ^ 1])
    return it[0], a, it[2], bytes([it[3][0] ^ 1]) + it[3][1:]


def _tamper(seal, word, rng):
    at = 4 + 32 * word
    return seal[:at] + m.be32(rng.randrange(m.P)) + seal[at + 32:]


def _damaged_queue(q, key, other, rng):
    q = list(q)
    bad = {}
    bad[5] = (_tamper(q[5][0], 7, rng),) + q[5][1:]                                  # C off the curve (or another point)
    bad[70] = _flip(q[70])                                                           # other inputs: the pairing fails
    bad[71] = (q[71][0][:259],) + q[71][1:]                                          # 259 and 261 bytes under the route's selector
    bad[72] = (q[72][0] + b'\0',) + q[72][1:]
    bad[200] = (key.selector + other[0][4:],) + other[1:]                            # valid under another key, this route's selector
    bad[300] = (key.selector + bytes(256),) + q[300][1:]                             # A = B = C = (0, 0)
    for k in range(333, len(q), 97):
        bad[k] = _flip(q[k]) if k % 2 else (_tamper(q[k][0], k % 8, rng),) + q[k][1:]
    for k, it in bad.items():
        q[k] = it
    return q, sorted(bad)


def _cols(items):
    return [s for s, _, _, _ in items], [a for _, a, _, _ in items], [b for _, _, b, _ in items]


def _routers(zkv, builtin, ks):
    return zkv.RiscZeroRouter(builtin, [k.triple() for k in ks]), rm.Router(builtin, [k.triple() for k in ks])


# ---------------------------------------------------------------- 1. parity and engagement
@pytest.fixture(scope='module')
def mixed(zkv, keys, volumes, real):
    """One built-in route (the real seal and damaged copies: 6 seals), three keyed routes (1,000, 900 and 1,100 seals, damaged ones of
    every class among them), tampered selectors and short seals: about 3,000 seals, shuffled."""
    rng = random.Random(0x17FA)
    rt, model = _routers(zkv, [(real['root'], real['cid'])], keys[:3])
    r4 = (real['seal'], real['image_id'], real['journal'], real['claim'])
    q0 = [r4, (_tamper(r4[0], 6, rng),) + r4[1:], r4, _flip(r4), (r4[0][:259],) + r4[1:], r4]
    queues, damaged = [q0], [list(range(len(q0)))]
    for j, n in enumerate((1000, 900, 1100)):
        q, bad = _damaged_queue(volumes[j][:n], keys[j], volumes[(j + 1) % 3][0], rng)
        queues.append(q); damaged.append(bad)
    qx = [(r4[0][:k],) + r4[1:] for k in range(4)]                                                 # shorter than 4 bytes
    for j in range(3):                                                                            # a keyed route's selector with one bit flipped
        it = volumes[j][3]
        qx.append((bytes([it[0][0] ^ 1]) + it[0][1:],) + it[1:])
    queues.append(qx); damaged.append(list(range(len(qx))))
    order = _merge(rng, queues)
    items = [queues[j][k] for j, k in order]
    route = rm.routes([it[0] for it in items], model.selectors)
    want = [np.zeros(len(items), np.uint8), np.zeros(len(items), np.uint8)]                        # verify, verify_integrity
    want_rv = [bytes(4)] * len(items)
    for i, (j, k) in enumerate(order):
        r = int(route[i])
        if r >= 0 and (k in damaged[j] or k < 8):                  # the model; every other seal is a re-randomised valid one: status 0
            want[0][i] = model.routes[r].verify(items[i][0], items[i][1], items[i][2])[0]
            want[1][i] = model.routes[r].verify_integrity(items[i][0], items[i][3])[0]
        elif r == rm.NOT_FOUND:
            want[0][i] = want[1][i] = 8
            want_rv[i] = items[i][0][:4]
        elif r < 0:
            want[0][i] = want[1][i] = 4
    assert {0, 1, 4, 8} <= set(want[0].tolist()) and rm.counts(route, 4)[:4] == [6, 1000, 900, 1100]
    assert want[0].tolist() == want[1].tolist()
    yield rt, items, want[0], want_rv, route
    rt.close()


@pytest.mark.parametrize('sub', [None, 16, 64, 256])
def test_statuses_equal_the_per_proof_path_and_the_model(mixed, low_min, sub):
    rt, items, want_st, want_rv, route = mixed
    rt.set_aggregate_check(False)
    st0, rv0 = rt.verify_batch(*_cols(items))
    bad = np.nonzero(st0 != want_st)[0]
    assert not len(bad), ('check off', bad.tolist()[:8], route[bad].tolist()[:8], st0[bad].tolist()[:8], want_st[bad].tolist()[:8])
    assert [bytes(x) for x in rv0] == want_rv
    c0 = _counters(rt)
    rt.set_aggregate_check(True, SEED, sub)
    st1, rv1 = rt.verify_batch(*_cols(items))
    c1 = _counters(rt)
    rt.set_aggregate_check(False)
    bad = np.nonzero(st1 != want_st)[0]
    assert not len(bad), (sub, bad.tolist()[:8], route[bad].tolist()[:8], st1[bad].tolist()[:8], want_st[bad].tolist()[:8])
    assert rv1.tobytes() == rv0.tobytes()
    assert rt.last_route_counts() == rm.counts(route, 4)
    # the built-in route holds fewer than 64 seals: what was checked in aggregate is the keyed group's
    assert c1[0] - c0[0] == _predicted([1000, 900, 1100], [1, 1, 1], sub or 32) and c1[1] > c0[1]


# ---------------------------------------------------------------- 2. the predicted sub-batches, all seals valid
@pytest.mark.parametrize('sub', [16, 64, 256])
def test_all_valid_counts_the_predicted_sub_batches(zkv, keys, volumes, real, low_min, sub):
    """A - 1, A, 2A + 1 and 0 seals on four keyed routes, 100 on a key with alpha at infinity, and 3 on the built-in route, which
    cannot engage."""
    unit = max(64, sub)
    counts = [unit - 1, unit, 2 * unit + 1, 0, 100]
    rt, _ = _routers(zkv, [(real['root'], real['cid'])], keys)
    try:
        r4 = (real['seal'], real['image_id'], real['journal'], real['claim'])
        queues = [[r4] * 3] + [volumes[j][:n] for j, n in enumerate(counts)]
        items = [queues[j][k] for j, k in _merge(random.Random(0x17FB + sub), queues)]
        rt.set_aggregate_check(True, SEED, sub)
        c0 = _counters(rt)
        st, rv = rt.verify_batch(*_cols(items))
        c1 = _counters(rt)
        assert not st.any() and not rv.any()
        assert rt.last_route_counts()[:6] == [3] + counts
        assert (c1[0] - c0[0], c1[1] - c0[1]) == (_predicted(counts, [1, 1, 1, 1, 0], sub), 0) and c1[0] - c0[0] == 3 * unit // sub
    finally:
        rt.close()


# ---------------------------------------------------------------- 3. failed sub-batches are verified again in place
def test_failed_sub_batches_reject_only_their_bad_seals(zkv, keys, volumes, low_min):
    A, B = keys[:2]
    rt, model = _routers(zkv, [], [A, B])
    try:
        qa, qb = list(volumes[0][:300]), list(volumes[1][:300])
        qa[77] = _flip(qa[77])                                      # rank 77 of key A: sub-batch 4 of its aggregate part (256 seals at sub 16)
        qb[255] = _flip(qb[255])                                    # the last seal of key B's aggregate part
        cross = volumes[0][5]
        qb[299] = (B.selector + cross[0][4:],) + cross[1:]          # valid under key A, key B's selector; rank 299: key B's per-proof part
        order = _merge(random.Random(0x17FC), [qa, qb])
        items = [(qa, qb)[j][k] for j, k in order]
        for it, w in ((qa[77], 1), (qb[255], 1), (qb[299], 1), (cross, 0)):
            r = model.routes[int(rm.routes([it[0]], model.selectors)[0])]
            assert r.verify(*it[:3])[0] == w
        want = np.array([1 if (j, k) in ((0, 77), (1, 255), (1, 299)) else 0 for j, k in order], np.uint8)
        rt.set_aggregate_check(True, SEED, 16)
        c0 = _counters(rt)
        st, rv = rt.verify_batch(*_cols(items))
        c1 = _counters(rt)
        assert st.tolist() == want.tolist() and not rv.any()
        assert (c1[0] - c0[0], c1[1] - c0[1]) == (32, 2)
    finally:
        rt.close()


# ---------------------------------------------------------------- 4. chunks and entry points
def _dev_call(rt, items, stream, shift):
    import torch
    dev = torch.device('cuda', 0)
    n = len(items)
    seals, in_a, in_b = _cols(items)
    up = lambda rows: torch.from_numpy(np.frombuffer(bytes(shift) + b''.join(rows), dtype=np.uint8).copy()).to(dev)
    d_s, d_a, d_b = up(seals), up(in_a), up(in_b)
    d_st = torch.full((n,), 255, dtype=torch.uint8, device=dev)
    d_rv = torch.full((n, 4), 255, dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()
    with torch.cuda.stream(stream):
        rt.verify_batch_dev(n, d_s.data_ptr() + shift, d_a.data_ptr() + shift, d_b.data_ptr() + shift, d_st.data_ptr(), d_rv.data_ptr(), stream.cuda_stream)
    stream.synchronize()
    return d_st.cpu().numpy(), d_rv.cpu().numpy()


@pytest.fixture(scope='module')
def small(keys, volumes):
    """Two keyed routes with 200 and 150 seals of 260 bytes, damaged ones among them, and a flipped selector."""
    rng = random.Random(0x17FD)
    A, B = keys[:2]
    qa, qb = list(volumes[0][:200]), list(volumes[1][:150])
    bad = {(0, 3): _flip(qa[3]), (0, 64): (A.selector + bytes(256),) + qa[64][1:], (0, 199): _flip(qa[199]),
           (1, 0): (_tamper(qb[0][0], 1, rng),) + qb[0][1:], (1, 127): _flip(qb[127]), (1, 128): (B.selector + qa[0][0][4:],) + qa[0][1:]}
    for (j, k), it in bad.items():
        (qa, qb)[j][k] = it
    it = volumes[0][1]
    queues = [qa, qb, [(bytes([it[0][0] ^ 1]) + it[0][1:],) + it[1:]]]
    order = _merge(rng, queues)
    items = [queues[j][k] for j, k in order]
    want = np.zeros(len(items), np.uint8)
    rv = [bytes(4)] * len(items)
    for i, (j, k) in enumerate(order):
        if (j, k) in bad:
            want[i] = (A, B)[j].route.verify(*items[i][:3])[0]
            assert (A, B)[j].route.verify_integrity(items[i][0], items[i][3])[0] == want[i]
        elif j == 2:
            want[i], rv[i] = 8, items[i][0][:4]
    assert {0, 1, 8} <= set(want.tolist())
    return items, want, rv


def test_several_aggregate_chunks_and_every_entry_point(zkv, keys, small, low_min, monkeypatch):
    """64-slot chunks with 16-seal sub-batches: the aggregate region (192 + 128 slots) runs in five chunks, the rests in one more."""
    import torch
    items, want, want_rv = small
    seals, in_a, in_b = _cols(items)
    claims = [c for _, _, _, c in items]
    monkeypatch.setenv('ZKV_CHUNK', '64')
    rt, _ = _routers(zkv, [], keys[:2])
    try:
        rt.set_aggregate_check(True, SEED, 16)
        c = [_counters(rt)]

        def step(st, rv, what):
            c.append(_counters(rt))
            assert st.tolist() == want.tolist(), what
            assert rv is None or [bytes(x) for x in rv] == want_rv, what
            # pairing failures in the aggregate region: A ranks 3 and 64 (points at infinity are well-formed: they reach the pairing) and
            # B rank 127, in three sub-batches; B rank 0 is refused before the pairing
            assert (c[-1][0] - c[-2][0], c[-1][1] - c[-2][1]) == (20, 3), what
        step(*rt.verify_batch(seals, in_a, in_b), 'verify')
        assert sum(rt.last_stage_ms()) > 0
        step(*rt.verify_integrity_batch(seals, claims), 'verify_integrity')
        step(*_dev_call(rt, items, torch.cuda.Stream(), 1), 'device-resident, caller stream, odd addresses')
        methods = [i % 2 for i in range(len(items))]
        step(*rt.verify_call_batch(methods, seals, [cl if mth else a for mth, cl, a in zip(methods, claims, in_a)], in_b), 'a method per seal')
        calls = [rt.encode_verify_integrity_call(s, cl, i % 2) if i % 3 == 0 else rt.encode_verify_call(s, a, b, i % 2)
                 for i, (s, a, b, cl) in enumerate(items)]
        _, _, wst = rt.eth_call_batch(calls)
        step(wst, None, 'eth_call')
        # a mapping fixed by the caller, and the check switched off: the per-proof path
        for lanes in (2, 16, 64):
            rt.set_lanes_per_proof(lanes)
            st, rv = rt.verify_batch(seals, in_a, in_b)
            assert st.tolist() == want.tolist() and [bytes(x) for x in rv] == want_rv and _counters(rt) == c[-1], lanes
        rt.set_lanes_per_proof(0)
        rt.set_aggregate_check(False)
        st, _ = rt.verify_batch(seals, in_a, in_b)
        assert st.tolist() == want.tolist() and _counters(rt) == c[-1]
    finally:
        rt.close()


# ---------------------------------------------------------------- 5. no wavefront timed out waiting
def test_no_wait_faults_across_the_module(zkv, faults_before):
    assert _faults() == faults_before

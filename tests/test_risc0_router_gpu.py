"""RISC Zero verifier router on the GPU (include/zkv_risc0_router.h).  A built-in route is pinned to
oracle_lib.Risc0Oracle; every other expectation is the model of tests/risc0_router_model.py (risc0/verifier.rs with the route's
parameters and key, the pairing by the C oracle) behind its routing rule -- parity unpinned.  Batches are 100 - 200 seals: group
boundaries inside and on wavefronts, every mapping."""
import ctypes as C
import os
import random

import numpy as np
import pytest

import oracle_lib as ol
import risc0_router_model as rm
import spec_model as m

H = bytes.fromhex
REF_WORDS = m.vk_to_words(m.RISC0_VK)


@pytest.fixture(scope='module')
def zkv():
    import stylus_zkvm_verifiers_amd as z
    assert z.device_count() >= 1, 'no gfx950 device visible'
    return z


@pytest.fixture(scope='module', autouse=True)
def no_gt_tables():
    """The built-in group of these routers sees a few seals per call; with the mapping fixed to lane pairs it would build its GT tables
    for them.  Same statuses without (the Miller path)."""
    old = os.environ.get('ZKV_GT_WINDOW_BITS')
    os.environ['ZKV_GT_WINDOW_BITS'] = '0'
    yield
    if old is None:
        del os.environ['ZKV_GT_WINDOW_BITS']
    else:
        os.environ['ZKV_GT_WINDOW_BITS'] = old


def _faults():
    from stylus_zkvm_verifiers_amd import _lib
    out = C.c_uint64(1 << 40)
    _lib.check(_lib.lib().zkv_diag_wait_faults(0, C.byref(out)), 'zkv_diag_wait_faults')
    return out.value


@pytest.fixture(scope='module')
def faults_before(zkv):
    return _faults()


@pytest.fixture(scope='module')
def real(real_proofs):
    r = real_proofs['risc0']
    return dict(root=H(r['control_root']), cid=H(r['bn254_control_id']), seal=H(r['seal']), image_id=H(r['image_id']),
                journal=H(r['journal_digest']), selector=H(r['selector']), claim=H(r['claim_digest']))


@pytest.fixture(scope='module')
def keys():
    return rm.Key(0x17B0), rm.Key(0x17B1), rm.Key(0x17B2)


def _dev_call(rt, seals, in_a, in_b=None, recv=True, shift=0):
    """Device-resident call on 260-byte seals.  Every buffer holds what the n seals need and `shift` bytes in front: shift = 1 hands the
    library odd addresses.  Statuses and received selectors are pre-filled with 255."""
    import torch
    dev = torch.device('cuda', 0)
    n = len(seals)
    assert all(len(s) == 260 for s in seals)
    up = lambda rows: torch.from_numpy(np.frombuffer(bytes(shift) + b''.join(rows), dtype=np.uint8).copy()).to(dev)
    d_s, d_a = up(seals), up(in_a)
    d_b = up(in_b) if in_b is not None else None
    d_st = torch.full((n,), 255, dtype=torch.uint8, device=dev)
    d_rv = torch.full((n, 4), 255, dtype=torch.uint8, device=dev)
    rt.verify_batch_dev(n, d_s.data_ptr() + shift, d_a.data_ptr() + shift, d_b.data_ptr() + shift if d_b is not None else 0, d_st.data_ptr(),
                        d_rv.data_ptr() if recv else 0, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return d_st.cpu().numpy(), d_rv.cpu().numpy()


def _tamper(seal, word, rng):
    """The seal with one coordinate word replaced by a random value (off the curve, or at least another proof)."""
    at = 4 + 32 * word
    return seal[:at] + m.be32(rng.randrange(m.P)) + seal[at + 32:]


def _merge(rng, queues):
    """One batch from per-route lists, shuffled but keeping every list's own order: the first and the last seal of a route in the batch
    are the first and the last of its list, which the stable partition makes the first and last slot of its group."""
    queues = [list(q) for q in queues if q]
    out = []
    while queues:
        q = rng.choice(queues)
        out.append(q.pop(0))
        if not q:
            queues.remove(q)
    return out


def _cols(items):
    return [s for s, _, _ in items], [a for _, a, _ in items], [b for _, _, b in items]


def _rerandomised(real, n, seed, mutate_every):
    """n seals of the real proof's route: re-randomisations of the real proof, some mutated into seals that must not verify."""
    from stylus_zkvm_verifiers_amd import synth
    seals, _, _, _ = synth.make_batch('risc0', real['seal'], n, seed, pool=4, mutate_every=mutate_every,
                                      classes=('flip_c_x', 'coord_plus_q', 'b_out_of_subgroup'))
    return [bytes(s) for s in seals]


def _check(got, want, what=''):
    st, rv = got
    want_st, want_rv, route = want
    bad = np.nonzero(st != want_st)[0]
    assert not len(bad), (what, bad.tolist(), route[bad].tolist(), st[bad].tolist(), want_st[bad].tolist())
    assert [bytes(x) for x in rv] == want_rv, what


# ---------------------------------------------------------------- 1. a built-in route is the reference's verifier
@pytest.mark.gpu
def test_builtin_route_is_pinned_and_the_reference_key_on_a_keyed_route(zkv, faults_before, real, verify_corpus):
    other_root, other_id = rm.params('pinned')
    rt = zkv.RiscZeroRouter([(real['root'], real['cid'])], [(REF_WORDS, other_root, other_id)])
    model = rm.Router([(real['root'], real['cid'])], [(REF_WORDS, other_root, other_id)])
    assert [r[0] for r in rt.routes()] == model.selectors and model.selectors[0] == real['selector'] and [r[1] for r in rt.routes()] == [False, True]
    assert rt.verify(real['seal'], real['image_id'], real['journal']) is True                      # ACCEPT, reference-pinned
    assert rt.verify_integrity(real['seal'], real['claim']) is True
    assert rt.last_route_counts() == [1, 0, 0, 0]
    oracle = ol.Risc0Oracle()
    assert oracle.initialize(real['root'], real['cid']) == 0 and oracle.get_selector() == real['selector']
    items = [(H(c['seal']), H(c['image_id']), H(c['journal_digest'])) for c in verify_corpus['cases'] if c['vm'] == 'risc0']
    items += [(s, real['image_id'], real['journal']) for s in _rerandomised(real, 64, 0x17B3, 7)]
    items += [(s, real['image_id'], real['journal'][:-1] + b'\0') for s in _rerandomised(real, 4, 0x17B4, 0)]      # another journal: refused
    ksel = model.selectors[1]
    items += [(ksel + real['seal'][4:], real['image_id'], real['journal']), (ksel + real['seal'][4:259], real['image_id'], real['journal'])]
    want_st, want_rv, n_foreign = [], [], 0
    for seal, iid, jd in items:
        st, rv = oracle.verify(seal, iid, jd)
        if st == 5 and seal[:4] == ksel:                 # the keyed route: the reference's key with other parameters refuses the real proof
            st, rv = (1 if len(seal) == 260 else 4), None
        elif st == 5:                                    # the one difference between a verifier and a router in front of it: no route instead of a mismatch
            st, n_foreign = 8, n_foreign + 1
        want_st.append(st); want_rv.append(bytes(rv or bytes(4)))
    assert {0, 1, 4, 8} <= set(want_st) and n_foreign >= 3 and want_st.count(0) >= 50
    mst, mrv, route = model.expect(*_cols(items))
    assert mst.tolist() == want_st and mrv == want_rv                                            # the model says the same as the oracle
    st, rv = rt.verify_batch(*_cols(items))
    assert st.tolist() == want_st and [bytes(x) for x in rv] == want_rv
    assert rt.last_route_counts() == rm.counts(route, 2)
    for (seal, iid, jd), ws, wr in zip(items[:40], want_st, want_rv):                              # the single-seal wrapper: a batch of one
        s = C.c_uint8(255); r = C.create_string_buffer(4)
        assert rt._L.zkv_risc0_router_verify(rt._h, seal, len(seal), iid, jd, C.byref(s), r) == 0
        assert (s.value, r.raw) == (ws, wr)
    assert sum(rt.last_stage_ms()) >= 0
    with pytest.raises(zkv.VerifierError) as ei:
        rt.verify(b'\x12\x34\x56\x78' + real['seal'][4:], real['image_id'], real['journal'])
    assert ei.value.status == 8 and ei.value.received == b'\x12\x34\x56\x78' and ei.value.revert == rm.selector_unknown_revert(b'\x12\x34\x56\x78')
    rt.close()


# ---------------------------------------------------------------- 2. several releases in one call, every mapping
def _keyed_queue(key, n, rng, integrity, ragged):
    """n seals of one keyed route: the first and the last valid, tampered words, foreign inputs and (ragged) wrong lengths between them."""
    def fresh():
        a = bytes(rng.randrange(256) for _ in range(32)); b = bytes(rng.randrange(256) for _ in range(32))
        return (key.prove_claim(a), a, None) if integrity else (key.prove(a, b), a, b)
    pool = [fresh() for _ in range(min(n, 3))]
    q = []
    for k in range(n):
        s, a, b = pool[k % len(pool)]
        if k in (0, n - 1) or k % 4 == 1:
            q.append((s, a, b))                                                                   # valid
        elif k % 4 == 2:
            q.append((_tamper(s, k % 8, rng), a, b))                                              # a tampered word
        elif k % 4 == 3:
            q.append((s, a[:-1] + bytes([a[-1] ^ 1]), b))                                         # a valid seal for other inputs
        elif ragged and k % 8 == 4:
            q.append((s[:259] if k % 16 == 4 else s + b'\0', a, b))                               # 259 / 261 bytes under the route's selector
        else:
            q.append((key.selector + bytes(256), a, b))                                           # A = B = C = (0, 0)
    return q


def _builtin_queues(real, model, rng, sizes, integrity, ragged):
    """The real proof's route gets re-randomisations (valid, and mutated ones); the other built-in routes the same seals under their own
    selectors, which their control roots refuse."""
    a, b = (real['claim'], None) if integrity else (real['image_id'], real['journal'])
    qs = []
    for r, n in enumerate(sizes):
        seals = _rerandomised(real, n, 0x17C0 + r, 5)
        q = [(model.selectors[r] + s[4:], a, b) for s in seals]
        if ragged and n >= 8:
            q[3] = (q[3][0][:259], a, b); q[5] = (q[5][0] + b'\0', a, b)
        if n >= 8:
            q[6] = (q[6][0], bytes(32), b)                                                        # other inputs
        qs.append(q)
    return qs


def _several(real, keys, builtin_params, sizes_b, sizes_k, seed, integrity, ragged):
    rng = random.Random(seed)
    model = rm.Router(builtin_params, [k.triple() for k in keys])
    a, b = (real['claim'], None) if integrity else (real['image_id'], real['journal'])
    queues = _builtin_queues(real, model, rng, sizes_b, integrity, ragged)
    queues += [_keyed_queue(k, n, rng, integrity, ragged) for k, n in zip(keys, sizes_k)]
    qx = [(bytes(rng.randrange(256) for _ in range(4)) + real['seal'][4:], a, b) for _ in range(4)]          # unknown selectors
    qx.append((keys[0].selector[:3] + bytes([keys[0].selector[3] ^ 1]) + real['seal'][4:], a, b))
    if ragged:
        qx += [(real['seal'][:3], a, b), (b'', a, b), (keys[1].selector[:3], a, b)]                       # shorter than 4 bytes
    items = _merge(rng, queues + [qx])
    seals, in_a, in_b = _cols(items)
    return model, items, model.expect(seals, in_a, None if integrity else in_b)


@pytest.fixture(scope='module')
def builtin_params(real):
    return [(real['root'], real['cid']), rm.params('b1'), rm.params('b2')]


@pytest.fixture(scope='module')
def router(zkv, keys, builtin_params):
    rt = zkv.RiscZeroRouter(builtin_params, [k.triple() for k in keys])
    yield rt
    rt.close()


@pytest.fixture(scope='module')
def several(real, keys, builtin_params):
    """Built-in routes with 64, 32 and 9 seals, keyed routes with 1, 33 and 32, unknown selectors, short seals: 179 seals."""
    return _several(real, keys, builtin_params, (64, 32, 9), (1, 33, 32), 0x17B5, integrity=False, ragged=True)


@pytest.mark.gpu
@pytest.mark.parametrize('lanes', [0, 2, 16, 64])
def test_several_releases_in_one_call(router, several, lanes):
    model, items, want = several
    want_st, want_rv, route = want
    assert router.routes() == [(r.selector, r.keyed, r.vk_digest) for r in model.routes]
    assert rm.counts(route, 6) == [64, 32, 9, 1, 33, 32, 5, 3] and 100 <= len(items) <= 200
    for r in (3, 4, 5):                                              # first and last slot of every keyed group hold a valid seal
        idx = np.nonzero(route == r)[0]
        assert want_st[idx[0]] == 0 and want_st[idx[-1]] == 0
    assert {0, 1, 4} <= set(want_st[route == 4].tolist()) and {0, 1, 4} <= set(want_st[route == 0].tolist())
    assert set(want_st[route == 1].tolist()) <= {1, 4} and 0 in want_st[route == 5]
    assert sorted({len(s) for s, _, _ in items}) == [0, 3, 259, 260, 261]
    router.set_lanes_per_proof(lanes)
    _check(router.verify_batch(*_cols(items)), want, lanes)
    assert router.last_route_counts() == rm.counts(route, 6)
    router.set_lanes_per_proof(0)


@pytest.mark.gpu
def test_several_count_blocks_and_a_chunked_keyed_group(zkv, router, several, keys, builtin_params, monkeypatch):
    """The 179 seals four times over under a seeded permutation: 716 seals are three 256-seal count blocks, so a slot is its route's first
    slot plus the scanned counts of the blocks in front plus the rank in its own block; the keyed groups hold 4, 132 and 128 seals.  Then
    a router created with 64-slot chunks: the built-in group runs in 7 chunks and the keyed group in 5 or more, on both ends of the
    mappings (one wavefront per proof pads nothing, lane pairs pad every group to 32)."""
    model, items, (want_st, want_rv, route) = several
    perm = list(range(4 * len(items)))
    random.Random(0x17B8).shuffle(perm)
    idx = [p % len(items) for p in perm]
    big = [items[i] for i in idx]
    want = (want_st[idx], [want_rv[i] for i in idx], route[idx])
    counts = [4 * c for c in rm.counts(route, 6)]
    assert len(big) == 716 and counts[:6] == [256, 128, 36, 4, 132, 128] and rm.counts(want[2], 6) == counts
    _check(router.verify_batch(*_cols(big)), want, 'defaults')
    assert router.last_route_counts() == counts
    monkeypatch.setenv('ZKV_CHUNK', '64')
    rt = zkv.RiscZeroRouter(builtin_params, [k.triple() for k in keys])
    try:
        for lanes in (0, 2):
            rt.set_lanes_per_proof(lanes)
            _check(rt.verify_batch(*_cols(big)), want, ('64-slot chunks', lanes))
            assert rt.last_route_counts() == counts
    finally:
        rt.close()


# ---------------------------------------------------------------- 3. verify_integrity and the device-resident call
@pytest.fixture(scope='module')
def several_integrity(real, keys, builtin_params):
    """Claim-digest rows on the same routes: keyed groups of 31, 64 and 5."""
    return _several(real, keys, builtin_params, (40, 3, 17), (31, 64, 5), 0x17B6, integrity=True, ragged=True)


@pytest.mark.gpu
def test_verify_integrity_batch(router, several_integrity):
    model, items, want = several_integrity
    seals, claims, _ = _cols(items)
    assert rm.counts(want[2], 6)[:6] == [40, 3, 17, 31, 64, 5] and {0, 1, 4, 8} <= set(want[0].tolist())
    _check(router.verify_integrity_batch(seals, claims), want)
    assert router.last_route_counts() == rm.counts(want[2], 6)
    # the same rows as verify rows are other claims: every seal that reached a pairing is refused, the rest keeps its status
    st, _ = router.verify_batch(seals, claims, claims)
    assert st.tolist() == [1 if s == 0 else int(s) for s in want[0]]


@pytest.mark.gpu
@pytest.mark.parametrize('integrity,shift,recv', [(False, 0, True), (True, 0, True), (False, 1, True), (True, 1, False)])
def test_device_resident_call(router, real, keys, builtin_params, integrity, shift, recv):
    model, items, want = _several(real, keys, builtin_params, (33, 2, 20), (32, 1, 35), 0x17B7 + integrity, integrity=integrity, ragged=False)
    seals, a, b = _cols(items)
    assert {0, 1, 8} <= set(want[0].tolist()) and 100 <= len(items) <= 200
    st, rv = _dev_call(router, seals, a, None if integrity else b, recv=recv, shift=shift)
    assert (st != 255).all()                                                                       # every status byte was written
    if recv:
        _check((st, rv), want, (integrity, shift))
    else:
        assert st.tolist() == want[0].tolist() and (rv == 255).all()                              # no received selectors asked for: none written
    assert router.last_route_counts() == rm.counts(want[2], 6)


# ---------------------------------------------------------------- 4. empty groups and singletons
@pytest.mark.gpu
def test_empty_groups_and_singletons(zkv, router, real, keys, builtin_params, several):
    model, items, (want_st, want_rv, route) = several
    pick = lambda cond: [i for i in range(len(items)) if cond(route[i])]
    for name, idx in (('no keyed seals', pick(lambda r: r < 3)), ('no built-in seals', pick(lambda r: r < 0 or r >= 3)),
                      ('only unknown selectors', pick(lambda r: r == rm.NOT_FOUND)), ('only short seals', pick(lambda r: r == rm.SHORT)),
                      ('an empty route between two', pick(lambda r: r in (0, 2, 3, 5))), ('one keyed route', pick(lambda r: r == 4))):
        sub = [items[i] for i in idx]
        assert sub, name
        st, rv = router.verify_batch(*_cols(sub))
        assert st.tolist() == want_st[idx].tolist() and [bytes(x) for x in rv] == [want_rv[i] for i in idx], name
        assert router.last_route_counts() == rm.counts(route[idx], 6), name
    # n = 1 on each kind of route through the single-seal wrappers
    singles = [pick(lambda r: r == 0)[0], pick(lambda r: r == 1)[0], pick(lambda r: r == 3)[0], pick(lambda r: r == 5)[-1], pick(lambda r: r == rm.NOT_FOUND)[0],
               pick(lambda r: r == rm.SHORT)[0]]
    for i in singles:
        seal, a, b = items[i]
        s = C.c_uint8(255); r = C.create_string_buffer(b'\xff' * 4, 4)
        assert router._L.zkv_risc0_router_verify(router._h, seal, len(seal), a, b, C.byref(s), r) == 0
        assert (s.value, r.raw) == (int(want_st[i]), want_rv[i]), i
        one = [0] * 8; one[int(route[i]) if route[i] >= 0 else (6 if route[i] == rm.NOT_FOUND else 7)] = 1
        assert router.last_route_counts() == one
    k = keys[2]
    claim = bytes(range(32))
    assert router.verify_integrity(k.prove_claim(claim), claim) is True                           # a keyed route alone, verify_integrity
    with pytest.raises(zkv.VerifierError) as ei:
        router.verify_integrity(k.prove_claim(claim), claim[::-1])
    assert ei.value.status == 1
    # routers of one kind of route only
    for builtin, keyed in ((builtin_params[:1], []), ([], [keys[1].triple()])):
        rt = zkv.RiscZeroRouter(builtin, keyed)
        mdl = rm.Router(builtin, keyed)
        sub = [items[i] for i in pick(lambda r: r in (0, 4, rm.NOT_FOUND, rm.SHORT))]
        want = mdl.expect(*_cols(sub))
        assert {0, 8} <= set(want[0].tolist())
        _check(rt.verify_batch(*_cols(sub)), want, (len(builtin), len(keyed)))
        assert rt.last_route_counts() == rm.counts(want[2], 1)
        rt.close()


# ---------------------------------------------------------------- 5. an invalid keyed key fails its own route only
@pytest.mark.gpu
def test_a_key_with_an_off_curve_ic_point_fails_its_own_route_only(zkv, keys, builtin_params, several):
    A, B, Cc = keys
    model, items, (good_st, good_rv, route) = several
    bad_words = rm.off_curve_ic(B.words)
    keyed = [A.triple(), (bad_words, B.control_root, B.control_id), Cc.triple()]
    rt = zkv.RiscZeroRouter(builtin_params, keyed)
    bad_model = rm.Router(builtin_params, keyed)
    bad_sel = bad_model.selectors[4]
    assert bad_sel != B.selector and [r[0] for r in rt.routes()] == bad_model.selectors            # other key words: another digest, another selector
    moved = [(bad_sel + s[4:] if s[:4] == B.selector else s, a, b) for s, a, b in items]           # route B's seals under the selector its bad key derives
    want = bad_model.expect(*_cols(moved))
    assert want[2].tolist() == route.tolist()
    on_b = route == 4
    assert set(want[0][on_b].tolist()) == {1, 4} and 0 in good_st[on_b]                            # every seal that reaches the key fails; length errors stay
    assert want[0][~on_b].tolist() == good_st[~on_b].tolist()
    got = rt.verify_batch(*_cols(moved))
    _check(got, want)
    # the neighbouring keyed route's last seal sits in the slot before the bad route's group, its first seal right behind it: both still pass
    for r in (3, 5):
        idx = np.nonzero(route == r)[0]
        assert got[0][idx[0]] == 0 and got[0][idx[-1]] == 0
    rt.set_lanes_per_proof(64)                                        # no padding between the groups: the neighbours are adjacent slots
    _check(rt.verify_batch(*_cols(moved)), want, 64)
    rt.close()


# ---------------------------------------------------------------- 6. resources
@pytest.mark.gpu
def test_no_wait_faults_across_the_module(zkv, faults_before):
    assert _faults() == faults_before

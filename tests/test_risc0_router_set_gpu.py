"""RISC Zero router with a set route on the GPU (include/zkv_risc0_router_set.h).  Every expectation is the model of
tests/risc0_router_set_model.py: risc0_router_model.Router behind its routing rule, set_inclusion_model.SetVerifier with that router as
its inner verifier, the pairing by the C oracle -- parity unpinned.  Root proofs are trapdoor proofs of keyed routes, so that a valid
root seal exists for any root."""
import ctypes as C
import os
import random

import numpy as np
import pytest

import risc0_router_model as rm
import risc0_router_set_model as rsm
import set_inclusion_model as sm
import spec_model as m

H = bytes.fromhex
SET_ID = m.sha256(b'risc0 router set gpu tests: set builder image id')
OK, FAILED, INVALID, NOT_FOUND = 0, 1, 4, 8
SHIFTS = (0, 1, 4, 16)


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
    return dict(root=H(r['control_root']), cid=H(r['bn254_control_id']), seal=H(r['seal']), image_id=H(r['image_id']), journal=H(r['journal_digest']))


@pytest.fixture(scope='module')
def keys():
    return rm.Key(0x17D0), rm.Key(0x17D1)


@pytest.fixture(scope='module')
def model(real, keys):
    return rsm.SetRouter(SET_ID, [(real['root'], real['cid'])], [k.triple() for k in keys])


@pytest.fixture()
def router(zkv, real, keys, model):
    rt = zkv.RiscZeroSetRouter(SET_ID, [(real['root'], real['cid'])], [k.triple() for k in keys])
    assert [r[0] for r in rt.routes()] == model.selectors
    yield rt
    rt.close()


def rand32(rng):
    return bytes(rng.randrange(256) for _ in range(32))


def root_seal(key, root):
    """A valid seal of keyed route `key` for verify(seal, SET_ID, sha256(SET_ID || root))."""
    return key.prove(SET_ID, sm.root_journal(SET_ID, root))


def claim(a, b):
    return m.receipt_claim_ok_digest(a, b)


def _ragged_dev(rt, seals, in_a, in_b=None, shift=0, recv=True):
    """zkv_risc0_router_verify_ragged_dev: the blob `shift` bytes past an allocation's (256-byte aligned) base, the other byte rows one byte
    past theirs.  Statuses and received selectors are pre-filled with 255."""
    import torch
    dev = torch.device('cuda', 0)
    n = len(seals)
    up = lambda data, sh: torch.from_numpy(np.frombuffer(bytes(sh) + data + b'\0', dtype=np.uint8).copy()).to(dev)
    blob = b''.join(seals)
    off = np.zeros(n + 1, dtype=np.uint64)
    off[1:] = np.cumsum([len(s) for s in seals], dtype=np.uint64)
    d_s, d_a = up(blob, shift), up(b''.join(in_a), 1)
    d_b = up(b''.join(in_b), 1) if in_b is not None else None
    d_off = torch.from_numpy(off.view(np.int64)).to(dev)
    d_st = torch.full((n,), 255, dtype=torch.uint8, device=dev)
    d_rv = torch.full((n, 4), 255, dtype=torch.uint8, device=dev)
    rt.verify_ragged_dev(n, d_s.data_ptr() + shift, d_off.data_ptr(), len(blob), d_a.data_ptr() + 1, d_b.data_ptr() + 1 if d_b is not None else 0,
                         d_st.data_ptr(), d_rv.data_ptr() if recv else 0, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return d_st.cpu().numpy(), d_rv.cpu().numpy()


def _check(got, want, what=''):
    st, rv = got
    want_st, want_rv, route = want
    bad = np.nonzero(st != want_st)[0]
    assert not len(bad), (what, bad.tolist(), route[bad].tolist(), st[bad].tolist(), want_st[bad].tolist())
    assert [bytes(x) for x in rv] == want_rv, what


def _tree(rng, model, key, leaves):
    """An honest tree of `leaves` claims under one valid root seal of `key`: [(seal, image id, journal digest)], the root seal, the root."""
    ab = [(rand32(rng), rand32(rng)) for _ in range(leaves)]
    root, paths = sm.tree_paths([sm.leaf(claim(a, b)) for a, b in ab])
    rs = root_seal(key, root)
    return [(model.encode_seal(p, rs), a, b) for (a, b), p in zip(ab, paths)], rs, root


# ---------------------------------------------------------------- 1. a mixed batch, forwards and reversed, four entry points
@pytest.fixture(scope='module')
def mixed(real, keys, model):
    """[(name, seal, image id, journal digest)] and the claim that names a stored root."""
    rng = random.Random(0x17D2)
    word = lambda v: int(v).to_bytes(32, 'big')
    patch = lambda s, at, d: s[:at] + d + s[at + len(d):]
    items = []
    add = lambda name, seal, a, b: items.append((name, bytes(seal), bytes(a), bytes(b)))
    # direct seals: the built-in route (the real proof and tampered copies), two keyed routes
    rs, ia, jd = real['seal'], real['image_id'], real['journal']
    add('built-in, real', rs, ia, jd)
    for w in (0, 3, 6):
        at = 4 + 32 * w
        add('built-in, word %d replaced' % w, patch(rs, at, m.be32(rng.randrange(m.P))), ia, jd)
    add('built-in, other journal', rs, ia, rand32(rng))
    for k, key in enumerate(keys):
        for _ in range(3):
            a, b = rand32(rng), rand32(rng)
            add('keyed %d, valid' % k, key.prove(a, b), a, b)
        add('keyed %d, other image id' % k, key.prove(a, b), rand32(rng), b)
        add('keyed %d, 261 bytes' % k, key.prove(a, b) + b'\0', a, b)
    add('unknown selector', b'\xde\xad\xbe\xef' + rs[4:], ia, jd)
    add('3 bytes', rs[:3], ia, jd)
    # set seals over 7 distinct valid keyed root seals (both keyed routes), stragglers among them
    trees = []
    for t, leaves in enumerate((1, 2, 3, 5, 6, 7, 9)):
        tr, seal_t, root_t = _tree(rng, model, keys[t & 1], leaves)
        trees.append((tr, seal_t, root_t))
        for q, (s, a, b) in enumerate(tr):
            add('tree %d leaf %d' % (t, q), s, a, b)
        if leaves >= 3:                                              # stragglers: the tree's seal in front of another claim, or of a damaged path
            add('tree %d straggler: another journal' % t, tr[1][0], tr[1][1], rand32(rng))
            add('tree %d straggler: a sibling changed' % t, patch(tr[2][0], 4 + 128, rand32(rng)), tr[2][1], tr[2][2])
            add('tree %d the same straggler again (verified on its own again)' % t, tr[1][0], tr[1][1], items[-2][3])
    tr, seal_t, _ = trees[4]
    s, a, b = tr[0]
    path = [s[4 + 128 + 32 * q:4 + 160 + 32 * q] for q in range(int.from_bytes(s[100:132], 'big'))]
    # root seals the router answers without a pairing, or with another route's
    add('root seal of the built-in route (the real proof: another claim)', model.encode_seal(path, rs), a, b)
    add('root seal of keyed route 0 under keyed route 1 selector', model.encode_seal(path, keys[1].selector + seal_t[4:]), a, b)
    add('root seal with an unknown selector', model.encode_seal(path, b'\xca\xfe\xf0\x0d' + seal_t[4:]), a, b)
    for n in (3, 259, 261):
        add('root seal of %d bytes' % n, model.encode_seal(path, (seal_t + bytes(8))[:n]), a, b)
    add('nested: the root seal is a set seal', model.encode_seal(path, s), a, b)
    # every non-canonical defect over a seal that verifies
    k = len(path)
    l_at = 4 + 128 + 32 * k
    add('first word 0x40', patch(s, 4, word(0x40)), a, b)
    add('path offset 0x60', patch(s, 36, word(0x60)), a, b)
    add('root seal offset 32 more', patch(s, 68, word(0x60 + 32 * k + 32)), a, b)
    add('path length one more', patch(s, 100, word(k + 1)), a, b)
    add('path length + 2^32', patch(s, 100 + 27, b'\1'), a, b)
    add('root seal length one more', patch(s, l_at, word(261)), a, b)
    add('root seal length + 2^32', patch(s, l_at + 27, b'\1'), a, b)
    add('padding byte set', patch(s, len(s) - 1, b'\1'), a, b)
    add('last byte missing', s[:-1], a, b)
    add('one trailing word', s + bytes(32), a, b)
    add('set selector alone', s[:4], a, b)
    # depths at the limit
    deep = [rand32(rng) for _ in range(65)]
    a64, b64 = rand32(rng), rand32(rng)
    add('depth 64', model.encode_seal(deep[:64], root_seal(keys[0], sm.walk(claim(a64, b64), deep[:64]))), a64, b64)
    add('depth 65', model.encode_seal(deep, root_seal(keys[0], sm.walk(claim(a64, b64), deep))), a64, b64)
    # a claim with an empty root seal
    sa, sb = rand32(rng), rand32(rng)
    spath = [rand32(rng) for _ in range(2)]
    add('empty root seal', model.encode_seal(spath, b''), sa, sb)
    stored_root = sm.walk(claim(sa, sb), spath)
    return items, (stored_root, root_seal(keys[1], stored_root))


def _run_all(rt, model, items, what):
    seals, in_a, in_b = [x[1] for x in items], [x[2] for x in items], [x[3] for x in items]
    claims = [claim(a, b) for a, b in zip(in_a, in_b)]
    model.reset_counts()
    want = model.expect(seals, in_a, in_b)
    want_counts = (int((want[2] == rsm.SET).sum()), len(model.root_seals), model.pairings, model.lookups)
    model.reset_counts()
    want_i = model.expect(seals, claims)
    assert want_i[0].tolist() == want[0].tolist() and want_i[1] == want[1]
    for name, got in (('host verify', rt.verify_batch(seals, in_a, in_b)), ('host integrity', rt.verify_integrity_batch(seals, claims)),
                      ('ragged verify', _ragged_dev(rt, seals, in_a, in_b, shift=1)), ('ragged integrity', _ragged_dev(rt, seals, claims, None, shift=4))):
        _check(got, want, (what, name))
        assert rt.set_last_counts() == want_counts, (what, name)
        assert rt.last_route_counts() == model.counts(want[2]), (what, name)
    return want


@pytest.mark.gpu
def test_mixed_batch_forwards_and_reversed(zkv, faults_before, router, model, mixed):
    items, (stored_root, stored_seal) = mixed
    model.set.roots.clear()
    want = _run_all(router, model, items, 'forwards')
    by_name = {x[0]: int(s) for x, s in zip(items, want[0])}
    assert by_name['empty root seal'] == FAILED and by_name['depth 64'] == OK and by_name['depth 65'] == INVALID and by_name['nested: the root seal is a set seal'] == INVALID
    assert by_name['root seal with an unknown selector'] == NOT_FOUND and by_name['root seal of 259 bytes'] == INVALID and by_name['root seal of 3 bytes'] == INVALID
    assert {OK, FAILED, INVALID, NOT_FOUND} == set(want[0].tolist()) and (want[0] == OK).sum() >= 40
    assert len(model.root_seals) >= 7 + 6 and model.pairings > len(model.root_seals)            # stragglers ran on their own
    _run_all(router, model, items[::-1], 'reversed')
    # the stored root: submitted through the router, then the claim with the empty root seal is OK
    assert not router.has_root(stored_root)
    assert router.submit_root(stored_root, stored_seal[:-1] + bytes([stored_seal[-1] ^ 1])) == (FAILED, bytes(4)) and not router.has_root(stored_root)
    assert model.submit_root(stored_root, stored_seal)[0] == OK
    assert router.submit_root(stored_root, stored_seal) == (OK, bytes(4)) and router.has_root(stored_root)
    want = _run_all(router, model, items, 'after submit_root')
    assert {x[0]: int(s) for x, s in zip(items, want[0])}['empty root seal'] == OK
    # one seal at a time through the trait-shaped calls
    for name, seal, a, b in items[::9]:
        st, rv = model.verify(seal, a, b)
        try:
            got = (OK if router.verify(seal, a, b) else None, bytes(4))
        except zkv.VerifierError as e:
            got = (e.status, bytes(e.received or bytes(4)))
        assert got == (st, rv), name
    model.set.roots.clear()
    assert _faults() == faults_before


# ---------------------------------------------------------------- 2. shapes: batch sizes, blob shifts, depths
@pytest.fixture(scope='module')
def pool(keys, model):
    """Claims of every depth 1 .. 64 under ONE root: a caterpillar tree -- claim A climbs 64 siblings, and sibling k is the leaf of claim
    B_k, whose path is A's running node below it and the siblings above -- so that one pairing answers all of them and a wrong hash at any
    depth shows.  Beside them a tree of one leaf (depth 0), a path of 65, and claims with one damaged sibling (stragglers).  Each item comes
    with the model's answer, computed once."""
    rng = random.Random(0x17D3)
    ab = [(rand32(rng), rand32(rng)) for _ in range(65)]
    leaves = [sm.leaf(claim(a, b)) for a, b in ab]
    run = [leaves[0]]                                                # run[k]: A's node below sibling k + 1
    for k in range(64):
        run.append(sm.node(run[k], leaves[k + 1]))
    root = run[64]
    rs = root_seal(keys[0], root)
    items = [(model.encode_seal(leaves[1:], rs),) + ab[0]]           # A: depth 64
    for k in range(1, 65):                                           # B_k: depth 65 - k
        items.append((model.encode_seal([run[k - 1]] + leaves[k + 1:], rs),) + ab[k])
    depths = [64] + [65 - k for k in range(1, 65)]
    a0, b0 = rand32(rng), rand32(rng)
    items.append((model.encode_seal([], root_seal(keys[1], sm.leaf(claim(a0, b0)))), a0, b0)); depths.append(0)
    items.append((model.encode_seal([rand32(rng) for _ in range(65)], rs),) + ab[0]); depths.append(65)
    for k in (0, 45, 64):                                            # depths 64, 20 and 1 with the last sibling damaged
        s, a, b = items[k]
        items.append((s[:4 + 128 + 32 * (depths[k] - 1)] + rand32(rng) + s[4 + 128 + 32 * depths[k]:], a, b)); depths.append(depths[k])
    assert {0, 1, 20, 64, 65} <= set(depths)
    want = [model.verify(s, a, b) for s, a, b in items]
    assert [w[0] for w in want] == [OK] * 66 + [INVALID] + [FAILED] * 3
    return items, want, depths


@pytest.mark.gpu
@pytest.mark.parametrize('n', [1, 63, 64, 65, 200])
def test_batch_sizes_blob_shifts_and_depths(zkv, faults_before, router, pool, n):
    items, want, depths = pool
    for shift in SHIFTS:
        k = SHIFTS.index(shift)
        must = [65, 66, 0, 45, 64]                                   # depths 0, 65, 64, 20 and 1 come first, then a walk over the pool (11 and 70 are coprime)
        pick = [must[(i + k) % 5] if i < 5 else (k + 11 * i) % len(items) for i in range(n)]
        seals, in_a, in_b = [items[p][0] for p in pick], [items[p][1] for p in pick], [items[p][2] for p in pick]
        if shift in (0, 4):
            got = _ragged_dev(router, seals, in_a, in_b, shift=shift)
        else:
            got = _ragged_dev(router, seals, [claim(a, b) for a, b in zip(in_a, in_b)], None, shift=shift)
        assert got[0].tolist() == [want[p][0] for p in pick], (n, shift, [depths[p] for p in pick])
        assert not got[1].any()
        assert n < 5 or {0, 1, 20, 64, 65} <= {depths[p] for p in pick}
    assert _faults() == faults_before


# ---------------------------------------------------------------- 3. root-seal identity
@pytest.mark.gpu
def test_identical_and_distinct_root_seals(zkv, faults_before, router, model, keys):
    rng = random.Random(0x17D4)
    # 200 claims of one tree: one root seal, one job
    tr, _, _ = _tree(rng, model, keys[0], 200)
    seals, in_a, in_b = [x[0] for x in tr], [x[1] for x in tr], [x[2] for x in tr]
    model.reset_counts()
    want = model.expect(seals, in_a, in_b)
    assert want[0].tolist() == [OK] * 200 and (len(model.root_seals), model.pairings) == (1, 1)
    _check(router.verify_batch(seals, in_a, in_b), want, 'one tree')
    assert router.set_last_counts() == (200, 1, 1, 0)
    assert router.last_route_counts() == [0, 0, 0, 200, 0, 0]
    # 200 claims with 200 root seals (each of an unknown selector of its own, so that every claim's answer is its own): 200 jobs
    body = root_seal(keys[0], bytes(32))[4:]
    sels = [bytes([0xE0, i, 0xA5, 0x5A]) for i in range(200)]
    seals = [model.encode_seal([rand32(rng)] * (i % 3), sel + body) for i, sel in enumerate(sels)]
    assert model.verify(seals[0], in_a[0], in_b[0]) == (NOT_FOUND, sels[0]) and model.verify(seals[199], in_a[199], in_b[199]) == (NOT_FOUND, sels[199])
    for shift in (0, 1):
        st, rv = _ragged_dev(router, seals, in_a, in_b, shift=shift)
        assert st.tolist() == [NOT_FOUND] * 200 and [bytes(x) for x in rv] == sels and router.set_last_counts() == (200, 200, 200, 0)
    # never merged: a pair that differs only in the last byte, and a 259 / 260 prefix pair (the 260-byte seal ends in the zero its padding
    # would hold); the answers differ, so a merge would show
    a, b = in_a[0], in_b[0]
    root = sm.leaf(claim(a, b))
    good = root_seal(keys[1], root)
    assert good[-1] != 0
    z = good[:-1] + b'\0'                                            # another C.y: refused
    pairs = [good, good[:-1] + bytes([good[-1] ^ 1]), z[:259], z, good, z[:259]]
    seals = [model.encode_seal([], s) for s in pairs]
    model.reset_counts()
    want = model.expect(seals, [a] * 6, [b] * 6)
    assert want[0].tolist() == [OK, FAILED, INVALID, FAILED, OK, INVALID] and model.pairings == 4
    for order in (list(range(6)), list(range(6))[::-1]):
        st, rv = router.verify_batch([seals[i] for i in order], [a] * 6, [b] * 6)
        assert st.tolist() == [int(want[0][i]) for i in order] and router.set_last_counts() == (6, 4, 4, 0)
    assert _faults() == faults_before


@pytest.mark.gpu
@pytest.mark.parametrize('n', [65, 200])
def test_collision_path_gives_the_same_representatives(zkv, faults_before, router, model, keys, n):
    """With mask 0 every claim starts at table slot 0 and probes linearly past the other seals' slots; the representatives are the ones
    the full fingerprint gives, the lowest index carrying those bytes."""
    rng = random.Random(0x17D5 + n)
    body = bytes(rng.randrange(256) for _ in range(256))
    distinct = [keys[0].selector + body, keys[0].selector + body[:-1] + bytes([body[-1] ^ 1]), (keys[0].selector + body)[:259], keys[1].selector + body, b'\1\2\3\4\5']
    which = [rng.randrange(5) for _ in range(n)]
    assert set(which) == set(range(5))
    seals = [model.encode_seal([rand32(rng)] * (i % 4), distinct[w]) for i, w in enumerate(which)]
    seals[3] = distinct[0]                                           # a Groth16 seal, an empty root seal and a malformed seal carry no root seal
    seals[7] = model.encode_seal([], b'')
    seals[11] = seals[11][:-1]
    none = 0xFFFFFFFF
    firsts = {}
    for i, w in enumerate(which):                                   # (a representative is itself a claim with that root seal)
        if i not in (3, 7, 11):
            firsts.setdefault(w, i)
    want = [none if i in (3, 7, 11) else firsts[w] for i, w in enumerate(which)]
    for shift in (0, 1):
        full = router.diag_groups(seals, 0xFFFFFFFF, blob_shift=shift).tolist()
        zero = router.diag_groups(seals, 0, blob_shift=shift).tolist()
        assert full == want and zero == want, (n, shift)
    assert router.diag_groups(seals, 0x3).tolist() == want           # four starting slots for five seals
    assert _faults() == faults_before


# ---------------------------------------------------------------- 4. the ragged call on a router without a set route
@pytest.mark.gpu
def test_ragged_call_on_a_router_without_a_set_route(zkv, faults_before, real, keys):
    import torch
    rng = random.Random(0x17D6)
    plain = zkv.RiscZeroRouter([(real['root'], real['cid'])], [k.triple() for k in keys])
    pm = rm.Router([(real['root'], real['cid'])], [k.triple() for k in keys])
    items = [(real['seal'], real['image_id'], real['journal'])]
    for k in keys:
        for _ in range(4):
            a, b = rand32(rng), rand32(rng)
            items.append((k.prove(a, b), a, b))
        items.append((k.prove(a, b), a, rand32(rng)))
    items.append((b'\xde\xad\xbe\xef' + real['seal'][4:], real['image_id'], real['journal']))
    items.append((rsm.SetRouter(SET_ID, [(real['root'], real['cid'])]).set_selector + bytes(256), real['image_id'], real['journal']))     # no set route here
    rng.shuffle(items)
    seals, in_a, in_b = [x[0] for x in items], [x[1] for x in items], [x[2] for x in items]
    want = pm.expect(seals, in_a, in_b)
    assert {OK, FAILED, NOT_FOUND} <= set(want[0].tolist())
    # equal to verify_batch_dev on the same 260-byte seals
    dev = torch.device('cuda', 0)
    up = lambda rows: torch.from_numpy(np.frombuffer(b''.join(rows), dtype=np.uint8).copy()).to(dev)
    n = len(seals)
    d_s, d_a, d_b = up(seals), up(in_a), up(in_b)
    d_st = torch.full((n,), 255, dtype=torch.uint8, device=dev); d_rv = torch.full((n, 4), 255, dtype=torch.uint8, device=dev)
    plain.verify_batch_dev(n, d_s.data_ptr(), d_a.data_ptr(), d_b.data_ptr(), d_st.data_ptr(), d_rv.data_ptr(), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    fixed = (d_st.cpu().numpy(), d_rv.cpu().numpy())
    _check(fixed, want, 'verify_batch_dev')
    counts = plain.last_route_counts()
    for shift in SHIFTS:
        got = _ragged_dev(plain, seals, in_a, in_b, shift=shift)
        assert got[0].tolist() == fixed[0].tolist() and got[1].tolist() == fixed[1].tolist(), shift
        assert plain.last_route_counts() == counts
    got = _ragged_dev(plain, seals, [claim(a, b) for a, b in zip(in_a, in_b)], None, shift=1, recv=False)
    assert got[0].tolist() == fixed[0].tolist() and (got[1] == 255).all()
    # ragged lengths: answered as the host batch call answers them
    cut = [(s + bytes(8))[:ln] for s, ln in zip(seals, [3, 4, 259, 261, 0, 260, 1, 292, 260, 259, 261, 4, 3])]
    want = pm.expect(cut, in_a, in_b)
    host = plain.verify_batch(cut, in_a, in_b)
    _check(host, want, 'host batch, ragged')
    assert {INVALID, OK} <= set(want[0].tolist())
    for shift in (0, 1):
        _check(_ragged_dev(plain, cut, in_a, in_b, shift=shift), want, ('ragged', shift))
    plain.close()
    assert _faults() == faults_before


# ---------------------------------------------------------------- 5. more than one chunk
@pytest.mark.gpu
def test_a_batch_that_spans_two_chunks_verifies_a_group_once_per_chunk(zkv, faults_before, router, model, keys):
    """2^20 + 3 integrity claims at depth 0: stored-root lookups of one digest (an empty root seal; nothing was submitted) around three
    groups, each a claim under its own root seal, with members on both sides of the chunk boundary; the raw C call on numpy buffers."""
    from stylus_zkvm_verifiers_amd import _lib
    rng = random.Random(0x17D7)
    n = (1 << 20) + 3
    digests = np.zeros((n, 32), dtype=np.uint8)
    digests[:] = np.frombuffer(rand32(rng), dtype=np.uint8)
    background = np.frombuffer(model.encode_seal([], b''), dtype=np.uint8)
    groups = []
    for g in range(3):
        d = rand32(rng)
        groups.append((d, np.frombuffer(model.encode_seal([], root_seal(keys[g & 1], sm.leaf(d))), dtype=np.uint8)))
    at = {5: 0, 7: 1, 9: 2, 11: 0, (1 << 20) - 1: 1, 1 << 20: 0, (1 << 20) + 1: 1, (1 << 20) + 2: 2}
    lens = np.full(n, len(background), dtype=np.uint64)
    for i, g in at.items():
        lens[i] = len(groups[g][1])
        digests[i] = np.frombuffer(groups[g][0], dtype=np.uint8)
    off = np.zeros(n + 1, dtype=np.uint64)
    off[1:] = np.cumsum(lens)
    blob = np.empty(int(off[n]), dtype=np.uint8)
    prev = 0
    for i in sorted(at) + [n]:
        if i > prev:
            blob[int(off[prev]):int(off[i])] = np.tile(background, i - prev)
        if i < n:
            blob[int(off[i]):int(off[i + 1])] = groups[at[i]][1]
        prev = i + 1
    st = np.full(n, 255, dtype=np.uint8); rv = np.full((n, 4), 255, dtype=np.uint8)
    _lib.check(router._L.zkv_risc0_router_verify_integrity_batch(router._h, n, blob.ctypes.data, off.ctypes.data, digests.ctypes.data, st.ctypes.data, rv.ctypes.data),
               'zkv_risc0_router_verify_integrity_batch')
    want = np.full(n, FAILED, dtype=np.uint8)
    want[list(at)] = OK
    for i, g in at.items():                                          # the model agrees about the eight claims and about a background claim
        assert model.verify_integrity(bytes(groups[g][1]), groups[g][0]) == (OK, bytes(4))
    assert model.verify_integrity(bytes(background), bytes(digests[0])) == (FAILED, bytes(4))
    assert (st == want).all() and not rv.any()
    # three groups in the first chunk, three in the second: a group that spans the boundary is verified once per chunk
    assert router.set_last_counts() == (n, 6, 6, n - len(at))
    assert router.last_route_counts() == [0, 0, 0, n, 0, 0]
    assert _faults() == faults_before

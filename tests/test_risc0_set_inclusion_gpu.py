"""RISC Zero set-inclusion receipts on the device (include/zkv_risc0_set_inclusion.h): the hash kernel against every hash case of
tests/golden/set_inclusion_cases.json, and the keyed and real-key batches of that fixture through the host call, the device-resident call
and verify_seals.  The expected statuses are those of tests/set_inclusion_model.py (PARITY UNPINNED: the reference holds no set verifier)."""
import json
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
H = bytes.fromhex
OK, FAILED, INVALID_PROOF_DATA, SELECTOR_MISMATCH = 0, 1, 4, 5
STORED = 0xFFFFFFFF


@pytest.fixture(scope='module')
def fx():
    return json.load(open(os.path.join(HERE, 'golden', 'set_inclusion_cases.json')))


def _keyed(fx):
    from stylus_zkvm_verifiers_amd import RiscZeroSetInclusionVerifier
    k = fx['keyed']
    return RiscZeroSetInclusionVerifier(H(k['control_root']), H(k['bn254_control_id']), H(fx['set_builder_image_id']), vk_words=H(k['vk_words']),
                                        root_selector=H(k['root_selector']))


@pytest.fixture(scope='module')
def kv(fx):
    """The keyed verifier of the fixture with the stored tree's root submitted."""
    v = _keyed(fx)
    s = fx['keyed']['stored']
    assert v.submit_root(H(s['root']), H(s['seal'])) == (OK, bytes(4))
    yield v
    v.close()


@pytest.fixture(scope='module')
def rv0(fx):
    from stylus_zkvm_verifiers_amd import RiscZeroSetInclusionVerifier
    r = fx['real']
    v = RiscZeroSetInclusionVerifier(H(r['control_root']), H(r['bn254_control_id']), H(fx['set_builder_image_id']))
    yield v
    v.close()


def _want(claims, field='status'):
    st = np.array([c[field] for c in claims], dtype=np.uint8)
    rv = np.array([list(H(c['recv'])) for c in claims], dtype=np.uint8).reshape(-1, 4)
    return st, rv


def _host(v, claims, seals, integrity=False):
    paths = [H(c['path']) for c in claims]
    idx = [c['root_idx'] for c in claims]
    if integrity:
        return v.verify_integrity_batch([H(c['claim']) for c in claims], paths, idx, seals)
    return v.verify_batch([H(c['image_id']) for c in claims], [H(c['journal_digest']) for c in claims], paths, idx, seals)


def _dev(v, claims, seals, integrity=False, stream=True, shift=0):
    """The device-resident call on rows that torch holds: 260-byte seal rows (every seal of `seals` must be 260 bytes), the path blob
    `shift` bytes into its allocation, outputs between sentinel bytes."""
    import torch
    dev = torch.device('cuda', 0)
    n = len(claims)
    up = lambda a: torch.from_numpy(np.array(a)).to(dev)           # (a writable copy)
    a = up(np.frombuffer(b''.join(H(c['claim'] if integrity else c['image_id']) for c in claims), dtype=np.uint8))
    b = None if integrity else up(np.frombuffer(b''.join(H(c['journal_digest']) for c in claims), dtype=np.uint8))
    blob = b''.join(H(c['path']) for c in claims)
    off = np.zeros(n + 1, dtype=np.uint32)
    off[1:] = np.cumsum([len(c['path']) // 64 for c in claims])
    d_blob = up(np.frombuffer(bytes(shift) + blob + bytes(64), dtype=np.uint8))
    d_off = up(off.view(np.int32))
    d_idx = up(np.array([c['root_idx'] for c in claims], dtype=np.uint32).view(np.int32))
    assert all(len(s) == 260 for s in seals)
    d_seals = up(np.frombuffer(b''.join(seals) + bytes(4), dtype=np.uint8))
    st = torch.full((n + 128,), 0xA5, dtype=torch.uint8, device=dev)
    rv = torch.full((4 * n + 128,), 0xA5, dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()
    s = torch.cuda.Stream() if stream else None
    v.verify_batch_dev(n, a.data_ptr(), 0 if integrity else b.data_ptr(), d_blob.data_ptr() + shift, d_off.data_ptr(), int(off[-1]), d_idx.data_ptr(),
                       len(seals), d_seals.data_ptr(), st.data_ptr() + 64, rv.data_ptr() + 64, s.cuda_stream if s else 0)
    if s: s.synchronize()
    v.synchronize()
    st, rv = st.cpu().numpy(), rv.cpu().numpy()
    for buf, m in ((st, n), (rv, 4 * n)):                           # outputs outside status / recv keep the sentinel
        assert (buf[:64] == 0xA5).all() and (buf[64 + m:] == 0xA5).all()
    return st[64:64 + n], rv[64:64 + 4 * n].reshape(n, 4)


# ---------------------------------------------------------------- the hash kernel alone
@pytest.fixture(scope='module')
def hv(fx):
    v = _keyed(fx)
    yield v
    v.close()


@pytest.mark.parametrize('shift', [0, 1, 4, 16])
@pytest.mark.parametrize('n', [1, 63, 64, 65, 200])
def test_hash_kernel_gives_the_fixture_roots(fx, hv, n, shift):
    walks = fx['hash']['walks']
    assert len(walks) == 43
    pick = [walks[(7 * n + k) % len(walks)] for k in range(n)]      # every case is reached: 200 claims cycle the list, the small batches start at different cases
    want = np.array([list(H(c['root'])) if len(c['path']) // 64 <= 64 else [0] * 32 for c in pick], dtype=np.uint8)
    got = hv.diag_roots([H(c['image_id']) for c in pick], [H(c['journal_digest']) for c in pick], [H(c['path']) for c in pick], blob_shift=shift)
    assert (got == want).all(), [c['name'] for c, g, w in zip(pick, got, want) if (g != w).any()]
    got = hv.diag_roots([H(c['claim']) for c in pick], None, [H(c['path']) for c in pick], blob_shift=shift)        # the integrity method: no SHA-256 chain
    assert (got == want).all()


def test_hash_kernel_covers_every_case_of_the_fixture(fx, hv):
    walks = fx['hash']['walks']
    got = hv.diag_roots([H(c['image_id']) for c in walks], [H(c['journal_digest']) for c in walks], [H(c['path']) for c in walks])
    for c, g in zip(walks, got):
        assert bytes(g) == (H(c['root']) if c['name'] != 'depth65' else bytes(32)), c['name']
    # leaves are walks of depth 0; nodes are walks of depth 1 from a leaf
    for c in fx['hash']['leaf']:
        assert bytes(hv.diag_roots([H(c['claim'])], None, [b''])[0]) == H(c['leaf'])


# ---------------------------------------------------------------- the keyed batches through every entry point
def test_keyed_batch_through_the_host_call(fx, kv):
    k = fx['keyed']
    seals = [H(s) for s in k['root_seals']]
    for claims in (k['claims'], k['claims'][::-1]):
        st, rv = _host(kv, claims, seals)
        wst, wrv = _want(claims)
        assert (st == wst).all(), [(c['kind'], int(a), int(b)) for c, a, b in zip(claims, st, wst) if a != b]
        assert (rv == wrv).all()
    assert {OK, FAILED, INVALID_PROOF_DATA, SELECTOR_MISMATCH} == set(int(x) for x in wst)
    st, rv = _host(kv, k['claims'], seals, integrity=True)
    assert (st == wst[::-1]).all() and (rv == wrv[::-1]).all()


def _dev_view(k):
    """The fixture's batch as the device-resident call can hold it: every root seal a 260-byte row, so the claim under the 259-byte seal
    is left out and the seal's row is zero."""
    claims = [c for c in k['claims'] if c['kind'] != 'short_seal']
    seals = [H(s) if len(s) == 520 else bytes(260) for s in k['root_seals']]
    return claims, seals


@pytest.mark.parametrize('shift', [0, 4])
def test_keyed_batch_through_the_device_resident_call(fx, kv, shift):
    claims, seals = _dev_view(fx['keyed'])
    for cl in (claims, claims[::-1]):
        st, rv = _dev(kv, cl, seals, shift=shift)
        wst, wrv = _want(cl)
        assert (st == wst).all(), [(c['kind'], int(a), int(b)) for c, a, b in zip(cl, st, wst) if a != b]
        assert (rv == wrv).all()
    st, rv = _dev(kv, claims, seals, integrity=True, stream=False, shift=shift)      # the context's own stream
    wst, wrv = _want(claims)
    assert (st == wst).all() and (rv == wrv).all()


def test_keyed_batch_through_verify_seals(fx, kv):
    k = fx['keyed']
    seals = [H(s) for s in k['root_seals']]
    claims = [c for c in k['claims'] if c['kind'] != 'bad_index']   # the on-chain form carries its root seal: no index to be out of range
    onchain = [kv.encode_seal(H(c['path']), b'' if c['root_idx'] == STORED else seals[c['root_idx']]) for c in claims]
    ids, jds = [H(c['image_id']) for c in claims], [H(c['journal_digest']) for c in claims]
    # one seal that does not decode and one with another selector are answered without reaching the device
    onchain += [onchain[0] + b'\0', b'\x00\x11\x22\x33' + onchain[0][4:]]
    ids += ids[:2]; jds += jds[:2]
    st, rv = kv.verify_seals(onchain, ids, jds)
    wst, wrv = _want(claims)
    assert (st[:-2] == wst).all() and (rv[:-2] == wrv).all()
    assert list(st[-2:]) == [INVALID_PROOF_DATA, SELECTOR_MISMATCH] and bytes(rv[-1]) == b'\x00\x11\x22\x33' and not rv[-2].any()
    n, jobs, looked = kv.last_counts()
    assert n == len(claims) and looked == sum(1 for c in claims if c['root_idx'] == STORED and c['kind'] != 'deep')


def test_last_counts_one_verification_per_root_seal_and_one_per_damaged_path(fx, kv):
    k = fx['keyed']
    seals = [H(s) for s in k['root_seals']]
    honest = [c for c in k['claims'] if c['kind'] == 'honest']
    used = {c['root_idx'] for c in honest} - {STORED}
    stored = sum(1 for c in honest if c['root_idx'] == STORED)
    assert len(used) == 3 and stored > 40
    st, _ = _host(kv, honest, seals)
    assert not st.any()
    assert kv.last_counts() == (len(honest), 3, stored)
    damaged = [c for c in k['claims'] if c['kind'] == 'straggler' and c['root_idx'] != STORED]
    assert len(damaged) == 3
    for kk in (1, 2, 3):                                             # behind the honest claims: every seal keeps an honest representative
        mixed = honest + damaged[:kk]
        st, _ = _host(kv, mixed, seals)
        assert list(np.nonzero(st)[0]) == list(range(len(honest), len(mixed))) and (st[len(honest):] == FAILED).all()
        assert kv.last_counts() == (len(mixed), 3 + kk, stored)
    # a damaged path as the lowest claim of its seal is the representative: its honest neighbours are then verified one by one
    t0 = [c for c in honest if c['root_idx'] == 0][:5]
    first = [c for c in damaged if c['root_idx'] == 0] + t0
    st, _ = _host(kv, first, seals)
    assert list(st) == [FAILED] + [OK] * 5 and kv.last_counts() == (6, 6, 0)


def test_submit_root_remembers_valid_roots_only(fx):
    k = fx['keyed']
    s = k['stored']
    seals = [H(x) for x in k['root_seals']]
    v = _keyed(fx)
    try:
        claims = k['claims']
        wst, wrv = _want(claims, 'status_unsubmitted')
        st, rv = _host(v, claims, seals)
        assert (st == wst).all() and (rv == wrv).all()
        stored = [i for i, c in enumerate(claims) if c['root_idx'] == STORED and c['kind'] == 'honest']
        assert len(stored) > 40 and (st[stored] == FAILED).all()
        assert not v.has_root(H(s['root']))
        # an invalid seal stores nothing: a valid proof of ANOTHER root, a spliced selector, a short seal
        assert v.submit_root(H(s['rejected_root']), H(s['rejected_seal'])) == (FAILED, bytes(4)) and not v.has_root(H(s['rejected_root']))
        assert v.submit_root(H(s['root']), seals[3]) == (SELECTOR_MISMATCH, seals[3][:4]) and not v.has_root(H(s['root']))
        assert v.submit_root(H(s['root']), H(s['seal'])[:-1]) == (INVALID_PROOF_DATA, bytes(4)) and not v.has_root(H(s['root']))
        assert v.submit_root(H(s['root']), b'\x01') == (INVALID_PROOF_DATA, bytes(4))
        st, _ = _host(v, claims, seals)
        assert (st == wst).all()
        # the valid one does, and resubmitting is OK
        assert v.submit_root(H(s['root']), H(s['seal'])) == (OK, bytes(4)) and v.has_root(H(s['root']))
        assert v.submit_root(H(s['root']), H(s['seal'])) == (OK, bytes(4)) and v.has_root(H(s['root'])) and not v.has_root(H(s['rejected_root']))
        st, rv = _host(v, claims, seals)
        wst2, wrv2 = _want(claims)
        assert (st == wst2).all() and (rv == wrv2).all() and (st[stored] == OK).all()
        # a second root: the table stays sorted whatever the order of submission
        assert v.submit_root(H(s['rejected_root']), seals[0]) == (OK, bytes(4)) and v.has_root(H(s['rejected_root']))
        t0 = [dict(c, root_idx=STORED) for c in claims if c['root_idx'] == 0 and c['kind'] == 'honest'][:8]
        st, _ = _host(v, t0 + [claims[i] for i in stored[:8]], [])
        assert not st.any() and v.last_counts() == (16, 0, 16)
    finally:
        v.close()


# ---------------------------------------------------------------- the built-in key
def test_real_key_batches_and_an_existing_verifier_afterwards(fx, rv0, real_proofs):
    r = fx['real']
    seals = [H(s) for s in r['root_seals']]
    for j in (0, 1):
        claims = [dict(c, root_idx=j, claim='', status=r['status'][j], recv=r['recv'][j]) for c in r['claims']]
        wst, wrv = _want(claims)
        for cl in (claims, claims[::-1]):
            st, rv = _host(rv0, cl, seals)
            assert (st == wst).all() and (rv == wrv).all()
            st, rv = _dev(rv0, cl, seals)
            assert (st == wst).all() and (rv == wrv).all()
        st, rv = rv0.verify_seals([rv0.encode_seal(H(c['path']), seals[j]) for c in claims], [H(c['image_id']) for c in claims],
                                  [H(c['journal_digest']) for c in claims])
        assert (st == wst).all() and (rv == wrv).all()
        assert rv0.last_counts() == (len(claims), 1, 0)
    assert rv0.submit_root(bytes(32), seals[0]) == (FAILED, bytes(4)) and rv0.submit_root(bytes(32), seals[1]) == (SELECTOR_MISMATCH, seals[1][:4])
    # an ordinary verifier of the same process is not disturbed
    from stylus_zkvm_verifiers_amd import RiscZeroVerifier
    p = real_proofs['risc0']
    v = RiscZeroVerifier(0)
    v.initialize(H(p['control_root']), H(p['bn254_control_id']))
    assert v.verify(H(p['seal']), H(p['image_id']), H(p['journal_digest'])) is True
    v.close()


# ---------------------------------------------------------------- more than one chunk
def test_a_batch_that_spans_two_chunks_verifies_a_group_once_per_chunk(fx, kv):
    """2^20 + 3 integrity claims: stored-root lookups of random digests (depth 0) around three honest claims of tree 0 under its seal, one in
    the first chunk and two in the second; the raw C call on numpy buffers (a million Python objects would take longer than the device)."""
    from stylus_zkvm_verifiers_amd import _lib, risc0_set_inclusion as rs
    k = fx['keyed']
    t0 = [c for c in k['claims'] if c['kind'] == 'honest' and c['root_idx'] == 0][:3]
    n = (1 << 20) + 3
    at = [5, (1 << 20) + 1, (1 << 20) + 2]
    g = np.random.default_rng(0x2C4)
    digests = g.integers(0, 256, (n, 32), dtype=np.uint8)
    depth = np.zeros(n, dtype=np.uint64)
    idx = np.full(n, STORED, dtype=np.uint32)
    for i, c in zip(at, t0):
        digests[i] = np.frombuffer(H(c['claim']), dtype=np.uint8)
        depth[i] = len(c['path']) // 64
        idx[i] = 0
    off = np.zeros(n + 1, dtype=np.uint32)
    off[1:] = np.cumsum(depth).astype(np.uint32)
    blob = b''.join(H(c['path']) for c in t0)
    seal = H(k['root_seals'][0])
    soff = np.array([0, len(seal)], dtype=np.uint64)
    st = np.full(n, 255, dtype=np.uint8); rv = np.full((n, 4), 255, dtype=np.uint8)
    _lib.check(rs.lib().zkv_risc0_setincl_verify_integrity_batch(kv.handle, n, digests.ctypes.data_as(rs._B), blob, off.ctypes.data, idx.ctypes.data, 1, seal,
                                                                 soff.ctypes.data, st.ctypes.data, rv.ctypes.data), 'zkv_risc0_setincl_verify_integrity_batch')
    want = np.full(n, FAILED, dtype=np.uint8)
    want[at] = OK
    assert (st == want).all() and not rv.any()
    assert kv.last_counts() == (n, 2, n - 3)

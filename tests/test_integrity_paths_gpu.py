"""verify_integrity on every batch path, on the GPU: the device-resident single-context call, verifier sets (host and device), mixed
batches with a per-proof method (host and device), the aggregate check and sharded contexts.  Every status and received selector equals
the C oracle's (`verify_integrity` / `verify` / `sp1_verify_proof`, per instance for sets).

Rows of the larger batches are drawn from pools of re-randomised real proofs (1/4 mutated) whose every row the oracle has checked, so
each row of every batch has an oracle answer; unplaced mixed rows follow the partition model of tests/mixed_model.py."""
import ctypes as C
import os

import numpy as np
import pytest

import mixed_model as mm

H = bytes.fromhex
POOL = 192


@pytest.fixture(scope='module')
def zkv():
    import stylus_zkvm_verifiers_amd as z
    assert z.device_count() >= 1, 'no gfx950 device visible'
    return z


def _rv(r):
    return bytes(r) if r else bytes(4)


@pytest.fixture(scope='module')
def pools(real_proofs):
    """Three oracle-checked pools of POOL rows: RISC Zero verify, RISC Zero verify_integrity, SP1 verify_proof."""
    import oracle_lib as ol
    from stylus_zkvm_verifiers_amd import synth
    r, s = real_proofs['risc0'], real_proofs['sp1']
    orc = ol.Risc0Oracle(); orc.initialize(H(r['control_root']), H(r['bn254_control_id']))
    p = {}
    sv, _, _, fv = synth.make_batch('risc0', H(r['seal']), POOL, 0x1A7E0001, pool=8, mutate_every=4)
    ids = np.tile(np.frombuffer(H(r['image_id']), dtype=np.uint8), (POOL, 1))
    jds = np.tile(np.frombuffer(H(r['journal_digest']), dtype=np.uint8), (POOL, 1)); jds[fv, 3] ^= 4
    res = [orc.verify(sv[i].tobytes(), ids[i].tobytes(), jds[i].tobytes()) for i in range(POOL)]
    p['verify'] = dict(seals=sv, a=ids, b=jds, st=np.array([x[0] for x in res], np.uint8), rv=np.array([list(_rv(x[1])) for x in res], np.uint8))
    si, cl, _, _, _ = synth.make_integrity_batch(H(r['seal']), H(r['claim_digest']), POOL, 0x1A7E0002, pool=8, mutate_every=4,
                                                 classes=('flip_claim', 'wrong_selector'))
    res = [orc.verify_integrity(si[i].tobytes(), cl[i].tobytes()) for i in range(POOL)]
    p['integrity'] = dict(seals=si, a=cl, st=np.array([x[0] for x in res], np.uint8), rv=np.array([list(_rv(x[1])) for x in res], np.uint8))
    ss, _, _, fs = synth.make_batch('sp1', H(s['proof']), POOL, 0x1A7E0003, pool=8, mutate_every=4)
    pv0 = H(s['public_values'])
    vk = np.tile(np.frombuffer(H(s['vkey']), dtype=np.uint8), (POOL, 1))
    pv = np.tile(np.frombuffer(pv0, dtype=np.uint8), (POOL, 1)); pv[fs, -1] ^= 1
    res = [ol.sp1_verify_proof(vk[i].tobytes(), pv[i].tobytes(), ss[i].tobytes()) for i in range(POOL)]
    p['sp1'] = dict(seals=ss, a=vk, b=pv, st=np.array([x[0] for x in res], np.uint8), rv=np.array([list(_rv(x[1])) for x in res], np.uint8))
    for k in p:
        assert set(p[k]['st'].tolist()) >= {0, 1} and 5 in p[k]['st'], k          # accepts, failures and selector mismatches in every pool
    p['orc'] = orc
    return p


@pytest.fixture(scope='module')
def r0(zkv, real_proofs):
    r = real_proofs['risc0']
    v = zkv.RiscZeroVerifier()
    v.initialize(H(r['control_root']), H(r['bn254_control_id']))
    yield v
    v.close()


@pytest.fixture(scope='module')
def mixed(zkv, real_proofs):
    r = real_proofs['risc0']
    v = zkv.MixedVerifier(H(r['control_root']), H(r['bn254_control_id']))
    yield v
    v.close()


def _up(*xs):
    import torch
    return [torch.from_numpy(np.ascontiguousarray(x)).to(torch.device('cuda', 0)) for x in xs]


def _outs(n):
    import torch
    dev = torch.device('cuda', 0)
    return torch.full((n,), 255, dtype=torch.uint8, device=dev), torch.full((n, 4), 255, dtype=torch.uint8, device=dev)


def _integrity_dev(v, seals, claims, stream=None):
    import torch
    n = len(seals)
    d = _up(seals, claims)
    st, rv = _outs(n)
    torch.cuda.synchronize()                   # inputs and the 255-filled outputs are in place before another stream touches them
    s = stream or torch.cuda.current_stream()
    v.verify_integrity_batch_dev(n, d[0].data_ptr(), d[1].data_ptr(), st.data_ptr(), rv.data_ptr(), s.cuda_stream)
    s.synchronize()
    v.synchronize()                            # torch's default stream is handle 0: the call then ran on the context's own stream
    return st.cpu().numpy(), rv.cpu().numpy()


# ---------------------------------------------------------------- 1. single context, device-resident
@pytest.mark.gpu
def test_integrity_dev_on_the_real_proof_and_the_corpus(zkv, r0, real_proofs, verify_corpus):
    """The real proof and every 260-byte RISC Zero seal of the verify corpus with its claim digest (claim of (image_id, journal_digest)),
    each also with a flipped claim bit; an un-initialised verifier answers INVALID_INITIALIZATION for every row."""
    import oracle_lib as ol
    r = real_proofs['risc0']
    ctx = verify_corpus['risc0_ctx']
    orc = ol.Risc0Oracle(); orc.initialize(H(ctx['control_root']), H(ctx['bn254_control_id']))
    v = zkv.RiscZeroVerifier(); v.initialize(H(ctx['control_root']), H(ctx['bn254_control_id']))
    rows = [(H(r['seal']), H(r['claim_digest']))]
    rows += [(H(c['seal']), ol.risc0_claim_digest(H(c['image_id']), H(c['journal_digest']))) for c in verify_corpus['cases']
             if c['vm'] == 'risc0' and len(H(c['seal'])) == 260]
    rows += [(sl, bytes([cd[0] ^ 0x80]) + cd[1:]) for sl, cd in rows]
    assert len(rows) >= 20
    seals = np.array([list(x[0]) for x in rows], np.uint8); claims = np.array([list(x[1]) for x in rows], np.uint8)
    st, rv = _integrity_dev(v, seals, claims)
    want = [orc.verify_integrity(sl, cd) for sl, cd in rows]
    assert st.tolist() == [w[0] for w in want]
    assert [bytes(x) for x in rv] == [_rv(w[1]) for w in want]
    assert st[0] == 0 and st[len(rows) // 2] == 1                     # the real proof is accepted, its flipped claim is not
    # the host-buffer entry point on the same rows
    hst, hrv = v.verify_integrity_batch([x[0] for x in rows], [x[1] for x in rows])
    assert (hst == st).all() and (hrv == rv).all()
    v.close()
    un = zkv.RiscZeroVerifier()
    st, rv = _integrity_dev(un, seals, claims)
    assert (st == 2).all() and (rv == 0).all()
    un.close()


@pytest.mark.gpu
@pytest.mark.parametrize('n', [1, 2049, 65536, 70000])
def test_integrity_dev_batch_sizes_on_a_caller_stream(zkv, r0, pools, n):
    """Across the small-batch, tail-split and chunk boundaries, on a caller stream: each row equals the oracle; at 65,536 the host-buffer
    call on the same rows gives the same bytes."""
    import torch
    p = pools['integrity']
    pick = np.random.default_rng(n).integers(0, POOL, n)
    st, rv = _integrity_dev(r0, p['seals'][pick], p['a'][pick], torch.cuda.Stream())
    assert (st == p['st'][pick]).all() and (rv == p['rv'][pick]).all()
    if n == 65536:
        hst, hrv = r0.verify_integrity_batch([p['seals'][i].tobytes() for i in pick], [p['a'][i].tobytes() for i in pick])
        assert (hst == st).all() and (hrv == rv).all()


@pytest.mark.gpu
def test_integrity_dev_with_the_aggregate_check(zkv, r0, pools):
    """Aggregate check on (forced onto a 70,000-proof batch, mostly valid rows): the statuses are those without it."""
    p = pools['integrity']
    rng = np.random.default_rng(0x1A7E)
    valid = np.nonzero(p['st'] == 0)[0]; bad = np.nonzero(p['st'] != 0)[0]
    pick = valid[rng.integers(0, len(valid), 70000)]
    pick[::997] = bad[rng.integers(0, len(bad), len(pick[::997]))]
    os.environ['ZKV_AGG_MIN'] = '4096'
    try:
        r0.set_aggregate_check(True, seed=bytes(range(32)), sub_batch=32)
        st, rv = _integrity_dev(r0, p['seals'][pick], p['a'][pick])
        checked = r0.aggregate_counters()[0]
    finally:
        r0.set_aggregate_check(False)
        del os.environ['ZKV_AGG_MIN']
    assert checked > 0
    assert (st == p['st'][pick]).all() and (rv == p['rv'][pick]).all()


# ---------------------------------------------------------------- 2. verifier sets
@pytest.mark.gpu
def test_set_integrity_host_and_device_per_instance(zkv, real_proofs, pools):
    """Three instances (the real parameters, another control root, a control id >= R) and indices past the set: each row is that
    instance's verify_integrity (oracle), an index past the set is INVALID_INITIALIZATION.  Host rows include short seals."""
    import torch
    import oracle_lib as ol
    r = real_proofs['risc0']
    roots = [H(r['control_root']), bytes([H(r['control_root'])[0] ^ 1]) + H(r['control_root'])[1:], H(r['control_root'])]
    ids = [H(r['bn254_control_id']), H(r['bn254_control_id']), b'\xff' * 32]
    vs = zkv.RiscZeroVerifierSet(roots, ids)
    orcs = []
    for a, b in zip(roots, ids):
        o = ol.Risc0Oracle(); o.initialize(a, b); orcs.append(o)
    p = pools['integrity']
    rng = np.random.default_rng(0x5E7)
    n = 300
    pick = rng.integers(0, POOL, n)
    inst = rng.integers(0, 5, n).astype(np.uint32); inst[::37] = 0xFFFFFFFF
    lens = np.full(n, 260); lens[5::23] = rng.integers(0, 260, len(lens[5::23]))
    seals = [p['seals'][pick[i]].tobytes()[:lens[i]] for i in range(n)]
    claims = [p['a'][pick[i]].tobytes() for i in range(n)]
    cache = {}

    def want(i, sl):
        if inst[i] >= 3:
            return 2, bytes(4)
        key = (int(inst[i]), sl, claims[i])
        if key not in cache:
            s_, r_ = orcs[inst[i]].verify_integrity(sl, claims[i]); cache[key] = (s_, _rv(r_))
        return cache[key]

    st, rv = vs.verify_integrity_batch(inst, seals, claims)
    exp = [want(i, seals[i]) for i in range(n)]
    assert st.tolist() == [e[0] for e in exp] and [bytes(x) for x in rv] == [e[1] for e in exp]
    assert {0, 2, 4, 5} <= set(st.tolist())
    # device form: fixed 260-byte rows, on a caller stream
    d = _up(inst, p['seals'][pick], p['a'][pick])
    dst, drv = _outs(n)
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    vs.verify_integrity_batch_dev(n, d[0].data_ptr(), d[1].data_ptr(), d[2].data_ptr(), dst.data_ptr(), drv.data_ptr(), side.cuda_stream)
    side.synchronize()
    exp = [want(i, p['seals'][pick[i]].tobytes()) for i in range(n)]
    assert dst.cpu().numpy().tolist() == [e[0] for e in exp] and [bytes(x) for x in drv.cpu().numpy()] == [e[1] for e in exp]
    vs.close()


# ---------------------------------------------------------------- 3. mixed batches with a per-proof method
def _mixed_rows(pools, vm, method, rng, pv_len=None):
    """Rows for (vm, method): data from the pool of the row's call (unplaced rows get any pool's data) and the expected bytes."""
    n = len(vm)
    kind = np.where(vm == 1, 2, np.where(method == 1, 1, 0))
    names = ('verify', 'integrity', 'sp1')
    pick = rng.integers(0, POOL, n)
    pvl = pools['sp1']['b'].shape[1] if pv_len is None else pv_len
    bw = max(32, pvl)
    seals = np.zeros((n, 260), np.uint8); a = np.zeros((n, 32), np.uint8); b = rng.integers(0, 256, (n, bw)).astype(np.uint8)
    st = np.zeros(n, np.uint8); rv = np.zeros((n, 4), np.uint8)
    for k, name in enumerate(names):
        sel = kind == k
        q = pools[name]
        seals[sel] = q['seals'][pick[sel]]; a[sel] = q['a'][pick[sel]]
        if name == 'verify':
            b[sel, :32] = q['b'][pick[sel]]
        elif name == 'sp1':
            b[sel, :pvl] = q['b'][pick[sel], :pvl]
        st[sel] = q['st'][pick[sel]]; rv[sel] = q['rv'][pick[sel]]
    _, _, _, unplaced, ust = mm.partition(vm, method)
    st[unplaced] = ust; rv[unplaced] = 0
    return seals, a, b, st, rv, kind


def _mixed_dev(mixed, vm, method, seals, a, b, pv_len, use_method=True):
    import torch
    n = len(vm)
    d = _up(vm, method, seals, a, b)
    st, rv = _outs(n)
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    mixed.verify_batch_dev(n, d[0].data_ptr(), d[2].data_ptr(), d[3].data_ptr(), d[4].data_ptr(), b.shape[1], pv_len, st.data_ptr(), rv.data_ptr(),
                           s.cuda_stream, d_method=d[1].data_ptr() if use_method else 0)
    s.synchronize()
    return st.cpu().numpy(), rv.cpu().numpy()


def _host_b(vm, method, b, pvl, rng):
    """Ragged in_b: 32 bytes for RISC Zero verify rows, the public values for SP1 rows, any length (0 included) otherwise."""
    out = []
    for i in range(len(vm)):
        if vm[i] == 0 and method[i] == 0:
            out.append(b[i, :32].tobytes())
        elif vm[i] == 1:
            out.append(b[i, :pvl].tobytes())
        else:
            out.append(b[i, :int(rng.integers(0, 41))].tobytes() if b.shape[1] >= 40 else b'')
    return out


@pytest.mark.gpu
@pytest.mark.parametrize('n', [1, 5, 4099, 1 << 17])
def test_mixed_calls_host_and_device_equal_the_oracle(zkv, mixed, pools, n):
    rng = np.random.default_rng(n)
    vm, method = mm.random_calls(rng, n)
    if n == 5:
        vm[:] = [0, 0, 1, 2, 1]; method[:] = [1, 0, 0, 1, 1]
    seals, a, b, st_w, rv_w, _ = _mixed_rows(pools, vm, method, rng)
    pvl = pools['sp1']['b'].shape[1]
    st, rv = _mixed_dev(mixed, vm, method, seals, a, b, pvl)
    assert (st == st_w).all() and (rv == rv_w).all()
    hst, hrv = mixed.verify_batch(vm, list(seals), list(a), _host_b(vm, method, b, pvl, rng), methods=method)
    assert (hst == st_w).all() and (hrv == rv_w).all()
    if n >= 4099:
        assert {0, 1, 5, 6, 7} <= set(st.tolist())


@pytest.mark.gpu
def test_mixed_call_without_a_method_is_the_method_less_call(zkv, mixed, pools):
    """A NULL method gives byte for byte what zkv_mixed_verify_batch[_dev] give on the same inputs (integrity rows included: without a
    method they are verify rows of whatever their in_b holds)."""
    from stylus_zkvm_verifiers_amd import _lib
    import torch
    rng = np.random.default_rng(77)
    n = 4099
    vm, method = mm.random_calls(rng, n)
    seals, a, b, _, _, _ = _mixed_rows(pools, vm, method, rng)
    pvl = pools['sp1']['b'].shape[1]
    old, old_rv = _mixed_dev(mixed, vm, method, seals, a, b, pvl, use_method=False)
    L = _lib.lib()
    d = _up(vm, seals, a, b)
    st, rv = _outs(n)
    torch.cuda.synchronize()
    _lib.check(L.zkv_mixed_verify_call_batch_dev(mixed._h, n, d[0].data_ptr(), None, d[1].data_ptr(), d[2].data_ptr(), d[3].data_ptr(), b.shape[1], pvl,
                                                 st.data_ptr(), rv.data_ptr(), None), 'zkv_mixed_verify_call_batch_dev')
    _lib.check(L.zkv_ctx_synchronize(mixed._h), 'zkv_ctx_synchronize')
    torch.cuda.synchronize()
    assert (st.cpu().numpy() == old).all() and (rv.cpu().numpy() == old_rv).all()
    hb = [b[i, :32].tobytes() if vm[i] == 0 else b[i, :pvl].tobytes() for i in range(n)]
    hst, hrv = mixed.verify_batch(vm, list(seals), list(a), hb)          # zkv_mixed_verify_batch
    from stylus_zkvm_verifiers_amd.risc0 import _blob, _cat32
    sblob, soff = _blob(list(seals)); bblob, boff = _blob(hb)
    nst = np.zeros(n, np.uint8); nrv = np.zeros((n, 4), np.uint8)
    tags = np.ascontiguousarray(vm)
    _lib.check(L.zkv_mixed_verify_call_batch(mixed._h, n, tags.ctypes.data, None, sblob, soff.ctypes.data, _cat32(list(a), 'in_a'), bblob, boff.ctypes.data,
                                             nst.ctypes.data, nrv.ctypes.data), 'zkv_mixed_verify_call_batch')
    assert (nst == hst).all() and (nrv == hrv).all() and (hst == old).all() and (hrv == old_rv).all()


@pytest.mark.gpu
def test_mixed_calls_with_empty_public_values(zkv, mixed, pools):
    """b_stride 32 and pv_len 0: every SP1 row has empty public values (oracle on those), the RISC Zero rows are unchanged."""
    import oracle_lib as ol
    rng = np.random.default_rng(32)
    n = 3001
    vm, method = mm.random_calls(rng, n)
    seals, a, b, st_w, rv_w, kind = _mixed_rows(pools, vm, method, rng, pv_len=0)
    assert b.shape[1] == 32
    cache = {}
    for i in np.nonzero((vm == 1) & (method == 0))[0]:
        key = (seals[i].tobytes(), a[i].tobytes())
        if key not in cache:
            s_, r_ = ol.sp1_verify_proof(a[i].tobytes(), b'', seals[i].tobytes()); cache[key] = (s_, _rv(r_))
        st_w[i] = cache[key][0]; rv_w[i] = list(cache[key][1])
    st, rv = _mixed_dev(mixed, vm, method, seals, a, b, 0)
    assert (st == st_w).all() and (rv == rv_w).all()
    hst, hrv = mixed.verify_batch(vm, list(seals), list(a), _host_b(vm, method, b, 0, rng), methods=method)
    assert (hst == st_w).all() and (hrv == rv_w).all()


@pytest.mark.gpu
def test_mixed_calls_with_the_aggregate_check(zkv, mixed, pools):
    """The aggregate check on a 2^17 mixed batch whose RISC Zero sub-batch interleaves verify and verify_integrity rows: same statuses."""
    rng = np.random.default_rng(0xA66)
    n = 1 << 17
    vm, method = mm.random_calls(rng, n, p_bad=0.01)
    seals, a, b, st_w, rv_w, _ = _mixed_rows(pools, vm, method, rng)
    pvl = pools['sp1']['b'].shape[1]
    os.environ['ZKV_AGG_MIN'] = '4096'
    try:
        mixed.set_aggregate_check(True, seed=bytes(range(32)), sub_batch=16)
        st, rv = _mixed_dev(mixed, vm, method, seals, a, b, pvl)
        checked = mixed.aggregate_counters()[0]
    finally:
        mixed.set_aggregate_check(False)
        del os.environ['ZKV_AGG_MIN']
    assert checked > 0
    assert (st == st_w).all() and (rv == rv_w).all()


# ---------------------------------------------------------------- 4. sharded contexts (two logical shards on device 0, staged)
@pytest.mark.gpu
def test_sharded_integrity_and_mixed_calls_equal_unsharded(zkv, real_proofs, pools, r0, mixed):
    import torch
    r = real_proofs['risc0']
    env = {'ZKV_SHARD_MIN': '256', 'ZKV_SHARD_FORCE_STAGING': '1', 'ZKV_SHARD_FIRST_PIECE': '300'}
    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        rng = np.random.default_rng(0x5A4D)
        n = 3001
        p = pools['integrity']
        pick = rng.integers(0, POOL, n)

        def mk0():
            v = zkv.RiscZeroVerifier(0); v.initialize(H(r['control_root']), H(r['bn254_control_id'])); return v
        sv = zkv.shard([mk0(), mk0()])
        st, rv = _integrity_dev(sv, p['seals'][pick], p['a'][pick], torch.cuda.Stream())
        st1, rv1 = _integrity_dev(r0, p['seals'][pick], p['a'][pick])
        assert (st == st1).all() and (rv == rv1).all() and (st == p['st'][pick]).all()
        sv.close()
        mk = lambda: zkv.MixedVerifier(H(r['control_root']), H(r['bn254_control_id']), 0)
        sm = zkv.shard([mk(), mk()])
        vm, method = mm.random_calls(rng, n)
        seals, a, b, st_w, rv_w, _ = _mixed_rows(pools, vm, method, rng)
        pvl = pools['sp1']['b'].shape[1]
        st, rv = _mixed_dev(sm, vm, method, seals, a, b, pvl)
        st1, rv1 = _mixed_dev(mixed, vm, method, seals, a, b, pvl)
        assert (st == st1).all() and (rv == rv1).all() and (st == st_w).all() and (rv == rv_w).all()
        hst, hrv = sm.verify_batch(vm, list(seals), list(a), _host_b(vm, method, b, pvl, rng), methods=method)
        assert (hst == st_w).all() and (hrv == rv_w).all()
        sm.close()
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


# ---------------------------------------------------------------- 5. no wavefront gave up waiting on its producer
@pytest.mark.gpu
def test_no_wait_faults_across_the_file(zkv):
    from stylus_zkvm_verifiers_amd import _lib
    out = C.c_uint64(0)
    _lib.check(_lib.lib().zkv_diag_wait_faults(0, C.byref(out)), 'zkv_diag_wait_faults')
    assert out.value == 0

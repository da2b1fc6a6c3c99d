"""eth_call batches on a PLONK key set of deployed contracts on the device (include/zkv_plonk_set_wire.h):
statuses, reasons, resolved keys, reverted flags and return data against the model (tests/plonk_set_wire_model.py) through the host call
and through the device call on a caller's stream; placed requests against verify_batch of the same set; the eight totals; unaligned
blobs; the aggregate check; and the wait-fault counter.  PARITY UNPINNED: the reference holds no PLONK code and no contract shell."""
import ctypes as C

import numpy as np
import pytest

import plonk_set_wire_model as pm
import plonk_shared_srs as S
import plonk_trapdoor_keys as T

pytestmark = pytest.mark.gpu
SEED = bytes(range(32))
SIZES = [1, 63, 64, 65, 3000]        # a partial wavefront, a block edge of the key-set kernels, a multi-block partition


@pytest.fixture(scope='module')
def zkv():
    import stylus_zkvm_verifiers_amd as z
    assert z.device_count() >= 1, 'no gfx950 device visible'
    return z


def _faults():
    from stylus_zkvm_verifiers_amd import _lib
    out = C.c_uint64(0)
    _lib.check(_lib.lib().zkv_diag_wait_faults(0, C.byref(out)), 'zkv_diag_wait_faults')
    return out.value


@pytest.fixture(scope='module')
def world(zkv):
    fx = pm.fixture()
    keys = pm.deployed_set(fx)
    reqs = pm.requests(keys, fx)
    model = pm.Contracts(keys)
    want = pm.expected(model, reqs)
    pm.check_coverage(model, reqs, want)                 # every status, every reason, both n_c, nb of 0 and of 128
    faults = _faults()
    s = zkv.PlonkDeployedSet(keys)
    yield s, keys, reqs, model, want
    assert _faults() == faults                           # no consumer wavefront ever waited in vain
    s.close()


def _host(s, to, blob, off):
    n = len(off) - 1
    rev, data, st, rs = s.eth_call_batch([to[20 * i:20 * i + 20] for i in range(n)], blob, offsets=off)
    return st, rs, rev, data


def _dev(s, to, blob, off, optional=True, own_stream=True):
    """The device call on a caller's stream (or the context's) -> (statuses, reasons, resolved keys); without the optional rows: None."""
    import torch
    dev = torch.device('cuda', 0)
    n = len(off) - 1
    st = torch.cuda.Stream() if own_stream else None
    with torch.cuda.stream(st):
        d_to = torch.frombuffer(bytearray(to), dtype=torch.uint8).to(dev)
        d_cd = torch.frombuffer(bytearray(blob + b'\0'), dtype=torch.uint8).to(dev)
        d_off = torch.from_numpy(off.astype(np.int64)).to(dev)
        d_st = torch.full((n,), 255, dtype=torch.uint8, device=dev)
        d_rs = torch.full((n,), 255, dtype=torch.uint8, device=dev)
        d_key = torch.full((n,), 0x55555555, dtype=torch.int32, device=dev)
        torch.cuda.synchronize()
        s.eth_call_batch_dev(n, d_to.data_ptr(), d_cd.data_ptr(), d_off.data_ptr(), len(blob), d_st.data_ptr(), d_rs.data_ptr() if optional else 0,
                             d_key.data_ptr() if optional else 0, st.cuda_stream if own_stream else 0)
        if own_stream:
            st.synchronize()
        else:
            s.synchronize()
    if not optional:
        assert (d_rs.cpu().numpy() == 255).all() and (d_key.cpu().numpy() == 0x55555555).all()
        return d_st.cpu().numpy(), None, None
    return d_st.cpu().numpy(), d_rs.cpu().numpy(), d_key.cpu().numpy().view(np.uint32)


def _check_host(exp, st, rs, rev, data):
    bad = [i for i, e in enumerate(exp) if (st[i], rs[i], bool(rev[i]), data[i]) != (e[0], e[1], e[3], e[4])]
    assert not bad, (bad[:8], [(st[i], rs[i], rev[i], data[i].hex(), exp[i]) for i in bad[:3]])


@pytest.mark.parametrize('n', SIZES)
def test_host_call_equals_the_model(world, n):
    s, keys, reqs, model, want = world
    to, blob, off, exp = pm.batch(reqs, want, n, 1000 + n)
    st, rs, rev, data = _host(s, to, blob, off)
    print('n', n, 'statuses', np.bincount(st, minlength=11).tolist(), 'reasons', np.bincount(rs, minlength=6).tolist(), 'decode + points ms', s.last_wire_ms())
    _check_host(exp, st, rs, rev, data)
    assert s.last_call_counts() == pm.counts(exp)
    for i, e in enumerate(exp):                          # the length rows: nothing, a bool word or an Error(string)
        assert len(data[i]) in (0, 32, 100) and len(data[i]) == len(e[4])


@pytest.mark.parametrize('n', SIZES)
def test_device_call_on_a_caller_stream_equals_the_model(world, n):
    s, keys, reqs, model, want = world
    to, blob, off, exp = pm.batch(reqs, want, n, 2000 + n)
    st, rs, key = _dev(s, to, blob, off)
    bad = [i for i, e in enumerate(exp) if (st[i], rs[i], key[i]) != e[:3]]
    assert not bad, (bad[:8], [(st[i], rs[i], key[i], exp[i][:3]) for i in bad[:3]])
    assert s.last_call_counts() == pm.counts(exp)
    for i, e in enumerate(exp):                          # return data is rendered on the host from status and reason
        assert s.eth_call_returndata(int(st[i]), int(rs[i])) == (e[3], e[4]), i
    st2, _, _ = _dev(s, to, blob, off, optional=False, own_stream=False)     # without the optional rows, on the context's own stream
    assert (st2 == st).all()
    assert s.last_call_counts() == pm.counts(exp)


def _rows(s, triples):
    ps, ins = s.proof_stride(), s.input_stride()
    proofs = np.zeros((len(triples), ps), np.uint8)
    pub = np.zeros((len(triples), ins // 32, 32), np.uint8)
    for r, (_, p, q) in enumerate(triples):
        proofs[r, :len(p)] = np.frombuffer(p, np.uint8)
        if q:
            pub[r, :len(q)] = np.frombuffer(b''.join(q), np.uint8).reshape(len(q), 32)
    return np.array([t[0] for t in triples], np.uint32), proofs, pub


def test_placed_requests_equal_verify_batch_and_the_classification_never_contradicts_it(world):
    s, keys, reqs, model, want = world
    to, blob, off, exp = pm.batch(reqs, want, 3000, 77)
    st, rs, _, _ = _host(s, to, blob, off)
    placed, caught, idx, cidx = [], [], [], []
    for i, e in enumerate(exp):
        if e[0] in (pm.OK, pm.FAILED) or e[1] in (pm.R_INPUT_RANGE, pm.R_OPENING_RANGE, pm.R_EC):
            v, j, r, proof, pub = model.classify(to[20 * i:20 * i + 20], blob[int(off[i]):int(off[i + 1])])
            nb, nc = model.shapes[j]
            if len(pub) != nb or len(proof) != 32 * (24 + 3 * nc):
                continue                                                     # (input >= r with a wrong size: no row of the set holds it)
            (placed if r == 0 else caught).append((j, proof, pub)); (idx if r == 0 else cidx).append(i)
    assert len(idx) > 300 and set(range(18)) <= set(t[0] for t in placed) and max(t[0] for t in placed) >= 18      # every shape key, and tampered keys
    got = s.verify_batch(*_rows(s, placed))
    assert got.any() and not got.all()
    assert (got == (st[idx] == pm.OK)).all() and set(st[idx]) == {pm.OK, pm.FAILED} and not rs[idx].any()
    # requests of reasons 2, 4 and 5 answer 0 from the core too
    assert {int(r) for r in rs[cidx]} == {pm.R_INPUT_RANGE, pm.R_OPENING_RANGE, pm.R_EC} and len(cidx) > 100
    assert not s.verify_batch(*_rows(s, caught)).any()
    # the ordinary set calls are untouched by the wire calls before them
    assert s.size() == len(keys) and s.proof_stride() == 864 and s.input_stride() == 32 * 128
    assert s.shapes[:18] == [(nb, nc, 32 * (24 + 3 * nc)) for nb, nc in T.SHAPES]


@pytest.mark.parametrize('shift', (1, 2, 3))
def test_a_blob_whose_requests_start_off_the_dword_grid(world, shift):
    s, keys, reqs, model, want = world
    whole = [i for i, r in enumerate(reqs) if len(r[3]) % 4 == 0 and len(r[3])]          # requests of whole dwords keep the blob's alignment
    pick = list(np.random.default_rng(shift).choice(whole, 127))
    to, blob, off, exp = pm.batch(reqs, want, 129, 40 + shift, pick=pick, shift=shift)
    assert {int(o) % 4 for o in off} == {shift}
    assert {e[1] for e in exp} == set(range(6)) and {pm.OK, pm.FAILED} <= {e[0] for e in exp}
    st, rs, key = _dev(s, to, blob, off)
    bad = [i for i, e in enumerate(exp) if (st[i], rs[i], key[i]) != e[:3]]
    assert not bad, (bad[:8], [(st[i], rs[i], key[i], exp[i][:3]) for i in bad[:3]])
    _check_host(exp, *_host(s, to, blob, off))


def test_aggregate_check_on_the_smallest_batch_that_engages_it(zkv, monkeypatch):
    """The check engages from ZKV_AGG_MIN placed requests (64 at the least): 64 placed requests to three contracts of one SRS, a few that
    are not placed, and the two offset cases; with one placed request fewer it does not engage.  Statuses are equal on and off."""
    monkeypatch.setenv('ZKV_AGG_MIN', '64')
    shapes = [('A', 2, 0, 0), ('A', 0, 1, 0), ('A', 3, 1, 0)]
    keys = [(S.key_bytes(*k), pm.address_of(S.key_bytes(*k))) for k in shapes]
    model = pm.Contracts(keys)
    reqs = []
    for j, k in enumerate(shapes):
        for v in range(2):
            proof, pub = S.valid(*k, v)
            pub = [x.to_bytes(32, 'big') for x in pub]
            reqs.append(('valid', j, keys[j][1], pm.encode(proof, pub), 1))
            l_eval = (int.from_bytes(proof[384:416], 'big') + 1) % pm.R                   # eval_l+1: fails at the pairing alone
            reqs.append(('pairing', j, keys[j][1], pm.encode(proof[:384] + pm.word(l_eval) + proof[416:], pub), 0))
        proof, pub = S.valid(*k, 0)
        pub = [x.to_bytes(32, 'big') for x in pub]
        reqs.append(('opening', j, keys[j][1], pm.encode(proof[:384] + pm.word(pm.R) + proof[416:], pub), None))
        reqs.append(('curve', j, keys[j][1], pm.encode(proof[:63] + bytes([proof[63] ^ 1]) + proof[64:], pub), None))
        reqs.append(('count', j, keys[j][1], pm.encode(proof, pub + [bytes(32)]), None))
        reqs.append(('short', j, keys[j][1], pm.encode(proof, pub)[:-1], None))
    want = pm.expected(model, reqs)
    placed = [i for i, w in enumerate(want) if w[0] in (pm.OK, pm.FAILED)]
    other = [i for i, w in enumerate(want) if w[0] not in (pm.OK, pm.FAILED)]
    assert {want[i][0] for i in placed} == {pm.OK, pm.FAILED} and {want[i][1] for i in other} == {0, 1, 4, 5}
    s = zkv.PlonkDeployedSet(keys)
    assert s.srs_classes() == ([0, 0, 0], 1)
    pick = [placed[i % len(placed)] for i in range(64)] + other
    to, blob, off, exp = pm.batch(reqs, want, len(pick) + 2, 5, pick=pick)
    assert pm.counts(exp)[0] == 64
    s.set_aggregate_check(False)
    r0 = _host(s, to, blob, off)
    c0 = s.aggregate_counters()
    s.set_aggregate_check(True, SEED, 16)
    r1 = _host(s, to, blob, off)
    st2, rs2, key2 = _dev(s, to, blob, off)
    c1 = s.aggregate_counters()
    s.set_aggregate_check(False)
    _check_host(exp, *r0)
    _check_host(exp, *r1)
    assert (st2 == r0[0]).all() and (rs2 == r0[1]).all() and [int(k) for k in key2] == [e[2] for e in exp]
    assert c1[0] > c0[0]                                 # sub-batches were checked in aggregate
    assert s.last_call_counts() == pm.counts(exp)
    drop = pick[1:]                                      # one placed request fewer: the check does not engage, the statuses are the same
    to, blob, off, exp = pm.batch(reqs, want, len(drop) + 2, 6, pick=drop)
    s.set_aggregate_check(True, SEED, 16)
    r3 = _host(s, to, blob, off)
    c2 = s.aggregate_counters()
    s.set_aggregate_check(False)
    _check_host(exp, *r3)
    assert c2 == c1
    s.close()


def test_a_set_of_one_contract_without_inputs_and_a_single_request(zkv):
    """nb = 0 alone: the input stride is zero, and the contract is callable with an empty array."""
    fx = pm.fixture()
    e = next(e for e in fx['pool'] if (e['nb_public'], e['n_c']) == (0, 0))
    vk, proofs, _ = T.pool_arrays(e)
    addr = bytes(range(40, 60))
    s = zkv.PlonkDeployedSet([(vk, addr)])
    assert s.input_stride() == 0 and s.proof_stride() == 768
    good = pm.encode(proofs[0].tobytes(), [])
    rev, data, st, rs = s.eth_call_batch([addr], [good])
    assert (list(st), list(rs), list(rev), data) == ([pm.OK], [0], [0], [pm.word(1)])
    assert s.last_call_counts() == [1, 0, 0, 0, 0, 0, 0, 0]
    proof = proofs[0].tobytes()
    wrong = proof[:384] + pm.word((int.from_bytes(proof[384:416], 'big') + 1) % pm.R) + proof[416:]       # eval_l+1: fails at the pairing alone
    rev, data, st, rs = s.eth_call_batch([addr, addr, bytes(20), addr], [pm.encode(proof, [bytes(32)]), b'', good, pm.encode(wrong, [])])
    assert list(st) == [pm.INVALID_PROOF_DATA, pm.BAD_CALLDATA, pm.NO_CONTRACT, pm.FAILED] and list(rs) == [1, 0, 0, 0] and list(rev) == [1, 1, 0, 0]
    assert data == [pm.error_data(1), b'', b'', pm.word(0)]
    assert s.last_call_counts() == [1, 1, 1, 1, 0, 0, 0, 0]
    assert list(s.verify_batch([0], [proofs[0].tobytes()], [[]])) == [1]
    s.close()

"""eth_call batches on a Groth16 key set of deployed contracts on the device (include/zkv_groth16_set_wire.h):
statuses, resolved keys, reverted flags and return data against the model (tests/groth16_set_wire_model.py) through the host call and
through the device call on a caller's stream; placed requests against verify_batch of the same set; the four totals; the aggregate
check; and the wait-fault counter.  PARITY UNPINNED: the reference holds no generic contract shell."""
import ctypes as C

import numpy as np
import pytest

import groth16_set_wire_model as gm

pytestmark = pytest.mark.gpu
SEED = bytes(range(32))
SIZES = [1, 63, 64, 65, 3000]        # a partial wavefront, a block edge of the key-set kernels, a multi-block partition


@pytest.fixture(scope='module')
def zkv():
    import stylus_zkvm_verifiers_amd as z
    if z.device_count() < 1:
        pytest.skip('no gfx950 device')
    return z


def _faults():
    from stylus_zkvm_verifiers_amd import _lib
    out = C.c_uint64(0)
    _lib.check(_lib.lib().zkv_diag_wait_faults(0, C.byref(out)), 'zkv_diag_wait_faults')
    return out.value


@pytest.fixture(scope='module')
def world(zkv):
    keys, tds = gm.deployed_set()
    reqs = gm.requests(keys, tds)
    model = gm.Contracts(keys)
    want = gm.expected(model, reqs)
    gm.check_coverage(keys, reqs, want)                  # the model accepts and rejects in every class, under both forms
    faults = _faults()
    s = zkv.Groth16DeployedSet(keys)
    yield s, keys, reqs, model, want
    assert _faults() == faults                           # no consumer wavefront ever waited in vain
    s.close()


def _host(s, to, blob, off):
    n = len(off) - 1
    rev, data, st = s.eth_call_batch([to[20 * i:20 * i + 20] for i in range(n)], blob, offsets=off)
    return st, rev, data


def _dev(s, to, blob, off, stream=None):
    """The device call on a caller's stream -> (statuses, resolved keys)."""
    import torch
    dev = torch.device('cuda', 0)
    n = len(off) - 1
    st = stream or torch.cuda.Stream()
    with torch.cuda.stream(st):
        d_to = torch.frombuffer(bytearray(to), dtype=torch.uint8).to(dev)
        d_cd = torch.frombuffer(bytearray(blob + b'\0'), dtype=torch.uint8).to(dev)
        d_off = torch.from_numpy(off.astype(np.int64)).to(dev)
        d_st = torch.full((n,), 255, dtype=torch.uint8, device=dev)
        d_key = torch.full((n,), 0x55555555, dtype=torch.int32, device=dev)
        s.eth_call_batch_dev(n, d_to.data_ptr(), d_cd.data_ptr(), d_off.data_ptr(), len(blob), d_st.data_ptr(), d_key.data_ptr(), st.cuda_stream)
        st.synchronize()
    return d_st.cpu().numpy(), d_key.cpu().numpy().view(np.uint32)


def _check_host(s, exp, st, rev, data):
    bad = [i for i, e in enumerate(exp) if (st[i], bool(rev[i]), data[i]) != (e[0], e[2], e[3])]
    assert not bad, (bad[:8], [(st[i], rev[i], data[i].hex(), exp[i]) for i in bad[:3]])


@pytest.mark.parametrize('n', SIZES)
def test_host_call_equals_the_model(world, n):
    s, keys, reqs, model, want = world
    to, blob, off, exp = gm.batch(reqs, want, n, 1000 + n)
    st, rev, data = _host(s, to, blob, off)
    print('n', n, 'statuses', np.bincount(st, minlength=11).tolist(), 'decode ms', s.last_wire_ms())
    _check_host(s, exp, st, rev, data)
    assert s.last_call_counts() == gm.counts(exp)
    for i, e in enumerate(exp):                          # the length rows: a bool word, an error selector or nothing
        assert len(data[i]) in (0, 4, 32) and len(data[i]) == len(e[3])


@pytest.mark.parametrize('n', SIZES)
def test_device_call_on_a_caller_stream_equals_the_model(world, n):
    s, keys, reqs, model, want = world
    to, blob, off, exp = gm.batch(reqs, want, n, 2000 + n)
    st, key = _dev(s, to, blob, off)
    bad = [i for i, e in enumerate(exp) if (st[i], key[i]) != (e[0], e[1])]
    assert not bad, (bad[:8], [(st[i], key[i], exp[i][:2]) for i in bad[:3]])
    assert s.last_call_counts() == gm.counts(exp)
    for i, e in enumerate(exp):                          # return data is rendered on the host from status and key
        assert s.eth_call_returndata(int(key[i]), int(st[i])) == (e[2], e[3]), i
    # without the key row, and on the context's own stream
    import torch
    dev = torch.device('cuda', 0)
    d_to = torch.frombuffer(bytearray(to), dtype=torch.uint8).to(dev)
    d_cd = torch.frombuffer(bytearray(blob + b'\0'), dtype=torch.uint8).to(dev)
    d_off = torch.from_numpy(off.astype(np.int64)).to(dev)
    d_st = torch.full((n,), 255, dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()
    s.eth_call_batch_dev(n, d_to.data_ptr(), d_cd.data_ptr(), d_off.data_ptr(), len(blob), d_st.data_ptr())
    s.synchronize()
    assert (d_st.cpu().numpy() == st).all()


def test_placed_requests_equal_verify_batch_on_the_decoded_triple(world):
    s, keys, reqs, model, want = world
    to, blob, off, exp = gm.batch(reqs, want, 3000, 77)
    st, _, _ = _host(s, to, blob, off)
    kk, proofs, sigs, idx = [], [], [], []
    for i, e in enumerate(exp):
        if e[0] in (gm.OK, gm.FAILED):
            v, j, proof, sig, big = model.decode(to[20 * i:20 * i + 20], blob[int(off[i]):int(off[i + 1])])
            assert v == 0 and not big
            kk.append(j); proofs.append(proof); sigs.append(sig); idx.append(i)
    assert len(idx) > 300 and len(set(kk)) == len(keys) - 1                   # every key with a method places requests
    got = s.verify_batch(kk, proofs, sigs)
    assert got.any() and not got.all()
    assert (got == (st[idx] == gm.OK)).all()
    assert set(st[idx]) == {gm.OK, gm.FAILED}
    # the ordinary set calls are untouched by the wire calls before them
    assert s.size() == len(keys) and s.signal_stride() == 32 * 128


def test_aggregate_check_on_the_smallest_batch_that_engages_it(world, monkeypatch):
    """The check engages from ZKV_AGG_MIN placed requests (64 at the least) of which 64 go to one capable key: 64 placed requests to
    the 7-IC contract, a few that are not placed, and the two offset cases."""
    s, keys, reqs, model, want = world
    monkeypatch.setenv('ZKV_AGG_MIN', '64')
    k7 = [j for j, k in enumerate(keys) if k[1] == 7][0]
    placed = [i for i, (r, w) in enumerate(zip(reqs, want)) if r[1] == k7 and w[0] in (gm.OK, gm.FAILED)]
    other = [i for i, (r, w) in enumerate(zip(reqs, want)) if w[0] not in (gm.OK, gm.FAILED)]
    assert {want[i][0] for i in placed} == {gm.OK, gm.FAILED}
    pick = [placed[i % len(placed)] for i in range(64)] + other[::9]
    to, blob, off, exp = gm.batch(reqs, want, len(pick) + 2, 5, pick=pick)
    assert gm.counts(exp)[0] == 64
    s.set_aggregate_check(False)
    st0, rev0, data0 = _host(s, to, blob, off)
    c0 = s.aggregate_counters()
    s.set_aggregate_check(True, SEED, 16)
    st1, rev1, data1 = _host(s, to, blob, off)
    st2, key2 = _dev(s, to, blob, off)
    c1 = s.aggregate_counters()
    s.set_aggregate_check(False)
    _check_host(s, exp, st0, rev0, data0)
    _check_host(s, exp, st1, rev1, data1)
    assert (st2 == st0).all() and [int(k) for k in key2] == [e[1] for e in exp]
    assert c1[0] > c0[0]                                 # sub-batches were checked in aggregate
    assert s.last_call_counts() == gm.counts(exp)
    # one placed request fewer: the check does not engage, the statuses are the same
    drop = pick[1:]
    to, blob, off, exp = gm.batch(reqs, want, len(drop) + 2, 6, pick=drop)
    s.set_aggregate_check(True, SEED, 16)
    st3, rev3, data3 = _host(s, to, blob, off)
    c2 = s.aggregate_counters()
    s.set_aggregate_check(False)
    _check_host(s, exp, st3, rev3, data3)
    assert c2 == c1


def test_a_set_of_one_contract_without_a_method_and_a_single_request(zkv):
    """n_ic = 1 alone: the signal stride is zero and every request is bad calldata or meets no contract; nothing is placed."""
    import random
    import spec_model as m
    vk, _ = m.trapdoor_vk(random.Random(3), 1)
    addr = bytes(range(40, 60))
    s = zkv.Groth16DeployedSet([(m.vk_to_words(vk), 1, 1, addr, gm.FORM_GNARK)])
    cd = gm.ol.keccak256(gm.signature(gm.FORM_GNARK, 0).encode())[:4] + bytes(256)
    rev, data, st = s.eth_call_batch([addr, addr, bytes(20)], [cd, b'', cd])
    assert list(st) == [gm.BAD_CALLDATA, gm.BAD_CALLDATA, gm.NO_CONTRACT] and list(rev) == [1, 1, 0] and data == [b'', b'', b'']
    assert s.last_call_counts() == [0, 1, 2, 0]
    s.close()

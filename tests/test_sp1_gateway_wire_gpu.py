"""eth_call batches on the SP1 gateway on the GPU (include/zkv_sp1_gateway_wire.h): every golden request of
tests/golden/gateway_wire_cases.json, both calldata forms interleaved in one batch, through the host and the device-resident entry
point; the answers do not depend on the neighbours; calldata against the decoded-input entry point; buffer geometry of the device path.
PARITY UNPINNED: the reference holds no gateway, no PLONK code and no router -- the fixture holds the answers of
tests/gateway_wire_model.py (decode, route, the route's oracle, revert data)."""
import json
import os
import random

import numpy as np
import pytest

import gateway_wire_model as gwm
from wire_util import apply_ops

HERE = os.path.dirname(os.path.abspath(__file__))
H = bytes.fromhex


@pytest.fixture(scope='module')
def zkv():
    import stylus_zkvm_verifiers_amd as z
    assert z.device_count() >= 1, 'no gfx950 device visible'
    return z


@pytest.fixture(scope='module')
def fx():
    d = json.load(open(os.path.join(HERE, 'golden', 'gateway_wire_cases.json')))
    for c in d['cases']:
        it = d['items'][c['item']]
        c['calldata'] = apply_ops(gwm.encode(c['form'], H(it['vkey']), H(it['pv']), H(it['proof'])), c['ops'])
        assert len(c['calldata']) == c['calldata_len']
    return d


@pytest.fixture(scope='module')
def gw(zkv, fx):
    g = zkv.Sp1Gateway(True, [(H(r['vk']), H(r['verifier_hash'])) for r in fx['routes']])
    yield g
    g.close()


def _interleaved(fx):
    """Every case, the two forms alternating."""
    per = [[c for c in fx['cases'] if c['form'] == f] for f in (0, 1)]
    out = []
    for k in range(max(len(p) for p in per)):
        out += [p[k] for p in per if k < len(p)]
    assert len(out) == len(fx['cases'])
    return out


def _dev(gw, blob, off, calldata_bytes, shift=0, recv=True):
    """Device-resident call: `blob` placed `shift` bytes past an allocation's start, outputs pre-filled with 255."""
    import torch
    dev = torch.device('cuda', 0)
    n = len(off) - 1
    d_buf = torch.from_numpy(np.frombuffer(bytes(shift) + bytes(blob), dtype=np.uint8).copy()).to(dev)
    d_off = torch.from_numpy(np.asarray(off, dtype=np.uint64).view(np.int64).copy()).to(dev)
    d_st = torch.full((n,), 255, dtype=torch.uint8, device=dev)
    d_rv = torch.full((n, 4), 255, dtype=torch.uint8, device=dev)
    gw.eth_call_batch_dev(n, d_buf.data_ptr() + shift, d_off.data_ptr(), calldata_bytes, d_st.data_ptr(), d_rv.data_ptr() if recv else 0,
                          torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return d_st.cpu().numpy(), d_rv.cpu().numpy()


def _check(gw, cases, rev, data, st, rv=None):
    for i, c in enumerate(cases):
        assert (int(rev[i]), data[i].hex(), int(st[i])) == (c['reverted'], c['returndata'], c['status']), (i, c['name'])
        if rv is not None:
            assert bytes(rv[i]).hex() == c['received'], (i, c['name'])


def _through_dev(gw, cases):
    calls = [c['calldata'] for c in cases]
    off = np.zeros(len(calls) + 1, dtype=np.uint64); off[1:] = np.cumsum([len(x) for x in calls])
    blob = b''.join(calls)
    st, rv = _dev(gw, blob, off, len(blob))
    out = [gw.eth_call_returndata(int(s), bytes(r)) for s, r in zip(st, rv)]
    return [o[0] for o in out], [o[1] for o in out], st, rv


@pytest.mark.gpu
def test_every_golden_case_both_forms_interleaved_through_both_entry_points(gw, fx):
    cases = _interleaved(fx)
    assert {c['form'] for c in cases[:2]} == {0, 1}
    model = gwm.Gateway(True, [(H(r['vk']), H(r['verifier_hash'])) for r in fx['routes']])
    want_counts = model.counts([c['column'] for c in cases])
    assert min(want_counts) > 0
    rev, data, st = gw.eth_call_batch([c['calldata'] for c in cases])
    _check(gw, cases, rev, data, st)
    assert gw.last_call_counts() == want_counts
    assert gw.last_route_counts() == want_counts[:-1]            # the old getter keeps its route_count + 2 columns
    assert gw.last_wire_ms() > 0
    rev, data, st, rv = _through_dev(gw, cases)
    _check(gw, cases, rev, data, st, rv)
    assert gw.last_call_counts() == want_counts
    assert gw.last_wire_ms() > 0
    assert sum(gw.last_stage_ms()) > 0


@pytest.mark.gpu
def test_an_answer_does_not_depend_on_the_neighbours(gw, fx):
    cases = _interleaved(fx)
    random.Random(0x6A7E7175).shuffle(cases)
    bad = [c['status'] == 6 for c in cases]
    assert any(bad[i] and not bad[i - 1] and not bad[i + 1] for i in range(1, len(cases) - 1))      # a bad request between good ones
    assert any(not bad[i] and bad[i - 1] and bad[i + 1] for i in range(1, len(cases) - 1))
    rev, data, st, rv = _through_dev(gw, cases)
    _check(gw, cases, rev, data, st, rv)
    rev, data, st = gw.eth_call_batch([c['calldata'] for c in cases])
    _check(gw, cases, rev, data, st)


@pytest.mark.gpu
def test_calldata_against_the_decoded_input_entry_point(gw, fx):
    """Statuses and received selectors through calldata equal those of zkv_sp1_gateway_verify_batch on the model-decoded arguments: the
    path tests/test_sp1_gateway_gpu.py checks against the oracle.  Both forms, ragged public values."""
    cases = [c for c in _interleaved(fx) if not c['ops']]
    dec = [gwm.decode(c['calldata']) for c in cases]
    assert all(d is not None and d[0] == c['form'] for d, c in zip(dec, cases))
    assert len({len(d[2]) for d in dec}) >= 6 and {d[0] for d in dec} == {0, 1}
    want_st, want_rv = gw.verify_batch([d[1] for d in dec], [d[2] for d in dec], [d[3] for d in dec])
    want_counts = gw.last_route_counts()
    _, _, st, rv = _through_dev(gw, cases)
    assert st.tolist() == want_st.tolist()
    assert rv.tolist() == want_rv.tolist()
    assert gw.last_call_counts() == want_counts + [0]
    assert {0, 1, 4, 8} <= set(st.tolist())


@pytest.mark.gpu
def test_device_path_geometry(gw, fx):
    """A blob 1, 2 and 3 bytes off alignment; requests whose offsets run backwards or past calldata_bytes (never read, BAD_CALLDATA); a form
    B request that ends at the blob's last byte; outputs pre-filled with 255 and overwritten, with and without received selectors."""
    by = {c['name']: c for c in fx['cases']}
    c0, c1 = by['U: PLONK key 1, valid'], by['B: PLONK key 2, valid, public values 33 bytes']
    c2, c3 = by['U: Groth16 real proof'], by['B: Groth16 real proof']
    c4 = by['B: last proof padding byte set [Groth16 real proof]']
    l0, l1, l2, l3, l4 = (len(c['calldata']) for c in (c0, c1, c2, c3, c4))
    blob = c2['calldata'] + c0['calldata'] + c1['calldata'] + c4['calldata'] + c3['calldata']
    x = l2 + l0 + l1
    # request:  c0        c1             backwards   c2   c0 | c1 (no call)  c4       c3 (to the last byte)   past the blob
    off = [l2, l2 + l0, x,          0,  l2,            x, x + l4, x + l4 + l3,         x + l4 + l3 + 164]
    assert off[3] < off[2] and off[-2] == len(blob) and off[-1] > len(blob)
    none = dict(status=6, received='00000000')
    want = [c0, c1, none, c2, none, c4, c3, none]
    assert [w['status'] for w in want] == [0, 0, 6, 0, 6, 6, 0, 6]
    for shift in (0, 1, 2, 3):
        st, rv = _dev(gw, blob, off, len(blob), shift)
        assert st.tolist() == [w['status'] for w in want], shift
        assert [bytes(r).hex() for r in rv] == [w['received'] for w in want], shift
        assert gw.last_call_counts() == [2, 1, 1, 0, 0, 4], shift
    st, rv = _dev(gw, blob, off, len(blob), 1, recv=False)
    assert st.tolist() == [w['status'] for w in want] and (rv == 255).all()
    # a smaller calldata_bytes than the buffer holds: the last call now lies past it
    st, rv = _dev(gw, blob, off, len(blob) - 1, 3)
    assert st.tolist() == [0, 0, 6, 0, 6, 6, 6, 6] and not rv[6].any()

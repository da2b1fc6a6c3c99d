"""eth_call batches and per-seal methods on the RISC Zero router on the GPU (include/zkv_risc0_router_wire.h):
every golden request of tests/golden/risc0_router_wire_cases.json, the four call shapes interleaved in one batch, through the host and the
device-resident entry point; the answers do not depend on the neighbours; calldata against the decoded-input call with a method row, that
call against the model and against the two batch-wide calls; batch sizes around the kernels' block sizes; buffer geometry of the device
path.  PARITY UNPINNED: the reference holds no router -- the fixture holds the answers of tests/risc0_router_wire_model.py."""
import json
import os
import random
import sys

import numpy as np
import pytest

import risc0_router_model as rm
import risc0_router_wire_model as wm
import spec_model as m

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, 'golden'))
import make_risc0_router_wire_cases as gen          # noqa: E402  (the item -> calldata rule of the fixture)

H = bytes.fromhex


@pytest.fixture(scope='module')
def zkv():
    import stylus_zkvm_verifiers_amd as z
    assert z.device_count() >= 1, 'no gfx950 device visible'
    return z


@pytest.fixture(scope='module')
def fx():
    d = json.load(open(os.path.join(HERE, 'golden', 'risc0_router_wire_cases.json')))
    for c in d['cases']:
        c['calldata'] = gen.calldata_of(d['items'][c['item']], c['form'], c['method'], c['ops'])
        assert len(c['calldata']) == c['calldata_len']
    return d


@pytest.fixture(scope='module')
def keys(fx):
    return [rm.Key(s) for s in fx['key_seeds']]


@pytest.fixture(scope='module')
def model(fx, keys):
    b = fx['builtin']
    return wm.WireRouter(rm.Router([(H(b['control_root']), H(b['bn254_control_id']))], [k.triple() for k in keys]))


@pytest.fixture(scope='module')
def rt(zkv, fx, keys):
    b = fx['builtin']
    r = zkv.RiscZeroRouter([(H(b['control_root']), H(b['bn254_control_id']))], [k.triple() for k in keys])
    assert [s.hex() for s, _, _ in r.routes()] == fx['route_selectors']
    yield r
    r.close()


def _interleaved(fx):
    """Every case, the four shapes taking turns."""
    per = [[c for c in fx['cases'] if (c['form'], c['method']) == s] for s in ((0, 0), (1, 1), (0, 1), (1, 0))]
    out = []
    for k in range(max(len(p) for p in per)):
        out += [p[k] for p in per if k < len(p)]
    assert len(out) == len(fx['cases'])
    return out


def _to_dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to(torch.device('cuda', 0))


def _dev(rt, blob, off, calldata_bytes, shift=0, optional=True):
    """Device-resident call: `blob` placed `shift` bytes past an allocation's start, outputs pre-filled with 255."""
    import torch
    dev = torch.device('cuda', 0)
    n = len(off) - 1
    d_buf = _to_dev(np.frombuffer(bytes(shift) + bytes(blob) + b'\0', dtype=np.uint8).copy())
    d_off = _to_dev(np.asarray(off, dtype=np.uint64).view(np.int64).copy())
    d_st = torch.full((n,), 255, dtype=torch.uint8, device=dev)
    d_rv = torch.full((n, 4), 255, dtype=torch.uint8, device=dev)
    d_ck = torch.full((n,), 255, dtype=torch.uint8, device=dev)
    d_ck[:] = 254
    rt.eth_call_batch_dev(n, d_buf.data_ptr() + shift, d_off.data_ptr(), calldata_bytes, d_st.data_ptr(), d_rv.data_ptr() if optional else 0,
                          d_ck.data_ptr() if optional else 0, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return d_st.cpu().numpy(), d_rv.cpu().numpy(), d_ck.cpu().numpy()


def _check(cases, rev, data, st, rv=None, ck=None):
    for i, c in enumerate(cases):
        assert (int(rev[i]), data[i].hex(), int(st[i])) == (c['reverted'], c['returndata'], c['status']), (i, c['name'])
        if rv is not None:
            assert (bytes(rv[i]).hex(), int(ck[i])) == (c['received'], c['kind']), (i, c['name'])


def _through_dev(rt, cases):
    calls = [c['calldata'] for c in cases]
    off = np.zeros(len(calls) + 1, dtype=np.uint64); off[1:] = np.cumsum([len(x) for x in calls])
    blob = b''.join(calls)
    st, rv, ck = _dev(rt, blob, off, len(blob))
    out = [rt.eth_call_returndata(int(s), bytes(r), int(k)) for s, r, k in zip(st, rv, ck)]
    return [o[0] for o in out], [o[1] for o in out], st, rv, ck


@pytest.mark.gpu
def test_every_golden_case_four_shapes_interleaved_through_both_entry_points(rt, fx, model):
    cases = _interleaved(fx)
    assert {(c['form'], c['method']) for c in cases[:4]} == {(0, 0), (0, 1), (1, 0), (1, 1)}
    want_counts = model.counts([c['column'] for c in cases])
    assert min(want_counts) > 0 and len(want_counts) == 6
    rev, data, st = rt.eth_call_batch([c['calldata'] for c in cases])
    _check(cases, rev, data, st)
    assert rt.last_call_counts() == want_counts
    assert rt.last_route_counts() == want_counts[:-1]            # the old getter keeps its route_count + 2 columns
    assert rt.last_wire_ms() > 0
    rev, data, st, rv, ck = _through_dev(rt, cases)
    _check(cases, rev, data, st, rv, ck)
    assert rt.last_call_counts() == want_counts
    assert rt.last_wire_ms() > 0
    assert sum(rt.last_stage_ms()) > 0


@pytest.mark.gpu
def test_an_answer_does_not_depend_on_the_neighbours(rt, fx):
    cases = _interleaved(fx)
    random.Random(0x7A7E7177).shuffle(cases)
    bad = [c['status'] == 6 for c in cases]
    assert any(bad[i] and not bad[i - 1] and not bad[i + 1] for i in range(1, len(cases) - 1))      # a bad request between good ones
    assert any(not bad[i] and bad[i - 1] and bad[i + 1] for i in range(1, len(cases) - 1))
    rev, data, st, rv, ck = _through_dev(rt, cases)
    _check(cases, rev, data, st, rv, ck)
    rev, data, st = rt.eth_call_batch([c['calldata'] for c in cases])
    _check(cases, rev, data, st)


def _decoded(cases):
    dec = [wm.decode(c['calldata']) for c in cases]
    assert all(d is not None and (d[0], d[1]) == (c['form'], c['method']) for d, c in zip(dec, cases))
    return [d[1] for d in dec], [d[2] for d in dec], [d[3] for d in dec], [d[4] if d[4] is not None else bytes(32) for d in dec]


@pytest.mark.gpu
def test_calldata_against_the_decoded_input_call(rt, fx):
    """Statuses and received selectors through calldata equal those of verify_call_batch on the model-decoded arguments."""
    cases = [c for c in _interleaved(fx) if not c['ops']]
    methods, seals, in_a, in_b = _decoded(cases)
    assert set(methods) == {0, 1}
    want_st, want_rv = rt.verify_call_batch(methods, seals, in_a, in_b)
    want_counts = rt.last_call_counts()
    assert want_counts[-1] == 0
    _, _, st, rv, _ = _through_dev(rt, cases)
    assert st.tolist() == want_st.tolist()
    assert rv.tolist() == want_rv.tolist()
    assert rt.last_call_counts() == want_counts
    assert set(st.tolist()) == {0, 1, 4, 8}


def _method_rows(fx):
    """Decoded rows of the plain golden cases (each item under both methods), and after every fourth a row with a method byte of 2."""
    cases = [c for c in _interleaved(fx) if not c['ops'] and c['form'] == 1]
    methods, seals, in_a, in_b = _decoded(cases)
    rows = []
    for k, row in enumerate(zip(methods, seals, in_a, in_b)):
        rows.append(row)
        if k % 4 == 1:
            rows.append((2 if k % 8 == 1 else 255,) + row[1:])
    return rows + [(2,) + rows[0][1:], (255,) + rows[1][1:]]        # (the first item is the real proof: bad rows over a seal that verifies)


@pytest.mark.gpu
def test_method_rows_against_the_model_and_the_batch_wide_calls(rt, fx, model):
    import torch
    rows = _method_rows(fx)
    methods, seals, in_a, in_b = (list(x) for x in zip(*rows))
    assert {0, 1, 2, 255} == set(methods)
    want_st, want_rv, cols = model.verify_batch(methods, seals, in_a, in_b)
    st, rv = rt.verify_call_batch(methods, seals, in_a, in_b)
    assert st.tolist() == want_st.tolist() and [bytes(r) for r in rv] == want_rv
    assert set(st.tolist()) == {0, 1, 4, 6, 8}
    assert rt.last_call_counts() == model.counts(cols) and rt.last_route_counts() == model.counts(cols)[:-1]
    # device-resident: fixed-stride slots, so the seals that fit one; outputs pre-filled, with and without the received selectors
    fit = [k for k, s in enumerate(seals) if len(s) == 260]
    assert len(fit) >= 18 and {methods[k] for k in fit} == {0, 1, 2, 255}
    dev = torch.device('cuda', 0)
    d_m = _to_dev(np.array([methods[k] for k in fit], dtype=np.uint8))
    d_s = _to_dev(np.frombuffer(b''.join(seals[k] for k in fit), dtype=np.uint8).copy())
    d_a = _to_dev(np.frombuffer(b''.join(in_a[k] for k in fit), dtype=np.uint8).copy())
    d_b = _to_dev(np.frombuffer(b''.join(in_b[k] for k in fit), dtype=np.uint8).copy())
    for recv in (True, False):
        d_st = torch.full((len(fit),), 255, dtype=torch.uint8, device=dev); d_rv = torch.full((len(fit), 4), 255, dtype=torch.uint8, device=dev)
        rt.verify_call_batch_dev(len(fit), d_m.data_ptr(), d_s.data_ptr(), d_a.data_ptr(), d_b.data_ptr(), d_st.data_ptr(), d_rv.data_ptr() if recv else 0,
                                 torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        assert d_st.cpu().tolist() == [int(want_st[k]) for k in fit]
        assert [bytes(r) for r in d_rv.cpu().numpy()] == [want_rv[k] if recv else b'\xff' * 4 for k in fit]
    # no method row: all verify
    v = [k for k in fit if methods[k] == 0]
    d_st = torch.full((len(fit),), 255, dtype=torch.uint8, device=dev)
    rt.verify_call_batch_dev(len(fit), 0, d_s.data_ptr(), d_a.data_ptr(), d_b.data_ptr(), d_st.data_ptr(), 0, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert [d_st.cpu().tolist()[fit.index(k)] for k in v] == [int(want_st[k]) for k in v]
    st0, _ = rt.verify_call_batch(None, seals, in_a, in_b)
    st_v, _ = rt.verify_batch(seals, in_a, in_b)
    assert st0.tolist() == st_v.tolist()
    # the mixed rows against the two batch-wide calls on the split halves
    for method, call in ((0, lambda k: rt.verify_batch([seals[i] for i in k], [in_a[i] for i in k], [in_b[i] for i in k])),
                         (1, lambda k: rt.verify_integrity_batch([seals[i] for i in k], [in_a[i] for i in k]))):
        half = [k for k, t in enumerate(methods) if t == method]
        h_st, h_rv = call(half)
        assert h_st.tolist() == [int(st[k]) for k in half] and h_rv.tolist() == [rv[k].tolist() for k in half], method
        assert 0 in h_st and 1 in h_st and 4 in h_st and 8 in h_st


@pytest.mark.gpu
@pytest.mark.parametrize('n', [1, 3, 4, 5, 63, 64, 65, 257])
def test_batch_sizes_around_the_block_sizes(rt, fx, model, n):
    """Four requests per workgroup in the decode, 64 lanes per wavefront, 256 seals per count block: valid and invalid cases taking turns."""
    good = [c for c in fx['cases'] if c['status'] == 0]
    other = [c for c in fx['cases'] if c['status'] != 0 and len(c['calldata']) < 600]           # (keeps the blob of the 257 small)
    rng = random.Random(0x7A7E7178 + n)
    cases = [rng.choice(good) if i % 3 == 0 else rng.choice(other) for i in range(n)]
    rev, data, st, rv, ck = _through_dev(rt, cases)
    _check(cases, rev, data, st, rv, ck)
    assert rt.last_call_counts() == model.counts([c['column'] for c in cases])


@pytest.mark.gpu
def test_device_path_geometry(rt, fx):
    """A blob 1, 2 and 3 bytes off alignment; requests whose offsets run backwards or past calldata_bytes (never read, BAD_CALLDATA); a form
    B request that ends at the blob's last byte; calldata_bytes one short; outputs pre-filled with 255 and overwritten, with and without
    the optional rows."""
    by = {c['name']: c for c in fx['cases']}
    c0, c1 = by['Uv: keyed route 0, valid'], by['Bi: keyed route 1, valid']
    c2, c3 = by['Ui: built-in route, real proof'], by['Bv: built-in route, real proof']
    c4 = by['Bv: last padding byte set [built-in route, real proof]']
    l0, l1, l2, l3, l4 = (len(c['calldata']) for c in (c0, c1, c2, c3, c4))
    blob = c2['calldata'] + c0['calldata'] + c1['calldata'] + c4['calldata'] + c3['calldata']
    x = l2 + l0 + l1
    # request:  c0        c1             backwards   c2   c0 | c1 (no call)  c4       c3 (to the last byte)   past the blob
    off = [l2, l2 + l0, x,          0,  l2,            x, x + l4, x + l4 + l3,         x + l4 + l3 + 164]
    assert off[3] < off[2] and off[-2] == len(blob) and off[-1] > len(blob)
    none = dict(status=6, received='00000000', kind=255)
    want = [c0, c1, none, c2, none, c4, c3, none]
    assert [w['status'] for w in want] == [0, 0, 6, 0, 6, 6, 0, 6]
    for shift in (0, 1, 2, 3):
        st, rv, ck = _dev(rt, blob, off, len(blob), shift)
        assert st.tolist() == [w['status'] for w in want], shift
        assert [bytes(r).hex() for r in rv] == [w['received'] for w in want], shift
        assert ck.tolist() == [w['kind'] for w in want], shift
        assert rt.last_call_counts() == [2, 1, 1, 0, 0, 4], shift
    st, rv, ck = _dev(rt, blob, off, len(blob), 1, optional=False)
    assert st.tolist() == [w['status'] for w in want] and (rv == 255).all() and (ck == 254).all()
    # a smaller calldata_bytes than the buffer holds: the last call now lies past it
    st, rv, ck = _dev(rt, blob, off, len(blob) - 1, 3)
    assert st.tolist() == [0, 0, 6, 0, 6, 6, 6, 6] and not rv[6].any() and ck[6] == 255

"""eth_call batches and per-seal methods on a RISC Zero router with a set route on the GPU (include/zkv_risc0_router_set_wire.h, DESIGN.md
section 17c): every golden request of tests/golden/risc0_router_set_wire_cases.json in one interleaved batch through the host and the
device-resident entry point, forwards and reversed; calldata against the decoded-input call and that call against the ragged call;
batch sizes around the kernels' block sizes; root-seal identity across forms and methods; blob geometry; a router without a set route
against the entry points it already has; a batch of two chunks.  Every expectation comes from tests/risc0_router_set_wire_model.py.
PARITY UNPINNED: the reference holds no router and no set verifier."""
import ctypes as C
import json
import os
import random

import numpy as np
import pytest

import risc0_router_model as rm
import risc0_router_set_model as rsm
import risc0_router_set_wire_model as swm
import risc0_router_wire_model as wm
import set_inclusion_model as sm
import spec_model as m

HERE = os.path.dirname(os.path.abspath(__file__))
H = bytes.fromhex
OK, FAILED, INVALID, BAD_CALLDATA, NOT_FOUND = 0, 1, 4, 6, 8
SHAPES = ((0, 0), (1, 1), (0, 1), (1, 0))


@pytest.fixture(scope='module')
def zkv():
    import stylus_zkvm_verifiers_amd as z
    assert z.device_count() >= 1, 'no gfx950 device visible'
    return z


@pytest.fixture(scope='module', autouse=True)
def no_gt_tables():
    """As tests/test_risc0_router_set_gpu.py: the built-in group sees a few seals per call; same statuses without its GT tables."""
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
def fx():
    return swm.load_fixture(os.path.join(HERE, 'golden', 'risc0_router_set_wire_cases.json'))


@pytest.fixture(scope='module')
def keys(fx):
    return [rm.Key(s) for s in fx['key_seeds']]


def _routes(fx, keys):
    b = fx['builtin']
    return [(H(b['control_root']), H(b['bn254_control_id']))], [k.triple() for k in keys]


@pytest.fixture(scope='module')
def model(fx, keys):
    s = rsm.SetRouter(H(fx['set_id']), *_routes(fx, keys))
    for r in fx['submitted_roots']:
        assert s.submit_root(H(r['root']), H(r['seal']))[0] == OK
    return swm.SetWireRouter(s)


@pytest.fixture(scope='module')
def rt(zkv, fx, keys):
    r = zkv.RiscZeroSetRouter(H(fx['set_id']), *_routes(fx, keys))
    assert [x[0].hex() for x in r.routes()] == fx['route_selectors']
    for s in fx['submitted_roots']:
        assert r.submit_root(H(s['root']), H(s['seal']))[0] == OK
    yield r
    r.close()


def _interleaved(fx):
    """Every case, the four shapes taking turns."""
    per = [[c for c in fx['cases'] if (c['form'], c['method']) == s] for s in SHAPES]
    out = []
    for k in range(max(len(p) for p in per)):
        out += [p[k] for p in per if k < len(p)]
    assert len(out) == len(fx['cases'])
    return out


def _to_dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to(torch.device('cuda', 0))


def _up(data, shift=0):
    return _to_dev(np.frombuffer(bytes(shift) + bytes(data) + b'\0', dtype=np.uint8).copy())


def _offsets(parts):
    off = np.zeros(len(parts) + 1, dtype=np.uint64)
    off[1:] = np.cumsum([len(x) for x in parts], dtype=np.uint64)
    return off


def _dev(handle, blob, off, calldata_bytes, shift=0, optional=True):
    """zkv_risc0_router_eth_call_ragged_dev: `blob` placed `shift` bytes past an allocation's start, outputs pre-filled with 255 (call kinds
    with 254)."""
    import torch
    from stylus_zkvm_verifiers_amd import risc0_router_set_wire as w
    dev = torch.device('cuda', 0)
    n = len(off) - 1
    d_buf = _up(blob, shift)
    d_off = _to_dev(np.asarray(off, dtype=np.uint64).view(np.int64).copy())
    d_st = torch.full((n,), 255, dtype=torch.uint8, device=dev)
    d_rv = torch.full((n, 4), 255, dtype=torch.uint8, device=dev)
    d_ck = torch.full((n,), 254, dtype=torch.uint8, device=dev)
    w.eth_call_ragged_dev(handle, n, d_buf.data_ptr() + shift, d_off.data_ptr(), calldata_bytes, d_st.data_ptr(), d_rv.data_ptr() if optional else 0,
                          d_ck.data_ptr() if optional else 0, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return d_st.cpu().numpy(), d_rv.cpu().numpy(), d_ck.cpu().numpy()


def _calls_dev(handle, calls, shift=0):
    blob = b''.join(calls)
    return _dev(handle, blob, _offsets(calls), len(blob), shift)


def _call_ragged_dev(handle, methods, seals, in_a, in_b, shift=0, recv=True):
    """zkv_risc0_router_verify_call_ragged_dev: the blob `shift` bytes past an allocation's base, the other rows one byte past theirs."""
    import torch
    from stylus_zkvm_verifiers_amd import risc0_router_set_wire as w
    dev = torch.device('cuda', 0)
    n = len(seals)
    blob = b''.join(seals)
    d_s, d_a, d_b = _up(blob, shift), _up(b''.join(in_a), 1), _up(b''.join(in_b), 1)
    d_m = _to_dev(np.array(methods, dtype=np.uint8)) if methods is not None else None
    d_off = _to_dev(_offsets(seals).view(np.int64).copy())
    d_st = torch.full((n,), 255, dtype=torch.uint8, device=dev)
    d_rv = torch.full((n, 4), 255, dtype=torch.uint8, device=dev)
    w.verify_call_ragged_dev(handle, n, d_m.data_ptr() if d_m is not None else 0, d_s.data_ptr() + shift, d_off.data_ptr(), len(blob), d_a.data_ptr() + 1,
                             d_b.data_ptr() + 1, d_st.data_ptr(), d_rv.data_ptr() if recv else 0, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return d_st.cpu().numpy(), d_rv.cpu().numpy()


def _check_rows(rows, st, rv=None, ck=None, rev=None, data=None, what=''):
    """rows: the model's eth_call rows (reverted, data, status, received, column, kind)."""
    want = [r[2] for r in rows]
    bad = [i for i in range(len(rows)) if int(st[i]) != want[i]]
    assert not bad, (what, bad[:10], [int(st[i]) for i in bad[:10]], [want[i] for i in bad[:10]])
    if rv is not None:
        assert [bytes(x) for x in rv] == [r[3] for r in rows], what
    if ck is not None:
        assert [int(k) for k in ck] == [r[5] for r in rows], what
    if rev is not None:
        assert [bool(x) for x in rev] == [bool(r[0]) for r in rows] and list(data) == [r[1] for r in rows], what


# ---------------------------------------------------------------- 1. the whole fixture, forwards and reversed, both entry points
@pytest.mark.gpu
def test_every_golden_case_interleaved_forwards_and_reversed(zkv, faults_before, rt, fx, model):
    cases = _interleaved(fx)
    assert {(c['form'], c['method']) for c in cases[:4]} == set(SHAPES)
    for order in (cases, cases[::-1]):
        calls = [c['calldata'] for c in order]
        want = model.eth_call_batch(calls)
        for c, r in zip(order, want['rows']):                         # the fixture is the model's answer, whatever the neighbours
            assert (c['reverted'], c['returndata'], c['status'], c['received'], c['column'], c['kind']) == \
                   (int(r[0]), r[1].hex(), r[2], r[3].hex(), r[4], r[5]), c['name']
        assert min(want['counts']) > 0 and len(want['counts']) == 7 and min(want['set_counts']) > 0
        rev, data, st = rt.eth_call_batch(calls)
        _check_rows(want['rows'], st, rev=rev, data=data, what='host')
        assert rt.last_call_counts() == want['counts'] and rt.last_route_counts() == want['counts'][:-1]
        assert rt.set_last_counts() == want['set_counts']
        assert rt.last_wire_ms() > 0
        st, rv, ck = _calls_dev(rt._h, calls)
        _check_rows(want['rows'], st, rv, ck, what='device')
        out = [rt.eth_call_returndata(int(s), bytes(r), int(k)) for s, r, k in zip(st, rv, ck)]
        assert [(o[0], o[1]) for o in out] == [(bool(r[0]), r[1]) for r in want['rows']]
        assert rt.last_call_counts() == want['counts'] and rt.set_last_counts() == want['set_counts']
    assert _faults() == faults_before


# ---------------------------------------------------------------- 2. calldata against the decoded call; method rows
def _decoded(cases):
    dec = [wm.decode(c['calldata']) for c in cases]
    assert all(d is not None and (d[0], d[1]) == (c['form'], c['method']) for d, c in zip(dec, cases))
    return [d[1] for d in dec], [d[2] for d in dec], [d[3] for d in dec], [d[4] if d[4] is not None else bytes(32) for d in dec]


@pytest.mark.gpu
def test_calldata_against_the_decoded_call_and_method_rows(zkv, faults_before, rt, fx, model):
    from stylus_zkvm_verifiers_amd import risc0_router_set as rs
    import torch
    cases = [c for c in _interleaved(fx) if not c['ops']]
    methods, seals, in_a, in_b = _decoded(cases)
    assert set(methods) == {0, 1}
    st_c, rv_c, _ = _calls_dev(rt._h, [c['calldata'] for c in cases])
    counts, set_counts = rt.last_call_counts(), rt.set_last_counts()
    assert counts[-1] == 0
    for shift in (0, 1):
        st, rv = _call_ragged_dev(rt._h, methods, seals, in_a, in_b, shift)
        assert st.tolist() == st_c.tolist() and rv.tolist() == rv_c.tolist(), shift
        assert rt.last_call_counts() == counts and rt.set_last_counts() == set_counts
    st, rv = rt.verify_call_batch(methods, seals, in_a, in_b)         # host buffers, staged
    assert st.tolist() == st_c.tolist() and rv.tolist() == rv_c.tolist()
    assert {OK, FAILED, INVALID, NOT_FOUND} <= set(st_c.tolist())
    # mixed rows with method bytes 2 and 255 over seals that verify (a set seal and a Groth16 seal among them)
    rows = []
    for k, row in enumerate(zip(methods, seals, in_a, in_b)):
        rows.append(row)
        if k % 4 == 1:
            rows.append((2 if k % 8 == 1 else 255,) + row[1:])
    mt, sl, a, b = (list(x) for x in zip(*rows))
    want = model.verify_call_batch(mt, sl, a, b)
    assert any(t > 1 and want['rows'][i - 1][0] == OK and want['columns'][i - 1] == swm.SET for i, t in enumerate(mt))
    st, rv = _call_ragged_dev(rt._h, mt, sl, a, b, 3)
    assert st.tolist() == [r[0] for r in want['rows']] and [bytes(x) for x in rv] == [r[1] for r in want['rows']]
    assert rt.last_call_counts() == want['counts'] and rt.set_last_counts() == want['set_counts']
    assert want['counts'][-1] == sum(1 for t in mt if t > 1) > 0
    # a row of one method against the ragged call: all verify (with and without the row), all verifyIntegrity (claim digests, no journal digests)
    dev = torch.device('cuda', 0)
    claims = [swm.in_a_of(fx['items'][c['item']], 1) for c in cases]
    ids = [H(fx['items'][c['item']]['image_id']) for c in cases]
    jds = [H(fx['items'][c['item']]['journal_digest']) for c in cases]
    n = len(seals)
    blob = b''.join(seals)
    d_s, d_off = _up(blob), _to_dev(_offsets(seals).view(np.int64).copy())

    def ragged(first, second):
        d_a, d_b = _up(b''.join(first)), (_up(b''.join(second)) if second is not None else None)
        d_st = torch.full((n,), 255, dtype=torch.uint8, device=dev); d_rv = torch.full((n, 4), 255, dtype=torch.uint8, device=dev)
        rs.verify_ragged_dev(rt._h, n, d_s.data_ptr(), d_off.data_ptr(), len(blob), d_a.data_ptr(), d_b.data_ptr() if d_b is not None else 0,
                             d_st.data_ptr(), d_rv.data_ptr(), torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        return d_st.cpu().tolist(), d_rv.cpu().tolist(), rt.set_last_counts()

    base_v, base_i = ragged(ids, jds), ragged(claims, None)
    for row, first, base in (([0] * n, ids, base_v), (None, ids, base_v), ([1] * n, claims, base_i)):
        st, rv = _call_ragged_dev(rt._h, row, seals, first, jds)
        assert (st.tolist(), rv.tolist(), rt.set_last_counts()) == base, row and row[0]
    assert base_v[0] != base_i[0]                                     # (the straggler item has its own claim digest)
    assert _faults() == faults_before


# ---------------------------------------------------------------- 3. batch sizes around the block sizes, blob shifts
@pytest.mark.gpu
@pytest.mark.parametrize('n', [1, 3, 4, 5, 63, 64, 65, 255, 256, 257])
def test_batch_sizes_and_blob_shifts(zkv, faults_before, rt, fx, model, n):
    """Four requests per workgroup in the decode, 256 lanes per workgroup and a seal per lane in the partition and the set stage's
    front: set seals and Groth16 seals, good and bad requests taking turns, the blob 0 to 3 bytes off alignment."""
    small = [c for c in fx['cases'] if len(c['calldata']) < 20000]
    pools = [[c for c in small if c['column'] == swm.SET and c['status'] == OK], [c for c in small if c['column'] >= 0],
             [c for c in small if c['column'] == swm.SET and c['status'] != OK], [c for c in small if c['status'] == BAD_CALLDATA and len(c['calldata']) < 600]]
    assert all(len(p) >= 4 for p in pools)
    rng = random.Random(0x5E7CA120 + n)
    cases = [rng.choice(pools[i % 4]) for i in range(n)]
    calls = [c['calldata'] for c in cases]
    want = model.eth_call_batch(calls)
    for shift in range(4):
        st, rv, ck = _calls_dev(rt._h, calls, shift)
        _check_rows(want['rows'], st, rv, ck, what=(n, shift))
        assert rt.last_call_counts() == want['counts'] and rt.set_last_counts() == want['set_counts'], (n, shift)
    assert _faults() == faults_before


# ---------------------------------------------------------------- 4. identity across forms and methods
@pytest.mark.gpu
def test_one_root_seal_in_four_shapes_is_one_root_job(zkv, faults_before, rt, fx, model, keys):
    rng = random.Random(0x5E7CA121)
    set_id, srouter = H(fx['set_id']), model.set_router
    rand32 = lambda: bytes(rng.randrange(256) for _ in range(32))
    ab = [(rand32(), rand32()) for _ in range(200)]
    digs = [m.receipt_claim_ok_digest(a, b) for a, b in ab]
    root, paths = sm.tree_paths([sm.leaf(d) for d in digs])
    rs = keys[0].prove(set_id, sm.root_journal(set_id, root))

    def call(i, seal):
        form, method = SHAPES[i % 4]
        return wm.encode(form, method, seal, ab[i][0] if method == 0 else digs[i], ab[i][1] if method == 0 else None)

    calls = [call(i, srouter.encode_seal(paths[i], rs)) for i in range(200)]
    want = model.eth_call_batch(calls)
    assert [r[2] for r in want['rows']] == [OK] * 200 and want['set_counts'] == (200, 1, 1, 0)
    st, rv, ck = _calls_dev(rt._h, calls, 1)
    _check_rows(want['rows'], st, rv, ck)
    assert rt.set_last_counts() == (200, 1, 1, 0) and rt.last_call_counts() == [0, 0, 0, 200, 0, 0, 0]
    # the same claims, each under a root seal of its own (an unknown selector each, so that every answer is the claim's own): 200 jobs
    body = rs[4:]
    sels = [bytes([0xE0, i, 0xA5, 0x5A]) for i in range(200)]
    calls = [call(i, srouter.encode_seal(paths[i], sels[i] + body)) for i in range(200)]
    st, rv, ck = _calls_dev(rt._h, calls, 2)
    assert st.tolist() == [NOT_FOUND] * 200 and [bytes(x) for x in rv] == sels and ck.tolist() == [2 * f + t for f, t in SHAPES] * 50
    assert rt.set_last_counts() == (200, 200, 200, 0)
    assert _faults() == faults_before


# ---------------------------------------------------------------- 5. blob geometry
@pytest.mark.gpu
def test_device_path_geometry(zkv, faults_before, rt, fx):
    """Offsets that run backwards or past calldata_bytes (never read, BAD_CALLDATA), a request that is two requests, a form B request
    that ends at the blob's last byte, calldata_bytes one short, the optional rows absent."""
    by = {c['name']: c for c in fx['cases']}
    c0, c1 = by['Uv: set seal, shared tree, leaf 0'], by['Bi: set seal, shared tree, leaf 1']
    c2, c3 = by['Ui: keyed route 0, valid'], by['Bv: set seal, depth 3, root seal of 260 bytes (keyed route 1)']
    c4 = by['Bv: last padding byte set [set seal, depth 3, valid (base of the edits)]']
    assert [c['status'] for c in (c0, c1, c2, c3, c4)] == [0, 0, 0, 0, 6]
    l0, l1, l2, l3, l4 = (len(c['calldata']) for c in (c0, c1, c2, c3, c4))
    blob = c2['calldata'] + c0['calldata'] + c1['calldata'] + c4['calldata'] + c3['calldata']
    x = l2 + l0 + l1
    # request:  c0        c1             backwards   c2   c0 | c1 (no call)  c4       c3 (to the last byte)   past the blob
    off = [l2, l2 + l0, x,          0,  l2,            x, x + l4, x + l4 + l3,         x + l4 + l3 + 164]
    assert off[3] < off[2] and off[-2] == len(blob) and off[-1] > len(blob)
    none = dict(status=6, received='00000000', kind=255)
    want = [c0, c1, none, c2, none, c4, c3, none]
    for shift in (0, 1, 2, 3):
        st, rv, ck = _dev(rt._h, blob, off, len(blob), shift)
        assert st.tolist() == [w['status'] for w in want], shift
        assert [bytes(r).hex() for r in rv] == [w['received'] for w in want], shift
        assert ck.tolist() == [w['kind'] for w in want], shift
        assert rt.last_call_counts() == [0, 1, 0, 3, 0, 0, 4], shift
        assert rt.set_last_counts() == (3, 2, 2, 0), shift
    st, rv, ck = _dev(rt._h, blob, off, len(blob), 1, optional=False)
    assert st.tolist() == [w['status'] for w in want] and (rv == 255).all() and (ck == 254).all()
    st, rv, ck = _dev(rt._h, blob, off, len(blob) - 1, 3)             # the last call now lies past calldata_bytes
    assert st.tolist() == [0, 0, 6, 0, 6, 6, 6, 6] and not rv[6].any() and ck[6] == 255
    assert rt.set_last_counts() == (2, 1, 1, 0)
    assert _faults() == faults_before


# ---------------------------------------------------------------- 6. a router without a set route
@pytest.mark.gpu
def test_a_plain_router_answers_what_its_own_entry_points_answer(zkv, faults_before):
    import torch
    from stylus_zkvm_verifiers_amd import risc0_router_set_wire as w
    import sys
    sys.path.insert(0, os.path.join(HERE, 'golden'))
    import make_risc0_router_wire_cases as gen
    d = json.load(open(os.path.join(HERE, 'golden', 'risc0_router_wire_cases.json')))
    calls = [gen.calldata_of(d['items'][c['item']], c['form'], c['method'], c['ops']) for c in d['cases']]
    b = d['builtin']
    plain = zkv.RiscZeroRouter([(H(b['control_root']), H(b['bn254_control_id']))], [rm.Key(s).triple() for s in d['key_seeds']])
    rev0, data0, st0 = plain.eth_call_batch(calls)
    counts = plain.last_call_counts()
    rev1, data1, st1 = w.eth_call_ragged(plain._h, calls)
    assert (rev1.tolist(), data1, st1.tolist()) == (rev0.tolist(), data0, st0.tolist()) and st0.tolist() == [c['status'] for c in d['cases']]
    assert w.last_ragged_call_counts(plain._h, 3) == counts == plain.last_call_counts()
    dev = torch.device('cuda', 0)
    n, blob, off = len(calls), b''.join(calls), _offsets(calls)
    d_buf, d_off = _up(blob), _to_dev(off.view(np.int64).copy())
    old = [torch.full(s, 255, dtype=torch.uint8, device=dev) for s in ((n,), (n, 4), (n,))]
    plain.eth_call_batch_dev(n, d_buf.data_ptr(), d_off.data_ptr(), len(blob), *(t.data_ptr() for t in old), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    st, rv, ck = _dev(plain._h, blob, off, len(blob))
    assert (st.tolist(), rv.tolist(), ck.tolist()) == tuple(t.cpu().tolist() for t in old)
    assert w.last_ragged_call_counts(plain._h, 3) == counts
    # the decoded call: the ragged twin of verify_call_batch
    plainc = [c for c, cs in zip(calls, d['cases']) if not cs['ops']]
    dec = [wm.decode(c) for c in plainc]
    mt, sl, a, bb = [x[1] for x in dec], [x[2] for x in dec], [x[3] for x in dec], [x[4] if x[4] is not None else bytes(32) for x in dec]
    mt[1], mt[2] = 2, 255
    want_st, want_rv = plain.verify_call_batch(mt, sl, a, bb)
    counts = plain.last_call_counts()
    st, rv = w.verify_call_ragged(plain._h, mt, sl, a, bb)
    assert st.tolist() == want_st.tolist() and rv.tolist() == want_rv.tolist()
    st, rv = _call_ragged_dev(plain._h, mt, sl, a, bb, 1)
    assert st.tolist() == want_st.tolist() and rv.tolist() == want_rv.tolist() and w.last_ragged_call_counts(plain._h, 3) == counts
    assert counts[-1] == 2
    plain.close()
    assert _faults() == faults_before


# ---------------------------------------------------------------- 7. two chunks
@pytest.mark.gpu
def test_a_calldata_batch_of_two_chunks_verifies_a_group_once_per_chunk(zkv, faults_before, rt, fx, model, keys):
    """2^20 + 3 form B verifyIntegrity requests at depth 0 with empty root seals (stored-root lookups of one digest that was never
    submitted) around three groups with members on both sides of the chunk boundary: tests/test_risc0_router_set_gpu.py's design, in
    calldata; the raw C call on numpy buffers."""
    from stylus_zkvm_verifiers_amd import _lib, risc0_router_set_wire as w
    rng = random.Random(0x5E7CA122)
    rand32 = lambda: bytes(rng.randrange(256) for _ in range(32))
    set_id, srouter = H(fx['set_id']), model.set_router
    n = (1 << 20) + 3
    bg_digest = rand32()
    background = np.frombuffer(wm.encode(1, 1, srouter.encode_seal([], b''), bg_digest), dtype=np.uint8)
    groups = []
    for g in range(3):
        dg = rand32()
        seal = srouter.encode_seal([], keys[g & 1].prove(set_id, sm.root_journal(set_id, sm.leaf(dg))))
        groups.append(np.frombuffer(wm.encode(1, 1, seal, dg), dtype=np.uint8))
        assert model.eth_call(bytes(groups[g]))[2] == OK
    assert model.eth_call(bytes(background))[2] == FAILED
    at = {5: 0, 7: 1, 9: 2, 11: 0, (1 << 20) - 1: 1, 1 << 20: 0, (1 << 20) + 1: 1, (1 << 20) + 2: 2}
    lens = np.full(n, len(background), dtype=np.uint64)
    for i, g in at.items():
        lens[i] = len(groups[g])
    off = np.zeros(n + 1, dtype=np.uint64)
    off[1:] = np.cumsum(lens)
    blob = np.empty(int(off[n]), dtype=np.uint8)
    prev = 0
    for i in sorted(at) + [n]:
        if i > prev:
            blob[int(off[prev]):int(off[i])] = np.tile(background, i - prev)
        if i < n:
            blob[int(off[i]):int(off[i + 1])] = groups[at[i]]
        prev = i + 1
    st = np.full(n, 255, dtype=np.uint8); rev = np.full(n, 255, dtype=np.uint8)
    ret = np.zeros((n, 96), dtype=np.uint8); ln = np.full(n, 255, dtype=np.uint32)
    _lib.check(w.lib().zkv_risc0_router_eth_call_ragged(rt._h, n, blob.ctypes.data, off.ctypes.data, rev.ctypes.data, ret.ctypes.data, ln.ctypes.data,
                                                        st.ctypes.data), 'zkv_risc0_router_eth_call_ragged')
    want = np.full(n, FAILED, dtype=np.uint8)
    want[list(at)] = OK
    assert (st == want).all() and (rev == (want != OK)).all()
    assert (ln[list(at)] == 0).all() and ln[0] == len(model.returndata(FAILED, bytes(4), 3)[1])
    assert rt.set_last_counts() == (n, 6, 6, n - len(at))
    assert rt.last_call_counts() == [0, 0, 0, n, 0, 0, 0]
    assert _faults() == faults_before

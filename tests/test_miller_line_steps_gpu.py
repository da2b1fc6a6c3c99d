"""The tangent and chord steps of k_miller2 as fused column sums (csrc/zkv_line_sums.h), on the device.

Known answers (include/zkv_diag_line_steps.h, one case per lane pair): the edge operands of tests/test_miller_line_steps_host.py and 64
random ones, every output against the plain formulas on integers and against the packed steps line_dbl / line_add that the existing
harness runs on the same rows (zkv_diag_primitive mapping 1 op 8), as field elements, every word below 2p.

Batches: 64 SP1 and 64 RISC Zero proofs resident in HBM -- two wavefronts of lane pairs -- with every 8th proof damaged (valid points that
the pairing rejects, so that the damage reaches the loop) and one B outside G2, through verify_batch_dev on the lane-pair mapping with the
fixed-base GT tables on and off (ZKV_GT_WINDOW_BITS=0): statuses equal the CPU oracle's byte for byte."""
import ctypes as C
import random

import numpy as np
import pytest

import spec_model as m
from test_miller_line_steps_host import RINV, _edge_cases, _model

pytestmark = pytest.mark.gpu

H = bytes.fromhex
P = m.P
N = 64
FOREIGN_B = 20


@pytest.fixture(scope='module')
def zkv():
    import stylus_zkvm_verifiers_amd as z
    assert z.device_count() >= 1, 'no gfx950 device visible'
    return z


def _words(v):
    return [(v >> (32 * i)) & 0xffffffff for i in range(8)]


def _val(row, word0):
    return sum(int(row[word0 + i]) << (32 * i) for i in range(8))


@pytest.fixture(scope='module')
def steps(zkv):
    """The cases, what the new bodies returned for them and what the packed steps returned (both raw words), run once."""
    from stylus_zkvm_verifiers_amd import _lib, diag_line_steps, diag_primitive
    rng = random.Random(0x11E7)
    cases = _edge_cases() + [[rng.randrange(2 * P) for _ in range(12)] for _ in range(64)]
    rows = []
    for c in cases:
        f = [rng.randrange(2 * P) for _ in range(12)]
        rows.append([w for v in c[:10] for w in _words(v)] + _words(c[10]) + _words(c[11]) + [w for v in f for w in _words(v)])
    n = len(rows)
    ins = np.array(rows, dtype=np.uint32)
    assert ins.shape == (n, diag_line_steps.IN_WORDS)
    new = np.zeros((n, diag_line_steps.OUT_WORDS), dtype=np.uint32)
    old = np.zeros((n, 816), dtype=np.uint32)
    u32p = C.POINTER(C.c_uint32)
    assert diag_line_steps.lib().zkv_diag_line_steps(0, n, ins.ctypes.data_as(u32p), new.ctypes.data_as(u32p)) == _lib.OK
    assert diag_primitive.lib().zkv_diag_primitive(0, 1, 8, n, ins.ctypes.data_as(u32p), old.ctypes.data_as(u32p)) == _lib.OK
    return cases, new, old


def _canon(row, word0, count):
    vals = [_val(row, word0 + 8 * k) for k in range(count)]
    assert all(v < 2 * P for v in vals)                                    # the loose range
    return [v * RINV % P for v in vals]


def test_steps_equal_plain_formulas(steps):
    """Tangent and chord with Q: T' l0 c3 c4 against the formulas on integers."""
    cases, new, _ = steps
    for c, row in zip(cases, new):
        dbl, add = _model(c)
        assert _canon(row, 0, 12) == dbl, [hex(v) for v in c]
        assert _canon(row, 96, 12) == add, [hex(v) for v in c]


def test_steps_equal_packed_steps_on_device(steps):
    """All five steps (tangent; chords with Q, -Q, psi(Q), -psi^2(Q)), the line product and the three-step chain against line_dbl /
    line_add on the same rows: T' and l0 the same field elements, c3 = l1 xs, c4 = l3 ys."""
    cases, new, old = steps
    for c, a, b in zip(cases, new, old):
        xs, ys = c[10] * RINV % P, c[11] * RINV % P
        for kind in range(5):
            got, ref = _canon(a, 96 * kind, 12), _canon(b, 96 * kind, 12)
            assert got[:8] == ref[:8], (kind, [hex(v) for v in c])
            assert got[8:10] == [v * xs % P for v in ref[8:10]] and got[10:12] == [v * ys % P for v in ref[10:12]], (kind, [hex(v) for v in c])
        assert _canon(a, 480, 12) == _canon(b, 480, 12)                    # f (l0 + c3 w + c4 w^3)
        assert _canon(a, 576, 6) == _canon(b, 576, 6)                      # T after tangent, chord, tangent


def test_z_zero_stays_zero_on_device(steps):
    cases, new, _ = steps
    seen = 0
    for c, row in zip(cases, new):
        if c[4] % P == 0 and c[5] % P == 0:
            seen += 1
            for kind in range(5):
                assert _canon(row, 96 * kind + 32, 2) == [0, 0]
            assert _canon(row, 576 + 32, 2) == [0, 0]
    assert seen >= 2


def _proofs(vm, real, seed, g2_membership_points):
    """64 proofs of the real proof's statement: re-randomisations; every 8th carries the C of another one; one has a B outside G2."""
    from stylus_zkvm_verifiers_amd import synth
    seals, _, _, _ = synth.make_batch(vm, real, N, seed, pool=4, mutate_every=0)
    out = [bytes(s) for s in seals]
    out[1] = real
    for i in range(0, N, 8):
        other = out[i + 2] if out[i + 2][196:] != out[i][196:] else out[i + 3]
        assert other[196:] != out[i][196:]
        out[i] = out[i][:196] + other[196:]
    q = next(H(''.join(c['point'])) for c in g2_membership_points if not c['in_subgroup'])
    out[FOREIGN_B] = real[:68] + q + real[196:]
    return out


def _dev(arrs):
    import torch
    return [torch.from_numpy(np.frombuffer(b''.join(a), dtype=np.uint8).copy()).to('cuda:0') for a in arrs]


def _tables(monkeypatch, tables):
    if tables == 'off':
        monkeypatch.setenv('ZKV_GT_WINDOW_BITS', '0')
    else:
        monkeypatch.delenv('ZKV_GT_WINDOW_BITS', raising=False)


@pytest.fixture(scope='module')
def sp1_batch(real_proofs, g2_membership_points):
    import oracle_lib as ol
    s = real_proofs['sp1']
    proofs = _proofs('sp1', H(s['proof']), 0x11E8, g2_membership_points)
    vks, pvs = [H(s['vkey'])] * N, [H(s['public_values'])] * N
    want = np.array([ol.sp1_verify_proof(k, p, x)[0] for k, p, x in zip(vks, pvs, proofs)], dtype=np.uint8)
    assert all(want[i] != 0 for i in list(range(0, N, 8)) + [FOREIGN_B]) and int((want == 0).sum()) == N - 9
    return vks, pvs, proofs, want


@pytest.fixture(scope='module')
def risc0_batch(real_proofs, g2_membership_points):
    import oracle_lib as ol
    r = real_proofs['risc0']
    seals = _proofs('risc0', H(r['seal']), 0x11E9, g2_membership_points)
    ids, jds = [H(r['image_id'])] * N, [H(r['journal_digest'])] * N
    orc = ol.Risc0Oracle(); orc.initialize(H(r['control_root']), H(r['bn254_control_id']))
    want = np.array([orc.verify(s, a, b)[0] for s, a, b in zip(seals, ids, jds)], dtype=np.uint8)
    assert all(want[i] != 0 for i in list(range(0, N, 8)) + [FOREIGN_B]) and int((want == 0).sum()) == N - 9
    return seals, ids, jds, want


@pytest.mark.parametrize('tables', ['on', 'off'])
def test_sp1_batch_resident_in_hbm(zkv, sp1_batch, monkeypatch, tables):
    import torch
    _tables(monkeypatch, tables)
    vks, pvs, proofs, want = sp1_batch
    d_vk, d_pv, d_pr = _dev((vks, pvs, proofs))
    d_st = torch.full((N,), 255, dtype=torch.uint8, device='cuda:0')
    v = zkv.Sp1Verifier()
    v.set_lanes_per_proof(2)
    v.verify_batch_dev(N, d_vk.data_ptr(), d_pv.data_ptr(), len(pvs[0]), d_pr.data_ptr(), d_st.data_ptr(), 0, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    got = d_st.cpu().numpy()
    assert got.tobytes() == want.tobytes(), np.flatnonzero(got != want).tolist()


@pytest.mark.parametrize('tables', ['on', 'off'])
def test_risc0_batch_resident_in_hbm(zkv, real_proofs, risc0_batch, monkeypatch, tables):
    import torch
    _tables(monkeypatch, tables)
    seals, ids, jds, want = risc0_batch
    r = real_proofs['risc0']
    d_se, d_id, d_jd = _dev((seals, ids, jds))
    d_st = torch.full((N,), 255, dtype=torch.uint8, device='cuda:0')
    v = zkv.RiscZeroVerifier()
    v.initialize(H(r['control_root']), H(r['bn254_control_id']))
    v.set_lanes_per_proof(2)
    v.verify_batch_dev(N, d_se.data_ptr(), d_id.data_ptr(), d_jd.data_ptr(), d_st.data_ptr(), 0, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    got = d_st.cpu().numpy()
    assert got.tobytes() == want.tobytes(), np.flatnonzero(got != want).tolist()

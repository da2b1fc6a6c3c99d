"""The Miller loop of the lane-pair kernels (k_miller2) with the Fp12 squaring as six direct column sums (csrc/zkv_tower_mem.h
f12m_sqr_fused_body), on the device: the smallest batches that reach the lane-pair mapping -- 33 proofs (a full wavefront of 32 lane
pairs and one pair in a second) and 96 (three wavefronts, one more than the two a SIMD holds) -- statuses against the CPU oracle byte
for byte, with the fixed-base GT tables on and off (ZKV_GT_WINDOW_BITS=0): the statuses are the same either way.  A batch holds the
real proof, re-randomised copies of it, one mutated proof (valid points that the pairing rejects, so that the mutation reaches the
loop), one proof whose B lies outside the subgroup and one whose A is the point at infinity."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

H = bytes.fromhex
REAL, MUTATED, FOREIGN_B, A_INF = 1, 7, 20, 32          # A_INF: the single pair of the second wavefront of the 33-proof batch


@pytest.fixture(scope='module')
def zkv():
    import stylus_zkvm_verifiers_amd as z
    assert z.device_count() >= 1, 'no gfx950 device visible'
    return z


def _proofs(vm, real, n, seed, g2_membership_points):
    from stylus_zkvm_verifiers_amd import synth
    seals, _, _, _ = synth.make_batch(vm, real, n, seed, pool=4, mutate_every=0)
    out = [bytes(s) for s in seals]
    out[REAL] = real
    q = next(H(''.join(c['point'])) for c in g2_membership_points if not c['in_subgroup'])
    out[FOREIGN_B] = real[:68] + q + real[196:]
    other = out[MUTATED + 2]                                                  # a valid re-randomisation with the C of another one
    assert other[196:] != out[MUTATED][196:]
    out[MUTATED] = out[MUTATED][:196] + other[196:]
    return out


@pytest.fixture(scope='module')
def risc0_batch(real_proofs, verify_corpus, g2_membership_points):
    """96 RISC Zero proofs and what the oracle says of them, computed once; the 33-proof batch is its head."""
    import oracle_lib as ol
    r = real_proofs['risc0']
    seals = _proofs('risc0', H(r['seal']), 96, 0x5171, g2_membership_points)
    ids, jds = [H(r['image_id'])] * 96, [H(r['journal_digest'])] * 96
    c = next(c for c in verify_corpus['cases'] if c['vm'] == 'risc0' and c['name'] == 'A = (0,Q) -> wraps to infinity under negate_g1')
    seals[A_INF], ids[A_INF], jds[A_INF] = H(c['seal']), H(c['image_id']), H(c['journal_digest'])
    orc = ol.Risc0Oracle(); orc.initialize(H(r['control_root']), H(r['bn254_control_id']))
    want = np.array([orc.verify(s, a, b)[0] for s, a, b in zip(seals, ids, jds)], dtype=np.uint8)
    assert want[REAL] == 0 and all(want[i] != 0 for i in (MUTATED, FOREIGN_B, A_INF)) and int((want == 0).sum()) == 93
    return seals, ids, jds, want


@pytest.fixture(scope='module')
def sp1_batch(real_proofs, g2_membership_points):
    import oracle_lib as ol
    s = real_proofs['sp1']
    real = H(s['proof'])
    proofs = _proofs('sp1', real, 96, 0x5172, g2_membership_points)
    proofs[A_INF] = real[:4] + bytes(64) + real[68:]                          # A at infinity
    vks, pvs = [H(s['vkey'])] * 96, [H(s['public_values'])] * 96
    want = np.array([ol.sp1_verify_proof(k, p, x)[0] for k, p, x in zip(vks, pvs, proofs)], dtype=np.uint8)
    assert want[REAL] == 0 and all(want[i] != 0 for i in (MUTATED, FOREIGN_B, A_INF)) and int((want == 0).sum()) == 93
    return vks, pvs, proofs, want


@pytest.mark.parametrize('tables', ['on', 'off'])
@pytest.mark.parametrize('n', [33, 96])
def test_risc0_statuses_on_lane_pairs(zkv, real_proofs, risc0_batch, monkeypatch, n, tables):
    if tables == 'off':
        monkeypatch.setenv('ZKV_GT_WINDOW_BITS', '0')
    else:
        monkeypatch.delenv('ZKV_GT_WINDOW_BITS', raising=False)
    seals, ids, jds, want = risc0_batch
    r = real_proofs['risc0']
    v = zkv.RiscZeroVerifier()
    v.initialize(H(r['control_root']), H(r['bn254_control_id']))
    v.set_lanes_per_proof(2)
    st, _ = v.verify_batch(seals[:n], ids[:n], jds[:n])
    got = np.array([int(x) for x in st], dtype=np.uint8)
    assert got.tobytes() == want[:n].tobytes(), np.flatnonzero(got != want[:n]).tolist()


@pytest.mark.parametrize('tables', ['on', 'off'])
@pytest.mark.parametrize('n', [33, 96])
def test_sp1_statuses_on_lane_pairs(zkv, sp1_batch, monkeypatch, n, tables):
    if tables == 'off':
        monkeypatch.setenv('ZKV_GT_WINDOW_BITS', '0')
    else:
        monkeypatch.delenv('ZKV_GT_WINDOW_BITS', raising=False)
    vks, pvs, proofs, want = sp1_batch
    v = zkv.Sp1Verifier()
    v.set_lanes_per_proof(2)
    st, _ = v.verify_batch(vks[:n], pvs[:n], proofs[:n])
    got = np.array([int(x) for x in st], dtype=np.uint8)
    assert got.tobytes() == want[:n].tobytes(), np.flatnonzero(got != want[:n]).tolist()

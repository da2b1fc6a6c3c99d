"""The Miller loop of the lane-pair kernels (k_miller2) with the variable-line product as six fused three-product sums
(csrc/zkv_tower_mem.h f12m_mul_by_034_body), on the device: 96 proofs per context -- three wavefronts of 32 lane pairs, one more than
the two a SIMD holds -- forced onto the lane-pair mapping, statuses against the CPU oracle byte for byte.  The batch holds the real
proof, re-randomised valid proofs, the corpus' cases whose points at infinity switch line products off (A = (0, Q), B and C at
infinity), a B outside G2, and one mutated proof per wavefront in lane pairs 0, 15 and 31 -- valid points that the pairing rejects, so that the
mutation reaches k_miller2 -- and a valid proof checked against a flipped public input."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

H = bytes.fromhex
N = 96
MUTATED = (0, 32 + 15, 64 + 31)            # wavefront 0 pair 0, wavefront 1 pair 15, wavefront 2 pair 31
REAL, FOREIGN_B, CORPUS0 = 1, 20, (5, 37, 70)


@pytest.fixture(scope='module')
def zkv():
    import stylus_zkvm_verifiers_amd as z
    assert z.device_count() >= 1, 'no gfx950 device visible'
    return z


def _proofs(vm, real, seed, g2_membership_points):
    """96 proofs of the real proof's statement: re-randomisations, the real proof, a foreign B, three mutations."""
    from stylus_zkvm_verifiers_amd import synth
    seals, _, _, _ = synth.make_batch(vm, real, N, seed, pool=4, mutate_every=0)
    out = [bytes(s) for s in seals]
    out[REAL] = real
    q = next(H(''.join(c['point'])) for c in g2_membership_points if not c['in_subgroup'])
    out[FOREIGN_B] = real[:68] + q + real[196:]
    # the three mutated proofs keep every point on its curve and in its group, so that they pass the stages before the pairing and are
    # rejected by it: a valid re-randomisation with the C of ANOTHER valid re-randomisation (the callers also flip a public-input bit of one)
    for k, i in enumerate(MUTATED):
        other = out[(i + 2) % N] if (i + 2) % N not in (REAL, FOREIGN_B) + CORPUS0 + MUTATED else out[(i + 3) % N]
        assert other[196:] != out[i][196:]
        out[i] = out[i][:196] + other[196:]
    return out


def _by_name(verify_corpus, vm, name):
    return next(c for c in verify_corpus['cases'] if c['vm'] == vm and c['name'] == name)


def test_risc0_statuses_on_lane_pairs(zkv, real_proofs, verify_corpus, g2_membership_points):
    import oracle_lib as ol
    r = real_proofs['risc0']
    seals = _proofs('risc0', H(r['seal']), 0x0341, g2_membership_points)
    ids, jds = [H(r['image_id'])] * N, [H(r['journal_digest'])] * N
    FLIPPED = 64 + 30                                                         # a valid proof of another statement: one journal bit flipped
    jds[FLIPPED] = jds[FLIPPED][:-1] + bytes([jds[FLIPPED][-1] ^ 1])
    names = ('A = (0,Q) -> wraps to infinity under negate_g1', 'B = infinity', 'C = infinity')
    for i, name in zip(CORPUS0, names):
        c = _by_name(verify_corpus, 'risc0', name)
        seals[i], ids[i], jds[i] = H(c['seal']), H(c['image_id']), H(c['journal_digest'])
    orc = ol.Risc0Oracle(); orc.initialize(H(r['control_root']), H(r['bn254_control_id']))
    want = np.array([orc.verify(s, a, b)[0] for s, a, b in zip(seals, ids, jds)], dtype=np.uint8)
    assert want[REAL] == 0 and all(want[i] != 0 for i in MUTATED + (FOREIGN_B, FLIPPED) + CORPUS0) and int((want == 0).sum()) == N - 8
    v = zkv.RiscZeroVerifier()
    v.initialize(H(r['control_root']), H(r['bn254_control_id']))
    v.set_lanes_per_proof(2)
    st, _ = v.verify_batch(seals, ids, jds)
    got = np.array([int(x) for x in st], dtype=np.uint8)
    assert got.tobytes() == want.tobytes(), np.flatnonzero(got != want).tolist()


def test_sp1_statuses_on_lane_pairs(zkv, real_proofs, verify_corpus, g2_membership_points):
    import oracle_lib as ol
    s = real_proofs['sp1']
    real = H(s['proof'])
    proofs = _proofs('sp1', real, 0x0342, g2_membership_points)
    vks, pvs = [H(s['vkey'])] * N, [H(s['public_values'])] * N
    FLIPPED = 64 + 30                                                         # a valid proof of another statement: one public-values bit flipped
    pvs[FLIPPED] = pvs[FLIPPED][:-1] + bytes([pvs[FLIPPED][-1] ^ 1])
    for i, name in zip(CORPUS0[:2], ('A = (0,Q) is NOT infinity on sp1', 'B = infinity')):
        c = _by_name(verify_corpus, 'sp1', name)
        proofs[i], vks[i], pvs[i] = H(c['proof']), H(c['vkey']), H(c['public_values'])
    proofs[CORPUS0[2]] = real[:196] + bytes(64)                               # C at infinity (the corpus has that case for RISC Zero only)
    want = np.array([ol.sp1_verify_proof(k, p, x)[0] for k, p, x in zip(vks, pvs, proofs)], dtype=np.uint8)
    assert want[REAL] == 0 and all(want[i] != 0 for i in MUTATED + (FOREIGN_B, FLIPPED) + CORPUS0) and int((want == 0).sum()) == N - 8
    v = zkv.Sp1Verifier()
    v.set_lanes_per_proof(2)
    st, _ = v.verify_batch(vks, pvs, proofs)
    got = np.array([int(x) for x in st], dtype=np.uint8)
    assert got.tobytes() == want.tobytes(), np.flatnonzero(got != want).tolist()

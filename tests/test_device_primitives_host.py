"""CPU counterpart of tests/test_device_primitives_gpu.py: the same case generators and references (tests/primitive_cases.py) through
host builds of the same harness (stylus_zkvm_verifiers_amd/csrc/zkv_selftest.h compiled by tests/host_sim/host_sim_selftest*.cpp, lanes
played by threads), so that the generators, the reference conversions and the harness are checked before any GPU time is spent; and
the argument checks of zkv_diag_primitive, which happen before any launch."""
import ctypes as C

import numpy as np
import pytest

import primitive_cases as pc


@pytest.mark.parametrize('op,n', [(0, 600), (1, 600), (2, 300), (3, 300), (4, 600), (5, 300), (6, 300), (7, 200), (8, 64 * 8 + 1),
                                  (9, 64 * 16 + 1), (10, 64 * 16 + 1)])
def test_lane_ops_on_the_host_build(op, n):
    ins = pc.cases_for(0, op, n, 7)
    if (0, op) in pc.PREDICATE_OPS:
        pc.assert_predicate_cases_bite(0, op, ins)
    if (0, op) in pc.G2_OPS:
        pc.assert_g2_cases_bite(0, op, ins)
    pc.check(0, op, ins, pc.run_host(0, op, ins))


@pytest.mark.parametrize('mapping,op,n', [(1, 0, 200), (1, 1, 600), (1, 2, 300), (1, 3, 9), (1, 4, 9), (2, 0, 9), (2, 1, 9), (3, 0, 5), (3, 1, 5),
                                          (1, 5, 32 * 12 + 1), (1, 6, 32 * 12 + 1), (1, 7, 32 * 12 + 1), (2, 2, 4 * 24 + 1), (3, 2, 48 + 1),
                                          (1, 8, 32 * 12 + 1), (1, 9, 32 * 6 + 1), (2, 3, 4 * 24 + 1), (3, 3, 48 + 1)])
def test_pair_and_wide_ops_on_the_host_build(mapping, op, n):
    ins = pc.cases_for(mapping, op, n, 7)
    if (mapping, op) in pc.PREDICATE_OPS:
        pc.assert_predicate_cases_bite(mapping, op, ins)
    if (mapping, op) in pc.G2_OPS:
        pc.assert_g2_cases_bite(mapping, op, ins)
    pc.check(mapping, op, ins, pc.run_host(mapping, op, ins))


@pytest.mark.parametrize('mapping,op', sorted(pc.BOUND_OPS))
def test_raw_operand_bounds_on_the_host_build(mapping, op):
    """raw operands at the bounds of the contract (2p - 1 everywhere, hot against cold, full limbs): the generators, the condition on
    the inputs alone, and the references, before any GPU time is spent"""
    ins = pc.bound_cases_for(mapping, op)
    pc.assert_bound_cases_bite(mapping, op, ins)
    pc.check(mapping, op, ins, pc.run_host(mapping, op, ins))


def test_bound_condition_bites():
    """assert_bound_cases_bite fails when one structured pattern is taken out of a batch (each case that holds it replaced by a
    value-domain case)"""
    for mapping, op, drop in ((1, 3, lambda r: r[0:12] == [pc.HOT, pc.COLD] * 6 and r[12:24] == [pc.ALL32] * 12),
                              (1, 3, lambda r: r[0:12] == [pc.COLD] * 12 and r[12:24] == [pc.COLD] * 10 + [pc.HOT] * 2),
                              (1, 4, lambda r: all(v >= pc.P for v in r[6:12]) and all(v < pc.P for v in r[0:6])),
                              (1, 8, lambda r: r[12:24] == [pc.HOT] * 12 and r[10:12] == [pc.COLD] * 2),
                              (0, 10, lambda r: r == [pc.ALL32] * 14),
                              (0, 7, lambda r: r[2] == pc.ALL29),
                              (0, 9, lambda r: r[15] == 2 * pc.P - 2)):
        ins = pc.bound_cases_for(mapping, op)
        pc.assert_bound_cases_bite(mapping, op, ins)
        plain = pc.cases_for(mapping, op, 1, 3)[0]
        cut = [plain if drop([pc._fp_of(w, k) for k in range(len(w) // 8)]) else w for w in ins]
        assert cut != ins
        with pytest.raises(AssertionError):
            pc.assert_bound_cases_bite(mapping, op, cut)


def test_references_agree_with_spec_model():
    """the shortcuts of the references: the linear Frobenius against f12pow(a, p^k), the slot <-> w-basis conversion round trip"""
    import random
    import spec_model as m
    rng = random.Random(3)
    a = [rng.randrange(m.P) for _ in range(12)]
    assert pc.slots_to_f12(pc.f12_to_slots(a)) == a
    for k in (1, 2, 3):
        assert pc.f12_frob(a, k) == m.f12pow(a, m.P ** k)
    c = pc.cyclotomic_pool()[0]
    assert m.f12mul(c, pc.f12_conj(c)) == m.F12_ONE           # cyclotomic: the conjugate is the inverse
    lam = m.g1_mul((1, 2), pc.GLV_LAMBDA)                       # the GLV endomorphism: lambda (x, y) = (beta x, y), beta^3 = 1
    assert lam[1] == 2 and lam[0] != 1 and pow(lam[0], 3, m.P) == 1


def test_predicate_references_agree_with_spec_model(g2_membership_points):
    """The `closes` reference against spec_model's own Frobenius on the twist: T = -psi^3(B) closes for the G2 generator and for subgroup
    points of the fixture, under any Z; for a twist point outside the subgroup the point the loop's 88 steps arrive at,
    [6u+2]B + psi(B) - psi^2(B) (formed with the group law; the line formulas are not replayed), does not.  For a subgroup point that
    sum IS -psi^3(B).  And is_one / eq_conj on the value-domain 1 and on a cyclotomic element and its inverse."""
    import random
    import spec_model as m
    rng = random.Random(11)
    H = lambda h: int(h, 16)
    pts = []
    for c in g2_membership_points:
        xi, xr, yi, yr = (H(h) for h in c['point'])             # EIP-197 order
        pt = ((xr, xi), (yr, yi))
        if m.g2_on_curve(pt):
            pts.append((pt, c['in_subgroup']))
    inside = [m.G2_GEN] + [p for p, ok in pts if ok][:2]
    outside = next(p for p, ok in pts if not ok)
    assert len(inside) == 3 and all(m.g2_in_subgroup(p) for p in inside) and not m.g2_in_subgroup(outside)
    psi = m.g2_frobenius

    def loop_end(b): return m.g2_add(m.g2_add(m.g2_mul(b, m.ATE_LOOP), psi(b)), m.g2_neg(psi(psi(b))))

    def verdict(t, b, z):
        raw = [pc._mont(c) for c in m.f2mul(t[0], z) + m.f2mul(t[1], z) + z + b[0] + b[1]]
        (name, miss, holds, lanes), = pc.predicate_reference(1, 7, pc._fpw(raw))
        return holds
    for b in inside:
        t = m.g2_neg(psi(psi(psi(b))))
        assert loop_end(b) == t
        for z in ((1, 0), (rng.randrange(pc.P), rng.randrange(pc.P))):
            assert verdict(t, b, z)
            assert not verdict(m.g2_neg(t), b, z) and not verdict(t, m.g2_neg(b), z)
    t = loop_end(outside)
    assert t is not None and not verdict(t, outside, (1, 0)) and not verdict(t, outside, (rng.randrange(pc.P), rng.randrange(pc.P)))
    cyc = pc.cyclotomic_pool()[1]
    inv = m.f12pow(cyc, m.P ** 12 - 2)
    one = pc.predicate_reference(1, 6, pc._fpw(pc._f12_raw(m.F12_ONE) + pc._f12_raw(m.F12_ONE)))
    assert [r[2] for r in one] == [True, True, True]
    rows = pc.predicate_reference(1, 6, pc._fpw(pc._f12_raw(cyc) + pc._f12_raw(inv)))
    assert [r[2] for r in rows] == [False, False, True] and m.f12mul(cyc, inv) == m.F12_ONE
    rows = pc.predicate_reference(1, 6, pc._fpw(pc._f12_raw(cyc) + pc._f12_raw(cyc)))
    assert not rows[2][2] and rows[2][1] == list(range(6, 12))


def test_line_references_agree_with_spec_model():
    """The restated line formulas (pc.line_dbl_ref, line_add_ref, aff_dbl_ref, aff_add_ref) on their own, before anything is compared
    with them: T' is spec_model's double / sum of the inputs, projectively; l0 y + l1 x + l3 vanishes at the affine T and, for a chord,
    at Q; the affine steps give proportional lines and the same point; the four chord operands are Q, -Q, psi(Q), -psi^2(Q) by
    spec_model's Frobenius; and the exceptional inputs leave Z' = 0, which then stays 0."""
    import random
    import spec_model as m
    rng = random.Random(5)
    sub, out = pc.g2_pools()
    assert all(m.g2_in_subgroup(q) for q in sub[:3]) and not any(m.g2_in_subgroup(q) for q in out[:3] + out[-3:])
    ev = lambda l0, l1, l3, pt: m.f2add(m.f2add(m.f2mul(l0, pt[1]), m.f2mul(l1, pt[0])), l3)
    for j, q in enumerate(sub[:4] + out[:4] + [m.g2_frobenius(sub[1])]):
        t = m.g2_mul(q, 2 + j)
        s = (rng.randrange(1, pc.P), rng.randrange(1, pc.P))
        T = (m.f2mul(t[0], s), m.f2mul(t[1], s), s)
        T2, l0, l1, l3 = pc.line_dbl_ref(T)
        assert pc.proj_to_aff(T2) == m.g2_add(t, t) and ev(l0, l1, l3, t) == (0, 0)
        at, nl, c = pc.aff_dbl_ref(t)
        assert at == m.g2_add(t, t) and m.f2mul(nl, l0) == l1 and m.f2mul(c, l0) == l3
        for kind in (1, 2, 3, 4):
            qk = pc.step_q(q, kind)
            assert qk == [q, m.g2_neg(q), m.g2_frobenius(q), m.g2_neg(m.g2_frobenius(m.g2_frobenius(q)))][kind - 1]
            T2, l0, l1, l3 = pc.line_add_ref(T, qk)
            assert pc.proj_to_aff(T2) == m.g2_add(t, qk) and ev(l0, l1, l3, t) == (0, 0) and ev(l0, l1, l3, qk) == (0, 0)
            at, nl, c = pc.aff_add_ref(t, qk)
            assert at == m.g2_add(t, qk) and m.f2mul(nl, l0) == l1 and m.f2mul(c, l0) == l3
        assert pc.proj_to_aff(pc.chain_ref(T, q)) == m.g2_add(m.g2_add(m.g2_add(t, t), q), m.g2_add(m.g2_add(t, t), q))
        # the exceptional inputs: Z' = 0 at once, and Z = 0 is absorbing
        S = lambda pt: (m.f2mul(pt[0], s), m.f2mul(pt[1], s), s)
        dead = [pc.line_add_ref(S(q), q)[0], pc.line_add_ref(S(m.g2_neg(q)), q)[0], pc.line_dbl_ref(((0, 0), s, (0, 0)))[0],
                pc.line_add_ref(((0, 0), s, (0, 0)), q)[0], pc.line_dbl_ref((s, t[0], (0, 0)))[0], pc.line_add_ref((s, t[0], (0, 0)), q)[0],
                pc.line_dbl_ref((s, (0, 0), t[1]))[0]]
        for D in dead:
            assert D[2] == (0, 0) and pc.line_dbl_ref(D)[0][2] == (0, 0) and pc.line_add_ref(D, q)[0][2] == (0, 0) and pc.chain_ref(D, q)[2] == (0, 0)
    half = m.g2_mul(sub[0], (m.R + 1) // 2)                    # 2 T = Q: the chord of the chain meets the tangent
    assert pc.chain_ref(half + ((1, 0),), sub[0])[2] == (0, 0) and pc.line_dbl_ref(half + ((1, 0),))[0][2] != (0, 0)


def test_harness_tables_agree():
    """selftest_io (both host builds), primitive_cases.IO and, for the G2 ops, the word counts in include/zkv_diag_primitive.h"""
    import os
    import re
    seen = {}
    for paired in (False, True):
        L = pc.host_lib(paired)
        for mapping in range(-1, 5):
            for op in range(-1, 14):
                i, o = C.c_int(0), C.c_int(0)
                if L.hs_selftest_io(mapping, op, C.byref(i), C.byref(o)) == 0:
                    seen[(mapping, op)] = (i.value, o.value)
    assert seen == pc.IO
    hdr = open(os.path.join(os.path.dirname(pc.HERE), 'include', 'zkv_diag_primitive.h')).read()
    parts = re.split(r'\n \*   mapping (\d)', hdr)
    text = {int(parts[k]): parts[k + 1] for k in range(1, len(parts), 2)}
    for (mapping, op) in sorted(pc.G2_OPS - {(3, 3)}):
        seg = re.search(r'\n \*     op %d .*?(?=\n \*     op \d|\Z)' % op, text[mapping], flags=re.S).group(0)
        i, o = pc.IO[(mapping, op)]
        assert re.search(r'\b%d\) ->' % i, seg), (mapping, op, i)
        if mapping < 2:
            assert '(%d)' % o in seg.split('->', 1)[1], (mapping, op, o)
        else:
            assert '(%d words for mapping 2, %d for mapping 3)' % (o, pc.IO[(3, op)][1]) in seg, (mapping, op, o)


def test_header_declares_exactly_the_harness_symbols():
    """include/zkv_diag_primitive.h is a companion of zkv.h: its entry point is bound by diag_primitive.SYMBOLS, not _lib.SYMBOLS"""
    import os
    import re
    from stylus_zkvm_verifiers_amd import _lib, diag_primitive
    root = os.path.dirname(pc.HERE)
    hdr = open(os.path.join(root, 'include', 'zkv_diag_primitive.h')).read()
    declared = set(re.findall(r'\b(zkv_\w+)\s*\(', re.sub(r'/\*.*?\*/', '', hdr, flags=re.S)))
    assert declared == set(diag_primitive.SYMBOLS) == {'zkv_diag_primitive'}
    assert '#include "zkv.h"' in hdr and '#define ZKV_DIAG_PRIMITIVE_MAX_CASES %d' % diag_primitive.MAX_CASES in hdr
    zkv_h = open(os.path.join(root, 'include', 'zkv.h')).read()
    for s in declared:
        assert s not in zkv_h and s not in _lib.SYMBOLS, s
    L = diag_primitive.lib()                  # binds every symbol: AttributeError if one is not exported
    assert all(hasattr(L, s) for s in declared)


def test_diag_primitive_argument_checks():
    from stylus_zkvm_verifiers_amd import _lib, diag_primitive
    L = diag_primitive.lib()
    buf = np.zeros(4096, dtype=np.uint32)
    p = buf.ctypes.data_as(C.POINTER(C.c_uint32))
    for mapping, op, n in ((0, 11, 1), (0, -1, 1), (1, 10, 1), (2, 4, 1), (3, 4, 1), (4, 0, 1), (-1, 0, 1), (0, 0, 0), (1, 3, 0), (0, 0, diag_primitive.MAX_CASES + 1)):
        assert L.zkv_diag_primitive(0, mapping, op, n, p, p) == _lib.ERR_INVALID_ARG, (mapping, op, n)
    assert L.zkv_diag_primitive(0, 0, 0, 1, None, p) == _lib.ERR_INVALID_ARG
    for dev in (-1, 99):                       # no such device (on a machine without a GPU every index is one)
        assert L.zkv_diag_primitive(dev, 0, 0, 1, p, p) == _lib.ERR_NO_DEVICE

"""The tangent and chord steps of the lane-pair Miller loop as fused column sums (csrc/zkv_line_sums.h line_dbl_sums / line_add_sums)
against the packed forms line_dbl / line_add (csrc/zkv_curve.h) followed by the two scalings of the line coefficients, in the host
emulation of a lane pair (tests/host_sim/host_sim_line_steps.cpp).  CPU only.

The host build forms every update of a 64-bit column again in 128 bits and counts the updates that differ, and the operands of every sum
piece that leave their contract (ZKV_SHADOW_COLS): the unit and value bounds written next to each sum in zkv_line_sums.h are checked
where they are tightest (all-ones limbs, the largest reduced values)."""
import ctypes as C
import os
import random
import subprocess

import pytest

import spec_model as m

HERE = os.path.dirname(os.path.abspath(__file__))
H = bytes.fromhex
P = m.P
R261 = pow(2, 261, P)
RINV = pow(R261, -1, P)
TANGENTS, CHORDS = 65, 23                      # line steps of the optimal-ate loop
# multiply-adds a lane: charged (the packed form and the two scalings) and issued by the column sums
DBL_CHARGE, ADD_CHARGE = 4 * 243 + 6 * 162 + 2 * 162, 11 * 243 + 2 * 162 + 2 * 162
DBL_ISSUED = 81 * (2 + 3 + 2 + 3 + 3 + 2 + 2 + 2 + 3 + 3 + 3) + 2 * 8        # b h c e m 3X^2 c3 c4 T.x T.y T.z, and two tripling carry passes
ADD_ISSUED = 81 * (3 + 3 + 5 + 2 + 2 + 2 + 3 + 3 + 2 + 3 + 3 + 5 + 3)        # s t l3 c4 c3 d e g c f T.x T.y T.z
DBL_EXCESS, ADD_EXCESS = DBL_ISSUED - DBL_CHARGE, ADD_ISSUED - ADD_CHARGE


@pytest.fixture(scope='module')
def hl():
    src = os.path.join(HERE, 'host_sim', 'host_sim_line_steps.cpp')
    lib = os.path.join(HERE, 'host_sim', 'libhost_sim_line_steps.so')
    csrc = os.path.join(HERE, '..', 'stylus_zkvm_verifiers_amd', 'csrc')
    deps = [src] + [os.path.join(csrc, f) for f in os.listdir(csrc) if f.endswith('.h')]
    if not os.path.exists(lib) or os.path.getmtime(lib) < max(os.path.getmtime(d) for d in deps):
        subprocess.check_call(['g++', '-O2', '-std=c++17', '-fPIC', '-shared', '-pthread', '-Wno-unknown-pragmas', '-o', lib, src])
    L = C.CDLL(lib)
    L.hls_steps.argtypes = [C.c_int] + [C.c_void_p] * 6
    L.hls_miller.argtypes = [C.c_int, C.c_void_p, C.c_uint32] + [C.c_void_p] * 5
    L.hls_fat_constants.argtypes = [C.c_void_p]
    return L


def _run(hl, cases):
    """cases: lists of 12 integers X0 X1 Y0 Y1 Z0 Z1 qx0 qx1 qy0 qy1 xs ys.  Returns per case the canonical outputs of the four bodies
    (T.x T.y T.z l0 c3 c4, real and imaginary part), the column-check counters, the loose-range flags and the counters."""
    n = len(cases)
    buf = b''.join(v.to_bytes(32, 'little') for c in cases for v in c)
    assert len(buf) == n * 96 * 4
    out = C.create_string_buffer(n * 4 * 96 * 4)
    shadow = (C.c_ulonglong * 8)(); loose = (C.c_int * 4)(); mads = (C.c_longlong * 12)(); muls = (C.c_ulonglong * 4)()
    assert hl.hls_steps(n, buf, out, shadow, loose, mads, muls) == 4
    res = []
    for i in range(n):
        per = []
        for b in range(4):
            o = (i * 4 + b) * 384
            per.append([int.from_bytes(out.raw[o + 32 * k: o + 32 * k + 32], 'little') for k in range(12)])
        res.append(per)
    return res, [int(x) for x in shadow], [int(x) for x in loose], [int(x) for x in mads], [int(x) for x in muls]


def _check(hl, cases):
    res, shadow, loose, _, _ = _run(hl, cases)
    for i, per in enumerate(res):
        assert per[0] == per[1], ('tangent', i, [hex(v) for v in cases[i]])       # all six outputs, as field elements
        assert per[2] == per[3], ('chord', i, [hex(v) for v in cases[i]])
        assert all(v < P for b in per for v in b)
    for b in range(4):
        assert shadow[2 * b] > 0 and shadow[2 * b + 1] == 0, (b, shadow)           # no column left its 128-bit value, no operand its contract
        assert loose[b] == 1, b                                                    # every output below 2p
    return res


def _f2(a, b):
    return ((a[0] * b[0] - a[1] * b[1]) % P, (a[0] * b[1] + a[1] * b[0]) % P)


def _sub(a, b):
    return ((a[0] - b[0]) % P, (a[1] - b[1]) % P)


def _k(k, a):
    return (k * a[0] % P, k * a[1] % P)


def _model(c):
    """Both steps on plain integers (the homogeneous formulas of line_dbl / line_add), from the Montgomery-domain inputs; canonical."""
    X, Y, Z, qx, qy = (((c[2 * i] * RINV) % P, (c[2 * i + 1] * RINV) % P) for i in range(5))
    xs, ys = c[10] * RINV % P, c[11] * RINV % P
    inv2 = pow(2, -1, P)
    b3 = _k(3, _f2((3, 0), (pow(82, -1, P) * 9 % P, -pow(82, -1, P) % P)))       # 3 b', b' = 3 / (9 + u)
    a = _k(inv2, _f2(X, Y)); b = _f2(Y, Y); cc = _f2(Z, Z); e = _f2(b3, cc); f = _k(3, e)
    g = _k(inv2, (b[0] + f[0], b[1] + f[1])); h = _k(2, _f2(Y, Z)); j = _f2(X, X); e2 = _f2(e, e)
    dbl = [_f2(a, _sub(b, f)), _sub(_f2(g, g), _k(3, e2)), _f2(b, h), _k(-1, h), _k(3 * xs, j), _k(ys, _sub(e, b))]
    th = _sub(Y, _f2(qy, Z)); la = _sub(X, _f2(qx, Z))
    c2 = _f2(th, th); d = _f2(la, la); e = _f2(la, d); f = _f2(Z, c2); g = _f2(X, d)
    h = _sub((e[0] + f[0], e[1] + f[1]), _k(2, g))
    add = [_f2(la, h), _sub(_f2(th, _sub(g, h)), _f2(e, Y)), _f2(Z, e), la, _k(-xs, th), _k(ys, _sub(_f2(th, qx), _f2(la, qy)))]
    flat = lambda o: [v % P for t in o for v in t]
    return flat(dbl), flat(add)


def _edge_values():
    top = (2 * P - 1) >> 232
    vmax = (top << 232) - 1                                                # limbs 0 .. 7 all ones below 2p
    assert vmax < 2 * P
    return [0, 1, P - 1, 2 * P - 1, vmax]


def _edge_cases():
    one = R261
    ev = _edge_values()
    cases = []
    for v in ev:                                                           # every coordinate of T and Q at the same edge ...
        for s in (one, v):
            cases.append([v] * 10 + [s, s])
    rng = random.Random(0x11E5)
    for v in ev:                                                           # ... and one coordinate (or one component) at a time
        for k in range(10):
            c = [rng.randrange(2 * P) for _ in range(10)] + [one, one]
            c[k] = v
            cases.append(c)
    for v in ev:                                                           # edge scalings
        cases.append([rng.randrange(2 * P) for _ in range(10)] + [v, v])
    return cases


def test_fat_constants(hl):
    """The borrow-free multiples of p the bodies derive: the form of 8p is the header's constant; each has the stated value and limbs."""
    out = (C.c_uint32 * 36)()
    hl.hls_fat_constants(out)
    fat8 = [0x23e7ea38, 0x282305b5, 0x23951a77, 0x36a91686, 0x2c2ecbbf, 0x36da0604, 0x25370a07, 0x32e1319f, 0x01832272]
    assert list(out[:9]) == fat8
    for k, (mult, lift) in enumerate(((8, 1), (2, 1), (5, 1), (4, 2))):
        limbs = list(out[9 * k: 9 * k + 9])
        assert sum(v << (29 * i) for i, v in enumerate(limbs)) == mult * P
        assert all((lift << 29) - lift <= v < ((lift + 1) << 29) for v in limbs[:8])


def test_line_steps_equal_packed_forms_on_edges(hl):
    cases = _edge_cases()
    res = _check(hl, cases)
    for c, per in zip(cases, res):
        dbl, add = _model(c)
        assert per[1] == dbl and per[3] == add, [hex(v) for v in c]
    assert cases[0][10] == cases[0][11] == R261                            # scalings one: c3 and c4 are l1 and l3 themselves


def test_z_zero_stays_zero(hl):
    """Z = 0 is absorbing for both steps (the subgroup verdict of miller_point_closes rests on it), in either representative of 0."""
    rng = random.Random(0x2E0)
    cases = []
    for z in ((0, 0), (P, P), (0, P), (P, 0)):
        for _ in range(4):
            c = [rng.randrange(2 * P) for _ in range(10)] + [R261, rng.randrange(2 * P)]
            c[4], c[5] = z
            cases.append(c)
    res = _check(hl, cases)
    for per in res:
        assert per[1][4:6] == [0, 0] and per[3][4:6] == [0, 0]


def test_line_steps_equal_packed_forms_on_random_points(hl):
    """256 seeded random operands anywhere in the loose range, and against the plain formulas."""
    rng = random.Random(0x11E6)
    cases = [[rng.randrange(2 * P) for _ in range(12)] for _ in range(256)]
    res = _check(hl, cases)
    for c, per in zip(cases[:16], res[:16]):
        dbl, add = _model(c)
        assert per[1] == dbl and per[3] == add


def test_counters_per_step(hl):
    """A step is CHARGED what the packed form and its two scalings are; what the column sums issue beyond that (a tangent step more, a
    chord step less: the excess is signed) is in zkv_line_mad_excess_counter and not in zkv_mad_issued_counter.  The 128-bit check sees
    every column update of the sums."""
    n = 3
    _, shadow, _, mads, muls = _run(hl, [[1] * 12] * n)
    ch0, is0, ex0, ch1, is1, ex1, ch2, is2, ex2, ch3, is3, ex3 = mads
    assert ch0 == is0 == ch1 == is1 == 2 * n * DBL_CHARGE and ex0 == 0
    assert ch2 == is2 == ch3 == is3 == 2 * n * ADD_CHARGE and ex2 == 0
    assert ex1 == 2 * n * DBL_EXCESS and ex3 == 2 * n * ADD_EXCESS
    assert (DBL_EXCESS, ADD_EXCESS) == (16, -162)
    assert muls[0] == muls[1] == 2 * n * 16 and muls[2] == muls[3] == 2 * n * 26
    # column updates: 81 a product, and 81 + 17 a reduction
    assert shadow[2] == 2 * n * (81 * (1 + 2 + 1 + 2 + 2 + 1 + 1 + 1 + 2 + 2 + 2) + 11 * 98) and shadow[3] == 0
    assert shadow[6] == 2 * n * (81 * (2 + 2 + 4 + 1 + 1 + 1 + 2 + 2 + 1 + 2 + 2 + 4 + 2) + 13 * 98) and shadow[7] == 0


from test_kernel_math_host import hs  # noqa: E402,F401  (the one-value-per-lane host build: its fixture, not a copy of its recipe)

FL_A_INF = 2


def _loop(hl, sums, t, flags, norm, b):
    out = (C.c_uint32 * 192)(); verdict = (C.c_int * 2)(); ops = (C.c_longlong * 5)()
    assert hl.hls_miller(sums, t, flags, norm, b, out, verdict, ops) == 1
    return list(out[:96]), list(out[96:]), list(verdict), [int(x) for x in ops]


def test_miller_loop_equals_loop_with_packed_line_steps(hl, hs, real_proofs, verify_corpus):
    """The flat loop the lane-pair kernels run, all 88 line steps, on the two real proofs: the same Miller value coefficient by
    coefficient, the same GT value and the same verdicts whichever bodies step the point; no column update differs from its 128-bit form;
    the charge is the same and the line steps report their excess, 65 tangent and 23 chord steps, both lanes.  The corpus's proofs with
    B outside G2 are still rejected by the loop's closing test, also with A at infinity."""
    hs.hs_prepare.restype = C.c_void_p
    r0, s = real_proofs['risc0'], real_proofs['sp1']
    cr, cid = H(r0['control_root']), H(r0['bn254_control_id'])
    v = m.Risc0Verifier(); v.initialize(cr, cid)
    sig = v.signals(m.receipt_claim_ok_digest(H(r0['image_id']), H(r0['journal_digest'])))
    cases = [(0, cr, cid, H(r0['seal'])[4:], m.be32(sig[2]), m.be32(sig[3])),
             (1, None, None, H(s['proof'])[4:], H(s['vkey']), m.be32(m.sp1_hash_public_values(H(s['public_values']))))]
    for args in cases:
        fl = C.c_uint32(0); norm = (C.c_uint32 * 48)(); b = (C.c_uint32 * 32)()
        t = hs.hs_prepare(*args, C.byref(fl), norm, b)
        assert t
        f_new, gt_new, v_new, ops_new = _loop(hl, 1, t, fl.value, norm, b)
        f_old, gt_old, v_old, ops_old = _loop(hl, 0, t, fl.value, norm, b)
        assert f_new == f_old and gt_new == gt_old and any(f_new[8:])
        assert v_new == v_old == [1, 1]                                   # B in G2, proof accepted
        assert ops_new[0] > 0 and ops_new[1] == 0 and ops_old[1] == 0
        assert ops_new[3] == ops_old[3] and ops_new[4] == ops_old[4]      # charged and zkv_mad_issued_counter: unchanged
        assert ops_new[2] == 2 * (TANGENTS * DBL_EXCESS + CHORDS * ADD_EXCESS) and ops_old[2] == 0
    bad = [c for c in verify_corpus['cases'] if c['vm'] == 'risc0' and c['name'] == 'B out of subgroup (on twist)']
    assert len(bad) == 1
    c = bad[0]
    sg = v.signals(m.receipt_claim_ok_digest(H(c['image_id']), H(c['journal_digest'])))
    fl = C.c_uint32(0); norm = (C.c_uint32 * 48)(); b = (C.c_uint32 * 32)()
    t = hs.hs_prepare(0, cr, cid, H(c['seal'])[4:], m.be32(sg[2]), m.be32(sg[3]), C.byref(fl), norm, b)
    assert t
    for extra in (0, FL_A_INF):
        f_new, gt_new, v_new, ops_new = _loop(hl, 1, t, fl.value | extra, norm, b)
        f_old, gt_old, v_old, _ = _loop(hl, 0, t, fl.value | extra, norm, b)
        assert v_new[0] == v_old[0] == 0                                  # the closing test rejects B
        assert f_new == f_old and gt_new == gt_old and ops_new[1] == 0

"""The variable-line product of the lane-pair Miller loop, f <- f (c0 + c3 w + c4 w^3), as six fused three-product sums
(csrc/zkv_tower_mem.h f12m_mul_by_034_body, csrc/zkv_field.h f2_dot3_first / f2_dot3_last) against the thirteen-product Karatsuba form
it replaced, in the host emulation of a lane pair (tests/host_sim/host_sim_var_line.cpp).  CPU only.

The host build forms every update of a 64-bit column again in 128 bits and counts the updates that differ (ZKV_SHADOW_COLS): the
range argument written next to f2_dot3_first -- two products, one exact carry pass, the third product, one reduction -- is checked
where it is tightest, and the bodies that were there before (Karatsuba, the fixed-line product, the squaring) pass the same check."""
import ctypes as C
import os
import random
import subprocess

import pytest

import spec_model as m

HERE = os.path.dirname(os.path.abspath(__file__))
H = bytes.fromhex
P = m.P
BODIES = ('fused', 'karatsuba', 'fixed_line', 'sqr')


@pytest.fixture(scope='module')
def hv():
    src = os.path.join(HERE, 'host_sim', 'host_sim_var_line.cpp')
    lib = os.path.join(HERE, 'host_sim', 'libhost_sim_var_line.so')
    csrc = os.path.join(HERE, '..', 'stylus_zkvm_verifiers_amd', 'csrc')
    deps = [src] + [os.path.join(csrc, f) for f in os.listdir(csrc) if f.endswith('.h')]
    if not os.path.exists(lib) or os.path.getmtime(lib) < max(os.path.getmtime(d) for d in deps):
        subprocess.check_call(['g++', '-O2', '-std=c++17', '-fPIC', '-shared', '-pthread', '-Wno-unknown-pragmas', '-o', lib, src])
    L = C.CDLL(lib)
    L.hsv_line_products.argtypes = [C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    L.hsv_miller_shadow.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p]
    L.hsv_miller_shadow.restype = C.c_ulonglong
    return L


def _run(hv, cases, nb=len(BODIES)):
    """cases: lists of 18 integers (f as g0 g1 g2 h0 h1 h2, then c0 c3 c4; real part, imaginary part).  Returns per case and body the
    twelve canonical output integers, the column-check counters and the loose-range flags."""
    n = len(cases)
    buf = b''.join(v.to_bytes(32, 'little') for c in cases for v in c)
    assert len(buf) == n * 144 * 4
    out = C.create_string_buffer(n * len(BODIES) * 96 * 4)
    shadow = (C.c_ulonglong * (2 * len(BODIES)))(); loose = (C.c_int * len(BODIES))()
    assert hv.hsv_line_products(n, nb, buf, out, shadow, loose) == len(BODIES)
    res = []
    for i in range(n):
        per = []
        for b in range(nb):
            o = (i * len(BODIES) + b) * 384
            per.append([int.from_bytes(out.raw[o + 32 * k: o + 32 * k + 32], 'little') for k in range(12)])
        res.append(per)
    return res, [int(x) for x in shadow], [int(x) for x in loose]


def _check(hv, cases, nb=len(BODIES)):
    res, shadow, loose = _run(hv, cases, nb)
    for i, per in enumerate(res):
        assert per[0] == per[1], (i, [hex(v) for v in cases[i]])           # coefficient by coefficient, as field elements
        assert all(v < P for v in per[0])
    for b, name in enumerate(BODIES[:nb]):
        assert shadow[2 * b] > 0 and shadow[2 * b + 1] == 0, (name, shadow)   # no 64-bit column ever left its 128-bit value
        assert loose[b] == 1, name                                             # every output below 2p
    return res


def _edge_cases(rng):
    """Operands at the edges of the loose range [0, 2p), as the integers the slots hold."""
    edge = [0, 1, P - 1, P, 2 * P - 1]
    cases = []
    rnd = lambda: rng.randrange(P)
    for e in edge:
        cases.append([e] * 18)                                                  # every operand at the edge
        cases.append([e] * 12 + [rnd() for _ in range(6)])                      # f at the edge
        for s in range(3):                                                      # one line coefficient at the edge
            c = [rnd() for _ in range(18)]
            c[12 + 2 * s] = c[13 + 2 * s] = e
            cases.append(c)
        for s in range(6):                                                      # one coefficient of f at the edge
            c = [rnd() for _ in range(18)]
            c[2 * s] = c[2 * s + 1] = e
            cases.append(c)
    # both representatives: x, and x + p where that is below 2p (always, for x < p) -- all operands, f only, the line only, alternating
    for _ in range(6):
        base = [rnd() for _ in range(18)]
        cases.append(base)
        cases.append([v + P for v in base])
        cases.append([v + P for v in base[:12]] + base[12:])
        cases.append(base[:12] + [v + P for v in base[12:]])
        cases.append([v + P * (k & 1) for k, v in enumerate(base)])
        cases.append([v + P * ((k >> 1) & 1) for k, v in enumerate(base)])
    # f = 1 (Montgomery one in g0's real part), in both representatives
    one = pow(2, 261, P)
    for o in (one, one + P):
        for z in (0, P):
            cases.append([o, z] + [z] * 10 + [rnd() for _ in range(6)])
    return cases


def _maximal_cases():
    """Every limb 2^29 - 1 where the value stays below 2p, and the multipliers' imaginary parts 0 so that 8p - b1 is largest."""
    top = (2 * P - 1) >> 232
    vmax = (top << 232) - 1                        # limbs 0 .. 7 all ones, the largest top limb that keeps the value below 2p
    assert vmax < 2 * P and all(((vmax >> (29 * k)) & 0x1fffffff) == 0x1fffffff for k in range(8))
    return [[vmax] * 12 + [vmax, 0] * 3,           # b1 = 0 in c0, c3 and c4
            [vmax] * 18,
            [vmax] * 12 + [0, vmax] * 3,
            [2 * P - 1] * 12 + [2 * P - 1, 0] * 3]


def test_fused_product_equals_karatsuba_on_edges(hv):
    rng = random.Random(0x034E)
    cases = _edge_cases(rng) + _maximal_cases()
    res = _check(hv, cases)
    # spot check against plain arithmetic: the all-zero line gives 0, f = 1 gives the line itself
    assert all(v == 0 for v in res[0][0])
    one = pow(2, 261, P)
    c = [one, 0] + [0] * 10 + [rng.randrange(P) for _ in range(6)]
    r = _check(hv, [c])[0][0]
    rinv = pow(2, -261, P)
    want = [0] * 12
    want[0], want[1] = c[12] * rinv % P, c[13] * rinv % P          # g0 = c0
    want[6], want[7] = c[14] * rinv % P, c[15] * rinv % P          # h0 = c3 (w^1)
    want[8], want[9] = c[16] * rinv % P, c[17] * rinv % P          # h1 = c4 (w^3)
    assert r == want


def test_fused_product_equals_karatsuba_on_random_operands(hv):
    """10,240 random (f, c0, c3, c4), every operand anywhere in the loose range."""
    rng = random.Random(0x0342)
    for _ in range(10):
        _check(hv, [[rng.randrange(2 * P) for _ in range(18)] for _ in range(1024)], nb=2)


def test_column_check_sees_every_update(hv):
    """The 128-bit check is live: per lane a fused product checks 6 x (6 x 81 products + 17 carries of the pass + a reduction of 81
    products and 17 carries) column updates."""
    res, shadow, loose = _run(hv, [[1] * 18])
    per_lane = 6 * (6 * 81 + 17 + 81 + 17)
    assert shadow[0] == 2 * per_lane and shadow[1] == 0


from test_kernel_math_host import hs  # noqa: E402,F401  (the one-value-per-lane host build: its fixture, not a copy of its recipe)

FL_A_INF, FL_B_INF, FL_C_INF, FL_L_INF = 2, 4, 8, 16
STEPS = 88                                          # line steps of the optimal-ate loop (ZKV_MILLER_STEPS)


def test_miller_loop_columns_and_issued_work_on_real_proofs(hv, hs, real_proofs):
    """The flat loop the kernels run, on the two real proofs under every combination of the flags that switch its line products on and
    off (A, B, C and the vk_x point at infinity): no column update differs from its 128-bit form and no fused sum gets an operand outside
    its contract.  And the two multiply-add counters: the loop is CHARGED the Karatsuba form of the variable-line product (the work
    figure of tests/golden/stage_mul_counts.json) and ISSUES 243 more per lane and step plus 17 in each of the six carry passes --
    exactly that where the variable pair contributes, nothing where it does not."""
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
        for extra in range(16):
            flags = fl.value | (FL_A_INF if extra & 1 else 0) | (FL_B_INF if extra & 2 else 0) | (FL_C_INF if extra & 4 else 0) | (FL_L_INF if extra & 8 else 0)
            ops = (C.c_ulonglong * 3)()
            assert hv.hsv_miller_shadow(t, flags, norm, b, ops) == 0, extra
            var_pair = not (flags & (FL_A_INF | FL_B_INF))
            assert ops[2] - ops[1] == (2 * STEPS * (243 + 6 * 17) if var_pair else 0), (extra, ops[1], ops[2])
            assert ops[0] > 0 or (flags & FL_B_INF and flags & FL_C_INF and flags & FL_L_INF)

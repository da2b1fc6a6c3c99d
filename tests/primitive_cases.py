"""Case generators, references and runners for the known-answer harness of the arithmetic primitives (zkv_diag_primitive,
stylus_zkvm_verifiers_amd/csrc/zkv_selftest.h).  Shared by the GPU test (tests/test_device_primitives_gpu.py) and its CPU counterpart
(tests/test_device_primitives_host.py), which runs the same cases through host builds of the same header (tests/host_sim).

Operands are Montgomery-domain integers (R = 2^261 for Fp and Fr); expectations come from Python integers and, for Fp12, G1 and G2, from
oracle/spec_model.py.  Every generator puts its edge operands first (lane 0, both lanes of the first pair, the first group), again at the
end of the first wavefront and the start of the second (lanes 63 / 64, across a pair / group boundary), and fills the rest at random."""
import ctypes as C
import os
import random
import subprocess

import numpy as np

import spec_model as m

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, '..', 'stylus_zkvm_verifiers_amd', 'csrc')
P, RR = m.P, m.R
RM = 1 << 261
RI = pow(RM, -1, P)              # Fp: Montgomery value x represents x RI
RIR = pow(RM, -1, RR)            # Fr
M29 = (1 << 29) - 1
WP = [0, 2, 4, 1, 3, 5]          # slot index -> power of w

# (mapping, op) -> (in words, out words): include/zkv_diag_primitive.h
IO = {(0, 0): (24, 128), (0, 1): (24, 16), (0, 2): (16, 16), (0, 3): (8, 8), (0, 4): (32, 64), (0, 5): (24, 40), (0, 6): (8, 12), (0, 7): (64, 72),
      (1, 0): (32, 80), (1, 1): (162, 18), (1, 2): (36, 18), (1, 3): (240, 11 * 96), (1, 4): (96, 192),
      (2, 0): (240, 768), (2, 1): (96, 96), (3, 0): (240, 768), (3, 1): (96, 96),
      (0, 8): (32, 2), (1, 5): (32, 4), (1, 6): (192, 6), (1, 7): (80, 2), (2, 2): (96, 16), (3, 2): (96, 64),      # the accept predicates
      (0, 9): (128, 248), (0, 10): (112, 384), (1, 8): (192, 816), (1, 9): (32, 4),                                # G2 and the line steps
      (2, 3): (288, 2 * (48 + 48 * 8) + 5 * 96 + 48), (3, 3): (288, 2 * (48 + 48 * 32) + 5 * 96 + 48)}
PER_WAVE = {0: 64, 1: 32, 2: 4, 3: 1}


def words(v, n=8): return [(v >> (32 * i)) & 0xffffffff for i in range(n)]
def unwords(w): return sum(int(x) << (32 * i) for i, x in enumerate(w))
def limbs9(v): return [(v >> (29 * i)) & M29 for i in range(8)] + [v >> 232]
def val9(l): return sum(int(x) << (29 * i) for i, x in enumerate(l))
def sval9(l): return sum((int(x) - (1 << 32) if int(x) >= (1 << 31) else int(x)) << (29 * i) for i, x in enumerate(l))


def place_edges(edges, randoms, n, per_wave=64):
    """n cases: the edges at the start, again just before and after the first wavefront boundary (when n reaches it), randoms elsewhere."""
    out = list(edges[:n])
    while len(out) < n:
        out.append(next(randoms))
    b = per_wave
    if n >= b + len(edges) and len(edges) <= b:
        out[b - len(edges) // 2:b - len(edges) // 2 + len(edges)] = edges
    return out[:n]


def gen_stream(f):
    while True:
        yield f()


# ---------------------------------------------------------------- mapping 0: one value per lane
def edge_fp2(): return [0, 1, 2, P - 1, P, P + 1, 2 * P - 2, 2 * P - 1, (P + 1) // 2, (1 << 253) - 1]
def edge_fp4(): return edge_fp2() + [2 * P, 2 * P + 1, 3 * P, 3 * P + 1, 4 * P - 1]


def lane_cases(op, n, rng):
    e2, e4 = edge_fp2(), edge_fp4()
    if op == 0:
        e2 = e2 + [1 << (32 * i) for i in range(8)] + [P ^ (1 << (32 * i)) for i in range(8)]      # one limb away from 0 and from p (fp_is_zero, fp_eq)
        edges = [[a, b, c] for a in e2 for b in (0, P, 2 * P - 1, a, (a + P) % (2 * P)) for c in (0, 2 * P - 1)]
        rnd = gen_stream(lambda: [rng.choice(e2) if rng.random() < 0.2 else rng.randrange(2 * P) for _ in range(3)])
        cs = place_edges(edges, rnd, n)
        return [words(a) + words(b) + words(c) for a, b, c in cs]
    if op == 1:
        any256 = [0, (1 << 256) - 1, 1 << 255, (1 << 232) - 1, int('5' * 64, 16), int('a' * 64, 16)]
        edges = [[a, b, rng.choice(e4 + any256)] for a in e4 for b in (0, 1, P - 1, 4 * P - 1, 2 * P - 1)] + [[4 * P - 1, 4 * P - 1, c] for c in any256]
        rnd = gen_stream(lambda: [rng.randrange(4 * P), rng.randrange(4 * P), rng.randrange(1 << 256) if rng.random() < 0.5 else rng.randrange(4 * P)])
        return [words(a) + words(b) + words(c) for a, b, c in place_edges(edges, rnd, n)]
    if op == 2:
        edges = [[x, y] for x in (0, 1, P - 1, P - 2, (1 << 253) - 1) for y in e2]
        rnd = gen_stream(lambda: [rng.randrange(P), rng.randrange(2 * P)])
        return [words(x) + words(y) for x, y in place_edges(edges, rnd, n)]
    if op == 3:
        edges = [[a] for a in e4 + [(1 << 256) - 1, 1 << 255, (1 << 256) - P, 5 * P, 5 * P + 1, (1 << 30) - 1, 1 << 30, (1 << 60) + 1]]
        rnd = gen_stream(lambda: [rng.randrange(1 << 256) if rng.random() < 0.3 else rng.randrange(2 * P)])
        return [words(a) for (a,) in place_edges(edges, rnd, n)]
    if op == 4:
        edges = [[a0, a1, b0, b1] for a0 in e2 for a1 in (0, P, 2 * P - 1) for b0, b1 in ((0, 4 * P - 1), (4 * P - 1, 4 * P - 1), (P, 2 * P))]
        edges += [[a0, a1, 4 * P - 1, 3 * P] for a0 in (3 * P, 4 * P - 1) for a1 in (0, 4 * P - 1)]
        rnd = gen_stream(lambda: [rng.randrange(2 * P), rng.randrange(2 * P), rng.randrange(4 * P), rng.randrange(4 * P)] if rng.random() < 0.7
                         else [rng.randrange(4 * P) for _ in range(4)])
        return [words(a0) + words(a1) + words(b0) + words(b1) for a0, a1, b0, b1 in place_edges(edges, rnd, n)]
    if op == 5:
        er = [0, 1, RR - 1, RR - 2, (RR + 1) // 2, (1 << 253) - 1]
        ex = [0, 1, RR - 1, RR, RR + 1, 2 * RR, 5 * RR - 1, (1 << 256) - 1, (1 << 256) - RR, 1 << 255]
        edges = [[a, b, x] for a in er for b in er[:4] for x in ex[:3]] + [[rng.randrange(RR), rng.randrange(RR), x] for x in ex]
        rnd = gen_stream(lambda: [rng.randrange(RR), rng.randrange(RR), rng.randrange(1 << 256)])
        return [words(a) + words(b) + words(x) for a, b, x in place_edges(edges, rnd, n)]
    if op == 6:
        u = m.U
        nn, a1, b2 = 2 * u + 1, 6 * u * u + 2 * u, 6 * u * u + 4 * u + 1
        base = [0, 1, RR - 1, RR, RR + 1, (1 << 256) - 1, (1 << 255), (1 << 128) - 1, 1 << 128]
        for v in (nn, a1, b2, a1 + nn, b2 - nn):
            for j in (1, 2, 3, 1 << 64, (1 << 126) // v if v < (1 << 126) else 1):
                for d in (-1, 0, 1):
                    if 0 <= j * v + d < (1 << 256):
                        base.append(j * v + d)
        edges = [[k] for k in base]
        rnd = gen_stream(lambda: [rng.randrange(1 << 256) if rng.random() < 0.5 else rng.randrange(RR)])
        return [words(k) for (k,) in place_edges(edges, rnd, n)]
    if op == 7:
        return g1_cases(n, rng)
    raise ValueError(op)


def _mont_rep(v, rng, loose=True):
    x = v * RM % P
    return x + P if loose and rng.random() < 0.3 else x


def _jac(pt, rng):
    """affine point (or None) -> Jacobian words with a random z; infinity has z = 0 (or p)."""
    if pt is None:
        return words(_mont_rep(1, rng)) + words(_mont_rep(1, rng)) + words(rng.choice([0, P]))
    z = rng.choice([1, rng.randrange(1, P)])
    x, y = pt[0] * z * z % P, pt[1] * z * z * z % P
    return words(_mont_rep(x, rng)) + words(_mont_rep(y, rng)) + words(_mont_rep(z, rng))


_G1_POOL = None


def _g1_pool():
    global _G1_POOL
    if _G1_POOL is None:
        r = random.Random(0x61)
        g = (1, 2)
        _G1_POOL = [g, m.g1_neg(g), m.g1_mul(g, 2), m.g1_mul(g, RR - 1)] + [m.g1_mul(g, r.randrange(1, RR)) for _ in range(12)]
    return _G1_POOL


def g1_cases(n, rng):
    """(P, Q affine, T): P + P, P + (-P), inf + P, P + inf and generic sums, mixed so that lanes of one wavefront take different branches."""
    pool = _g1_pool()

    def case(kind):
        p = rng.choice(pool)
        q = rng.choice(pool)
        t = rng.choice(pool)
        if kind == 1: q = t = p                                     # P + P
        elif kind == 2: q = t = m.g1_neg(p)                         # P + (-P)
        elif kind == 3: p = None                                    # inf + P
        elif kind == 4: t = None                                    # P + inf (g1j_add)
        elif kind == 5: p = None; t = None
        return (p, q, t)
    edges = [case(k) for k in (1, 2, 3, 4, 5, 0, 1, 2, 0, 3)]
    cs = place_edges(edges, gen_stream(lambda: case(rng.choice([0, 0, 1, 2, 3, 4]))), n)
    out = []
    for p, q, t in cs:
        out.append(_jac(p, rng) + words(_mont_rep(q[0], rng)) + words(_mont_rep(q[1], rng)) + _jac(t, rng))
    return out


def _fp_of(w, k): return unwords(w[8 * k:8 * k + 8])


def _jac_to_aff(w):
    x, y, z = (_fp_of(w, k) * RI % P for k in range(3))
    if z == 0:
        return None
    zi = pow(z, -1, P)
    return (x * zi * zi % P, y * zi * zi * zi % P)


def check_lane(op, ins, outs):
    bad = []
    for idx, (wi, wo) in enumerate(zip(ins, outs)):
        try:
            _check_lane_one(op, wi, wo)
        except AssertionError as e:
            bad.append((idx, str(e)))
            if len(bad) > 5:
                break
    assert not bad, 'op %d: %d failing cases, first %s' % (op, len(bad), bad[:3])


def _check_lane_one(op, wi, wo):
    f = lambda k: _fp_of(wi, k)
    o = lambda k: _fp_of(wo, k)
    if op == 0:
        a, b, c = f(0), f(1), f(2)
        want = [a + b, a - b, -a, 2 * a, a * pow(2, -1, P), a + b, c + a, a - b, c - a, a + b, b + c, c + a, a - b, b - c, c - a]
        names = ['add', 'sub', 'neg', 'dbl', 'half', 'add_x2.0', 'add_x2.1', 'sub_x2.0', 'sub_x2.1', 'add_n.0', 'add_n.1', 'add_n.2', 'sub_n.0', 'sub_n.1', 'sub_n.2']
        for k, (w, nm) in enumerate(zip(want, names)):
            assert o(k) < 2 * P and (o(k) - w) % P == 0, (nm, hex(a), hex(b), hex(c), hex(o(k)))
        assert wo[120] == (1 if a % P == 0 else 0), ('is_zero', hex(a))
        assert wo[121] == (1 if (a - b) % P == 0 else 0), ('eq', hex(a), hex(b))
        assert list(wo[122:128]) == [0] * 6
    elif op == 1:
        a, b, c = f(0), f(1), f(2)
        assert o(0) < 2 * P and (o(0) - a * b * RI) % P == 0, ('mul', hex(a), hex(b), hex(o(0)))
        assert o(1) < 2 * P and (o(1) - c * c * RI) % P == 0, ('sqr', hex(c), hex(o(1)))
    elif op == 2:
        x, y = f(0), f(1)
        assert o(0) < 2 * P and (o(0) - x * RM) % P == 0, ('from_raw', hex(x), hex(o(0)))
        assert o(1) == y * RI % P, ('to_raw', hex(y), hex(o(1)))
    elif op == 3:
        a = f(0)
        v = a * RI % P
        want = pow(v, -1, P) * RM % P if v else 0
        assert o(0) < 2 * P and (o(0) - want) % P == 0, ('inv', hex(a), hex(o(0)))
    elif op == 4:
        a0, a1, b0, b1 = f(0), f(1), f(2), f(3)
        r = [o(k) for k in range(8)]
        assert all(x < 2 * P for x in r[:2]), ('f2_mul bound', [hex(x) for x in r[:2]])
        assert (r[0] - (a0 * b0 - a1 * b1) * RI) % P == 0 and (r[1] - (a0 * b1 + a1 * b0) * RI) % P == 0, ('f2_mul', hex(a0), hex(a1), hex(b0), hex(b1))
        if max(a0, a1) < 2 * P:
            assert all(x < 2 * P for x in r[2:8]), ('f2 bound', [hex(x) for x in r[2:8]])
            assert (r[2] - (a0 * a0 - a1 * a1) * RI) % P == 0 and (r[3] - 2 * a0 * a1 * RI) % P == 0, ('f2_sqr', hex(a0), hex(a1))
            assert (r[4] - (9 * a0 - a1)) % P == 0 and (r[5] - (9 * a1 + a0)) % P == 0, ('f2_mul_xi', hex(a0), hex(a1))
            v0, v1 = a0 * RI % P, a1 * RI % P
            nrm = (v0 * v0 + v1 * v1) % P
            w0, w1 = (v0 * pow(nrm, -1, P) % P, -v1 * pow(nrm, -1, P) % P) if nrm else (0, 0)
            assert (r[6] - w0 * RM) % P == 0 and (r[7] - w1 * RM) % P == 0, ('f2_inv', hex(a0), hex(a1))
    elif op == 5:
        a, b, x = f(0), f(1), f(2)
        r = [o(k) for k in range(5)]
        va = a * RIR % RR
        want = [a * b * RIR % RR, (a + b) % RR, (a - b) % RR, (pow(va, -1, RR) * RM % RR) if va else 0, (x % RR) * RM % RR]
        for k, nm in enumerate(['fr_mul', 'fr_add', 'fr_sub', 'fr_inv', 'fr_from_raw_reduce']):
            assert r[k] == want[k], (nm, hex(a), hex(b), hex(x), hex(r[k]), hex(want[k]))          # canonical, not merely congruent
    elif op == 6:
        k = f(0)
        m1, n1, m2, n2 = unwords(wo[0:5]), wo[5], unwords(wo[6:11]), wo[11]
        assert n1 in (0, 1) and n2 in (0, 1) and m1 < (1 << 128) and m2 < (1 << 128), ('glv bound', hex(k), hex(m1), hex(m2))
        k1, k2 = (-m1 if n1 else m1), (-m2 if n2 else m2)
        assert (k1 + k2 * GLV_LAMBDA - k) % RR == 0, ('glv identity', hex(k))
    elif op == 7:
        p = _jac_to_aff(wi[0:24]); q = (_fp_of(wi, 3) * RI % P, _fp_of(wi, 4) * RI % P); t = _jac_to_aff(wi[40:64])
        assert all(x < 2 * P for x in [o(k) for k in range(9)]), 'g1 bound'
        assert _jac_to_aff(wo[0:24]) == m.g1_add(p, p), ('g1j_dbl', p)
        assert _jac_to_aff(wo[24:48]) == m.g1_add(p, q), ('g1j_add_affine', p, q)
        assert _jac_to_aff(wo[48:72]) == m.g1_add(p, t), ('g1j_add', p, t)


GLV_LAMBDA = (6 * m.U * m.U + 2 * m.U) * pow(2 * m.U + 1, -1, RR) % RR       # a1 - n lambda = 0 (mod r): the basis of zkv_scalar.h glv_split


# ---------------------------------------------------------------- mapping 1: lane pairs (Fp2, L9)
def pair_f2_cases(n, rng):
    e4 = [0, 1, P - 1, P, P + 1, 2 * P - 1, 2 * P, 2 * P + 1, 3 * P, 4 * P - 1]
    e2 = [v for v in e4 if v < 2 * P]
    edges = [[a0, a1, b0, b1] for a0 in e4 for a1 in (0, P, 4 * P - 1) for b0, b1 in ((0, 4 * P - 1), (4 * P - 1, 4 * P - 1), (P, 2 * P))]
    edges += [[a0, a1, b0, b1] for a0 in e2 for a1 in e2[::2] for b0, b1 in ((2 * P - 1, 0), (0, 2 * P - 1))]
    rnd = gen_stream(lambda: [rng.randrange(4 * P) for _ in range(4)] if rng.random() < 0.5 else [rng.randrange(2 * P) for _ in range(4)])
    cs = place_edges(edges, rnd, n, 32)
    return [words(a0) + words(a1) + words(b0) + words(b1) for a0, a1, b0, b1 in cs]


def check_pair_f2(ins, outs):
    for idx, (wi, wo) in enumerate(zip(ins, outs)):
        a0, a1, b0, b1 = (_fp_of(wi, k) for k in range(4))
        r = [_fp_of(wo, k) for k in range(10)]
        ctx = (idx, hex(a0), hex(a1), hex(b0), hex(b1))
        assert r[0] < 2 * P and r[1] < 2 * P, ('mul bound',) + ctx
        assert (r[0] - (a0 * b0 - a1 * b1) * RI) % P == 0 and (r[1] - (a0 * b1 + a1 * b0) * RI) % P == 0, ('mul',) + ctx
        if max(a0, a1, b0, b1) < 2 * P:
            assert all(x < 2 * P for x in r), ('bound',) + ctx
            assert (r[2] - (a0 * a0 - a1 * a1) * RI) % P == 0 and (r[3] - 2 * a0 * a1 * RI) % P == 0, ('sqr',) + ctx
            assert (r[4] - (9 * a0 - a1)) % P == 0 and (r[5] - (9 * a1 + a0)) % P == 0, ('xi',) + ctx
            assert (r[6] - (a0 + b0)) % P == 0 and (r[7] - (a1 + b1)) % P == 0, ('add',) + ctx
            assert (r[8] - (a0 - b0)) % P == 0 and (r[9] - (a1 - b1)) % P == 0, ('sub',) + ctx


# (coefficients of the even lane, of the odd lane, c, which terms are lazy three-term sums): the call sites of zkv_tower_mem.h /
# zkv_tower_wide.h, with the per-lane signs (k1 = -1 / +1, k3 = 3 / -3) they use
LINCOMB_SITES = [((1, 9, -1), (1, 9, 1), 4, ()), ((3, -30, 3, -2), (3, -30, -3, -2), 72, ()), ((6, 2), (6, 2), 1, ()),
                 ((54, -6, 2), (54, 6, 2), 14, ()), ((1, 9, -1), (1, 9, 1), 48, (1, 2)), ((1, 9, -1), (1, 9, 1), 8, (0,)), ((1,), (1,), 8, (0,)),
                 ((1, 9, -1, -1), (1, 9, 1, -1), 52, (1, 2)), ((1, 9, -1, -1), (1, 9, 1, -1), 12, (0,)), ((1, -1), (1, -1), 12, (0,)),
                 ((0, 6, 0, 2), (0, 6, 0, 2), 72, ()), ((0, 54, 6, 2), (0, 54, -6, 2), 72, ()), ((3, -30, 3, -2), (0, 6, 0, 2), 72, ()),
                 ((1, 1), (1, 1), 1, ()), ((-1,), (-1,), 3, ()), ((1, 9, 1, -1), (1, 9, -1, -1), 12, (0,)),
                 ((2, 2, 18, 18, -2, 2, 0, 0), (2, 2, 18, 18, 2, -2, 0, 0), 20, ()), ((1, 9, -1, 9, -1), (1, 9, 1, 9, 1), 8, ())]


def lincomb_cases(n, rng):
    edge = [0, 1, P - 1, P, P + 1, 2 * P - 1, (1 << 232) - 1, 2 * P - 2]

    def pick(): return rng.choice(edge) if rng.random() < 0.5 else rng.randrange(2 * P)

    def lazy3():
        sign = -1 if rng.random() < 0.7 else 1
        x, y, z = (limbs9(pick()) for _ in range(3))
        return [(a + sign * (b + c)) & 0xffffffff for a, b, c in zip(x, y, z)]

    def one(site, rep):
        ke, ko, c, lazy = site
        w = [len(ke), c] + [k & 0xffffffff for k in ke] + [0] * (8 - len(ke)) + [k & 0xffffffff for k in ko] + [0] * (8 - len(ko))
        for ks in (ke, ko):
            terms = []
            for j, k in enumerate(ks):
                if j in lazy:
                    terms += lazy3()
                else:
                    terms += limbs9(pick() if rep else (2 * P - 1 if k < 0 else 0))        # rep 0: the most negative combination
            w += terms + [0] * (72 - len(terms))
        return w
    edges = [one(s, 0) for s in LINCOMB_SITES]
    k = [0]

    def rnd():
        k[0] += 1
        return one(LINCOMB_SITES[k[0] % len(LINCOMB_SITES)], k[0])
    return place_edges(edges, gen_stream(rnd), n, 32)


def check_lincomb(ins, outs):
    for idx, (wi, wo) in enumerate(zip(ins, outs)):
        nt, c = wi[0], wi[1]
        for par in (0, 1):
            ks = [int(np.int32(np.uint32(x))) for x in wi[2 + 8 * par:2 + 8 * par + nt]]
            total = sum(k * sval9(wi[18 + 72 * par + 9 * j:18 + 72 * par + 9 * j + 9]) for j, k in enumerate(ks))
            got = [int(x) for x in wo[9 * par:9 * par + 9]]
            assert all(x <= M29 for x in got[:8]), (idx, par, ks, c, got)
            v = val9(got)
            assert v % P == total % P and v < P + (P >> 6), (idx, par, ks, c, hex(v))


def l9mul_cases(n, rng):
    big = [limbs9(2 * P - 1), [M29] * 8 + [(2 * P - 1) >> 232], limbs9(0), limbs9(P)]

    def mcand():
        x, y = (rng.choice(big) if rng.random() < 0.4 else limbs9(rng.randrange(2 * P)) for _ in range(2))
        return [a + b for a, b in zip(x, y)]

    def mplier(v=None): return limbs9(v if v is not None else rng.choice([0, P, 2 * P - 1, 4 * P - 1, 7 * P + (P >> 1), rng.randrange(4 * P), rng.randrange(8 * P - P // 10)]))
    top = [M29 * 2 - 1] * 8 + [((2 * P - 1) >> 232) * 2]
    edges = [top + top + mplier(7 * P + (P >> 1)) + mplier(7 * P + (P >> 1)), top + top + mplier(0) + mplier(7 * P + (P >> 1)),
             limbs9(0) * 2 + mplier(0) * 2, top + limbs9(0) + mplier(4 * P - 1) + mplier(0)]
    return place_edges(edges, gen_stream(lambda: mcand() + mcand() + mplier() + mplier()), n, 32)


def check_l9mul(ins, outs):
    for idx, (wi, wo) in enumerate(zip(ins, outs)):
        A0, A1, B0, B1 = (val9(wi[9 * k:9 * k + 9]) for k in range(4))
        r0, r1 = val9(wo[:9]), val9(wo[9:])
        assert all(int(x) <= M29 for x in list(wo[:8]) + list(wo[9:17])), idx
        assert r0 % P == (A0 * B0 - A1 * B1) * RI % P and r1 % P == (A0 * B1 + A1 * B0) * RI % P, idx
        assert r0 < 2 * P and r1 < 2 * P, idx


# ---------------------------------------------------------------- Fp12 (mappings 1-3)
def slots_to_f12(slots):
    """six Fp2 value-domain pairs in slot order -> spec_model's w-basis (12 Fp coefficients)"""
    out = [0] * 12
    for i, c in enumerate(slots):
        out = [(x + y) % P for x, y in zip(out, m.f2_to_f12(c, WP[i]))]
    return out


def f12_to_slots(t):
    slots = [None] * 6
    for i in range(6):
        k = WP[i]
        a1 = t[k + 6] % P
        slots[i] = ((t[k] + 9 * a1) % P, a1)
    return slots


def f12_words(slots_mont):
    w = []
    for c0, c1 in slots_mont:
        w += words(c0) + words(c1)
    return w


def f12_from_words(w):
    """96 words -> (raw Montgomery integers per component, value-domain w-basis element)"""
    raw = [(unwords(w[16 * i:16 * i + 8]), unwords(w[16 * i + 8:16 * i + 16])) for i in range(6)]
    return raw, slots_to_f12([(a * RI % P, b * RI % P) for a, b in raw])


def _mont_words_of(t, rng, loose):
    out = []
    for c0, c1 in f12_to_slots(t):
        out.append((_mont_rep(c0, rng, loose), _mont_rep(c1, rng, loose)))
    return out


def f12_conj(t): return [x if k % 2 == 0 else -x % P for k, x in enumerate(t)]


_FROB = {}


def f12_frob(t, k):
    """pi^k(a) = a^(p^k): linear over Fp, so sum_j t_j (w^(p^k))^j, with the powers of w computed once by f12pow"""
    if k not in _FROB:
        wk = m.f12pow([0, 1] + [0] * 10, P ** k)
        pw = [m.F12_ONE]
        for _ in range(11):
            pw.append(m.f12mul(pw[-1], wk))
        _FROB[k] = pw
    out = [0] * 12
    for j, x in enumerate(t):
        if x:
            out = [(o + x * y) % P for o, y in zip(out, _FROB[k][j])]
    return out


def line_f12(c0, c3, c4): return slots_to_f12([c0, (0, 0), (0, 0), c3, c4, (0, 0)])


_CYCLO = None


def cyclotomic_pool():
    """a handful of seeded elements of the cyclotomic subgroup, f^((p^6 - 1)(p^2 + 1))"""
    global _CYCLO
    if _CYCLO is None:
        r = random.Random(0xC1C)
        _CYCLO = []
        for _ in range(4):
            f = [r.randrange(P) for _ in range(12)]
            _CYCLO.append(m.f12pow(f, (P ** 6 - 1) * (P ** 2 + 1)))
    return _CYCLO


def _f12_special(kind, rng):
    if kind == 0:
        return m.F12_ONE
    if kind == 1:
        return [0] * 12
    if kind == 2:                                  # zero and one coefficients
        return slots_to_f12([rng.choice([(0, 0), (1, 0), (0, 1), (P - 1, 0), (rng.randrange(P), rng.randrange(P))]) for _ in range(6)])
    return [rng.randrange(P) for _ in range(12)]


def f12_cases(n, rng):
    """a b c0 c3 c4: random elements, elements with x + p coefficients, zero and one coefficients"""
    def case(ka, kb):
        a, b = _f12_special(ka, rng), _f12_special(kb, rng)
        loose = rng.random() < 0.5
        lines = [(_mont_rep(rng.randrange(P), rng, loose), _mont_rep(rng.randrange(P), rng, loose)) for _ in range(3)]
        if rng.random() < 0.15:
            lines[0] = (P if loose else 0, 0)
        w = f12_words(_mont_words_of(a, rng, loose)) + f12_words(_mont_words_of(b, rng, rng.random() < 0.5))
        for c in lines:
            w += words(c[0]) + words(c[1])
        return w
    edges = [case(ka, kb) for ka, kb in ((0, 3), (3, 0), (2, 3), (3, 2), (2, 2), (1, 3), (3, 3), (0, 0))]
    return place_edges(edges, gen_stream(lambda: case(3 if rng.random() < 0.7 else 2, 3 if rng.random() < 0.7 else 2)), n, 4)


def cyclo_cases(n, rng):
    pool = cyclotomic_pool()

    def case():
        a = rng.choice(pool)
        if rng.random() < 0.3:
            a = m.f12mul(a, rng.choice(pool))
        return f12_words(_mont_words_of(a, rng, rng.random() < 0.6))
    edges = [f12_words(_mont_words_of(m.F12_ONE, rng, False)), f12_words(_mont_words_of(m.F12_ONE, rng, True))] + \
            [f12_words(_mont_words_of(c, rng, lo)) for c in pool for lo in (False, True)]
    return place_edges(edges, gen_stream(case), n, 4)


def _f12_out(wo, k):
    raw, v = f12_from_words(wo[96 * k:96 * k + 96])
    assert all(x < 2 * P for c in raw for x in c), ('bound', k, [hex(x) for c in raw for x in c if x >= 2 * P])
    return v


def f12_inputs(wi):
    a = f12_from_words(wi[0:96])[1]
    b = f12_from_words(wi[96:192])[1]
    cs = [(unwords(wi[192 + 16 * j:200 + 16 * j]) * RI % P, unwords(wi[200 + 16 * j:208 + 16 * j]) * RI % P) for j in range(3)]
    return a, b, cs


def check_pair_f12(ins, outs):
    names = ['f12m_mul', 'f12m_mul_conj', 'f12m_sqr', 'f12m_inv', 'f12m_frob1', 'f12m_frob2', 'f12m_frob3', 'f12m_mul_by_034', 'f12m_mul_by_134',
             'f12l9_mul', 'f12l9_mul(conj_b)']
    for idx, (wi, wo) in enumerate(zip(ins, outs)):
        a, b, (c0, c3, c4) = f12_inputs(wi)
        want = [m.f12mul(a, b), m.f12mul(a, f12_conj(b)), m.f12mul(a, a), None, f12_frob(a, 1), f12_frob(a, 2), f12_frob(a, 3),
                m.f12mul(a, line_f12(c0, c3, c4)), m.f12mul(a, line_f12((1, 0), c3, c4)), m.f12mul(a, b), m.f12mul(a, f12_conj(b))]
        for k, nm in enumerate(names):
            got = _f12_out(wo, k)
            if k == 3:
                ok = (m.f12mul(got, a) == m.F12_ONE) if any(a) else not any(got)
                assert ok, (idx, nm)
            else:
                assert got == want[k], (idx, nm)


def check_cyclo(ins, outs, nout):
    for idx, (wi, wo) in enumerate(zip(ins, outs)):
        a = f12_from_words(wi[0:96])[1]
        want = m.f12mul(a, a)
        for k in range(nout):
            assert _f12_out(wo, k) == want, (idx, k)


def check_wide_f12(ins, outs):
    names = ['w12_mul', 'w12_mul(conj_b)', 'w12_sqr', 'w12_mul_sparse', 'w12_mul_sparse(one)', 'w12_frob1', 'w12_frob2', 'w12_frob3']
    for idx, (wi, wo) in enumerate(zip(ins, outs)):
        a, b, (c0, c3, c4) = f12_inputs(wi)
        want = [m.f12mul(a, b), m.f12mul(a, f12_conj(b)), m.f12mul(a, a), m.f12mul(a, line_f12(c0, c3, c4)), m.f12mul(a, line_f12((1, 0), c3, c4)),
                f12_frob(a, 1), f12_frob(a, 2), f12_frob(a, 3)]
        for k, nm in enumerate(names):
            assert _f12_out(wo, k) == want[k], (idx, nm)


# ---------------------------------------------------------------- the accept predicates (0 / 1 words, one per lane)
# f2_is_zero / f2_eq (mapping 0 op 8, mapping 1 op 5), f12m_is_one and f12m_eq_conj (mapping 1 op 6), miller_point_closes (mapping 1 op 7),
# f12m_is_one on the wide accumulator (mappings 2 and 3, op 2).  A verdict is a conjunction over Fp components, so the reference lists
# the components that MISS: none means true, exactly one is a "one component off" case, and its position is what the coverage
# conditions of predicate_profile count.  Inputs are raw Montgomery integers below 2p; a true input is tried in every mix of x and x + p.
PREDICATE_OPS = {(0, 8), (1, 5), (1, 6), (1, 7), (2, 2), (3, 2)}
ONE_M = RM % P                                          # 1 in Montgomery form
ODD_AT = {0: (0, 63), 1: (0, 15, 31), 2: (0, 3), 3: (0,)}       # where the odd case of a run sits in its wavefront
G2C = m.f2pow(m.XI, (P ** 3 - 1) // 3)                  # psi^3 on the twist: (x, y) -> (conj(x) G2C, conj(y) G3C)
G3C = m.f2pow(m.XI, (P ** 3 - 1) // 2)


def truth_plan(n, per_wave, odd_at):
    """(holds a true input?, zone) per case.  The first half of the wavefronts alternates true and false case by case (zones 'a', 'b': the
    phase flips from one wavefront to the next, so false cases meet even and odd places); then runs of per_wave - 1 true cases with
    one false (zone 's'), and the reverse, the odd one at odd_at; a last partial wavefront alternates.  One case per wavefront
    (per_wave = 1) has no neighbours: T F F T, so that both kinds still meet even and odd indices."""
    if per_wave == 1:
        return [(k % 4 in (0, 3), 'ab'[(k // 4) % 2]) for k in range(n)]
    waves = n // per_wave
    runs = waves // 4
    alt = waves - 2 * runs
    plan = []
    for w in range(waves):
        for k in range(per_wave):
            if w < alt:
                plan.append(((k + w) % 2 == 0, 'a' if w < (alt + 1) // 2 else 'b'))
            else:
                r = w - alt
                plan.append(((k == odd_at[r % len(odd_at)]) != (r < runs), 's'))
    for k in range(n - len(plan)):
        plan.append((k % 2 == 0, 'ab'[(k // 2) % 2]))
    return plan


def _mont(v): return v * RM % P


def _reps(vals, rng, j):
    """the j-th representative mix of canonical components: all canonical, all shifted by p, then seeded random mixes"""
    if j == 0:
        return list(vals)
    if j == 1:
        return [v + P for v in vals]
    return [v + P if rng.random() < 0.5 else v for v in vals]


def _near(r):
    """the raw value r moved by one, and with the low or the high bit of one limb flipped; only values below 2p (the contract)"""
    out = [r + 1, r - 1] + [r ^ (1 << (32 * i + b)) for i in range(8) for b in (0, 31)]
    return [v for v in dict.fromkeys(out) if 0 <= v < 2 * P]


def _one_off(tgt, positions, rng, unit=None):
    """[(k, v)]: v replaces component k of the canonical vector tgt and is NOT congruent to it: the neighbours (_near) of both
    representatives and, where `unit` is given, the other field's unit.  +-1 and a flip in limb 7, then the unit, come first (so that
    even the shortest case list has a value that differs in the top limb alone); the positions
    are interleaved in rotating order, so that a short prefix already covers all of them."""
    per = []
    for k in positions:
        c = tgt[k]
        first = [c + 1, c ^ (1 << 224), c + P - 1, (c + P) ^ (1 << 224)]
        if k % 2:
            first = first[2:] + first[:2]
        first += ([unit(k)] if unit else []) + [c + P + 1, c - 1]
        rest = [v for r in (c, c + P) for v in _near(r)]
        rng.shuffle(rest)
        vs = [v for v in dict.fromkeys(first + rest) if 0 <= v < 2 * P]
        assert all((v - c) % P for v in vs)
        per.append([(k, v) for v in vs])
    out = []
    for r in range(max(len(x) for x in per)):
        for i in range(len(per)):
            x = per[(i + r) % len(per)]
            if r < len(x):
                out.append(x[r])
    return out


def _assign(parities, entries):
    """one entry (key, payload) per slot, the slot's parity given: among the next unused entries the first whose key (the altered
    position) has not met this parity yet, so that every position meets even and odd places early; the list is cycled"""
    pending, seen, out = [], {}, []
    for par in parities:
        if not pending:
            pending = list(entries)
        pick = next((i for i, (key, _) in enumerate(pending[:24]) if key is not None and par not in seen.get(key, ())), 0)
        key, payload = pending.pop(pick)
        seen.setdefault(key, set()).add(par)
        out.append(payload)
    return out


def _fpw(vals):
    w = []
    for v in vals:
        w += words(v)
    return w


def _cycle(xs):
    while True:
        for x in xs:
            yield x


def _fill(plan, true_of, false_entries, zoned=False):
    """cases by plan: true_of(j, zone) makes the j-th true case; false_entries(zone) -> [(key, payload)] are dealt to the false places
    (zone by zone where the zones take different lists)"""
    out = [None] * len(plan)
    for zone in ('a', 'b', 's') if zoned else ('abs',):
        idx = [i for i, (t, z) in enumerate(plan) if z in zone and not t]
        for i, c in zip(idx, _assign([i % 2 for i in idx], false_entries(zone))):
            out[i] = c
    j = 0
    for i, (t, z) in enumerate(plan):
        if t:
            out[i] = true_of(j, z)
            j += 1
    return out


# ---- f2_is_zero(a), f2_eq(a, b): a0 a1 b0 b1
def f2_pred_cases(n, rng, mapping):
    plan = truth_plan(n, PER_WAVE[mapping], ODD_AT[mapping])
    nz = lambda: rng.randrange(1, P)

    def true_of(j, zone):                       # in a run: both verdicts true; elsewhere also eq alone and is_zero alone
        kind = 0 if zone == 's' else j % 4
        if kind == 1:
            a = [nz(), nz()]
            return _fpw(_reps(a, rng, j // 4) + _reps(a, rng, 2))
        if kind == 2:
            return _fpw(_reps([0, 0], rng, j // 4) + [rng.randrange(1, 2 * P), rng.randrange(2 * P)])
        return _fpw(_reps([0, 0, 0, 0], rng, j // 4 if zone != 's' else j))

    ent = []
    for k, v in _one_off([0, 0], (0, 1), rng, unit=lambda k: ONE_M):           # is_zero misses in component k alone; b is anything
        a = _reps([0, 0], rng, 2)
        a[k] = v
        ent.append((('z', k), _fpw(a + [rng.randrange(1, 2 * P), rng.randrange(1, 2 * P)])))
    eqs = []
    for t in range(2):                                                           # eq misses in component k alone, a != 0
        tgt = [nz(), nz()]
        for j, (k, v) in enumerate(_one_off(tgt, (0, 1), rng)):
            x, y = _reps(tgt, rng, 2), _reps(tgt, rng, 2)
            y[k] = v
            eqs.append((('e', k), _fpw(x + y if (j + t) % 2 else y + x)))
    ent = [e for pair in zip(ent, eqs) for e in pair] + eqs[len(ent):]
    a = [nz(), nz()]
    shapes = [a + [a[0], P - a[1]], a + [a[1], a[0]], a + [P - a[0], P - a[1]], [0, P] + a]
    ent[8:8] = [(None, _fpw(x)) for x in shapes]
    return _fill(plan, true_of, lambda zone: ent)


# ---- Fp12: twelve raw components in slot order (g0 g1 g2 h0 h1 h2, c0 then c1)
def _one_tgt(): return [ONE_M] + [0] * 11
def _f12_raw(t): return [_mont(c) for s in f12_to_slots(t) for c in s]
def _conj_raw(raw): return [x % P for x in raw[:6]] + [-x % P for x in raw[6:]]


def is_one_false_entries(rng):
    """[(position or None, twelve components)]: 1 with one component off; then -1, 1 in another coefficient, 0"""
    tgt = _one_tgt()
    ent = []
    for k, v in _one_off(tgt, range(12), rng, unit=lambda k: 0 if k == 0 else ONE_M):
        x = _reps(tgt, rng, 2)
        x[k] = v
        ent.append((k, x))
    shapes = [[P - ONE_M] + [0] * 11, [2 * P - ONE_M] + [P] * 11, [0] * 12, [P] * 12]
    for k in range(1, 12):
        x = _reps([0] * 12, rng, 2)
        x[k] = ONE_M + (P if k % 2 else 0)
        shapes.append(x)
    ent[24:24] = [(None, x) for x in shapes]
    return ent


def _conj_pool():
    r = random.Random(0xC0)
    cyc = cyclotomic_pool()
    return [_f12_raw(cyc[0]), _f12_raw([r.randrange(P) for _ in range(12)]), _f12_raw(m.f12mul(cyc[1], cyc[2])), _f12_raw([r.randrange(P) for _ in range(12)])]


def eq_conj_false_entries(rng):
    """[(position or None, f, t)]: t = conj(f) with one component off, for cyclotomic and generic f; then t = f, an h coefficient
    (Fp2) of conj(f) with its sign restored, g negated instead of h"""
    pool = _conj_pool()
    lists = [_one_off(_conj_raw(f), range(12), rng) for f in pool]
    ent = []
    for j in range(max(len(x) for x in lists)):
        f, lst = pool[j % len(pool)], lists[j % len(pool)]
        if j < len(lst):
            k, v = lst[j]
            t = _reps(_conj_raw(f), rng, 2)
            t[k] = v
            ent.append((k, _reps(f, rng, 2) + t))
    shapes = []
    for f in pool[:2]:
        shapes.append(_reps(f, rng, 2) + _reps(f, rng, 2))                                   # t = f, h != 0
        for c in (3, 4, 5):
            t = _conj_raw(f)
            t[2 * c:2 * c + 2] = f[2 * c:2 * c + 2]
            shapes.append(_reps(f, rng, 2) + _reps(t, rng, 2))
        shapes.append(_reps(f, rng, 2) + _reps([-x % P for x in f[:6]] + f[6:], rng, 2))
    ent[24:24] = [(None, x) for x in shapes]
    return ent


def pair_f12_pred_cases(n, rng):
    """f t.  Zone 'a': f = 1 in every mix against f one component off (t = conj(f) throughout: eq_conj stays true); zone 'b': generic and
    cyclotomic f with t = conj(f) against t one component off (is_one stays false); runs: all three verdicts true against all three false."""
    plan = truth_plan(n, 32, ODD_AT[1])
    pool = _conj_pool()

    def true_of(j, zone):
        if zone == 'b':
            f = pool[j % len(pool)]
            if j % 5 == 4:                      # h = 0 mod p: t = f is conj(f) as well
                f = f[:6] + [0] * 6
                return _fpw(_reps(f, rng, 2) + _reps(f, rng, 2))
            return _fpw(_reps(f, rng, j // len(pool)) + _reps(_conj_raw(f), rng, 2 if j % 3 else (j // len(pool) + 1) % 2))
        jj = j // 2 if zone == 'a' else j
        mixes = [(0, 0), (1, 1), (0, 1), (1, 0)]
        mf, mt = mixes[jj] if jj < 4 else (2, 2)
        return _fpw(_reps(_one_tgt(), rng, mf) + _reps(_one_tgt(), rng, mt))

    ones, conjs = is_one_false_entries(rng), eq_conj_false_entries(rng)

    def false_entries(zone):
        if zone == 'a':
            return [(k, _fpw(f + _reps(_conj_raw(f), rng, 2))) for k, f in ones]
        if zone == 'b':
            return [(k, _fpw(x)) for k, x in conjs]
        out = []
        for j, (k, f) in enumerate(ones):       # runs: f is not 1 AND t is conj(f) with one component off
            tgt = _conj_raw(f)
            t = _reps(tgt, rng, 2)
            t[j % 12] = _near(tgt[j % 12] + (P if j % 2 else 0))[(j // 12) % 4]
            out.append((k, _fpw(f + t)))
        return out
    return _fill(plan, true_of, false_entries, zoned=True)


def wide_is_one_cases(n, rng, mapping):
    plan = truth_plan(n, PER_WAVE[mapping], ODD_AT[mapping])
    ent = [(k, _fpw(f)) for k, f in is_one_false_entries(rng)]
    return _fill(plan, lambda j, zone: _fpw(_reps(_one_tgt(), rng, j)), lambda zone: ent)


# ---- miller_point_closes: X Y Z bx by (Fp2 each)
def closing_xy(bx, by, z):
    """value domain: the X, Y with (X, Y, z) = -psi^3((bx, by)) in the loop's coordinates (x = X / Z, y = Y / Z)"""
    return m.f2mul(m.f2mul(m.f2conj(bx), G2C), z), m.f2neg(m.f2mul(m.f2mul(m.f2conj(by), G3C), z))


def _closing_raw(bx, by, z):
    x, y = closing_xy(bx, by, z)
    return [_mont(c) for c in x + y + z + bx + by]


def closes_cases(n, rng):
    plan = truth_plan(n, 32, ODD_AT[1])
    f2r = lambda: (rng.randrange(P), rng.randrange(1, P))
    zs = [(1, 0), (0, 1), (P - 1, 0), (0, P - 1), (2, 0)]

    def true_of(j, zone):
        z = zs[j % 8] if j % 8 < len(zs) else f2r()
        return _fpw(_reps(_closing_raw(f2r(), f2r(), z), rng, j // 8 if j % 8 == 7 else 2))

    bases = [_closing_raw(f2r(), f2r(), z) for z in (f2r(), (1, 0), f2r(), (0, 5))]
    lists = [_one_off(b, range(4), rng) for b in bases]
    ent = []
    for j in range(max(len(x) for x in lists)):
        lst = lists[j % len(bases)]
        if j < len(lst):
            k, v = lst[j]
            x = _reps(bases[j % len(bases)], rng, 2)
            x[k] = v
            ent.append((k, _fpw(x)))
    shapes = []
    for j in range(6):
        bx, by, z = f2r(), f2r(), f2r()
        good = _closing_raw(bx, by, z)
        shapes.append(_reps(_closing_raw(bx, by, (0, 0)), rng, j))                           # T = (0, 0, 0): closes but for Z = 0 (or p)
        shapes.append(good[:4] + _reps([0, 0], rng, j) + good[6:])                          # Z alone replaced by 0 (or p)
        x, y = closing_xy(bx, by, z)
        shapes.append(_reps([_mont(c) for c in x + m.f2neg(y) + z + bx + by], rng, 2))       # Y = +conj(by) g3 Z
        shapes.append(_reps(good[:6] + [_mont(c) for c in m.f2conj(bx) + by], rng, 2))       # bx, then by, handed over conjugated
        shapes.append(_reps(good[:6] + [_mont(c) for c in bx + m.f2conj(by)], rng, 2))
        for k in (4, 5):                                                                     # Z one off: X and Y both miss
            w = _reps(good, rng, 2)
            w[k] = _near(good[k] + (P if j % 2 else 0))[j % 3]
            shapes.append(w)
    for j, x in enumerate(shapes):
        ent.insert(8 + 3 * j, (None, _fpw(x)))
    return _fill(plan, true_of, lambda zone: ent)


def predicate_cases(mapping, op, n, rng):
    if (mapping, op) in ((0, 8), (1, 5)):
        return f2_pred_cases(n, rng, mapping)
    if (mapping, op) == (1, 6):
        return pair_f12_pred_cases(n, rng)
    if (mapping, op) == (1, 7):
        return closes_cases(n, rng)
    return wide_is_one_cases(n, rng, mapping)


def predicate_reference(mapping, op, wi):
    """[(verdict, components that miss, holds?, lanes that return it)] of one case, from Python integers mod p"""
    c = [_fp_of(wi, k) for k in range(len(wi) // 8)]
    if (mapping, op) in ((0, 8), (1, 5)):
        lanes = 1 if mapping == 0 else 2
        z = [k for k in (0, 1) if c[k] % P]
        e = [k for k in (0, 1) if (c[k] - c[2 + k]) % P]
        return [('is_zero', z, not z, lanes), ('eq', e, not e, lanes)]
    if (mapping, op) == (1, 6) or op == 2:
        one = [k for k in range(12) if (c[k] - _one_tgt()[k]) % P]
        if op == 2:
            return [('is_one', one, not one, 16 if mapping == 2 else 64)]
        cj = [k for k in range(12) if ((c[k] - c[12 + k]) if k < 6 else (c[k] + c[12 + k])) % P]
        return [('is_one', one, not one, 2), ('is_one', one, not one, 2), ('eq_conj', cj, not cj, 2)]
    v = [x * RI % P for x in c]
    z = (v[4], v[5])
    x, y = closing_xy((v[6], v[7]), (v[8], v[9]), z)
    miss = [k for k in range(4) if v[k] != (x + y)[k]]
    return [('closes', miss if z != (0, 0) else [], z != (0, 0) and not miss, 2)]


def predicate_profile(mapping, op, ins):
    """(expected words of every case, {(verdict, position): parities of the case indices at which that component alone misses})"""
    want, cover = [], {}
    for idx, wi in enumerate(as_array(ins, mapping, op)):
        row = []
        for name, miss, holds, lanes in predicate_reference(mapping, op, [int(x) for x in wi]):
            row += [1 if holds else 0] * lanes
            if len(miss) == 1:
                cover.setdefault((name, miss[0]), set()).add(idx % 2)
        want.append(row)
    return want, cover


PREDICATE_POSITIONS = {(0, 8): [('is_zero', 0), ('is_zero', 1), ('eq', 0), ('eq', 1)], (1, 7): [('closes', k) for k in range(4)],
                       (1, 6): [(v, k) for v in ('is_one', 'eq_conj') for k in range(12)], (2, 2): [('is_one', k) for k in range(12)]}
PREDICATE_POSITIONS[(1, 5)] = PREDICATE_POSITIONS[(0, 8)]
PREDICATE_POSITIONS[(3, 2)] = PREDICATE_POSITIONS[(2, 2)]


def assert_predicate_cases_bite(mapping, op, ins):
    """on the reference alone: a quarter of the expected words are 1 and a quarter 0, and the one-component-off cases reach every
    position at an even and at an odd case index (the two lane pairs of a DPP quad, the two halves of a row of groups)"""
    want, cover = predicate_profile(mapping, op, ins)
    flat = [b for row in want for b in row]
    assert 4 * sum(flat) >= len(flat) and 4 * (len(flat) - sum(flat)) >= len(flat), (sum(flat), len(flat))
    for key in PREDICATE_POSITIONS[(mapping, op)]:
        assert cover.get(key) == {0, 1}, (key, cover.get(key))


def check_predicates(mapping, op, ins, outs):
    want, _ = predicate_profile(mapping, op, ins)
    bad = []
    for idx, (wi, wo, ww) in enumerate(zip(ins, outs, want)):
        k = 0
        for name, miss, holds, lanes in predicate_reference(mapping, op, wi):
            got = list(wo[k:k + lanes])
            if len(set(got)) != 1:
                bad.append((idx, name, 'the lanes of the case disagree', got[:16], 'misses', miss))
            elif got[0] != (1 if holds else 0):
                bad.append((idx, name, 'every lane returned %d, the reference is %d' % (got[0], 1 if holds else 0), 'misses', miss))
            k += lanes
        assert k == len(wo) == len(ww)
        if list(wo) != ww and not bad:
            bad.append((idx, 'words', list(wo)[:16], ww[:16]))
    assert not bad, 'op %d: %d failing verdicts, first %s' % (op, len(bad), bad[:4])


# ---------------------------------------------------------------- G2: Jacobian group ops, membership, Miller line steps
# mapping 0 op 9 (group ops), op 10 (line steps, one value per lane); mapping 1 op 8 (the steps as miller_loop_p runs them), op 9
# (g2_on_twist / g2_in_subgroup in both lanes); mappings 2, 3 op 3 (w_line_dbl, w_line_add and the wide line products).
# The Jacobian ops are compared as group elements with spec_model's affine group law (which never uses the curve constant: a point off
# the twist lies on y^2 = x^3 + b' for its own b', and P, Q, R of one case are multiples of one point); the line steps with the formulas
# of zkv_curve.h restated over spec_model's f2* helpers (line_dbl_ref, line_add_ref, aff_*_ref -- checked on their own against the
# group law in test_line_references_agree_with_spec_model).
#
# Shares, asserted on the reference alone (assert_g2_cases_bite).  The category of case k of wavefront w is c = (k + w) % 4, so every
# category meets even and odd case indices and the first and the last case of a wavefront.  (place_edges is not used here: it puts a
# list of edges at the start of the batch and across the FIRST wavefront boundary only, while these conditions ask for both values of a
# verdict at the first and last case of wavefronts and at both parities, i.e. for edge and regular cases side by side in EVERY wavefront,
# group and pair block.)
#   membership   c = 0 subgroup, 1 off the twist, 2 on the twist outside the subgroup, 3 psi image of a subgroup point / outside / off the
#                twist, in turn: on_twist 2/3 ones, 1/3 zeros; in_subgroup 1/3 ones, 1/3 zeros (the verdict of a point off the twist is
#                not defined: raw_g2_valid never asks for it)
#   g2j_eq       1 for (k / 2 + w) even: half ones
#   line steps   c = 0, 2 regular (Z' != 0 in all three), 1: T = (0 : Y : 0) or Z = 0 (Z' = 0 after the tangent, the chord and the chain),
#                3: T = Q, T = -Q (chord only), Y = 0 (tangent and chain), 2 T = Q (chain only) in turn: zeros 5/16, 3/8, 3/8
G2_OPS = {(0, 9), (0, 10), (1, 8), (1, 9), (2, 3), (3, 3)}
INV2 = pow(2, -1, P)
B3 = m.f2smul(m.B2, 3)
GOLDEN = os.path.join(HERE, 'golden')


def f2sqr(a): return m.f2mul(a, a)
def f2dbl(a): return m.f2add(a, a)
def f2tpl(a): return m.f2smul(a, 3)
def f2half(a): return m.f2smul(a, INV2)
def f2inv0(a): return (0, 0) if a == (0, 0) else m.f2inv(a)          # f2_inv(0) = 0


def line_dbl_ref(T):
    """zkv_curve.h line_dbl: (T', l0, l1, l3), homogeneous projective T"""
    X, Y, Z = T
    a = f2half(m.f2mul(X, Y)); b = f2sqr(Y); c = f2sqr(Z)
    e = m.f2mul(B3, c); f = f2tpl(e); g = f2half(m.f2add(b, f))
    h = m.f2sub(f2sqr(m.f2add(Y, Z)), m.f2add(b, c)); j = f2sqr(X); e2 = f2sqr(e)
    T2 = (m.f2mul(a, m.f2sub(b, f)), m.f2sub(f2sqr(g), f2tpl(e2)), m.f2mul(b, h))
    return T2, m.f2neg(h), f2tpl(j), m.f2sub(e, b)


def line_add_ref(T, Q):
    """zkv_curve.h line_add"""
    X, Y, Z = T
    qx, qy = Q
    theta = m.f2sub(Y, m.f2mul(qy, Z)); lam = m.f2sub(X, m.f2mul(qx, Z))
    c = f2sqr(theta); d = f2sqr(lam); e = m.f2mul(lam, d); f = m.f2mul(Z, c); g = m.f2mul(X, d)
    h = m.f2sub(m.f2add(e, f), f2dbl(g))
    T2 = (m.f2mul(lam, h), m.f2sub(m.f2mul(theta, m.f2sub(g, h)), m.f2mul(e, Y)), m.f2mul(Z, e))
    return T2, lam, m.f2neg(theta), m.f2sub(m.f2mul(theta, qx), m.f2mul(lam, qy))


def aff_dbl_ref(T):
    """zkv_curve.h aff_dbl: ((x3, y3), nl, c)"""
    x, y = T
    lam = m.f2mul(f2tpl(f2sqr(x)), f2inv0(f2dbl(y)))
    x3 = m.f2sub(f2sqr(lam), f2dbl(x))
    return (x3, m.f2sub(m.f2mul(lam, m.f2sub(x, x3)), y)), m.f2neg(lam), m.f2sub(m.f2mul(lam, x), y)


def aff_add_ref(T, Q):
    x, y = T
    lam = m.f2mul(m.f2sub(Q[1], y), f2inv0(m.f2sub(Q[0], x)))
    x3 = m.f2sub(m.f2sub(f2sqr(lam), x), Q[0])
    return (x3, m.f2sub(m.f2mul(lam, m.f2sub(x, x3)), y)), m.f2neg(lam), m.f2sub(m.f2mul(lam, x), y)


def psi2(pt): return m.g2_frobenius(m.g2_frobenius(pt))


def step_q(Q, kind):
    """the chord operand of step kind 1..4 of ZKV_MILLER_STEP_KIND: Q, -Q, psi(Q), -psi^2(Q)"""
    return [None, Q, m.g2_neg(Q), m.g2_frobenius(Q), m.g2_neg(psi2(Q))][kind]


def chain_ref(T, Q):
    """T after tangent, chord(Q), tangent"""
    T = line_dbl_ref(T)[0]
    T = line_add_ref(T, Q)[0]
    return line_dbl_ref(T)[0]


def proj_to_aff(T):
    if T[2] == (0, 0):
        return None
    zi = m.f2inv(T[2])
    return (m.f2mul(T[0], zi), m.f2mul(T[1], zi))


_G2_POOLS = None
_IN_SUB = {}
OUT_MEMBERSHIP, OUT_KATS = [], []      # the twist points outside the subgroup by fixture: g2_membership_points, precompile_kats['g2_subgroup']


def outside_walk():
    """the points outside the subgroup in the order the line cases use them: a small-order point of precompile_kats, a point of
    g2_membership_points, and so on in turn -- the shortest case list (49 cases, about a dozen such Q) holds some of both"""
    g2_pools()
    k = max(len(OUT_KATS), len(OUT_MEMBERSHIP))
    return [pool[i % len(pool)] for i in range(k) for pool in (OUT_KATS, OUT_MEMBERSHIP)]


def g2_pools():
    """(subgroup points, twist points outside the subgroup) -- the generator and multiples, and the points of tests/golden"""
    global _G2_POOLS
    if _G2_POOLS is None:
        import json
        r = random.Random(0x62)
        sub = [m.G2_GEN, m.g2_mul(m.G2_GEN, 2), m.g2_neg(m.G2_GEN)] + [m.g2_mul(m.G2_GEN, r.randrange(1, RR)) for _ in range(5)]
        out = []
        H = lambda h: int(h, 16)
        pts = json.load(open(os.path.join(GOLDEN, 'g2_membership_points.json')))['points']
        n_membership = len(pts)
        pts += [c for c in json.load(open(os.path.join(GOLDEN, 'precompile_kats.json')))['g2_subgroup'] if c.get('on_twist', True)]
        for k, c in enumerate(pts):
            xi, xr, yi, yr = (H(h) for h in c['point'])             # EIP-197 order
            pt = ((xr, xi), (yr, yi))
            if max(xi, xr, yi, yr) < P and m.g2_on_curve(pt) and pt not in sub and pt not in out:
                (sub if c['in_subgroup'] else out).append(pt)
                if not c['in_subgroup']:
                    (OUT_MEMBERSHIP if k < n_membership else OUT_KATS).append(pt)
        for pt in sub:
            _IN_SUB[pt] = _IN_SUB[m.g2_frobenius(pt)] = True
        for pt in out:
            _IN_SUB[pt] = False
        assert len(sub) >= 12 and len(OUT_MEMBERSHIP) >= 20 and len(OUT_KATS) >= 4
        _G2_POOLS = (sub, out)
    return _G2_POOLS


def in_subgroup_ref(pt):
    if pt not in _IN_SUB:
        _IN_SUB[pt] = m.g2_in_subgroup(pt)
    return _IN_SUB[pt]


def _f2r(rng): return (rng.randrange(P), rng.randrange(P))
def _f2nz(rng): return (rng.randrange(1, P), rng.randrange(1, P))
def _f2w(c, rng): return words(_mont_rep(c[0], rng)) + words(_mont_rep(c[1], rng))
def _f2_of(w, k): return (_fp_of(w, 2 * k) * RI % P, _fp_of(w, 2 * k + 1) * RI % P)


def category(idx, n, per_wave):
    """(category 0..3, wavefront, place in it) of case idx: (k + w) % 4; a closing partial wavefront starts with category 1; one case
    per wavefront: the phase moves on every four, so that a category meets even and odd indices"""
    w, k = divmod(idx, per_wave)
    if per_wave == 1:
        return (w + w // 4) % 4, w, 0
    if w == n // per_wave:
        return (1, 2, 0, 3)[k % 4], w, k
    return (k + w) % 4, w, k


OFF_TWIST = [((0, 0), (0, 0)), ((0, 0), (1, 0)), ((1, 0), (0, 0)), ((1, 0), (1, 0)), ((P - 1, 0), (0, 1)), ((0, 1), (P - 1, P - 1)), ((P - 1, P - 1), (1, 1)),
             ((0, P - 1), (0, 0)), ((2, 0), (0, 3))]


def membership_point(c, j, rng):
    """the j-th point of category c (see the shares above)"""
    sub, out = g2_pools()
    if c == 0:
        return sub[j % len(sub)]
    if c == 2 or (c == 3 and j % 3 == 1):
        return out[(j if c == 2 else j // 3 + 7) % len(out)]
    if c == 3 and j % 3 == 0:
        return m.g2_frobenius(sub[(j // 3) % len(sub)])
    if c == 3:
        j = 3 * (j // 3) + 1 + (j // 3) % 2               # off the twist: a twist point with a coordinate altered, or random
    if j % 3 == 0:
        return OFF_TWIST[(j // 3) % len(OFF_TWIST)]
    x, y = rng.choice(sub + out)
    if j % 3 == 1:                                      # a twist point with one coordinate one off, conjugated or swapped
        return [(x, m.f2add(y, (1, 0))), (m.f2add(x, (0, 1)), y), (m.f2conj(x), y), (y, x)][(j // 3) % 4]
    return (_f2r(rng), _f2r(rng))


def _jac2(pt, rng):
    """affine Fp2 point (or None) -> Jacobian words with a random z; infinity has z = 0 (either representative) and any x, y"""
    if pt is None:
        return _f2w(_f2nz(rng), rng) + _f2w(_f2nz(rng), rng) + words(rng.choice([0, P])) + words(rng.choice([0, P]))
    z = rng.choice([(1, 0), (0, 1), _f2nz(rng), _f2nz(rng)])
    z2 = f2sqr(z)
    return _f2w(m.f2mul(pt[0], z2), rng) + _f2w(m.f2mul(pt[1], m.f2mul(z2, z)), rng) + _f2w(z, rng)


def g2_group_cases(n, rng):
    """P Q R: Q by category; P a multiple of Q (Q itself, -Q, infinity, 2Q, others); R equal to P in another representative where
    g2j_eq is to hold, else -P, another multiple or infinity -- so that the branches for infinity, equal and opposite points are taken
    by neighbours of regular cases"""
    cnt = [0] * 4
    out = []
    for idx in range(n):
        c, w, k = category(idx, n, 64)
        j = cnt[c]
        cnt[c] += 1
        q = membership_point(c, j, rng)
        mults = [1, -1, 0, 2, rng.randrange(3, 40), rng.randrange(3, 40), 1, -1][(j + w) % 8 if n > 8 else idx % 8]
        mul = lambda kk: None if kk == 0 else (m.g2_mul(q, kk) if kk > 0 else m.g2_neg(m.g2_mul(q, -kk)))
        p = mul(mults)
        if (k // 2 + w) % 2 == 0:
            r = p
        else:
            r = [m.g2_neg(p), mul(mults + 1), None, mul(-2)][j % 4]
            if r == p:
                r = mul(5) if p is None else None
        out.append(_jac2(p, rng) + _f2w(q[0], rng) + _f2w(q[1], rng) + _jac2(r, rng))
    return out


def membership_cases(n, rng):
    cnt = [0] * 4
    out = []
    for idx in range(n):
        c = category(idx, n, 32)[0]
        q = membership_point(c, cnt[c], rng)
        cnt[c] += 1
        out.append(_f2w(q[0], rng) + _f2w(q[1], rng))
    return out


def _jac2_to_aff(w):
    x, y, z = (_f2_of(w, k) for k in range(3))
    if z == (0, 0):
        return None
    zi = m.f2inv(z)
    zi2 = f2sqr(zi)
    return (m.f2mul(x, zi2), m.f2mul(y, m.f2mul(zi2, zi)))


def g2_group_reference(wi):
    """the expected group elements and verdicts of one case of mapping 0 op 9"""
    p, q, r = _jac2_to_aff(wi[0:48]), (_f2_of(wi, 3), _f2_of(wi, 4)), _jac2_to_aff(wi[80:128])
    on = m.g2_on_curve(q)
    return {'dbl': m.g2_add(p, p), 'add_affine': m.g2_add(p, q), 'add': m.g2_add(p, r), 'psi': None if p is None else m.g2_frobenius(p),
            'mul_u': m.g2_mul(q, m.U), 'eq': p == r, 'on_twist': on, 'in_subgroup': in_subgroup_ref(q) if on else None}


def membership_reference(wi):
    q = (_f2_of(wi, 0), _f2_of(wi, 1))
    on = m.g2_on_curve(q)
    return {'on_twist': on, 'in_subgroup': in_subgroup_ref(q) if on else None}


def _below_2p(w, what):
    vals = [_fp_of(w, k) for k in range(len(w) // 8)]
    assert all(v < 2 * P for v in vals), (what, 'not below 2p', [hex(v) for v in vals if v >= 2 * P][:2])


def check_g2_group(ins, outs):
    bad = []
    for idx, (wi, wo) in enumerate(zip(ins, outs)):
        try:
            want = g2_group_reference(wi)
            _below_2p(wo[:240], 'g2')
            for k, nm in enumerate(['dbl', 'add_affine', 'add', 'psi', 'mul_u']):
                assert _jac2_to_aff(wo[48 * k:48 * k + 48]) == want[nm], ('g2j_' + nm, 'infinity expected' if want[nm] is None else '')
            assert wo[240] == int(want['eq']), ('g2j_eq', wo[240])
            assert wo[241] == int(want['on_twist']), ('g2_on_twist', wo[241])
            assert wo[242] in (0, 1) and (want['in_subgroup'] is None or wo[242] == int(want['in_subgroup'])), ('g2_in_subgroup', wo[242])
            assert list(wo[243:248]) == [0] * 5
        except AssertionError as e:
            bad.append((idx, str(e)))
    assert not bad, 'g2 group ops: %d failing cases, first %s' % (len(bad), bad[:3])


def check_membership(ins, outs):
    bad = []
    for idx, (wi, wo) in enumerate(zip(ins, outs)):
        want = membership_reference(wi)
        if wo[0] != wo[1] or wo[2] != wo[3]:
            bad.append((idx, 'the lanes of the pair disagree', list(wo)))
        elif wo[0] != int(want['on_twist']) or wo[2] not in (0, 1) or (want['in_subgroup'] is not None and wo[2] != int(want['in_subgroup'])):
            bad.append((idx, list(wo), want))
    assert not bad, 'membership: %d failing cases, first %s' % (len(bad), bad[:3])


# ---- line steps: T (X Y Z) Q (x y), value domain
LINE_EDGE = [0, 1, P - 1]


def line_values(n, rng, per_wave):
    """[(T, Q, Q2)] by category (see the shares above).  Regular cases: T a random projective scaling of a multiple of Q, Q in the
    subgroup, outside it (tests/golden, in the order of outside_walk: small-order and membership points in turn) or a psi image; coordinates 0, 1, p - 1 and a Q with a zero component; generic field elements
    and small distinct primes (no two of theta, lambda, qx, qy, X, Y, Z equal: a wrong operand pick of a wide round changes a product,
    and with the primes each product of a round is a small value of its own) and one family in which two of them DO coincide
    (qx = qy, X = Y, Y = Z), where a swapped pick of just those two would go unseen."""
    sub, out = g2_pools()
    walk = outside_walk()
    HALF = (RR + 1) // 2
    cnt = [0] * 4
    used = [0]                                  # outside points handed out so far, over all categories
    res = []

    def outside():
        used[0] += 1
        return walk[(used[0] - 1) % len(walk)]

    def scaled(t):
        s = rng.choice([(1, 0), _f2nz(rng), _f2nz(rng)])
        return (m.f2mul(t[0], s), m.f2mul(t[1], s), s)

    for idx in range(n):
        c = category(idx, n, per_wave)[0]
        j = cnt[c]
        cnt[c] += 1
        q = sub[(j // 3) % len(sub)] if j % 3 == 0 else outside() if j % 3 == 1 and c != 2 else m.g2_frobenius(sub[(j // 3 + 3) % len(sub)])
        if c == 0:
            while True:                         # a multiple of THIS Q that keeps clear of the exceptional cases (some multiplier below 30 does,
                for _ in range(60):             # whatever the order of Q; else the next outside point)
                    t = m.g2_mul(q, rng.randrange(2, 30))
                    if t is not None and t[0] != q[0] and proj_to_aff(chain_ref(t + ((1, 0),), q)) is not None:
                        break
                else:
                    q = outside()
                    continue
                break
            T = scaled(t)
        elif c == 2:
            if j % 3 == 0:
                e = lambda: (rng.choice(LINE_EDGE), rng.choice(LINE_EDGE))
                T = (e(), e(), rng.choice([(1, 0), (0, 1), (P - 1, P - 1), (1, P - 1)]))
                q = [((0, 0), _f2nz(rng)), (_f2nz(rng), (0, 0)), (e(), e()), ((0, rng.randrange(1, P)), (rng.randrange(1, P), 0))][(j // 3) % 4]
            elif j % 3 == 1:
                T, q = (_f2nz(rng), _f2nz(rng), _f2nz(rng)), (_f2nz(rng), _f2nz(rng))
                f = (j // 3) % 3
                if f == 0: q = (q[0], q[0])
                elif f == 1: T = (T[0], T[0], T[2])
                else: T = (T[0], T[1], T[1])
            elif j % 2:
                T, q = (_f2nz(rng), _f2nz(rng), _f2nz(rng)), (_f2nz(rng), _f2nz(rng))
            else:                               # X Y Z qx qy: five distinct small primes, each times 1, i or 1 + i, in any order: every one of
                while True:                     # the 10 / 13 products is a small value no other product equals
                    v = [m.f2smul(rng.choice([(1, 0), (0, 1), (1, 1)]), k) for k in rng.sample([2, 3, 5, 7, 11, 13, 17, 19, 23], 5)]
                    T, q = (v[0], v[1], v[2]), (v[3], v[4])
                    if len(set(v + [m.f2sub(v[1], m.f2mul(v[4], v[2])), m.f2sub(v[0], m.f2mul(v[3], v[2]))])) == 7:
                        break
        elif c == 1:
            T = ((0, 0), rng.choice([(1, 0), _f2nz(rng)]), (0, 0)) if j % 2 == 0 else (_f2r(rng), _f2r(rng), (0, 0))
        else:
            f = j % 4
            if f == 0: T = scaled(q)
            elif f == 1: T = scaled(m.g2_neg(q))
            elif f == 2: T = (_f2nz(rng), (0, 0), _f2nz(rng))
            else:
                q = sub[j % len(sub)]
                T = scaled(m.g2_mul(q, HALF))
        q2 = q if j % 5 == 0 else (m.g2_neg(q) if j % 5 == 1 else rng.choice(sub + out))
        res.append((T, q, q2))
    return res


def _pt_words(vals, rng):
    w = []
    for c in vals:
        w += _f2w(c, rng)
    return w


def _f12_rand_words(rng, j):
    a = _f12_special([3, 3, 2, 0, 3, 1][j % 6], rng)
    return f12_words(_mont_words_of(a, rng, rng.random() < 0.5))


def line_cases(mapping, n, rng):
    out = []
    for j, (T, q, q2) in enumerate(line_values(n, rng, PER_WAVE[mapping])):
        w = _pt_words(T, rng) + _pt_words(q, rng)
        if mapping == 0:
            w += _pt_words(q2, rng)
        else:
            w += words(_mont_rep(rng.randrange(P), rng)) + words(_mont_rep(rng.randrange(P), rng)) + _f12_rand_words(rng, j)
        if mapping >= 2:
            for _ in range(4):
                w += _f2w(_f2r(rng), rng)
            for _ in range(4):
                w += words(_mont_rep(rng.choice([0, 1, rng.randrange(P), rng.randrange(P)]), rng))
        out.append(w)
    return out


def line_reference(wi):
    """T, Q of a case (both start at word 0 in every mapping) -> the tangent and the four chords as (T', l0, l1, l3), the chain's T"""
    T = tuple(_f2_of(wi, k) for k in range(3))
    Q = (_f2_of(wi, 3), _f2_of(wi, 4))
    return T, Q, [line_dbl_ref(T)] + [line_add_ref(T, step_q(Q, kind)) for kind in (1, 2, 3, 4)], chain_ref(T, Q)


def assert_line_cases_hold_golden_points(ins, mapping, op):
    """on the inputs alone: some Q is a small-order point of precompile_kats['g2_subgroup'], some Q a point of g2_membership_points outside
    the subgroup, some Q a subgroup point"""
    sub, _ = g2_pools()
    qs = {(_f2_of(wi, 3), _f2_of(wi, 4)) for wi in ([int(x) for x in r] for r in as_array(ins, mapping, op))}
    assert qs & set(OUT_KATS) and qs & set(OUT_MEMBERSHIP) and qs & set(sub), (len(qs & set(OUT_KATS)), len(qs & set(OUT_MEMBERSHIP)))


def line_verdicts(wi):
    T, Q, steps, chain = line_reference(wi)
    return {'tangent Z = 0': steps[0][0][2] == (0, 0), 'chord Z = 0': steps[1][0][2] == (0, 0), 'chain Z = 0': chain[2] == (0, 0)}


def _f2s_match(w, want, what):
    """w: 16 words per expected Fp2: below 2p and congruent (either representative of 0 is 0)"""
    _below_2p(w, what)
    for k, c in enumerate(want):
        assert _f2_of(w, k) == c, (what, 'Fp2 %d' % k, 'want 0' if c == (0, 0) else '')


def _step_words(step): return list(step[0]) + list(step[1:])


def _f12_match(w, want, what):
    assert _f12_out(w, 0) == want, what


def _var_line_ref(f, step, xs, ys): return m.f12mul(f, line_f12(step[1], m.f2smul(step[2], xs), m.f2smul(step[3], ys)))


def check_lane_lines(ins, outs):
    bad = []
    for idx, (wi, wo) in enumerate(zip(ins, outs)):
        try:
            T, Q, steps, _ = line_reference(wi)
            Q2 = (_f2_of(wi, 5), _f2_of(wi, 6))
            _f2s_match(wo[0:96], _step_words(steps[0]), 'line_dbl')
            _f2s_match(wo[96:192], _step_words(steps[1]), 'line_add')
            _f2s_match(wo[192:224], m.g2_frobenius(Q), 'g2_frob_affine')
            _f2s_match(wo[224:256], psi2(Q), 'g2_frob2_affine')
            for k, (pt, nl, c) in enumerate([aff_dbl_ref(Q), aff_add_ref(Q, Q2)]):
                _f2s_match(wo[256 + 64 * k:320 + 64 * k], [pt[0], pt[1], nl, c], ['aff_dbl', 'aff_add'][k])
        except AssertionError as e:
            bad.append((idx, str(e)))
    assert not bad, 'lane line steps: %d failing cases, first %s' % (len(bad), bad[:3])


def check_pair_lines(ins, outs):
    bad = []
    for idx, (wi, wo) in enumerate(zip(ins, outs)):
        try:
            T, Q, steps, chain = line_reference(wi)
            xs, ys = _fp_of(wi, 10) * RI % P, _fp_of(wi, 11) * RI % P
            f = f12_from_words(wi[96:192])[1]
            for k in range(5):
                _f2s_match(wo[96 * k:96 * k + 96], _step_words(steps[k]), ['tangent', 'chord Q', 'chord -Q', 'chord psi(Q)', 'chord -psi^2(Q)'][k])
            _f12_match(wo[480:576], _var_line_ref(f, steps[0], xs, ys), 'variable-line product')
            _f2s_match(wo[576:624], chain, 'tangent, chord, tangent')
            assert list(wo[624:720]) == list(wo[0:96]), 'g2m_line_dbl differs from the step of miller_loop_p'
            assert list(wo[720:816]) == list(wo[96:192]), 'g2m_line_add differs from the step of miller_loop_p'
        except AssertionError as e:
            bad.append((idx, str(e)))
    assert not bad, 'pair line steps: %d failing cases, first %s' % (len(bad), bad[:3])


def check_wide_lines(ins, outs, S):
    bad = []
    step_w = 48 + 48 * 8 * S
    for idx, (wi, wo) in enumerate(zip(ins, outs)):
        try:
            T, Q, steps, chain = line_reference(wi)
            xs, ys = _fp_of(wi, 10) * RI % P, _fp_of(wi, 11) * RI % P
            f = f12_from_words(wi[96:192])[1]
            L = [_f2_of(wi, 12 + k) for k in range(4)]
            ks = [_fp_of(wi, 32 + k) * RI % P for k in range(4)]
            for k, nm in enumerate(['w_line_dbl', 'w_line_add']):
                o = wo[step_w * k:step_w * (k + 1)]
                _f2s_match(o[0:48], steps[k][0], nm + ' T')
                for pr in range(8 * S):
                    _f2s_match(o[48 + 48 * pr:96 + 48 * pr], steps[k][1:], '%s, the copy of pair %d' % (nm, pr))
                    assert list(o[48 + 48 * pr:96 + 48 * pr]) == list(o[48:96]), (nm, 'pair %d holds other words than pair 0' % pr)
            o = wo[2 * step_w:]
            _f12_match(o[0:96], _var_line_ref(f, steps[0], xs, ys), 'var_line_mul_w')
            ll = line_f12((1, 0), m.f2smul(L[0], ks[0]), m.f2smul(L[1], ks[1]))
            lc = line_f12((1, 0), m.f2smul(L[2], ks[2]), m.f2smul(L[3], ks[3]))
            _f12_match(o[96:192], m.f12mul(m.f12mul(f, ll), lc), 'fixed_lines_mul_w(1, 1)')
            _f12_match(o[192:288], m.f12mul(f, ll), 'fixed_lines_mul_w(1, 0)')
            _f12_match(o[288:384], m.f12mul(f, lc), 'fixed_lines_mul_w(0, 1)')
            inv = _f12_out(o[384:480], 0)
            assert (m.f12mul(inv, f) == m.F12_ONE) if any(f) else not any(inv), 'f12m_inv_w'
            _f2s_match(o[480:528], chain, 'tangent, chord, tangent')
        except AssertionError as e:
            bad.append((idx, str(e)))
    assert not bad, 'wide line steps: %d failing cases, first %s' % (len(bad), bad[:3])


def g2_verdicts(mapping, op, ins):
    """per case {verdict name: bool, or None where the reference leaves it open}: the 0 / 1 outputs, and Z' = 0 of the line steps"""
    rows = []
    for wi in as_array(ins, mapping, op):
        wi = [int(x) for x in wi]
        if (mapping, op) == (0, 9):
            r = g2_group_reference(wi)
            rows.append({k: r[k] for k in ('eq', 'on_twist', 'in_subgroup')})
        elif (mapping, op) == (1, 9):
            rows.append(membership_reference(wi))
        else:
            rows.append(line_verdicts(wi))
    return rows


def assert_g2_cases_bite(mapping, op, ins):
    """on the reference alone: every verdict is 1 in at least a quarter of the cases and 0 in at least a quarter, takes both values at
    even and at odd case indices, and at the first and at the last case of a wavefront"""
    rows = g2_verdicts(mapping, op, ins)
    if (mapping, op) in ((0, 10), (1, 8), (2, 3), (3, 3)):
        assert_line_cases_hold_golden_points(ins, mapping, op)
    n, pw = len(rows), PER_WAVE[mapping]
    for name in rows[0]:
        bits = [r[name] for r in rows]
        ones, zeros = sum(1 for b in bits if b is True), sum(1 for b in bits if b is False)
        assert 4 * ones >= n and 4 * zeros >= n, (name, ones, zeros, n)
        assert {(b, i % 2) for i, b in enumerate(bits) if b is not None} == {(False, 0), (False, 1), (True, 0), (True, 1)}, name
        full = n // pw * pw
        assert {bits[i] for i in range(0, full, pw)} >= {False, True} and {bits[i] for i in range(pw - 1, full, pw)} >= {False, True}, name


# ---------------------------------------------------------------- raw operands at the bounds of the contract
# The Fp12 routines, the cyclotomic squarings, the line steps and the Jacobian ops take "reduced values (below 2p)".  The generators above
# hand them v R mod p (sometimes + p): random-looking words.  These hand them the RAW integers at which a lazy sum inside a fused body
# is largest: 2p - 1 in every place ("hot"), 0 ("cold") where a difference is to be most negative, every 29-bit limb or every 32-bit
# word full.  The references read their expectation off the input words (f12_from_words, _f2_of, _jac_to_aff), so check() is unchanged.
#   Fp12 products      (1, 3) (2, 0) (3, 0): every Fp of a, b, c0, c3, c4 is free
#   cyclotomic squares (1, 4) (2, 1) (3, 1): the value must be cyclotomic; each coefficient is x or x + p
#   line steps         (0, 10) (1, 8) (2, 3) (3, 3): the formulas are algebraic, every Fp is free
#   Jacobian ops       (0, 7) (0, 9): P, Q, R stay multiples of one point (the reference is the affine group law); z's raw word is free
# A batch is place_edges(bound cases, cases_for(...)): the bound cases first, again across the first wavefront boundary where the list
# fits into a wavefront (a longer list crosses the boundaries by itself), value-domain cases in the rest, so that hot lanes run beside
# ordinary ones.  A new fused body adds the pattern that drives ITS largest column to the structured lists below, and to the
# independent restatement of them in assert_bound_cases_bite.
BOUND_OPS = {(1, 3): 'f12', (2, 0): 'f12', (3, 0): 'f12', (1, 4): 'cyclo', (2, 1): 'cyclo', (3, 1): 'cyclo',
             (0, 10): 'line', (1, 8): 'line', (2, 3): 'line', (3, 3): 'line', (0, 7): 'g1', (0, 9): 'g2'}
HOT, COLD = 2 * P - 1, 0
ALL29 = val9([M29] * 8 + [(HOT >> 232) - 1])                 # all eight low 29-bit limbs full, the top limb one below that of 2p - 1
ALL32 = unwords([0xffffffff] * 7 + [(HOT >> 224) - 1])      # all seven low 32-bit words full, likewise
BOUND_EDGES = [HOT, 2 * P - 2, P + 1, P, P - 1, 1, 0, ALL29, ALL32]
assert all(0 <= v < 2 * P for v in BOUND_EDGES) and len(BOUND_EDGES) % 2 == 1
LINE_SETTINGS = [[HOT] * 6, [COLD] * 6, [HOT, COLD] * 3, [COLD, HOT] * 3, [ALL29] * 6, [P] * 6]       # c0 c3 c4 of the Fp12 ops
LINE_NFP = {0: 14, 1: 24, 2: 36, 3: 36}                     # T 0-5, Q 6-9, then Q2 10-13 (mapping 0) or xs ys 10 11, f 12-23, L0 L1 24-31, lxs lys cxs cys 32-35


def _bound_row(vals):
    assert all(0 <= v < 2 * P for v in vals), 'a bound case holds a word that is not below 2p'
    return _fpw(vals)


def _edge_mix(rng, k): return [rng.choice(BOUND_EDGES) for _ in range(k)]


def f12_patterns():
    """(patterns over the twelve Fp of an Fp12 that are no slot patterns, slot patterns); position 2 slot + component, slots g0 g1 g2 h0 h1 h2"""
    flat = [[e] * 12 for e in BOUND_EDGES]
    flat += [[HOT, COLD] * 6, [COLD, HOT] * 6]              # c0 against c1: a0 b0 - a1 b1 most positive, most negative
    flat += [[HOT] * 6 + [COLD] * 6, [COLD] * 6 + [HOT] * 6]                               # g against h
    slot = []
    for s in range(6):
        slot.append([HOT if k // 2 == s else COLD for k in range(12)])
        slot.append([COLD if k // 2 == s else HOT for k in range(12)])
    return flat, slot


def f12_bound_cases(rng, mixes=4):
    """a b c0 c3 c4: every ordered pair of the non-slot patterns (13 x 13: with an odd count the index 13 i + j gives every pattern of
    a and of b both parities), every slot pattern against uniform hot and uniform cold in both orders, seeded mixes of the edge values.
    The line operands cycle through LINE_SETTINGS, the phase moving on after every round (so that a setting meets both parities)."""
    flat, slot = f12_patterns()
    assert len(flat) % 2 == 1
    ab = [(a, b) for a in flat for b in flat]
    for s in slot:
        for u in ([HOT] * 12, [COLD] * 12):
            ab += [(s, u), (u, s)]
    ab += [(_edge_mix(rng, 12), _edge_mix(rng, 12)) for _ in range(mixes)]
    return [_bound_row(a + b + LINE_SETTINGS[(k + k // 6) % 6]) for k, (a, b) in enumerate(ab)]


def cyclo_shifts():
    """which of the twelve coefficients hold x + p: none, all, c0, c1, g, h, each slot"""
    masks = [[False] * 12, [True] * 12, [k % 2 == 0 for k in range(12)], [k % 2 == 1 for k in range(12)], [k < 6 for k in range(12)], [k >= 6 for k in range(12)]]
    return masks + [[k // 2 == s for k in range(12)] for s in range(6)]


def cyclo_bound_cases(rng=None):
    """every element of cyclotomic_pool() and 1, in every shift of cyclo_shifts(); shift by shift, so that with five elements a
    coefficient meets both representatives at both parities"""
    elems = [_f12_raw(c) for c in cyclotomic_pool()] + [_f12_raw(m.F12_ONE)]
    assert len(elems) % 2 == 1
    return [_bound_row([x + P if s else x for x, s in zip(e, mask)]) for mask in cyclo_shifts() for e in elems]


def line_patterns(mapping):
    """structured rows over every Fp of the op's operands (LINE_NFP)"""
    n = LINE_NFP[mapping]
    T, Q = range(0, 6), range(6, 14 if mapping == 0 else 10)
    f, scal = range(12, 24), [10, 11] + list(range(24, n))          # f; xs ys and, wide, L0 L1 lxs lys cxs cys
    rows = [[e] * n for e in BOUND_EDGES]
    rows += [[HOT if k % 2 == 0 else COLD for k in range(n)], [COLD if k % 2 == 0 else HOT for k in range(n)]]
    for t, q in ((HOT, COLD), (COLD, HOT)):
        rows.append([t if k in T else q if k in Q else ALL29 for k in range(n)])
    if mapping:                                 # f against the operands that scale and form the lines (T and Q full, or the lines are 0)
        for a, b in ((HOT, COLD), (COLD, HOT)):
            rows.append([a if k in f else b if k in scal else ALL29 for k in range(n)])
    return rows


def line_bound_cases(mapping, rng, mixes=6):
    """the structured rows, seeded mixes, and the structured rows again from an odd index (every row meets both parities)"""
    rows = line_patterns(mapping)
    out = rows + [_edge_mix(rng, LINE_NFP[mapping]) for _ in range(mixes)]
    if len(out) % 2 == 0:
        out.append(_edge_mix(rng, LINE_NFP[mapping]))
    return [_bound_row(r) for r in out + rows]


def _z_plan(k, shift=0):
    """(index into BOUND_EDGES, component of an Fp2 z) of case k: the edges in turn, the component changing every two rounds -- nine edges,
    so case 9 q + j has the parity of q + j and every (edge, component) meets both"""
    return (k + shift) % len(BOUND_EDGES), ((k // len(BOUND_EDGES)) // 2) % 2


def _jac_raw_z(pt, zraw):
    """_jac with z's raw Montgomery word given and x, y in the x + p representative; z = 0 (mod p) is infinity, for which x = y = 1"""
    z = zraw * RI % P
    if pt is None or z == 0:
        assert z == 0
        return words(ONE_M + P) + words(ONE_M + P) + words(zraw)
    return words(_mont(pt[0] * z * z % P) + P) + words(_mont(pt[1] * z * z * z % P) + P) + words(zraw)


def g1_bound_cases(rng, n=72):
    """the points of g1_cases (decoded from its rows); z of P and of T at each edge value.  A point at infinity keeps z = 0 or p."""
    out = []
    for k, w in enumerate(g1_cases(n, rng)):
        p, t = _jac_to_aff(w[0:24]), _jac_to_aff(w[40:64])
        zp, zt = BOUND_EDGES[_z_plan(k)[0]], BOUND_EDGES[_z_plan(k, 4)[0]]
        zp = zp if p is not None else (P if k % 2 else 0)
        zt = zt if t is not None else (0 if k % 2 else P)
        q = [_fp_of(w, 3) % P + P, _fp_of(w, 4) % P + P]
        out.append(_bound_row([unwords(x) for x in _chunks(_jac_raw_z(p, zp) + _fpw(q) + _jac_raw_z(t, zt))]))
    return out


def _chunks(w): return [w[8 * k:8 * k + 8] for k in range(len(w) // 8)]


def _jac2_raw_z(pt, zraw):
    """_jac2 with both raw words of z given and x, y in the x + p representative; z = 0 (mod p) in both components is infinity"""
    z = (zraw[0] * RI % P, zraw[1] * RI % P)
    if pt is None or z == (0, 0):
        assert z == (0, 0)
        return [ONE_M + P, P, ONE_M + P, P, zraw[0], zraw[1]]
    z2 = f2sqr(z)
    x, y = m.f2mul(pt[0], z2), m.f2mul(pt[1], m.f2mul(z2, z))
    return [_mont(c) + P for c in x + y] + list(zraw)


def g2_bound_cases(rng, n=72):
    """the points of g2_group_cases (decoded from its rows); each component of z of P and of R at each edge value, the other component
    a random nonzero value, or (every third round) the same edge.  A point at infinity keeps z = 0 or p in both components."""
    out = []
    for k, w in enumerate(g2_group_cases(n, rng)):
        row = []
        for pt, shift, flip in ((_jac2_to_aff(w[0:48]), 0, 0), (_jac2_to_aff(w[80:128]), 4, 1)):
            j, comp = _z_plan(k, shift)
            comp ^= flip
            if pt is None:
                z = [P if (k + flip) % 2 else 0, 0 if (k // 2) % 2 else P]
            else:
                z = [_mont(rng.randrange(1, P)) + (P if k % 2 else 0)] * 2
                z[comp] = BOUND_EDGES[j]
                if (k // len(BOUND_EDGES)) % 3 == 2 and BOUND_EDGES[j] % P:
                    z[1 - comp] = BOUND_EDGES[j]
            row.append(_jac2_raw_z(pt, z))
        q = [_fp_of(w, 6 + c) % P + P for c in range(4)]
        out.append(_bound_row(row[0] + q + row[1]))
    return out


def bound_batch_size(mapping, nb):
    """64 3 + 1 lanes, 32 7 + 1 lane pairs; wide groups: whole blocks of four wavefronts that hold the nb bound cases and at least one
    block of other cases, and one case more (a last partial block)"""
    if mapping < 2:
        return (64 * 3 + 1, 32 * 7 + 1)[mapping]
    block = 4 * PER_WAVE[mapping]
    return -(-(nb + block) // block) * block + 1


def bound_cases_for(mapping, op, seed=7):
    """the batch of (mapping, op): its bound cases, placed by place_edges among the value-domain cases of cases_for"""
    rng = random.Random(0xB0D + seed * 1000 + mapping * 10 + op)
    kind = BOUND_OPS[(mapping, op)]
    bounds = {'f12': lambda: f12_bound_cases(rng), 'cyclo': lambda: cyclo_bound_cases(rng), 'line': lambda: line_bound_cases(mapping, rng),
              'g1': lambda: g1_bound_cases(rng), 'g2': lambda: g2_bound_cases(rng)}[kind]()
    n = bound_batch_size(mapping, len(bounds))
    assert len(bounds) < n
    return place_edges(bounds, iter(cases_for(mapping, op, n, seed)), n, PER_WAVE[mapping])


def all_hot_case(mapping, op):
    """one case with every operand word at 2p - 1"""
    return [_bound_row([HOT] * (IO[(mapping, op)][0] // 8))]


def assert_bound_cases_bite(mapping, op, ins):
    """On the inputs alone, before anything is compared.  Every operand word is below 2p; every free Fp position holds each of 2p - 1,
    p, 0 and ALL29 at an even and at an odd case index (the two lane pairs of a DPP quad, the two halves of a row of groups); the
    all-hot case and every structured pattern are there, both halves of each complementary pair among them.  The patterns are
    restated here by position, NOT taken from the generators: a pattern dropped from a generator makes this fail."""
    kind = BOUND_OPS[(mapping, op)]
    rows = [[_fp_of(r, k) for k in range(len(r) // 8)] for r in ([int(x) for x in row] for row in as_array(ins, mapping, op))]
    assert all(v < 2 * P for r in rows for v in r), 'an operand word is not below 2p'
    hot, p, all29, all32 = 2 * P - 1, P, sum(M29 << (29 * i) for i in range(8)) + ((((2 * P - 1) >> 232) - 1) << 232), \
        (1 << 224) - 1 + ((((2 * P - 1) >> 224) - 1) << 224)
    edges = [hot, hot - 1, p + 1, p, p - 1, 1, 0, all29, all32]

    def both_parities(positions, values):
        for k in positions:
            for v in values:
                seen = {i % 2 for i, r in enumerate(rows) if r[k] == v}
                assert seen == {0, 1}, ('Fp position %d holds %s at case parities %s only' % (k, hex(v), sorted(seen)))

    def holds(name, want, lo=0):
        assert any(r[lo:lo + len(want)] == want for r in rows), 'no case with the pattern: ' + name

    if kind == 'f12':
        both_parities(range(30), (hot, p, 0, all29))
        holds('every operand uniform 2p - 1', [hot] * 30)
        flat = [('uniform ' + hex(e), [e] * 12) for e in edges]
        flat += [('c0 hot, c1 cold', [hot, 0] * 6), ('c1 hot, c0 cold', [0, hot] * 6), ('g hot, h cold', [hot] * 6 + [0] * 6), ('h hot, g cold', [0] * 6 + [hot] * 6)]
        pairs = {(tuple(r[0:12]), tuple(r[12:24])) for r in rows}
        for na, a in flat:
            for nb, b in flat:
                assert (tuple(a), tuple(b)) in pairs, 'no case with a: %s and b: %s' % (na, nb)
        for s in range(6):
            for x, y, nm in ((hot, 0, 'hot'), (0, hot, 'cold')):
                pat = tuple(x if k // 2 == s else y for k in range(12))
                for u in ((hot,) * 12, (0,) * 12):
                    assert (pat, u) in pairs and (u, pat) in pairs, 'slot %d alone %s is not tried against uniform %s in both orders' % (s, nm, hex(u[0]))
        for nm, c in (('hot', [hot] * 6), ('cold', [0] * 6), ('hot / cold', [hot, 0] * 3), ('cold / hot', [0, hot] * 3), ('ALL29', [all29] * 6), ('p', [p] * 6)):
            holds('line operands ' + nm, c, 24)
    elif kind == 'cyclo':
        masks = {tuple(v >= P for v in r) for r in rows}
        for k in range(12):
            seen = {(r[k] >= P, i % 2) for i, r in enumerate(rows)}
            assert seen == {(False, 0), (False, 1), (True, 0), (True, 1)}, ('coefficient %d' % k, sorted(seen))
        want = [('none', lambda k: False), ('all', lambda k: True), ('c0', lambda k: k % 2 == 0), ('c1', lambda k: k % 2 == 1), ('g', lambda k: k < 6), ('h', lambda k: k >= 6)]
        want += [('slot %d' % s, lambda k, s=s: k // 2 == s) for s in range(6)]
        for nm, f in want:
            assert tuple(f(k) for k in range(12)) in masks, 'no case shifted by p in: ' + nm
        one = [RM % P] + [0] * 11
        for nm, f in want:                      # 1 = (R mod p, 0, ...) in every shift: raw p in every coefficient but the first
            holds('1 shifted in ' + nm, [x + P if f(k) else x for k, x in enumerate(one)])
    elif kind == 'line':
        n = len(rows[0])
        both_parities(range(n), (hot, p, 0, all29))
        for e in edges:
            holds('uniform ' + hex(e), [e] * n)
        holds('hot / cold alternating', [hot if k % 2 == 0 else 0 for k in range(n)])
        holds('cold / hot alternating', [0 if k % 2 == 0 else hot for k in range(n)])
        nq = 8 if mapping == 0 else 4
        holds('T hot, Q cold', [hot] * 6 + [0] * nq)
        holds('T cold, Q hot', [0] * 6 + [hot] * nq)
        if mapping:
            assert any(r[12:24] == [hot] * 12 and set(r[10:12] + r[24:]) == {0} and 0 not in r[:10] for r in rows), 'no case with f hot, the line operands cold'
            assert any(r[12:24] == [0] * 12 and set(r[10:12] + r[24:]) == {hot} and 0 not in r[:10] for r in rows), 'no case with f cold, the line operands hot'
    else:
        zs = {'g1': (2, 7), 'g2': (4, 5, 14, 15)}[kind]
        both_parities(zs, (hot, p, 0, all29))
        for k in zs:
            for e in edges:
                assert any(r[k] == e for r in rows), 'z (Fp position %d) never holds %s' % (k, hex(e))
        assert any(all(v >= P for k, v in enumerate(r) if k not in zs) for r in rows), 'no case with every coordinate in the x + p representative'
        if kind == 'g2':
            assert any(r[4] == r[5] == hot for r in rows) and any(r[14] == r[15] == hot for r in rows), 'no z with both components 2p - 1'


# ---------------------------------------------------------------- runners
def as_array(cases, mapping, op):
    iw = IO[(mapping, op)][0]
    a = np.array(cases, dtype=np.uint32).reshape(len(cases), iw)
    return np.ascontiguousarray(a)


def _ptr(a): return a.ctypes.data_as(C.POINTER(C.c_uint32))


def run_device(lib, mapping, op, ins, device=0):
    ins = as_array(ins, mapping, op)
    out = np.zeros((len(ins), IO[(mapping, op)][1]), dtype=np.uint32)
    rc = lib.zkv_diag_primitive(device, mapping, op, len(ins), _ptr(ins), _ptr(out))
    assert rc == 0, rc
    return out


_HOST = {}


def host_lib(paired):
    """the host build of zkv_selftest.h: tests/host_sim/host_sim_selftest.cpp (mapping 0) or host_sim_selftest_pair.cpp (mappings 1-3)"""
    name = 'host_sim_selftest_pair' if paired else 'host_sim_selftest'
    if name not in _HOST:
        src = os.path.join(HERE, 'host_sim', name + '.cpp')
        lib = os.path.join(HERE, 'host_sim', 'lib%s.so' % name)
        deps = [src] + [os.path.join(CSRC, f) for f in os.listdir(CSRC) if f.endswith('.h')]
        if not os.path.exists(lib) or os.path.getmtime(lib) < max(os.path.getmtime(d) for d in deps):
            subprocess.check_call(['g++', '-O2', '-std=c++17', '-fPIC', '-shared', '-pthread', '-Wno-unknown-pragmas', '-o', lib, src])
        L = C.CDLL(lib)
        L.hs_selftest.argtypes = [C.c_int, C.c_int, C.c_size_t, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)]
        L.hs_selftest_io.argtypes = [C.c_int, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int)]
        _HOST[name] = L
    return _HOST[name]


def run_host(mapping, op, ins):
    ins = as_array(ins, mapping, op)
    out = np.zeros((len(ins), IO[(mapping, op)][1]), dtype=np.uint32)
    assert host_lib(mapping != 0).hs_selftest(mapping, op, len(ins), _ptr(ins), _ptr(out)) == 0
    return out


def cases_for(mapping, op, n, seed):
    rng = random.Random(seed * 1000 + mapping * 10 + op)
    if (mapping, op) in PREDICATE_OPS:
        return predicate_cases(mapping, op, n, rng)
    if (mapping, op) in G2_OPS:
        return g2_group_cases(n, rng) if (mapping, op) == (0, 9) else membership_cases(n, rng) if (mapping, op) == (1, 9) else line_cases(mapping, n, rng)
    if mapping == 0:
        return lane_cases(op, n, rng)
    if mapping == 1:
        return [pair_f2_cases, lincomb_cases, l9mul_cases, f12_cases, cyclo_cases][op](n, rng)
    return [f12_cases, cyclo_cases][op](n, rng)


def check(mapping, op, ins, outs):
    ins = [list(map(int, r)) for r in as_array(ins, mapping, op)]
    outs = [list(map(int, r)) for r in outs]
    if (mapping, op) in PREDICATE_OPS:
        return check_predicates(mapping, op, ins, outs)
    if (mapping, op) in G2_OPS:
        return {(0, 9): check_g2_group, (0, 10): check_lane_lines, (1, 8): check_pair_lines, (1, 9): check_membership,
                (2, 3): lambda i, o: check_wide_lines(i, o, 1), (3, 3): lambda i, o: check_wide_lines(i, o, 4)}[(mapping, op)](ins, outs)
    if mapping == 0:
        return check_lane(op, ins, outs)
    if mapping == 1:
        return [check_pair_f2, check_lincomb, check_l9mul, check_pair_f12, lambda i, o: check_cyclo(i, o, 2)][op](ins, outs)
    return [check_wide_f12, lambda i, o: check_cyclo(i, o, 1)][op](ins, outs)

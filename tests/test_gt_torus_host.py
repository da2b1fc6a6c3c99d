"""The arithmetic of the table walk on torus-compressed entries (csrc/zkv_gt.h, f12l9_mul_aw in csrc/zkv_tower_mem.h), on the spec model's
Fp12 and Python integers: a unitary t = g + h w is stored as a = (1 + g) / h in Fp6, the walk carries u with M = u / conj(u) and multiplies
u by (sign a + w) per window, and the final test FE u == conj(u) stands for FE M == 1.

Plus the stand-alone host program of the walk's body (tests/host_cpp/test_gt_torus.cpp): built and run plain and under AddressSanitizer and
UndefinedBehaviorSanitizer."""
import os
import random
import subprocess

import pytest

import spec_model as m

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, 'tests', 'host_cpp', 'test_gt_torus.cpp')
W_ELT = [0, 1] + [0] * 10                                  # w


def f12inv(a):
    """Inverse in Fp12 by Gaussian elimination on the matrix of x -> a x."""
    cols = [m.f12mul(a, [int(k == j) for k in range(12)]) for j in range(12)]
    M = [[cols[j][i] for j in range(12)] + [int(i == 0)] for i in range(12)]
    for c in range(12):
        p = next(i for i in range(c, 12) if M[i][c])
        M[c], M[p] = M[p], M[c]
        inv = pow(M[c][c], -1, m.P)
        M[c] = [x * inv % m.P for x in M[c]]
        for i in range(12):
            if i != c and M[i][c]:
                f = M[i][c]
                M[i] = [(x - f * y) % m.P for x, y in zip(M[i], M[c])]
    return [M[i][12] for i in range(12)]


def conj(a): return [x if i % 2 == 0 else -x % m.P for i, x in enumerate(a)]
def add(a, b): return [(x + y) % m.P for x, y in zip(a, b)]
def neg(a): return [-x % m.P for x in a]
def is_fp6(a): return not any(a[1::2])                      # Fp6 = the even powers of w (v = w^2)


def compress(t):
    """a = (1 + g) / h for t = g + h w."""
    g = [x if i % 2 == 0 else 0 for i, x in enumerate(t)]
    h = m.f12mul([x if i % 2 else 0 for i, x in enumerate(t)], f12inv(W_ELT))
    assert is_fp6(h) and any(h)
    a = m.f12mul(add(g, m.F12_ONE), f12inv(h))
    assert is_fp6(a)
    return a


def decompress(a):
    return m.f12mul(add(a, W_ELT), f12inv(add(a, neg(W_ELT))))


def step(u, a, sign):
    """u <- u (sign a + w), written out on the halves: N' = sign N a + v D, D' = N + sign a D."""
    sa = a if sign > 0 else neg(a)
    N = [x if i % 2 == 0 else 0 for i, x in enumerate(u)]
    Dw = [x if i % 2 else 0 for i, x in enumerate(u)]
    Dv = m.f12mul(Dw, W_ELT)                                # D w * w = v D
    N2 = add(m.f12mul(N, sa), Dv)
    D2w = add(m.f12mul(N, W_ELT), m.f12mul(Dw, sa))
    out = add(N2, D2w)
    assert is_fp6(N2) and out == m.f12mul(u, add(sa, W_ELT))
    return out


def ratio(u): return m.f12mul(u, f12inv(conj(u)))


@pytest.fixture(scope='module')
def unitary():
    """G (the spec pairing value of the generators, of order R) and 20 seeded powers of it with their exponents."""
    G = m.final_exponentiate(m.miller_loop(m.G2_GEN, m.G1_GEN))
    assert G != m.F12_ONE and m.f12mul(G, conj(G)) == m.F12_ONE
    rng = random.Random(2020)
    exps = [rng.randrange(2, m.R) for _ in range(20)]
    return G, exps, [m.f12pow(G, e) for e in exps]


def test_compress_then_decompress_is_the_identity(unitary):
    _, _, ts = unitary
    for t in ts:
        a = compress(t)
        assert any(a) and decompress(a) == t
        assert decompress(neg(a)) == conj(t)                # t^-1 has the torus value -a


def test_one_step_multiplies_by_the_entry_or_its_inverse(unitary):
    _, _, ts = unitary
    u = m.F12_ONE
    M = m.F12_ONE
    for k, t in enumerate(ts):
        a = compress(t)
        for sign in (1, -1):
            u2 = step(u, a, sign)
            assert any(u2)
            assert ratio(u2) == m.f12mul(M, t if sign > 0 else conj(t))
        u = step(u, a, 1 if k % 3 else -1)                  # go on from a general u, not only from 1
        M = ratio(u)


def test_chain_of_26_steps_and_the_final_test(unitary):
    G, exps, ts = unitary
    rng = random.Random(26)
    u, e = m.F12_ONE, 0
    assert ratio(u) == m.F12_ONE                            # (N, D) = (1, 0)
    for k in range(26):
        sign = rng.choice([1, -1, 0]) if k not in (0, 25) else (-1 if k else 1)      # 0: a lane without a digit keeps u
        if sign:
            u = step(u, compress(ts[k % 20]), sign)
            e += sign * exps[k % 20]
        assert any(u)
    M = ratio(u)
    assert M == m.f12pow(G, e % m.R)
    fe = conj(M)                                            # FE M == 1
    assert m.f12mul(fe, M) == m.F12_ONE and m.f12mul(fe, u) == conj(u)
    bad = m.f12mul(fe, G)                                   # wrong by one factor G
    assert m.f12mul(bad, M) != m.F12_ONE and m.f12mul(bad, u) != conj(u)
    assert m.f12mul(m.F12_ONE, u) != conj(u)                # FE = 1 against M != 1


@pytest.mark.parametrize('flags,name', [([], 'plain'), (['-fsanitize=address,undefined', '-fno-sanitize-recover=all'], 'san')])
def test_walk_body_against_the_packed_product(tmp_path, flags, name):
    """f12l9_mul_aw (the host build of the lane-pair code, two threads playing the pair) against f12m_mul_body by the full element
    (+-a + w), coefficient by coefficient over 1,000 seeded inputs; the program prints the count it compared."""
    exe = str(tmp_path / name)
    subprocess.check_call(['g++', '-std=c++17', '-O1', '-g', '-pthread'] + flags + ['-o', exe, SRC])
    out = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)
    assert out.returncode == 0, (out.stdout.decode()[-2000:], out.stderr.decode()[-2000:])
    assert not out.stderr, out.stderr.decode()[-2000:]
    assert out.stdout.decode().splitlines()[-1] == 'ok 1000 inputs'

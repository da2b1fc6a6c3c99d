"""The table walk on torus-compressed entries (csrc/zkv_gt.h, f12l9_mul_aw) on the device: the product k_finalexp2's walk forms
(zkv_diag_gt_product: u / conj(u) of the u the kernel leaves) against the spec model's powers of e(IC_i, gamma)^K, at n = 66 on lane pairs --
two full wavefronts and two pairs -- for the signal patterns the walk treats specially, and the statuses of 66 rows of the real SP1 proof
with the tables on and off."""
import functools
import random

import numpy as np
import pytest

import spec_model as m

pytestmark = pytest.mark.gpu

H = bytes.fromhex
W = 20
K = 2 * m.U * (6 * m.U * m.U + 3 * m.U + 1)          # the library's final exponentiation computes e(.,.)^K, gcd(K, R) = 1
HARD_K = (m.P ** 4 - m.P ** 2 + 1) // m.R * K
N = 66                                             # 32 proofs per wavefront: two full wavefronts and two pairs
TOP = 1 << 19


@pytest.fixture(scope='module')
def zkv():
    import stylus_zkvm_verifiers_amd as z
    assert z.device_count() >= 1, 'no gfx950 device visible'
    return z


def digits(s, n):
    out = []
    for j in range(n):
        w = (s >> (W * j)) & ((1 << W) - 1)
        c = (s >> (W * j - 1)) & 1 if j else 0
        out.append(w + c - ((w >> 19) << W))
    assert sum(d << (W * j) for j, d in enumerate(out)) == s
    return out


def to_f12(coeffs):
    out = [0] * 12
    for k in range(3):
        for c, e in ((coeffs[k], 2 * k), (coeffs[3 + k], 2 * k + 1)):
            t = m.f2_to_f12(c, e)
            out = [(x + y) % m.P for x, y in zip(out, t)]
    return out


def f12inv(a):
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


@functools.lru_cache(maxsize=None)
def spec_squares(vm):
    """G_i^(2^k), k = 0 .. 20 nw, for the two per-proof signals of the key: G_i = e(IC_i, gamma)^K from the spec model's Miller loop,
    exponentiated as f^(p^6 - 1) = conj(f) / f, then ^(p^2 + 1), then the hard part and K in one power.  Computed once per key."""
    vk, var, nw = (m.SP1_VK, (1, 2), 13) if vm == 'sp1' else (m.RISC0_VK, (3, 4), 7)
    g2 = m.vk_g2_point(vk['gamma2'])
    out = []
    for i in var:
        f = m.miller_loop(g2, vk['ic'][i])
        g = m.f12mul([x if k % 2 == 0 else -x % m.P for k, x in enumerate(f)], f12inv(f))
        g = m.f12mul(m.f12pow(g, m.P * m.P), g)
        t = [m.f12pow(g, HARD_K)]
        for _ in range(W * nw):
            t.append(m.f12mul(t[-1], t[-1]))
        out.append(t)
    return out


def want_product(vm, s0, s1):
    sq = spec_squares(vm)
    want = m.F12_ONE
    for sig, s in ((0, s0), (1, s1)):
        for k in range(s.bit_length()):
            if (s >> k) & 1:
                want = m.f12mul(want, sq[sig][k])
    return want


def built(zkv, monkeypatch, real_proofs, vm, n):
    """A verifier that has verified n copies of the real proof on lane pairs: its tables are built and its workspace holds n proofs."""
    monkeypatch.delenv('ZKV_GT_WINDOW_BITS', raising=False)
    monkeypatch.delenv('ZKV_GT_MAX_BYTES', raising=False)
    s, r = real_proofs['sp1'], real_proofs['risc0']
    if vm == 'sp1':
        v = zkv.Sp1Verifier()
        v.set_lanes_per_proof(2)
        st, _ = v.verify_batch([H(s['vkey'])] * n, [H(s['public_values'])] * n, [H(s['proof'])] * n)
    else:
        v = zkv.RiscZeroVerifier()
        v.initialize(H(r['control_root']), H(r['bn254_control_id']))
        v.set_lanes_per_proof(2)
        st, _ = v.verify_batch([H(r['seal'])] * n, [H(r['image_id'])] * n, [H(r['journal_digest'])] * n)
    assert all(int(x) == 0 for x in st)
    return v


def dense(rng, nw):
    """A signal all of whose nw digits are nonzero."""
    bits = 253 if nw == 13 else 128
    while True:
        s = rng.randrange(1 << (bits - 1), 1 << bits)
        if all(digits(s, nw)):
            return s


def extreme(nw, phase):
    """Digits of magnitude 2^19 in every window but the top one.  A digit of -2^19 (window 2^19, no carry in) hands a carry on, and the next
    window can only answer it with +2^19 (window 2^19 - 1 plus the carry, no carry out), so the two alternate: phase 0 has -2^19 in the even
    windows and +2^19 in the odd ones; phase 1 the other way round from window 1 on, behind a window 0 of 1 (window 0 takes no carry, so it
    cannot be +2^19).  The top window takes the last carry."""
    wins = [(TOP if (j + phase) % 2 == 0 else TOP - 1) for j in range(nw - 1)]
    if phase:
        wins[0] = 1
    s = sum(w << (W * j) for j, w in enumerate(wins))
    d = digits(s, nw)
    assert all(x == (-TOP if (j + phase) % 2 == 0 else TOP) for j, x in enumerate(d[:nw - 1]) if j >= phase) and (not phase or d[0] == 1)
    return s


def batches(vm):
    """Two launches of 66 signal pairs.
      A  wavefront 0: one lane pair (17) with a single nonzero digit, in the top window of signal 1; every other pair all zero
         wavefront 1: one lane pair (32 + 9) all zero, every other pair with all digits of both signals nonzero
         the two pairs of the third: the extreme digits +-2^19, both phases in both positions
      B  wavefront 0: a signal whose first nonzero window differs from lane to lane (pair i: window i mod nw of signal 0; the windows below it
         are skipped by that pair alone), signal 1 likewise from another window, every fourth pair with signal 0 = 0 (its walk starts in signal 1)
         wavefront 1: both signals 0 in every pair -- every window skipped wave-wide, M = 1 through (N, D) = (1, 0)
         the two pairs of the third: (0, 0) and a random pair."""
    nw = 13 if vm == 'sp1' else 7
    rng = random.Random(66 + nw)
    lim = 1 << (253 if nw == 13 else 128)
    a = [(0, 0)] * 32
    a[17] = (0, 5 << (W * (nw - 1)))
    a += [(dense(rng, nw), dense(rng, nw)) for _ in range(32)]
    a[32 + 9] = (0, 0)
    a += [(extreme(nw, 0), extreme(nw, 1)), (extreme(nw, 1), extreme(nw, 0))]
    b = []
    for i in range(32):
        k0, k1 = i % nw, (3 * i + 1) % nw
        s0 = 0 if i % 4 == 3 else ((rng.randrange(lim) >> (W * k0)) | 1) << (W * k0)
        s1 = ((rng.randrange(lim) >> (W * k1)) | 1) << (W * k1)
        d0, d1 = digits(s0, nw), digits(s1, nw)
        assert (s0 == 0 or (not any(d0[:k0]) and d0[k0])) and not any(d1[:k1]) and d1[k1]
        b.append((s0, s1))
    b += [(0, 0)] * 32 + [(0, 0), (rng.randrange(lim), rng.randrange(lim))]
    for rows in (a, b):
        assert len(rows) == N and all(s < 1 << (W * nw - 1) for p in rows for s in p)
    return a, b


@pytest.mark.parametrize('vm', ['sp1', 'risc0'])
def test_walk_product_for_the_special_signal_patterns(zkv, monkeypatch, real_proofs, vm):
    from stylus_zkvm_verifiers_amd import diag_gt
    v = built(zkv, monkeypatch, real_proofs, vm, N)
    try:
        for name, rows in zip('AB', batches(vm)):
            got = [to_f12(x) for x in diag_gt.product(v._h, rows)]
            for i, (s0, s1) in enumerate(rows):
                if s0 == 0 and s1 == 0:
                    assert got[i] == m.F12_ONE, (vm, name, i)          # exactly 1
                else:
                    assert got[i] == want_product(vm, s0, s1), (vm, name, i, hex(s0), hex(s1))
    finally:
        v.close()


def test_statuses_of_the_real_proof_with_tables_on_and_off(zkv, monkeypatch, real_proofs):
    """66 rows of the real SP1 proof, every third with one public-values byte flipped (its signal 1 changes: the proof fails), lane pairs
    forced: the statuses with the tables on and off (ZKV_GT_WINDOW_BITS=0) are identical and are those of the construction."""
    from stylus_zkvm_verifiers_amd import diag_gt
    s = real_proofs['sp1']
    pv = H(s['public_values'])
    rows, want = [], []
    for i in range(N):
        bad = i % 3 == 2
        p = bytearray(pv)
        if bad:
            p[(7 * i) % len(p)] ^= 1 << (i % 8)
        rows.append(bytes(p))
        want.append(1 if bad else 0)
    got = {}
    for bits in (20, 0):
        monkeypatch.setenv('ZKV_GT_WINDOW_BITS', str(bits))
        monkeypatch.delenv('ZKV_GT_MAX_BYTES', raising=False)
        v = zkv.Sp1Verifier()
        v.set_lanes_per_proof(2)
        got[bits] = v.verify_batch([H(s['vkey'])] * N, rows, [H(s['proof'])] * N)
        assert diag_gt.info(v._h)['built'] == (bits == 20)
        v.close()
    assert [int(x) for x in got[20][0]] == want
    assert np.array_equal(got[20][0], got[0][0]) and np.array_equal(got[20][1], got[0][1])

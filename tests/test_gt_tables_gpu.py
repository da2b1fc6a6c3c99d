"""Fixed-base GT tables of the (vk_x, gamma) pairing (csrc/zkv_gt.h, k_gt.hip) on the device: table entries and the folded constant
against the spec model's pairing, the product the final exponentiation kernel forms from them against e(vk_x, gamma) with vk_x from the
ecMul / ecAdd chain, and the statuses of the corpus, of signals >= R and of random signals with the tables on, off (ZKV_GT_WINDOW_BITS=0) and refused
(ZKV_GT_MAX_BYTES) -- SP1, RISC Zero and a mixed batch, lane pairs forced, two full wavefronts and a partial one."""
import random

import numpy as np
import pytest

import spec_model as m

pytestmark = pytest.mark.gpu

H = bytes.fromhex
W = 20
K = 2 * m.U * (6 * m.U * m.U + 3 * m.U + 1)          # the library's final exponentiation computes e(.,.)^K (final_exp_is_one_m), gcd(K, R) = 1
N = 80                                             # lane pairs: 32 proofs per wavefront -> two full wavefronts and one of 16


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
    """six (re, im) pairs g0 g1 g2 h0 h1 h2 -> the spec model's polynomial in w: sum g_k w^(2k) + h_k w^(2k+1)."""
    out = [0] * 12
    for k in range(3):
        for c, e in ((coeffs[k], 2 * k), (coeffs[3 + k], 2 * k + 1)):
            t = m.f2_to_f12(c, e)
            out = [(x + y) % m.P for x, y in zip(out, t)]
    return out


def f12inv_unitary(a):
    return m.f12pow(a, m.R - 1)                      # GT has order R


@pytest.fixture(scope='module')
def spec_gt():
    """e(IC_i, gamma)^K for the per-proof signals of both keys (spec model, computed once)."""
    out = {}
    for name, vk, var in (('sp1', m.SP1_VK, (1, 2)), ('risc0', m.RISC0_VK, (3, 4))):
        g = m.vk_g2_point(vk['gamma2'])
        out[name] = [m.f12pow(m.final_exponentiate(m.miller_loop(g, vk['ic'][i])), K) for i in var]
    return out


def make_sp1(zkv, monkeypatch, bits=None, max_bytes=None):
    if bits is not None:
        monkeypatch.setenv('ZKV_GT_WINDOW_BITS', str(bits))
    if max_bytes is not None:
        monkeypatch.setenv('ZKV_GT_MAX_BYTES', str(max_bytes))
    v = zkv.Sp1Verifier()
    v.set_lanes_per_proof(2)
    return v


def sp1_rows(real_proofs, verify_corpus):
    """N rows: the corpus, proofs whose vkey is >= R, and the real proof under random vkeys and public values (every one must reject)."""
    s = real_proofs['sp1']
    rng = random.Random(7)
    sc = [c for c in verify_corpus['cases'] if c['vm'] == 'sp1']
    rows = [(H(c['vkey']), H(c['public_values']), H(c['proof']), c['status']) for c in sc]
    rows += [(m.be32(x), H(s['public_values']), H(s['proof']), 1) for x in (m.R, m.R + 1, (1 << 256) - 1)]
    while len(rows) < N:
        good = len(rows) % 5 == 0
        rows.append((H(s['vkey']), H(s['public_values']), H(s['proof']), 0) if good else
                    (m.be32(rng.randrange(m.R)), rng.randbytes(rng.randrange(1, 90)), H(s['proof']), 1))
    rng.shuffle(rows)
    return rows[:N]


def risc0_rows(real_proofs, verify_corpus):
    r = real_proofs['risc0']
    rng = random.Random(8)
    rc = [c for c in verify_corpus['cases'] if c['vm'] == 'risc0']
    rows = [(H(c['seal']), H(c['image_id']), H(c['journal_digest']), c['status']) for c in rc]
    while len(rows) < N:
        good = len(rows) % 5 == 0
        rows.append((H(r['seal']), H(r['image_id']), H(r['journal_digest']), 0) if good else (H(r['seal']), rng.randbytes(32), rng.randbytes(32), 1))
    rng.shuffle(rows)
    return rows[:N]


def test_info_and_switch(zkv, monkeypatch, real_proofs, verify_corpus):
    from stylus_zkvm_verifiers_amd import diag_gt
    rows = sp1_rows(real_proofs, verify_corpus)
    v = make_sp1(zkv, monkeypatch)
    st_on, rv_on = v.verify_batch([r[0] for r in rows], [r[1] for r in rows], [r[2] for r in rows])
    info = diag_gt.info(v._h)
    print('sp1 tables:', info)
    assert info['built'] and info['windows'] == (13, 13) and info['bytes'] == 26 * (1 << 19) * 384
    v.close()
    v = make_sp1(zkv, monkeypatch, bits=0)
    st_off, rv_off = v.verify_batch([r[0] for r in rows], [r[1] for r in rows], [r[2] for r in rows])
    info = diag_gt.info(v._h)
    assert not info['built'] and info['tried']
    v.close()
    assert [int(x) for x in st_off] == [r[3] for r in rows]
    assert np.array_equal(st_on, st_off) and np.array_equal(rv_on, rv_off)


def test_risc0_statuses_identical(zkv, monkeypatch, real_proofs, verify_corpus):
    from stylus_zkvm_verifiers_amd import diag_gt
    r = real_proofs['risc0']
    rows = risc0_rows(real_proofs, verify_corpus)
    got = {}
    for bits in (20, 0):
        monkeypatch.setenv('ZKV_GT_WINDOW_BITS', str(bits))
        v = zkv.RiscZeroVerifier()
        v.initialize(H(r['control_root']), H(r['bn254_control_id']))
        v.set_lanes_per_proof(2)
        got[bits] = v.verify_batch([x[0] for x in rows], [x[1] for x in rows], [x[2] for x in rows])
        info = diag_gt.info(v._h)
        assert info['built'] == (bits == 20) and (not info['built'] or info['windows'] == (7, 7))
        v.close()
    assert [int(x) for x in got[0][0]] == [x[3] for x in rows]
    assert np.array_equal(got[20][0], got[0][0]) and np.array_equal(got[20][1], got[0][1])


def test_mixed_statuses_identical(zkv, monkeypatch, real_proofs, verify_corpus):
    r = real_proofs['risc0']
    a, b = sp1_rows(real_proofs, verify_corpus), risc0_rows(real_proofs, verify_corpus)
    rows = [(1, x[2], x[0], x[1], x[3]) for x in a] + [(0, x[0], x[1], x[2], x[3]) for x in b]
    random.Random(9).shuffle(rows)
    got = {}
    for bits in (20, 0):
        monkeypatch.setenv('ZKV_GT_WINDOW_BITS', str(bits))
        mx = zkv.MixedVerifier(H(r['control_root']), H(r['bn254_control_id']), 0)
        mx.set_lanes_per_proof(2)
        got[bits] = mx.verify_batch([x[0] for x in rows], [x[1] for x in rows], [x[2] for x in rows], [x[3] for x in rows])
        mx.close()
    assert [int(x) for x in got[0][0]] == [x[4] for x in rows]
    assert np.array_equal(got[20][0], got[0][0]) and np.array_equal(got[20][1], got[0][1])


@pytest.mark.parametrize('vm', ['sp1', 'risc0', 'mixed'])
def test_fallback_without_room_for_the_tables(zkv, monkeypatch, real_proofs, verify_corpus, vm):
    """A context that may not take the tables' memory (ZKV_GT_MAX_BYTES below their size) keeps the Miller path and verifies the corpus.
    (The branch that frees a partial allocation after a failing hipMalloc has no test: nothing here can make the device run out.)"""
    from stylus_zkvm_verifiers_amd import diag_gt
    monkeypatch.setenv('ZKV_GT_MAX_BYTES', str(1 << 30))
    r = real_proofs['risc0']
    if vm == 'sp1':
        rows = sp1_rows(real_proofs, verify_corpus)
        v = make_sp1(zkv, monkeypatch)
        cols = [[x[k] for x in rows] for k in range(3)]
    elif vm == 'risc0':
        rows = risc0_rows(real_proofs, verify_corpus)
        v = zkv.RiscZeroVerifier()
        v.initialize(H(r['control_root']), H(r['bn254_control_id']))
        v.set_lanes_per_proof(2)
        cols = [[x[k] for x in rows] for k in range(3)]
    else:
        a, b = sp1_rows(real_proofs, verify_corpus), risc0_rows(real_proofs, verify_corpus)
        rows = [(1, x[2], x[0], x[1], x[3]) for x in a] + [(0, x[0], x[1], x[2], x[3]) for x in b]
        random.Random(9).shuffle(rows)
        v = zkv.MixedVerifier(H(r['control_root']), H(r['bn254_control_id']), 0)
        v.set_lanes_per_proof(2)
        cols = [[x[k] for x in rows] for k in range(4)]
    st, _ = v.verify_batch(*cols)
    if vm != 'mixed':
        info = diag_gt.info(v._h)
        assert info['tried'] and not info['built'] and info['bytes'] == 0
    v.close()
    assert [int(x) for x in st] == [x[-1] for x in rows]


def test_window_bits_other_than_0_and_20_are_refused(zkv, monkeypatch, real_proofs):
    s = real_proofs['sp1']
    v = make_sp1(zkv, monkeypatch, bits=16)
    with pytest.raises(Exception):
        v.verify_batch([H(s['vkey'])], [H(s['public_values'])], [H(s['proof'])])
    v.close()


def _built(zkv, monkeypatch, real_proofs, vm, n=1):
    """A verifier that has verified n copies of the real proof on lane pairs: its tables are built and its workspace holds n proofs."""
    s, r = real_proofs['sp1'], real_proofs['risc0']
    if vm == 'sp1':
        v = make_sp1(zkv, monkeypatch)
        st, _ = v.verify_batch([H(s['vkey'])] * n, [H(s['public_values'])] * n, [H(s['proof'])] * n)
    else:
        v = zkv.RiscZeroVerifier()
        v.initialize(H(r['control_root']), H(r['bn254_control_id']))
        v.set_lanes_per_proof(2)
        st, _ = v.verify_batch([H(r['seal'])] * n, [H(r['image_id'])] * n, [H(r['journal_digest'])] * n)
    assert all(int(x) == 0 for x in st)
    return v


@pytest.mark.parametrize('vm', ['sp1', 'risc0'])
def test_table_entries_against_the_spec_pairing(zkv, monkeypatch, real_proofs, spec_gt, vm):
    from stylus_zkvm_verifiers_amd import diag_gt
    v = _built(zkv, monkeypatch, real_proofs, vm)
    nw = diag_gt.info(v._h)['windows']
    rng = random.Random(11)
    for sig in (0, 1):
        G = spec_gt[vm][sig]
        for win in (0, nw[sig] - 1, rng.randrange(1, nw[sig] - 1)):
            for d in [1, 2, (1 << 19) - 1, 1 << 19] + [rng.randrange(3, 1 << 19) for _ in range(3)]:
                got = to_f12(diag_gt.read(v._h, sig, win, d))
                assert got == m.f12pow(G, (d << (W * win)) % m.R), (vm, sig, win, d)
    v.close()


def base_point(vm, real_proofs):
    """(key, the fixed part of vk_x, a function from the two per-proof signals to the key's full signal list)."""
    if vm == 'sp1':
        return m.SP1_VK, m.SP1_VK['ic'][0], lambda s0, s1: [s0, s1]
    r = real_proofs['risc0']
    rv = m.Risc0Verifier()
    assert rv.initialize(H(r['control_root']), H(r['bn254_control_id'])) == m.OK
    fixed = rv.signals(bytes(32))
    full = lambda s0, s1: fixed[:2] + [s0, s1] + fixed[4:]
    return m.RISC0_VK, m.compute_vk_x(m.RISC0_VK, full(0, 0)), full


@pytest.mark.parametrize('vm', ['sp1', 'risc0'])
def test_folded_constant_against_the_spec_pairing(zkv, monkeypatch, real_proofs, vm):
    """FE(ML(alpha, beta) ML(base, gamma)) = e(alpha, beta) e(base, gamma); base is IC0 for SP1 and IC0 plus the control-root and
    control-id terms (the spec model's fixed signals through its G1 arithmetic) for RISC Zero."""
    from stylus_zkvm_verifiers_amd import diag_gt
    v = _built(zkv, monkeypatch, real_proofs, vm)
    got = m.final_exponentiate(to_f12(diag_gt.read(v._h, -1)))
    v.close()
    vk, base, _ = base_point(vm, real_proofs)
    assert (base == vk['ic'][0]) == (vm == 'sp1')
    want = m.final_exponentiate(m.f12mul(m.miller_loop(m.vk_g2_point(vk['beta2']), vk['alpha1']), m.miller_loop(m.vk_g2_point(vk['gamma2']), base)))
    assert got == want


def f12inv(a):
    """Inverse in Fp12 by Gaussian elimination on the matrix of x -> a x (columns a w^j)."""
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


HARD_K = (m.P ** 4 - m.P ** 2 + 1) // m.R * K


def pairing_k(f):
    """final_exponentiate(f)^K in a third of the time: f^(p^6 - 1) = conj(f) / f (p^6 is w -> -w), then ^(p^2 + 1), then the hard part
    and K in one power.  Checked against the spec model's own final exponentiation in the test below."""
    g = m.f12mul([x if i % 2 == 0 else -x % m.P for i, x in enumerate(f)], f12inv(f))
    g = m.f12mul(m.f12pow(g, m.P * m.P), g)
    return m.f12pow(g, HARD_K)


def edge_signals(nw):
    """The edge signals of the recoding test, for a signal of nw windows (below 2^(20 (nw - 1) + 8)): digits 0, +-1, +-(2^19 - 1), -2^19,
    +2^19 (a window of 2^19 - 1 with a carry in), a run of windows that all carry, and the largest signal."""
    run = sum(((1 << 19) + 5) << (W * j) for j in range(nw - 1))
    top = m.R - 1 if nw == 13 else (1 << 128) - 1
    return [0, 1, (1 << 19) - 1, 1 << 19, (1 << 19) + 1, (1 << 20) - 1, (((1 << 19) - 1) << W) | (1 << 19), run, top]


@pytest.mark.parametrize('vm', ['sp1', 'risc0'])
def test_product_the_kernel_forms_is_the_pairing_of_vk_x(zkv, monkeypatch, real_proofs, spec_gt, vm):
    """The product M that k_finalexp2's own table walk forms (zkv_diag_gt_product: the verify path's kernel on proofs whose Miller value is
    1) for N = 80 signal pairs in one launch -- two full wavefronts and one of 16 lane pairs:
      wavefront 0: signal 0 below 2^59 in every lane, so its windows 3 and up are zero in the whole wavefront (the wave-wide skip);
      wavefronts 1, 2: the edge signals in both positions among random ones (zero, positive and negative digits mixed in a wavefront).
    Every M equals G_0^s0 G_1^s1 with G_i the spec model's e(IC_i, gamma)^K; and for the 9 edge rows and 24 random rows, M e(base, gamma)^K
    equals e(vk_x, gamma)^K with vk_x from compute_vk_x (the ecMul / ecAdd chain) and the spec model's Miller loop."""
    from stylus_zkvm_verifiers_amd import diag_gt
    nw = 13 if vm == 'sp1' else 7
    lim = (m.R, 1 << 253) if vm == 'sp1' else (1 << 128, 1 << 128)
    rng = random.Random(13)
    E = edge_signals(nw)
    pairs = [(rng.choice([0, 1, rng.randrange(1 << 59)]), rng.randrange(lim[1])) for _ in range(32)]
    tail = [(rng.randrange(lim[0]), rng.randrange(lim[1])) for _ in range(N - 32 - len(E))]
    edge = [(E[k], E[(k + 4) % len(E)]) for k in range(len(E))]
    rest = tail + edge
    rng.shuffle(rest)
    pairs += rest
    assert len(pairs) == N and all(s < 1 << (W * nw - 1) for p in pairs for s in p)
    chained = set(pairs.index(p) for p in edge) | set(rng.sample(range(N), 24))

    v = _built(zkv, monkeypatch, real_proofs, vm, n=N)
    got = [to_f12(x) for x in diag_gt.product(v._h, pairs)]
    v.close()

    sq = []                                            # G_i^(2^k)
    for G in spec_gt[vm]:
        t = [G]
        for _ in range(W * nw):
            t.append(m.f12mul(t[-1], t[-1]))
        sq.append(t)
    for i, (s0, s1) in enumerate(pairs):
        want = m.F12_ONE
        for sig, s in ((0, s0), (1, s1)):
            for k in range(s.bit_length()):
                if (s >> k) & 1:
                    want = m.f12mul(want, sq[sig][k])
        assert got[i] == want, (vm, i, hex(s0), hex(s1))

    vk, base, full = base_point(vm, real_proofs)
    g = m.vk_g2_point(vk['gamma2'])
    ml = m.miller_loop(g, base)
    e_base = pairing_k(ml)
    assert e_base == m.f12pow(m.final_exponentiate(ml), K)              # the shortened exponentiation is the spec model's
    for i in sorted(chained):
        vkx = m.compute_vk_x(vk, full(*pairs[i]))
        assert m.f12mul(got[i], e_base) == pairing_k(m.miller_loop(g, vkx)), (vm, i, [hex(s) for s in pairs[i]])

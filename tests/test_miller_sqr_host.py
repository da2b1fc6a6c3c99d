"""The Fp12 squaring of the lane-pair Miller loop as six direct column sums over the powers of w (csrc/zkv_tower_mem.h
f12m_sqr_fused_body, csrc/zkv_field.h f2_sum_open / f2_sum_cross / f2_sum_cross_dbl / f2_sum_sqr / f2_sum_close and the doubling carry
pass fp_cols_carry32_dbl) against the complex-squaring Karatsuba form it replaced (f12m_sqr_karatsuba_body), in the host emulation of
a lane pair (tests/host_sim/host_sim_sqr.cpp).  CPU only.

The host build forms every update of a 64-bit column again in 128 bits and counts the updates that differ, and the operands of every
piece that leave their contract (ZKV_SHADOW_COLS): the range argument written above f12m_sqr_fused_body -- two products, the carry pass
that doubles, then a square and a product or a product on doubled limbs, one reduction -- is checked where it is tightest."""
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
XI = (9, 1)
SQUARINGS = 64                      # doubling steps of the optimal-ate loop after step 0
EXCESS = 933                        # multiply-adds a lane and squaring beyond the Karatsuba charge: 3,849 - 2,916
FUSED_MADS = 39 * 81 + 6 * 81 + 6 * 2 * 17


def _build(name, extra):
    src = os.path.join(HERE, 'host_sim', 'host_sim_sqr.cpp')
    lib = os.path.join(HERE, 'host_sim', name)
    csrc = os.path.join(HERE, '..', 'stylus_zkvm_verifiers_amd', 'csrc')
    deps = [src] + [os.path.join(csrc, f) for f in os.listdir(csrc) if f.endswith('.h')]
    if not os.path.exists(lib) or os.path.getmtime(lib) < max(os.path.getmtime(d) for d in deps):
        subprocess.check_call(['g++', '-O2', '-std=c++17', '-fPIC', '-shared', '-pthread', '-Wno-unknown-pragmas'] + extra + ['-o', lib, src])
    L = C.CDLL(lib)
    L.hsq_squarings.argtypes = [C.c_int] + [C.c_void_p] * 6
    L.hsq_miller.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    L.hsq_miller.restype = C.c_ulonglong
    return L


@pytest.fixture(scope='module')
def hq():
    return _build('libhost_sim_sqr.so', [])


@pytest.fixture(scope='module')
def hq_karatsuba():
    """The same emulation with the loop's squaring switched back to the Karatsuba body."""
    return _build('libhost_sim_sqr_karatsuba.so', ['-DZKV_SQR_KARATSUBA'])


def _run(hq, cases):
    """cases: lists of 12 integers (f as g0 g1 g2 h0 h1 h2; real part, imaginary part).  Returns per case the canonical outputs of the
    two bodies, the column-check counters, the loose-range flags, the multiply-add counters and the Fp products charged."""
    n = len(cases)
    buf = b''.join(v.to_bytes(32, 'little') for c in cases for v in c)
    assert len(buf) == n * 96 * 4
    out = C.create_string_buffer(n * 2 * 96 * 4)
    shadow = (C.c_ulonglong * 4)(); loose = (C.c_int * 2)(); mads = (C.c_ulonglong * 6)(); muls = (C.c_ulonglong * 2)()
    assert hq.hsq_squarings(n, buf, out, shadow, loose, mads, muls) == 2
    res = []
    for i in range(n):
        per = []
        for b in range(2):
            o = (i * 2 + b) * 384
            per.append([int.from_bytes(out.raw[o + 32 * k: o + 32 * k + 32], 'little') for k in range(12)])
        res.append(per)
    return res, [int(x) for x in shadow], [int(x) for x in loose], [int(x) for x in mads], [int(x) for x in muls]


def _check(hq, cases):
    res, shadow, loose, _, _ = _run(hq, cases)
    for i, per in enumerate(res):
        assert per[0] == per[1], (i, [hex(v) for v in cases[i]])           # coefficient by coefficient, as field elements
        assert all(v < P for v in per[0])
    for b in range(2):
        assert shadow[2 * b] > 0 and shadow[2 * b + 1] == 0, (b, shadow)   # no column left its 128-bit value, no operand its contract
        assert loose[b] == 1, b                                            # every output below 2p
    return res


def _f2_mul(a, b):
    return ((a[0] * b[0] - a[1] * b[1]) % P, (a[0] * b[1] + a[1] * b[0]) % P)


def _model_sqr(c):
    """f^2 by the schoolbook convolution over the powers of w, on the Montgomery-domain integers of a case; canonical outputs."""
    rinv = pow(R261, -1, P)
    slot = (0, 3, 1, 4, 2, 5)                                              # slot of the coefficient of w^k
    a = [((c[2 * slot[k]] * rinv) % P, (c[2 * slot[k] + 1] * rinv) % P) for k in range(6)]
    out = [(0, 0)] * 6
    for i in range(6):
        for j in range(6):
            t = _f2_mul(a[i], a[j])
            if i + j >= 6:
                t = _f2_mul(t, XI)
            k = (i + j) % 6
            out[k] = ((out[k][0] + t[0]) % P, (out[k][1] + t[1]) % P)
    flat = [0] * 12
    for k in range(6):
        flat[2 * slot[k]], flat[2 * slot[k] + 1] = out[k]
    return flat


def _cases():
    one = R261
    cases = [[0] * 12,
             [one] + [0] * 11, [one + P] + [P] * 11,                       # f = 1 in both representatives
             [1] * 12,
             [P - 1] * 12,
             [2 * P - 1] * 12]                                             # the largest reduced value
    top = (2 * P - 1) >> 232
    vmax = (top << 232) - 1                                                # limbs 0 .. 7 all ones below 2p
    assert vmax < 2 * P
    cases += [[vmax] * 12, [vmax, 0] * 6, [0, vmax] * 6]
    for e in (1, P - 1, 2 * P - 1, vmax):                                  # single non-zero coefficients, and single components
        for s in range(6):
            c = [0] * 12; c[2 * s] = c[2 * s + 1] = e; cases.append(c)
            c = [0] * 12; c[2 * s] = e; cases.append(c)
            c = [0] * 12; c[2 * s + 1] = e; cases.append(c)
    return cases


def test_fused_squaring_equals_karatsuba_on_edges(hq):
    cases = _cases()
    res = _check(hq, cases)
    assert all(v == 0 for v in res[0][0])
    assert res[1][0] == [pow(R261, -1, P) * R261 % P] + [0] * 11 == res[2][0]      # 1^2 = 1
    for c, per in zip(cases, res):
        assert per[0] == _model_sqr(c)


def test_fused_squaring_equals_karatsuba_on_random_values(hq):
    """256 seeded random values anywhere in the loose range, and against the plain convolution."""
    rng = random.Random(0x5152)
    cases = [[rng.randrange(2 * P) for _ in range(12)] for _ in range(256)]
    res = _check(hq, cases)
    for c, per in zip(cases[:16], res[:16]):
        assert per[0] == _model_sqr(c)


def test_column_check_and_counters_per_squaring(hq):
    """The 128-bit check sees every update: per lane 39 column products of 81, six doubling carry passes of 17, six reductions of 81
    products and 17 carries.  The counters: a squaring is CHARGED what the Karatsuba form is (2,916 multiply-adds and 24 Fp products a
    lane), zkv_mad_issued_counter moves with the charge, and the 933 it issues beyond it are in zkv_sqr_mad_excess_counter."""
    n = 3
    _, shadow, _, mads, muls = _run(hq, [[1] * 12] * n)
    assert shadow[0] == 2 * n * (39 * 81 + 6 * 17 + 6 * (81 + 17)) and shadow[1] == 0
    charged_f, issued_f, excess_f, charged_k, issued_k, excess_k = mads
    assert charged_k == issued_k == 2 * n * 12 * 243 and excess_k == 0
    assert charged_f == charged_k and issued_f == charged_f
    assert excess_f == 2 * n * EXCESS and FUSED_MADS - 12 * 243 == EXCESS
    assert muls[0] == muls[1] == 2 * n * 24


from test_kernel_math_host import hs  # noqa: E402,F401  (the one-value-per-lane host build: its fixture, not a copy of its recipe)

FL_A_INF, FL_B_INF, FL_C_INF, FL_L_INF = 2, 4, 8, 16


def test_miller_loop_equals_loop_with_karatsuba_squaring(hq, hq_karatsuba, hs, real_proofs):
    """The flat loop the kernels run, on the two real proofs (and with the variable pair, or a fixed pair, switched off): the accumulator
    after the loop is the same field element, coefficient by coefficient, whichever body squares it; no column update differs from its
    128-bit form; the squarings report their excess -- 64 of them, both lanes -- and the Karatsuba loop none."""
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
        for extra in (0, FL_A_INF, FL_C_INF, FL_L_INF):
            flags = fl.value | extra
            got = (C.c_uint32 * 96)(); want = (C.c_uint32 * 96)()
            ops = (C.c_ulonglong * 2)(); kops = (C.c_ulonglong * 2)()
            assert hq.hsq_miller(t, flags, norm, b, got, ops) == 0, extra
            assert hq_karatsuba.hsq_miller(t, flags, norm, b, want, kops) == 0, extra
            assert list(got) == list(want), extra
            assert any(got) and ops[0] > 0
            assert ops[1] == 2 * SQUARINGS * EXCESS and kops[1] == 0


U = 4965661367192848881                               # the BN parameter: p = 36 u^4 + 36 u^3 + 24 u^2 + 6 u + 1


def test_start_exponent(hq):
    """e = (2^64 h)^-1 mod r with h = k (p^12 - 1) / r, k = 2u (6u^2 + 3u + 1), the exponent the final exponentiation applies: the header's
    constants are those, 2^64 h is invertible mod r, and the host's own assertion (miller_start_exponent_ok) says the same."""
    R = m.R
    assert P == 36 * U**4 + 36 * U**3 + 24 * U**2 + 6 * U + 1 and R == 36 * U**4 + 36 * U**3 + 18 * U**2 + 6 * U + 1
    assert (P**12 - 1) % R == 0
    h = 2 * U * (6 * U * U + 3 * U + 1) * ((P**12 - 1) // R)
    assert ((1 << 64) * h) % R != 0
    e = pow((1 << 64) * h, -1, R)
    hr = (C.c_uint32 * 8)(); ex = (C.c_uint32 * 8)()
    hq.hsq_start_exponent.argtypes = [C.c_void_p, C.c_void_p]
    bits = hq.hsq_start_exponent(hr, ex)
    assert bits == e.bit_length()
    assert sum(v << (32 * i) for i, v in enumerate(hr)) == h % R
    assert sum(v << (32 * i) for i, v in enumerate(ex)) == e
    assert (e * (1 << 64) * h) % R == 1


def test_start_value_on_both_keys(hq, hs, real_proofs):
    """For both hard-coded keys, with m the key's Miller constant and c = FE(m)^e: FE(c^(2^64)) equals FE(m); and the loop started from c
    followed by the final exponentiation gives the same verdict and the same GT value as the loop started from 1, times m, followed by
    it -- on the real proof (accepted) and with the C pair switched off (rejected)."""
    hs.hs_prepare.restype = C.c_void_p
    hq.hsq_start_value.argtypes = [C.c_void_p, C.c_uint32] + [C.c_void_p] * 4
    r0, s = real_proofs['risc0'], real_proofs['sp1']
    cr, cid = H(r0['control_root']), H(r0['bn254_control_id'])
    v = m.Risc0Verifier(); v.initialize(cr, cid)
    sig = v.signals(m.receipt_claim_ok_digest(H(r0['image_id']), H(r0['journal_digest'])))
    cases = [(0, cr, cid, H(r0['seal'])[4:], m.be32(sig[2]), m.be32(sig[3])),
             (1, None, None, H(s['proof'])[4:], H(s['vkey']), m.be32(m.sp1_hash_public_values(H(s['public_values']))))]
    consts = []
    for args in cases:
        fl = C.c_uint32(0); norm = (C.c_uint32 * 48)(); b = (C.c_uint32 * 32)()
        t = hs.hs_prepare(*args, C.byref(fl), norm, b)
        assert t
        for extra, accepted in ((0, 1), (FL_C_INF, 0)):
            out = (C.c_uint32 * (4 * 96))(); verdict = (C.c_int * 2)()
            assert hq.hsq_start_value(t, fl.value | extra, norm, b, out, verdict) == 1
            fe_m, fe_c, gt_one, gt_start = (list(out[96 * k: 96 * k + 96]) for k in range(4))
            assert fe_m == fe_c and any(fe_m[8:])                      # FE(c^(2^64)) == FE(m), and not the identity
            assert gt_one == gt_start
            assert list(verdict) == [accepted, accepted]
        consts.append(fe_m)
    assert consts[0] != consts[1]                                      # two keys, two constants

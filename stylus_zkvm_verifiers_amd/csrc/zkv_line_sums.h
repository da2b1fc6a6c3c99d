// Tangent and chord steps of the running point B of the lane-pair Miller loop as fused column sums.
//
// line_dbl / line_add (zkv_curve.h) give every Fp2 product and square its own reduction and pack, and join them with packed additions,
// subtractions, doublings and halvings: carry chains, each with the wait state a VCC-chained add needs on gfx950.  The bodies below
// compute the same field elements by the same homogeneous formulas -- the same T.x, T.y, T.z and the same line l0 + l1 xP w + l3 yP w^3,
// in the same scaling -- from the sum pieces of zkv_field.h (f2_sum_open / f2_sum_cross / f2_sum_cross_dbl / f2_sum_sqr):
//   * a value that only feeds further products stays on its nine 29-bit limbs as the reduction leaves them (limbs 0 .. 7 below 2^29,
//     value below 2p): no pack, no unpack;
//   * a small-integer combination (3e, b - 3e, (b + 3e)/2, e + f - 2g, 3g - e - f) is formed limb by limb on 32-bit limbs and
//     carried to normalised limbs in one pass of shifts (limbs_carry, limbs_carry_signed): no carry chain;
//   * a difference of two products is ONE column sum with one reduction, the subtrahend entering through the negated multiplier form
//     (limbs_y_neg: 8p - x on the components where the positive form holds x);
//   * the line coefficients leave scaled, c3 = l1 xs and c4 = l3 ys (xs = xP/yP, ys = 1/yP of the G1 point), because l1 and l3 have no other
//     reader: their scaling is one 81-term product from the limbs at hand, and l1, l3 themselves are never packed.
// Z = 0 stays absorbing: T.z is still b h = 2 Y^3 Z in the tangent step and Z e = Z lambda^3 in the chord step, as field elements.
// line_dbl and line_add remain the independent check (tests/host_sim/host_sim_line_steps.cpp) and the path of every kernel that is not
// a lane-pair Miller kernel.
//
// Units of 2^58 a column (a column holds 64; the reduction adds 9), even lane | odd lane, for operands with limbs below 2^29:
//   product (f2_sum_cross)                         27 | 18      value at most (4 + 16) p^2 for reduced operands
//   negated product (f2_sum_cross_neg)             27 | 36
//   product on doubled multiplicand limbs          54 | 36
//   square (f2_sum_sqr, M below 2^30)              18 | 18
// Every sum below states its total and its value bound (the reduction takes values below 169 p^2).
#pragma once
#include "zkv_tower_mem.h"

#if defined(ZKV_PAIRED)
#if defined(ZKV_COUNT_FP_MUL)
// What the two bodies issue beyond the charge of the forms they replace (which zkv_mad_counter, zkv_mad_issued_counter and zkv_fp_mul_counter
// keep receiving, so that tests/golden/stage_mul_counts.json and the difference pinned by tests/test_miller_var_line_host.py stay what they
// are): +16 a lane for a tangent step (2,284 against 2,268 with the two scalings: the two tripling carry passes), -162 a lane for a chord
// step (3,159 against 3,321).  Signed.  tests/test_miller_line_steps_host.py pins both.
static thread_local long long zkv_line_mad_excess_counter = 0;
#endif

namespace zkv {

ZKV_HD void limbs_partner(const uint32_t (&a)[9], uint32_t (&p)[9]) {
#pragma unroll
    for (int i = 0; i < 9; i++) p[i] = zkv_partner_u32(a[i]);
}
// Lazy limbs -> normalised limbs (0 .. 7 below 2^29, the rest in limb 8) in one pass of shifts, no carry chain.  limbs_carry: limbs that
// are not negative, any 32-bit size; limbs_carry_signed: signed limbs of a value that is not negative, |limb| below 2^31 - 2^3 (a limb
// and the carry of the one below stay inside 32 bits).  A top limb that is negative before its carry arrives wraps and comes out right.
ZKV_HD void limbs_carry(uint32_t (&a)[9]) {
#pragma unroll
    for (int k = 0; k < 8; k++) { a[k + 1] += a[k] >> 29; a[k] &= 0x1fffffffu; }
}
ZKV_HD void limbs_carry_signed(uint32_t (&a)[9]) {
#pragma unroll
    for (int k = 0; k < 8; k++) { a[k + 1] += (uint32_t)((int32_t)a[k] >> 29); a[k] &= 0x1fffffffu; }
}
// a <- 3 a, normalised: limbs 0 .. 7 not negative; one multiply-add, one mask and one shift a limb (counted as issued).
ZKV_HD void limbs_carry_x3(uint32_t (&a)[9]) {
    ZKV_COUNT_MADS_ISSUED(8);
    uint32_t c = 0;
#pragma unroll
    for (int k = 0; k < 8; k++) { const uint64_t t = (uint64_t)a[k] * 3u + c; a[k] = (uint32_t)t & 0x1fffffffu; c = (uint32_t)(t >> 29); }
    a[8] = a[8] * 3u + c;
}
// k p in a borrow-free form: limbs 0 .. 7 in [lift * 2^29 - lift, (lift + 1) * 2^29), so that F - x has no negative limb below the top one
// for limb-wise x below lift * 2^29 - lift + 1 (ZKV_FP_FAT8P_LIMBS is this form of 8p with lift 1).  Constants: folded by the compiler.
template <int K, int LIFT> ZKV_HD void limbs_kp_fat(uint32_t (&F)[9]) {
    const uint32_t P29[9] = ZKV_FP_P29_LIMBS;
#pragma unroll
    for (int i = 0; i < 9; i++) F[i] = (uint32_t)K * P29[i];
    limbs_carry(F);
#pragma unroll
    for (int i = 0; i < 9; i++) F[i] += (i < 8 ? (uint32_t)LIFT << 29 : 0u) - (i > 0 ? (uint32_t)LIFT : 0u);
}
// a <- (a + (a odd ? p : 0)) / 2 on lazy limbs, normalised on return.  The parity of the value is the parity of limb 0.
template <bool SIGNED> ZKV_HD void limbs_half_carry(uint32_t (&a)[9]) {
    const uint32_t P29[9] = ZKV_FP_P29_LIMBS;
    const uint32_t m = 0u - (a[0] & 1u);
#pragma unroll
    for (int i = 0; i < 9; i++) a[i] += P29[i] & m;
    if (SIGNED) limbs_carry_signed(a);
    else limbs_carry(a);
#pragma unroll
    for (int k = 0; k < 8; k++) a[k] = (a[k] >> 1) | ((a[k + 1] & 1u) << 28);
    a[8] >>= 1;
}
// Multiplier forms from normalised limbs y of this lane's component (value below 8p): positive as f2_limbs_y, without the unpack; negated
// so that a product taken with it is -(a y): U = 8p - y0 in both lanes, V = y1 in the even lane and 8p - y1 in the odd one.
ZKV_HD void limbs_y(const uint32_t (&y)[9], uint32_t (&U)[9], uint32_t (&V)[9]) {
    const uint32_t FAT[9] = ZKV_FP_FAT8P_LIMBS;
    const bool even = zkv_parity() == 0;
#pragma unroll
    for (int i = 0; i < 9; i++) { U[i] = zkv_pair_even_u32(y[i]); const uint32_t v = zkv_pair_odd_u32(y[i]); V[i] = even ? FAT[i] - v : v; }
}
ZKV_HD void limbs_y_neg(const uint32_t (&y)[9], uint32_t (&U)[9], uint32_t (&V)[9]) {
    const uint32_t FAT[9] = ZKV_FP_FAT8P_LIMBS;
    const bool even = zkv_parity() == 0;
#pragma unroll
    for (int i = 0; i < 9; i++) { U[i] = FAT[i] - zkv_pair_even_u32(y[i]); const uint32_t v = zkv_pair_odd_u32(y[i]); V[i] = even ? v : FAT[i] - v; }
}
// - a b from the negated multiplier form: multiplicand limbs below 2^29, U below 2^30, V below 2^30.  27 | 36 units.
ZKV_HD void f2_sum_cross_neg(uint64_t (&col)[18], const uint32_t (&ao)[9], const uint32_t (&ap)[9], const uint32_t (&nU)[9], const uint32_t (&nV)[9]) {
#if defined(ZKV_COUNT_FP_MUL)
    zkv_fp_mul_counter += 2;
#endif
    ZKV_LIMBS_BELOW(ao, 29); ZKV_LIMBS_BELOW(ap, 29); ZKV_LIMBS_BELOW(nU, 30); ZKV_LIMBS_BELOW(nV, 30);
    fp_mac81(col, ao, nU); fp_mac81(col, ap, nV);
}
// One 81-term product of lazy limbs a (below 2^29 + 2^30: e + 8p - b and the like) with the normalised limbs of an Fp scalar.  27 units.
ZKV_HD void fp_sum_scale(uint64_t (&col)[18], const uint32_t (&a)[9], const uint32_t (&k)[9]) {
#if defined(ZKV_COUNT_FP_MUL)
    zkv_fp_mul_counter += 1;
#endif
    ZKV_LIMBS_BELOW(a, 31); ZKV_LIMBS_BELOW(k, 29);
    fp_mac81(col, a, k);
}
// Close a sum on limbs: what f2_sum_close does, without the pack.
ZKV_HD void f2_sum_close_limbs(uint64_t (&col)[18], uint32_t (&r)[9]) {
    fp_reduce_cols_limbs(col, r);
#if defined(__HIP_DEVICE_COMPILE__)
    limbs_pin(r);
    __builtin_amdgcn_sched_barrier(0);
#endif
}
// The factors of a square from normalised limbs (own, par) of a value below 4.5 p (f2_limbs_sqr takes reduced values): even lane
// M = a0 + a1, N = a0 - a1 + 5p (below 9.5 p); odd lane M = 2 a0, N = a1.
ZKV_HD void limbs_sqr_factors_5p(const uint32_t (&own)[9], const uint32_t (&par)[9], uint32_t (&M)[9], uint32_t (&N)[9]) {
    uint32_t F[9]; limbs_kp_fat<5, 1>(F);
    const bool odd = zkv_parity() != 0;
#pragma unroll
    for (int i = 0; i < 9; i++) {
        M[i] = par[i] + (odd ? par[i] : own[i]);
        N[i] = own[i] + (odd ? 0u : F[i] - par[i]);
    }
    limbs_carry(N);
}
// ... and of -3 (a^2) for a reduced value: M as above; even lane N = 3 (a1 - a0 + 2p), odd lane N = 3 (2p - a1), both below 12 p.
ZKV_HD void limbs_sqr_factors_neg3(const uint32_t (&own)[9], const uint32_t (&par)[9], uint32_t (&M)[9], uint32_t (&N)[9]) {
    uint32_t F[9]; limbs_kp_fat<2, 1>(F);
    const bool odd = zkv_parity() != 0;
#pragma unroll
    for (int i = 0; i < 9; i++) {
        M[i] = par[i] + (odd ? par[i] : own[i]);
        N[i] = F[i] - own[i] + (odd ? 0u : par[i]);
    }
    limbs_carry_x3(N);
}

#if defined(ZKV_COUNT_FP_MUL)
struct LineCharge {                     // see zkv_line_mad_excess_counter
    unsigned long long c0, i0, m0;
    LineCharge() : c0(zkv_mad_counter), i0(zkv_mad_issued_counter), m0(zkv_fp_mul_counter) {}
    void settle(unsigned long long mads, unsigned long long muls) {
        zkv_line_mad_excess_counter += (long long)(zkv_mad_issued_counter - i0) - (long long)mads;
        zkv_mad_counter = c0 + mads; zkv_mad_issued_counter = i0 + mads; zkv_fp_mul_counter = m0 + muls;
    }
};
#endif

// Both steps take the running point through its slot tm (Fp2 values 0, 1, 2 = X, Y, Z: the LDS rows of k_miller2, HBM rows in the aggregate
// kernels): a coordinate is read where its limbs are needed and written as soon as the new one is formed -- every read of the old one lies
// before that -- so no packed coordinate is held across the body.  scale(0), scale(1): xs and ys, likewise fetched where they are used.
//
// Tangent step.  T <- 2T; l0 = -h, c3 = 3 X^2 xs, c4 = (e - b) ys with b = Y^2, e = 3 b' Z^2, h = 2 Y Z (line_dbl's names).
// X, Y, Z, xs, ys: reduced values (below 2p).  Outputs below 2p.
template <class RT, class SC> ZKV_HD void line_dbl_sums(RT tm, Fp2& l0, Fp2& c3, Fp2& c4, SC scale) {
#if defined(ZKV_COUNT_FP_MUL)
    LineCharge charge;
#endif
    const uint32_t FAT[9] = ZKV_FP_FAT8P_LIMBS;
    const Fp2C b3c = ZKV_TWIST_3B;
    uint64_t col[18];
    uint32_t yo[9], yp[9], tU[9], tV[9], M[9], N[9], xo[9], xp[9];
    uint32_t b[9], h[9], m[9], e[9], q[9], qp[9], k9[9];
    // b = Y^2: 18 + 9 units, 40 p^2
    f2_limbs_x(m_ld_f2(tm, 1).h, yo, yp);
    f2_limbs_sqr(yo, yp, M, N);
    f2_sum_open(col); f2_sum_sqr(col, M, N); f2_sum_close_limbs(col, b);
    // h = 2 Y Z on doubled multiplicand limbs: 54 + 9 = 63 | 45 units, 2 * 20 p^2
    fp_unpack29(m_ld_f2(tm, 2).h, xo);
    limbs_y(xo, tU, tV);
#pragma unroll
    for (int i = 0; i < 9; i++) { q[i] = yo[i] << 1; qp[i] = yp[i] << 1; }
    f2_sum_open(col); f2_sum_cross_dbl(col, q, qp, tU, tV); f2_sum_close_limbs(col, h);
    { Fp2 hp; hp.h = fp_pack29(h); l0 = f2_neg(hp); }
    // c = Z^2 (18 + 9 units, 40 p^2), e = 3 b' c (27 + 9 units, 20 p^2)
    limbs_partner(xo, xp);
    f2_limbs_sqr(xo, xp, M, N);
    f2_sum_open(col); f2_sum_sqr(col, M, N); f2_sum_close_limbs(col, q);
    limbs_partner(q, qp);
    {
        // the multiplier form of the constant 3 b': no exchange, U is the same in both lanes and V is b'1 in the odd lane, 8p - b'1 in the
        // even one: a constant plus a masked constant, on a lane mask the compiler cannot tell from a new value (selects of two constants
        // on the lane's parity leave the loop as invariants and hold nine registers across the whole of it)
        uint32_t em = zkv_parity() == 0 ? ~0u : 0u;
#if defined(__HIP_DEVICE_COMPILE__)
        asm volatile("" : "+v"(em));
#endif
        uint32_t y1[9]; fp_unpack29(b3c.c0, tU); fp_unpack29(b3c.c1, y1);
#pragma unroll
        for (int i = 0; i < 9; i++) tV[i] = y1[i] + (em & (FAT[i] - 2u * y1[i]));
    }
    f2_sum_open(col); f2_sum_cross(col, q, qp, tU, tV); f2_sum_close_limbs(col, e);
    // m = X Y: 27 + 9 units, 20 p^2
    f2_limbs_x(m_ld_f2(tm, 0).h, xo, xp);
    limbs_y(yo, tU, tV);
    f2_sum_open(col); f2_sum_cross(col, xo, xp, tU, tV); f2_sum_close_limbs(col, m);
    // c3 = (3 X^2) xs: the square with N tripled in its carry pass (N = 3 (x0 + 8p - x1) below 30 p, top limb below 2^27): 18 + 9 units,
    // 4p * 30p = 120 p^2; then one 81-term product with xs: 9 + 9 units, 4 p^2
    {
        const bool odd = zkv_parity() != 0;
#pragma unroll
        for (int i = 0; i < 9; i++) { M[i] = xp[i] + (odd ? xp[i] : xo[i]); N[i] = xo[i] + (odd ? 0u : FAT[i] - xp[i]); }
        limbs_carry_x3(N);
    }
    f2_sum_open(col); f2_sum_sqr(col, M, N); f2_sum_close_limbs(col, q);
    fp_unpack29(scale(0), k9);
    f2_sum_open(col); fp_sum_scale(col, q, k9); c3.h = f2_sum_close(col);
    // c4 = (e - b) ys on lazy limbs e + 8p - b (below 2^29 + 2^30, value below 10 p): 27 + 9 units, 20 p^2
#pragma unroll
    for (int i = 0; i < 9; i++) q[i] = e[i] + FAT[i] - b[i];
    fp_unpack29(scale(1), k9);
    f2_sum_open(col); fp_sum_scale(col, q, k9); c4.h = f2_sum_close(col);
    // T.x = m (b - 3e) / 2: the multiplicand (b + 8p - 3e [+ p]) / 2 is below 5.5 p; 27 + 9 units, 5.5p * 2p + 5.5p * 8p = 55 p^2.
    // Signed limbs: b + 8p - 3e + p lies in (-3 * 2^29, 3.61 * 2^29) a limb (the limbs of 8p are below 0.86 * 2^30, those of p below 0.89 * 2^29).
#pragma unroll
    for (int i = 0; i < 9; i++) q[i] = b[i] + FAT[i] - 3u * e[i];
    limbs_half_carry<true>(q);
    limbs_partner(q, qp);
    limbs_y(m, tU, tV);
    f2_sum_open(col); f2_sum_cross(col, q, qp, tU, tV);
    { Fp2 o; o.h = f2_sum_close(col); m_st_f2(tm, 0, o); }
    // T.y = g^2 - 3 e^2 as ONE sum of two squares, g = (b + 3e [+ p]) / 2 below 4.5 p (limbs before the carry below 4.89 * 2^29):
    //   g^2:     M below 9 p, N = g0 - g1 + 5p below 9.5 p (odd lane: 9 p, 4.5 p)         18 units, 85.5 p^2
    //   -3 e^2:  M below 4 p, N = 3 (e1 - e0 + 2p) below 12 p (odd lane: 3 (2p - e1))     18 units, 48 p^2
    // 36 + 9 units, 133.5 p^2
#pragma unroll
    for (int i = 0; i < 9; i++) q[i] = b[i] + 3u * e[i];
    limbs_half_carry<false>(q);
    limbs_partner(q, qp);
    limbs_sqr_factors_5p(q, qp, M, N);
    f2_sum_open(col); f2_sum_sqr(col, M, N);
    limbs_partner(e, qp);
    limbs_sqr_factors_neg3(e, qp, M, N);
    f2_sum_sqr(col, M, N);
    { Fp2 o; o.h = f2_sum_close(col); m_st_f2(tm, 1, o); }
    // T.z = b h: 27 + 9 units, 20 p^2
    limbs_partner(b, qp);
    limbs_y(h, tU, tV);
    f2_sum_open(col); f2_sum_cross(col, b, qp, tU, tV);
    { Fp2 o; o.h = f2_sum_close(col); m_st_f2(tm, 2, o); }
#if defined(ZKV_COUNT_FP_MUL)
    charge.settle(4 * 243 + 6 * 162 + 2 * 162, 4 * 2 + 6 + 2);         // line_dbl and the two scalings of the mul034 region
#endif
}

// Chord step.  T <- T + Q, Q = (qx, qy) affine; l0 = lambda, c3 = -theta xs, c4 = (theta qx - lambda qy) ys (line_add's names).
// X, Y, Z, qx, qy, xs, ys: reduced values.  Outputs below 2p.
// Registers: of lambda and theta only the nine limbs are held; their multiplier forms are made where a product needs them (limbs_pin in
// front of a second preparation, so that it is not merged with the first and kept).  Z's multiplier form is held throughout.
template <class RT, class SC> ZKV_HD void line_add_sums(RT tm, const Fp2& qx, const Fp2& qy, Fp2& l0, Fp2& c3, Fp2& c4, SC scale) {
#if defined(ZKV_COUNT_FP_MUL)
    LineCharge charge;
#endif
    const uint32_t FAT[9] = ZKV_FP_FAT8P_LIMBS;
    uint32_t F4[9]; limbs_kp_fat<4, 2>(F4);                      // 4p with limbs 0 .. 7 at least 2^30 - 2: e + f - 2g + F4 has no negative limb
    uint64_t col[18];
    uint32_t zU[9], zV[9], ao[9], ap[9], bo[9], bp[9], tU[9], tV[9], M[9], N[9];
    uint32_t th[9], la[9], e[9], f[9], g[9], w[9], k9[9];
    // lambda = X - qx Z, theta = Y - qy Z: the products 27 + 9 units, 20 p^2; the two subtractions stay packed (l0 = lambda goes out packed
    // and below 2p, and theta takes the same road: their limbs are the operands of everything that follows)
    f2_limbs_y(m_ld_f2(tm, 2).h, zU, zV);
    f2_limbs_x(qx.h, ao, ap);
    f2_sum_open(col); f2_sum_cross(col, ao, ap, zU, zV);
    { Fp2 s; s.h = f2_sum_close(col); l0 = f2_sub(m_ld_f2(tm, 0), s); }
    f2_limbs_x(qy.h, bo, bp);
    f2_sum_open(col); f2_sum_cross(col, bo, bp, zU, zV);
    { Fp2 s; s.h = f2_sum_close(col); s = f2_sub(m_ld_f2(tm, 1), s); fp_unpack29(s.h, th); }
    fp_unpack29(l0.h, la);
    // l3 = theta qx - lambda qy as ONE sum: 27 + 27 + 9 = 63 | 18 + 36 + 9 = 63 units, 20 + 32 = 52 p^2; c4 = l3 ys: 9 + 9 units, 4 p^2
    limbs_y(th, tU, tV);
    f2_sum_open(col); f2_sum_cross(col, ao, ap, tU, tV);
    limbs_y_neg(la, tU, tV);
    f2_sum_cross_neg(col, bo, bp, tU, tV); f2_sum_close_limbs(col, w);
    fp_unpack29(scale(1), k9);
    f2_sum_open(col); fp_sum_scale(col, w, k9); c4.h = f2_sum_close(col);
    // c3 = -theta xs on lazy limbs 8p - theta (below 2^30): 18 + 9 units, 8p * 2p = 16 p^2
#pragma unroll
    for (int i = 0; i < 9; i++) w[i] = FAT[i] - th[i];
    fp_unpack29(scale(0), k9);
    f2_sum_open(col); fp_sum_scale(col, w, k9); c3.h = f2_sum_close(col);
    // d = lambda^2 (18 + 9 units, 40 p^2); e = lambda d, g = X d (27 + 9 units, 20 p^2)
    limbs_partner(la, ap);
    f2_limbs_sqr(la, ap, M, N);
    f2_sum_open(col); f2_sum_sqr(col, M, N); f2_sum_close_limbs(col, ao);
    limbs_partner(ao, ap);
    limbs_y(la, tU, tV);
    f2_sum_open(col); f2_sum_cross(col, ao, ap, tU, tV); f2_sum_close_limbs(col, e);
    f2_limbs_y(m_ld_f2_again(tm, 0).h, tU, tV);
    f2_sum_open(col); f2_sum_cross(col, ao, ap, tU, tV); f2_sum_close_limbs(col, g);
    // c = theta^2 (18 + 9 units, 40 p^2); f = Z c (27 + 9 units, 20 p^2)
    limbs_partner(th, bp);
    f2_limbs_sqr(th, bp, M, N);
    f2_sum_open(col); f2_sum_sqr(col, M, N); f2_sum_close_limbs(col, bo);
    limbs_partner(bo, bp);
    f2_sum_open(col); f2_sum_cross(col, bo, bp, zU, zV); f2_sum_close_limbs(col, f);
    // T.x = lambda h, h = e + f - 2g limb by limb (+ 4p: in (0, 8p)): 27 + 9 units, 8p * 2p + 8p * 8p = 80 p^2
#pragma unroll
    for (int i = 0; i < 9; i++) w[i] = e[i] + f[i] + F4[i] - 2u * g[i];
    limbs_carry(w);
    limbs_partner(w, ap);
    limbs_pin(la);
    limbs_y(la, tU, tV);
    f2_sum_open(col); f2_sum_cross(col, w, ap, tU, tV);
    { Fp2 o; o.h = f2_sum_close(col); m_st_f2(tm, 0, o); }
    // T.y = theta (g - h) - e Y as ONE sum, g - h = 3g - e - f limb by limb (+ 4p: in (0, 10p)):
    // 27 + 27 + 9 = 63 | 18 + 36 + 9 = 63 units, (10p * 2p + 10p * 8p) + (2p * 8p + 2p * 2p) = 120 p^2
#pragma unroll
    for (int i = 0; i < 9; i++) w[i] = 3u * g[i] + F4[i] - e[i] - f[i];
    limbs_carry(w);
    limbs_partner(w, ap);
    limbs_pin(th);
    limbs_y(th, tU, tV);
    f2_sum_open(col); f2_sum_cross(col, w, ap, tU, tV);
    { uint32_t y[9]; fp_unpack29(m_ld_f2_again(tm, 1).h, y); limbs_y_neg(y, tU, tV); }
    limbs_partner(e, bp);
    f2_sum_cross_neg(col, e, bp, tU, tV);
    { Fp2 o; o.h = f2_sum_close(col); m_st_f2(tm, 1, o); }
    // T.z = Z e: 27 + 9 units, 20 p^2
    f2_sum_open(col); f2_sum_cross(col, e, bp, zU, zV);
    { Fp2 o; o.h = f2_sum_close(col); m_st_f2(tm, 2, o); }
#if defined(ZKV_COUNT_FP_MUL)
    charge.settle(11 * 243 + 2 * 162 + 2 * 162, 11 * 2 + 2 + 2);       // line_add and the two scalings of the mul034 region
#endif
}

}  // namespace zkv
#endif  // ZKV_PAIRED

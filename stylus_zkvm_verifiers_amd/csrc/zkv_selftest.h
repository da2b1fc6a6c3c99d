// Known-answer harness of the arithmetic primitives (zkv_diag_primitive, include/zkv.h).  TEST ONLY: nothing on a verify path calls it.
//
// One case is one set of operands; the case bodies below call the library's own primitives -- nothing is re-implemented here -- in the
// mapping the verify kernels run them in:
//   mapping 0  one value per lane (k_selftest.hip, ZKV_PAIRED undefined): k_prep, k_msm, k_plonk, k_precompile, the aggregate check;
//   mapping 1  one case per lane pair (k_selftest_pair.hip): k_miller2, k_finalexp2, the precompile pairing; Fp12 values in LDS slots
//              (LRef, and L9Ref for the resident-limb accumulator) with the S operand of f12l9_mul in a global row (SoaRW);
//   mapping 2  one case per 16 lanes (zkv_tower_wide.h, S = 1), mapping 3  one case per wavefront (S = 4), slots laid out as in k_wide.hip.
// The bodies are ZKV_HD so that the host emulations (tests/host_sim) run the same code on the same cases.
// Words: every Fp / Fr is eight little-endian 32-bit words (a Montgomery-domain integer, not necessarily reduced); an Fp2 is c0 then c1;
// an Fp12 is six Fp2 in slot order g0 g1 g2 h0 h1 h2 (powers 0 2 4 1 3 5 of w), 96 words.  Layouts per op: include/zkv_diag_primitive.h.
#pragma once
#include <stdint.h>

namespace zkv {

// words per case of (mapping, op): in, out; false for an unknown pair
inline bool selftest_io(int mapping, int op, int* in_w, int* out_w) {
    static const int LANE[11][2] = {{24, 128}, {24, 16}, {16, 16}, {8, 8}, {32, 64}, {24, 40}, {8, 12}, {64, 72}, {32, 2}, {128, 248}, {112, 384}};
    static const int PAIR[10][2] = {{32, 80}, {162, 18}, {36, 18}, {240, 11 * 96}, {96, 2 * 96}, {32, 4}, {192, 6}, {80, 2}, {192, 816}, {32, 4}};
    static const int WIDE[4][2] = {{240, 8 * 96}, {96, 96}, {96, 16}, {288, 0}};     // op 2: one word per lane of the group, 16 S; op 3: below
    const int* w = nullptr;
    if (mapping == 0 && op >= 0 && op < 11) w = LANE[op];
    else if (mapping == 1 && op >= 0 && op < 10) w = PAIR[op];
    else if ((mapping == 2 || mapping == 3) && op >= 0 && op < 4) w = WIDE[op];
    if (!w) return false;
    *in_w = w[0]; *out_w = (mapping == 3 && op == 2) ? 4 * w[1] : w[1];
    // wide op 3: two line steps of T' (48) and three coefficients (48) per pair of the group (8 S pairs), five Fp12, the chain's T
    if (mapping >= 2 && op == 3) *out_w = 2 * (48 + 48 * 8 * (mapping == 3 ? 4 : 1)) + 5 * 96 + 48;
    return true;
}
// cases one wavefront holds in each mapping (the host pads a batch to whole wavefronts with zero operands)
inline int selftest_cases_per_wave(int mapping) { return mapping == 0 ? 64 : mapping == 1 ? 32 : mapping == 2 ? 4 : 1; }

}  // namespace zkv

#if defined(ZKV_SELFTEST_BODIES)
#if defined(ZKV_PAIRED)
#include "zkv_tower_wide.h"
#else
#include "zkv_verify.h"
#include "zkv_scalar.h"
#endif

namespace zkv {

ZKV_HD Fp st_ld(const uint32_t* w) { Fp r; for (int i = 0; i < 8; i++) r.v[i] = w[i]; return r; }
ZKV_HD void st_st(uint32_t* w, const Fp& a) { for (int i = 0; i < 8; i++) w[i] = a.v[i]; }

#if !defined(ZKV_PAIRED)
ZKV_HD Fr st_ldr(const uint32_t* w) { Fr r; for (int i = 0; i < 8; i++) r.v[i] = w[i]; return r; }
ZKV_HD void st_str(uint32_t* w, const Fr& a) { for (int i = 0; i < 8; i++) w[i] = a.v[i]; }
ZKV_HD void st_stj(uint32_t* w, const G1J& p) { st_st(w, p.x); st_st(w + 8, p.y); st_st(w + 16, p.z); }
ZKV_HD G1J st_ldj(const uint32_t* w) { G1J p; p.x = st_ld(w); p.y = st_ld(w + 8); p.z = st_ld(w + 16); return p; }
ZKV_HD Fp2 st_ld2(const uint32_t* w) { Fp2 r; r.c0 = st_ld(w); r.c1 = st_ld(w + 8); return r; }
ZKV_HD void st_st2(uint32_t* w, const Fp2& a) { st_st(w, a.c0); st_st(w + 8, a.c1); }
ZKV_HD G2J st_ldj2(const uint32_t* w) { G2J p; p.x = st_ld2(w); p.y = st_ld2(w + 16); p.z = st_ld2(w + 32); return p; }
ZKV_HD void st_stj2(uint32_t* w, const G2J& p) { st_st2(w, p.x); st_st2(w + 16, p.y); st_st2(w + 32, p.z); }

// one case, one lane
ZKV_HD void selftest_lane(int op, const uint32_t* in, uint32_t* out) {
    switch (op) {
    case 0: {                // linear ops: in a b c; out add sub neg dbl half (a+b, c+a) (a-b, c-a) add_n sub_n [is_zero(a), eq(a, b)]
        const Fp a = st_ld(in), b = st_ld(in + 8), c = st_ld(in + 16);
        st_st(out, fp_add(a, b)); st_st(out + 8, fp_sub(a, b)); st_st(out + 16, fp_neg(a)); st_st(out + 24, fp_dbl(a)); st_st(out + 32, fp_half(a));
        Fp r0, r1;
        fp_add_x2(a, b, c, a, r0, r1); st_st(out + 40, r0); st_st(out + 48, r1);
        fp_sub_x2(a, b, c, a, r0, r1); st_st(out + 56, r0); st_st(out + 64, r1);
        const Fp x[3] = {a, b, c}, y[3] = {b, c, a};
        Fp r[3];
        fp_add_n<3>(x, y, r); for (int k = 0; k < 3; k++) st_st(out + 72 + 8 * k, r[k]);
        fp_sub_n<3>(x, y, r); for (int k = 0; k < 3; k++) st_st(out + 96 + 8 * k, r[k]);
        for (int k = 120; k < 128; k++) out[k] = 0;
        out[120] = fp_is_zero(a) ? 1u : 0u; out[121] = fp_eq(a, b) ? 1u : 0u;
        break;
    }
    case 1: {                // in a b c; out fp_mul(a, b), fp_sqr(c)
        st_st(out, fp_mul(st_ld(in), st_ld(in + 8))); st_st(out + 8, fp_sqr(st_ld(in + 16)));
        break;
    }
    case 2: {                // in x (canonical raw), y (Montgomery); out fp_from_raw(x), fp_to_raw(y)
        st_st(out, fp_from_raw(in)); fp_to_raw(out + 8, st_ld(in + 8));
        break;
    }
    case 3: st_st(out, fp_inv(st_ld(in))); break;
    case 4: {                // in a b (Fp2); out f2_mul(a, b) f2_sqr(a) f2_mul_xi(a) f2_inv(a)
        const Fp2 a = st_ld2(in), b = st_ld2(in + 16);
        st_st2(out, f2_mul(a, b)); st_st2(out + 16, f2_sqr(a)); st_st2(out + 32, f2_mul_xi(a)); st_st2(out + 48, f2_inv(a));
        break;
    }
    case 5: {                // in a b (Montgomery Fr), x (any 256-bit word); out fr_mul fr_add fr_sub fr_inv(a) fr_from_raw_reduce(x)
        const Fr a = st_ldr(in), b = st_ldr(in + 8);
        st_str(out, fr_mul(a, b)); st_str(out + 8, fr_add(a, b)); st_str(out + 16, fr_sub(a, b)); st_str(out + 24, fr_inv(a));
        st_str(out + 32, fr_from_raw_reduce(in + 16));
        break;
    }
    case 6: {                // in k (raw scalar); out |k1| (5 words) neg1 |k2| (5 words) neg2
        uint32_t k[8], m1[5], m2[5], n1, n2;
        for (int i = 0; i < 8; i++) k[i] = in[i];
        glv_split(k, m1, n1, m2, n2);
        for (int i = 0; i < 5; i++) { out[i] = m1[i]; out[6 + i] = m2[i]; }
        out[5] = n1; out[11] = n2;
        break;
    }
    case 7: {                // in P (Jacobian), Q (affine), R (Jacobian); out g1j_dbl(P), g1j_add_affine(P, Q), g1j_add(P, R)
        const G1J p = st_ldj(in), r = st_ldj(in + 40);
        st_stj(out, g1j_dbl(p)); st_stj(out + 24, g1j_add_affine(p, st_ld(in + 24), st_ld(in + 32))); st_stj(out + 48, g1j_add(p, r));
        break;
    }
    case 8: {                // in a b (Fp2); out f2_is_zero(a), f2_eq(a, b) as 0 / 1 words
        const Fp2 a = st_ld2(in), b = st_ld2(in + 16);
        out[0] = f2_is_zero(a) ? 1u : 0u; out[1] = f2_eq(a, b) ? 1u : 0u;
        break;
    }
    case 9: {                // in P (Jacobian x y z, Fp2) Q (affine) R (Jacobian); out g2j_dbl(P) g2j_add_affine(P, Q) g2j_add(P, R) g2j_psi(P) g2_mul_u(Q),
                             // then g2j_eq(P, R), g2_on_twist(Q), g2_in_subgroup(Q) as 0 / 1 words and five zero words
        const G2J p = st_ldj2(in), r = st_ldj2(in + 80);
        const Fp2 qx = st_ld2(in + 48), qy = st_ld2(in + 64);
        st_stj2(out, g2j_dbl(p)); st_stj2(out + 48, g2j_add_affine(p, qx, qy)); st_stj2(out + 96, g2j_add(p, r)); st_stj2(out + 144, g2j_psi(p));
        st_stj2(out + 192, g2_mul_u(qx, qy));
        for (int k = 240; k < 248; k++) out[k] = 0;
        out[240] = g2j_eq(p, r) ? 1u : 0u; out[241] = g2_on_twist(qx, qy) ? 1u : 0u; out[242] = g2_in_subgroup(qx, qy) ? 1u : 0u;
        break;
    }
    case 10: {               // in T (homogeneous X Y Z, Fp2) Q Q2 (affine); out line_dbl(T), line_add(T, Q) as (T', l0, l1, l3), g2_frob_affine(Q),
                             // g2_frob2_affine(Q), aff_dbl(Q), aff_add(Q, Q2) as (T', nl, c) with the line passed through line_to_table
        const Fp2 qx = st_ld2(in + 48), qy = st_ld2(in + 64), q2x = st_ld2(in + 80), q2y = st_ld2(in + 96);
        Fp2 l0, l1, l3;
        G2H T; T.x = st_ld2(in); T.y = st_ld2(in + 16); T.z = st_ld2(in + 32);
        line_dbl(T, l0, l1, l3);
        st_st2(out, T.x); st_st2(out + 16, T.y); st_st2(out + 32, T.z); st_st2(out + 48, l0); st_st2(out + 64, l1); st_st2(out + 80, l3);
        T.x = st_ld2(in); T.y = st_ld2(in + 16); T.z = st_ld2(in + 32);
        line_add(T, qx, qy, l0, l1, l3);
        st_st2(out + 96, T.x); st_st2(out + 112, T.y); st_st2(out + 128, T.z); st_st2(out + 144, l0); st_st2(out + 160, l1); st_st2(out + 176, l3);
        Fp2 x, y;
        g2_frob_affine(x, y, qx, qy); st_st2(out + 192, x); st_st2(out + 208, y);
        g2_frob2_affine(x, y, qx, qy); st_st2(out + 224, x); st_st2(out + 240, y);
        for (int k = 0; k < 2; k++) {
            G2A A; A.x = qx; A.y = qy;
            const LineAffC L = line_to_table(k == 0 ? aff_dbl(A) : aff_add(A, q2x, q2y));
            uint32_t* o = out + 256 + 64 * k;
            st_st2(o, A.x); st_st2(o + 16, A.y); st_st(o + 32, L.nl.c0); st_st(o + 40, L.nl.c1); st_st(o + 48, L.c.c0); st_st(o + 56, L.c.c1);
        }
        break;
    }
    default: break;
    }
}
#else   // ---------------------------------------------------------------- lane pairs and wide groups

template <int N> ZKV_HD L9 st_lincomb_n(const uint32_t* xs, const uint32_t* ks, int c) {
    LTerm t[N];
    for (int j = 0; j < N; j++) { t[j].x = xs + 9 * j; t[j].k = (int32_t)ks[j]; }
    return l9_lincomb(t, c);
}
ZKV_HD Fp2 st_ldh(const uint32_t* w, uint32_t par) { Fp2 r; r.h = st_ld(w + 8 * par); return r; }

// one case, one lane of its pair.  lds: this lane's column of a (144 + 54) x 64-word LDS block (word k of the column at lds[64 k]).
ZKV_HD void selftest_pair(int op, const uint32_t* in, uint32_t* out, uint32_t* lds) {
    const uint32_t par = zkv_parity();
    switch (op) {
    case 0: {                // in a0 a1 b0 b1; out (c0, c1) of f2_mul(a, b) f2_sqr(a) f2_mul_xi(a) f2_add(a, b) f2_sub(a, b)
        const Fp2 a = st_ldh(in, par), b = st_ldh(in + 16, par);
        const Fp2 r[5] = {f2_mul(a, b), f2_sqr(a), f2_mul_xi(a), f2_add(a, b), f2_sub(a, b)};
        for (int k = 0; k < 5; k++) st_st(out + 16 * k + 8 * par, r[k].h);
        break;
    }
    case 1: {                // in n c k_even[8] k_odd[8] x_even[8][9] x_odd[8][9]; out this lane's nine limbs (even lane first)
        const int n = (int)in[0], c = (int)in[1];
        const uint32_t* ks = in + 2 + 8 * par;
        const uint32_t* xs = in + 18 + 72 * par;
        L9 r;
        switch (n) {
        case 1: r = st_lincomb_n<1>(xs, ks, c); break;
        case 2: r = st_lincomb_n<2>(xs, ks, c); break;
        case 3: r = st_lincomb_n<3>(xs, ks, c); break;
        case 4: r = st_lincomb_n<4>(xs, ks, c); break;
        case 5: r = st_lincomb_n<5>(xs, ks, c); break;
        case 6: r = st_lincomb_n<6>(xs, ks, c); break;
        case 7: r = st_lincomb_n<7>(xs, ks, c); break;
        case 8: r = st_lincomb_n<8>(xs, ks, c); break;
        default: for (int i = 0; i < 9; i++) r.l[i] = 0; break;
        }
        for (int i = 0; i < 9; i++) out[9 * par + i] = r.l[i];
        break;
    }
    case 2: {                // in a0 a1 b0 b1 as nine limbs each; out l9_mul(a, b), nine limbs per component
        L9 a, b;
        for (int i = 0; i < 9; i++) { a.l[i] = in[9 * par + i]; b.l[i] = in[18 + 9 * par + i]; }
        const L9 r = l9_mul(a, b);
        for (int i = 0; i < 9; i++) out[9 * par + i] = r.l[i];
        break;
    }
    case 3: {                // in a b (Fp12) c0 c3 c4 (Fp2); out the eleven results listed in include/zkv.h
        const LRef A = l_ref(lds), B = l_ref(lds + 48 * 64), D = l_ref(lds + 96 * 64);
        const L9Ref acc = l9_ref(lds + 144 * 64);
        const MRef ga = m_ref((uint32_t*)in + 8 * par, 1, 16), gb = m_ref((uint32_t*)in + 96 + 8 * par, 1, 16);
        const Fp2 c0 = st_ldh(in + 192, par), c3 = st_ldh(in + 208, par), c4 = st_ldh(in + 224, par);
        f12m_copy(A, ga); f12m_copy(B, gb);
        f12m_copy(D, A); f12m_mul(D, D, B); f12m_copy(m_ref(out + 8 * par, 1, 16), D);                 // d aliases a, as in the kernels
        f12m_copy(D, A); f12m_mul_conj(D, D, B); f12m_copy(m_ref(out + 96 + 8 * par, 1, 16), D);
        f12m_copy(D, A); f12m_sqr(D); f12m_copy(m_ref(out + 192 + 8 * par, 1, 16), D);
        f12m_inv(D, A); f12m_copy(m_ref(out + 288 + 8 * par, 1, 16), D);
        for (int k = 1; k <= 3; k++) { f12m_frob(D, A, k); f12m_copy(m_ref(out + 288 + 96 * k + 8 * par, 1, 16), D); }
        f12m_copy(D, A); f12m_mul_by_034(D, &c0, &c3, &c4); f12m_copy(m_ref(out + 672 + 8 * par, 1, 16), D);
        f12m_copy(D, A); f12m_mul_by_134(D, &c3, &c4); f12m_copy(m_ref(out + 768 + 8 * par, 1, 16), D);
        for (int cj = 0; cj < 2; cj++) {
            SoaRW S; S.p = (uint32_t*)in + 96; S.stride = 1; S.off = 32u * par;
            f12m_copy(acc, A);
            f12l9_mul(acc, S, cj != 0);
            f12m_copy(m_ref(out + 864 + 96 * cj + 8 * par, 1, 16), acc);
        }
        break;
    }
    case 4: {                // in a (cyclotomic Fp12); out f12m_cyclo_sqr(a), f12l9_cyclo_sqr(a)
        const LRef D = l_ref(lds + 96 * 64);
        const L9Ref acc = l9_ref(lds + 144 * 64);
        const MRef ga = m_ref((uint32_t*)in + 8 * par, 1, 16);
        f12m_copy(D, ga); f12m_cyclo_sqr(D); f12m_copy(m_ref(out + 8 * par, 1, 16), D);
        f12m_copy(acc, ga); f12l9_cyclo_sqr(acc); f12m_copy(m_ref(out + 96 + 8 * par, 1, 16), acc);
        break;
    }
    // The accept predicates.  Every lane writes the verdict IT returns (even lane's word, then the odd lane's): the kernels store the
    // status from one lane only, so both words must hold the combined verdict of the pair.
    case 5: {                // in a b (Fp2); out f2_is_zero(a) (even, odd), f2_eq(a, b) (even, odd)
        const Fp2 a = st_ldh(in, par), b = st_ldh(in + 16, par);
        out[par] = f2_is_zero(a) ? 1u : 0u; out[2 + par] = f2_eq(a, b) ? 1u : 0u;
        break;
    }
    case 6: {                // in f t (Fp12); out f12m_is_one(f) from an LDS slot, from a global row, f12m_eq_conj(f as the accumulator, t)
        const LRef A = l_ref(lds);
        const L9Ref acc = l9_ref(lds + 144 * 64);
        const MRef gf = m_ref((uint32_t*)in + 8 * par, 1, 16);
        SoaRW F; F.p = (uint32_t*)in; F.stride = 1; F.off = 32u * par;             // the rows fe_slot hands ISONE and EQCONJ
        SoaRW T; T.p = (uint32_t*)in + 96; T.stride = 1; T.off = 32u * par;
        f12m_copy(A, gf);
        out[par] = f12m_is_one(A) ? 1u : 0u;
        out[2 + par] = f12m_is_one(F) ? 1u : 0u;
        f12m_copy(acc, gf);
        out[4 + par] = f12m_eq_conj(acc, T) ? 1u : 0u;
        break;
    }
    case 7: {                // in T (X Y Z, Fp2) bx by (Fp2); out miller_point_closes(T; bx, by), T in an LDS slot as k_miller2 holds it
        const LRef tm = l_ref(lds + 48 * 64);
        for (int k = 0; k < 3; k++) m_st_f2(tm, k, st_ldh(in + 16 * k, par));
        const Fp2 bx = st_ldh(in + 48, par), by = st_ldh(in + 64, par);
        out[par] = miller_point_closes(tm, bx, by) ? 1u : 0u;
        break;
    }
    // The G2 steps of the Miller loop as miller_loop_p runs them: T in the LDS slot k_miller2 keeps it in, B re-read through a SoaRef row
    // for every chord, the scalings of A' through another, f in an LDS slot.  Every step starts from the input T.
    case 8: {                // in T (X Y Z) Q (x y) xs ys (Fp) f (Fp12); out the results listed in include/zkv_diag_primitive.h
        const LRef fm = l_ref(lds), tm = l_ref(lds + 48 * 64);
        SoaRef bsrc; bsrc.p = in + 48; bsrc.stride = 1; bsrc.off = 32u * par;
        SoaRef norm; norm.p = in + 80; norm.stride = 1; norm.off = 0;
        auto load_t = [&]() { for (int k = 0; k < 3; k++) m_st_f2(tm, k, st_ldh(in + 16 * k, par)); };
        auto step = [&](int kind, Fp2& l0, Fp2& l1, Fp2& l3) {          // the body of `if (do_t)` in miller_loop_p
            G2H T; T.x = m_ld_f2(tm, 0); T.y = m_ld_f2(tm, 1); T.z = m_ld_f2(tm, 2);
            if (kind == 0) line_dbl(T, l0, l1, l3);
            else {
                Fp2 qx, qy; qx.h = bsrc.fp(0); qy.h = bsrc.fp(16);
                if (kind == 2) qy = f2_neg(qy);
                else if (kind == 3) { Fp2 x, y; g2_frob_affine(x, y, qx, qy); qx = x; qy = y; }
                else if (kind == 4) { Fp2 x, y; g2_frob2_affine(x, y, qx, qy); qx = x; qy = f2_neg(y); }
                line_add(T, qx, qy, l0, l1, l3);
            }
            m_st_f2(tm, 0, T.x); m_st_f2(tm, 1, T.y); m_st_f2(tm, 2, T.z);
        };
        auto put = [&](uint32_t* o, const Fp2& l0, const Fp2& l1, const Fp2& l3) {
            for (int k = 0; k < 3; k++) st_st(o + 16 * k + 8 * par, m_ld_f2(tm, k).h);
            st_st(o + 48 + 8 * par, l0.h); st_st(o + 64 + 8 * par, l1.h); st_st(o + 80 + 8 * par, l3.h);
        };
        Fp2 l0, l1, l3, t0, t1, t3;
        load_t(); step(0, t0, t1, t3); put(out, t0, t1, t3);
        for (int kind = 1; kind <= 4; kind++) { load_t(); step(kind, l0, l1, l3); put(out + 96 * kind, l0, l1, l3); }
        f12m_copy(fm, m_ref((uint32_t*)in + 96 + 8 * par, 1, 16));
        {
            const Fp2 c3 = f2_mul_fp(t1, norm.fp(0)), c4 = f2_mul_fp(t3, norm.fp(8));
            f12m_mul_by_034_body(fm, t0, c3, c4);
        }
        f12m_copy(m_ref(out + 480 + 8 * par, 1, 16), fm);
        load_t(); step(0, l0, l1, l3); step(1, l0, l1, l3); step(0, l0, l1, l3);
        for (int k = 0; k < 3; k++) st_st(out + 576 + 16 * k + 8 * par, m_ld_f2(tm, k).h);
        load_t(); g2m_line_dbl(tm, &l0, &l1, &l3); put(out + 624, l0, l1, l3);          // the wrappers of miller_loop_m
        const Fp2 qx = st_ldh(in + 48, par), qy = st_ldh(in + 64, par);
        load_t(); g2m_line_add(tm, &qx, &qy, &l0, &l1, &l3); put(out + 720, l0, l1, l3);
        break;
    }
    case 9: {                // in Q (x y); out g2_on_twist(Q) (even, odd), g2_in_subgroup(Q) (even, odd), as k_g2chk2 forms them
        const Fp2 qx = st_ldh(in, par), qy = st_ldh(in + 16, par);
        out[par] = g2_on_twist(qx, qy) ? 1u : 0u; out[2 + par] = g2_in_subgroup(qx, qy) ? 1u : 0u;
        break;
    }
    default: break;
    }
}

// The G2 steps of k_miller2 as fused column sums (zkv_line_sums.h; zkv_diag_line_steps, include/zkv_diag_line_steps.h): the input row of
// op 8 above, T in the LDS slot of k_miller2, B and the scalings re-read through their SoaRef rows, every step starting from the input T.
// out: the tangent step and the chord steps of kinds 1 2 3 4 as T' l0 c3 c4 (5 x 96), f after the variable-line product with the tangent's
// line (96), T after tangent, chord(Q), tangent (48).
constexpr int ST_LINE_SUMS_IN = 192, ST_LINE_SUMS_OUT = 624;
ZKV_HD void selftest_line_sums(const uint32_t* in, uint32_t* out, uint32_t* lds) {
    const uint32_t par = zkv_parity();
    const LRef fm = l_ref(lds), tm = l_ref(lds + 48 * 64);
    SoaRef bsrc; bsrc.p = in + 48; bsrc.stride = 1; bsrc.off = 32u * par;
    SoaRef norm; norm.p = in + 80; norm.stride = 1; norm.off = 0;
    const auto scale = [&](int k) { return norm.fp(8 * k); };
    auto load_t = [&]() { for (int k = 0; k < 3; k++) m_st_f2(tm, k, st_ldh(in + 16 * k, par)); };
    auto step = [&](int kind, Fp2& l0, Fp2& c3, Fp2& c4) {          // the body of `if (do_t)` in miller_loop_p<true>
        if (kind == 0) line_dbl_sums(tm, l0, c3, c4, scale);
        else {
            Fp2 qx, qy; qx.h = bsrc.fp(0); qy.h = bsrc.fp(16);
            if (kind == 2) qy = f2_neg(qy);
            else if (kind == 3) { Fp2 x, y; g2_frob_affine(x, y, qx, qy); qx = x; qy = y; }
            else if (kind == 4) { Fp2 x, y; g2_frob2_affine(x, y, qx, qy); qx = x; qy = f2_neg(y); }
            line_add_sums(tm, qx, qy, l0, c3, c4, scale);
        }
    };
    auto put = [&](uint32_t* o, const Fp2& l0, const Fp2& c3, const Fp2& c4) {
        for (int k = 0; k < 3; k++) st_st(o + 16 * k + 8 * par, m_ld_f2(tm, k).h);
        st_st(o + 48 + 8 * par, l0.h); st_st(o + 64 + 8 * par, c3.h); st_st(o + 80 + 8 * par, c4.h);
    };
    Fp2 l0, c3, c4, t0, t3, t4;
    load_t(); step(0, t0, t3, t4); put(out, t0, t3, t4);
#pragma unroll 1
    for (int kind = 1; kind <= 4; kind++) { load_t(); step(kind, l0, c3, c4); put(out + 96 * kind, l0, c3, c4); }
    f12m_copy(fm, m_ref((uint32_t*)in + 96 + 8 * par, 1, 16));
    f12m_mul_by_034_body(fm, t0, t3, t4);
    f12m_copy(m_ref(out + 480 + 8 * par, 1, 16), fm);
    load_t(); step(0, l0, c3, c4); step(1, l0, c3, c4); step(0, l0, c3, c4);
    for (int k = 0; k < 3; k++) st_st(out + 576 + 16 * k + 8 * par, m_ld_f2(tm, k).h);
}

// words of group memory per case of the wide mappings: slots a, b, d and the slices' rows, or k_wide.hip's f, T, 13 scratch Fp2 and rows
constexpr int ST_WIDE_SLOT = 96 + 48 + 13 * 16 + W_RED_WORDS;
// This lane's index in its 16 S-lane group (lane 0 is the one that stores the status in k_finalexp_w / k_finalexp_w64).  On the device
// from the lane counter, as zkv_parity (blocks are whole wavefronts and groups are aligned): pairs 6 and 7, which shadow pairs 0 and 1,
// have indices of their own.  The host emulation has no threads for those two pairs; its index follows from the coefficient and slice.
template <int S> ZKV_HD int st_group_lane(WL w, uint32_t par) {
#if defined(__HIP_DEVICE_COMPILE__)
    (void)w; (void)par;
    return (int)(__builtin_amdgcn_mbcnt_hi(~0u, __builtin_amdgcn_mbcnt_lo(~0u, 0u)) & (uint32_t)(16 * S - 1));
#else
    return 16 * w.s + 2 * w.q + (int)par;
#endif
}
// one case, one lane of its 16 S-lane group.  g: the group's ST_WIDE_SLOT words (LDS on the device); w: this lane's coefficient and slice.
template <int S> ZKV_HD void selftest_wide(int op, const uint32_t* in, uint32_t* out, uint32_t* g, WL w) {
    const uint32_t par = zkv_parity();
    const int q = w.q;
    uint32_t* base = g + 8 * par;
    const MRef A = m_ref(base, 1, 16), B = m_ref(base + 96, 1, 16), D = m_ref(base + 192, 1, 16), red = m_ref(base + 288, 1, 16);
    const MRef ga = m_ref((uint32_t*)in + 8 * par, 1, 16), gb = m_ref((uint32_t*)in + 96 + 8 * par, 1, 16);
    auto put = [&](int k) { w12_copy(m_ref(out + 96 * k + 8 * par, 1, 16), D, q); };
    switch (op) {
    case 0: {                // in a b (Fp12) c0 c3 c4 (Fp2); out the eight results listed in include/zkv.h
        const Fp2 c0 = st_ldh(in + 192, par), c3 = st_ldh(in + 208, par), c4 = st_ldh(in + 224, par);
        w12_copy(A, ga, q); w12_copy(B, gb, q);
        w12_copy(D, A, q); w12_mul<S>(D, D, B, w, false, red); put(0);          // d aliases a, as in exp_u_w
        w12_copy(D, A, q); w12_mul<S>(D, D, B, w, true, red); put(1);
        w12_copy(D, A, q); w12_sqr<S>(D, w, red); put(2);
        w12_copy(D, A, q); w12_mul_sparse<S>(D, &c0, &c3, &c4, w, false, red); put(3);
        w12_copy(D, A, q); w12_mul_sparse<S>(D, &c3, &c3, &c4, w, true, red); put(4);        // with `one`, c0 aliases c3 (fixed_lines_mul_w)
        for (int k = 1; k <= 3; k++) { w12_frob(D, A, k, q); put(4 + k); }
        break;
    }
    case 1: {                // in a (cyclotomic Fp12); out w12_cyclo_sqr(a)
        w12_copy(D, ga, q); w12_cyclo_sqr<S>(D, w, red); put(0);
        break;
    }
    case 2: {                // in f (Fp12); out f12m_is_one(acc) as THIS lane returns it, acc laid out as finalexp_w_body's accumulator
        w12_copy(A, ga, q);
        const int lane = st_group_lane<S>(w, par);
        out[lane] = f12m_is_one(A) ? 1u : 0u;
#if !defined(__HIP_DEVICE_COMPILE__)
        if (q < 2) out[lane + 12] = out[lane];          // the host emulation has no shadow pairs: their words repeat pairs 0 and 1
#endif
        break;
    }
    // The line steps and line products of miller_loop_w and the inversion of final_exp_is_one_w, the group's memory laid out as in
    // k_wide.hip: f, T (3 Fp2), the 13 scratch Fp2 `sc`, the slices' rows.  Every step starts from the input T, every product from f.
    case 3: {                // in T Q xs ys f L0 L1 lxs lys cxs cys; out the results listed in include/zkv_diag_primitive.h
        const MRef fm = A, tm = m_ref(base + 96, 1, 16), sc = m_ref(base + 144, 1, 16), rd = m_ref(base + 352, 1, 16);
        const MRef gf = m_ref((uint32_t*)in + 96 + 8 * par, 1, 16);
        const Fp2 qx = st_ldh(in + 48, par), qy = st_ldh(in + 64, par);
        G1Norm n; n.axs = st_ld(in + 80); n.ays = st_ld(in + 88); n.lxs = st_ld(in + 256); n.lys = st_ld(in + 264); n.cxs = st_ld(in + 272); n.cys = st_ld(in + 280);
        LineAffC L[2];
        for (int k = 0; k < 2; k++) {
            L[k].nl.c0 = st_ld(in + 192 + 32 * k); L[k].nl.c1 = st_ld(in + 200 + 32 * k); L[k].c.c0 = st_ld(in + 208 + 32 * k); L[k].c.c1 = st_ld(in + 216 + 32 * k);
        }
        const int pi = st_group_lane<S>(w, par) >> 1;          // this pair's place among the 8 S pairs of the group
        constexpr int STEP = 48 + 48 * 8 * S;
        auto load_t = [&]() { wide_sync(); for (int k = 0; k < 3; k++) m_st_f2(tm, k, st_ldh(in + 16 * k, par)); wide_fence(); };
        auto put_t = [&](uint32_t* o) { for (int k = 0; k < 3; k++) st_st(o + 16 * k + 8 * par, m_ld_f2(tm, k).h); };
        auto put_l = [&](uint32_t* o, const Fp2& l0, const Fp2& l1, const Fp2& l3) {          // this pair's OWN copy of the coefficients
            uint32_t* c = o + 48 + 48 * pi + 8 * par;
            st_st(c, l0.h); st_st(c + 16, l1.h); st_st(c + 32, l3.h);
#if !defined(__HIP_DEVICE_COMPILE__)
            if (q < 2) { st_st(c + 48 * 6, l0.h); st_st(c + 48 * 6 + 16, l1.h); st_st(c + 48 * 6 + 32, l3.h); }      // no shadow pairs on the host: theirs repeat pairs 0 and 1
#endif
        };
        auto put_f = [&](uint32_t* o) { w12_copy(m_ref(o + 8 * par, 1, 16), fm, q); };
        Fp2 l0, l1, l3, t0, t1, t3;
        load_t(); w_line_dbl(tm, sc, &t0, &t1, &t3, q); put_t(out); put_l(out, t0, t1, t3);
        load_t(); w_line_add(tm, sc, &qx, &qy, &l0, &l1, &l3, q); put_t(out + STEP); put_l(out + STEP, l0, l1, l3);
        uint32_t* of = out + 2 * STEP;
        w12_copy(fm, gf, q); var_line_mul_w<S>(fm, sc, t0, t1, t3, n.axs, n.ays, w, rd); put_f(of);
        for (int k = 0; k < 3; k++) {               // (do_l, do_c) = (1, 1) (1, 0) (0, 1)
            w12_copy(fm, gf, q); fixed_lines_mul_w<S>(fm, sc, L[0], L[1], n, k != 2, k != 1, w, rd); put_f(of + 96 * (1 + k));
        }
        w12_copy(fm, gf, q); f12m_inv_w(fm); put_f(of + 4 * 96);
        load_t(); w_line_dbl(tm, sc, &l0, &l1, &l3, q); w_line_add(tm, sc, &qx, &qy, &l0, &l1, &l3, q); w_line_dbl(tm, sc, &l0, &l1, &l3, q);
        put_t(of + 5 * 96);
        break;
    }
    default: break;
    }
}
#endif  // ZKV_PAIRED

}  // namespace zkv
#endif  // ZKV_SELFTEST_BODIES

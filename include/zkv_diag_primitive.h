/*
 * zkv_diag_primitive.h -- known-answer harness of the arithmetic primitives.  TEST ONLY: no verification path uses it.
 *
 * Runs operands the caller chooses through the library's own field, tower, G1 and G2 code on the device, in the mappings the verify
 * kernels use (one value per lane, one case per lane pair, one per 16 lanes, one per wavefront), and returns the raw result words, so
 * that a test can check a primitive at the edges of its contract.  Companion of zkv.h (same library, same ZKV_OK / ZKV_ERR_* codes);
 * the case bodies are stylus_zkvm_verifiers_amd/csrc/zkv_selftest.h.
 */
#ifndef ZKV_DIAG_PRIMITIVE_H
#define ZKV_DIAG_PRIMITIVE_H
#include "zkv.h"

#ifdef __cplusplus
extern "C" {
#endif

#define ZKV_DIAG_PRIMITIVE_MAX_CASES 65536

/* Synchronous, host buffers: runs n cases (1 <= n <= ZKV_DIAG_PRIMITIVE_MAX_CASES) of one op
 * through the library's own field, tower and G1 code in the mapping the verify kernels use, and returns the raw result words.
 * ZKV_ERR_INVALID_ARG for an unknown (mapping, op), n = 0 or n > 65,536, or a NULL buffer (checked before anything is launched);
 * ZKV_ERR_NO_DEVICE without a gfx950 device.  Words are little-endian uint32; an Fp or Fr is 8 words holding a Montgomery-domain
 * integer (R = 2^261 for both fields; inputs need not be reduced), an Fp2 is c0 then c1 (16 words), an Fp12 six Fp2 in slot order
 * g0 g1 g2 h0 h1 h2 = powers 0 2 4 1 3 5 of w (96 words).  "Need not be reduced" holds for the Fp and Fp2 ops (mapping 0 ops 0-4, mapping 1
 * op 0: words up to 4p - 1, or any 256-bit word, as tests/primitive_cases.py tries them); the Fp12 routines, the cyclotomic squarings, the
 * line steps, the predicates and the G1 / G2 ops run routines whose contract is "reduced values, below 2p": every Fp word of their
 * operands must be below 2p -- ANY such word, 2p - 1 in all of them at once included -- and every Fp word they return is below 2p.
 * in: n x IN words, out: n x OUT words; per op (IN -> OUT):
 *   mapping 0, one value per lane:
 *     op 0  a b c (24) -> fp_add(a,b) fp_sub(a,b) fp_neg(a) fp_dbl(a) fp_half(a), fp_add_x2 -> (a+b, c+a), fp_sub_x2 -> (a-b, c-a),
 *           fp_add_n<3>([a b c], [b c a]), fp_sub_n<3>(same), then fp_is_zero(a), fp_eq(a,b) and six zero words (128)
 *     op 1  a b c (24) -> fp_mul(a,b) fp_sqr(c) (16)           op 2  x (raw, < p) y (16) -> fp_from_raw(x) fp_to_raw(y) (16)
 *     op 3  a (8) -> fp_inv(a) (8)                             op 4  a b (Fp2, 32) -> f2_mul(a,b) f2_sqr(a) f2_mul_xi(a) f2_inv(a) (64)
 *     op 5  a b (Fr) x (raw 256-bit) (24) -> fr_mul(a,b) fr_add(a,b) fr_sub(a,b) fr_inv(a) fr_from_raw_reduce(x) (40)
 *     op 6  k (raw, 8) -> glv_split: |k1| (5 words) neg1 |k2| (5 words) neg2 (12)
 *     op 7  P (Jacobian x y z) Q (affine x y) T (Jacobian) (64) -> g1j_dbl(P) g1j_add_affine(P,Q) g1j_add(P,T) (72)
 *     op 8  a b (Fp2, 32) -> f2_is_zero(a) f2_eq(a,b), one 0 / 1 word each (2)
 *     op 9  P (Jacobian x y z over Fp2, 48) Q (affine x y, 32) R (Jacobian, 48) (128) -> g2j_dbl(P) g2j_add_affine(P,Q) g2j_add(P,R)
 *           g2j_psi(P) g2_mul_u(Q), 48 Jacobian words each, then g2j_eq(P,R) g2_on_twist(Q) g2_in_subgroup(Q), one 0 / 1 word each, and
 *           five zero words (248).  Infinity is z = 0 (mod p).
 *     op 10 T (homogeneous X Y Z, 48) Q Q2 (affine, 32 each) (112) -> line_dbl(T) and line_add(T,Q), each as T' l0 l1 l3 (96),
 *           g2_frob_affine(Q) g2_frob2_affine(Q) (x y, 32 each), aff_dbl(Q) and aff_add(Q,Q2), each as the new point x y and the
 *           line nl c as line_to_table lays it out (64) (384)
 *   mapping 1, one case per lane pair (ZKV_PAIRED: the even lane holds c0, the odd lane c1):
 *     op 0  a b (Fp2, 32) -> f2_mul(a,b) f2_sqr(a) f2_mul_xi(a) f2_add(a,b) f2_sub(a,b) (80)
 *     op 1  n c k_even[8] k_odd[8] x_even[8][9] x_odd[8][9] (162) -> l9_lincomb of the first n (1..8; otherwise zeros) terms with
 *           coefficient c, nine 29-bit limbs per lane, even lane first (18)
 *     op 2  a0 a1 b0 b1, nine limbs each (36) -> l9_mul(a, b), nine limbs per component (18)
 *     op 3  a b (Fp12) c0 c3 c4 (Fp2) (240) -> eleven Fp12 (1056): f12m_mul(a,b) f12m_mul_conj(a,b) f12m_sqr(a) f12m_inv(a)
 *           f12m_frob(a,1) (a,2) (a,3) f12m_mul_by_034(a; c0,c3,c4) f12m_mul_by_134(a; c3,c4) f12l9_mul(a,b) f12l9_mul(a,conj b),
 *           with a and the results in LDS slots (LRef; L9Ref for f12l9_*) and the S operand of f12l9_mul in the input row
 *     op 4  a (cyclotomic Fp12, 96) -> f12m_cyclo_sqr(a) f12l9_cyclo_sqr(a) (192)
 *     ops 5-7, the accept predicates: every verdict is two 0 / 1 words, what the even lane returned and then what the odd lane returned
 *     (the verify kernels store the status from the even lane alone)
 *     op 5  a b (Fp2, 32) -> f2_is_zero(a) f2_eq(a,b) (4)
 *     op 6  f t (Fp12, 192) -> f12m_is_one(f) with f in an LDS slot (LRef), f12m_is_one(f) with f read as a global row (SoaRW),
 *           f12m_eq_conj(f, t) with f in the resident-limb accumulator (L9Ref) and t a global row (SoaRW) (6)
 *     op 7  T (X Y Z, Fp2) bx by (Fp2) (80) -> miller_point_closes(T; bx, by) with T in an LDS slot (2)
 *     op 8  T (X Y Z, 48) Q (x y, 32) xs ys (Fp, 8 each) f (Fp12, 96) (192) -> the G2 steps as miller_loop_p runs them, T in the LDS slot
 *           of k_miller2, Q re-read through a SoaRef row for every chord, f in an LDS slot; every step starts from the input T (816):
 *           words   0  the tangent step as T' (read back from the slot) l0 l1 l3 (96)
 *           words  96  the chord steps of kinds 1 2 3 4 -- with Q, -Q, psi(Q), -psi^2(Q) -- likewise (4 x 96)
 *           words 480  f after the variable-line product with the tangent's line: f2_mul_fp(l1, xs) f2_mul_fp(l3, ys), then
 *                      f12m_mul_by_034_body (96)
 *           words 576  T after tangent, chord(Q), tangent (48)
 *           words 624  g2m_line_dbl(T) and words 720 g2m_line_add(T, Q), the wrappers of miller_loop_m, as T' l0 l1 l3 (2 x 96): the
 *                      same words as at 0 and at 96
 *     op 9  Q (x y, 32) -> g2_on_twist(Q) g2_in_subgroup(Q), two 0 / 1 words each as for ops 5-7 (4)
 *   mapping 2 (one case per 16 lanes, S = 1) and mapping 3 (one case per wavefront, S = 4), zkv_tower_wide.h:
 *     op 0  a b c0 c3 c4 as for mapping 1 op 3 (240) -> eight Fp12 (768): w12_mul(a,b) w12_mul(a,conj b) w12_sqr(a)
 *           w12_mul_sparse(a; c0,c3,c4) w12_mul_sparse(a; 1,c3,c4) w12_frob(a,1) (a,2) (a,3)
 *     op 1  a (cyclotomic Fp12, 96) -> w12_cyclo_sqr(a) (96)
 *     op 2  f (Fp12, 96) -> f12m_is_one(f) with f in the group's accumulator slot as k_finalexp_w lays it out, one 0 / 1 word per lane of
 *           the group in lane order (16 for mapping 2, 64 for mapping 3); word 0 is the lane that stores the status
 *     op 3  T (48) Q (32) xs ys (8 each) f (Fp12, 96) L0 L1 (LineAffC: nl c, 32 each) lxs lys cxs cys (Fp, 8 each) (288) -> the line steps
 *           and line products of miller_loop_w, the group's memory laid out as in k_wide.hip (f, T, 13 scratch Fp2, the slices' rows);
 *           G = 8 pairs (mapping 2) or 32 pairs (mapping 3), STEP = 48 + 48 G, 2 STEP + 528 in all (1392 words for mapping 2, 3696 for mapping 3):
 *           words 0             w_line_dbl(T): T' read from the slot (48), then l0 l1 l3 as EACH pair of the group returned them, 48
 *                               words per pair in pair order (pair = lane / 2; pairs 6 and 7 of every 16 lanes are the shadow pairs)
 *           words STEP          w_line_add(T, Q), likewise
 *           words 2 STEP        f after var_line_mul_w with the tangent's line (96)
 *           words 2 STEP + 96   f after fixed_lines_mul_w with (do_l, do_c) = (1, 1), (1, 0), (0, 1) (3 x 96)
 *           words 2 STEP + 384  f after f12m_inv_w (96)
 *           words 2 STEP + 480  T after w_line_dbl, w_line_add(Q), w_line_dbl (48) */
int zkv_diag_primitive(int device, int mapping, int op, size_t n, const uint32_t* in, uint32_t* out);

#ifdef __cplusplus
}
#endif
#endif /* ZKV_DIAG_PRIMITIVE_H */

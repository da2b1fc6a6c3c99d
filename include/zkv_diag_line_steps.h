/*
 * zkv_diag_line_steps.h -- known-answer harness of the tangent and chord steps of k_miller2 as fused column sums.  TEST ONLY: no
 * verification path uses it.
 *
 * Companion of zkv_diag_primitive.h (same library, same ZKV_OK / ZKV_ERR_* codes, same word conventions): mapping 1 op 8 of
 * zkv_diag_primitive runs the packed line steps line_dbl / line_add that every other kernel keeps; this entry runs, on the same input
 * row, the bodies k_miller2 takes instead (stylus_zkvm_verifiers_amd/csrc/zkv_line_sums.h), which hand over the SCALED line coefficients
 * c3 = l1 xs and c4 = l3 ys.  The case body is selftest_line_sums in stylus_zkvm_verifiers_amd/csrc/zkv_selftest.h.
 */
#ifndef ZKV_DIAG_LINE_STEPS_H
#define ZKV_DIAG_LINE_STEPS_H
#include "zkv_diag_primitive.h"

#ifdef __cplusplus
extern "C" {
#endif

#define ZKV_DIAG_LINE_STEPS_IN 192       /* words per case in */
#define ZKV_DIAG_LINE_STEPS_OUT 624      /* words per case out */

/* Synchronous, host buffers: runs n cases (1 <= n <= ZKV_DIAG_PRIMITIVE_MAX_CASES), one case per lane pair (the even lane holds c0, the
 * odd lane c1).  ZKV_ERR_INVALID_ARG for n = 0, n > 65,536 or a NULL buffer (checked before anything is launched); ZKV_ERR_NO_DEVICE
 * without a gfx950 device.  Every Fp word of the operands must be below 2p, and every Fp word returned is below 2p.
 *   in   T (homogeneous X Y Z, 48) Q (x y, 32) xs ys (Fp, 8 each) f (Fp12, 96) (192): the row of zkv_diag_primitive mapping 1 op 8
 *   out  the G2 steps as miller_loop_p<true> runs them, T in the LDS slot of k_miller2, Q and the scalings re-read through their SoaRef
 *        rows, f in an LDS slot; every step starts from the input T (624):
 *        words   0  the tangent step as T' (read back from the slot) l0 c3 c4 (96)
 *        words  96  the chord steps of kinds 1 2 3 4 -- with Q, -Q, psi(Q), -psi^2(Q) -- likewise (4 x 96)
 *        words 480  f after f12m_mul_by_034_body with the tangent's l0 c3 c4 (96)
 *        words 576  T after tangent, chord(Q), tangent (48) */
int zkv_diag_line_steps(int device, size_t n, const uint32_t* in, uint32_t* out);

#ifdef __cplusplus
}
#endif
#endif /* ZKV_DIAG_LINE_STEPS_H */

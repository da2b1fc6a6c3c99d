/*
 * zkv_diag_gt.h -- read-back of the fixed-base GT tables of an SP1 / RISC Zero context (zkv.h, "GT tables") and of the product the final
 * exponentiation kernel forms from them.  TEST ONLY: no verification path uses it.  Companion of zkv.h (same library, same codes).
 */
#ifndef ZKV_DIAG_GT_H
#define ZKV_DIAG_GT_H
#include "zkv.h"

#ifdef __cplusplus
extern "C" {
#endif

#define ZKV_DIAG_GT_ENTRY_WORDS 96

/* out6 = {tables built (0 / 1), windows of signal 0, windows of signal 1, table bytes on the device, build time in microseconds,
 * build attempted (0 / 1: a context builds its tables the first time a call can run lane-pair chunks)}. */
int zkv_diag_gt_info(zkv_ctx* ctx, uint64_t* out6);

/* Synchronous copy of one stored value, 96 uint32 words: an Fp12 as six Fp2 coefficients g0 g1 g2 h0 h1 h2 (the element is
 * sum g_k v^k + (sum h_k v^k) w with v^3 = 9 + u, w^2 = v), each as (real, imaginary), each Fp as 8 little-endian limbs in Montgomery
 * form with R = 2^261, value below 2p (either representative).
 *   signal = 0 / 1, window < that signal's window count, 1 <= d <= 2^19:  the entry G^(d 2^(20 window)), G being the library's final
 *       exponentiation of the Miller value of (IC_signal, gamma): e(IC_signal, gamma)^k, k = 2u(6u^2 + 3u + 1);
 *   signal < 0:  the folded MILLER constant the lane-pair Miller kernel multiplies in, ML(alpha, beta) * ML(base, gamma) (not yet
 *       exponentiated: compare after a final exponentiation).
 * ZKV_ERR_INVALID_ARG: NULL arguments, a context without tables, an index out of range. */
int zkv_diag_gt_read(zkv_ctx* ctx, int signal, uint32_t window, uint32_t d, uint32_t* out96);

/* The product M the lane-pair final exponentiation kernel forms for given signals: n proofs (1 <= n <= the context's workspace capacity,
 * i.e. at most the largest batch it has verified) are given the Miller value 1, the verify path's own kernel runs on them -- n proofs on
 * consecutive lane pairs, 32 per wavefront --, and the accumulator it tests against 1 is read back.
 *   scalars: n x 2 x 8 uint32, signal 0 then signal 1 of each proof, least significant word first; each below 2^(20 windows - 1)
 *   out:     n x 96 uint32, M = G_0^(s_0) G_1^(s_1) per proof in the layout of zkv_diag_gt_read (G_i as defined there)
 * Overwrites the context's workspace (no call may be in flight).  ZKV_ERR_INVALID_ARG: NULL arguments, a context without tables, n out of
 * range, a scalar too large. */
int zkv_diag_gt_product(zkv_ctx* ctx, size_t n, const uint32_t* scalars, uint32_t* out);

/* The walk-prefix cache of an SP1 context with tables (the u the walk holds after signal 0's windows, kept per program vkey):
 * out3 = {entries that hold a value, insertions so far, entries the cache can hold}.  All 0 for a context without one (RISC Zero, no
 * tables, ZKV_GT_CACHE=0).  Waits for the device.  zkv_diag_gt_product runs the cache's stages like a verify call: it may insert, and it
 * reads back what the cached path computes. */
int zkv_diag_gt_cache(zkv_ctx* ctx, uint64_t* out3);

#ifdef __cplusplus
}
#endif
#endif /* ZKV_DIAG_GT_H */

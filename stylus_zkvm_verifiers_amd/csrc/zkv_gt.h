// Fixed-base GT tables for the (vk_x, gamma) pairing of the SP1 and RISC Zero contexts (lane-pair chunks only).
//
// vk_x = base + sum_i s_i IC_i with context-fixed points, so e(vk_x, gamma) = e(base, gamma) * prod_i e(IC_i, gamma)^(s_i): the first factor
// is folded into the per-context Miller constant beside e(alpha, beta), and every power is a walk over signed 20-bit windows of s_i,
//     s = sum_j d_j 2^(20 j),  |d_j| <= 2^19,        e(IC_i, gamma)^s = prod_j T_i,j[|d_j|]^(sign d_j),
// with T_i,j[d] = G_i^(d 2^(20 j)), d = 1 .. 2^19, tabulated at set-up (k_gt.hip).  G_i is what the final exponentiation of this library
// makes of the Miller value of (IC_i, gamma) -- e(IC_i, gamma)^k with the fixed k = 2u(6u^2 + 3u + 1) of final_exp_is_one_m --, so the
// product M of a proof's entries multiplies the exponentiated value of the other pairs: FE(f_AB f_Cdelta m_const) * M == 1.  Entries
// are unitary (GT is in the cyclotomic subgroup): a negative digit multiplies by the conjugate.
//
// TORUS-COMPRESSED ENTRIES.  Fp12 = Fp6[w] / (w^2 - v), an element is g + h w.  A unitary t = g + h w other than +-1 is (a + w) / (a - w) with
// a = (1 + g) / h in Fp6 (its affine torus value; (a + w)^2 / (a^2 - v) has g = (a^2 + v) / (a^2 - v), h = 2 a / (a^2 - v)), and t^-1 = conj(t) has
// the value -a.  Every entry is G^(d 2^(20 j)) with G of prime order R and d 2^(20 j) no multiple of R, so no entry is +-1, h is invertible and
// a is finite and nonzero.  The tables hold a, and the walk carries an ordinary Fp12 value u = N + D w standing for M = u / conj(u):
//     start u = 1;   one window with digit d and entry a:   u <- u (sigma a + w), sigma = sign(d):   N' = sigma N a + v D,  D' = N + sigma a D
// -- conj(u') = conj(u)(sigma a - w), so M' = M t^sigma --, two Fp6 products where the full entry took three, and no conjugation for a
// negative digit.  u never becomes 0 (that would need a^2 = v, and v is no square in Fp6).  The test FE * M == 1 becomes FE * u == conj(u)
// (conj(u) is invertible: its norm is N^2 - v D^2 != 0): one Fp12 product and a comparison close the walk (final_exp_prog_p, zkv_verify.h).
// An entry keeps its 384-byte place (the geometry below is what the host tests pin): a0 a1 a2, (c0, c1) each, in the first 192 bytes, which is
// all the walk fetches; the second 192 bytes are unused after the build's last step (k_gt_torus) -- they still hold h of the full form, which
// nothing reads.  Halving the tables means changing that geometry and the tests that pin it.
//
// This header is plain C++ (the recoding and the table indexing are tested on the host).
#pragma once
#include <stdint.h>
#include <stddef.h>

#if defined(__HIPCC__)
#define ZKV_GT_HD __host__ __device__ __forceinline__
#else
#define ZKV_GT_HD inline
#endif

namespace zkv {

constexpr uint32_t GT_WINDOW_BITS = 20;
constexpr uint32_t GT_ROW_ENTRIES = 1u << (GT_WINDOW_BITS - 1);     // d = 1 .. 2^19 at index d - 1
constexpr uint32_t GT_ENTRY_WORDS = 96;                             // an entry's place, 384 contiguous bytes: one Fp12 while the tables are built, then a0 a1 a2 in the first 192
constexpr uint32_t GT_MAX_SIG = 2;                                  // RISC Zero and SP1 have two per-proof signals
constexpr uint32_t GT_MAX_WINDOWS = 13;                             // 13 x 20 = 260 bits
constexpr size_t GT_ROW_BYTES = (size_t)GT_ROW_ENTRIES * GT_ENTRY_WORDS * 4;     // 201,326,592: below 2^32, a lane addresses its entry by a 32-bit offset

// Windows of a signal of `bits` bits: the top window must take the last carry, i.e. the signal is below 2^(20 n - 1).
ZKV_GT_HD uint32_t gt_windows(uint32_t bits) { return bits / GT_WINDOW_BITS + 1; }

// Signed digit j of a scalar given as 32-bit words, least significant first (word(k), k = 0 .. 7): with w_j the j-th 20-bit window,
//     d_j = w_j + bit(20 j - 1) - 2^20 bit(20 j + 19):
// a window whose top bit is set hands a carry to the next one and becomes negative.  The carry into window j is a bit of the scalar itself,
// so a digit needs no state from the windows below it.  |d_j| <= 2^19, and sum d_j 2^(20 j) telescopes to the scalar as long as the top
// window's top bit is clear (gt_windows).
// gt_digit_word(j): the first of the two consecutive scalar words digit j is cut from; gt_digit_of(lo, hi, j): the digit, given that word
// and the next one (0 beyond word 7).
ZKV_GT_HD uint32_t gt_digit_word(uint32_t j) { return j == 0 ? 0u : (GT_WINDOW_BITS * j - 1u) >> 5; }
ZKV_GT_HD int32_t gt_digit_of(uint32_t lo, uint32_t hi, uint32_t j) {
    const uint64_t two = (uint64_t)lo | ((uint64_t)hi << 32);
    // v = bits 20 j - 1 .. 20 j + 19 of the scalar (bit -1 is 0)
    const uint64_t v = j == 0 ? (two & 0xfffffu) << 1 : (two >> ((GT_WINDOW_BITS * j - 1u) & 31u)) & 0x1fffffu;
    return (int32_t)((v >> 1) & 0xfffffu) + (int32_t)(v & 1u) - (int32_t)(((v >> 20) & 1u) << 20);
}
ZKV_GT_HD int32_t gt_digit(const uint32_t s[8], uint32_t j) {
    const uint32_t k = gt_digit_word(j);
    return gt_digit_of(s[k], k + 1 < 8 ? s[k + 1] : 0u, j);
}

// Byte offset of the entry of digit magnitude m (1 .. 2^19) inside its window's sub-table.
ZKV_GT_HD uint32_t gt_entry_offset(uint32_t m) { return (m - 1u) * (GT_ENTRY_WORDS * 4u); }
// First word of window `row`'s sub-table (rows: signal 0's windows, then signal 1's).
ZKV_GT_HD size_t gt_row_word(uint32_t row) { return (size_t)row * GT_ROW_ENTRIES * GT_ENTRY_WORDS; }

// What the kernels get: the tables (nullptr: none, the Miller loop takes the pair), the folded Miller constant
// ML(alpha, beta) * ML(base, gamma) (96 words, the layout of VkTables::f_alpha_beta) and the window counts of the two signals.
struct GtTab { const uint32_t* tab; const uint32_t* mconst; uint32_t nw[GT_MAX_SIG]; };

}  // namespace zkv

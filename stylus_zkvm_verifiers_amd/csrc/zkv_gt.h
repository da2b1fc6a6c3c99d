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

// WALK-PREFIX CACHE (SP1 contexts only).  Signal 0 of an SP1 proof is the program vkey, which a deployment repeats from proof to proof, so
// the u the walk holds after signal 0's windows (starting from u = 1) is the same Fp12 value for every proof of a program.  A context keeps
// GT_CACHE_ENTRIES of them on the device, keyed by the eight words of signal 0: k_gt_cache_fill inserts at most one per chunk, k_gt_cache_tag
// writes one byte per proof (0: miss, 1 + slot: hit), and a hit lane of k_finalexp2 starts its walk from the stored u with signal 0's digits
// taken as 0 (final_exp_prog_p).  Signal 1 (the hash of the public values) differs for every proof in real use and is never cached; RISC
// Zero's signals are halves of a claim digest, and its contexts have no cache.
// The selection below is plain C++ and is what the fill kernel runs: up to GT_CACHE_SAMPLES proofs of a chunk are sampled at evenly spread
// positions; a sample is a candidate if it is usable (its proof alive, i.e. its scalar passed PREP's range check), its key is not cached
// and the same key occurs in another usable sample; the lowest-indexed candidate is inserted at the round-robin cursor.  A chunk whose
// vkeys are all distinct inserts nothing.
constexpr uint32_t GT_CACHE_ENTRIES = 4;                            // a tag byte holds 1 + slot
constexpr uint32_t GT_CACHE_SAMPLES = 32;                           // one per lane pair of the fill kernel's wavefront
struct GtCache {
    uint32_t cursor, fills, entries, pad;                           // next slot to fill, insertions so far, GT_CACHE_ENTRIES
    uint32_t valid[GT_CACHE_ENTRIES];
    uint32_t key[GT_CACHE_ENTRIES][8];                              // signal 0, least significant word first
    uint32_t val[GT_CACHE_ENTRIES][GT_ENTRY_WORDS];                 // u = N + D w in the packed layout of the final exponentiation's slots
};
// Samples of a chunk of n proofs and the proof sample k (< gt_cache_samples(n)) looks at: chunks under 32 proofs sample each proof once.
ZKV_GT_HD uint32_t gt_cache_samples(size_t n) { return n < GT_CACHE_SAMPLES ? (uint32_t)n : GT_CACHE_SAMPLES; }
ZKV_GT_HD size_t gt_cache_sample_pos(size_t n, uint32_t k) { return (size_t)(((unsigned long long)k * n) / gt_cache_samples(n)); }
ZKV_GT_HD bool gt_key_eq(const uint32_t* a, const uint32_t* b) {
    uint32_t d = 0;
    for (int k = 0; k < 8; k++) d |= a[k] ^ b[k];
    return d == 0;
}
// 1 + the slot that holds `key`, 0 if none does (the tag byte)
ZKV_GT_HD uint32_t gt_cache_find(const GtCache& c, const uint32_t* key) {
    uint32_t t = 0;
    for (uint32_t e = GT_CACHE_ENTRIES; e-- > 0;) if (c.valid[e] && gt_key_eq(c.key[e], key)) t = e + 1u;
    return t;
}
// keys: m x 8 words, ok[k] != 0: sample k is usable
ZKV_GT_HD bool gt_cache_candidate(const GtCache& c, const uint32_t* keys, const uint32_t* ok, uint32_t m, uint32_t k) {
    if (k >= m || !ok[k] || gt_cache_find(c, keys + 8 * k)) return false;
    for (uint32_t o = 0; o < m; o++) if (o != k && ok[o] && gt_key_eq(keys + 8 * k, keys + 8 * o)) return true;
    return false;
}
// the sample to insert, -1: none
ZKV_GT_HD int gt_cache_select(const GtCache& c, const uint32_t* keys, const uint32_t* ok, uint32_t m) {
    for (uint32_t k = 0; k < m; k++) if (gt_cache_candidate(c, keys, ok, m, k)) return (int)k;
    return -1;
}
// Takes the slot at the cursor for `key` (evicting what it held) and returns it; the caller stores the value there.
ZKV_GT_HD uint32_t gt_cache_claim(GtCache& c, const uint32_t* key) {
    const uint32_t slot = c.cursor % GT_CACHE_ENTRIES;
    for (int k = 0; k < 8; k++) c.key[slot][k] = key[k];
    c.valid[slot] = 1u;
    c.cursor = (slot + 1u) % GT_CACHE_ENTRIES;
    c.fills += 1u;
    return slot;
}

// What the kernels get: the tables (nullptr: none, the Miller loop takes the pair), the folded Miller constant
// ML(alpha, beta) * ML(base, gamma) (96 words, the layout of VkTables::f_alpha_beta; the 96 words behind it hold the start value of the
// lane-pair Miller loop made of it, miller_start_value in zkv_verify.h), the window counts of the two signals and the
// walk-prefix cache (nullptr: none).
struct GtTab { const uint32_t* tab; const uint32_t* mconst; uint32_t nw[GT_MAX_SIG]; GtCache* cache; };

}  // namespace zkv

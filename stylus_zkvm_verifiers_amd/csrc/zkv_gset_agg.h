// Aggregate check on Groth16 key sets (zkv_ctx_set_aggregate_check on a set): the scalar-sum form of
// sum_i r_i vk_x_i for keys of any signal count, shared by the device (k_gset_agg.hip) and the host build of the tests
// (tests/host_sim/host_sim_gset_agg.cpp).
//
// Every sub-batch holds proofs of one key, so sum_i r_i vk_x_i = R IC_0 + sum_b T_b IC_b with R = sum_i r_i and T_b = sum_i r_i s_ib
// (mod r).  The `sub` lanes of a sub-batch take the key's signals one at a time: a lane multiplies its proof's signal by its r_i, a
// butterfly sums the products into T_b, and the lane adds the table entries of windows lane, lane + sub, ... of T_b (the set's 8-bit
// long-key rows of IC_b) to its share of U; R IC_0 comes from the key's AggTables::base_win the same way.  The lanes' shares add up
// to U: per proof one Fr product per signal, per sub-batch 32 look-ups per signal, and no per-proof vk_x.
#pragma once
#include "zkv_agg.h"

namespace zkv {

// Windows lane, lane + sub, ... of T (canonical, 8 limbs) in one signal's rows (row: LONG_ROW_ENTRIES entries; win: 32, or 0 when
// IC_b is the point at infinity), added to acc
ZKV_HD G1J gset_agg_sig_share(G1J acc, const G1A* row, uint32_t win, const uint32_t T[8], uint32_t lane, uint32_t sub) {
#pragma unroll 1
    for (uint32_t w = lane; w < win; w += sub) {
        const uint32_t d = (T[w >> 2] >> ((w & 3u) * 8u)) & 255u;
        if (d) { const G1A e = row[(size_t)w * MSM_DIGITS + d]; acc = g1j_add_affine(acc, e.x, e.y); }
    }
    return acc;
}
// ... and of R in the key's IC_0 rows (nothing when IC_0 is the point at infinity)
ZKV_HD G1J gset_agg_base_share(G1J acc, const AggTables& t, uint32_t base_inf, const uint32_t R[8], uint32_t lane, uint32_t sub) {
    if (base_inf) return acc;
#pragma unroll 1
    for (uint32_t w = lane; w < (uint32_t)MSM_MAX_WINDOWS; w += sub) {
        const uint32_t d = (R[w >> 2] >> ((w & 3u) * 8u)) & 255u;
        if (d) { const G1A e = t.base_win[w][d]; acc = g1j_add_affine(acc, e.x, e.y); }
    }
    return acc;
}

}  // namespace zkv

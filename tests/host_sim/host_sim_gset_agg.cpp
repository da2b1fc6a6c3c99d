// Host build of the key-set aggregate layout (csrc/zkv_gset_layout.h: gset_agg_choose, gset_agg_slot, gset_agg_chunk_plan) and of the per-signal share loop
// of the scalar-sum form (csrc/zkv_gset_agg.h) for tests/test_groth16_key_sets_aggregate_host.py.  TEST ONLY.
#include <stdint.h>
#include <string.h>
#include <vector>
#include "../../stylus_zkvm_verifiers_amd/csrc/zkv_host_vk.h"
#include "../../stylus_zkvm_verifiers_amd/csrc/zkv_gset_layout.h"
#include "../../stylus_zkvm_verifiers_amd/csrc/zkv_gset_agg.h"
using namespace zkv;

extern "C" int hga_choose(const uint32_t* cnt, const uint8_t* capable, uint32_t n_keys, uint32_t sub, int lanes, uint32_t* agg, uint64_t* astart,
                          uint32_t* rest, uint64_t* pstart, uint64_t* agg_slots, uint64_t* slots) {
    return gset_agg_choose(cnt, capable, n_keys, sub, lanes, 0, agg, astart, rest, pstart, agg_slots, slots);
}
extern "C" uint64_t hga_slot(uint32_t k, uint32_t rank, const uint32_t* agg, const uint64_t* astart, const uint64_t* pstart) {
    return gset_agg_slot(k, rank, agg, astart, pstart);
}

// The pseudo-proof plan of one aggregate chunk (gset_agg_chunk_plan), for both kinds of set: rep = null for a Groth16 set's key regions
extern "C" int hga_chunk_plan(const uint64_t* beg, const uint64_t* end, const uint32_t* rep, uint32_t n_regions, uint64_t base, uint64_t m, uint32_t sub,
                              int lanes, uint64_t cap, uint32_t* nsb, uint64_t* pst, uint32_t* psl, uint32_t* skey2, uint64_t* slots) {
    return gset_agg_chunk_plan(beg, end, rep, n_regions, base, m, sub, lanes, cap, nsb, pst, psl, skey2, slots);
}

// One sub-batch of `sub` proofs under a key with n_sig signals: ic (n_sig + 1 affine points, 16 big-endian words each... as raw limbs:
// x then y, 8 limbs each), r (sub raw scalars < r), s (sub x n_sig raw scalars < r).  Every lane's share (per signal: the product r_i s_ib,
// the sum over the lanes, the look-ups of gset_agg_sig_share; then R IC_0 by gset_agg_base_share), the shares added; out64: x, y big-endian.
static void fp_to_be(uint8_t* o, const Fp& a) {
    uint32_t r[8];
    fp_to_raw(r, a);
    for (int k = 0; k < 8; k++) { uint32_t v = r[7 - k]; o[4 * k] = v >> 24; o[4 * k + 1] = v >> 16; o[4 * k + 2] = v >> 8; o[4 * k + 3] = v; }
}
extern "C" int hga_u(uint32_t n_sig, uint32_t sub, const uint32_t* ic, const uint32_t* r, const uint32_t* s, uint8_t* out64) {
    std::vector<G1A> rows((size_t)(n_sig ? n_sig : 1) * LONG_ROW_ENTRIES);
    std::vector<uint32_t> win(n_sig ? n_sig : 1);
    for (uint32_t b = 0; b < n_sig; b++)
        for (uint32_t w = 0; w < (uint32_t)MSM_MAX_WINDOWS; w++)
            setup_long_row((const uint32_t(*)[8])(ic + 16 * (b + 1)), w, rows.data() + ((size_t)b * MSM_MAX_WINDOWS + w) * MSM_DIGITS, &win[b]);
    static AggTables t;                                         // (512 KB: not on the stack)
    VkTables* vk = new VkTables();
    vk->base_inf = raw_g1_is_inf((const uint32_t(*)[8])ic) ? 1u : 0u;
    if (!vk->base_inf) { vk->base.x = fp_from_raw(ic); vk->base.y = fp_from_raw(ic + 8); }
    for (int w = 0; w < MSM_MAX_WINDOWS; w++) setup_agg_base_row(*vk, t, w);
    std::vector<Fr> rm(sub);
    Fr Rs = fr_zero();
    for (uint32_t i = 0; i < sub; i++) { rm[i] = fr_from_raw(r + 8 * i); Rs = fr_add(Rs, rm[i]); }
    std::vector<G1J> share(sub, g1j_infinity());
    for (uint32_t b = 0; b < n_sig; b++) {
        Fr T = fr_zero();
        for (uint32_t i = 0; i < sub; i++) T = fr_add(T, fr_mul(fr_from_raw(s + 8 * ((size_t)i * n_sig + b)), rm[i]));
        uint32_t Tr[8];
        fr_to_raw(Tr, T);
        for (uint32_t lane = 0; lane < sub; lane++)
            share[lane] = gset_agg_sig_share(share[lane], rows.data() + (size_t)b * LONG_ROW_ENTRIES, win[b], Tr, lane, sub);
    }
    uint32_t R[8];
    fr_to_raw(R, Rs);
    G1J U = g1j_infinity();
    for (uint32_t lane = 0; lane < sub; lane++) U = g1j_add(U, gset_agg_base_share(share[lane], t, vk->base_inf, R, lane, sub));
    delete vk;
    G1A a; uint32_t inf;
    g1j_to_affine(U, a, inf);
    fp_to_be(out64, a.x); fp_to_be(out64 + 32, a.y);
    return inf ? 1 : 0;
}

// Aggregate check on PLONK key sets (include/zkv_plonk_set_agg.h).  A PLONK proof's pairing equation
// e(D, [1]_2) e(-Q, [tau]_2) == 1 has two FIXED pairs, and the key gives it nothing but those two G2 points, so a sub-batch may hold proofs
// of any keys of one SRS class (zkv_gset_layout.h pset_agg_choose): prod_i (e(D_i, [1]_2) e(-Q_i, [tau]_2))^{r_i} =
// e(sum r_i D_i, [1]_2) e(sum r_i (-Q_i), [tau]_2), no per-proof Miller loop.  PREP is k_pset_prep and the per-proof G1 stage k_agg_plonk_g1,
// both unchanged (they work slot by slot; a pad slot's flags are 0); the verdicts and the in-place second pass are k_gset_agg_mark's.
// This unit: the per-sub-batch sums with the pseudo-proof at the slot the class layout gives it (psl[sb]), so that k_gset_miller* run the
// pseudo-proofs of one class per wavefront, and the sums of 128 / 256-slot sub-batches.  A translation unit of its own, so that every
// existing kernel compiles exactly as before.  Parity unpinned by construction (no PLONK in the reference).
#include "zkv_internal.h"
#include "zkv_agg.h"

namespace zkv {

__device__ __forceinline__ G1J pa_xor(const G1J& p, int mask) {
    G1J r;
#pragma unroll
    for (int k = 0; k < 8; k++) {
        r.x.v[k] = (uint32_t)__shfl_xor((int)p.x.v[k], mask, 64);
        r.y.v[k] = (uint32_t)__shfl_xor((int)p.y.v[k], mask, 64);
        r.z.v[k] = (uint32_t)__shfl_xor((int)p.z.v[k], mask, 64);
    }
    return r;
}
__device__ __forceinline__ G1J pa_ld_g1j(const uint32_t* rows, size_t cap, int word0, size_t i) {
    G1J p; p.x = ws_ld(rows, cap, word0, i); p.y = ws_ld(rows, cap, word0 + 8, i); p.z = ws_ld(rows, cap, word0 + 16, i);
    return p;
}
// The rows of one pseudo-proof at slot q of ws2: no (A, B) pair, U = sum r_i D_i against [1]_2 (the gamma slot of the class's tables),
// W = sum r_i (-Q_i) against [tau]_2 (the delta slot)
__device__ __forceinline__ void pa_pseudo(const G1J& U, const G1J& W, const Workspace& ws2, size_t q) {
    uint32_t flags = FL_ALIVE | FL_B_INF;
    G1Norm o;
    agg_normalize3(g1j_infinity(), U, W, flags, o);
    ws_st(ws2.norm, ws2.cap, 0, q, o.axs); ws_st(ws2.norm, ws2.cap, 8, q, o.ays);
    ws_st(ws2.norm, ws2.cap, 16, q, o.lxs); ws_st(ws2.norm, ws2.cap, 24, q, o.lys);
    ws_st(ws2.norm, ws2.cap, 32, q, o.cxs); ws_st(ws2.norm, ws2.cap, 40, q, o.cys);
    ws2.flags[q] = flags;
}

// One wavefront per 64 slots = 64 / sub sub-batches (sub = 16, 32 or 64; m a multiple of 64).  Lane l holds slot 64 blockIdx + l of the
// chunk: its scaled points if the slot holds a proof that PREP left alive, nothing otherwise (pad slots, rejected proofs, proofs of a
// failed key: their saved flags word is 0).  Butterflies inside each group of `sub` lanes give the sums; the group's first lane writes the
// pseudo-proof to slot psl[sb] of ws2, or (park: sub-batches of 128 / 256 slots) the 64-slot sums to row blockIdx of ws2.fe for
// k_pset_agg_combine.  A sub-batch with nothing alive is switched off.
__global__ __launch_bounds__(ZKV_BLOCK) void k_pset_agg_reduce(size_t m, uint32_t sub, Workspace ws, const uint32_t* __restrict__ agg, Workspace ws2,
                                                               uint8_t* __restrict__ status2, const uint32_t* __restrict__ psl, uint32_t park) {
    const size_t i = (size_t)blockIdx.x * ZKV_BLOCK + threadIdx.x;
    const uint32_t lane = threadIdx.x & (sub - 1u);
    const size_t sb = (size_t)blockIdx.x * (64u / sub) + threadIdx.x / sub;
    const bool in = i < m && (agg[(size_t)AGG_W_FLAGS * ws.cap + i] & FL_ALIVE);
    G1J U = g1j_infinity(), W = g1j_infinity();
    uint32_t cnt = in ? 1u : 0u;
    if (in) { U = pa_ld_g1j(agg, ws.cap, AGG_W_U, i); W = pa_ld_g1j(agg, ws.cap, AGG_W_W, i); }
#pragma unroll 1
    for (uint32_t d = sub >> 1; d >= 1u; d >>= 1) {
        U = g1j_add(U, pa_xor(U, (int)d));
        W = g1j_add(W, pa_xor(W, (int)d));
        cnt += (uint32_t)__shfl_xor((int)cnt, (int)d, 64);
    }
    if (lane != 0) return;
    if (park) {                                                 // (ws2.fe is unused until the pseudo-proofs' final exponentiation)
        uint32_t* row = ws2.fe;
        const size_t pb = blockIdx.x;
        ws_st(row, ws2.cap, 24, pb, U.x); ws_st(row, ws2.cap, 32, pb, U.y); ws_st(row, ws2.cap, 40, pb, U.z);
        ws_st(row, ws2.cap, 48, pb, W.x); ws_st(row, ws2.cap, 56, pb, W.y); ws_st(row, ws2.cap, 64, pb, W.z);
        row[(size_t)72 * ws2.cap + pb] = cnt;
        return;
    }
    const size_t q = psl[sb];
    ws2.g2bad[q] = 0;
    if (cnt == 0) { ws2.flags[q] = 0; status2[q] = ST_OK; return; }
    pa_pseudo(U, W, ws2, q);
    status2[q] = ST_VERIFICATION_FAILED;
}
// Sub-batch j of `wide` = 2 / 4 parked 64-slot blocks becomes the pseudo-proof at slot psl[j] (n2 = m / (64 wide) sub-batches)
__global__ __launch_bounds__(ZKV_BLOCK) void k_pset_agg_combine(size_t n2, uint32_t wide, Workspace ws2, uint8_t* __restrict__ status2,
                                                                const uint32_t* __restrict__ psl) {
    const size_t j = (size_t)blockIdx.x * ZKV_BLOCK + threadIdx.x;
    if (j >= n2) return;
    const uint32_t* row = ws2.fe;
    G1J U = g1j_infinity(), W = g1j_infinity();
    uint32_t cnt = 0;
#pragma unroll 1
    for (uint32_t t = 0; t < wide; t++) {
        const size_t pb = j * wide + t;
        const uint32_t cb = row[(size_t)72 * ws2.cap + pb];
        if (!cb) continue;
        cnt += cb;
        U = g1j_add(U, pa_ld_g1j(row, ws2.cap, 24, pb));
        W = g1j_add(W, pa_ld_g1j(row, ws2.cap, 48, pb));
    }
    const size_t q = psl[j];
    ws2.g2bad[q] = 0;
    if (cnt == 0) { ws2.flags[q] = 0; status2[q] = ST_OK; return; }
    pa_pseudo(U, W, ws2, q);
    status2[q] = ST_VERIFICATION_FAILED;
}

void launch_pset_agg_reduce(size_t m, uint32_t sub, const Workspace& ws, const uint32_t* agg, const Workspace& ws2, uint8_t* status2, const uint32_t* psl,
                            bool park, hipStream_t s) {
    if (!m) return;
    hipLaunchKernelGGL(k_pset_agg_reduce, dim3((unsigned)((m + ZKV_BLOCK - 1) / ZKV_BLOCK)), dim3(ZKV_BLOCK), 0, s, m, sub, ws, agg, ws2, status2, psl,
                       park ? 1u : 0u);
}
void launch_pset_agg_combine(size_t n2, uint32_t wide, const Workspace& ws2, uint8_t* status2, const uint32_t* psl, hipStream_t s) {
    if (!n2) return;
    hipLaunchKernelGGL(k_pset_agg_combine, dim3((unsigned)((n2 + ZKV_BLOCK - 1) / ZKV_BLOCK)), dim3(ZKV_BLOCK), 0, s, n2, wide, ws2, status2, psl);
}

}  // namespace zkv

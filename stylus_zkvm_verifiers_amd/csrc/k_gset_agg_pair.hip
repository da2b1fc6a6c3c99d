// Aggregate check on Groth16 key sets, the lane-pair kernels: k_agg_miller and k_agg_fprod (k_pair.hip) for the aggregate region of a set
// call (k_gset_agg.hip).  The Miller loop of the variable pair reads no key; the ML(alpha, beta) factor is the slot's key's.  The product of
// a sub-batch's Miller values goes to its pseudo-proof's slot psl[sb].
#define ZKV_PAIRED 1
#include "zkv_internal.h"
#include "zkv_agg.h"

namespace zkv {

constexpr int GA_PAIR_BLOCK = ZKV_BLOCK;       // one wavefront per workgroup (k_pair.hip's PAIR_BLOCK at its default)

// k_agg_miller<G> with skey (chunk-relative): G proofs per lane pair share one accumulator, pair q of a 64-proof block taking proofs q + p L.
// A wavefront covers 32 pairs, which is 32 / L blocks (G = 4, 8: two or four blocks, maybe of different keys), so f_alpha_beta is read through
// the pair's own key; the block's G proofs are of one key by the layout.
template <int G>
__global__ __launch_bounds__(GA_PAIR_BLOCK, 2) void k_gset_agg_miller(size_t n, const uint32_t* __restrict__ skey, const GsetKey* __restrict__ keys, Workspace ws,
                                                                      uint8_t* __restrict__ status) {
    __shared__ uint32_t lds[48 * GA_PAIR_BLOCK];
    constexpr uint32_t L = 64u / G;
    const size_t gp = ((size_t)blockIdx.x * GA_PAIR_BLOCK + threadIdx.x) >> 1;
    const size_t i0 = (gp / L) * 64 + (gp % L);
    if (i0 >= n) return;
    uint32_t alive = 0, mask = 0, abmask = 0;
#pragma unroll
    for (uint32_t p = 0; p < (uint32_t)G; p++) {
        const size_t i = i0 + p * L;
        const uint32_t f = i < n ? ws.flags[i] : 0u;
        if (f & FL_ALIVE) {
            alive |= 1u << p;
            if (!(f & FL_B_INF)) { mask |= 1u << p; if (!(f & FL_A_INF)) abmask |= 1u << p; }
        }
    }
    if (!alive) return;
    const uint32_t par = threadIdx.x & 1u;
    uint32_t* wl = lds + (threadIdx.x & 63u);
    LRef fm = l_ref(wl);
    SoaRef norm = {ws.norm, ws.cap, (uint32_t)i0 * 4u};
    SoaRef bsrc = {ws.prep + 32 * ws.cap, ws.cap, (uint32_t)(8 * par * ws.cap + i0) * 4u};
    SoaRW tq = {ws.fe, ws.cap, (uint32_t)(8 * par * ws.cap + i0) * 4u};
    const uint32_t fine = miller_loop_pg<G>(mask, abmask, norm, bsrc, tq, L * 4u, fm);
    if ((fine & mask) != mask) {
        if (!par) {
#pragma unroll 1
            for (uint32_t p = 0; p < (uint32_t)G; p++) {
                if (!((alive >> p) & 1u)) continue;
                const bool bad = ((mask & ~fine) >> p) & 1u;
                ws.g2bad[i0 + p * L] = bad ? 1u : 2u;
                if (bad) status[i0 + p * L] = ST_VERIFICATION_FAILED;
            }
        }
        return;
    }
    const VkTables* vk = keys[skey[i0]].tab;
    MRef ab = m_ref((uint32_t*)(vk->f_alpha_beta) + 8 * par, 1, 16);
    MRef out = m_ref(ws.f + (size_t)(8 * par) * ws.cap + i0, (uint32_t)ws.cap, 16);
    f12m_mul_body(out, fm, ab, false);
}
void launch_gset_agg_miller(size_t n, uint32_t g, const uint32_t* skey, const GsetKey* keys, const Workspace& ws, uint8_t* status, hipStream_t s) {
    if (!n) return;
    const size_t pairs = ((n + 63) / 64) * (64 / g);
    const dim3 grid((unsigned)((2 * pairs + GA_PAIR_BLOCK - 1) / GA_PAIR_BLOCK)), block(GA_PAIR_BLOCK);
    if (g == 8) hipLaunchKernelGGL(k_gset_agg_miller<8>, grid, block, 0, s, n, skey, keys, ws, status);
    else if (g == 4) hipLaunchKernelGGL(k_gset_agg_miller<4>, grid, block, 0, s, n, skey, keys, ws, status);
    else hipLaunchKernelGGL(k_gset_agg_miller<2>, grid, block, 0, s, n, skey, keys, ws, status);
}

// k_agg_fprod with the pseudo-proof of sub-batch sb at slot psl[sb] of ws2
__global__ __launch_bounds__(ZKV_BLOCK, 2) void k_gset_agg_fprod(size_t n, size_t n2, uint32_t sub, uint32_t g, Workspace ws, const uint32_t* __restrict__ agg,
                                                                 Workspace ws2, const uint32_t* __restrict__ psl) {
    __shared__ uint32_t lds[48 * ZKV_BLOCK];
    const size_t sb = ((size_t)blockIdx.x * ZKV_BLOCK + threadIdx.x) >> 1;
    if (sb >= n2) return;
    const size_t q = psl[sb];
    if (!(ws2.flags[q] & FL_ALIVE)) return;
    const uint32_t par = threadIdx.x & 1u;
    LRef acc = l_ref(lds + threadIdx.x);
    MRef P2 = m_ref(ws2.f + (size_t)(8 * par) * ws2.cap + q, (uint32_t)ws2.cap, 16);
    f12m_copy(acc, P2);
    const uint32_t L = 64u / g, w = (sub < 64u ? sub : 64u) / g, nblk = sub > 64u ? sub / 64u : 1u, per = sub > 64u ? 1u : 64u / sub;
#pragma unroll 1
    for (uint32_t b = 0; b < nblk; b++) {
        const size_t i0 = sub > 64u ? sb * sub + (size_t)b * 64 : (sb / per) * 64 + (sb % per) * w;
#pragma unroll 1
        for (uint32_t k = 0; k < w; k++) {
            bool in = false;
#pragma unroll 1
            for (uint32_t p = 0; p < g && !in; p++) {
                const size_t i = i0 + k + p * L;
                if (i < n) in = (agg[(size_t)AGG_W_FLAGS * ws.cap + i] & FL_ALIVE) && !ws.g2bad[i];
            }
            if (!in) continue;
            MRef Pi = m_ref(ws.f + (size_t)(8 * par) * ws.cap + i0 + k, (uint32_t)ws.cap, 16);
            f12m_mul(acc, acc, Pi);
        }
    }
    f12m_copy(P2, acc);
}
void launch_gset_agg_fprod(size_t n, size_t n2, uint32_t sub, uint32_t g, const Workspace& ws, const uint32_t* agg, const Workspace& ws2, const uint32_t* psl,
                           hipStream_t s) {
    if (!n2) return;
    hipLaunchKernelGGL(k_gset_agg_fprod, dim3((unsigned)((2 * n2 + ZKV_BLOCK - 1) / ZKV_BLOCK)), dim3(ZKV_BLOCK), 0, s, n, n2, sub, g, ws, agg, ws2, psl);
}

}  // namespace zkv

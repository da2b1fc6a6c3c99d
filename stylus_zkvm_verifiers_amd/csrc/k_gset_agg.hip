// Aggregate check on Groth16 key sets (zkv_ctx_set_aggregate_check on a set).  The check itself is the one of
// zkv_agg.h; what a set adds is a key per sub-batch.  The aggregate region of a call (zkv_gset_layout.h: gset_agg_choose) holds whole
// 64-proof blocks of one key each, and every sub-batch lies inside one key's proofs, so a wavefront of these kernels reads one key
// (readfirstlane of its first slot's key) and the equation of a sub-batch uses that key's alpha, beta, gamma and delta.
// This unit: every key's AggTables, the placement into the two regions, the per-sub-batch reduction with vk_x in the scalar-sum form for
// any signal count (zkv_gset_agg.h), the sums of 128 / 256-proof sub-batches, and the verdicts.  The per-proof G1 stage is k_agg_g1
// (it reads no key); the Miller loops of the proofs and the product of their values are in k_gset_agg_pair.hip; the pseudo-proofs run
// through k_gset_miller* (k_gset_pair.hip) and the single-key final exponentiation.
#include "zkv_internal.h"
#include "zkv_gset_agg.h"

namespace zkv {

// ------------------------------------------------------------------ set-up: k_setup_agg for every key (grid y = key)
__global__ __launch_bounds__(64) void k_gset_setup_agg(const VkRaw* __restrict__ raw, const VkTables* __restrict__ tab, AggTables* __restrict__ t) {
    const uint32_t k = blockIdx.y;
    const int j = blockIdx.x * 64 + threadIdx.x;
    if (j < AGG_ALPHA_POW) setup_agg_alpha(raw[k], t[k], j);
    if (j == AGG_ALPHA_POW) {
        for (int q = 0; q < 4; q++) t[k].beta[q] = fp_from_raw(raw[k].beta[q]);
        t[k].ok = (tab[k].vk_valid && !raw_g1_is_inf(raw[k].alpha) && !raw_g2_is_inf(raw[k].beta)) ? 1u : 0u;
    }
    const int w = j - AGG_ALPHA_POW - 1;
    if (w >= 0 && w < MSM_MAX_WINDOWS) setup_agg_base_row(tab[k], t[k], w);
}
void launch_gset_setup_agg(uint32_t n_keys, const VkRaw* d_raw, const VkTables* d_tabs, AggTables* d_agg, hipStream_t s) {
    hipLaunchKernelGGL(k_gset_setup_agg, dim3(2, n_keys), dim3(64), 0, s, d_raw, d_tabs, d_agg);
}

// ------------------------------------------------------------------ placement into the aggregate and per-proof regions
// k_gset_place with the two-region slot: k_gset_scan (k_gset.hip) ran with zero starts, so off[] holds every (key, block)'s first RANK
// among the key's proofs, and a rank becomes its slot as gset_agg_slot does.  map: astart[K + 1] | pstart[K + 1] | agg[K + 1]
// (64-bit words, zkv_gset_layout.h).
constexpr uint32_t GSET_AGG_MAX_KEYS = 1024;      // (ZKV_GROTH16_SET_MAX_KEYS)
__global__ __launch_bounds__(64) void k_gset_agg_place(GsetPart p, const uint64_t* __restrict__ map) {
    __shared__ uint32_t run[GSET_AGG_MAX_KEYS];
    for (uint32_t k = threadIdx.x; k < p.n_keys; k += 64) run[k] = p.off[(size_t)k * p.blocks + blockIdx.x];
    __syncthreads();
    const uint64_t* astart = map;
    const uint64_t* pstart = map + (p.n_keys + 1);
    const uint64_t* agg = map + 2 * (size_t)(p.n_keys + 1);
    const size_t i0 = (size_t)blockIdx.x * p.per_block;
    const uint32_t lane = threadIdx.x;
#pragma unroll 1
    for (uint32_t t = 0; t < p.per_block; t += 64) {
        const size_t i = i0 + t + lane;
        const bool live = i < p.n;
        uint32_t k = live ? p.key[i] : GSET_NONE;
        if (k >= p.n_keys) k = GSET_NONE;
        uint32_t rank = 0;
        bool last = true;
#pragma unroll 1
        for (uint32_t j = 0; j < 64; j++) {
            const uint32_t kj = (uint32_t)__shfl((int)k, (int)j);
            if (kj == k) { rank += j < lane ? 1u : 0u; last = last && !(j > lane); }
        }
        uint32_t r = 0, slot = GSET_NONE;
        if (k != GSET_NONE) {
            r = run[k] + rank;
            slot = (uint32_t)(r < agg[k] ? astart[k] + r : pstart[k] + (r - agg[k]));
        }
        __syncthreads();
        if (k != GSET_NONE && last) run[k] = r + 1;
        __syncthreads();
        if (live) p.pos[i] = slot;
        if (k != GSET_NONE) { p.idx[slot] = (uint32_t)i; p.skey[slot] = k; }
    }
}
void launch_gset_agg_place(const GsetPart& p, const uint64_t* d_zero, const uint64_t* d_map, hipStream_t s) {
    hipLaunchKernelGGL(k_gset_scan, dim3((p.n_keys + 63) / 64), dim3(64), 0, s, p, d_zero);
    hipLaunchKernelGGL(k_gset_agg_place, dim3(p.blocks), dim3(64), 0, s, p, d_map);
}

// ------------------------------------------------------------------ per sub-batch: sums, U in the scalar-sum form, E, the pseudo-proof
__device__ __forceinline__ G1J ga_xor(const G1J& p, int mask) {
    G1J r;
#pragma unroll
    for (int k = 0; k < 8; k++) {
        r.x.v[k] = (uint32_t)__shfl_xor((int)p.x.v[k], mask, 64);
        r.y.v[k] = (uint32_t)__shfl_xor((int)p.y.v[k], mask, 64);
        r.z.v[k] = (uint32_t)__shfl_xor((int)p.z.v[k], mask, 64);
    }
    return r;
}
__device__ __forceinline__ Fr ga_fr_xor(const Fr& a, int mask) {
    Fr r;
#pragma unroll
    for (int k = 0; k < 8; k++) r.v[k] = (uint32_t)__shfl_xor((int)a.v[k], mask, 64);
    return r;
}
__device__ __forceinline__ G1J ga_ld_g1j(const uint32_t* agg, size_t cap, int word0, size_t i) {
    G1J p; p.x = ws_ld(agg, cap, word0, i); p.y = ws_ld(agg, cap, word0 + 8, i); p.z = ws_ld(agg, cap, word0 + 16, i);
    return p;
}
// The rows of one pseudo-proof (A := E, B := the key's beta, vk_x := U, C := W) at slot q of ws2
__device__ __forceinline__ void ga_pseudo(const G1J& E, const G1J& U, const G1J& W, const AggTables& tab, const Workspace& ws2, size_t q) {
    uint32_t flags = FL_ALIVE;
    G1Norm o;
    agg_normalize3(E, U, W, flags, o);
    ws_st(ws2.norm, ws2.cap, 0, q, o.axs); ws_st(ws2.norm, ws2.cap, 8, q, o.ays);
    ws_st(ws2.norm, ws2.cap, 16, q, o.lxs); ws_st(ws2.norm, ws2.cap, 24, q, o.lys);
    ws_st(ws2.norm, ws2.cap, 32, q, o.cxs); ws_st(ws2.norm, ws2.cap, 40, q, o.cys);
#pragma unroll 1
    for (int k = 0; k < 4; k++) ws_st(ws2.prep, ws2.cap, 32 + 8 * k, q, tab.beta[k]);
    ws2.flags[q] = flags;
}
// k_agg_reduce for a set chunk (c.m a multiple of 64: one wavefront per 64-proof block, one key per block).  Lane l holds slot 64 blockIdx + l;
// g, sub, the lane numbering and the butterflies as there.  After the sums of r, W, r1, r2 and the group count, the lanes walk the key's
// signals (zkv_gset_agg.h): only the running share of U and one T_b are live at a time.  The sub-batch's pseudo-proof goes to slot psl[sb]
// of ws2 (sub <= 64), or its sums are parked at row blockIdx of ws2.fe for k_gset_agg_combine (sub = 128, 256).
__global__ __launch_bounds__(ZKV_BLOCK) void k_gset_agg_reduce(GsetChunk c, uint32_t sub, uint32_t g, Workspace ws, const uint32_t* __restrict__ agg,
                                                               const AggTables* __restrict__ tabs, Workspace ws2, uint8_t* __restrict__ status2,
                                                               const uint32_t* __restrict__ psl, uint32_t park) {
    const size_t i = (size_t)blockIdx.x * ZKV_BLOCK + threadIdx.x;
    const uint32_t L = 64u / g, w = sub / g;
    const uint32_t dist = (63u & ~(L - 1u)) | (w - 1u);
    const uint32_t lane = (threadIdx.x & (w - 1u)) + (threadIdx.x / L) * w;
    const size_t sb = (size_t)blockIdx.x * (64u / sub) + (threadIdx.x & (L - 1u)) / w;
    const uint32_t kk = (uint32_t)__builtin_amdgcn_readfirstlane((int)c.skey[c.slot0 + (size_t)blockIdx.x * ZKV_BLOCK]);
    const GsetKey key = c.keys[kk];
    const AggTables& tab = tabs[kk];
    bool in = false;
    if (i < c.m) in = (agg[(size_t)AGG_W_FLAGS * ws.cap + i] & FL_ALIVE) && !ws.g2bad[i];
    G1J W = g1j_infinity();
    Fr r = fr_zero();
    uint32_t s1[3] = {0, 0, 0}, s2[3] = {0, 0, 0}, cnt = in ? 1u : 0u;
    {                                                           // count a group once: at its first member in the check
        const unsigned long long inb = __ballot(in);
        unsigned long long lower = 0;
        for (uint32_t l = threadIdx.x & (L - 1u); l < threadIdx.x; l += L) lower |= 1ull << l;
        if (inb & lower) cnt = 0;
    }
    if (in) {
#pragma unroll
        for (int k = 0; k < 8; k++) r.v[k] = agg[(size_t)(AGG_W_U + k) * ws.cap + i];
        W = ga_ld_g1j(agg, ws.cap, AGG_W_W, i);
        s1[0] = agg[(size_t)(AGG_W_R + 0) * ws.cap + i]; s1[1] = agg[(size_t)(AGG_W_R + 1) * ws.cap + i];
        s2[0] = agg[(size_t)(AGG_W_R + 2) * ws.cap + i]; s2[1] = agg[(size_t)(AGG_W_R + 3) * ws.cap + i];
    }
    Fr Rm = r;
#pragma unroll 1
    for (int m = 32; m >= 1; m >>= 1) {
        if (!(dist & (uint32_t)m)) continue;
        Rm = fr_add(Rm, ga_fr_xor(Rm, m));
        W = g1j_add(W, ga_xor(W, m));
        uint32_t cy = 0;
        s1[0] = addc(s1[0], (uint32_t)__shfl_xor((int)s1[0], m, 64), cy); s1[1] = addc(s1[1], (uint32_t)__shfl_xor((int)s1[1], m, 64), cy);
        s1[2] = addc(s1[2], (uint32_t)__shfl_xor((int)s1[2], m, 64), cy);
        cy = 0;
        s2[0] = addc(s2[0], (uint32_t)__shfl_xor((int)s2[0], m, 64), cy); s2[1] = addc(s2[1], (uint32_t)__shfl_xor((int)s2[1], m, 64), cy);
        s2[2] = addc(s2[2], (uint32_t)__shfl_xor((int)s2[2], m, 64), cy);
        cnt += (uint32_t)__shfl_xor((int)cnt, m, 64);
    }
    uint32_t R[8];
    fr_to_raw(R, Rm);
    G1J U = gset_agg_base_share(g1j_infinity(), tab, key.tab->base_inf, R, lane, sub);
#pragma unroll 1
    for (uint32_t b = 0; b < key.n_sig; b++) {
        Fr t = fr_zero();
        if (in) {
            uint32_t sv[8];
#pragma unroll
            for (int k = 0; k < 8; k++) sv[k] = c.sig[(size_t)(8 * b + k) * c.sig_cap + i];
            t = fr_mul(fr_from_raw(sv), r);                     // signals are < r (k_gset_prep)
        }
#pragma unroll 1
        for (int m = 32; m >= 1; m >>= 1) if (dist & (uint32_t)m) t = fr_add(t, ga_fr_xor(t, m));
        uint32_t T[8];
        fr_to_raw(T, t);
        const uint32_t q = key.sig0 + b;
        U = gset_agg_sig_share(U, c.rows + (size_t)q * LONG_ROW_ENTRIES, c.win[q], T, lane, sub);
    }
#pragma unroll 1
    for (int m = 32; m >= 1; m >>= 1) if (dist & (uint32_t)m) U = g1j_add(U, ga_xor(U, m));
    G1J E = agg_e_share(tab, lane, sub, ((uint64_t)s1[1] << 32) | s1[0], s1[2], ((uint64_t)s2[1] << 32) | s2[0], s2[2], cnt + 1u);
#pragma unroll 1
    for (int m = 32; m >= 1; m >>= 1) if (dist & (uint32_t)m) E = g1j_add(E, ga_xor(E, m));
    if (lane != 0) return;
    if (park) {                                                 // (k_agg_reduce's parking rows, ws2.fe unused until the final exponentiation)
        uint32_t* row = ws2.fe;
        const size_t pb = blockIdx.x;
        ws_st(row, ws2.cap, 0, pb, E.x); ws_st(row, ws2.cap, 8, pb, E.y); ws_st(row, ws2.cap, 16, pb, E.z);
        ws_st(row, ws2.cap, 24, pb, U.x); ws_st(row, ws2.cap, 32, pb, U.y); ws_st(row, ws2.cap, 40, pb, U.z);
        ws_st(row, ws2.cap, 48, pb, W.x); ws_st(row, ws2.cap, 56, pb, W.y); ws_st(row, ws2.cap, 64, pb, W.z);
        row[(size_t)72 * ws2.cap + pb] = cnt;
        return;
    }
    const size_t q = psl[sb];
    ws2.g2bad[q] = 0;
    if (cnt == 0) { ws2.flags[q] = 0; status2[q] = ST_OK; return; }       // nothing left to check in this sub-batch
    ga_pseudo(E, U, W, tab, ws2, q);
    status2[q] = ST_VERIFICATION_FAILED;
}
// k_agg_combine for a set chunk: sub-batch j (of `wide` = 2 / 4 parked 64-proof blocks) becomes the pseudo-proof at slot psl[j]
__global__ __launch_bounds__(ZKV_BLOCK) void k_gset_agg_combine(GsetChunk c, size_t n2, uint32_t wide, const AggTables* __restrict__ tabs, Workspace ws2,
                                                                uint8_t* __restrict__ status2, const uint32_t* __restrict__ psl) {
    const size_t j = (size_t)blockIdx.x * ZKV_BLOCK + threadIdx.x;
    if (j >= n2) return;
    const AggTables& tab = tabs[c.skey[c.slot0 + j * 64 * wide]];
    const uint32_t* row = ws2.fe;
    G1J E = g1j_infinity(), U = g1j_infinity(), W = g1j_infinity();
    uint32_t cnt = 0, blocks = 0;
#pragma unroll 1
    for (uint32_t t = 0; t < wide; t++) {
        const size_t sb = j * wide + t;
        const uint32_t cb = row[(size_t)72 * ws2.cap + sb];
        if (!cb) continue;
        cnt += cb; blocks++;
        G1J p;
        p.x = ws_ld(row, ws2.cap, 0, sb); p.y = ws_ld(row, ws2.cap, 8, sb); p.z = ws_ld(row, ws2.cap, 16, sb); E = g1j_add(E, p);
        p.x = ws_ld(row, ws2.cap, 24, sb); p.y = ws_ld(row, ws2.cap, 32, sb); p.z = ws_ld(row, ws2.cap, 40, sb); U = g1j_add(U, p);
        p.x = ws_ld(row, ws2.cap, 48, sb); p.y = ws_ld(row, ws2.cap, 56, sb); p.z = ws_ld(row, ws2.cap, 64, sb); W = g1j_add(W, p);
    }
    const size_t q = psl[j];
    ws2.g2bad[q] = 0;
    if (cnt == 0) { ws2.flags[q] = 0; status2[q] = ST_OK; return; }
    if (blocks > 1u) {                                          // one pseudo-proof for `blocks` "- 1"s: the others' alpha back
        const uint32_t extra = blocks - 1u;
        if (extra & 1u) { const G1A a = tab.alpha_pow[0]; E = g1j_add_affine(E, a.x, a.y); }
        if (extra & 2u) { const G1A a = tab.alpha_pow[1]; E = g1j_add_affine(E, a.x, a.y); }
    }
    ga_pseudo(E, U, W, tab, ws2, q);
    status2[q] = ST_VERIFICATION_FAILED;
}

// ------------------------------------------------------------------ verdicts, and the second pass IN PLACE
// k_agg_mark with the sub-batch's verdict at psl[sb]; a proof of a failed sub-batch keeps its slot: its PREP flags come back (and its g2bad
// is cleared), every other slot is switched off, and the set's per-proof kernels run over the chunk once more.  Slots, keys and staged
// signals stay where k_gset_msm and k_gset_miller2 read them, so their wavefronts stay key-uniform whatever keys fail side by side.
// counters: [0] sub-batches checked, [1] sub-batches that failed.
__global__ __launch_bounds__(ZKV_BLOCK) void k_gset_agg_mark(size_t n, uint32_t sub, uint32_t g, Workspace ws, const uint32_t* __restrict__ agg,
                                                             const uint8_t* __restrict__ status2, const uint32_t* __restrict__ psl, uint8_t* __restrict__ status,
                                                             unsigned long long* __restrict__ counters) {
    const size_t i = (size_t)blockIdx.x * ZKV_BLOCK + threadIdx.x;
    if (i >= n) return;
    const uint32_t L = 64u / g, w = (sub < 64u ? sub : 64u) / g;
    const size_t sb = sub > 64u ? i / sub : (size_t)blockIdx.x * (64u / sub) + (threadIdx.x & (L - 1u)) / w;
    const bool first = sub > 64u ? (i % sub) == 0 : (threadIdx.x < L && (threadIdx.x & (w - 1u)) == 0);
    const bool passed = status2[psl[sb]] == ST_OK;
    if (first) { atomicAdd(&counters[0], 1ull); if (!passed) atomicAdd(&counters[1], 1ull); }
    const uint32_t flags0 = agg[(size_t)AGG_W_FLAGS * ws.cap + i];
    const uint32_t bad = ws.g2bad[i];
    bool again = false;
    if (flags0 & FL_ALIVE) {
        if (bad == 2u) again = true;                            // another B of its group failed the subgroup test: the group had no Miller value
        else if (!bad) { if (passed) status[i] = ST_OK; else again = true; }
    }
    ws.flags[i] = again ? flags0 : 0u;
    if (again) ws.g2bad[i] = 0;
}

void launch_gset_agg_reduce(const GsetChunk& c, uint32_t sub, uint32_t g, const Workspace& ws, const uint32_t* agg, const AggTables* tabs,
                            const Workspace& ws2, uint8_t* status2, const uint32_t* psl, bool park, hipStream_t s) {
    if (!c.m) return;
    hipLaunchKernelGGL(k_gset_agg_reduce, dim3((unsigned)((c.m + ZKV_BLOCK - 1) / ZKV_BLOCK)), dim3(ZKV_BLOCK), 0, s, c, sub, g, ws, agg, tabs, ws2, status2,
                       psl, park ? 1u : 0u);
}
void launch_gset_agg_combine(const GsetChunk& c, size_t n2, uint32_t wide, const AggTables* tabs, const Workspace& ws2, uint8_t* status2, const uint32_t* psl,
                             hipStream_t s) {
    if (!n2) return;
    hipLaunchKernelGGL(k_gset_agg_combine, dim3((unsigned)((n2 + ZKV_BLOCK - 1) / ZKV_BLOCK)), dim3(ZKV_BLOCK), 0, s, c, n2, wide, tabs, ws2, status2, psl);
}
void launch_gset_agg_mark(size_t n, uint32_t sub, uint32_t g, const Workspace& ws, const uint32_t* agg, const uint8_t* status2, const uint32_t* psl,
                          uint8_t* status, unsigned long long* counters, hipStream_t s) {
    if (!n) return;
    hipLaunchKernelGGL(k_gset_agg_mark, dim3((unsigned)((n + ZKV_BLOCK - 1) / ZKV_BLOCK)), dim3(ZKV_BLOCK), 0, s, n, sub, g, ws, agg, status2, psl, status, counters);
}

}  // namespace zkv

// Groth16 key sets (zkv_groth16_set_*): many verification keys in one batch, the key chosen per proof.
// This unit: the set-up of all keys in a fixed number of launches (grid y = key), the K-way partition of a batch by key, the prep stage
// with a per-slot key, the long-key vk_x walk with a per-lane key, and the return of the verdicts to the caller's order.  The Miller
// loops are in k_gset_pair.hip; the G2 subgroup check and the final exponentiation are the single-key kernels (they read no key).
#include "zkv_internal.h"

namespace zkv {

// ------------------------------------------------------------------ set-up: every key of the set per launch, six launches whatever K is
__global__ __launch_bounds__(64) void k_gset_setup_validate(const VkRaw* __restrict__ raw, VkTables* __restrict__ tab) {
    if (threadIdx.x == 0) setup_validate(raw[blockIdx.y], tab[blockIdx.y]);
}
__global__ __launch_bounds__(64) void k_gset_setup_base(const VkRaw* __restrict__ raw, VkTables* __restrict__ tab) {
    if (threadIdx.x == 0) setup_base(raw[blockIdx.y], tab[blockIdx.y]);
}
__global__ __launch_bounds__(64) void k_gset_setup_lines(const VkRaw* __restrict__ raw, VkTables* __restrict__ tab) {
    if (threadIdx.x == 0) setup_lines(raw[blockIdx.y].gamma, tab[blockIdx.y].lines[0]);
    if (threadIdx.x == 1) setup_lines(raw[blockIdx.y].delta, tab[blockIdx.y].lines[1]);
}
__global__ __launch_bounds__(64) void k_gset_setup_alpha_beta(const VkRaw* __restrict__ raw, VkTables* __restrict__ tab) {
    __shared__ uint32_t lds[96 + 48];
    if (threadIdx.x != 0) return;
    setup_alpha_beta(raw[blockIdx.y], tab[blockIdx.y], m_ref(lds, 1), m_ref(lds + 96, 1));
}
// IC[1..] of all keys back to back (n_sig_all points, 16 raw limbs each); sig_key[j]: the key point j belongs to.  An invalid point
// clears its own key's vk_valid only (after k_gset_setup_validate, same stream).
__global__ __launch_bounds__(64) void k_gset_setup_long_validate(const uint32_t* __restrict__ ic, const uint32_t* __restrict__ sig_key, uint32_t n_sig_all,
                                                                 VkTables* __restrict__ tab) {
    const uint32_t j = blockIdx.x * 64 + threadIdx.x;
    if (j < n_sig_all && !long_ic_valid(ic, j, j + 1, 1)) atomicAnd(&tab[sig_key[j]].vk_valid, 0u);
}
__global__ __launch_bounds__(64) void k_gset_setup_long_rows(const uint32_t* __restrict__ ic, G1A* __restrict__ rows, uint32_t* __restrict__ win) {
    const uint32_t b = blockIdx.x, w = threadIdx.x;
    if (w < (uint32_t)MSM_MAX_WINDOWS) setup_long_row((const uint32_t(*)[8])(ic + 16 * (size_t)b), w, rows + ((size_t)b * MSM_MAX_WINDOWS + w) * MSM_DIGITS, win + b);
}
void launch_gset_setup(uint32_t n_keys, const VkRaw* d_raw, VkTables* d_tabs, uint32_t n_sig_all, const uint32_t* d_ic, const uint32_t* d_sig_key,
                       G1A* rows, uint32_t* win, hipStream_t s) {
    const dim3 grid(1, n_keys), block(64);
    hipLaunchKernelGGL(k_gset_setup_validate, grid, block, 0, s, d_raw, d_tabs);
    hipLaunchKernelGGL(k_gset_setup_base, grid, block, 0, s, d_raw, d_tabs);
    hipLaunchKernelGGL(k_gset_setup_lines, grid, block, 0, s, d_raw, d_tabs);
    hipLaunchKernelGGL(k_gset_setup_alpha_beta, grid, block, 0, s, d_raw, d_tabs);
    if (!n_sig_all) return;
    hipLaunchKernelGGL(k_gset_setup_long_validate, dim3((n_sig_all + 63) / 64), block, 0, s, d_ic, d_sig_key, n_sig_all, d_tabs);
    hipLaunchKernelGGL(k_gset_setup_long_rows, dim3(n_sig_all), block, 0, s, d_ic, rows, win);
}

// ------------------------------------------------------------------ partition by key (count per block, host layout, place)
// One wavefront per block; block b owns proofs [b * per_block, (b + 1) * per_block).  Keys >= n_keys are counted nowhere.
constexpr uint32_t GSET_MAX_KEYS = 1024;
__global__ __launch_bounds__(64) void k_gset_count(GsetPart p) {
    __shared__ uint32_t hist[GSET_MAX_KEYS];
    for (uint32_t k = threadIdx.x; k < p.n_keys; k += 64) hist[k] = 0;
    __syncthreads();
    const size_t i0 = (size_t)blockIdx.x * p.per_block;
#pragma unroll 1
    for (uint32_t t = threadIdx.x; t < p.per_block; t += 64) {
        const size_t i = i0 + t;
        if (i < p.n) { const uint32_t k = p.key[i]; if (k < p.n_keys) atomicAdd(&hist[k], 1u); }
    }
    __syncthreads();
    for (uint32_t k = threadIdx.x; k < p.n_keys; k += 64) {
        const uint32_t h = hist[k];
        p.cnt[(size_t)k * p.blocks + blockIdx.x] = h;
        if (h) atomicAdd(&p.totals[k], h);
    }
}
// first slot of every (key, block): one lane per key, the blocks in order (start: zkv_gset_layout.h, computed on the host from the totals)
__global__ __launch_bounds__(64) void k_gset_scan(GsetPart p, const uint64_t* __restrict__ start) {
    const uint32_t k = blockIdx.x * 64 + threadIdx.x;
    if (k >= p.n_keys) return;
    uint32_t run = (uint32_t)start[k];
    const size_t row = (size_t)k * p.blocks;
#pragma unroll 1
    for (uint32_t b = 0; b < p.blocks; b++) { p.off[row + b] = run; run += p.cnt[row + b]; }
}
// Stable placement: the block walks its proofs 64 at a time in order; a proof's slot is its key's running slot plus the number of
// earlier lanes of the same 64 with the same key.
__global__ __launch_bounds__(64) void k_gset_place(GsetPart p) {
    __shared__ uint32_t run[GSET_MAX_KEYS];
    for (uint32_t k = threadIdx.x; k < p.n_keys; k += 64) run[k] = p.off[(size_t)k * p.blocks + blockIdx.x];
    __syncthreads();
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
        uint32_t slot = GSET_NONE;
        if (k != GSET_NONE) slot = run[k] + rank;
        __syncthreads();
        if (k != GSET_NONE && last) run[k] = slot + 1;
        __syncthreads();
        if (live) p.pos[i] = slot;
        if (k != GSET_NONE) { p.idx[slot] = (uint32_t)i; p.skey[slot] = k; }
    }
}
void launch_gset_count(const GsetPart& p, hipStream_t s) {
    hipLaunchKernelGGL(k_gset_count, dim3(p.blocks), dim3(64), 0, s, p);
}
void launch_gset_place(const GsetPart& p, const uint64_t* d_start, hipStream_t s) {
    hipLaunchKernelGGL(k_gset_scan, dim3((p.n_keys + 63) / 64), dim3(64), 0, s, p, d_start);
    hipLaunchKernelGGL(k_gset_place, dim3(p.blocks), dim3(64), 0, s, p);
}

// ------------------------------------------------------------------ prep: one slot per lane (k_prep_groth16_long with the slot's key)
__global__ __launch_bounds__(ZKV_BLOCK) void k_gset_prep(GsetChunk c, Workspace ws) {
    const size_t j = (size_t)blockIdx.x * ZKV_BLOCK + threadIdx.x;
    if (j >= c.m) return;
    const uint32_t i = c.idx[c.slot0 + j];
    uint32_t flags = 0;
    if (i != GSET_NONE) {
        const GsetKey key = c.keys[c.skey[c.slot0 + j]];
        if (key.tab->vk_valid) {                                   // a key with an invalid point fails its own proofs (groth16.rs: the precompiles reject)
            bool ok = true;
            const uint8_t* row = c.signals + (size_t)c.sig_stride * i;
#pragma unroll 1
            for (uint32_t b = 0; b < key.n_sig; b++) {
                uint32_t s[8];
                load_be256(s, row + 32 * b);
                ok = raw_lt_r(s) && ok;                            // groth16.rs:32
#pragma unroll
                for (int k = 0; k < 8; k++) c.sig[(size_t)(8 * b + k) * c.sig_cap + j] = s[k];
            }
            if (ok) {
                PrepOut o;
                uint32_t w[8][8];
                const uint8_t* rec = c.proofs + 256 * (size_t)i;
#pragma unroll 1
                for (int q = 0; q < 8; q++) load_be256(w[q], rec + 32 * q);
                if (prep_points(w, key.negate != 0, o)) {
                    flags = o.flags;
                    ws_st(ws.prep, ws.cap, 0, j, o.ax); ws_st(ws.prep, ws.cap, 8, j, o.ay);
                    ws_st(ws.prep, ws.cap, 16, j, o.cx); ws_st(ws.prep, ws.cap, 24, j, o.cy);
                    ws_st(ws.prep, ws.cap, 32, j, o.bx.c0); ws_st(ws.prep, ws.cap, 40, j, o.bx.c1);
                    ws_st(ws.prep, ws.cap, 48, j, o.by.c0); ws_st(ws.prep, ws.cap, 56, j, o.by.c1);
                }
            }
        }
    }
    ws.flags[j] = flags;
    ws.g2bad[j] = 0;
    c.status[j] = ST_VERIFICATION_FAILED;
}
void launch_gset_prep(const GsetChunk& c, const Workspace& ws, hipStream_t s) {
    if (!c.m) return;
    hipLaunchKernelGGL(k_gset_prep, dim3((unsigned)((c.m + ZKV_BLOCK - 1) / ZKV_BLOCK)), dim3(ZKV_BLOCK), 0, s, c, ws);
}

// ------------------------------------------------------------------ vk_x: the long-key walk (long_msm_slice) with the slot's key
// G lanes per slot as k_msm_long; the G lanes of a slot share its key, so the table reads stay per-lane gathers as they are there.
__device__ __forceinline__ G1J gset_shfl_xor(const G1J& p, int mask) {      // (k_msm.hip's butterfly step)
    G1J r;
#pragma unroll
    for (int k = 0; k < 8; k++) {
        r.x.v[k] = (uint32_t)__shfl_xor((int)p.x.v[k], mask, 64);
        r.y.v[k] = (uint32_t)__shfl_xor((int)p.y.v[k], mask, 64);
        r.z.v[k] = (uint32_t)__shfl_xor((int)p.z.v[k], mask, 64);
    }
    return r;
}
template <uint32_t G> __global__ __launch_bounds__(64) void k_gset_msm(GsetChunk c, Workspace ws) {
    const uint32_t lane = threadIdx.x % G;
    const size_t j = (size_t)blockIdx.x * (64 / G) + threadIdx.x / G;
    if (j >= c.m) return;
    uint32_t flags = ws.flags[j];
    if (!(flags & FL_ALIVE)) return;
    const GsetKey key = c.keys[c.skey[c.slot0 + j]];
    auto digit = [&](uint32_t b, uint32_t w) { return (c.sig[(size_t)(8 * b + (w >> 2)) * c.sig_cap + j] >> ((w & 3) * 8)) & 255u; };
    G1J acc = long_msm_slice(key.n_sig, c.win + key.sig0, c.rows + (size_t)key.sig0 * LONG_ROW_ENTRIES, digit, lane, G);
#pragma unroll 1
    for (uint32_t m = G / 2; m > 0; m >>= 1) acc = g1j_add(acc, gset_shfl_xor(acc, (int)m));
    if (lane != 0) return;
    const VkTables* vk = key.tab;
    if (!vk->base_inf) acc = g1j_add_affine(acc, vk->base.x, vk->base.y);
    PrepOut in;
    in.ax = ws_ld(ws.prep, ws.cap, 0, j); in.ay = ws_ld(ws.prep, ws.cap, 8, j);
    in.cx = ws_ld(ws.prep, ws.cap, 16, j); in.cy = ws_ld(ws.prep, ws.cap, 24, j);
    G1Norm o;
    msm_normalize_acc(acc, in, flags, o);
    ws_st(ws.norm, ws.cap, 0, j, o.axs); ws_st(ws.norm, ws.cap, 8, j, o.ays);
    ws_st(ws.norm, ws.cap, 16, j, o.lxs); ws_st(ws.norm, ws.cap, 24, j, o.lys);
    ws_st(ws.norm, ws.cap, 32, j, o.cxs); ws_st(ws.norm, ws.cap, 40, j, o.cys);
    ws.flags[j] = flags;
}
void launch_gset_msm(const GsetChunk& c, uint32_t lanes, const Workspace& ws, hipStream_t s) {
    if (!c.m) return;
    const dim3 grid((unsigned)((c.m * lanes + 63) / 64)), block(64);
    if (lanes == 64) hipLaunchKernelGGL(k_gset_msm<64>, grid, block, 0, s, c, ws);
    else if (lanes == 16) hipLaunchKernelGGL(k_gset_msm<16>, grid, block, 0, s, c, ws);
    else hipLaunchKernelGGL(k_gset_msm<1>, grid, block, 0, s, c, ws);
}
// compute_vk_x alone (zkv_groth16_set_vk_x_batch): caller order, key[i] < n_keys checked by the host; digits straight from the big-endian rows
template <uint32_t G> __global__ __launch_bounds__(64) void k_gset_vk_x(size_t n, const uint32_t* __restrict__ keyi, const GsetKey* __restrict__ keys,
                                                                         const G1A* __restrict__ rows, const uint32_t* __restrict__ win,
                                                                         const uint8_t* __restrict__ sig, uint32_t sig_stride, uint8_t* __restrict__ out) {
    const uint32_t lane = threadIdx.x % G;
    const size_t i = (size_t)blockIdx.x * (64 / G) + threadIdx.x / G;
    if (i >= n) return;
    const GsetKey key = keys[keyi[i]];
    const uint8_t* row = sig + (size_t)sig_stride * i;
    auto digit = [&](uint32_t b, uint32_t w) { return (uint32_t)row[32 * b + 31 - w]; };
    G1J acc = long_msm_slice(key.n_sig, win + key.sig0, rows + (size_t)key.sig0 * LONG_ROW_ENTRIES, digit, lane, G);
#pragma unroll 1
    for (uint32_t m = G / 2; m > 0; m >>= 1) acc = g1j_add(acc, gset_shfl_xor(acc, (int)m));
    if (lane != 0) return;
    if (!key.tab->base_inf) acc = g1j_add_affine(acc, key.tab->base.x, key.tab->base.y);
    G1A a; uint32_t inf;
    g1j_to_affine(acc, a, inf);
    uint32_t r[8];
    uint8_t* o = out + 64 * i;
#pragma unroll 1
    for (int c = 0; c < 2; c++) {
        fp_to_raw(r, c ? a.y : a.x);
#pragma unroll 1
        for (int k = 0; k < 8; k++) {
            uint32_t v = r[7 - k];
            o[32 * c + 4 * k] = (uint8_t)(v >> 24); o[32 * c + 4 * k + 1] = (uint8_t)(v >> 16);
            o[32 * c + 4 * k + 2] = (uint8_t)(v >> 8); o[32 * c + 4 * k + 3] = (uint8_t)v;
        }
    }
}
void launch_gset_vk_x(size_t n, uint32_t lanes, const uint32_t* key, const GsetKey* keys, const G1A* rows, const uint32_t* win, const uint8_t* sig,
                      uint32_t sig_stride, uint8_t* out, hipStream_t s) {
    if (!n) return;
    const dim3 grid((unsigned)((n * lanes + 63) / 64)), block(64);
    if (lanes == 64) hipLaunchKernelGGL(k_gset_vk_x<64>, grid, block, 0, s, n, key, keys, rows, win, sig, sig_stride, out);
    else if (lanes == 16) hipLaunchKernelGGL(k_gset_vk_x<16>, grid, block, 0, s, n, key, keys, rows, win, sig, sig_stride, out);
    else hipLaunchKernelGGL(k_gset_vk_x<1>, grid, block, 0, s, n, key, keys, rows, win, sig, sig_stride, out);
}

// ------------------------------------------------------------------ return: slot statuses -> 1 / 0 in the caller's order (k_status_to_bool's rule)
__global__ __launch_bounds__(ZKV_BLOCK) void k_gset_return(size_t n, const uint32_t* __restrict__ pos, const uint8_t* __restrict__ status, uint8_t* __restrict__ verified) {
    const size_t i = (size_t)blockIdx.x * ZKV_BLOCK + threadIdx.x;
    if (i >= n) return;
    const uint32_t p = pos[i];
    verified[i] = (p != GSET_NONE && status[p] == ST_OK) ? 1 : 0;
}
void launch_gset_return(size_t n, const uint32_t* pos, const uint8_t* status, uint8_t* verified, hipStream_t s) {
    if (!n) return;
    hipLaunchKernelGGL(k_gset_return, dim3((unsigned)((n + ZKV_BLOCK - 1) / ZKV_BLOCK)), dim3(ZKV_BLOCK), 0, s, n, pos, status, verified);
}

}  // namespace zkv

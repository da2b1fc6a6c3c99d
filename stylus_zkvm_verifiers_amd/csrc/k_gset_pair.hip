// Groth16 key sets: the Miller loops of k_pair.hip / k_wide.hip (k_miller2, k_miller_w, k_miller_w64, k_miller_w64d) with the key of each
// wavefront's first slot.  The slot layout (zkv_gset_layout.h) puts only proofs of one key into a wavefront, so the key is read once per
// wavefront and made wave-uniform with readfirstlane: the line-table and f_alpha_beta reads stay scalar, as in the single-key kernels.
#define ZKV_PAIRED 1
#include "zkv_internal.h"
#include "zkv_tower_wide.h"

namespace zkv {

// The VkTables of the wavefront whose first slot is `first` (chunk-relative; first >= m: no live slot, any key will do)
__device__ __forceinline__ const VkTables* gset_wave_tab(const uint32_t* __restrict__ skey, const GsetKey* __restrict__ keys, size_t first, size_t m) {
    const uint32_t k = (uint32_t)__builtin_amdgcn_readfirstlane((int)(first < m ? skey[first] : 0u));
    const uint64_t p = (uint64_t)keys[k].tab;
    const uint32_t lo = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)p), hi = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)(p >> 32));
    return (const VkTables*)(((uint64_t)hi << 32) | lo);
}

// k_miller2 (one proof per lane pair, 32 per wavefront; also the subgroup test of B)
__global__ __launch_bounds__(ZKV_BLOCK, 2) void k_gset_miller2(size_t n, const uint32_t* __restrict__ skey, const GsetKey* __restrict__ keys, Workspace ws,
                                                               uint8_t* __restrict__ status) {
    __shared__ uint32_t lds[(48 + 24) * ZKV_BLOCK];
    const VkTables* vk = gset_wave_tab(skey, keys, ((size_t)blockIdx.x * ZKV_BLOCK) >> 1, n);
    size_t i = ((size_t)blockIdx.x * ZKV_BLOCK + threadIdx.x) >> 1;
    if (i >= n) return;
    uint32_t flags = ws.flags[i];
    if (!(flags & FL_ALIVE)) return;
    const uint32_t par = threadIdx.x & 1u;
    uint32_t* wl = lds + (threadIdx.x & 63u);
    LRef fm = l_ref(wl);
    LRef tm = l_ref(wl + 48 * ZKV_BLOCK);
    SoaRef norm = {ws.norm, ws.cap, (uint32_t)i * 4u};
    SoaRef bsrc = {ws.prep + 32 * ws.cap, ws.cap, (uint32_t)(8 * par * ws.cap + i) * 4u};
    if (!miller_loop_p(vk, flags, norm, bsrc, fm, tm, true)) {
        if (!par) { ws.g2bad[i] = 1; status[i] = ST_VERIFICATION_FAILED; }
        return;
    }
    MRef ab = m_ref((uint32_t*)(vk->f_alpha_beta) + 8 * par, 1, 16);
    MRef out = m_ref(ws.f + (size_t)(8 * par) * ws.cap + i, (uint32_t)ws.cap, 16);
    f12m_mul_body(out, fm, ab, false);
}

// k_miller_w / k_miller_w64: SLICES = 1, four proofs per wavefront; SLICES = 4, one
template <int SLICES> __device__ __forceinline__ void gset_miller_w_body(size_t n, const VkTables* __restrict__ vk, const Workspace& ws, uint32_t* lds) {
    constexpr int GROUP = 16 * SLICES, PER_BLOCK = ZKV_BLOCK / GROUP;
    constexpr int SLOT = 96 + 48 + 13 * 16 + (SLICES > 1 ? W_RED_WORDS : 0);
    const uint32_t g = threadIdx.x / GROUP, half = threadIdx.x & 1u;
    WL wl;
    wl.q = (int)((threadIdx.x >> 1) & 7u);
    if (wl.q >= 6) wl.q -= 6;
    wl.s = (int)((threadIdx.x % GROUP) >> 4);
    const size_t i = (size_t)blockIdx.x * PER_BLOCK + g;
    if (i >= n) return;
    const uint32_t flags = ws.flags[i];
    if (!(flags & FL_ALIVE)) return;
    G1Norm nm;
    nm.axs = ws_ld(ws.norm, ws.cap, 0, i); nm.ays = ws_ld(ws.norm, ws.cap, 8, i);
    nm.lxs = ws_ld(ws.norm, ws.cap, 16, i); nm.lys = ws_ld(ws.norm, ws.cap, 24, i);
    nm.cxs = ws_ld(ws.norm, ws.cap, 32, i); nm.cys = ws_ld(ws.norm, ws.cap, 40, i);
    Fp2 bx, by;
    bx.h = ws_ld(ws.prep, ws.cap, 32 + 8 * (int)half, i); by.h = ws_ld(ws.prep, ws.cap, 48 + 8 * (int)half, i);
    uint32_t* base = lds + g * SLOT + 8 * half;
    MRef fm = m_ref(base, 1, 16), tm = m_ref(base + 96, 1, 16), sc = m_ref(base + 144, 1, 16), red = m_ref(base + 352, 1, 16);
    miller_loop_w<SLICES>(*vk, flags, nm, bx, by, fm, tm, sc, wl, red);
    MRef ab = m_ref((uint32_t*)(vk->f_alpha_beta) + 8 * half, 1, 16);
    MRef out = m_ref(ws.f + (size_t)(8 * half) * ws.cap + i, (uint32_t)ws.cap, 16);
    w12_mul<SLICES>(out, fm, ab, wl, false, red);
}
__global__ __launch_bounds__(ZKV_BLOCK, 2) void k_gset_miller_w(size_t n, const uint32_t* __restrict__ skey, const GsetKey* __restrict__ keys, Workspace ws) {
    __shared__ uint32_t lds[4 * (96 + 48 + 13 * 16)];
    gset_miller_w_body<1>(n, gset_wave_tab(skey, keys, (size_t)blockIdx.x * 4, n), ws, lds);
}
__global__ __launch_bounds__(ZKV_BLOCK, 2) void k_gset_miller_w64(size_t n, const uint32_t* __restrict__ skey, const GsetKey* __restrict__ keys, Workspace ws) {
    __shared__ uint32_t lds[96 + 48 + 13 * 16 + W_RED_WORDS];
    gset_miller_w_body<4>(n, gset_wave_tab(skey, keys, blockIdx.x, n), ws, lds);
}

// Consumer wavefronts of k_gset_miller_w64d that gave up waiting for their producer (see g_zkv_wait_faults in k_wide.hip): counted here,
// added to zkv_diag_wait_faults by the C ABI.
__device__ unsigned int g_zkv_gset_wait_faults = 0;
int read_gset_wait_faults(unsigned long long* out) {
    unsigned int v = 0;
    if (hipMemcpyFromSymbol(&v, HIP_SYMBOL(g_zkv_gset_wait_faults), sizeof v) != hipSuccess) { (void)hipGetLastError(); return -1; }
    *out = v;
    return 0;
}
// k_miller_w64d: two wavefronts per proof (the producer steps the running point, the consumer accumulates f); the workgroup is one proof,
// so both wavefronts read the same key
__global__ __launch_bounds__(128, 2) void k_gset_miller_w64d(size_t n, const uint32_t* __restrict__ skey, const GsetKey* __restrict__ keys, Workspace ws,
                                                             uint8_t* __restrict__ status) {
    constexpr int F_WORDS = 96 + 64 + W_RED_WORDS, T_WORDS = 48 + 13 * 16, LINE_WORDS = ZKV_MILLER_STEPS * 48;
    __shared__ uint32_t lds[F_WORDS + T_WORDS + LINE_WORDS + 4];
    const VkTables* vk = gset_wave_tab(skey, keys, blockIdx.x, n);
    const size_t i = blockIdx.x;
    if (i >= n) return;
    const uint32_t flags = ws.flags[i];
    if (!(flags & FL_ALIVE)) return;
    const uint32_t wave = (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const uint32_t lane = threadIdx.x & 63u, half = lane & 1u;
    WL w;
    w.q = (int)((lane >> 1) & 7u);
    if (w.q >= 6) w.q -= 6;
    w.s = (int)(lane >> 4);
    volatile uint32_t* ready = lds + F_WORDS + T_WORDS + LINE_WORDS;
    MRef lines = m_ref(lds + F_WORDS + T_WORDS + 8 * half, 1, 16);
    const bool do_ab = !(flags & (FL_A_INF | FL_B_INF));
    if (threadIdx.x == 64) *ready = 0;
    __syncthreads();
    if (wave == 1) {
        if (!do_ab) return;
        Fp2 bx, by;
        bx.h = ws_ld(ws.prep, ws.cap, 32 + 8 * (int)half, i); by.h = ws_ld(ws.prep, ws.cap, 48 + 8 * (int)half, i);
        MRef tm = m_ref(lds + F_WORDS + 8 * half, 1, 16), sc = m_ref(lds + F_WORDS + 48 + 8 * half, 1, 16);
        miller_lines_producer(bx, by, tm, sc, lines, ready, w.q);
        return;
    }
    G1Norm nm;
    nm.axs = ws_ld(ws.norm, ws.cap, 0, i); nm.ays = ws_ld(ws.norm, ws.cap, 8, i);
    nm.lxs = ws_ld(ws.norm, ws.cap, 16, i); nm.lys = ws_ld(ws.norm, ws.cap, 24, i);
    nm.cxs = ws_ld(ws.norm, ws.cap, 32, i); nm.cys = ws_ld(ws.norm, ws.cap, 40, i);
    uint32_t* base = lds + 8 * half;
    MRef fm = m_ref(base, 1, 16), sc = m_ref(base + 96, 1, 16), red = m_ref(base + 160, 1, 16);
    if (!miller_loop_consumer<4>(vk, flags, nm, fm, sc, lines, ready, w, red)) {
        if (lane == 0) { ws.g2bad[i] = 1; status[i] = ST_VERIFICATION_FAILED; atomicAdd(&g_zkv_gset_wait_faults, 1u); }     // fail closed, and count it
        return;
    }
    MRef ab = m_ref((uint32_t*)(vk->f_alpha_beta) + 8 * half, 1, 16);
    MRef out = m_ref(ws.f + (size_t)(8 * half) * ws.cap + i, (uint32_t)ws.cap, 16);
    w12_mul<4>(out, fm, ab, w, false, red);
}

void launch_gset_miller(int lanes, size_t m, const uint32_t* skey, const GsetKey* keys, const Workspace& ws, uint8_t* status, hipStream_t s) {
    if (!m) return;
    if (lanes == 128) hipLaunchKernelGGL(k_gset_miller_w64d, dim3((unsigned)m), dim3(128), 0, s, m, skey, keys, ws, status);
    else if (lanes == 64) hipLaunchKernelGGL(k_gset_miller_w64, dim3((unsigned)m), dim3(ZKV_BLOCK), 0, s, m, skey, keys, ws);
    else if (lanes == 16) hipLaunchKernelGGL(k_gset_miller_w, dim3((unsigned)((m + 3) / 4)), dim3(ZKV_BLOCK), 0, s, m, skey, keys, ws);
    else hipLaunchKernelGGL(k_gset_miller2, dim3((unsigned)((2 * m + ZKV_BLOCK - 1) / ZKV_BLOCK)), dim3(ZKV_BLOCK), 0, s, m, skey, keys, ws, status);
}

}  // namespace zkv

// PLONK key sets (include/zkv_plonk_set.h): many gnark keys in one batch, the key chosen per proof.
// This unit: the PlonkKey of every key of the set in three launches whatever K is (grid y = key), the per-key validity words, and stage
// PREP with the key of each wavefront.  The line tables of every key's [1]_2 / [tau]_2 are k_gset.hip's set-up kernels, the partition by
// key and the return are k_gset.hip's, the Miller loops k_gset_pair.hip's (they take a VkTables per wavefront), the final exponentiation
// the single-key kernels.  A translation unit of its own, so that every existing kernel compiles exactly as before.  Parity unpinned by
// construction (no PLONK in the reference).
#include "zkv_internal.h"
#include "zkv_plonk.h"

namespace zkv {

#ifndef ZKV_PLONK_WAVES
#define ZKV_PLONK_WAVES 4        /* as k_plonk.hip */
#endif

// ------------------------------------------------------------------ set-up: k_plonk_setup_keys / k_plonk_keys_mult / k_plonk_keys_joint per key
__global__ __launch_bounds__(64) void k_pset_setup_key(const PlonkKeyRaw* __restrict__ raw, PlonkKey* __restrict__ key) {
    if (blockIdx.x == 0 && threadIdx.x == 0) plonk_setup_key(raw[blockIdx.y], key[blockIdx.y], true);
}
__global__ __launch_bounds__(64) void k_pset_mult(PlonkKey* __restrict__ key) {
    if (threadIdx.x == 0 && blockIdx.x <= PK_POINTS) plonk_setup_mult(key[blockIdx.y], (int)blockIdx.x);
}
__global__ __launch_bounds__(64) void k_pset_joint(PlonkKey* __restrict__ key) {
    const int t = (int)(blockIdx.x * 64 + threadIdx.x);
    if (t < (PK_POINTS + 1) * (PK_JA + 1)) plonk_joint_row(key[blockIdx.y], t / (PK_JA + 1), t % (PK_JA + 1));
}
// ok[k]: key k's own rule (points, size_inv / generator / coset_shift < R) and its two G2 points (k_gset_setup_validate) -- the set form
// of PrepArgs::force_fail
__global__ __launch_bounds__(64) void k_pset_valid(const PlonkKey* __restrict__ key, const VkTables* __restrict__ tab, uint32_t n_keys, uint32_t* __restrict__ ok) {
    const uint32_t k = blockIdx.x * 64 + threadIdx.x;
    if (k < n_keys) ok[k] = (key[k].valid && tab[k].vk_valid) ? 1u : 0u;
}
void launch_pset_setup(uint32_t n_keys, const PlonkKeyRaw* d_raw, PlonkKey* d_keys, const VkTables* d_tabs, uint32_t* d_ok, hipStream_t s) {
    const dim3 block(64);
    hipLaunchKernelGGL(k_pset_setup_key, dim3(1, n_keys), block, 0, s, d_raw, d_keys);
    hipLaunchKernelGGL(k_pset_mult, dim3(PK_POINTS + 1, n_keys), block, 0, s, d_keys);
    hipLaunchKernelGGL(k_pset_joint, dim3(((PK_POINTS + 1) * (PK_JA + 1) + 63) / 64, n_keys), block, 0, s, d_keys);
    hipLaunchKernelGGL(k_pset_valid, dim3((n_keys + 63) / 64), block, 0, s, d_keys, d_tabs, n_keys, d_ok);
}

// ------------------------------------------------------------------ PREP: k_plonk_prep_keys with the key of the wavefront
// One slot per lane.  Key groups start on multiples of 64 slots (zkv_gset_layout.h pset_choose) and the first slot of every 64-slot block
// is a proof, so the block's key is that of its first slot, made wave-uniform with readfirstlane: the key's header and point reads stay
// scalar.  Pad slots (idx = GSET_NONE) and proofs of an invalid key get flags 0 and status VerificationFailed without running PREP.
__global__ __launch_bounds__(ZKV_BLOCK, ZKV_PLONK_WAVES) void k_pset_prep(PsetChunk c, Workspace ws) {
    const size_t first = (size_t)blockIdx.x * ZKV_BLOCK, j = first + threadIdx.x;
    const uint32_t k = (uint32_t)__builtin_amdgcn_readfirstlane((int)(first < c.m ? c.skey[c.slot0 + first] : 0u));
    if (j >= c.m) return;
    const uint32_t i = c.idx[c.slot0 + j];
    uint32_t flags = 0;
    const PlonkKey* key = c.keys + k;
    if (i != GSET_NONE && c.ok[k]) {
        const uint8_t* rec = c.proofs + (size_t)i * c.proof_stride;
        const uint32_t nw = 24 + 3 * key->n_c;                                     // 24 or 27
        uint32_t w[27][8];
#pragma unroll 1
        for (int q = 0; q < 27; q++) {
            if ((uint32_t)q < nw) load_be256(w[q], rec + 32 * q);
            else for (int b = 0; b < 8; b++) w[q][b] = 0;
        }
        PlonkOut o;
        const TabRef tab = {c.plonk_tab + j * (size_t)PLONK_TAB_WORDS};
        const PlonkPubRow pub = {c.inputs + (size_t)i * c.input_stride};
        if (plonk_prepare(*key, w, pub, o, tab)) {
            // x/y = X Z / Y and 1/y = Z^3 / Y of the two points, as k_plonk_prep_keys writes them
            const Fp one = fp_one();
            const bool d_inf = fp_is_zero(o.d.z), q_inf = fp_is_zero(o.q.z);
            const Fp yd = d_inf ? one : o.d.y, yq = q_inf ? one : o.q.y;
            const Fp inv = fp_inv(fp_mul(yd, yq));
            const Fp iyd = fp_mul(inv, yq), iyq = fp_mul(inv, yd);
            const Fp z = fp_zero();
            ws_st(ws.norm, ws.cap, 0, j, z); ws_st(ws.norm, ws.cap, 8, j, z);
            ws_st(ws.norm, ws.cap, 16, j, fp_mul(fp_mul(o.d.x, o.d.z), iyd)); ws_st(ws.norm, ws.cap, 24, j, fp_mul(fp_mul(fp_sqr(o.d.z), o.d.z), iyd));
            ws_st(ws.norm, ws.cap, 32, j, fp_mul(fp_mul(o.q.x, o.q.z), iyq)); ws_st(ws.norm, ws.cap, 40, j, fp_mul(fp_mul(fp_sqr(o.q.z), o.q.z), iyq));
            flags = FL_ALIVE | FL_A_INF | FL_B_INF | (d_inf ? FL_L_INF : 0u) | (q_inf ? FL_C_INF : 0u);
        }
    }
    ws.flags[j] = flags;
    ws.g2bad[j] = 0;
    c.status[j] = ST_VERIFICATION_FAILED;
}
void launch_pset_prep(const PsetChunk& c, const Workspace& ws, hipStream_t s) {
    if (!c.m) return;
    hipLaunchKernelGGL(k_pset_prep, dim3((unsigned)((c.m + ZKV_BLOCK - 1) / ZKV_BLOCK)), dim3(ZKV_BLOCK), 0, s, c, ws);
}

}  // namespace zkv

// PLONK core for any key (include/zkv_plonk_keys.h): key set-up under the generic rule and stage PREP of a
// batch, the public inputs read from a per-proof row.  Everything after PREP -- the joint tables (k_plonk_mult / k_plonk_joint), the
// lane-pair Miller loop, the final exponentiation, the aggregate check -- is the SP1 PLONK path's.  A translation unit of its own, so that
// the SP1 kernels of k_plonk.hip compile exactly as before.  Parity unpinned by construction (no PLONK in the reference).
#include "zkv_internal.h"
#include "zkv_plonk.h"

namespace zkv {

#ifndef ZKV_PLONK_WAVES
#define ZKV_PLONK_WAVES 4        /* as k_plonk.hip */
#endif

__global__ __launch_bounds__(64) void k_plonk_setup_keys(const PlonkKeyRaw* __restrict__ raw, PlonkKey* __restrict__ key) {
    if (blockIdx.x == 0 && threadIdx.x == 0) plonk_setup_key(*raw, *key, true);
}

// Any key (include/zkv_plonk_keys.h): one proof per lane as k_plonk_prep, without selector or SP1 public values.  Proof i is the
// a.stride = 32 (24 + 3 n_c) bytes at a.blob + i * a.stride (the MarshalSolidity words without selector: no BSB22 words for n_c = 0),
// its public inputs the key.nb_public (= a.n_sig) 32-byte big-endian words at a.in32_a + i * 32 * a.n_sig.  Status VerificationFailed
// unless the pairing stages turn it into OK; D and Q go where k_plonk_prep puts them.
__global__ __launch_bounds__(ZKV_BLOCK, ZKV_PLONK_WAVES) void k_plonk_prep_keys(PrepArgs a, const PlonkKey* __restrict__ key, Workspace ws) {
    const size_t i = (size_t)blockIdx.x * ZKV_BLOCK + threadIdx.x;
    if (i >= a.n) return;
    uint32_t flags = 0;
    if (!a.force_fail) {
        const uint8_t* rec = a.blob + i * (size_t)a.stride;
        const uint32_t nw = a.stride / 32;                                          // 24 or 27
        uint32_t w[27][8];
#pragma unroll 1
        for (int k = 0; k < 27; k++) {
            if ((uint32_t)k < nw) load_be256(w[k], rec + 32 * k);
            else for (int j = 0; j < 8; j++) w[k][j] = 0;
        }
        PlonkOut o;
        const TabRef tab = {a.plonk_tab + i * (size_t)PLONK_TAB_WORDS};
        const PlonkPubRow pub = {a.in32_a + i * 32 * (size_t)a.n_sig};
        if (plonk_prepare(*key, w, pub, o, tab)) {
            // x/y = X Z / Y and 1/y = Z^3 / Y of the two points, as k_plonk_prep writes them
            const Fp one = fp_one();
            const bool d_inf = fp_is_zero(o.d.z), q_inf = fp_is_zero(o.q.z);
            const Fp yd = d_inf ? one : o.d.y, yq = q_inf ? one : o.q.y;
            const Fp inv = fp_inv(fp_mul(yd, yq));
            const Fp iyd = fp_mul(inv, yq), iyq = fp_mul(inv, yd);
            const Fp z = fp_zero();
            ws_st(ws.norm, ws.cap, 0, i, z); ws_st(ws.norm, ws.cap, 8, i, z);
            ws_st(ws.norm, ws.cap, 16, i, fp_mul(fp_mul(o.d.x, o.d.z), iyd)); ws_st(ws.norm, ws.cap, 24, i, fp_mul(fp_mul(fp_sqr(o.d.z), o.d.z), iyd));
            ws_st(ws.norm, ws.cap, 32, i, fp_mul(fp_mul(o.q.x, o.q.z), iyq)); ws_st(ws.norm, ws.cap, 40, i, fp_mul(fp_mul(fp_sqr(o.q.z), o.q.z), iyq));
                    flags = FL_ALIVE | FL_A_INF | FL_B_INF | (d_inf ? FL_L_INF : 0u) | (q_inf ? FL_C_INF : 0u);
        }
    }
    ws.flags[i] = flags;
    ws.g2bad[i] = 0;
    a.status[i] = ST_VERIFICATION_FAILED;
}

// the key points' multiples and joint P / phi(P) rows, as k_plonk_mult / k_plonk_joint build them for an SP1 key
__global__ __launch_bounds__(64) void k_plonk_keys_mult(PlonkKey* __restrict__ key) {
    if (threadIdx.x == 0 && blockIdx.x <= PK_POINTS) plonk_setup_mult(*key, (int)blockIdx.x);
}
__global__ __launch_bounds__(64) void k_plonk_keys_joint(PlonkKey* __restrict__ key) {
    const int t = (int)(blockIdx.x * 64 + threadIdx.x);
    if (t < (PK_POINTS + 1) * (PK_JA + 1)) plonk_joint_row(*key, t / (PK_JA + 1), t % (PK_JA + 1));
}
void launch_plonk_setup_keys(const PlonkKeyRaw* d_raw, PlonkKey* d_key, hipStream_t s) {
    hipLaunchKernelGGL(k_plonk_setup_keys, dim3(1), dim3(64), 0, s, d_raw, d_key);
    hipLaunchKernelGGL(k_plonk_keys_mult, dim3(PK_POINTS + 1), dim3(64), 0, s, d_key);
    hipLaunchKernelGGL(k_plonk_keys_joint, dim3(((PK_POINTS + 1) * (PK_JA + 1) + 63) / 64), dim3(64), 0, s, d_key);
}
void launch_plonk_prep_keys(const PrepArgs& a, const PlonkKey* d_key, const Workspace& ws, hipStream_t s) {
    if (!a.n) return;
    hipLaunchKernelGGL(k_plonk_prep_keys, dim3((unsigned)((a.n + ZKV_BLOCK - 1) / ZKV_BLOCK)), dim3(ZKV_BLOCK), 0, s, a, d_key, ws);
}

}  // namespace zkv

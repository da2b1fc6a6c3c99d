// Set-up of the fixed-base GT tables (zkv_gt.h), once per SP1 / RISC Zero context that runs lane-pair chunks.
//   k_gt_bases   one lane per per-proof signal: G_i = FE(ML(IC_i, gamma)) through the set-up pairing code that tabulates e(alpha, beta)
//                (miller_loop_m, then the library's final exponentiation), and the first entry G_i^(2^(20 j)) of every window by twenty
//                cyclotomic squarings each; a third lane folds ML(base, gamma) into the Miller constant beside ML(alpha, beta)
//   k_gt_level   level L: entry d = 2^L + t of every window from entry d / 2 -- one cyclotomic squaring, and one multiplication by the
//                window's first entry when d is odd
//   k_gt_torus   the last step: every entry t = g + h w is replaced by its affine torus value a = (1 + g) / h (zkv_gt.h), a0 a1 a2 in the
//                first 48 words of the entry's place.  In place: a lane reads and writes its own entry only.
// One value per lane (the Fp12 code of the set-up kernels); until k_gt_torus every entry is in the full layout g0 g1 g2 h0 h1 h2 x (c0, c1),
// 96 words, which the level launches read.
#include "zkv_internal.h"

namespace zkv {

__global__ __launch_bounds__(64) void k_gt_bases(const VkRaw* __restrict__ raw, const VkTables* __restrict__ t, uint32_t* __restrict__ tab, uint32_t* __restrict__ mconst,
                                                 uint32_t* __restrict__ scratch, uint32_t nw0, uint32_t nw1) {
    if (threadIdx.x != 0) return;
    const uint32_t b = blockIdx.x;                               // 0, 1: the signals; 2: the constant
    uint32_t* sc = scratch + (size_t)b * 12 * 96;
    MRef fm = m_ref(sc, 1), tm = m_ref(sc + 96, 1), E = m_ref(sc + 2 * 96, 1), Y1 = m_ref(sc + 3 * 96, 1), Y3 = m_ref(sc + 4 * 96, 1), Y4 = m_ref(sc + 5 * 96, 1),
         W = m_ref(sc + 6 * 96, 1), acc = m_ref(sc + 9 * 96, 1);
    Fp2 gx, gy;
    gx.c0 = fp_from_raw(raw->gamma[0]); gx.c1 = fp_from_raw(raw->gamma[1]);
    gy.c0 = fp_from_raw(raw->gamma[2]); gy.c1 = fp_from_raw(raw->gamma[3]);
    G1Norm n;
    n.lxs = n.lys = n.cxs = n.cys = fp_zero();
    if (b == 2) {
        MRef out = m_ref(mconst, 1), ab = m_ref(const_cast<uint32_t*>(t->f_alpha_beta), 1);
        if (t->base_inf) f12m_copy(out, ab);
        else {
            const Fp iy = fp_inv(t->base.y);
            n.axs = fp_mul(t->base.x, iy); n.ays = iy;
            miller_loop_m((const VkTables*)nullptr, 0, n, gx, gy, fm, tm);
            f12m_mul(out, fm, ab);
        }
        // ... and behind it the start value of the lane-pair loop, FE(constant)^e (miller_start_value, zkv_verify.h)
        f12m_copy(fm, out);
        miller_start_value(m_ref(mconst + 96, 1), fm, E, Y1, Y3, Y4, W, acc);
        return;
    }
    const uint32_t nw = b ? nw1 : nw0, row0 = b ? nw0 : 0u;
    const uint32_t ici = raw->var_ic[b];
    const Fp px = fp_from_raw(raw->ic[ici][0]), py = fp_from_raw(raw->ic[ici][1]);
    const Fp iy = fp_inv(py);
    n.axs = fp_mul(px, iy); n.ays = iy;
    miller_loop_m((const VkTables*)nullptr, 0, n, gx, gy, fm, tm);
    (void)final_exp_is_one_m(fm, E, Y1, Y3, Y4, W, acc);         // acc = ML^(k (p^12 - 1) / r): the GT value the verify path's program computes
#pragma unroll 1
    for (uint32_t j = 0; j < nw; j++) {
        f12m_copy(m_ref(tab + gt_row_word(row0 + j), 1), acc);
#pragma unroll 1
        for (uint32_t k = 0; k < GT_WINDOW_BITS; k++) f12m_cyclo_sqr(acc);
    }
}

__global__ __launch_bounds__(64) void k_gt_level(uint32_t* __restrict__ tab, uint32_t rows, uint32_t level) {
    const uint32_t cnt = level == GT_WINDOW_BITS - 1 ? 1u : 1u << level;     // the top level is the single entry d = 2^19
    const uint32_t tt = blockIdx.x * 64 + threadIdx.x, row = blockIdx.y;
    if (tt >= cnt || row >= rows) return;
    const uint32_t d = (1u << level) + tt;                                    // 2 <= d <= 2^19
    uint32_t* base = tab + gt_row_word(row);
    MRef dst = m_ref(base + (size_t)(d - 1) * GT_ENTRY_WORDS, 1), src = m_ref(base + (size_t)((d >> 1) - 1) * GT_ENTRY_WORDS, 1), one = m_ref(base, 1);
    f12m_copy(dst, src);
    f12m_cyclo_sqr(dst);
    if (d & 1u) f12m_mul(dst, dst, one);
}

__global__ __launch_bounds__(64) void k_gt_torus(uint32_t* __restrict__ tab, uint32_t rows) {
    const uint32_t e = blockIdx.x * 64 + threadIdx.x, row = blockIdx.y;
    if (e >= GT_ROW_ENTRIES || row >= rows) return;
    MRef t = m_ref(tab + gt_row_word(row) + (size_t)e * GT_ENTRY_WORDS, 1);
    Fp6 g = m_ld_f6(t, 0);
    const Fp6 h = m_ld_f6(t, 3);                                              // invertible: no entry is +-1 (zkv_gt.h)
    g.c0 = f2_add(g.c0, f2_one());
    m_st_f6(t, 0, f6_mul(g, f6_inv(h)));
}

// TEST ONLY (zkv_diag_gt_read): the full entry g + h w = (a + w) / (a - w) from its stored a: g = (a^2 + v) / (a^2 - v), h = 2 a / (a^2 - v).
__global__ __launch_bounds__(64) void k_gt_diag_expand(const uint32_t* __restrict__ a48, uint32_t* __restrict__ out96) {
    if (blockIdx.x != 0 || threadIdx.x != 0) return;
    MRef s = m_ref(const_cast<uint32_t*>(a48), 1), o = m_ref(out96, 1);
    const Fp6 a = m_ld_f6(s, 0), q = f6_mul(a, a);
    Fp6 num = q, den = q;
    num.c1 = f2_add(q.c1, f2_one()); den.c1 = f2_sub(q.c1, f2_one());
    const Fp6 di = f6_inv(den);
    m_st_f6(o, 0, f6_mul(num, di));
    m_st_f6(o, 3, f6_mul(f6_add(a, a), di));
}
// TEST ONLY (zkv_diag_gt_product): M = u / conj(u) for the n values u the walk left in the TMP rows (word k of proof i at tmp[k cap + i]);
// out and scr: 96 n words each, word k of proof i at [k n + i].
__global__ __launch_bounds__(64) void k_gt_diag_ratio(size_t n, const uint32_t* __restrict__ tmp, size_t cap, uint32_t* __restrict__ out, uint32_t* __restrict__ scr) {
    const size_t i = (size_t)blockIdx.x * 64 + threadIdx.x;
    if (i >= n) return;
    MRef u = m_ref(const_cast<uint32_t*>(tmp) + i, (uint32_t)cap), o = m_ref(out + i, (uint32_t)n), c = m_ref(scr + i, (uint32_t)n);
    f12m_copy(c, u);
    f12m_conj(c);
    f12m_inv(c, c);
    f12m_mul(o, u, c);
}

void launch_gt_bases(const VkRaw* d_raw, const VkTables* d_tab, uint32_t* tab, uint32_t* mconst, uint32_t* scratch, uint32_t nw0, uint32_t nw1, hipStream_t s) {
    hipLaunchKernelGGL(k_gt_bases, dim3(3), dim3(64), 0, s, d_raw, d_tab, tab, mconst, scratch, nw0, nw1);
}
void launch_gt_level(uint32_t* tab, uint32_t rows, uint32_t level, hipStream_t s) {
    if (!rows || level < 1 || level >= GT_WINDOW_BITS) return;
    const uint32_t cnt = level == GT_WINDOW_BITS - 1 ? 1u : 1u << level;
    hipLaunchKernelGGL(k_gt_level, dim3((cnt + 63) / 64, rows), dim3(64), 0, s, tab, rows, level);
}
void launch_gt_torus(uint32_t* tab, uint32_t rows, hipStream_t s) {
    if (!rows) return;
    hipLaunchKernelGGL(k_gt_torus, dim3(GT_ROW_ENTRIES / 64, rows), dim3(64), 0, s, tab, rows);
}
void launch_gt_diag_expand(const uint32_t* a48, uint32_t* out96, hipStream_t s) {
    hipLaunchKernelGGL(k_gt_diag_expand, dim3(1), dim3(64), 0, s, a48, out96);
}
void launch_gt_diag_ratio(size_t n, const uint32_t* tmp, size_t cap, uint32_t* out, uint32_t* scr, hipStream_t s) {
    if (!n) return;
    hipLaunchKernelGGL(k_gt_diag_ratio, dim3((unsigned)((n + 63) / 64)), dim3(64), 0, s, n, tmp, cap, out, scr);
}

}  // namespace zkv

// Host build of the long-key vk_x path (stylus_zkvm_verifiers_amd/csrc/zkv_verify.h: setup_long_row, long_ic_valid, long_msm_slice) for
// CPU-side tests.  TEST ONLY: the walk is sliced over `lanes` simulated lanes exactly as k_msm_long / k_vk_x_long deal the (signal, window)
// pairs, and the partial sums are folded in the kernels' butterfly order (lane l adds lane l ^ m for m = lanes / 2 .. 1).
#include <stdint.h>
#include <string.h>
#include <stdlib.h>
#include <vector>
#define ZKV_COUNT_FP_MUL 1
#include "../../stylus_zkvm_verifiers_amd/csrc/zkv_host_vk.h"

using namespace zkv;

namespace {
struct LongHost {
    std::vector<uint8_t> key;
    VkTables* t = nullptr;
    std::vector<G1A> tab;
    std::vector<uint32_t> win;
    uint32_t n_sig = 0;
    bool valid = false;
};
LongHost g;

// the context set-up of a long key: VkTables from alpha, beta, gamma, delta and IC[0] only, IC[1..] into their own rows
const LongHost& key_tables(const uint8_t* vk, int n_ic) {
    const size_t bytes = 448 + 64 * (size_t)n_ic;
    if (g.t && g.key.size() == bytes && memcmp(g.key.data(), vk, bytes) == 0) return g;
    g.key.assign(vk, vk + bytes);
    VkRaw raw; host::fill_vk_generic(raw, vk, 1u);
    if (!g.t) g.t = (VkTables*)malloc(sizeof(VkTables));
    memset(g.t, 0, sizeof *g.t);
    setup_validate(raw, *g.t);
    setup_base(raw, *g.t);
    setup_lines(raw.gamma, g.t->lines[0]);
    setup_lines(raw.delta, g.t->lines[1]);
    { uint32_t ab[96 + 48]; MRef fm = m_ref(ab, 1), tm = m_ref(ab + 96, 1); setup_alpha_beta(raw, *g.t, fm, tm); }
    g.n_sig = (uint32_t)n_ic - 1;
    std::vector<uint32_t> ic(16 * (size_t)g.n_sig);
    for (uint32_t b = 0; b < g.n_sig; b++) {
        host::be_to_limbs(&ic[16 * (size_t)b], vk + 448 + 64 * (size_t)(b + 1));
        host::be_to_limbs(&ic[16 * (size_t)b + 8], vk + 480 + 64 * (size_t)(b + 1));
    }
    g.valid = g.t->vk_valid && long_ic_valid(ic.data(), 0, g.n_sig, 1);
    g.tab.assign((size_t)g.n_sig * LONG_ROW_ENTRIES, G1A());
    g.win.assign(g.n_sig, 0);
    for (uint32_t b = 0; b < g.n_sig; b++)
        for (uint32_t w = 0; w < (uint32_t)MSM_MAX_WINDOWS; w++)
            setup_long_row((const uint32_t(*)[8])&ic[16 * (size_t)b], w, &g.tab[((size_t)b * MSM_MAX_WINDOWS + w) * MSM_DIGITS], &g.win[b]);
    return g;
}
// signals (n_sig x 32 bytes BE) staged as k_prep_groth16_long does (stride 1: one proof), then the sliced walk and the butterfly
G1J long_vk_x(const LongHost& h, const uint8_t* signals, uint32_t lanes) {
    std::vector<uint32_t> sig(8 * (size_t)h.n_sig + 1);
    for (uint32_t b = 0; b < h.n_sig; b++) load_be256(&sig[8 * (size_t)b], signals + 32 * (size_t)b);
    auto digit = [&](uint32_t b, uint32_t w) { return (sig[8 * b + (w >> 2)] >> ((w & 3) * 8)) & 255u; };
    std::vector<G1J> acc(lanes), nx(lanes);
    for (uint32_t l = 0; l < lanes; l++) acc[l] = long_msm_slice(h.n_sig, h.win.data(), h.tab.data(), digit, l, lanes);
    for (uint32_t m = lanes / 2; m > 0; m >>= 1) {
        for (uint32_t l = 0; l < lanes; l++) nx[l] = g1j_add(acc[l], acc[l ^ m]);
        acc.swap(nx);
    }
    G1J r = acc[0];
    if (!h.t->base_inf) r = g1j_add_affine(r, h.t->base.x, h.t->base.y);
    return r;
}
}  // namespace

extern "C" {
// compute_vk_x of a long key through the kernel walk: 1 and out64 = affine (x, y) big-endian ((0,0) = infinity), 0 when a key point
// is not a valid precompile input (the reference's ecMul / ecAdd call fails)
int hsl_vk_x(const uint8_t* vk_words, int n_ic, const uint8_t* signals, int lanes, uint8_t* out64) {
    const LongHost& h = key_tables(vk_words, n_ic);
    if (!h.valid) return 0;
    G1A a; uint32_t inf; g1j_to_affine(long_vk_x(h, signals, (uint32_t)lanes), a, inf);
    uint32_t r[8];
    for (int c = 0; c < 2; c++) {
        fp_to_raw(r, c ? a.y : a.x);
        for (int i = 0; i < 8; i++) for (int k = 0; k < 4; k++) out64[32 * c + 31 - 4 * i - k] = (uint8_t)(r[i] >> (8 * k));
    }
    return 1;
}
// verify_proof_with_key for a long key through the long-key PREP / MSM functions and the unchanged pairing stages
int hsl_verify(const uint8_t* vk_words, int n_ic, int negate_a, const uint8_t* words, const uint8_t* signals, int lanes) {
    const LongHost& h = key_tables(vk_words, n_ic);
    if (!h.valid) return 0;
    for (uint32_t b = 0; b < h.n_sig; b++) { uint32_t s[8]; load_be256(s, signals + 32 * (size_t)b); if (!raw_lt_r(s)) return 0; }
    PrepOut p; memset(&p, 0, sizeof p);
    uint32_t w[8][8];
    for (int k = 0; k < 8; k++) load_be256(w[k], words + 32 * k);
    if (!prep_points(w, negate_a != 0, p)) return 0;
    if (!(p.flags & FL_B_INF) && !g2_in_subgroup(p.bx, p.by)) return 0;
    G1Norm n; uint32_t fl = p.flags;
    msm_normalize_acc(long_vk_x(h, signals, (uint32_t)lanes), p, fl, n);
    static uint32_t buf[96 + 48], slots[8 * 96];
    MRef fm = m_ref(buf, 1), tm = m_ref(buf + 96, 1);
    miller_loop_m(h.t, fl, n, p.bx, p.by, fm, tm);
    MRef F = m_ref(slots, 1), E = m_ref(slots + 96, 1), Y1 = m_ref(slots + 192, 1), Y3 = m_ref(slots + 288, 1), Y4 = m_ref(slots + 384, 1);
    for (int k = 0; k < 96; k++) slots[k] = h.t->f_alpha_beta[k];
    f12m_mul(F, F, fm);
    return final_exp_is_one_m(F, E, Y1, Y3, Y4, m_ref(slots + 480, 1), fm) ? 1 : 0;
}
// multiply-adds (v_mad_u64_u32 on the device) of one proof's long-key walk with one lane per proof (the host count behind the issue-roof
// share of tools/bench_groth16_keys.py)
unsigned long long hsl_msm_mads(const uint8_t* vk_words, int n_ic, const uint8_t* signals) {
    const LongHost& h = key_tables(vk_words, n_ic);
    const unsigned long long d0 = zkv_mad_counter;
    (void)long_vk_x(h, signals, 1);
    return zkv_mad_counter - d0;
}
}

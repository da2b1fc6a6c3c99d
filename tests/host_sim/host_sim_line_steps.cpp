// Host emulation of the tangent and chord steps of the lane-pair Miller loop as fused column sums (line_dbl_sums / line_add_sums,
// csrc/zkv_line_sums.h) against the packed forms they are to replace (line_dbl / line_add, csrc/zkv_curve.h, followed by the two scalings
// of the line coefficients), on raw operands, with every update of a 64-bit column formed again in 128 bits and every operand of a sum
// piece held to its contract (ZKV_SHADOW_COLS, csrc/zkv_field.h).  The two lanes of a pair are two threads, as in host_sim_paired.cpp.
// The flat loop (miller_loop_p) is run with either pair of bodies.  TEST ONLY (tests/test_miller_line_steps_host.py).
#define ZKV_PAIRED 1
#define ZKV_COUNT_FP_MUL 1
#define ZKV_SHADOW_COLS 1
#include <atomic>
#include <stdint.h>
#include <string.h>
#include <thread>
#include "../../stylus_zkvm_verifiers_amd/csrc/zkv_verify.h"

static thread_local uint32_t tl_par = 0;
static volatile uint32_t g_xch[2];
static std::atomic<int> g_cnt{0}, g_gen{0};
static void pair_barrier() {
    int g = g_gen.load(std::memory_order_acquire);
    if (g_cnt.fetch_add(1, std::memory_order_acq_rel) == 1) { g_cnt.store(0, std::memory_order_relaxed); g_gen.fetch_add(1, std::memory_order_acq_rel); }
    else while (g_gen.load(std::memory_order_acquire) == g) std::this_thread::yield();
}
namespace zkv {
uint32_t zkv_parity() { return tl_par; }
uint32_t zkv_partner_u32(uint32_t x) {
    g_xch[tl_par] = x; pair_barrier();
    uint32_t r = g_xch[tl_par ^ 1u]; pair_barrier();
    return r;
}
}
using namespace zkv;

// One case: 96 words in -- X, Y, Z of the running point, then qx, qy of the affine point (every Fp2 as c0 then c1, eight little-endian
// words each), then xs and ys (eight words each) -- the integers as the slots hold them (Montgomery domain, any value below 2p).  Per body
// 96 words out, canonical: T.x T.y T.z l0 c3 c4 with c3 = l1 xs, c4 = l3 ys.  Bodies: 0 line_dbl and the scalings, 1 line_dbl_sums,
// 2 line_add and the scalings, 3 line_add_sums.  shadow[2 b], shadow[2 b + 1]: column updates of body b checked in 128 bits, and how many
// differed (operand-contract violations included); loose[b]: 1 when every output of body b stayed below 2p; mads[3 b ..]: multiply-adds
// charged (zkv_mad_counter), zkv_mad_issued_counter, and the signed excess of zkv_line_mad_excess_counter; muls[b]: Fp products charged.
enum { N_BODIES = 4 };
struct Job { int n; const uint32_t* in; uint32_t* out; unsigned long long shadow[2][2 * N_BODIES], muls[2][N_BODIES]; long long mads[2][3 * N_BODIES]; int loose[2][N_BODIES]; };
static Fp ld(const uint32_t* w) { Fp r; memcpy(r.v, w, 32); return r; }
static void lane(Job* j, uint32_t par) {
    tl_par = par;
    const uint32_t P2[8] = ZKV_FP_2P_LIMBS;
    for (int b = 0; b < N_BODIES; b++) {
        j->shadow[par][2 * b] = j->shadow[par][2 * b + 1] = 0; j->loose[par][b] = 1; j->muls[par][b] = 0;
        j->mads[par][3 * b] = j->mads[par][3 * b + 1] = j->mads[par][3 * b + 2] = 0;
    }
    uint32_t slot[24];
    MRef tm = m_ref(slot, 1, 8);                                  // the running point's slot, this lane's halves
    for (int i = 0; i < j->n; i++) {
        const uint32_t* in = j->in + (size_t)96 * i;
        const Fp xs = ld(in + 80), ys = ld(in + 88);
        const auto scale = [&](int k) { return k == 0 ? xs : ys; };
        for (int b = 0; b < N_BODIES; b++) {
            G2H T; T.x.h = ld(in + 8 * par); T.y.h = ld(in + 16 + 8 * par); T.z.h = ld(in + 32 + 8 * par);
            Fp2 qx, qy; qx.h = ld(in + 48 + 8 * par); qy.h = ld(in + 64 + 8 * par);
            Fp2 l0, l1, l3, c3, c4;
            const unsigned long long o0 = zkv_col_shadow_ops, b0 = zkv_col_shadow_bad, c0 = zkv_mad_counter, i0 = zkv_mad_issued_counter, m0 = zkv_fp_mul_counter;
            const long long e0 = zkv_line_mad_excess_counter;
            if (b == 0) { line_dbl(T, l0, l1, l3); c3 = f2_mul_fp(l1, xs); c4 = f2_mul_fp(l3, ys); }
            else if (b == 1) { m_st_f2(tm, 0, T.x); m_st_f2(tm, 1, T.y); m_st_f2(tm, 2, T.z); line_dbl_sums(tm, l0, c3, c4, scale); }
            else if (b == 2) { line_add(T, qx, qy, l0, l1, l3); c3 = f2_mul_fp(l1, xs); c4 = f2_mul_fp(l3, ys); }
            else { m_st_f2(tm, 0, T.x); m_st_f2(tm, 1, T.y); m_st_f2(tm, 2, T.z); line_add_sums(tm, qx, qy, l0, c3, c4, scale); }
            if (b & 1) { T.x = m_ld_f2(tm, 0); T.y = m_ld_f2(tm, 1); T.z = m_ld_f2(tm, 2); }
            j->shadow[par][2 * b] += zkv_col_shadow_ops - o0; j->shadow[par][2 * b + 1] += zkv_col_shadow_bad - b0;
            j->mads[par][3 * b] += (long long)(zkv_mad_counter - c0); j->mads[par][3 * b + 1] += (long long)(zkv_mad_issued_counter - i0);
            j->mads[par][3 * b + 2] += zkv_line_mad_excess_counter - e0; j->muls[par][b] += zkv_fp_mul_counter - m0;
            uint32_t* out = j->out + ((size_t)N_BODIES * i + b) * 96;
            const Fp o[6] = {T.x.h, T.y.h, T.z.h, l0.h, c3.h, c4.h};
            for (int k = 0; k < 6; k++) {
                if (u256_geq(o[k].v, P2)) j->loose[par][b] = 0;
                fp_to_raw(out + 16 * k + 8 * par, o[k]);
            }
        }
    }
}
extern "C" int hls_steps(int n, const uint32_t* in, uint32_t* out, unsigned long long* shadow, int* loose, long long* mads, unsigned long long* muls) {
    Job j; j.n = n; j.in = in; j.out = out;
    g_cnt = 0;
    std::thread t1(lane, &j, 1u);
    lane(&j, 0u);
    t1.join();
    for (int k = 0; k < 2 * N_BODIES; k++) shadow[k] = j.shadow[0][k] + j.shadow[1][k];
    for (int k = 0; k < 3 * N_BODIES; k++) mads[k] = j.mads[0][k] + j.mads[1][k];
    for (int b = 0; b < N_BODIES; b++) { loose[b] = j.loose[0][b] && j.loose[1][b]; muls[b] = j.muls[0][b] + j.muls[1][b]; }
    return N_BODIES;
}

// The borrow-free constants the bodies derive (limbs_kp_fat): out[0 .. 8] the form of 8p with lift 1, which must be ZKV_FP_FAT8P_LIMBS,
// then 2p and 5p with lift 1 and 4p with lift 2.
extern "C" void hls_fat_constants(uint32_t* out) {
    uint32_t F[9];
    limbs_kp_fat<8, 1>(F); memcpy(out, F, 36);
    limbs_kp_fat<2, 1>(F); memcpy(out + 9, F, 36);
    limbs_kp_fat<5, 1>(F); memcpy(out + 18, F, 36);
    limbs_kp_fat<4, 2>(F); memcpy(out + 27, F, 36);
}

// The whole flat loop (miller_loop_p with the fixed pairs of the tables, check_b on; sums != 0: the column-sum line steps k_miller2 takes,
// else line_dbl / line_add), then the closing product with the key's Miller
// constant and the final exponentiation.  out: the loop's value f (96 words: lane 0's six halves at words 16 k .. 16 k + 7, lane 1's
// behind them) and the GT value behind it, both canonical.  verdict[0]: the loop's subgroup verdict for B, verdict[1]: whether the GT value
// is one.  ops[0]: column updates checked, ops[1]: how many differed, ops[2]: the line steps' excess (signed, both lanes), ops[3]: the
// multiply-adds charged, ops[4]: zkv_mad_issued_counter.  Returns 1 when the two lanes agree on both verdicts, else -1.
struct MJob { int sums; const VkTables* t; uint32_t flags; const uint32_t* norm48; const uint32_t* b32; uint32_t* out; int verdict[2][2]; long long ops[2][5]; };
static uint32_t g_full[10 * 96];                                 // shared by the two lanes like the HBM slots
static void mlane(MJob* j, uint32_t par) {
    tl_par = par;
    auto S = [&](int s) { return m_ref(g_full + 96 * s + 8 * par, 1, 16); };
    MRef M = S(0), E = S(1), Y1 = S(2), Y3 = S(3), Y4 = S(4), W = S(5), acc = S(8);
    MRef mc = m_ref((uint32_t*)j->t->f_alpha_beta + 8 * par, 1, 16);
    uint32_t half[48 + 24];
    MRef fm = m_ref(half, 1, 8), tm = m_ref(half + 48, 1, 8);
    SoaRef norm = {j->norm48, 1, 0u}, bsrc = {j->b32 + 8 * par, 1, 0u};
    const unsigned long long o0 = zkv_col_shadow_ops, b0 = zkv_col_shadow_bad, c0 = zkv_mad_counter, i0 = zkv_mad_issued_counter;
    const long long e0 = zkv_line_mad_excess_counter;
    j->verdict[par][0] = (j->sums ? miller_loop_p<true>(j->t, j->flags, norm, bsrc, fm, tm, true) : miller_loop_p<false>(j->t, j->flags, norm, bsrc, fm, tm, true)) ? 1 : 0;
    j->ops[par][0] = (long long)(zkv_col_shadow_ops - o0); j->ops[par][1] = (long long)(zkv_col_shadow_bad - b0);
    j->ops[par][2] = zkv_line_mad_excess_counter - e0;
    j->ops[par][3] = (long long)(zkv_mad_counter - c0); j->ops[par][4] = (long long)(zkv_mad_issued_counter - i0);
    for (int k = 0; k < 6; k++) fp_to_raw(j->out + 16 * k + 8 * par, m_ld_f2(fm, k).h);
    f12m_mul(M, fm, mc);
    j->verdict[par][1] = final_exp_is_one_m(M, E, Y1, Y3, Y4, W, acc) ? 1 : 0;
    for (int k = 0; k < 6; k++) fp_to_raw(j->out + 96 + 16 * k + 8 * par, m_ld_f2(acc, k).h);
}
extern "C" int hls_miller(int sums, const void* tables, uint32_t flags, const uint32_t* norm48, const uint32_t* b32, uint32_t* out, int* verdict, long long* ops) {
    MJob j; j.sums = sums; j.t = (const VkTables*)tables; j.flags = flags; j.norm48 = norm48; j.b32 = b32; j.out = out;
    g_cnt = 0;
    std::thread t1(mlane, &j, 1u);
    mlane(&j, 0u);
    t1.join();
    for (int k = 0; k < 5; k++) ops[k] = j.ops[0][k] + j.ops[1][k];
    if (j.verdict[0][0] != j.verdict[1][0] || j.verdict[0][1] != j.verdict[1][1]) return -1;
    verdict[0] = j.verdict[0][0]; verdict[1] = j.verdict[0][1];
    return 1;
}

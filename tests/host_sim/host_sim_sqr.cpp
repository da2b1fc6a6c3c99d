// Host emulation of the Fp12 squaring of the lane-pair Miller loop (f12m_sqr_body, csrc/zkv_tower_mem.h): the six direct column sums over
// the powers of w that the kernels run against the complex-squaring Karatsuba form they replaced (f12m_sqr_karatsuba_body), on raw
// operands, with every update of a 64-bit column formed again in 128 bits (ZKV_SHADOW_COLS, csrc/zkv_field.h).  The two lanes of a pair
// are two threads, as in host_sim_paired.cpp.  Built a second time with -DZKV_SQR_KARATSUBA the loop below squares with the Karatsuba
// body: the reference of the whole-loop comparison.  TEST ONLY (tests/test_miller_sqr_host.py).
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

// One case: 96 words in -- f as six Fp2 coefficients in memory order g0 g1 g2 h0 h1 h2, every Fp2 as c0 then c1, eight little-endian
// words each, the integers as the slots hold them (Montgomery domain, any value below 2p) -- and per body 96 words out, brought out of
// Montgomery form (canonical).  Bodies: 0 the column sums, 1 the Karatsuba form.  shadow[2 b], shadow[2 b + 1]: column updates of body b
// checked in 128 bits, and how many of them differed (operand-contract violations of the sums included); loose[b]: 1 when every output
// of body b stayed below 2p; mads[3 b ..]: the multiply-adds body b was charged, issued according to zkv_mad_issued_counter, and the
// excess the squaring reports beside them (zkv_sqr_mad_excess_counter), summed over the cases and both lanes; muls[b]: Fp products charged.
enum { N_BODIES = 2 };
struct Job { int n; const uint32_t* in; uint32_t* out; unsigned long long shadow[2][2 * N_BODIES], mads[2][3 * N_BODIES], muls[2][N_BODIES]; int loose[2][N_BODIES]; };
static void lane(Job* j, uint32_t par) {
    tl_par = par;
    const uint32_t P2[8] = ZKV_FP_2P_LIMBS;
    for (int b = 0; b < N_BODIES; b++) {
        j->shadow[par][2 * b] = j->shadow[par][2 * b + 1] = 0; j->loose[par][b] = 1; j->muls[par][b] = 0;
        j->mads[par][3 * b] = j->mads[par][3 * b + 1] = j->mads[par][3 * b + 2] = 0;
    }
    uint32_t half[48];
    MRef fm = m_ref(half, 1, 8);
    for (int i = 0; i < j->n; i++) {
        const uint32_t* in = j->in + (size_t)96 * i;
        for (int b = 0; b < N_BODIES; b++) {
            for (int k = 0; k < 6; k++) memcpy(half + 8 * k, in + 16 * k + 8 * par, 32);
            const unsigned long long o0 = zkv_col_shadow_ops, b0 = zkv_col_shadow_bad, c0 = zkv_mad_counter, i0 = zkv_mad_issued_counter,
                                     e0 = zkv_sqr_mad_excess_counter, m0 = zkv_fp_mul_counter;
            if (b == 0) f12m_sqr_fused_body(fm);
            else f12m_sqr_karatsuba_body(fm);
            j->shadow[par][2 * b] += zkv_col_shadow_ops - o0; j->shadow[par][2 * b + 1] += zkv_col_shadow_bad - b0;
            j->mads[par][3 * b] += zkv_mad_counter - c0; j->mads[par][3 * b + 1] += zkv_mad_issued_counter - i0;
            j->mads[par][3 * b + 2] += zkv_sqr_mad_excess_counter - e0; j->muls[par][b] += zkv_fp_mul_counter - m0;
            uint32_t* out = j->out + ((size_t)N_BODIES * i + b) * 96;
            for (int k = 0; k < 6; k++) {
                if (u256_geq(half + 8 * k, P2)) j->loose[par][b] = 0;
                Fp v; memcpy(v.v, half + 8 * k, 32);
                fp_to_raw(out + 16 * k + 8 * par, v);
            }
        }
    }
}
extern "C" int hsq_squarings(int n, const uint32_t* in, uint32_t* out, unsigned long long* shadow, int* loose, unsigned long long* mads, unsigned long long* muls) {
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

// The whole flat loop (miller_loop_p, with the fixed pairs of the tables): f as the slots hold it after the loop, 96 words (lane 0's six
// halves at words 16 k .. 16 k + 7, lane 1's behind them), canonical.  Returns the number of column updates that differed from their
// 128-bit form; ops[0] how many were checked, ops[1] the excess the squarings report (both lanes).
struct MJob { const VkTables* t; uint32_t flags; const uint32_t* norm48; const uint32_t* b32; uint32_t* out; unsigned long long ops[2], bad[2], excess[2]; };
static void mlane(MJob* j, uint32_t par) {
    tl_par = par;
    uint32_t half[48 + 24];
    MRef fm = m_ref(half, 1, 8), tm = m_ref(half + 48, 1, 8);
    SoaRef norm = {j->norm48, 1, 0u}, bsrc = {j->b32 + 8 * par, 1, 0u};
    const unsigned long long o0 = zkv_col_shadow_ops, b0 = zkv_col_shadow_bad, e0 = zkv_sqr_mad_excess_counter;
    (void)miller_loop_p(j->t, j->flags, norm, bsrc, fm, tm, true);
    j->ops[par] = zkv_col_shadow_ops - o0; j->bad[par] = zkv_col_shadow_bad - b0; j->excess[par] = zkv_sqr_mad_excess_counter - e0;
    for (int k = 0; k < 6; k++) {
        Fp v; memcpy(v.v, half + 8 * k, 32);
        fp_to_raw(j->out + 16 * k + 8 * par, v);
    }
}
extern "C" unsigned long long hsq_miller(const void* tables, uint32_t flags, const uint32_t* norm48, const uint32_t* b32, uint32_t* out, unsigned long long* ops) {
    MJob j; j.t = (const VkTables*)tables; j.flags = flags; j.norm48 = norm48; j.b32 = b32; j.out = out;
    g_cnt = 0;
    std::thread t1(mlane, &j, 1u);
    mlane(&j, 0u);
    t1.join();
    ops[0] = j.ops[0] + j.ops[1]; ops[1] = j.excess[0] + j.excess[1];
    return j.bad[0] + j.bad[1];
}

// The per-context Miller constant as the loop's start value (miller_start_value, csrc/zkv_verify.h), with m = f_alpha_beta of the tables.
// out: four Fp12, canonical, 96 words each (lane 0's halves at words 16 k .. 16 k + 7, lane 1's behind them):
//   0  FE(m)                     1  FE(c^(2^64)), c = FE(m)^e, the 64 squarings taken with f12m_sqr
//   2  FE(loop from 1, times m)  3  FE(loop from c)
// verdict[0], verdict[1]: whether 2 and 3 are one.  Returns 1 when the two lanes agree on both verdicts, else -1.
struct SJob { const VkTables* t; uint32_t flags; const uint32_t* norm48; const uint32_t* b32; uint32_t* out; int verdict[2][2]; };
static uint32_t g_full[14 * 96];                                 // shared by the two lanes like the HBM slots
static void dump12(uint32_t* out, MRef a, uint32_t par) {
    for (int k = 0; k < 6; k++) fp_to_raw(out + 16 * k + 8 * par, m_ld_f2(a, k).h);
}
static void slane(SJob* j, uint32_t par) {
    tl_par = par;
    auto S = [&](int s) { return m_ref(g_full + 96 * s + 8 * par, 1, 16); };
    MRef M = S(0), E = S(1), Y1 = S(2), Y3 = S(3), Y4 = S(4), W = S(5), acc = S(8), c = S(9), sq = S(10);
    MRef mc = m_ref((uint32_t*)j->t->f_alpha_beta + 8 * par, 1, 16);
    f12m_copy(M, mc);
    miller_start_value(c, M, E, Y1, Y3, Y4, W, acc);             // acc is left holding FE(m)
    dump12(j->out, acc, par);
    f12m_copy(sq, c);
    for (int i = 0; i < 64; i++) f12m_sqr(sq);
    (void)final_exp_is_one_m(sq, E, Y1, Y3, Y4, W, acc);
    dump12(j->out + 96, acc, par);
    uint32_t half[48 + 24];
    MRef fm = m_ref(half, 1, 8), tm = m_ref(half + 48, 1, 8);
    SoaRef norm = {j->norm48, 1, 0u}, bsrc = {j->b32 + 8 * par, 1, 0u};
    (void)miller_loop_p(j->t, j->flags, norm, bsrc, fm, tm, true);
    f12m_mul(M, fm, mc);
    j->verdict[par][0] = final_exp_is_one_m(M, E, Y1, Y3, Y4, W, acc) ? 1 : 0;
    dump12(j->out + 2 * 96, acc, par);
    (void)miller_loop_p(j->t, j->flags, norm, bsrc, fm, tm, true, g_full + 96 * 9);
    f12m_copy(M, fm);
    j->verdict[par][1] = final_exp_is_one_m(M, E, Y1, Y3, Y4, W, acc) ? 1 : 0;
    dump12(j->out + 3 * 96, acc, par);
}
extern "C" int hsq_start_value(const void* tables, uint32_t flags, const uint32_t* norm48, const uint32_t* b32, uint32_t* out, int* verdict) {
    SJob j; j.t = (const VkTables*)tables; j.flags = flags; j.norm48 = norm48; j.b32 = b32; j.out = out;
    g_cnt = 0;
    std::thread t1(slane, &j, 1u);
    slane(&j, 0u);
    t1.join();
    if (j.verdict[0][0] != j.verdict[1][0] || j.verdict[0][1] != j.verdict[1][1]) return -1;
    verdict[0] = j.verdict[0][0]; verdict[1] = j.verdict[0][1];
    return 1;
}
// The constants of the start value and the host's assertion on them: hr = h mod r, e, eight little-endian words each.
extern "C" int hsq_start_exponent(uint32_t* hr, uint32_t* e) {
    const uint32_t HR[8] = ZKV_MILLER_START_HR, EX[8] = ZKV_MILLER_START_E;
    for (int i = 0; i < 8; i++) { hr[i] = HR[i]; e[i] = EX[i]; }
    return miller_start_exponent_ok() ? ZKV_MILLER_START_E_BITS : -1;
}

// Host emulation of the variable-line product of the lane-pair Miller loop (f12m_mul_by_034_body, csrc/zkv_tower_mem.h): the fused
// three-product form the kernels run against the Karatsuba form it replaced, on raw operands, with every update of a 64-bit column
// formed again in 128 bits (ZKV_SHADOW_COLS, csrc/zkv_field.h).  The two lanes of a pair are two threads, as in host_sim_paired.cpp.
// TEST ONLY (tests/test_miller_var_line_host.py).
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

// One case: 144 words in -- f as six Fp2 coefficients in memory order g0 g1 g2 h0 h1 h2, then c0, c3, c4, every Fp2 as c0 then c1, eight
// little-endian words each, the integers as the slots hold them (Montgomery domain, any value below 2p) -- and per body 96 words out,
// brought out of Montgomery form (canonical).  Bodies: 0 the fused product, 1 the Karatsuba product, 2 the fixed-line product
// f (1 + c3 w + c4 w^3), 3 the squaring of f.  shadow[2 b], shadow[2 b + 1]: column updates of body b checked in 128 bits, and how many
// of them differed; loose[b]: 1 when every output of body b stayed below 2p.  Only the first nb bodies run (their output rows are written).
enum { N_BODIES = 4 };
struct Job { int n, nb; const uint32_t* in; uint32_t* out; unsigned long long shadow[2][2 * N_BODIES]; int loose[2][N_BODIES]; };
static void lane(Job* j, uint32_t par) {
    tl_par = par;
    const uint32_t P2[8] = ZKV_FP_2P_LIMBS;
    for (int b = 0; b < N_BODIES; b++) { j->shadow[par][2 * b] = j->shadow[par][2 * b + 1] = 0; j->loose[par][b] = 1; }
    uint32_t half[48];
    MRef fm = m_ref(half, 1, 8);
    for (int i = 0; i < j->n; i++) {
        const uint32_t* in = j->in + (size_t)144 * i;
        Fp2 c0, c3, c4;
        memcpy(c0.h.v, in + 96 + 8 * par, 32); memcpy(c3.h.v, in + 112 + 8 * par, 32); memcpy(c4.h.v, in + 128 + 8 * par, 32);
        for (int b = 0; b < j->nb; b++) {
            for (int k = 0; k < 6; k++) memcpy(half + 8 * k, in + 16 * k + 8 * par, 32);
            const unsigned long long o0 = zkv_col_shadow_ops, b0 = zkv_col_shadow_bad;
            if (b == 0) f12m_mul_by_034_body(fm, c0, c3, c4);
            else if (b == 1) f12m_mul_by_034_karatsuba_body(fm, c0, c3, c4);
            else if (b == 2) f12m_mul_by_134_body(fm, c3, c4);
            else f12m_sqr_body(fm);
            j->shadow[par][2 * b] += zkv_col_shadow_ops - o0; j->shadow[par][2 * b + 1] += zkv_col_shadow_bad - b0;
            uint32_t* out = j->out + ((size_t)N_BODIES * i + b) * 96;
            for (int k = 0; k < 6; k++) {
                if (u256_geq(half + 8 * k, P2)) j->loose[par][b] = 0;
                Fp v; memcpy(v.v, half + 8 * k, 32);
                fp_to_raw(out + 16 * k + 8 * par, v);
            }
        }
    }
}
extern "C" int hsv_line_products(int n, int nb, const uint32_t* in, uint32_t* out, unsigned long long* shadow, int* loose) {
    if (nb < 1 || nb > N_BODIES) return -1;
    Job j; j.n = n; j.nb = nb; j.in = in; j.out = out;
    g_cnt = 0;
    std::thread t1(lane, &j, 1u);
    lane(&j, 0u);
    t1.join();
    for (int k = 0; k < 2 * N_BODIES; k++) shadow[k] = j.shadow[0][k] + j.shadow[1][k];
    for (int b = 0; b < N_BODIES; b++) loose[b] = j.loose[0][b] && j.loose[1][b];
    return N_BODIES;
}

// The whole flat loop (miller_loop_p, with the fixed pairs of the tables) under the same column check: returns the number of column
// updates that differed from their 128-bit form (operand-contract violations of the fused sums included), and in ops[0] how many were
// checked, in ops[1] the multiply-adds the loop was CHARGED (zkv_mad_counter, the work figure) and in ops[2] those it ISSUED
// (zkv_mad_issued_counter), both lanes.
struct MJob { const VkTables* t; uint32_t flags; const uint32_t* norm48; const uint32_t* b32; unsigned long long ops[2], bad[2], charged[2], issued[2]; };
static void mlane(MJob* j, uint32_t par) {
    tl_par = par;
    uint32_t half[48 + 24];
    MRef fm = m_ref(half, 1, 8), tm = m_ref(half + 48, 1, 8);
    SoaRef norm = {j->norm48, 1, 0u}, bsrc = {j->b32 + 8 * par, 1, 0u};
    const unsigned long long o0 = zkv_col_shadow_ops, b0 = zkv_col_shadow_bad, c0 = zkv_mad_counter, i0 = zkv_mad_issued_counter;
    (void)miller_loop_p(j->t, j->flags, norm, bsrc, fm, tm, true);
    j->ops[par] = zkv_col_shadow_ops - o0; j->bad[par] = zkv_col_shadow_bad - b0;
    j->charged[par] = zkv_mad_counter - c0; j->issued[par] = zkv_mad_issued_counter - i0;
}
extern "C" unsigned long long hsv_miller_shadow(const void* tables, uint32_t flags, const uint32_t* norm48, const uint32_t* b32, unsigned long long* ops) {
    MJob j; j.t = (const VkTables*)tables; j.flags = flags; j.norm48 = norm48; j.b32 = b32;
    g_cnt = 0;
    std::thread t1(mlane, &j, 1u);
    mlane(&j, 0u);
    t1.join();
    ops[0] = j.ops[0] + j.ops[1]; ops[1] = j.charged[0] + j.charged[1]; ops[2] = j.issued[0] + j.issued[1];
    return j.bad[0] + j.bad[1];
}

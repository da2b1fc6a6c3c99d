// Host build of the table walk's body on torus-compressed entries (stylus_zkvm_verifiers_amd/csrc/zkv_tower_mem.h: f12l9_mul_aw, the
// ZKV_PAIRED code k_finalexp2 runs, the two lanes of a pair played by two threads as in tests/host_sim/host_sim_paired.cpp) against the
// packed f12m_mul_body multiplying by the full element (+-a + w), coefficient by coefficient, for tests/test_gt_torus_host.py.
// Stand-alone: built and run once plain and once under AddressSanitizer and UndefinedBehaviorSanitizer.
// 1,000 seeded inputs; among them u = 1, D = 0, every operand at the largest representatives (just below 2p), keep = false (the
// accumulator must not change) and both signs; every input is compared in both lanes of the pair.
#define ZKV_PAIRED 1
#include <atomic>
#include <stdint.h>
#include <stdio.h>
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

constexpr int N_INPUTS = 1000;

struct Rng {
    uint64_t s;
    uint64_t next() { s ^= s << 13; s ^= s >> 7; s ^= s << 17; return s; }
    // a representative below 2p: 254 random bits (2^254 < 2p)
    Fp fp() { Fp r; for (int k = 0; k < 8; k += 2) { const uint64_t x = next(); r.v[k] = (uint32_t)x; r.v[k + 1] = (uint32_t)(x >> 32); } r.v[7] &= 0x3fffffffu; return r; }
};
static Fp two_p_minus(uint32_t k) {                          // 2p - k, k small and positive
    const uint32_t P2[8] = ZKV_FP_2P_LIMBS;
    Fp r; uint64_t br = k;
    for (int i = 0; i < 8; i++) { const uint64_t d = (uint64_t)P2[i] - br; r.v[i] = (uint32_t)d; br = (d >> 32) & 1u; }
    return r;
}

static int g_bad[2];
static int g_first_bad[2] = {-1, -1};

// One lane of the pair.  Both threads draw the same operands (component c of coefficient k is the (2 k + c)-th value) and keep their own.
static void lane(uint32_t par) {
    tl_par = par;
    static uint32_t full[2][4 * 96];                         // per lane: packed u, the entry a, the full element +-a + w, the reference product
    static uint32_t acc9[2][54 * 64];                        // per lane: the accumulator in resident limbs, one lane's column of the LDS slot
    uint32_t* mine = full[par];
    const L9Ref acc = l9_ref(acc9[par]);
    SoaRW U = {mine, 1, 0u}, A = {mine + 96, 1, 0u}, B = {mine + 2 * 96, 1, 0u}, D = {mine + 3 * 96, 1, 0u};
    Rng rng = {0x9e3779b97f4a7c15ull};
    const Fp one = fp_one(), zero = fp_zero();
    int bad = 0;
    for (int it = 0; it < N_INPUTS; it++) {
        Fp u[6][2], a[3][2];
        for (int k = 0; k < 6; k++) for (int c = 0; c < 2; c++) u[k][c] = rng.fp();
        for (int k = 0; k < 3; k++) for (int c = 0; c < 2; c++) a[k][c] = rng.fp();
        if (it == 0 || it == 1) for (int k = 0; k < 6; k++) for (int c = 0; c < 2; c++) u[k][c] = k == 0 && c == 0 ? one : zero;      // u = 1, both signs
        if (it == 2 || it == 3) for (int k = 3; k < 6; k++) for (int c = 0; c < 2; c++) u[k][c] = zero;                                // D = 0
        if (it >= 4 && it < 12) {                                                                                                       // just below 2p
            for (int k = 0; k < 6; k++) for (int c = 0; c < 2; c++) u[k][c] = two_p_minus(1u + (uint32_t)((it + k + c) % 3));
            for (int k = 0; k < 3; k++) for (int c = 0; c < 2; c++) a[k][c] = two_p_minus(1u + (uint32_t)((it + 2 * k + c) % 4));
        }
        const bool neg = (it & 1) != 0, keep = it % 7 != 5;
        for (int k = 0; k < 6; k++) { Fp2 x; x.h = u[k][par]; m_st_f2(U, k, x); l9_st(acc, k, l9_from_fp(x.h)); }
        for (int k = 0; k < 3; k++) {
            Fp2 x; x.h = a[k][par];
            m_st_f2(A, k, x);
            m_st_f2(B, k, neg ? f2_neg(x) : x);
        }
        m_st_f2(B, 3, f2_one()); m_st_f2(B, 4, f2_zero()); m_st_f2(B, 5, f2_zero());
        f12m_mul_body(D, U, B, false);
        f12l9_mul_aw(acc, A, neg, keep);
        for (int k = 0; k < 6; k++) {
            const L9 got9 = l9_ld(acc, k);
            bool ok = true;
            for (int i = 0; i < 8; i++) ok = ok && got9.l[i] < (1u << 29);                   // normalised limbs
            uint32_t got[8], want[8];
            fp_to_raw(got, l9_to_fp(got9));
            fp_to_raw(want, m_ld_f2(keep ? D : U, k).h);
            if (!ok || memcmp(got, want, sizeof got)) { bad++; if (g_first_bad[par] < 0) g_first_bad[par] = it; }
        }
    }
    g_bad[par] = bad;
}

int main() {
    std::thread t1(lane, 1u);
    lane(0u);
    t1.join();
    if (g_bad[0] || g_bad[1]) {
        printf("mismatch: %d coefficients in the even lane (first input %d), %d in the odd lane (first input %d)\n", g_bad[0], g_first_bad[0], g_bad[1], g_first_bad[1]);
        return 1;
    }
    printf("ok %d inputs\n", N_INPUTS);
    return 0;
}

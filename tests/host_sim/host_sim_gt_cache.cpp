// Host emulation of the walk-prefix cache (csrc/zkv_gt.h) around the lane-pair final exponentiation: the code k_gt_cache_fill,
// k_gt_cache_tag and k_finalexp2 run (final_exp_prog_p with tables, f12l9_mul_aw, gt_cache_*), with the two lanes of a pair played by two
// threads as in host_sim_paired.cpp.  TEST ONLY.
// The tables are SYNTHETIC: the caller sets the torus value a of every entry a run touches (any nonzero Fp6 value is a valid multiplier of
// the walk u <- u (sigma a + w)); rows keep the real geometry (gt_row_word, gt_entry_offset) in a sparse mapping.  What is tested is that a
// walk which starts from the cached u gives the verdict and the u of the walk over all windows -- a property of the program, whatever
// the entries are.
#define ZKV_PAIRED 1
#include <atomic>
#include <stdint.h>
#include <string.h>
#include <sys/mman.h>
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

static uint32_t* g_tab = nullptr;
static uint32_t g_nw0 = 0, g_nw1 = 0;
static GtCache g_cache;

// rows of the real size, untouched pages never materialise
extern "C" int hs_gtc_init(uint32_t nw0, uint32_t nw1) {
    if (!nw0 || !nw1 || nw0 > GT_MAX_WINDOWS || nw1 > GT_MAX_WINDOWS) return -1;
    if (g_tab) munmap(g_tab, (size_t)(g_nw0 + g_nw1) * GT_ROW_BYTES);
    g_tab = nullptr;
    void* p = mmap(nullptr, (size_t)(nw0 + nw1) * GT_ROW_BYTES, PROT_READ | PROT_WRITE, MAP_PRIVATE | MAP_ANONYMOUS | MAP_NORESERVE, -1, 0);
    if (p == MAP_FAILED) return -1;
    g_tab = (uint32_t*)p; g_nw0 = nw0; g_nw1 = nw1;
    return 0;
}
// a0 a1 a2 of one entry, (c0, c1) each: 48 words in the library's Montgomery form
extern "C" int hs_gtc_set_entry(uint32_t row, uint32_t mag, const uint32_t* w48) {
    if (!g_tab || row >= g_nw0 + g_nw1 || mag < 1 || mag > GT_ROW_ENTRIES) return -1;
    memcpy(g_tab + gt_row_word(row) + gt_entry_offset(mag) / 4, w48, 48 * 4);
    return 0;
}
extern "C" void hs_gtc_reset() {
    memset(&g_cache, 0, sizeof g_cache);
    g_cache.entries = GT_CACHE_ENTRIES;
}
extern "C" void hs_gtc_state(uint32_t* out3) {
    out3[0] = 0;
    for (uint32_t e = 0; e < GT_CACHE_ENTRIES; e++) out3[0] += g_cache.valid[e] ? 1u : 0u;
    out3[1] = g_cache.fills; out3[2] = g_cache.cursor;
}

// ---- what the selected pair of k_gt_cache_fill does for `key`: the walk over signal 0's windows from u = 1, u stored at the cursor
static void fill_lane(const uint32_t* key, uint32_t par) {
    tl_par = par;
    static thread_local uint32_t acc9[54 * 64];
    L9Ref acc = l9_ref(acc9);
    f12m_set_one(acc);
    for (uint32_t j = 0; j < g_nw0; j++) {
        const int32_t dg = gt_digit(key, j);
        if (dg == 0) continue;
        SoaRW T;
        T.p = g_tab + gt_row_word(j); T.stride = 1;
        T.off = gt_entry_offset((uint32_t)(dg < 0 ? -dg : dg)) + 32u * par;
        f12l9_mul_aw(acc, T, dg < 0, true);
    }
    const uint32_t slot = g_cache.cursor % GT_CACHE_ENTRIES;
    f12m_copy(m_ref(g_cache.val[slot] + 8 * par, 1, 16), acc);
    (void)zkv_partner_u32(0);                                       // both lanes have read the cursor and stored their half
    if (!par) (void)gt_cache_claim(g_cache, key);
}
extern "C" int hs_gtc_fill(const uint32_t* key8) {
    if (!g_tab) return -1;
    const uint32_t slot = g_cache.cursor % GT_CACHE_ENTRIES;
    g_cnt = 0;
    std::thread t1(fill_lane, key8, 1u);
    fill_lane(key8, 0u);
    t1.join();
    return (int)slot;
}

// ---- one pair through k_miller2's product (tables != nullptr) or with the Miller value 1, then k_finalexp2's program with the walk
struct Job { const VkTables* t; uint32_t flags; const uint32_t* norm48; const uint32_t* b32; const uint32_t* sc16; const uint8_t* tag; uint32_t* full; int accept[2]; };
static void lane(Job* j, uint32_t par) {
    tl_par = par;
    static thread_local uint32_t half[48 + 24];
    uint32_t* full = j->full;                        // F and the seven cold slots, shared by the two lanes like the HBM rows
    MRef F = m_ref(full + 8 * par, 1, 16);
    if (j->t) {
        MRef fm = m_ref(half, 1, 8), tm = m_ref(half + 48, 1, 8);
        SoaRef norm = {j->norm48, 1, 0u}, bsrc = {j->b32 + 8 * par, 1, 0u};
        if (!miller_loop_p(j->t, j->flags, norm, bsrc, fm, tm, true)) { j->accept[par] = -2; return; }
        MRef ab = m_ref((uint32_t*)j->t->f_alpha_beta + 8 * par, 1, 16);
        f12m_mul(F, fm, ab);
    } else f12m_set_one(F);
    static thread_local uint32_t acc9[54 * 64];
    uint32_t* ebase = full + 96;
    const GtRef g = {true, (ptrdiff_t)(g_tab - ebase), j->sc16, g_nw0, g_nw1, j->tag, (ptrdiff_t)(&g_cache.val[0][0] - ebase)};
    j->accept[par] = final_exp_prog_p(full, ebase, 1, 4u * 8u * par, l9_ref(acc9), g) ? 1 : 0;
}
// use_cache = 0: the walk without a cache (GtRef::tag == nullptr).  1: the tag byte is what k_gt_cache_tag computes (gt_cache_find).
// u96: the u the walk leaves in the slot TMP.  Returns verdict | tag << 8, -1 if the lanes disagree, -2 if B fails the subgroup test.
static int run_pair(Job& j) {
    std::thread t1(lane, &j, 1u);
    lane(&j, 0u);
    t1.join();
    if (j.accept[0] != j.accept[1]) return -1;
    return j.accept[0];
}
extern "C" int hs_gtc_run(const void* tables, uint32_t flags, const uint32_t* norm48, const uint32_t* b32, const uint32_t* sc16, int use_cache, uint32_t* u96) {
    if (!g_tab) return -1;
    static uint32_t full[8 * 96];
    const uint8_t tag = use_cache ? (uint8_t)gt_cache_find(g_cache, sc16) : 0;
    Job j; j.t = (const VkTables*)tables; j.flags = flags; j.norm48 = norm48; j.b32 = b32; j.sc16 = sc16; j.tag = use_cache ? &tag : nullptr; j.full = full;
    g_cnt = 0;
    const int r = run_pair(j);
    if (r < 0) return r;
    memcpy(u96, full + 96 * 7, 96 * 4);                          // TMP = slot 8: the seventh slot from E
    return r | ((int)tag << 8);
}

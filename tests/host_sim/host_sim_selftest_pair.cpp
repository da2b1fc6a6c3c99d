// Host build of the known-answer harness (stylus_zkvm_verifiers_amd/csrc/zkv_selftest.h), lane pairs and wide groups: the same case
// bodies k_selftest_pair.hip runs, every lane played by a thread.  The DPP exchange inside a pair is a shared slot and a two-thread
// barrier; the lockstep of a wide group (every load of a routine before its stores) and the work-group fence are a rendezvous of the
// group's threads (12 S: pairs 6 and 7 of the device only shadow pairs 0 and 1; where an op returns one word group per pair, theirs
// repeat those of pairs 0 and 1).  TEST ONLY.
#define ZKV_PAIRED 1
#include <atomic>
#include <stddef.h>
#include <stdint.h>
#include <thread>
#include <vector>
#include "../../stylus_zkvm_verifiers_amd/csrc/zkv_field.h"

static constexpr int PAIRS = 6, MAX_SLICES = 4;
static thread_local uint32_t tl_par = 0, tl_pair = 0;          // tl_pair = slice * PAIRS + coefficient
static int g_threads = 2;
struct Barrier {
    std::atomic<int> cnt{0}, gen{0};
    void wait(int n) {
        int g = gen.load(std::memory_order_acquire);
        if (cnt.fetch_add(1, std::memory_order_acq_rel) == n - 1) { cnt.store(0, std::memory_order_relaxed); gen.fetch_add(1, std::memory_order_acq_rel); }
        else while (gen.load(std::memory_order_acquire) == g) std::this_thread::yield();
    }
};
static Barrier g_pair_bar[PAIRS * MAX_SLICES], g_group_bar;
static volatile uint32_t g_xch[PAIRS * MAX_SLICES][2];
static uint32_t g_pair_tmp[PAIRS * MAX_SLICES][96];
namespace zkv {
uint32_t zkv_parity() { return tl_par; }
uint32_t zkv_partner_u32(uint32_t x) {
    g_xch[tl_pair][tl_par] = x; g_pair_bar[tl_pair].wait(2);
    uint32_t r = g_xch[tl_pair][tl_par ^ 1u]; g_pair_bar[tl_pair].wait(2);
    return r;
}
void zkv_wide_host_barrier() { g_group_bar.wait(g_threads); }
void zkv_wide_host_yield() { std::this_thread::yield(); }
uint32_t* zkv_wide_host_pair_tmp() { return g_pair_tmp[tl_pair]; }
}
#define ZKV_SELFTEST_BODIES 1
#include "../../stylus_zkvm_verifiers_amd/csrc/zkv_selftest.h"
using namespace zkv;

static void pair_lane(int op, size_t n, const uint32_t* in, uint32_t* out, int iw, int ow, uint32_t par) {
    tl_pair = 0; tl_par = par;
    std::vector<uint32_t> lds((144 + 54) * 64);          // this lane's column of the LDS block is column 0
    for (size_t i = 0; i < n; i++) selftest_pair(op, in + i * (size_t)iw, out + i * (size_t)ow, lds.data());
}
static uint32_t g_group[ST_WIDE_SLOT];
template <int S> static void wide_lane(int op, size_t n, const uint32_t* in, uint32_t* out, int iw, int ow, int slice, int pair, uint32_t par) {
    tl_pair = (uint32_t)(slice * PAIRS + pair); tl_par = par;
    const WL w = {pair, slice};
    for (size_t i = 0; i < n; i++) selftest_wide<S>(op, in + i * (size_t)iw, out + i * (size_t)ow, g_group, w);
}

// hs_selftest(mapping, op, n, in, out) for mappings 1 (lane pair), 2 (16 lanes, S = 1) and 3 (one wavefront, S = 4): what
// zkv_diag_primitive returns on the device; -1 for an unknown (mapping, op)
extern "C" int hs_selftest(int mapping, int op, size_t n, const uint32_t* in, uint32_t* out) {
    int iw = 0, ow = 0;
    if (mapping < 1 || !selftest_io(mapping, op, &iw, &ow)) return -1;
    std::vector<std::thread> ts;
    if (mapping == 1) {
        g_threads = 2;
        ts.emplace_back(pair_lane, op, n, in, out, iw, ow, 1u);
        pair_lane(op, n, in, out, iw, ow, 0u);
    } else {
        const int S = mapping == 2 ? 1 : 4;
        g_threads = 2 * PAIRS * S;
        for (int sl = 0; sl < S; sl++) for (int p = 0; p < PAIRS; p++) for (uint32_t h = 0; h < 2; h++) {
            if (!sl && !p && !h) continue;
            if (S == 1) ts.emplace_back(wide_lane<1>, op, n, in, out, iw, ow, sl, p, h);
            else ts.emplace_back(wide_lane<4>, op, n, in, out, iw, ow, sl, p, h);
        }
        if (S == 1) wide_lane<1>(op, n, in, out, iw, ow, 0, 0, 0u);
        else wide_lane<4>(op, n, in, out, iw, ow, 0, 0, 0u);
    }
    for (auto& t : ts) t.join();
    return 0;
}
// the (in, out) words per case of (mapping, op) as selftest_io states them; -1 for a pair this build does not run
extern "C" int hs_selftest_io(int mapping, int op, int* in_w, int* out_w) {
    return (mapping < 1 || !selftest_io(mapping, op, in_w, out_w)) ? -1 : 0;
}

// Host build of the selector routers' layout function (stylus_zkvm_verifiers_amd/csrc/zkv_gset_layout.h: route_layout) against brute
// force, for tests/test_route_layout_host.py.  Stand-alone: built and run once plain and once under AddressSanitizer and
// UndefinedBehaviorSanitizer.  No input; prints "ok <layouts checked>" or the first layout that fails, and exits non-zero then.
//
// Shapes: a gateway has [one own-context column] [0 .. 8 keyed columns] [own-context columns], 8 at the most; the router is the shape
// with one column in front and none behind.  Keyed records are 260 bytes, own-context ones 260 or 868.  Mappings: lanes 2, 16, 64,
// fixed by the caller or the start of the automatic choice.  Totals: exhaustive over small value sets, then seeded random ones up to
// 5,000 per column.  Behind the routed columns the totals go on with the unrouted columns, which the layout must not look at.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <vector>
#include "../../stylus_zkvm_verifiers_amd/csrc/zkv_gset_layout.h"

using namespace zkv;

struct Case { uint32_t n_cols, key0, n_keyed; uint32_t tot[ROUTE_MAX_COLS + 3], rec[ROUTE_MAX_COLS]; int lanes, fixed; };

static void fail(const Case& k, const char* what) {
    printf("FAIL %s: n_cols %u key0 %u n_keyed %u lanes %d fixed %d tot", what, k.n_cols, k.key0, k.n_keyed, k.lanes, k.fixed);
    for (uint32_t c = 0; c < k.n_cols; c++) printf(" %u/%u", k.tot[c], k.rec[c]);
    printf("\n");
    exit(1);
}
#define CHECK(cond, what) do { if (!(cond)) fail(k, what); } while (0)

static bool keyed(const Case& k, uint32_t c) { return c >= k.key0 && c < k.key0 + k.n_keyed; }

static uint64_t n_checked = 0;
static void check(const Case& k) {
    RouteLayout* L = (RouteLayout*)malloc(sizeof(RouteLayout));      // (a heap block: a write past the struct is a sanitizer error)
    if (!L) abort();
    route_layout(k.tot, k.n_cols, k.key0, k.n_keyed, k.rec, k.lanes, k.fixed, L);
    // the keyed group is gset_choose's alone
    uint64_t gstart[ROUTE_MAX_COLS + 1] = {0}, M = 0;
    int lanes = 0;
    if (k.n_keyed) lanes = gset_choose(k.tot + k.key0, k.n_keyed, k.lanes, k.fixed, gstart, &M);
    CHECK(L->m == M && L->lanes == lanes, "group size or mapping");
    const uint32_t align = gset_align_of_lanes(L->lanes);
    for (uint32_t q = 0; q < k.n_keyed; q++) {
        CHECK(L->gstart[q] == gstart[q] && L->start[k.key0 + q] == L->g0 + gstart[q], "key start");
        CHECK(gstart[q] % align == 0, "key alignment");
    }
    if (k.n_keyed) CHECK(L->base[k.key0] == L->b0 && L->start[k.key0] == L->g0, "group origin");
    // every routed item a slot of its own; the other slots are pad slots, and only keyed columns have any
    std::vector<uint8_t> live((size_t)L->slots, 0), seen((size_t)L->slots, 0);
    uint64_t items = 0, keyed_items = 0;
    for (uint32_t c = 0; c < k.n_cols; c++) {
        for (uint32_t r = 0; r < k.tot[c]; r++) {
            const uint64_t slot = (uint64_t)L->start[c] + r;
            CHECK(slot < L->slots && !live[(size_t)slot], "slot taken twice or past the end");
            if (keyed(k, c)) CHECK(slot >= L->g0 && slot < L->g0 + L->m, "keyed slot outside the group");
            else CHECK(slot < L->g0 || slot >= L->g0 + L->m, "own-context slot inside the group");
            live[(size_t)slot] = 1;
        }
        items += k.tot[c];
        if (keyed(k, c)) keyed_items += k.tot[c];
    }
    CHECK(L->slots == items - keyed_items + L->m, "slot count");
    // records: 4-byte aligned, disjoint, inside the call's bytes; a keyed column's run to the next key's (pad slots have records)
    uint64_t lo[ROUTE_MAX_COLS], hi[ROUTE_MAX_COLS];
    for (uint32_t c = 0; c < k.n_cols; c++) {
        const uint64_t span = keyed(k, c) ? gstart[c - k.key0 + 1] - gstart[c - k.key0] : k.tot[c];
        lo[c] = L->base[c]; hi[c] = lo[c] + span * (keyed(k, c) ? k.rec[k.key0] : k.rec[c]);
        CHECK(lo[c] % 4 == 0 && hi[c] <= L->bytes, "record base");
        if (keyed(k, c)) CHECK(lo[c] == L->b0 + 260 * gstart[c - k.key0], "keyed record base");
        for (uint32_t d = 0; d < c; d++) CHECK(hi[d] <= lo[c] || hi[c] <= lo[d] || lo[c] == hi[c] || lo[d] == hi[d], "records overlap");
    }
    // the runs: exactly the live slots, each once, in slot order
    CHECK(L->n_runs <= k.n_cols, "run count");
    uint64_t at = 0;
    for (uint32_t q = 0; q < L->n_runs; q++) {
        CHECK(L->run_n[q] > 0 && L->run_at[q] >= at && L->run_at[q] + L->run_n[q] <= L->slots, "run bounds");
        for (uint64_t j = 0; j < L->run_n[q]; j++) seen[(size_t)(L->run_at[q] + j)]++;
        at = L->run_at[q] + L->run_n[q];
    }
    for (uint64_t j = 0; j < L->slots; j++) CHECK(seen[(size_t)j] == live[(size_t)j], "runs are not the live slots");
    free(L);
    n_checked++;
}

// a shape with its record sizes; the unrouted columns behind the routed ones hold `junk`
static Case shape(uint32_t key0, uint32_t n_keyed, uint32_t after, bool swapped, int lanes, int fixed, uint32_t junk) {
    Case k;
    k.n_cols = key0 + n_keyed + after; k.key0 = key0; k.n_keyed = n_keyed; k.lanes = lanes; k.fixed = fixed;
    for (uint32_t c = 0; c < ROUTE_MAX_COLS; c++) k.rec[c] = keyed(k, c) ? 260u : ((c < key0) != swapped ? 260u : 868u);
    for (uint32_t c = 0; c < ROUTE_MAX_COLS + 3; c++) k.tot[c] = junk;
    return k;
}

static void exhaustive(Case k, const std::vector<uint32_t>& values) {
    std::vector<uint32_t> digit(k.n_cols, 0);
    for (;;) {
        for (uint32_t c = 0; c < k.n_cols; c++) k.tot[c] = values[digit[c]];
        check(k);
        uint32_t c = 0;
        while (c < k.n_cols && ++digit[c] == values.size()) digit[c++] = 0;
        if (c == k.n_cols) return;
    }
}

static uint64_t rng_state = 0x17B0C0DEull;
static uint32_t rnd(uint32_t below) {                               // xorshift64*
    rng_state ^= rng_state >> 12; rng_state ^= rng_state << 25; rng_state ^= rng_state >> 27;
    return (uint32_t)(((rng_state * 0x2545F4914F6CDD1Dull) >> 33) % below);
}

int main() {
    const int lanes_of[3] = {2, 16, 64};
    const std::vector<uint32_t> few = {0, 1, 2, 3, 4, 5, 31, 32, 33}, some = {0, 1, 4, 33}, three = {0, 3, 33}, two = {0, 33};
    for (uint32_t key0 = 0; key0 <= 1; key0++)
        for (uint32_t n_keyed = 0; key0 + n_keyed <= 8; n_keyed++)
            for (uint32_t after = 0; key0 + n_keyed + after <= 8; after++)
                for (int mode = 0; mode < 12; mode++) {
                    const Case k = shape(key0, n_keyed, after, (mode & 1) != 0, lanes_of[(mode >> 1) % 3], mode >= 6, 7);
                    exhaustive(k, k.n_cols <= 3 ? few : k.n_cols <= 4 ? some : k.n_cols <= 6 ? three : two);
                }
    for (int t = 0; t < 400; t++) {
        const uint32_t key0 = rnd(2), n_keyed = rnd(9 - key0), after = rnd(9 - key0 - n_keyed);
        Case k = shape(key0, n_keyed, after, rnd(2) != 0, lanes_of[rnd(3)], (int)rnd(2), rnd(5000));
        for (uint32_t c = 0; c < k.n_cols; c++) k.tot[c] = rnd(4) ? rnd(5001) : rnd(3);
        check(k);
    }
    // the degenerate cases by name, with the figures worked out by hand (lane pairs, fixed: 32 proofs per wavefront)
    {
        Case k = shape(1, 3, 2, false, 2, 1, 9);                     // all columns empty; only unrouted items behind them
        for (uint32_t c = 0; c < k.n_cols; c++) k.tot[c] = 0;
        check(k);
        RouteLayout L;
        route_layout(k.tot, k.n_cols, k.key0, k.n_keyed, k.rec, k.lanes, k.fixed, &L);
        CHECK(L.slots == 0 && L.bytes == 0 && L.m == 0 && L.n_runs == 0, "empty call");
    }
    {
        Case k = shape(1, 3, 1, false, 2, 1, 0);                     // an empty keyed column between two non-empty ones
        const uint32_t tot[5] = {10, 5, 0, 7, 2};
        for (uint32_t c = 0; c < 5; c++) k.tot[c] = tot[c];
        check(k);
        RouteLayout L;
        route_layout(k.tot, k.n_cols, k.key0, k.n_keyed, k.rec, k.lanes, k.fixed, &L);
        CHECK(L.g0 == 10 && L.b0 == 2600 && L.m == 64 && L.lanes == 2, "group");
        CHECK(L.start[1] == 10 && L.start[2] == 42 && L.start[3] == 42 && L.start[4] == 74 && L.slots == 76, "starts");
        CHECK(L.base[3] == 2600 + 260 * 32 && L.base[4] == 2600 + 260 * 64 && L.bytes == L.base[4] + 2 * 868, "bases");
        CHECK(L.n_runs == 3 && L.run_at[0] == 0 && L.run_n[0] == 15 && L.run_at[1] == 42 && L.run_n[1] == 7 && L.run_at[2] == 74 && L.run_n[2] == 2, "runs");
    }
    {
        Case k = shape(1, 2, 0, false, 16, 1, 0);                    // a keyed block that is last (the router's shape), 4 proofs per wavefront
        const uint32_t tot[3] = {3, 6, 1};
        for (uint32_t c = 0; c < 3; c++) k.tot[c] = tot[c];
        check(k);
        RouteLayout L;
        route_layout(k.tot, k.n_cols, k.key0, k.n_keyed, k.rec, k.lanes, k.fixed, &L);
        CHECK(L.g0 == 3 && L.m == 12 && L.slots == 15 && L.bytes == 260 * 15, "last group");
        CHECK(L.n_runs == 2 && L.run_n[0] == 9 && L.run_at[1] == 11 && L.run_n[1] == 1, "last group runs");
    }
    printf("ok %llu\n", (unsigned long long)n_checked);
    return 0;
}

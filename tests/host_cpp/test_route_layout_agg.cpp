// Host build of the selector routers' layout with the aggregate check on the keyed group (stylus_zkvm_verifiers_amd/csrc/zkv_gset_layout.h:
// route_layout_agg) and of the PREP lane's two-region key lookup (zkv_gwset_prep.h: gwset_key_of_slot2) against brute force, for
// tests/test_keyed_group_aggregate_host.py.  Stand-alone: built and run once plain and once under AddressSanitizer and
// UndefinedBehaviorSanitizer.  No input; prints "ok <layouts checked>" or the first layout that fails, and exits non-zero then.
//
// Shapes: 1 .. 3 keyed columns with 0 .. 2 own-context columns around them, before, behind or on both sides; sub in {16, 64, 128, 256},
// so the unit A is 64, 64, 128, 256; every keyed total from {0, 1, A - 1, A, A + 1, 2A + 33}, own-context totals from {0, 1, 70} (one
// column) or {0, 70} (two); every capable mask, and no mask at all.  The brute force places every item by its rank as the place kernels
// do (gset_agg_slot) and reads the layout back slot by slot.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <vector>
#include "../../stylus_zkvm_verifiers_amd/csrc/zkv_gwset_prep.h"
#include "../../stylus_zkvm_verifiers_amd/csrc/zkv_gset_layout.h"

using namespace zkv;

struct Case { uint32_t n_cols, key0, n_keyed, sub; uint32_t tot[ROUTE_MAX_COLS + 3], rec[ROUTE_MAX_COLS]; uint8_t capable[ROUTE_MAX_COLS]; bool mask; int lanes; };

static void fail(const Case& k, const char* what) {
    printf("FAIL %s: n_cols %u key0 %u n_keyed %u sub %u lanes %d mask %d tot", what, k.n_cols, k.key0, k.n_keyed, k.sub, k.lanes, (int)k.mask);
    for (uint32_t c = 0; c < k.n_cols; c++) printf(" %u/%u", k.tot[c], k.rec[c]);
    printf(" capable");
    for (uint32_t q = 0; q < k.n_keyed; q++) printf(" %u", k.capable[q]);
    printf("\n");
    exit(1);
}
#define CHECK(cond, what) do { if (!(cond)) fail(k, what); } while (0)

static bool keyed(const Case& k, uint32_t c) { return c >= k.key0 && c < k.key0 + k.n_keyed; }

static uint64_t n_checked = 0, n_engaged = 0;
static void check(const Case& k) {
    RouteLayout* L = (RouteLayout*)malloc(sizeof(RouteLayout));      // (heap blocks: a write past a struct is a sanitizer error)
    RouteLayout* P = (RouteLayout*)malloc(sizeof(RouteLayout));
    RouteAggLayout* A = (RouteAggLayout*)malloc(sizeof(RouteAggLayout));
    if (!L || !P || !A) abort();
    const uint32_t unit = gset_agg_unit(k.sub), K = k.n_keyed;
    route_layout_agg(k.tot, k.n_cols, k.key0, K, k.rec, k.lanes, 0, k.mask ? k.capable : nullptr, k.sub, L, A);
    // what must come out: R and every key's share by the rule itself
    uint64_t R = 0, n = 0;
    uint32_t agg[ROUTE_MAX_COLS] = {0};
    for (uint32_t q = 0; q < K; q++) {
        agg[q] = k.mask && k.capable[q] ? k.tot[k.key0 + q] / unit * unit : 0u;
        R += agg[q];
    }
    for (uint32_t c = 0; c < k.n_cols; c++) n += k.tot[c];
    CHECK(A->R == R, "aggregate region size");
    for (uint32_t q = 0; q < K; q++) CHECK(A->agg[q] == agg[q] && A->rest[q] == k.tot[k.key0 + q] - agg[q], "key share");
    for (uint32_t q = 0; q <= K; q++) CHECK(A->pstart[q] == L->gstart[q], "per-proof starts are the layout's key starts");
    if (!R) {                                                      // nothing capable, or no key holds a unit: route_layout bit for bit
        memset(P, 0xA5, sizeof *P);
        RouteLayout* Q = (RouteLayout*)malloc(sizeof(RouteLayout));
        if (!Q) abort();
        memset(Q, 0xA5, sizeof *Q);
        route_layout(k.tot, k.n_cols, k.key0, K, k.rec, k.lanes, 0, P);
        route_layout_agg(k.tot, k.n_cols, k.key0, K, k.rec, k.lanes, 0, k.mask ? k.capable : nullptr, k.sub, Q, A);
        CHECK(memcmp(P, Q, sizeof *P) == 0, "not route_layout's result");
        free(Q);
    } else n_engaged++;
    // the stated slot bound
    CHECK(L->slots <= n + 31ull * K, "slot bound");
    // the per-proof region is gset_choose over the rests, behind the aggregate region
    uint64_t pst[ROUTE_MAX_COLS + 1] = {0}, pm = 0;
    const int lanes = gset_choose(A->rest, K, k.lanes, 0, pst, &pm);
    CHECK(L->lanes == lanes && L->m == R + pm, "group size or mapping");
    uint64_t as = 0;
    for (uint32_t q = 0; q < K; q++) {
        CHECK(A->astart[q] == as, "aggregate starts lie back to back");
        CHECK(A->pstart[q] == R + pst[q] && L->start[k.key0 + q] == L->g0 + A->pstart[q], "per-proof start");
        CHECK(L->base[k.key0 + q] == L->b0 + 260ull * A->pstart[q], "per-proof record base");
        as += agg[q];
    }
    CHECK(A->astart[K] == R && A->pstart[K] == L->m, "region ends");
    // place every item by its rank; own-context columns one slot per item from their start
    std::vector<int> owner((size_t)L->slots, -1);
    uint64_t own_before = 0, own_bytes_before = 0;
    for (uint32_t c = 0; c < k.n_cols; c++) {
        if (c < k.key0) { own_before += k.tot[c]; own_bytes_before += (uint64_t)k.tot[c] * k.rec[c]; }
        for (uint32_t r = 0; r < k.tot[c]; r++) {
            uint64_t slot;
            if (keyed(k, c)) {
                slot = L->g0 + gset_agg_slot(c - k.key0, r, A->agg, A->astart, A->pstart);
                CHECK(slot >= L->g0 && slot < L->g0 + L->m, "keyed slot outside the group");
                CHECK((r < agg[c - k.key0]) == (slot < L->g0 + R), "rank and region disagree");
            } else {
                slot = (uint64_t)L->start[c] + r;
                CHECK(slot < L->g0 || slot >= L->g0 + L->m, "own-context slot inside the group");
            }
            CHECK(slot < L->slots && owner[(size_t)slot] < 0, "slot taken twice or past the end");
            owner[(size_t)slot] = (int)c;
        }
    }
    // the own-context columns before and after the block are where route_layout puts them, given the block's size
    CHECK(L->g0 == own_before && L->b0 == own_bytes_before, "group origin");
    {
        uint64_t s = 0, b = 0;
        for (uint32_t c = 0; c < k.n_cols; c++) {
            if (keyed(k, c)) { if (c + 1 == k.key0 + K) { s = L->g0 + L->m; b = L->b0 + 260ull * L->m; } continue; }
            CHECK(L->start[c] == s && L->base[c] == b, "own-context column moved");
            s += k.tot[c]; b += (uint64_t)k.tot[c] * k.rec[c];
        }
        CHECK(L->slots == s && L->bytes == b, "call size");
    }
    // the aggregate region: no pad slot; every 64-slot block and every sub-batch inside one key; the two-region lookup names every slot's key
    uint32_t ast32[ROUTE_MAX_COLS] = {0}, pst32[ROUTE_MAX_COLS] = {0};
    for (uint32_t q = 0; q < K; q++) { ast32[q] = (uint32_t)A->astart[q]; pst32[q] = (uint32_t)A->pstart[q]; }
    CHECK(R % 64 == 0 && R % k.sub == 0 && R % unit == 0, "aggregate region is not whole units");
    for (uint64_t j = 0; j < R; j++) {
        const int o = owner[(size_t)(L->g0 + j)];
        CHECK(o >= 0, "pad slot in the aggregate region");
        CHECK(o == owner[(size_t)(L->g0 + j / 64 * 64)], "64-slot block spans two keys");
        CHECK(o == owner[(size_t)(L->g0 + j / k.sub * k.sub)], "sub-batch spans two keys");
        CHECK(o == owner[(size_t)(L->g0 + j / unit * unit)], "unit spans two keys");
    }
    for (uint64_t j = 0; j < L->m; j++) {
        const uint32_t key = gwset_key_of_slot2(ast32, pst32, K, (uint32_t)R, (uint32_t)(j / 64 * 64), (uint32_t)j);
        const int o = owner[(size_t)(L->g0 + j)];
        if (o >= 0) CHECK(key == (uint32_t)o - k.key0, "key of a live slot");
        else {                                                      // a pad slot: of the key whose per-proof part it pads
            CHECK(j >= R && key < K && j >= A->pstart[key] + A->rest[key] && j < A->pstart[key + 1], "key of a pad slot");
        }
        // PREP chunks begin at any multiple of 64 in the aggregate region and anywhere from R on: the region choice needs the block's first slot only
        if (j >= R) CHECK(gwset_key_of_slot2(ast32, pst32, K, (uint32_t)R, (uint32_t)R, (uint32_t)j) == key, "region of a per-proof block");
    }
    if (!R) for (uint64_t j = 0; j < L->m; j++)
        CHECK(gwset_key_of_slot2(ast32, pst32, K, 0, (uint32_t)(j / 64 * 64), (uint32_t)j) == gwset_key_of_slot(pst32, K, (uint32_t)j), "one-region lookup");
    // record offsets: group slot j at b0 + 260 j, so every live keyed slot's row lies inside the group's bytes and clear of the other columns
    for (uint32_t c = 0; c < k.n_cols; c++) {
        if (keyed(k, c)) continue;
        const uint64_t lo = L->base[c], hi = lo + (uint64_t)k.tot[c] * k.rec[c];
        CHECK(lo % 4 == 0 && hi <= L->bytes && (hi <= L->b0 || lo >= L->b0 + 260ull * L->m || lo == hi), "own-context records");
    }
    CHECK(L->b0 % 4 == 0 && L->b0 + 260ull * L->m <= L->bytes, "group records");
    // the runs: exactly the live slots, each once, in slot order; never more than the non-empty columns
    uint32_t nonempty = 0;
    for (uint32_t c = 0; c < k.n_cols; c++) nonempty += k.tot[c] ? 1u : 0u;
    CHECK(L->n_runs <= nonempty && L->n_runs <= ROUTE_MAX_COLS, "run count");
    std::vector<uint8_t> seen((size_t)L->slots, 0);
    uint64_t at = 0;
    for (uint32_t q = 0; q < L->n_runs; q++) {
        CHECK(L->run_n[q] > 0 && L->run_at[q] >= at && L->run_at[q] + L->run_n[q] <= L->slots, "run bounds");
        CHECK(q == 0 || L->run_at[q] > at, "two runs that lie back to back");
        for (uint64_t j = 0; j < L->run_n[q]; j++) seen[(size_t)(L->run_at[q] + j)]++;
        at = L->run_at[q] + L->run_n[q];
    }
    for (uint64_t j = 0; j < L->slots; j++) CHECK(seen[(size_t)j] == (owner[(size_t)j] >= 0 ? 1 : 0), "runs are not the live slots");
    if (R && K) {                                                   // adjacent keys: the aggregate region lies in one run
        uint32_t q = 0;
        while (q < L->n_runs && !(L->run_at[q] <= L->g0 && L->g0 + R <= L->run_at[q] + L->run_n[q])) q++;
        CHECK(q < L->n_runs, "aggregate region split over runs");
    }
    free(L); free(P); free(A);
    n_checked++;
}

int main() {
    const uint32_t subs[4] = {16, 64, 128, 256};
    const int lanes_of[3] = {2, 16, 64};
    for (uint32_t si = 0; si < 4; si++) {
        const uint32_t sub = subs[si], A = gset_agg_unit(sub);
        const uint32_t vals[6] = {0, 1, A - 1, A, A + 1, 2 * A + 33};
        for (uint32_t key0 = 0; key0 <= 2; key0++)
            for (uint32_t n_keyed = 1; n_keyed <= 3; n_keyed++)
                for (uint32_t after = 0; key0 + after <= 2; after++)
                    for (uint32_t mask = 0; mask <= (1u << n_keyed); mask++) {          // (the last value: no mask at all)
                        Case k;
                        memset(&k, 0, sizeof k);
                        k.n_cols = key0 + n_keyed + after; k.key0 = key0; k.n_keyed = n_keyed; k.sub = sub;
                        k.mask = mask < (1u << n_keyed);
                        for (uint32_t q = 0; q < n_keyed; q++) k.capable[q] = k.mask && ((mask >> q) & 1u) ? 1 : 0;
                        for (uint32_t c = 0; c < ROUTE_MAX_COLS; c++) k.rec[c] = keyed(k, c) ? 260u : (c < key0 ? 260u : 868u);
                        for (uint32_t c = 0; c < ROUTE_MAX_COLS + 3; c++) k.tot[c] = 7;   // unrouted columns behind: not to be looked at
                        k.lanes = lanes_of[(mask + key0 + after + si) % 3];
                        const uint32_t own3[3] = {0, 1, 70}, own2[2] = {0, 70};
                        const uint32_t n_own_vals = key0 + after == 2 ? 2u : 3u;
                        const uint32_t* own_vals = key0 + after == 2 ? own2 : own3;
                        std::vector<uint32_t> digit(k.n_cols, 0);
                        for (;;) {
                            for (uint32_t c = 0; c < k.n_cols; c++) k.tot[c] = keyed(k, c) ? vals[digit[c]] : own_vals[digit[c]];
                            check(k);
                            uint32_t c = 0;
                            while (c < k.n_cols && ++digit[c] == (keyed(k, c) ? 6u : n_own_vals)) digit[c++] = 0;
                            if (c == k.n_cols) break;
                        }
                    }
    }
    // one case by name, figures by hand: a router with 5 built-in seals, keys of 130 (capable), 100 (not capable) and 64 (capable) seals,
    // sub 16 (unit 64), lane pairs
    {
        Case k;
        memset(&k, 0, sizeof k);
        k.n_cols = 4; k.key0 = 1; k.n_keyed = 3; k.sub = 16; k.mask = true; k.lanes = 2;
        const uint32_t tot[4] = {5, 130, 100, 64};
        for (uint32_t c = 0; c < 4; c++) { k.tot[c] = tot[c]; k.rec[c] = 260; }
        k.capable[0] = 1; k.capable[2] = 1;
        check(k);
        RouteLayout L;
        RouteAggLayout A;
        route_layout_agg(k.tot, 4, 1, 3, k.rec, 2, 0, k.capable, 16, &L, &A);
        CHECK(A.R == 192 && A.agg[0] == 128 && A.agg[1] == 0 && A.agg[2] == 64, "named: shares");
        CHECK(A.astart[0] == 0 && A.astart[1] == 128 && A.astart[2] == 128 && A.astart[3] == 192, "named: aggregate starts");
        // rests 2, 100, 0: lane pairs would pad 102 proofs to 160 slots (> 1.25 x), 16 lanes pad them to 104
        CHECK(L.lanes == 16 && A.pstart[0] == 192 && A.pstart[1] == 196 && A.pstart[2] == 296 && L.m == 296, "named: per-proof region");
        CHECK(L.g0 == 5 && L.slots == 301 && L.bytes == 260 * 301, "named: call");
        CHECK(L.n_runs == 2 && L.run_at[0] == 0 && L.run_n[0] == 5 + 192 + 2 && L.run_at[1] == 5 + 196 && L.run_n[1] == 100, "named: runs");
    }
    if (!n_engaged) { printf("FAIL no layout engaged the check\n"); return 1; }
    printf("ok %llu\n", (unsigned long long)n_checked);
    return 0;
}

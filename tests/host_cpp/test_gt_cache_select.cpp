// Stand-alone test of the walk-prefix cache's selection logic (csrc/zkv_gt.h): sample positions, the at-least-twice rule, lowest index
// wins, absent candidates against a full cache, the cursor's wrap, keys that differ in their last word only.  The functions are the ones
// k_gt_cache_fill and k_gt_cache_tag run.  Prints "ok <checks>" or the first failed check.  Also built with
// -fsanitize=address,undefined by tests/test_gt_cache_host.py.
#include <stdio.h>
#include <string.h>
#include <stdlib.h>
#include <vector>
#include "../../stylus_zkvm_verifiers_amd/csrc/zkv_gt.h"

using namespace zkv;

static int g_checks = 0;
#define CHECK(x) do { g_checks++; if (!(x)) { printf("FAILED line %d: %s\n", __LINE__, #x); return 1; } } while (0)

struct Samples {
    std::vector<uint32_t> keys, ok;
    uint32_t m;
    explicit Samples(uint32_t m_) : keys(8 * m_, 0u), ok(m_, 1u), m(m_) {
        for (uint32_t k = 0; k < m; k++) set(k, 1000u + k);          // all distinct
    }
    void set(uint32_t k, uint32_t id, uint32_t top = 7u) {           // a key made of id: every word differs between ids
        for (int w = 0; w < 8; w++) keys[8 * k + w] = id * 0x9e3779b1u + (uint32_t)w;
        keys[8 * k + 7] ^= top;
    }
    int select(const GtCache& c) const { return gt_cache_select(c, keys.data(), ok.data(), m); }
};

static GtCache empty_cache() {
    GtCache c;
    memset(&c, 0, sizeof c);
    c.entries = GT_CACHE_ENTRIES;
    return c;
}

static int positions() {
    const size_t ns[] = {1, 31, 32, 33, 1000003};
    for (size_t n : ns) {
        const uint32_t m = gt_cache_samples(n);
        CHECK(m == (n < 32 ? n : 32));
        CHECK(gt_cache_sample_pos(n, 0) == 0);
        size_t prev = 0;
        for (uint32_t k = 0; k < m; k++) {
            const size_t p = gt_cache_sample_pos(n, k);
            CHECK(p < n);                                            // inside the chunk
            CHECK(k == 0 || p > prev);                               // strictly increasing: no proof is sampled twice
            CHECK(p == (size_t)((unsigned long long)k * n / m));     // evenly spread
            prev = p;
        }
        CHECK(n - 1 - prev <= n / m);                                // the last sample is within one stride of the end
    }
    CHECK(gt_cache_samples(0) == 0);
    // under 32 proofs every proof is its own sample
    for (uint32_t k = 0; k < 31; k++) CHECK(gt_cache_sample_pos(31, k) == k);
    CHECK(gt_cache_sample_pos(33, 31) == 31 && gt_cache_sample_pos(33, 16) == 16);
    CHECK(gt_cache_sample_pos(1000003, 31) == 968752);
    return 0;
}

static int selection() {
    GtCache c = empty_cache();
    {   // all distinct: nothing
        Samples s(32);
        CHECK(s.select(c) == -1);
        for (uint32_t k = 0; k < 32; k++) CHECK(!gt_cache_candidate(c, s.keys.data(), s.ok.data(), 32, k));
    }
    {   // one key twice: the lower of the two
        Samples s(32);
        s.set(9, 77); s.set(20, 77);
        CHECK(s.select(c) == 9);
        CHECK(gt_cache_candidate(c, s.keys.data(), s.ok.data(), 32, 20));
        // its twin unusable (a dead proof, e.g. a vkey >= R): occurs once among the usable samples
        s.ok[20] = 0;
        CHECK(s.select(c) == -1);
        s.ok[20] = 1; s.ok[9] = 0;
        CHECK(s.select(c) == -1);
    }
    {   // two repeated keys: the lowest index wins, whichever key it belongs to
        Samples s(32);
        s.set(5, 50); s.set(30, 50); s.set(3, 60); s.set(4, 60); s.set(31, 60);
        CHECK(s.select(c) == 3);
        s.ok[3] = 0;
        CHECK(s.select(c) == 4);
        s.ok[4] = 0;                                                 // 60 now occurs once
        CHECK(s.select(c) == 5);
    }
    {   // unusable samples with equal (stale) keys are no pair
        Samples s(32);
        s.set(1, 5); s.set(2, 5); s.ok[1] = s.ok[2] = 0;
        CHECK(s.select(c) == -1);
    }
    {   // fewer than 32 samples: entries beyond m are not looked at
        Samples s(32);
        s.set(2, 8); s.set(10, 8);
        CHECK(gt_cache_select(c, s.keys.data(), s.ok.data(), 10) == -1);
        CHECK(gt_cache_select(c, s.keys.data(), s.ok.data(), 11) == 2);
        CHECK(!gt_cache_candidate(c, s.keys.data(), s.ok.data(), 10, 10));
        CHECK(gt_cache_select(c, s.keys.data(), s.ok.data(), 1) == -1);
        CHECK(gt_cache_select(c, s.keys.data(), s.ok.data(), 0) == -1);
    }
    {   // equal in seven words, different in the eighth: different keys
        Samples s(32);
        s.set(6, 90, 7u); s.set(7, 90, 0x80000007u);
        for (int w = 0; w < 7; w++) CHECK(s.keys[8 * 6 + w] == s.keys[8 * 7 + w]);
        CHECK(s.keys[8 * 6 + 7] != s.keys[8 * 7 + 7]);
        CHECK(!gt_key_eq(&s.keys[8 * 6], &s.keys[8 * 7]));
        CHECK(s.select(c) == -1);
        s.set(7, 90, 7u);
        CHECK(gt_key_eq(&s.keys[8 * 6], &s.keys[8 * 7]));
        CHECK(s.select(c) == 6);
        // and different in the first word only
        s.keys[8 * 7] ^= 1u;
        CHECK(s.select(c) == -1);
    }
    return 0;
}

static int cache_and_cursor() {
    GtCache c = empty_cache();
    Samples s(32);
    // fill all slots, one insertion per "launch", the inserted key repeated in the samples
    for (uint32_t r = 0; r < GT_CACHE_ENTRIES; r++) {
        s.set(0, 200 + r); s.set(1, 200 + r);
        CHECK(s.select(c) == 0);
        CHECK(gt_cache_find(c, &s.keys[0]) == 0);
        const uint32_t slot = gt_cache_claim(c, &s.keys[0]);
        CHECK(slot == r && c.fills == r + 1 && c.cursor == (r + 1) % GT_CACHE_ENTRIES);
        CHECK(gt_cache_find(c, &s.keys[0]) == slot + 1);
        CHECK(s.select(c) == -1);                                    // cached now: not inserted again
    }
    CHECK(c.cursor == 0 && c.fills == GT_CACHE_ENTRIES);
    // a cached key repeated beside an absent repeated key at a higher index: the absent one is taken
    s.set(0, 200); s.set(1, 200); s.set(12, 300); s.set(13, 300);
    CHECK(gt_cache_find(c, &s.keys[0]) == 1);
    CHECK(s.select(c) == 12);
    // the full cache takes it at the wrapped cursor, evicting the oldest
    const uint32_t slot = gt_cache_claim(c, &s.keys[8 * 12]);
    CHECK(slot == 0 && c.cursor == 1 && c.fills == GT_CACHE_ENTRIES + 1);
    CHECK(gt_cache_find(c, &s.keys[8 * 12]) == 1);
    CHECK(gt_cache_find(c, &s.keys[0]) == 0);                        // 200 is gone ...
    CHECK(s.select(c) == 0);                                         // ... and a candidate again
    for (uint32_t r = 1; r < GT_CACHE_ENTRIES; r++) {                // the others are still there
        Samples t(1); t.set(0, 200 + r);
        CHECK(gt_cache_find(c, &t.keys[0]) == r + 1);
    }
    // a key that matches a slot in seven words is absent; an invalid slot with an equal key does not count
    uint32_t near[8];
    memcpy(near, c.key[2], sizeof near); near[7] ^= 0x10000000u;
    CHECK(gt_cache_find(c, near) == 0 && gt_cache_find(c, c.key[2]) == 3);
    c.valid[2] = 0;
    CHECK(gt_cache_find(c, c.key[2]) == 0);
    // the same key in two slots (cannot arise through select + claim): the lower slot is reported
    c.valid[2] = 1; memcpy(c.key[3], c.key[2], sizeof c.key[2]);
    CHECK(gt_cache_find(c, c.key[2]) == 3);
    // the all-zero key against an empty cache (valid flags, not key contents, decide)
    GtCache e = empty_cache();
    uint32_t zero[8] = {0};
    CHECK(gt_cache_find(e, zero) == 0);
    return 0;
}

int main() {
    if (positions() || selection() || cache_and_cursor()) return 1;
    printf("ok %d\n", g_checks);
    return 0;
}

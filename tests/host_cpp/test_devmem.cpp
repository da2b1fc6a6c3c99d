// The owners of csrc/zkv_devmem.h against a counting fake of the runtime (no HIP): growth policy, exact allocations, release and move
// semantics, the reset of an aggregate of owners, and a group of allocations with a refusal injected at every position.
#include <stdio.h>
#include <stdlib.h>
#include <set>
#include <utility>
#include <vector>

struct FakeApi {
    typedef int* event_t;
    typedef long* stream_t;
    static inline size_t live_blocks = 0, live_bytes = 0, live_events = 0, live_streams = 0, calls = 0, refuse_at = ~(size_t)0, max_live_blocks = 0;
    static inline std::vector<size_t> asked;             // every size asked of alloc, refused ones included
    static inline std::set<void*> blocks;
    static bool alloc(void** p, size_t bytes) {
        asked.push_back(bytes);
        if (calls++ == refuse_at) { *p = nullptr; return false; }
        *p = malloc(bytes ? bytes : 1);
        blocks.insert(*p);
        live_blocks++; live_bytes += bytes;
        if (live_blocks > max_live_blocks) max_live_blocks = live_blocks;
        return true;
    }
    static void free(void* p, size_t bytes) {
        if (!blocks.erase(p)) { printf("free of a block that is not live\n"); exit(1); }
        ::free(p);
        live_blocks--; live_bytes -= bytes;
    }
    static bool event_create(event_t* e, unsigned) { *e = new int(0); live_events++; return true; }
    static void event_destroy(event_t e) { delete e; live_events--; }
    static bool stream_create(stream_t* s) { *s = new long(0); live_streams++; return true; }
    static void stream_destroy(stream_t s) { delete s; live_streams--; }
    static void reset() { calls = 0; refuse_at = ~(size_t)0; max_live_blocks = live_blocks; asked.clear(); }
    static bool clean() { return !live_blocks && !live_bytes && !live_events && !live_streams && blocks.empty(); }
};
#define ZKV_DEVMEM_API FakeApi
#include "../../stylus_zkvm_verifiers_amd/csrc/zkv_devmem.h"

using namespace zkv;

static long checks = 0;
#define CHECK(x) do { checks++; if (!(x)) { printf("line %d: %s\n", __LINE__, #x); return 1; } } while (0)

struct Group {                                           // shaped like a context's device state: owners, a view and a flag, all defaulted
    DevBuf<uint32_t> rows[3];
    DevBuf<> staging[4], lone;
    DevEvent ev[5], done;
    DevStream copy, run;
    const uint32_t* view = nullptr;
    bool ready = false;
};
static int fill(Group& g) {                              // the shape of a reserve: a chain that stops at the first refusal
    if (g.rows[0].alloc(100) || g.rows[1].alloc(200) || g.rows[2].alloc(300) || g.staging[0].grow(10) || g.staging[1].grow(20) ||
        g.staging[2].grow(30) || g.staging[3].grow(40) || g.lone.alloc(7)) return ZKV_ERR_OOM;
    g.view = g.rows[0]; g.ready = true;
    return ZKV_OK;
}

int main() {
    {   // grow: nothing at need <= cap, else need + need / 4 + 4096, the old block freed BEFORE the new one is asked for
        FakeApi::reset();
        DevBuf<> b;
        CHECK(!b && b.cap() == 0);
        for (size_t need : {(size_t)1, (size_t)4095, (size_t)5000, (size_t)5121, (size_t)5122, (size_t)100000, (size_t)3, (size_t)1 << 20}) {
            const size_t before = FakeApi::asked.size(), cap0 = b.cap();
            uint8_t* p0 = b;
            CHECK(b.grow(need) == ZKV_OK);
            if (need <= cap0) CHECK(FakeApi::asked.size() == before && b.cap() == cap0 && (uint8_t*)b == p0);
            else CHECK(FakeApi::asked.size() == before + 1 && FakeApi::asked.back() == need + need / 4 + 4096 && b.cap() == FakeApi::asked.back());
            CHECK(b && FakeApi::live_blocks == 1 && FakeApi::live_bytes == b.cap());
        }
        CHECK(FakeApi::max_live_blocks == 1);                // never two live blocks for one buffer
        CHECK(b.grow(b.cap()) == ZKV_OK && FakeApi::max_live_blocks == 1);
        // a refused allocation: empty buffer, ZKV_ERR_OOM, and the old block is gone (it went first)
        FakeApi::refuse_at = FakeApi::calls;
        CHECK(b.grow(b.cap() + 1) == ZKV_ERR_OOM && !b && b.cap() == 0 && FakeApi::clean());
        CHECK(b.grow(16) == ZKV_OK && b.cap() == 16 + 4 + 4096);          // and usable again
        b.release(); b.release();                                        // twice is harmless
        CHECK(!b && b.cap() == 0 && FakeApi::clean());
    }
    {   // alloc: the exact size, replacing what was held; 0 stays empty without a call
        FakeApi::reset();
        DevBuf<uint64_t> t;
        for (size_t bytes : {(size_t)8, (size_t)4097, (size_t)24, (size_t)1 << 22}) {
            CHECK(t.alloc(bytes) == ZKV_OK && FakeApi::asked.back() == bytes && t.cap() == bytes && FakeApi::live_blocks == 1 && FakeApi::live_bytes == bytes);
        }
        CHECK(FakeApi::max_live_blocks == 1);
        const size_t n = FakeApi::asked.size();
        CHECK(t.alloc(0) == ZKV_OK && !t && FakeApi::asked.size() == n && FakeApi::clean());
        FakeApi::refuse_at = FakeApi::calls;
        CHECK(t.alloc(64) == ZKV_ERR_OOM && !t && t.cap() == 0 && FakeApi::clean());
        CHECK(t.alloc(64) == ZKV_OK);
        CHECK(t.as<uint8_t>() == (uint8_t*)(uint64_t*)t);                  // the typed accessor is the same address
    }
    CHECK(FakeApi::clean());                                             // (the destructor)
    {   // moves: the source is empty, the target's old block is released, nothing is freed twice
        FakeApi::reset();
        DevBuf<> a, b;
        CHECK(a.alloc(10) == ZKV_OK && b.alloc(20) == ZKV_OK);
        uint8_t* pa = a;
        DevBuf<> c(std::move(a));
        CHECK(!a && a.cap() == 0 && (uint8_t*)c == pa && c.cap() == 10 && FakeApi::live_blocks == 2);
        b = std::move(c);
        CHECK(!c && c.cap() == 0 && (uint8_t*)b == pa && b.cap() == 10 && FakeApi::live_blocks == 1 && FakeApi::live_bytes == 10);
        DevBuf<>& self = b;
        b = std::move(self);
        CHECK((uint8_t*)b == pa && FakeApi::live_blocks == 1);
        a.release(); c.release();
        DevEvent e, f;
        CHECK(!e && e.create(2) == ZKV_OK && e && FakeApi::live_events == 1);
        f = std::move(e);
        CHECK(!e && f && FakeApi::live_events == 1);
        CHECK(f.create() == ZKV_OK && FakeApi::live_events == 1);          // creating again lets the old one go
        f.release(); f.release();
        CHECK(FakeApi::live_events == 0);
        DevStream s, t;
        CHECK(s.create() == ZKV_OK && FakeApi::live_streams == 1);
        t = std::move(s);
        CHECK(!s && t && FakeApi::live_streams == 1);
        std::vector<DevEvent> v;                                         // (how the trace events and the per-device events are kept)
        for (int k = 0; k < 9; k++) { DevEvent x; CHECK(x.create() == ZKV_OK); v.push_back(std::move(x)); }
        CHECK(FakeApi::live_events == 9);
    }
    CHECK(FakeApi::clean());
    {   // an aggregate of owners reset to a default-constructed one: everything returned, views and flags back to their defaults
        FakeApi::reset();
        Group g;
        CHECK(fill(g) == ZKV_OK);
        for (auto& e : g.ev) CHECK(e.create() == ZKV_OK);
        CHECK(g.done.create(2) == ZKV_OK && g.copy.create() == ZKV_OK && g.run.create() == ZKV_OK);
        CHECK(FakeApi::live_blocks == 8 && FakeApi::live_events == 6 && FakeApi::live_streams == 2);
        CHECK(FakeApi::live_bytes == 100 + 200 + 300 + 7 + (10 + 2 + 4096) + (20 + 5 + 4096) + (30 + 7 + 4096) + (40 + 10 + 4096));
        g = Group();
        CHECK(FakeApi::clean() && !g.view && !g.ready && !g.rows[0] && !g.staging[3] && !g.done && !g.run);
        CHECK(fill(g) == ZKV_OK && FakeApi::live_blocks == 8);             // and it fills again
    }
    CHECK(FakeApi::clean());
    // a refusal at every position k of the group's allocations: the chain stops there, and releasing the group leaves nothing
    for (size_t k = 0; k < 8; k++) {
        FakeApi::reset();
        Group g;
        FakeApi::refuse_at = k;
        CHECK(fill(g) == ZKV_ERR_OOM && FakeApi::asked.size() == k + 1 && FakeApi::live_blocks == k && !g.ready);
        g = Group();
        CHECK(FakeApi::clean());
        FakeApi::reset();
        CHECK(fill(g) == ZKV_OK);                                          // a second reserve after the failed one
        FakeApi::refuse_at = FakeApi::calls + k;                           // ... and a failure while the group is full: old blocks go one by one
        CHECK((fill(g) == ZKV_ERR_OOM) == (k < 4));                        // (staging that fits asks for nothing: only the three exact rows and `lone` can be refused)
        g = Group();
        CHECK(FakeApi::clean());
    }
    printf("ok %ld\n", checks);
    return 0;
}

// Host build of the RISC Zero router's per-slot front end (stylus_zkvm_verifiers_amd/csrc/zkv_rzrouter_prep.h: rzrouter_prep_slot,
// rzrouter_column) and of the selector derivation over key words (zkv_host_vk.h), for tests/test_risc0_router_host.py.  Stand-alone:
// built and run once plain and once under AddressSanitizer and UndefinedBehaviorSanitizer.  Every input buffer is a heap block of exactly
// its length, so a read past a record, an image id or a journal digest is a sanitizer error.
//
//   prep    stdin lines "vk_valid len control_root(64 hex) control_id(64 hex) in_a(64 hex) in_b(64 hex or -) record(520 hex)" ->
//           "status flags sig0 .. sig4 (64 hex each) ax ay bx_re bx_im by_re by_im cx cy (64 hex each, canonical; zeros unless alive)".
//           in_b = "-": verify_integrity, in_a is the claim digest.  Each slot runs twice, from a staged row (4-byte aligned words, as the
//           kernel's LDS copy) with aligned inputs and byte by byte from odd addresses; the two must agree.
//   derive  stdin lines "control_root control_id key_words(1664 hex)" -> "key digest (64 hex) selector (8 hex)"
//   column  stdin lines "n_builtin n_keyed selector(8 hex) route selectors(8 hex each)" -> "column instance"
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>
#include "../../stylus_zkvm_verifiers_amd/csrc/zkv_rzrouter_prep.h"
#include "../../stylus_zkvm_verifiers_amd/csrc/zkv_host_vk.h"

using namespace zkv;

static std::vector<uint8_t> unhex(const std::string& s) {
    std::vector<uint8_t> o;
    if (s == "-") return o;
    for (size_t i = 0; i + 1 < s.size(); i += 2) o.push_back((uint8_t)strtoul(s.substr(i, 2).c_str(), nullptr, 16));
    return o;
}
static uint8_t* heap_copy(const std::vector<uint8_t>& v, size_t lead) {      // exactly lead + v.size() bytes; the data starts at +lead
    uint8_t* p = (uint8_t*)malloc(lead + v.size());
    if (!p) abort();
    if (!v.empty()) memcpy(p + lead, v.data(), v.size());
    return p;
}
static void put_limbs(const uint32_t* l) { for (int k = 7; k >= 0; k--) printf("%08x", l[k]); }
static void put_fp(const Fp& a) { uint32_t r[8]; fp_to_raw(r, a); printf(" "); put_limbs(r); }

// the route's constants as zkv_risc0_router_create forms them
static RzrRoute route_of(const uint8_t* root, const uint8_t* id) {
    RzrRoute rt;
    memset(&rt, 0, sizeof rt);
    uint8_t lo[16], hi[16], w[32];
    host::split_digest(root, lo, hi);
    memset(w, 0, 32); memcpy(w + 16, lo, 16); host::be_to_limbs(rt.cr0, w);
    memset(w, 0, 32); memcpy(w + 16, hi, 16); host::be_to_limbs(rt.cr1, w);
    host::be_to_limbs(rt.id, id);
    rt.id_ge_r = raw_lt_r(rt.id) ? 0u : 1u;
    return rt;
}

static int run_prep() {
    Risc0Consts kc;
    host::risc0_consts(kc);
    std::string line;
    while (std::getline(std::cin, line)) {
        std::istringstream in(line);
        unsigned vk_valid, len; std::string root_h, id_h, a_h, b_h, rec_h;
        if (!(in >> vk_valid >> len >> root_h >> id_h >> a_h >> b_h >> rec_h)) continue;
        const std::vector<uint8_t> root = unhex(root_h), id = unhex(id_h), ia = unhex(a_h), ib = unhex(b_h), rec = unhex(rec_h);
        if (root.size() != 32 || id.size() != 32 || ia.size() != 32 || (ib.size() != 32 && !ib.empty()) || rec.size() != 260) return 2;
        const RzrRoute rt = route_of(root.data(), id.data());
        uint32_t* row = (uint32_t*)malloc(260);
        if (!row) abort();
        memcpy(row, rec.data(), 260);
        uint8_t *a0 = heap_copy(ia, 0), *a1 = heap_copy(ia, 1), *b0 = ib.empty() ? nullptr : heap_copy(ib, 0), *b1 = ib.empty() ? nullptr : heap_copy(ib, 1);
        uint8_t* rec_b = heap_copy(rec, 1);
        RzrSlot a, b;
        GwsetRec ra = {row, nullptr}, rb = {nullptr, rec_b + 1};
        rzrouter_prep_slot(vk_valid, rt, kc, len, a0, b0, ra, a);
        rzrouter_prep_slot(vk_valid, rt, kc, len, a1 + 1, b1 ? b1 + 1 : nullptr, rb, b);
        if (a.status != b.status || a.flags != b.flags || memcmp(a.sig, b.sig, sizeof a.sig)) return 3;
        const bool alive = (a.flags & FL_ALIVE) != 0;
        if (alive && (memcmp(&a.o.ax, &b.o.ax, sizeof a.o.ax) || memcmp(&a.o.ay, &b.o.ay, sizeof a.o.ay) || memcmp(&a.o.bx, &b.o.bx, sizeof a.o.bx) ||
                      memcmp(&a.o.by, &b.o.by, sizeof a.o.by) || memcmp(&a.o.cx, &b.o.cx, sizeof a.o.cx) || memcmp(&a.o.cy, &b.o.cy, sizeof a.o.cy))) return 4;
        printf("%u %u", (unsigned)a.status, a.flags);
        for (int s = 0; s < 5; s++) { printf(" "); put_limbs(a.sig[s]); }
        const Fp z = fp_zero();
        put_fp(alive ? a.o.ax : z); put_fp(alive ? a.o.ay : z);
        put_fp(alive ? a.o.bx.c0 : z); put_fp(alive ? a.o.bx.c1 : z); put_fp(alive ? a.o.by.c0 : z); put_fp(alive ? a.o.by.c1 : z);
        put_fp(alive ? a.o.cx : z); put_fp(alive ? a.o.cy : z);
        printf("\n");
        free(row); free(a0); free(a1); free(b0); free(b1); free(rec_b);
    }
    return 0;
}

static int run_derive() {
    std::string line;
    while (std::getline(std::cin, line)) {
        std::istringstream in(line);
        std::string root_h, id_h, key_h;
        if (!(in >> root_h >> id_h >> key_h)) continue;
        const std::vector<uint8_t> root = unhex(root_h), id = unhex(id_h), key = unhex(key_h);
        if (root.size() != 32 || id.size() != 32 || key.size() != 832) return 2;
        uint8_t* k = heap_copy(key, 1);
        uint8_t d[32], sel[4];
        host::risc0_vk_digest_words(k + 1, 6, d);
        host::risc0_selector_with(root.data(), id.data(), d, sel);
        for (int i = 0; i < 32; i++) printf("%02x", d[i]);
        printf(" ");
        for (int i = 0; i < 4; i++) printf("%02x", sel[i]);
        printf("\n");
        free(k);
    }
    return 0;
}

static int run_column() {
    std::string line;
    while (std::getline(std::cin, line)) {
        std::istringstream in(line);
        unsigned nb, nk; std::string sel_h, s;
        if (!(in >> nb >> nk >> sel_h)) continue;
        std::vector<uint32_t> sels;
        while (in >> s) sels.push_back((uint32_t)strtoul(s.c_str(), nullptr, 16));
        if (sels.size() != nb + nk || nb + nk > (unsigned)RZR_MAX_ROUTES || nk > (unsigned)RZR_MAX_KEYED) return 2;
        uint32_t* tab = (uint32_t*)malloc(4 * sels.size() + 4);      // exactly the routes: a read past them is a sanitizer error
        if (!tab) abort();
        if (!sels.empty()) memcpy(tab, sels.data(), 4 * sels.size());
        uint32_t inst = 0;
        uint32_t* exact = (uint32_t*)realloc(tab, sels.empty() ? 4 : 4 * sels.size());
        if (!exact) abort();
        const int c = rzrouter_column(exact, nb, nk, (uint32_t)strtoul(sel_h.c_str(), nullptr, 16), &inst);
        printf("%d %u\n", c, inst);
        free(exact);
    }
    return 0;
}

int main(int argc, char** argv) {
    if (argc == 2 && !strcmp(argv[1], "prep")) return run_prep();
    if (argc == 2 && !strcmp(argv[1], "derive")) return run_derive();
    if (argc == 2 && !strcmp(argv[1], "column")) return run_column();
    return 1;
}

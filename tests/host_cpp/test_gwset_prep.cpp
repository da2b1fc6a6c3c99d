// Host build of the keyed gateway routes' per-slot front end (stylus_zkvm_verifiers_amd/csrc/zkv_gwset_prep.h: gwset_prep_slot,
// gwset_key_of_slot) and of the slot layout it relies on (zkv_gset_layout.h), for tests/test_sp1_gateway_keys_host.py.  Stand-alone: built
// and run once plain and once under AddressSanitizer and UndefinedBehaviorSanitizer.  Every input buffer is a heap block of exactly its
// length, so a read past a record, a program vkey or the public values is a sanitizer error.
//
//   prep    stdin lines "vk_valid len vkey(64 hex) pv(hex or -) record(520 hex)" -> "status flags sig0(64 hex) sig1(64 hex)".  Each slot
//           runs twice, from a staged row (4-byte aligned words, as the kernel's LDS copy) and byte by byte from an odd address; the two
//           must agree.
//   layout  stdin lines "lanes fixed cnt..." -> "lanes slots start... | key of every slot"
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>
#include "../../stylus_zkvm_verifiers_amd/csrc/zkv_gwset_prep.h"
#include "../../stylus_zkvm_verifiers_amd/csrc/zkv_gset_layout.h"

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

static int run_prep() {
    std::string line;
    while (std::getline(std::cin, line)) {
        std::istringstream in(line);
        unsigned vk_valid, len; std::string vkey_h, pv_h, rec_h;
        if (!(in >> vk_valid >> len >> vkey_h >> pv_h >> rec_h)) continue;
        const std::vector<uint8_t> vkey = unhex(vkey_h), pv = unhex(pv_h), rec = unhex(rec_h);
        if (vkey.size() != 32 || rec.size() != 260) return 2;
        uint32_t* vk_words = (uint32_t*)malloc(32);
        uint32_t* row = (uint32_t*)malloc(260);
        if (!vk_words || !row) abort();
        memcpy(vk_words, vkey.data(), 32); memcpy(row, rec.data(), 260);
        uint8_t* pv_a = heap_copy(pv, 0);
        uint8_t* pv_b = heap_copy(pv, 1);
        uint8_t* rec_b = heap_copy(rec, 1);
        GwsetSlot a, b;
        GwsetRec ra = {row, nullptr}, rb = {nullptr, rec_b + 1};
        gwset_prep_slot(vk_valid, len, vk_words, pv_a, pv.size(), ra, a);
        gwset_prep_slot(vk_valid, len, vk_words, pv_b + 1, pv.size(), rb, b);
        if (a.status != b.status || a.flags != b.flags || memcmp(a.sig, b.sig, sizeof a.sig)) return 3;
        if ((a.flags & FL_ALIVE) && (memcmp(&a.o.ax, &b.o.ax, sizeof a.o.ax) || memcmp(&a.o.by, &b.o.by, sizeof a.o.by) || memcmp(&a.o.cy, &b.o.cy, sizeof a.o.cy))) return 4;
        printf("%u %u ", (unsigned)a.status, a.flags); put_limbs(a.sig[0]); printf(" "); put_limbs(a.sig[1]); printf("\n");
        free(vk_words); free(row); free(pv_a); free(pv_b); free(rec_b);
    }
    return 0;
}

static int run_layout() {
    std::string line;
    while (std::getline(std::cin, line)) {
        std::istringstream in(line);
        int lanes, fixed;
        if (!(in >> lanes >> fixed)) continue;
        std::vector<uint32_t> cnt; uint32_t v;
        while (in >> v) cnt.push_back(v);
        std::vector<uint64_t> start(cnt.size() + 1);
        uint64_t slots = 0;
        const int got = gset_choose(cnt.data(), (uint32_t)cnt.size(), lanes, fixed, start.data(), &slots);
        std::vector<uint32_t> s32(cnt.size());
        for (size_t k = 0; k < cnt.size(); k++) s32[k] = (uint32_t)start[k];
        printf("%d %llu", got, (unsigned long long)slots);
        for (size_t k = 0; k < cnt.size(); k++) printf(" %u", s32[k]);
        printf(" |");
        for (uint64_t j = 0; j < slots; j++) printf(" %u", gwset_key_of_slot(s32.data(), (uint32_t)cnt.size(), (uint32_t)j));
        printf("\n");
    }
    return 0;
}

int main(int argc, char** argv) {
    if (argc == 2 && !strcmp(argv[1], "prep")) return run_prep();
    if (argc == 2 && !strcmp(argv[1], "layout")) return run_layout();
    return 1;
}

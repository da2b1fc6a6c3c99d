// Host build of what the RISC Zero router's set route adds to the kernels' header arithmetic, for tests/test_risc0_router_set_host.py.
// Stand-alone: built and run once plain and once under AddressSanitizer and UndefinedBehaviorSanitizer.  Every input is a heap block that
// ends with its last byte, so a read outside a seal is a sanitizer error.  TEST ONLY.
//
//   parse   the function k_rzset_front runs on every seal (stylus_zkvm_verifiers_amd/csrc/zkv_rzrouter_set.h rzs_parse): stdin lines
//           "shift set_selector(8 hex) seal(hex or -)" -> "kind depth root_len root_at".  The seal is parsed from a private copy placed
//           `shift` bytes (0 .. 31) past a 16-byte boundary, with the word loads its address allows, and from a second copy byte by byte.
//   ident   the identity pair of k_rzset_ident (rzs_fingerprint, rzs_equal): stdin lines "shift_a shift_b a(hex or -) b(hex or -)" ->
//           "fingerprint_a fingerprint_b equal" (8 hex each, then 0 / 1).
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>
#include "../../stylus_zkvm_verifiers_amd/csrc/zkv_rzrouter_set.h"

using namespace zkv;

static std::vector<uint8_t> unhex(const std::string& s) {
    std::vector<uint8_t> o;
    if (s == "-") return o;
    for (size_t i = 0; i + 1 < s.size(); i += 2) o.push_back((uint8_t)strtoul(s.substr(i, 2).c_str(), nullptr, 16));
    return o;
}
// a block of exactly shift + v.size() bytes (malloc blocks are 16-byte aligned): the copy starts `shift` bytes in and ends with the block
static uint8_t* placed(const std::vector<uint8_t>& v, unsigned shift, uint8_t** at) {
    uint8_t* blk = (uint8_t*)malloc(v.size() + shift ? v.size() + shift : 1);
    if (!blk) abort();
    if (!v.empty()) memcpy(blk + shift, v.data(), v.size());
    *at = blk + shift;
    return blk;
}

static int run_parse() {
    std::string line;
    while (std::getline(std::cin, line)) {
        std::istringstream in(line);
        unsigned shift; std::string sel_h, seal_h;
        if (!(in >> shift >> sel_h >> seal_h)) continue;
        if (shift > 31) return 2;
        const uint32_t sel = (uint32_t)strtoul(sel_h.c_str(), nullptr, 16);
        const std::vector<uint8_t> seal = unhex(seal_h);
        uint8_t *p, *q;
        uint8_t* b0 = placed(seal, shift, &p);
        uint8_t* b1 = placed(seal, 0, &q);
        const RzsSeal a = rzs_parse(p, seal.size(), (((uintptr_t)p) & 3u) == 0, sel);
        const RzsSeal b = rzs_parse(q, seal.size(), false, sel);         // byte loads whatever the address
        if (a.kind != b.kind || a.depth != b.depth || a.root_len != b.root_len || a.root_at != b.root_at) return 3;
        if (a.kind == RZS_CLAIM && (RZS_PATH_AT + 32ull * a.depth + 32 != a.root_at || a.root_at + a.root_len > seal.size())) return 4;
        printf("%u %u %u %llu\n", a.kind, a.depth, a.root_len, (unsigned long long)a.root_at);
        free(b0); free(b1);
    }
    return 0;
}

static int run_ident() {
    std::string line;
    while (std::getline(std::cin, line)) {
        std::istringstream in(line);
        unsigned sa, sb; std::string a_h, b_h;
        if (!(in >> sa >> sb >> a_h >> b_h)) continue;
        if (sa > 31 || sb > 31) return 2;
        const std::vector<uint8_t> a = unhex(a_h), b = unhex(b_h);
        uint8_t *pa, *pb;
        uint8_t* b0 = placed(a, sa, &pa);
        uint8_t* b1 = placed(b, sb, &pb);
        const uint32_t fa = rzs_fingerprint(pa, (uint32_t)a.size()), fb = rzs_fingerprint(pb, (uint32_t)b.size());
        const bool eq = rzs_equal(pa, (uint32_t)a.size(), pb, (uint32_t)b.size());
        if (eq != rzs_equal(pb, (uint32_t)b.size(), pa, (uint32_t)a.size())) return 3;
        printf("%08x %08x %d\n", fa, fb, eq ? 1 : 0);
        free(b0); free(b1);
    }
    return 0;
}

int main(int argc, char** argv) {
    if (argc == 2 && !strcmp(argv[1], "parse")) return run_parse();
    if (argc == 2 && !strcmp(argv[1], "ident")) return run_ident();
    return 1;
}

// Host build of what the calldata path of a RISC Zero router with a set route adds to the kernels, for
// tests/test_risc0_router_set_wire_host.py.  Stand-alone: built and run once plain and once under AddressSanitizer and
// UndefinedBehaviorSanitizer.  Every input is a heap block of exactly its length, so a read outside a call, a decoded seal or a method
// row is a sanitizer error.  TEST ONLY.
//
//   decode  the composed decode of one request as k_wire_rzset and k_rzset_front run it: rzw_parse on the call
//           (stylus_zkvm_verifiers_amd/csrc/zkv_wire_rzrouter.h), the body streamed as the kernel streams it (every uint8[] element, every
//           padding byte), the seal's bytes compacted into a block of exactly the seal's length -- for a uint8[] request the
//           rzsw_keep() bytes the arena gets, which the test expects to be all of a set seal --, then rzs_parse on them (zkv_rzrouter_set.h).
//           stdin lines "shift sel0 sel1 sel2 sel3 set_sel (8 hex each) calldata(hex or -)" ->
//           "ok form method seal_len kept kind depth root_len root_at first260(hex or -)".  The call is parsed from a private copy of
//           exactly its length `shift` bytes past a 16-byte boundary; shift 0 takes the aligned word loads.
//   arena   rzsw_arena_at (zkv_wire_rzset.h) over every blob offset below argv[2] and every decoded length below argv[3], for both
//           head sizes of a uint8[] request: alignment, room below floor(o1 / 32), disjoint from the placement of a request that begins
//           where this one ends, and monotone in the offset.  Prints "ok <checks>".
//   method  rzs_claim_given: stdin lines "methods(hex, one byte per row, or -) have_in_b i" -> "0" (derive the claim digest) or "1"
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>
#include "../../stylus_zkvm_verifiers_amd/csrc/zkv_wire_rzset.h"

using namespace zkv;

static std::vector<uint8_t> unhex(const std::string& s) {
    std::vector<uint8_t> o;
    if (s == "-") return o;
    auto nib = [](char c) { return (uint8_t)(c <= '9' ? c - '0' : (c | 0x20) - 'a' + 10); };
    o.resize(s.size() / 2);
    for (size_t i = 0; i < o.size(); i++) o[i] = (uint8_t)(nib(s[2 * i]) << 4 | nib(s[2 * i + 1]));
    return o;
}
static uint8_t* heap_block(size_t n) {
    uint8_t* p = (uint8_t*)malloc(n ? n : 1);
    if (!p) abort();
    return p;
}

static int run_decode() {
    std::string line;
    while (std::getline(std::cin, line)) {
        std::istringstream in(line);
        unsigned shift; std::string s[5], cd_h;
        if (!(in >> shift >> s[0] >> s[1] >> s[2] >> s[3] >> s[4] >> cd_h)) continue;
        uint32_t sel[4];
        for (int k = 0; k < 4; k++) sel[k] = (uint32_t)strtoul(s[k].c_str(), nullptr, 16);
        const uint32_t set_sel = (uint32_t)strtoul(s[4].c_str(), nullptr, 16);
        const std::vector<uint8_t> v = unhex(cd_h);
        const size_t len = v.size();
        if (shift > 3) return 2;
        uint8_t* blk = heap_block(len + shift);                        // malloc blocks are 16-byte aligned: the call ends with the block
        if (len) memcpy(blk + shift, v.data(), len);
        const uint8_t* cd = blk + shift;
        const bool al = (((uintptr_t)cd) & 3u) == 0;
        const RzwCall h = rzw_parse(cd, len, al, sel);
        bool ok = h.ok != 0;
        uint32_t kept = 0;
        uint8_t* seal = nullptr;
        if (ok && h.form == GWW_FORM_UINT8_ARRAY) {
            const uint8_t* el = cd + h.seal_at;
            uint32_t first4 = 0;
            if (h.seal_len >= 4) first4 = ((uint32_t)el[31] << 24) | ((uint32_t)el[63] << 16) | ((uint32_t)el[95] << 8) | el[127];
            kept = rzsw_keep(h.seal_len, first4, set_sel);
            seal = heap_block(kept);
            for (uint32_t k = 0; k < h.seal_len; k++) {                // the check never stops, the copy does
                for (int b = 0; b < 31; b++) if (el[32 * (size_t)k + b]) ok = false;
                if (k < kept) seal[k] = el[32 * (size_t)k + 31];
            }
        } else if (ok) {
            kept = h.seal_len;
            seal = heap_block(kept);
            if (kept) memcpy(seal, cd + h.seal_at, kept);
            for (uint32_t q = 0; q < (uint32_t)(-h.seal_len & 31u); q++) if (cd[h.seal_at + h.seal_len + q]) ok = false;
        }
        RzsSeal r = {RZS_NOT_SET, 0, 0, 0};
        // (a kept prefix of a longer seal has another selector: rzs_parse returns before it looks at the length)
        if (ok) r = rzs_parse(seal, kept, (((uintptr_t)seal) & 3u) == 0, set_sel);
        printf("%u %u %u %u %u %u %u %u %llu ", ok ? 1u : 0u, ok ? h.form : 0u, ok ? h.method : 0u, ok ? h.seal_len : 0u, ok ? kept : 0u, r.kind, r.depth,
               r.root_len, (unsigned long long)r.root_at);
        const uint32_t m = ok ? (kept < 260u ? kept : 260u) : 0u;
        if (!m) printf("-");
        for (uint32_t k = 0; k < m; k++) printf("%02x", seal[k]);
        printf("\n");
        free(seal); free(blk);
    }
    return 0;
}

static int run_arena(uint64_t offsets, uint64_t lengths) {
    unsigned long long checks = 0;
    uint64_t prev = 0;
    for (uint64_t o0 = 0; o0 < offsets; o0++) {
        const uint64_t at = rzsw_arena_at(o0);
        if (at & 3u) return 3;
        if (at < prev) return 4;                                       // monotone: a later request is never placed in front of an earlier one
        prev = at;
        for (uint64_t head = 100; head <= 132; head += 32)
            for (uint64_t L = 0; L < lengths; L++) {
                const uint64_t o1 = o0 + head + 32 * L;
                if (at + L > o1 / 32) return 5;                        // room: ends at or below floor(o1 / 32) <= calldata_bytes / 32
                if (at + L > rzsw_arena_bytes(o1)) return 6;
                if (rzsw_arena_at(o1) < at + L) return 7;              // disjoint from whatever begins at or behind o1 (monotone)
                checks += 3;
            }
    }
    printf("ok %llu\n", checks);
    return 0;
}

static int run_method() {
    std::string line;
    while (std::getline(std::cin, line)) {
        std::istringstream in(line);
        std::string m_h; unsigned have_b; size_t i;
        if (!(in >> m_h >> have_b >> i)) continue;
        const std::vector<uint8_t> mv = unhex(m_h);
        if (!mv.empty() && i >= mv.size()) return 2;
        uint8_t* row = mv.empty() ? nullptr : heap_block(mv.size());
        if (row) memcpy(row, mv.data(), mv.size());
        printf("%u\n", rzs_claim_given(row, have_b != 0, i) ? 1u : 0u);
        free(row);
    }
    return 0;
}

int main(int argc, char** argv) {
    if (argc == 2 && !strcmp(argv[1], "decode")) return run_decode();
    if (argc == 4 && !strcmp(argv[1], "arena")) return run_arena(strtoull(argv[2], nullptr, 10), strtoull(argv[3], nullptr, 10));
    if (argc == 2 && !strcmp(argv[1], "method")) return run_method();
    return 1;
}

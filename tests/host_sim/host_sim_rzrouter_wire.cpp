// Host build of what the RISC Zero router's calldata path adds to the kernels, for tests/test_risc0_router_wire_host.py.  Stand-alone:
// built and run once plain and once under AddressSanitizer and UndefinedBehaviorSanitizer.  Every input is a heap block of exactly its
// length, so a read outside a call, an input row or a method row is a sanitizer error.  TEST ONLY.
//
//   parse   the header arithmetic k_wire_rzrouter runs on every request (stylus_zkvm_verifiers_amd/csrc/zkv_wire_rzrouter.h rzw_parse):
//           stdin lines "shift sel0 sel1 sel2 sel3 (8 hex each, by call kind) calldata(hex or -)" ->
//           "ok form method seal_len a_at seal_at".  The call is parsed from a private copy of exactly its length placed `shift` bytes
//           past a 16-byte boundary; shift 0 takes the aligned word loads.
//   slot    the per-slot method choice of the keyed group's PREP body (zkv_rzrouter_prep.h rzrouter_slot_in_b in front of
//           rzrouter_prep_slot): stdin lines "kinds(hex, one byte per slot, or -) slot vk_valid len control_root control_id
//           in_a rows(hex, 32 bytes per slot) in_b rows(hex or -) record(520 hex)" -> test_rzrouter_prep.cpp's prep line.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>
#include "../../stylus_zkvm_verifiers_amd/csrc/zkv_wire_rzrouter.h"
#include "../../stylus_zkvm_verifiers_amd/csrc/zkv_rzrouter_prep.h"
#include "../../stylus_zkvm_verifiers_amd/csrc/zkv_host_vk.h"

using namespace zkv;

static std::vector<uint8_t> unhex(const std::string& s) {
    std::vector<uint8_t> o;
    if (s == "-") return o;
    for (size_t i = 0; i + 1 < s.size(); i += 2) o.push_back((uint8_t)strtoul(s.substr(i, 2).c_str(), nullptr, 16));
    return o;
}
static uint8_t* heap_copy(const std::vector<uint8_t>& v) {           // exactly v.size() bytes (one for an empty vector)
    uint8_t* p = (uint8_t*)malloc(v.empty() ? 1 : v.size());
    if (!p) abort();
    if (!v.empty()) memcpy(p, v.data(), v.size());
    return p;
}

static int run_parse() {
    std::string line;
    while (std::getline(std::cin, line)) {
        std::istringstream in(line);
        unsigned shift; std::string s[4], cd_h;
        if (!(in >> shift >> s[0] >> s[1] >> s[2] >> s[3] >> cd_h)) continue;
        uint32_t sel[4];
        for (int k = 0; k < 4; k++) sel[k] = (uint32_t)strtoul(s[k].c_str(), nullptr, 16);
        const std::vector<uint8_t> cd = unhex(cd_h);
        const size_t len = cd.size();
        if (shift > 3) return 2;
        uint8_t* blk = (uint8_t*)malloc(len + shift ? len + shift : 1);  // malloc blocks are 16-byte aligned: the call ends with the block
        if (!blk) abort();
        uint8_t* exact = (uint8_t*)malloc(len ? len : 1);              // a second copy, read byte by byte whatever its address
        if (!exact) abort();
        if (len) { memcpy(blk + shift, cd.data(), len); memcpy(exact, cd.data(), len); }
        const RzwCall a = rzw_parse(blk + shift, len, (((uintptr_t)(blk + shift)) & 3u) == 0, sel);
        const RzwCall b = rzw_parse(exact, len, false, sel);           // byte loads from a block of exactly the call
        if (a.ok != b.ok || a.form != b.form || a.method != b.method || a.seal_len != b.seal_len || a.a_at != b.a_at || a.seal_at != b.seal_at) return 3;
        printf("%u %u %u %u %u %llu\n", a.ok, a.form, a.method, a.seal_len, a.a_at, (unsigned long long)a.seal_at);
        free(blk); free(exact);
    }
    return 0;
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

static int run_slot() {
    Risc0Consts kc;
    host::risc0_consts(kc);
    std::string line;
    while (std::getline(std::cin, line)) {
        std::istringstream in(line);
        unsigned slot, vk_valid, len; std::string kind_h, root_h, id_h, a_h, b_h, rec_h;
        if (!(in >> kind_h >> slot >> vk_valid >> len >> root_h >> id_h >> a_h >> b_h >> rec_h)) continue;
        const std::vector<uint8_t> kinds = unhex(kind_h), root = unhex(root_h), id = unhex(id_h), ia = unhex(a_h), ib = unhex(b_h), rec = unhex(rec_h);
        if (root.size() != 32 || id.size() != 32 || ia.size() < 32 * (slot + 1) || (!ib.empty() && ib.size() != ia.size()) ||
            (!kinds.empty() && 32 * kinds.size() != ia.size()) || rec.size() != 260) return 2;
        const RzrRoute rt = route_of(root.data(), id.data());
        uint8_t *k0 = kinds.empty() ? nullptr : heap_copy(kinds), *a0 = heap_copy(ia), *b0 = ib.empty() ? nullptr : heap_copy(ib), *r0 = heap_copy(rec);
        RzrSlot r;
        GwsetRec rd = {nullptr, r0};
        rzrouter_prep_slot(vk_valid, rt, kc, len, a0 + 32 * slot, rzrouter_slot_in_b(k0, b0, slot), rd, r);
        const bool alive = (r.flags & FL_ALIVE) != 0;
        printf("%u %u", (unsigned)r.status, r.flags);
        for (int s = 0; s < 5; s++) { printf(" "); put_limbs(r.sig[s]); }
        const Fp z = fp_zero();
        put_fp(alive ? r.o.ax : z); put_fp(alive ? r.o.ay : z);
        put_fp(alive ? r.o.bx.c0 : z); put_fp(alive ? r.o.bx.c1 : z); put_fp(alive ? r.o.by.c0 : z); put_fp(alive ? r.o.by.c1 : z);
        put_fp(alive ? r.o.cx : z); put_fp(alive ? r.o.cy : z);
        printf("\n");
        free(k0); free(a0); free(b0); free(r0);
    }
    return 0;
}

int main(int argc, char** argv) {
    if (argc == 2 && !strcmp(argv[1], "parse")) return run_parse();
    if (argc == 2 && !strcmp(argv[1], "slot")) return run_slot();
    return 1;
}

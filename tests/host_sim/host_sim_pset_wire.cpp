// Host build of the functions k_pset_wire_decode and k_pset_wire_points run on every eth_call request to a set of deployed gnark PLONK
// verifier contracts (stylus_zkvm_verifiers_amd/csrc/zkv_wire_pset.h): offsets, the address search, the canonical head, the length
// rules, the copy into the set's ordinary inputs with the tests "an input word >= r" and "an opening word >= r", and the curve test of
// the copied proof's points -- a request start to end (psw_request) and the kernel's wavefront form.  TEST ONLY.
//
// With -DHSPSW_MAIN the file is a stand-alone program (for a sanitizer build: g++ -fsanitize=address,undefined -DHSPSW_MAIN) that decodes
// a few requests of its own making, at every alignment, from exact-size allocations.
#include <stdint.h>
#include <string.h>
#include <stdlib.h>
#include <stdio.h>
#include "../../stylus_zkvm_verifiers_amd/csrc/zkv_wire_pset.h"
using namespace zkv;

// One wavefront of k_pset_wire_decode, its lanes one after the other: every lane resolves its request, then the calls of the wavefront
// are copied one by one, lane by lane, and the two ballots of a step are built from the lanes' answers.
static void wave(const PswArgs& a, size_t i0) {
    PswCall c[64];
    uint32_t in_ge[64] = {0}, op_ge[64] = {0};
    uint64_t calls = 0;
    const uint32_t row_dwords = a.proof_stride / 4;
    for (uint32_t lane = 0; lane < 64; lane++) {
        c[lane] = PswCall{PSW_BAD_CALLDATA, PSW_NONE, 0, 0, 0, 0, 0};
        if (i0 + lane < a.n) c[lane] = psw_resolve(a, i0 + lane);
        if (i0 + lane < a.n && c[lane].verdict == PSW_CALL && c[lane].pre != PSW_R_INPUT_COUNT) calls |= 1ull << lane;
    }
    for (uint32_t j = 0; j < 64; j++) {
        if (!((calls >> j) & 1)) continue;
        const bool store = c[j].pre == PSW_R_NONE;
        const uint8_t* cd = a.cd + c[j].at;
        const bool al = (((uintptr_t)cd) & 3u) == 0;
        const uint8_t* src = cd + PSW_HEAD + psw_pad32(c[j].lp) + 32;
        uint32_t* row = (uint32_t*)(a.rows + (size_t)a.input_stride * (i0 + j));
        const uint32_t n_dwords = 8 * c[j].nb;
        bool ge = false;
        for (uint32_t w0 = 0; w0 < n_dwords; w0 += 64) {
            uint64_t gt = 0, lt = 0;
            for (uint32_t lane = 0; lane < 64; lane++) {
                const uint32_t cls = psw_input_dword(src, al, row, store, w0 + lane, n_dwords);
                gt |= (uint64_t)(cls == 2) << lane; lt |= (uint64_t)(cls == 1) << lane;
            }
            ge = gsw_any_ge_r(gt, lt) || ge;
        }
        in_ge[j] = ge ? 1 : 0;
        if (!store) continue;
        uint32_t* proof = (uint32_t*)(a.proofs + (size_t)a.proof_stride * (i0 + j));
        ge = false;
        for (uint32_t w0 = 0; w0 < row_dwords; w0 += 64) {
            uint64_t gt = 0, lt = 0;
            for (uint32_t lane = 0; lane < 64; lane++) {
                const uint32_t cls = psw_proof_dword(cd + PSW_HEAD, al, proof, w0 + lane, c[j].n_c, row_dwords);
                gt |= (uint64_t)(cls == 2) << lane; lt |= (uint64_t)(cls == 1) << lane;
            }
            if (w0 >= 64) ge = gsw_any_ge_r(gt, lt) || ge;
        }
        op_ge[j] = ge ? 1 : 0;
    }
    for (uint32_t lane = 0; lane < 64 && i0 + lane < a.n; lane++) psw_finish(a, i0 + lane, c[lane], psw_reason(c[lane], in_ge[lane] != 0, op_ge[lane] != 0));
}

// The batch is decoded from private copies of exactly the given sizes -- the blob `shift` (0 .. 3) bytes into its allocation and ending
// where the allocation ends, so that the calldata words sit at every alignment and a read past the blob is a read outside the
// allocation.  tab: n_tab rows of eight words
// (PswEntry).  Outputs as PswArgs: key and rkey (n words each), proofs (n x proof_stride), rows (n x input_stride), verdict, reason, npt
// and ec (n bytes each).  form 0: psw_request per request (the plain form); form 1: the wavefront form, 64 requests at a time.  Either
// way the point test follows, one (request, point) after the other.
extern "C" int hspsw_decode(uint64_t n, const uint8_t* to, const uint8_t* cd, uint64_t cd_bytes, const uint64_t* off, uint32_t shift, const uint32_t* tab,
                            uint32_t n_tab, uint32_t sel_be, uint32_t proof_stride, uint32_t input_stride, uint32_t* key, uint32_t* rkey, uint8_t* proofs,
                            uint8_t* rows, uint8_t* verdict, uint8_t* reason, uint8_t* npt, uint8_t* ec, int form) {
    if (shift > 3) return -1;
    uint8_t* blob = (uint8_t*)malloc((size_t)(cd_bytes + shift) + (cd_bytes + shift ? 0 : 1));     // (malloc aligns to 8 at the least)
    uint8_t* to_copy = (uint8_t*)malloc((size_t)(20 * n + 1));
    PswEntry* t = (PswEntry*)malloc(sizeof(PswEntry) * (n_tab + 1));
    if (!blob || !to_copy || !t) { free(blob); free(to_copy); free(t); return -1; }
    static_assert(sizeof(PswEntry) == 32, "a table row is eight words");
    uint8_t* at = blob + shift;
    memcpy(t, tab, sizeof(PswEntry) * n_tab);
    if (cd_bytes) memcpy(at, cd, (size_t)cd_bytes);
    memcpy(to_copy, to, (size_t)(20 * n));
    PswArgs a;
    memset(&a, 0, sizeof a);
    a.n = (size_t)n; a.to = to_copy; a.cd = at; a.off = off; a.cd_bytes = cd_bytes; a.tab = t; a.n_tab = n_tab; a.sel_be = sel_be;
    a.key = key; a.rkey = rkey; a.proofs = proofs; a.proof_stride = proof_stride; a.rows = rows; a.input_stride = input_stride;
    a.verdict = verdict; a.reason = reason; a.npt = npt; a.ec = ec;
    if (form) for (size_t i0 = 0; i0 < a.n; i0 += 64) wave(a, i0);
    else for (size_t i = 0; i < a.n; i++) psw_request(a, i);
    for (size_t i = 0; i < a.n; i++) for (uint32_t p = 0; p < PSW_MAX_POINTS; p++) psw_point(a, i, p);
    free(blob); free(to_copy); free(t);
    return 0;
}

#ifdef HSPSW_MAIN
static void put_word(uint8_t* p, uint64_t v) { memset(p, 0, 32); for (int k = 0; k < 8; k++) p[31 - k] = (uint8_t)(v >> (8 * k)); }
int main() {
    // two contracts (nb = 2, n_c = 0 and nb = 0, n_c = 1); every proof word is small, so every point is off the curve unless it is (0, 0)
    static const uint8_t r_be[32] = {0x30, 0x64, 0x4e, 0x72, 0xe1, 0x31, 0xa0, 0x29, 0xb8, 0x50, 0x45, 0xb6, 0x81, 0x81, 0x58, 0x5d,
                                     0x28, 0x33, 0xe8, 0x48, 0x79, 0xb9, 0x70, 0x91, 0x43, 0xe1, 0xf5, 0x93, 0xf0, 0x00, 0x00, 0x01};
    const uint32_t SEL = 0x7e4f7a8au;
    const uint32_t tab[2][8] = {{1, 2, 3, 4, 5, 1, 2, 0}, {9, 2, 3, 4, 5, 0, 0, 1}};
    uint8_t addr[3][20] = {{0}};
    for (int q = 0; q < 3; q++) for (int k = 0; k < 5; k++) addr[q][4 * k + 3] = (uint8_t)(k + 1);
    addr[1][3] = 9; addr[2][3] = 7;
    static uint8_t blob[16384];
    uint64_t off[12]; uint8_t to[11 * 20]; size_t at = 0; int q = 0;
    // a call of lp proof bytes (all zero: every point is infinity) and n_in input words (zero)
    auto put = [&](const uint8_t* a20, size_t lp, size_t n_in, size_t extra) -> uint8_t* {
        memcpy(to + 20 * q, a20, 20); off[q++] = at;
        uint8_t* p = blob + at;
        const size_t span = (lp + 31) / 32 * 32;
        p[0] = (uint8_t)(SEL >> 24); p[1] = (uint8_t)(SEL >> 16); p[2] = (uint8_t)(SEL >> 8); p[3] = (uint8_t)SEL;
        put_word(p + 4, 0x40); put_word(p + 36, 0x60 + span); put_word(p + 68, lp);
        memset(p + 100, 0, span); put_word(p + 100 + span, n_in); memset(p + 132 + span, 0, 32 * n_in);
        at += 132 + span + 32 * n_in + extra;
        return p;
    };
    put(addr[0], 768, 2, 0);                                         // 0: placed (the verifier would answer 0)
    put(addr[1], 864, 0, 0);                                         // 1: placed
    uint8_t* p2 = put(addr[0], 768, 2, 0); memcpy(p2 + 132 + 768 + 32, r_be, 32);          // 2: second input = r
    uint8_t* p3 = put(addr[0], 768, 2, 0); memcpy(p3 + 100 + 32 * 19, r_be, 32);           // 3: opening 19 = r
    uint8_t* p4 = put(addr[1], 864, 0, 0); p4[100 + 32 * 25 + 31] = 1;                     // 4: the commitment (1, 0) is off the curve
    put(addr[0], 768, 3, 0);                                         // 5: count
    put(addr[0], 864, 2, 0);                                         // 6: proof size
    put(addr[1], 864, 0, 1);                                         // 7: a trailing byte
    put(addr[2], 864, 0, 0);                                         // 8: no contract
    const uint64_t total = at;
    memcpy(to + 20 * q, addr[0], 20); off[q++] = total; memcpy(to + 20 * q, addr[0], 20); off[q++] = total + 100; off[q] = total;
    const uint32_t N = PSW_NONE;
    const uint32_t want_key[11] = {1, 0, N, N, N, N, N, N, N, N, N}, want_rkey[11] = {1, 0, 1, 1, 0, 1, 1, 0, N, N, N};
    const uint8_t want_v[11] = {0, 0, 0, 0, 0, 0, 0, 6, 9, 6, 6}, want_r[11] = {0, 0, 2, 4, 0, 1, 3, 0, 0, 0, 0}, want_ec[11] = {0, 0, 0, 0, 1, 0, 0, 0, 0, 0, 0};
    int bad = 0;
    for (uint32_t run = 0; run < 8; run++) {
        const uint32_t shift = run & 3;
        uint32_t key[11], rkey[11]; uint8_t v[11], rs[11], npt[11], ec[11];
        uint8_t* proofs = (uint8_t*)malloc(11 * 864); uint8_t* rows = (uint8_t*)malloc(11 * 64);
        memset(proofs, 0xEE, 11 * 864); memset(rows, 0xEE, 11 * 64);
        if (hspsw_decode(11, to, blob, total, off, shift, &tab[0][0], 2, SEL, 864, 64, key, rkey, proofs, rows, v, rs, npt, ec, run >> 2) != 0) return 2;
        for (int i = 0; i < 11; i++) bad += key[i] != want_key[i] || rkey[i] != want_rkey[i] || v[i] != want_v[i] || rs[i] != want_r[i] || ec[i] != want_ec[i];
        for (int k = 0; k < 864; k++) bad += proofs[k] != 0 || proofs[864 + k] != 0;     // a 768-byte proof: zeros behind it
        bad += memcmp(proofs + 3 * 864 + 32 * 19, r_be, 32) != 0 || memcmp(rows + 2 * 64 + 32, r_be, 32) != 0;
        bad += rows[64] != 0xEE || proofs[5 * 864] != 0xEE || proofs[6 * 864] != 0xEE || rows[6 * 64] != 0xEE || proofs[7 * 864] != 0xEE;
        free(proofs); free(rows);
    }
    printf(bad ? "FAILED %d\n" : "ok\n", bad);
    return bad ? 1 : 0;
}
#endif

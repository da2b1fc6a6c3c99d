// Host build of the functions k_gset_wire_decode runs on every eth_call request to a set of deployed Groth16 verifier contracts
// (stylus_zkvm_verifiers_amd/csrc/zkv_wire_gset.h): offsets, the address search, selector and length, the copy into the set's ordinary
// inputs and the test "a signal word >= r" -- a request start to end (gsw_request) and the kernel's wavefront form.  TEST ONLY.
//
// With -DHSGSW_MAIN the file is a stand-alone program (for a sanitizer build: g++ -fsanitize=address,undefined -DHSGSW_MAIN) that decodes a
// few requests of its own making, at every alignment, from exact-size allocations.
#include <stdint.h>
#include <string.h>
#include <stdlib.h>
#include <stdio.h>
#include "../../stylus_zkvm_verifiers_amd/csrc/zkv_wire_gset.h"
using namespace zkv;

// One wavefront of k_gset_wire_decode, its lanes one after the other: every lane resolves its request, then the calls of the wavefront
// are copied one by one, lane by lane, and the two ballots of a step are built from the lanes' answers.
static void wave(const GswArgs& a, size_t i0) {
    GswCall c[64];
    uint32_t big[64] = {0};
    uint64_t calls = 0;
    for (uint32_t lane = 0; lane < 64; lane++) {
        c[lane] = GswCall{GSW_BAD_CALLDATA, GSW_NONE, 0, 0};
        if (i0 + lane < a.n) c[lane] = gsw_resolve(a, i0 + lane);
        if (i0 + lane < a.n && c[lane].verdict == GSW_CALL) calls |= 1ull << lane;
    }
    for (uint32_t j = 0; j < 64; j++) {
        if (!((calls >> j) & 1)) continue;
        const uint32_t n_dwords = 8 * c[j].n_sig;
        const uint8_t* src = a.cd + c[j].at + 4;
        const bool al = (((uintptr_t)src) & 3u) == 0;
        uint32_t* row = (uint32_t*)(a.rows + (size_t)a.sig_stride * (i0 + j));
        for (uint32_t lane = 0; lane < 64; lane++) ((uint32_t*)(a.proofs + 256 * (i0 + j)))[lane] = gsw_ld4(src + 4 * lane, al);
        bool ge = false;
        for (uint32_t w0 = 0; w0 < n_dwords; w0 += 64) {
            uint64_t gt = 0, lt = 0;
            for (uint32_t lane = 0; lane < 64; lane++) {
                const uint32_t cls = gsw_signal_dword(src + 256, al, row, w0 + lane, n_dwords);
                gt |= (uint64_t)(cls == 2) << lane; lt |= (uint64_t)(cls == 1) << lane;
            }
            ge = gsw_any_ge_r(gt, lt) || ge;
        }
        big[j] = ge ? 1 : 0;
    }
    for (uint32_t lane = 0; lane < 64 && i0 + lane < a.n; lane++) gsw_finish(a, i0 + lane, c[lane], big[lane]);
}

// The batch is decoded from private copies of exactly the given sizes -- the blob `shift` bytes past a 16-byte boundary, so that the
// calldata words sit at every alignment and a read outside the blob is a read outside the allocation.  tab: n_tab rows of eight words
// (GswEntry).  Outputs as GswArgs: key and rkey (n words each), proofs (n x 256), rows (n x sig_stride), verdict and ge_r (n bytes each).
// form 0: gsw_request per request (the plain form); form 1: the wavefront form, 64 requests at a time.
extern "C" int hsgsw_decode(uint64_t n, const uint8_t* to, const uint8_t* cd, uint64_t cd_bytes, const uint64_t* off, uint32_t shift, const uint32_t* tab,
                            uint32_t n_tab, uint32_t sig_stride, uint32_t* key, uint32_t* rkey, uint8_t* proofs, uint8_t* rows, uint8_t* verdict, uint8_t* ge_r,
                            int form) {
    uint8_t* raw = (uint8_t*)aligned_alloc(16, (size_t)((cd_bytes + shift + 15) / 16 * 16 + 16));
    uint8_t* to_copy = (uint8_t*)malloc((size_t)(20 * n + 1));
    GswEntry* t = (GswEntry*)malloc(sizeof(GswEntry) * (n_tab + 1));
    if (!raw || !to_copy || !t) { free(raw); free(to_copy); free(t); return -1; }
    static_assert(sizeof(GswEntry) == 32, "a table row is eight words");
    memcpy(t, tab, sizeof(GswEntry) * n_tab);
    if (cd_bytes) memcpy(raw + shift, cd, (size_t)cd_bytes);
    memcpy(to_copy, to, (size_t)(20 * n));
    GswArgs a;
    memset(&a, 0, sizeof a);
    a.n = (size_t)n; a.to = to_copy; a.cd = raw + shift; a.off = off; a.cd_bytes = cd_bytes; a.tab = t; a.n_tab = n_tab;
    a.key = key; a.rkey = rkey; a.proofs = proofs; a.rows = rows; a.sig_stride = sig_stride; a.verdict = verdict; a.ge_r = ge_r;
    if (form) for (size_t i0 = 0; i0 < a.n; i0 += 64) wave(a, i0);
    else for (size_t i = 0; i < a.n; i++) gsw_request(a, i);
    free(raw); free(to_copy); free(t);
    return 0;
}

#ifdef HSGSW_MAIN
int main() {
    // two contracts (2 and 1 signals), requests: a call to each, one with a signal = r, a trailing byte, an unknown address, offsets
    // past the blob and backwards
    static const uint8_t r_be[32] = {0x30, 0x64, 0x4e, 0x72, 0xe1, 0x31, 0xa0, 0x29, 0xb8, 0x50, 0x45, 0xb6, 0x81, 0x81, 0x58, 0x5d,
                                     0x28, 0x33, 0xe8, 0x48, 0x79, 0xb9, 0x70, 0x91, 0x43, 0xe1, 0xf5, 0x93, 0xf0, 0x00, 0x00, 0x01};
    const uint32_t tab[2][8] = {{1, 2, 3, 4, 5, 1, 0xAABBCCDDu, 2}, {9, 2, 3, 4, 5, 0, 0x11223344u, 1}};
    uint8_t addr[3][20] = {{0}};
    for (int k = 0; k < 5; k++) { addr[0][4 * k + 3] = (uint8_t)(k + 1); addr[1][4 * k + 3] = (uint8_t)(k + 1); addr[2][4 * k + 3] = (uint8_t)(k + 1); }
    addr[1][3] = 9; addr[2][3] = 7;
    uint8_t blob[4096];
    for (size_t k = 0; k < sizeof blob; k++) blob[k] = (uint8_t)(k * 7 + 1) & 0x1F;     // every word far below r
    uint64_t off[8]; uint8_t to[7 * 20]; size_t at = 0; int q = 0;
    auto put = [&](const uint8_t* a20, uint32_t sel, size_t words, size_t extra) {
        memcpy(to + 20 * q, a20, 20); off[q++] = at;
        blob[at] = (uint8_t)(sel >> 24); blob[at + 1] = (uint8_t)(sel >> 16); blob[at + 2] = (uint8_t)(sel >> 8); blob[at + 3] = (uint8_t)sel;
        at += 4 + 32 * words + extra;
    };
    put(addr[0], 0xAABBCCDDu, 10, 0); put(addr[1], 0x11223344u, 9, 0);
    put(addr[0], 0xAABBCCDDu, 10, 0); memcpy(blob + off[2] + 4 + 32 * 9, r_be, 32);
    put(addr[1], 0x11223344u, 9, 1); put(addr[2], 0x11223344u, 9, 0);
    const uint64_t total = at;
    memcpy(to + 20 * q, addr[0], 20); off[q++] = total; memcpy(to + 20 * q, addr[0], 20); off[q++] = total + 100; off[q] = total;
    const uint32_t want_key[7] = {1, 0, GSW_NONE, GSW_NONE, GSW_NONE, GSW_NONE, GSW_NONE}, want_rkey[7] = {1, 0, 1, 0, GSW_NONE, GSW_NONE, GSW_NONE};
    const uint8_t want_v[7] = {0, 0, 0, 6, 9, 6, 6}, want_big[7] = {0, 0, 1, 0, 0, 0, 0};
    int bad = 0;
    for (uint32_t run = 0; run < 8; run++) {
        const uint32_t shift = run & 3;
        uint32_t key[7], rkey[7]; uint8_t v[7], big[7];
        uint8_t* proofs = (uint8_t*)aligned_alloc(16, 7 * 256); uint8_t* rows = (uint8_t*)aligned_alloc(16, 7 * 64);
        memset(proofs, 0xEE, 7 * 256); memset(rows, 0xEE, 7 * 64);
        if (hsgsw_decode(7, to, blob, total, off, shift, &tab[0][0], 2, 64, key, rkey, proofs, rows, v, big, run >> 2) != 0) return 2;
        for (int i = 0; i < 7; i++) bad += key[i] != want_key[i] || rkey[i] != want_rkey[i] || v[i] != want_v[i] || big[i] != want_big[i];
        bad += memcmp(proofs, blob + 4, 256) != 0 || memcmp(rows, blob + 260, 64) != 0 || memcmp(rows + 64, blob + off[1] + 260, 32) != 0;
        bad += rows[64 + 32] != 0xEE || proofs[3 * 256] != 0xEE;                          // nothing past a key's signals, nothing for a bad request
        free(proofs); free(rows);
    }
    printf(bad ? "FAILED %d\n" : "ok\n", bad);
    return bad ? 1 : 0;
}
#endif

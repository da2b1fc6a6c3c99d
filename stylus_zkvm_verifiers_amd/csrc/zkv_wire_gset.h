// Decode rule of one `verifyProof` eth_call to a deployed Groth16 verifier contract (include/zkv_groth16_set_wire.h), shared by
// k_gset_wire_decode (k_gset_wire.hip) and the host (tests/host_sim/host_sim_gset_wire.cpp).  Both contract forms have one body:
//   sel | 8 proof words (A.x A.y B.x1 B.x0 B.y1 B.y0 C.x C.y, the precompiles' order) | N signal words          4 + 32 (8 + N) bytes
// so a request is decoded by its length and its selector alone, and its words are moved, never interpreted -- except for the one test
// both contracts make before anything else: a signal word >= r.  Parity unpinned: the reference holds no generic contract shell.
#pragma once
#include <stdint.h>
#include <stddef.h>
#include "zkv_sha256.h"

namespace zkv {

constexpr uint32_t GSW_NONE = 0xFFFFFFFFu;               // no key (GswArgs::key, rkey); GswEntry::n_sig: the key has no callable method
// decode verdicts: 0 = the request is a canonical call of its contract, else the status it is answered with
constexpr uint32_t GSW_CALL = 0, GSW_BAD_CALLDATA = 6 /* ZKV_STATUS_BAD_CALLDATA */, GSW_NO_CONTRACT = 9 /* ZKV_STATUS_NO_CONTRACT */;

// One deployed contract; the table is ascending by address (the 20 bytes as five big-endian words, addr[0] first).
struct GswEntry { uint32_t addr[5]; uint32_t key, sel_be, n_sig; };

ZKV_HD int gsw_addr_cmp(const uint32_t a[5], const uint32_t b[5]) {
    for (int k = 0; k < 5; k++) if (a[k] != b[k]) return a[k] < b[k] ? -1 : 1;
    return 0;
}
// Index of the entry with address `to` (20 bytes, any alignment) among tab[0 .. n), GSW_NONE when there is none.  Entry: GswEntry, or
// the entry of another kind of deployed set (zkv_wire_pset.h) -- anything with addr[5].
template <class Entry>
ZKV_HD uint32_t gsw_find(const Entry* tab, uint32_t n, const uint8_t* to) {
    uint32_t a[5];
    for (int k = 0; k < 5; k++) a[k] = load_be32(to + 4 * k);
    uint32_t lo = 0, hi = n;                              // the entry, if any, is in [lo, hi)
    while (lo < hi) {
        const uint32_t mid = lo + (hi - lo) / 2;
        const int c = gsw_addr_cmp(tab[mid].addr, a);
        if (c == 0) return mid;
        if (c < 0) lo = mid + 1; else hi = mid;
    }
    return GSW_NONE;
}
// w: one 32-byte word as eight big-endian dwords, w[0] the most significant.  True when it is >= r, the BN254 group order.
ZKV_HD bool gsw_ge_r(const uint32_t w[8]) {
    const uint32_t r[8] = {0x30644e72u, 0xe131a029u, 0xb85045b6u, 0x8181585du, 0x2833e848u, 0x79b97091u, 0x43e1f593u, 0xf0000001u};
    for (int k = 0; k < 8; k++) if (w[k] != r[k]) return w[k] > r[k];
    return true;
}
// Four bytes in memory order as one little-endian dword; `al`: p is 4-byte aligned.
ZKV_HD uint32_t gsw_ld4(const uint8_t* p, bool al) {
    if (al) return *(const uint32_t*)p;
    return (uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16) | ((uint32_t)p[3] << 24);
}

// A batch of requests.  Request i is cd[off[i] .. off[i + 1]) to the contract at to[20 i ..]; every output row is the library's own
// (4-byte aligned): key / proofs / rows are the inputs of zkv_groth16_set_verify_batch_dev.
struct GswArgs {
    size_t n;
    const uint8_t* to; const uint8_t* cd; const uint64_t* off; uint64_t cd_bytes;
    const GswEntry* tab; uint32_t n_tab;
    uint32_t* key;                                        // n: the key of a request that is to be placed, else GSW_NONE
    uint32_t* rkey;                                       // n: the key its address resolved to, GSW_NONE without a lookup or a contract
    uint8_t* proofs;                                      // n x 256
    uint8_t* rows; uint32_t sig_stride;                   // n x sig_stride: the first N words of row i are written
    uint8_t* verdict;                                     // n: GSW_CALL / GSW_BAD_CALLDATA / GSW_NO_CONTRACT
    uint8_t* ge_r;                                        // n: 1 = a canonical call with a signal word >= r (not placed)
};

// What the header of request i says.  at: where the request starts in cd (calls only).
struct GswCall { uint32_t verdict, rkey, n_sig; uint64_t at; };

// The rules, in order: offsets that run backwards or leave the blob (the request is never read); an address without a contract;
// anything but the contract's selector in front of exactly 32 (8 + N) bytes, and every request to a key without signals (uint256[0] is
// no type: such a contract has no method).  Every read of the request lies in [off[i], off[i + 1]): the selector is read only when the
// length is the one the key demands, which is at least 260.
ZKV_HD GswCall gsw_resolve(const GswArgs& a, size_t i) {
    const uint64_t o0 = a.off[i], o1 = a.off[i + 1];
    GswCall c = {GSW_BAD_CALLDATA, GSW_NONE, 0, 0};
    if (o0 <= o1 && o1 <= a.cd_bytes) {
        const uint32_t e = gsw_find(a.tab, a.n_tab, a.to + 20 * i);
        if (e == GSW_NONE) c.verdict = GSW_NO_CONTRACT;
        else {
            const GswEntry t = a.tab[e];
            c.rkey = t.key;
            if (t.n_sig != GSW_NONE && o1 - o0 == 4 + 32 * (8 + (uint64_t)t.n_sig) && load_be32(a.cd + o0) == t.sel_be) { c.verdict = GSW_CALL; c.n_sig = t.n_sig; c.at = o0; }
        }
    }
    return c;
}
// The rows of request i once its words are copied; big: a signal word of a call is >= r (the last rule: such a call is not placed).
ZKV_HD void gsw_finish(const GswArgs& a, size_t i, const GswCall& c, uint32_t big) {
    a.key[i] = c.verdict == GSW_CALL && !big ? c.rkey : GSW_NONE;
    a.rkey[i] = c.rkey;
    a.verdict[i] = (uint8_t)c.verdict;
    a.ge_r[i] = (uint8_t)big;
}
// Request i, start to end, by one thread: the plain form of the decode, which the wavefront form below must equal.
ZKV_HD void gsw_request(const GswArgs& a, size_t i) {
    const GswCall c = gsw_resolve(a, i);
    uint32_t big = 0;
    if (c.verdict == GSW_CALL) {
        const uint8_t* src = a.cd + c.at + 4;
        const bool al = (((uintptr_t)src) & 3u) == 0;
        uint32_t* proof = (uint32_t*)(a.proofs + 256 * i);
        uint32_t* row = (uint32_t*)(a.rows + (size_t)a.sig_stride * i);
        for (uint32_t k = 0; k < 64; k++) proof[k] = gsw_ld4(src + 4 * k, al);
        src += 256;
        for (uint32_t b = 0; b < c.n_sig; b++, src += 32) {
            uint32_t w[8];
            for (int k = 0; k < 8; k++) { const uint32_t v = gsw_ld4(src + 4 * k, al); row[8 * b + k] = v; w[k] = __builtin_bswap32(v); }
            big |= gsw_ge_r(w) ? 1u : 0u;
        }
    }
    gsw_finish(a, i, c, big);
}

// ---- The wavefront form (k_gset_wire_decode): every lane resolves its own request, then the 64 lanes copy the words of one call after
// the other together, a dword per lane, so that a wave instruction reads and writes 256 contiguous bytes.  Dword w of the signal words
// (w = 8 b + k: dword k of signal b, k = 0 the most significant) goes to lane w % 64, so eight neighbouring lanes hold one signal word.
// One lane's share of one step: copies dword w of the `n_dwords` signal dwords at `sig` and compares it with r's dword of the same
// significance.  -> 0 equal, 1 less (also: no such dword), 2 greater.
ZKV_HD uint32_t gsw_signal_dword(const uint8_t* sig, bool al, uint32_t* row, uint32_t w, uint32_t n_dwords) {
    if (w >= n_dwords) return 1;
    const uint32_t k = w & 7u;                            // (selects, not an indexed array: a lane keeps its k through every step)
    const uint32_t rk = k == 0 ? 0x30644e72u : k == 1 ? 0xe131a029u : k == 2 ? 0xb85045b6u : k == 3 ? 0x8181585du : k == 4 ? 0x2833e848u
                      : k == 5 ? 0x79b97091u : k == 6 ? 0x43e1f593u : 0xf0000001u;
    const uint32_t v = gsw_ld4(sig + 4 * (size_t)w, al), be = __builtin_bswap32(v);
    row[w] = v;
    return be == rk ? 0u : be < rk ? 1u : 2u;
}
// The lanes' answers of one step as two masks (bit = lane): true when one of the eight words in flight is >= r -- its first dword that
// differs from r's is greater, or none differs.
ZKV_HD bool gsw_any_ge_r(uint64_t gt, uint64_t lt) {
    for (int g = 0; g < 8; g++) {
        const uint32_t g8 = (uint32_t)(gt >> (8 * g)) & 0xFFu, l8 = (uint32_t)(lt >> (8 * g)) & 0xFFu, u = g8 | l8;
        if (!u || (g8 & (u & (0u - u)))) return true;
    }
    return false;
}

}  // namespace zkv

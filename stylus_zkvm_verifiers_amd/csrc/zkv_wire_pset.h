// Rules of one `Verify(bytes proof, uint256[] public_inputs)` eth_call to a deployed gnark PLONK verifier contract
// (include/zkv_plonk_set_wire.h), shared by k_pset_wire_decode / k_pset_wire_points (k_pset_wire.hip) and the host
// (tests/host_sim/host_sim_pset_wire.cpp).  The one accepted layout, every argument dynamic:
//   sel | 0x40 | 0x60 + pad32(Lp) | Lp | proof, padded to 32 | N' | N' words                  4 + 96 + pad32(Lp) + 32 + 32 N' bytes
// A request is answered by the first rule that catches it: offsets, address, canonical ABI (the three: PSW_BAD_CALLDATA / PSW_NO_CONTRACT),
// then the contract's own checks in gnark's order -- N' against the key's nb (reason 1), an input word >= r (2), Lp against the key's
// Lkey = 32 (24 + 3 n_c) (3), an opening word >= r (4) -- and the EC precompiles on the proof's points (5).  Parity unpinned: the
// reference holds no PLONK code and no contract shell.
#pragma once
#include <stdint.h>
#include <stddef.h>
#include "zkv_plonk.h"           // plonk_g1: a G1 point as the precompiles take it
#include "zkv_wire_gateway.h"    // gww_word: an ABI word as its low 64 bits and "one of the upper 24 bytes is set"
#include "zkv_wire_gset.h"       // gsw_find, gsw_ld4, gsw_ge_r, gsw_any_ge_r

namespace zkv {

constexpr uint32_t PSW_NONE = 0xFFFFFFFFu;               // no key (PswArgs::key, rkey)
// decode verdicts: 0 = the request is a canonical call of its contract, else the status it is answered with
constexpr uint32_t PSW_CALL = 0, PSW_BAD_CALLDATA = 6 /* ZKV_STATUS_BAD_CALLDATA */, PSW_NO_CONTRACT = 9 /* ZKV_STATUS_NO_CONTRACT */;
// reasons (ZKV_PLONK_REVERT_*)
constexpr uint32_t PSW_R_NONE = 0, PSW_R_INPUT_COUNT = 1, PSW_R_INPUT_RANGE = 2, PSW_R_PROOF_SIZE = 3, PSW_R_OPENING_RANGE = 4, PSW_R_EC = 5;
constexpr uint64_t PSW_HEAD = 4 + 96;                    // selector, the two offset words, the proof's length word
constexpr uint32_t PSW_MAX_POINTS = 10;                  // L R O H0 H1 H2 Z H_zeta H_zeta_omega, and the BSB22 commitment when n_c = 1

// One deployed contract; the table is ascending by address (the 20 bytes as five big-endian words, addr[0] first).
struct PswEntry { uint32_t addr[5]; uint32_t key, nb, n_c; };

static_assert(PSW_NONE == GSW_NONE, "gsw_find answers GSW_NONE");

// The head of one call.  ok = 0: not the canonical encoding (the other fields are 0).  lp, n_in: the two lengths, both below 2^32.
struct PswHead { uint32_t ok, lp, n_in; };
ZKV_HD uint64_t psw_pad32(uint64_t len32) { return (len32 + 31) & ~(uint64_t)31; }      // len32 < 2^32: no 64-bit overflow
// cd: the `len` bytes of one call (every read stays inside them); al: cd is 4-byte aligned; sel_be: Verify's selector as a big-endian word.
ZKV_HD PswHead psw_parse(const uint8_t* cd, uint64_t len, bool al, uint32_t sel_be) {
    PswHead r = {0, 0, 0};
    if (len < PSW_HEAD + 32) return r;                               // shortest call: both arguments empty
    if (load_be32(cd) != sel_be) return r;
    const GwWord o1 = gww_word(cd + 4, al), o2 = gww_word(cd + 36, al), lp = gww_word(cd + 68, al);
    if (!gww_fits32(o1) || o1.lo != 0x40 || !gww_fits32(lp)) return r;
    const uint64_t span = psw_pad32(lp.lo);                          // < 2^33
    if (o2.high || o2.lo != 0x60 + span) return r;
    if (len < PSW_HEAD + span + 32) return r;                        // the N' word lies inside the call
    const GwWord n_in = gww_word(cd + PSW_HEAD + span, al);
    if (!gww_fits32(n_in)) return r;
    if (len != PSW_HEAD + span + 32 + 32 * n_in.lo) return r;        // (below 2^38)
    r.ok = 1; r.lp = (uint32_t)lp.lo; r.n_in = (uint32_t)n_in.lo;
    return r;
}

// A batch of requests.  Request i is cd[off[i] .. off[i + 1]) to the contract at to[20 i ..]; every output row is the library's own
// (4-byte aligned): key / proofs / rows are the inputs of zkv_plonk_set_verify_batch_dev.
struct PswArgs {
    size_t n;
    const uint8_t* to; const uint8_t* cd; const uint64_t* off; uint64_t cd_bytes;
    const PswEntry* tab; uint32_t n_tab; uint32_t sel_be;
    uint32_t* key;                                        // n: the key of a request that is to be placed, else PSW_NONE
    uint32_t* rkey;                                       // n: the key its address resolved to, PSW_NONE without a lookup or a contract
    uint8_t* proofs; uint32_t proof_stride;               // n x proof_stride: row i holds the Lkey proof bytes, zeros behind them
    uint8_t* rows; uint32_t input_stride;                 // n x input_stride: the first nb words of row i are written
    uint8_t* verdict;                                     // n: PSW_CALL / PSW_BAD_CALLDATA / PSW_NO_CONTRACT
    uint8_t* reason;                                      // n: PSW_R_* 0 .. 4 of the decode
    uint8_t* npt;                                         // n: points the point test looks at: 9 + n_c of a request still standing, else 0
    uint8_t* ec;                                          // n: 0 from the decode; 1 from the point test (reason 5)
};

// What the header of request i says.  at: where the request starts in cd; pre: PSW_R_INPUT_COUNT when N' is not the key's nb, else
// PSW_R_PROOF_SIZE when Lp is not the key's Lkey, else 0 (calls only).
struct PswCall { uint32_t verdict, rkey, nb, n_c, lp, pre; uint64_t at; };

// Rules 1-3 and the two length rules of rule 4.  Every read of the request lies in [off[i], off[i + 1]).
ZKV_HD PswCall psw_resolve(const PswArgs& a, size_t i) {
    const uint64_t o0 = a.off[i], o1 = a.off[i + 1];
    PswCall c = {PSW_BAD_CALLDATA, PSW_NONE, 0, 0, 0, 0, 0};
    if (o0 <= o1 && o1 <= a.cd_bytes) {
        const uint32_t e = gsw_find(a.tab, a.n_tab, a.to + 20 * i);
        if (e == PSW_NONE) c.verdict = PSW_NO_CONTRACT;
        else {
            const PswEntry t = a.tab[e];
            c.rkey = t.key;
            const uint8_t* cd = a.cd + o0;
            const PswHead h = psw_parse(cd, o1 - o0, (((uintptr_t)cd) & 3u) == 0, a.sel_be);
            if (h.ok) {
                c.verdict = PSW_CALL; c.nb = t.nb; c.n_c = t.n_c; c.lp = h.lp; c.at = o0;
                c.pre = h.n_in != t.nb ? PSW_R_INPUT_COUNT : h.lp != 32 * (24 + 3 * t.n_c) ? PSW_R_PROOF_SIZE : PSW_R_NONE;
            }
        }
    }
    return c;
}
// Where the input words of a call start, from the start of the call
ZKV_HD uint64_t psw_inputs_at(const PswCall& c) { return PSW_HEAD + psw_pad32(c.lp) + 32; }
// The reason of a call once its words are scanned, in gnark's order: count, inputs >= r, proof size, openings >= r.
ZKV_HD uint32_t psw_reason(const PswCall& c, bool input_ge, bool opening_ge) {
    if (c.pre == PSW_R_INPUT_COUNT) return PSW_R_INPUT_COUNT;
    if (input_ge) return PSW_R_INPUT_RANGE;
    if (c.pre == PSW_R_PROOF_SIZE) return PSW_R_PROOF_SIZE;
    return opening_ge ? PSW_R_OPENING_RANGE : PSW_R_NONE;
}
// The rows of request i once its words are copied.  A request still standing gets its key; the point test may take it back.
ZKV_HD void psw_finish(const PswArgs& a, size_t i, const PswCall& c, uint32_t reason) {
    const bool stands = c.verdict == PSW_CALL && reason == PSW_R_NONE;
    a.key[i] = stands ? c.rkey : PSW_NONE;
    a.rkey[i] = c.rkey;
    a.verdict[i] = (uint8_t)c.verdict;
    a.reason[i] = (uint8_t)(c.verdict == PSW_CALL ? reason : PSW_R_NONE);
    a.npt[i] = (uint8_t)(stands ? 9 + c.n_c : 0);
    a.ec[i] = 0;
}
// Proof word `word` is an opening the contract tests against r: l r o s1 s2 (12-16), z(omega zeta) (19) and, with a commitment, qcp(zeta) (24)
ZKV_HD bool psw_is_opening(uint32_t word, uint32_t n_c) { return (word >= 12 && word <= 16) || word == 19 || (word == 24 && n_c != 0); }
// r's dword of significance k (k = 0 the most significant), by selects: a lane keeps its k through every step
ZKV_HD uint32_t psw_r_dword(uint32_t k) {
    return k == 0 ? 0x30644e72u : k == 1 ? 0xe131a029u : k == 2 ? 0xb85045b6u : k == 3 ? 0x8181585du : k == 4 ? 0x2833e848u
         : k == 5 ? 0x79b97091u : k == 6 ? 0x43e1f593u : 0xf0000001u;
}
// A dword in memory order against r's dword of significance k -> 0 equal, 1 less, 2 greater
ZKV_HD uint32_t psw_cmp_r(uint32_t v, uint32_t k) {
    const uint32_t be = __builtin_bswap32(v), rk = psw_r_dword(k);
    return be == rk ? 0u : be < rk ? 1u : 2u;
}

// Request i, start to end, by one thread: the plain form of the decode, which the wavefront form below must equal.
ZKV_HD void psw_request(const PswArgs& a, size_t i) {
    const PswCall c = psw_resolve(a, i);
    bool in_ge = false, op_ge = false;
    if (c.verdict == PSW_CALL && c.pre != PSW_R_INPUT_COUNT) {
        const uint8_t* cd = a.cd + c.at;
        const bool al = (((uintptr_t)cd) & 3u) == 0, store = c.pre == PSW_R_NONE;
        const uint8_t* src = cd + psw_inputs_at(c);
        uint32_t* row = (uint32_t*)(a.rows + (size_t)a.input_stride * i);
        for (uint32_t b = 0; b < c.nb; b++, src += 32) {
            uint32_t w[8];
            for (int k = 0; k < 8; k++) { const uint32_t v = gsw_ld4(src + 4 * k, al); if (store) row[8 * b + k] = v; w[k] = __builtin_bswap32(v); }
            in_ge = gsw_ge_r(w) || in_ge;
        }
        if (store) {
            uint32_t* proof = (uint32_t*)(a.proofs + (size_t)a.proof_stride * i);
            const uint32_t n_words = 24 + 3 * c.n_c;
            src = cd + PSW_HEAD;
            for (uint32_t b = 0; b < a.proof_stride / 32; b++, src += 32) {
                uint32_t w[8];
                for (int k = 0; k < 8; k++) { const uint32_t v = b < n_words ? gsw_ld4(src + 4 * k, al) : 0u; proof[8 * b + k] = v; w[k] = __builtin_bswap32(v); }
                if (b < n_words && psw_is_opening(b, c.n_c)) op_ge = gsw_ge_r(w) || op_ge;
            }
        }
    }
    psw_finish(a, i, c, psw_reason(c, in_ge, op_ge));
}

// ---- The wavefront form (k_pset_wire_decode): every lane resolves its own request, then the 64 lanes copy the words of one call after
// the other together, a dword per lane, so that a wave instruction reads and writes 256 contiguous bytes.  Dword w of a run of words
// (w = 8 b + k: dword k of word b, k = 0 the most significant) goes to lane w % 64, so eight neighbouring lanes hold one word, and the
// lanes' answers of a step make the two masks gsw_any_ge_r takes.
// One lane's share of one step over the input words: dword w of the `n_dwords` at `src`, stored when `store`.  -> 0 equal to r's dword
// of the same significance, 1 less (also: no such dword), 2 greater.
ZKV_HD uint32_t psw_input_dword(const uint8_t* src, bool al, uint32_t* row, bool store, uint32_t w, uint32_t n_dwords) {
    if (w >= n_dwords) return 1;
    const uint32_t v = gsw_ld4(src + 4 * (size_t)w, al);
    if (store) row[w] = v;
    return psw_cmp_r(v, w & 7u);
}
// The same over a proof row of `row_dwords` dwords: dword w of the 8 (24 + 3 n_c) at `src`, zero behind them; a word that is no
// opening answers 1.
ZKV_HD uint32_t psw_proof_dword(const uint8_t* src, bool al, uint32_t* row, uint32_t w, uint32_t n_c, uint32_t row_dwords) {
    if (w >= row_dwords) return 1;
    if (w >= 8 * (24 + 3 * n_c)) { row[w] = 0; return 1; }
    const uint32_t v = gsw_ld4(src + 4 * (size_t)w, al);
    row[w] = v;
    return psw_is_opening(w >> 3, n_c) ? psw_cmp_r(v, w & 7u) : 1u;
}

// ---- The point test (k_pset_wire_points), on the copied row of a request still standing after the decode: point p of the proof is no
// input of the EC precompiles -- a coordinate >= p, or off the curve; (0, 0) is infinity and passes.
ZKV_HD uint32_t psw_point_word(uint32_t p) {              // L R O H0 H1 H2 Z H_zeta H_zeta_omega BSB22
    return p < 6 ? 2 * p : p == 6 ? 17u : p == 7 ? 20u : p == 8 ? 22u : 25u;
}
ZKV_HD bool psw_point_bad(const uint8_t* proof_row, uint32_t p) {
    const uint32_t* q = (const uint32_t*)proof_row + 8 * psw_point_word(p);
    uint32_t x[8], y[8];
    for (int k = 0; k < 8; k++) { x[7 - k] = __builtin_bswap32(q[k]); y[7 - k] = __builtin_bswap32(q[8 + k]); }
    G1A pt; uint32_t inf;
    return !plonk_g1(x, y, pt, inf);
}
// Point p of request i, one thread: "bad" is a plain byte store into the request's row, and the request loses its key.  Several points
// of one request may store; they store the same values.
ZKV_HD void psw_point(const PswArgs& a, size_t i, uint32_t p) {
    if (p >= a.npt[i]) return;
    if (psw_point_bad(a.proofs + (size_t)a.proof_stride * i, p)) { a.ec[i] = 1; a.key[i] = PSW_NONE; }
}

}  // namespace zkv

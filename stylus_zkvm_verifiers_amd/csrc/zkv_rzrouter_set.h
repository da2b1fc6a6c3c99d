// RISC Zero router, set route (include/zkv_risc0_router_set.h): the header arithmetic of one on-chain set-inclusion
// seal, set_selector || abi.encode(Seal{bytes32[] path; bytes rootSeal}), and the identity of root seals -- a fingerprint that picks a
// table slot and the byte comparison that decides.  Shared by k_rzrouter_set.hip and the host (tests/host_sim/host_sim_rzrouter_set.cpp).
//   body = 0x20 | 0x40 | 0x60 + 32 k | k | k path elements | L | root seal, zero padded to pad32(L)
// Only the canonical encoding passes (tests/set_inclusion_model.py abi_decode_seal is the definition): every word lies inside the seal
// before it is read, each offset word holds its one value, k and L are below 2^32 (refused before they are multiplied), the padding
// behind the root seal is zero, and the total length is exactly 4 + 160 + 32 k + pad32(L).  Parity unpinned: the reference has no router
// and no set verifier.
#pragma once
#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#include "zkv_verify.h"
#endif
#include "zkv_bytes.h"
#include "zkv_wire_gateway.h"

namespace zkv {

constexpr uint32_t RZS_NOT_SET = 0, RZS_MALFORMED = 1, RZS_CLAIM = 2;
constexpr uint64_t RZS_PATH_AT = 4 + 128;                            // the first path element, from the start of the seal

// kind RZS_NOT_SET: shorter than 4 bytes or another selector (the router's own partition answers it); RZS_MALFORMED: the set selector
// in front of a body that is not canonical; RZS_CLAIM: depth path elements from byte RZS_PATH_AT and root_len root-seal bytes from byte
// root_at of the seal, both inside [0, len).  Every field but kind is 0 unless kind is RZS_CLAIM.
struct RzsSeal { uint32_t kind, depth, root_len; uint64_t root_at; };

// seal: the `len` bytes of one seal (every read stays inside them); al: seal is 4-byte aligned; set_sel_be: the set selector as a
// big-endian word.
ZKV_HD RzsSeal rzs_parse(const uint8_t* seal, uint64_t len, bool al, uint32_t set_sel_be) {
    RzsSeal r = {RZS_NOT_SET, 0, 0, 0};
    if (len < 4 || load_be32(seal) != set_sel_be) return r;
    r.kind = RZS_MALFORMED;
    const uint8_t* b = seal + 4;
    const uint64_t blen = len - 4;
    if (blen < 160 || (blen & 31)) return r;                         // the shortest body: 0x20, two offsets, two length words
    const GwWord w0 = gww_word(b, al), w1 = gww_word(b + 32, al), k = gww_word(b + 96, al);
    if (!gww_fits32(w0) || w0.lo != 0x20 || !gww_fits32(w1) || w1.lo != 0x40 || !gww_fits32(k)) return r;
    if (k.lo > (blen - 160) / 32) return r;                          // the path leaves room for the root seal's length word
    const GwWord w2 = gww_word(b + 64, al);
    if (w2.high || w2.lo != 0x60 + 32 * k.lo) return r;              // k < 2^32: no overflow
    const uint64_t l_at = 128 + 32 * k.lo;                           // l_at + 32 <= blen by the bound on k
    const GwWord n = gww_word(b + l_at, al);
    if (!gww_fits32(n)) return r;
    const uint64_t padded = gww_span(GWW_FORM_BYTES, n.lo);          // < 2^33
    if (blen != l_at + 32 + padded) return r;                        // nothing missing, nothing trailing
    for (uint64_t q = n.lo; q < padded; q++) if (b[l_at + 32 + q]) return r;     // at most 31 bytes of padding, all zero
    r.kind = RZS_CLAIM; r.depth = (uint32_t)k.lo; r.root_len = (uint32_t)n.lo; r.root_at = 4 + l_at + 32;
    return r;
}

// The seal of row i given as a record instead of a pair of offsets (decoded calldata: zkv_wire_rzset.h): `len` bytes from `at`, a
// distance from RzsArgs::seals.  A request that is not a canonical call has {0, 0}.
struct RzsSpan { uint64_t at; uint32_t len, pad; };

// The claim digest of row i of a batch: true = in_a holds it (verifyIntegrity), false = it is ReceiptClaim::ok(in_a, in_b) (verify).
// method: the per-row method bytes (ZKV_METHOD_*; rows with other bytes are no set seals) or nullptr: one method for the batch, verify
// iff the batch has second inputs.
ZKV_HD bool rzs_claim_given(const uint8_t* method, bool have_in_b, size_t i) { return method ? method[i] == 1 : !have_in_b; }

// Root-seal identity.  The fingerprint of (length, first min(length, 260) bytes) only picks where a claim starts probing the table; two
// root seals are one group iff rzs_equal says so.  Any alignment.  The fingerprint is the XOR of every word mixed with its position, so
// that the lanes of a wavefront can each take words and combine them in any order (k_rzset_ident); the host walks the words in turn.
ZKV_HD uint32_t rzs_mix(uint32_t x) { x ^= x >> 16; x *= 0x85EBCA6Bu; x ^= x >> 13; x *= 0xC2B2AE35u; return x ^ (x >> 16); }
ZKV_HD uint32_t rzs_fp_word(uint32_t v, uint32_t w) { return rzs_mix(v + 0x9E3779B1u * (w + 1)); }      // word w (bytes 4 w .. 4 w + 3, zero padded)
ZKV_HD uint32_t rzs_fp_finish(uint32_t acc, uint32_t len) { return rzs_mix(acc ^ rzs_mix(len ^ 0x811C9DC5u)); }
ZKV_HD uint32_t rzs_fp_take(uint32_t len) { return len < 260u ? len : 260u; }
ZKV_HD uint32_t rzs_fingerprint(const uint8_t* p, uint32_t len) {
    const uint32_t take = rzs_fp_take(len);
    uint32_t acc = 0;
    for (uint32_t w = 0; 4 * w < take; w++) acc ^= rzs_fp_word(gw_ld4(p + 4 * w, take - 4 * w), w);
    return rzs_fp_finish(acc, len);
}
ZKV_HD bool rzs_equal(const uint8_t* a, uint32_t la, const uint8_t* b, uint32_t lb) {
    if (la != lb) return false;
    for (uint64_t at = 0; at < la; at += 4) if (gw_ld4(a + at, la - at) != gw_ld4(b + at, la - at)) return false;
    return true;
}

}  // namespace zkv

// ---------------------------------------------------------------- kernels (k_rzrouter_set.hip) and their host-side launchers
#if defined(__HIPCC__)
#include "zkv_setincl.h"

namespace zkv {

// claim_job of a seal that is not a set seal (beside SETINCL_DONE / _MEMBER / _PENDING and the job slots): the set stage never writes
// its status
constexpr uint32_t RZS_JOB_NOT_SET = 0xFFFFFFFCu;
constexpr uint32_t RZS_EMPTY = 0xFFFFFFFFu;         // table slot nobody owns

// Claim record of a canonical set seal, byte positions in the caller's blob: `depth` path elements from path_at, root_len root-seal
// bytes from root_at (root_len = 0: the root is looked up among the submitted roots).
struct RzsRec { uint64_t path_at, root_at; uint32_t depth, root_len; };

// What the set stage adds to a chunk's SetinclChunk.  The chunk's claims are ALL seals of the chunk, set seals or not: claim_job tells
// them apart.  SetinclChunk::m is the table size, ::rep / ::gslot have one word per table slot and ::root_idx (= root_idx below) holds
// the slot a claim's root seal lives in, so k_setincl_group runs on it as it is.  ::counters has four words: [0] jobs of the chunk,
// and, summed over the call's chunks, [1] stored-root lookups, [2] set seals, [3] distinct root seals (slots taken).
struct RzsArgs {
    const uint8_t* seals; const uint64_t* seal_off; uint64_t seal_bytes;       // the call's blob; the chunk's n + 1 offsets
    const RzsSpan* span; const uint32_t* wire_len;                             // decoded calldata (seal_off == nullptr): the chunk's records and true
                                                                               // lengths, 0xFFFFFFFF = not a canonical call; read by rzs_span alone
    const uint8_t* method;                                                     // the chunk's method row, or nullptr (rzs_claim_given)
    uint32_t set_sel, table, fp_mask, pad;                                     // table: a power of two >= 2 n; fp_mask: ~0 (diagnostic: less)
    RzsRec* rec; uint32_t* owner; uint32_t* root_idx; uint8_t* ans;            // per seal; per slot: the claim that took it; per seal: the answer of a
                                                                               // claim that is SETINCL_DONE (written to status by the scatter)
};
void launch_rzset_front(const SetinclChunk& c, const RzsArgs& a, hipStream_t s);      // classify, parse, limits; then root-seal identity
void launch_rzset_hash(const SetinclChunk& c, const RzsArgs& a, const Risc0Consts& k, hipStream_t s);
void launch_rzset_jobs(const SetinclChunk& c, const RzsArgs& a, const SetinclJobs& j, hipStream_t s);
void launch_rzset_scatter(const SetinclChunk& c, const RzsArgs& a, const SetinclJobs& j, hipStream_t s);
void launch_rzset_reps(const SetinclChunk& c, const RzsArgs& a, uint32_t* out, hipStream_t s);     // diagnostic: every claim's representative

}  // namespace zkv
#endif

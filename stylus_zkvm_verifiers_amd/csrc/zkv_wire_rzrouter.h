// Header arithmetic of one `verify` / `verifyIntegrity` call to the RISC Zero router (include/zkv_risc0_router_wire.h), shared by
// k_wire_rzrouter (k_wire.hip) and the host (tests/host_sim/host_sim_rzrouter_wire.cpp).  Four call shapes, told apart by the function
// selector; `kind` = 2 form + method is the index of the selector (RZW_KINDS of them):
//   kind 0  form U  verify(uint8[],bytes32,bytes32)    = sel | 0x60 | image_id | journal_digest | L | L element words
//   kind 1  form U  verifyIntegrity(uint8[],bytes32)   = sel | 0x40 | claim_digest | L | L element words
//   kind 2  form B  verify(bytes,bytes32,bytes32)      = sel | 0x60 | image_id | journal_digest | L | seal, zero padded to pad32(L)
//   kind 3  form B  verifyIntegrity((bytes,bytes32))   = sel | 0x20 | 0x40 | claim_digest | L | seal, zero padded to pad32(L)
// Only the canonical encoding passes: the offset words exactly as above, L below 2^32 (refused before it is multiplied), every word inside
// the call before it is read, and a total length of exactly the head, the length word and 32 L (form U) or pad32(L) (form B) bytes.  What
// the header cannot see -- a uint8[] element above 255, a non-zero padding byte -- is left to the caller, who streams the body.
// Parity unpinned: the reference has no router.
#pragma once
#include "zkv_wire_gateway.h"

namespace zkv {

constexpr int RZW_KINDS = 4;
constexpr uint32_t RZW_KIND_BAD = 255;                               // the call kind of a request that is not a canonical call

// ok = 0: not a canonical call (every other field is 0).  a_at: byte position, from the start of the call, of the image id (the journal
// digest follows it) or the claim digest; seal_at: of the first element word (form U) or first seal byte (form B).  The body,
// [seal_at, len), lies inside the call.
struct RzwCall { uint32_t ok, form, method, seal_len; uint32_t a_at; uint64_t seal_at; };

// cd: the `len` bytes of one call (every read stays inside them); al: cd is 4-byte aligned; sel_be[kind]: the four selectors as
// big-endian words.
ZKV_HD RzwCall rzw_parse(const uint8_t* cd, uint64_t len, bool al, const uint32_t* sel_be) {
    RzwCall r = {0, 0, 0, 0, 0, 0};
    if (len < 4) return r;
    const uint32_t sel = load_be32(cd);
    int kind = -1;
    for (int k = 0; k < RZW_KINDS; k++) if (sel == sel_be[k]) kind = k;
    if (kind < 0) return r;
    const uint32_t form = (uint32_t)kind >> 1, method = (uint32_t)kind & 1u;
    const uint64_t l_at = kind == 1 ? 4 + 64 : 4 + 96;               // the length word: behind two head words (kind 1) or three
    if (len < l_at + 32) return r;                                   // the head words and the length word lie inside the call
    const GwWord o = gww_word(cd + 4, al);
    if (!gww_fits32(o) || o.lo != (kind == 3 ? 0x20u : (uint32_t)(l_at - 4))) return r;
    if (kind == 3) {                                                 // the Receipt tuple: its own offset to the seal
        const GwWord o2 = gww_word(cd + 36, al);
        if (!gww_fits32(o2) || o2.lo != 0x40) return r;
    }
    const GwWord n = gww_word(cd + l_at, al);
    if (!gww_fits32(n)) return r;
    if (len != l_at + 32 + gww_span(form, n.lo)) return r;           // span < 2^37: no overflow
    r.ok = 1; r.form = form; r.method = method; r.seal_len = (uint32_t)n.lo;
    r.a_at = kind == 3 ? 68u : 36u; r.seal_at = l_at + 32;
    return r;
}

}  // namespace zkv

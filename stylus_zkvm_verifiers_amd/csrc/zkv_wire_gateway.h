// Header arithmetic of one `verifyProof` call to the SP1 gateway (include/zkv_sp1_gateway_wire.h), shared by k_wire_gateway (k_wire.hip)
// and the host (tests/host_sim/host_sim_gateway_wire.cpp).  Two calldata forms, told apart by the function selector:
//   form U  verifyProof(bytes32,uint8[],uint8[]) = sel | vkey | 0x60 | 0x80 + 32 Lpv        | Lpv | Lpv words       | Lproof | Lproof words
//   form B  verifyProof(bytes32,bytes,bytes)     = sel | vkey | 0x60 | 0x80 + pad32(Lpv)    | Lpv | pv, zero padded | Lproof | proof, zero padded
// Only the canonical encoding passes: both offsets exactly as above, both lengths below 2^32, and a total length of exactly
// 4 + 96 + 32 + span(Lpv) + 32 + span(Lproof) with span(L) = 32 L (form U) or pad32(L) (form B).  What the header cannot see -- a uint8[]
// element above 255, a non-zero padding byte -- is left to the caller, who streams the bodies.  Parity unpinned: the reference has no gateway.
#pragma once
#include <stdint.h>
#include <stddef.h>
#include "zkv_sha256.h"

namespace zkv {

constexpr uint32_t GWW_FORM_UINT8_ARRAY = 0, GWW_FORM_BYTES = 1;    // ZKV_CALLDATA_FORM_*
constexpr uint64_t GWW_HEAD = 4 + 96 + 32;                           // selector, three head words, the first length word

// One 32-byte ABI word as its low 64 bits and "one of the upper 24 bytes is set".  `al`: the word is 4-byte aligned.
struct GwWord { uint64_t lo; bool high; };
ZKV_HD GwWord gww_word(const uint8_t* p, bool al) {
    uint32_t hi = 0, w6, w7;
    if (al) {
        const uint32_t* q = (const uint32_t*)p;
        hi = q[0] | q[1] | q[2] | q[3] | q[4] | q[5];
        w6 = __builtin_bswap32(q[6]); w7 = __builtin_bswap32(q[7]);
    } else {
        for (int k = 0; k < 24; k++) hi |= p[k];
        w6 = load_be32(p + 24); w7 = load_be32(p + 28);
    }
    GwWord r; r.lo = ((uint64_t)w6 << 32) | w7; r.high = hi != 0;
    return r;
}
ZKV_HD bool gww_fits32(const GwWord& w) { return !w.high && w.lo <= 0xFFFFFFFFull; }

// ok = 0: not a canonical call (every other field is 0).  pv_at / proof_at: byte position, from the start of the call, of the first
// element word (form U) or first byte (form B) of the two arguments; both bodies lie inside [0, len).
struct GwCall { uint32_t ok, form, pv_len, proof_len; uint64_t pv_at, proof_at; };

ZKV_HD uint64_t gww_span(uint32_t form, uint64_t len32) {           // bytes of an argument's body; len32 < 2^32, so no 64-bit overflow
    return form == GWW_FORM_UINT8_ARRAY ? 32 * len32 : (len32 + 31) & ~(uint64_t)31;
}

// cd: the `len` bytes of one call (every read stays inside them); al: cd is 4-byte aligned; the two selectors as big-endian words.
ZKV_HD GwCall gww_parse(const uint8_t* cd, uint64_t len, bool al, uint32_t sel_u_be, uint32_t sel_b_be) {
    GwCall r = {0, 0, 0, 0, 0, 0};
    if (len < GWW_HEAD + 32) return r;                               // shortest call: both arguments empty
    const uint32_t sel = load_be32(cd);
    if (sel != sel_u_be && sel != sel_b_be) return r;
    const uint32_t form = sel == sel_u_be ? GWW_FORM_UINT8_ARRAY : GWW_FORM_BYTES;
    const GwWord o1 = gww_word(cd + 36, al), o2 = gww_word(cd + 68, al), n1 = gww_word(cd + 100, al);
    if (!gww_fits32(o1) || o1.lo != 0x60 || !gww_fits32(n1)) return r;
    const uint64_t span1 = gww_span(form, n1.lo);                    // < 2^37
    if (o2.high || o2.lo != 0x80 + span1) return r;
    if (len < GWW_HEAD + span1 + 32) return r;                       // the second length word lies inside the call
    const GwWord n2 = gww_word(cd + GWW_HEAD + span1, al);
    if (!gww_fits32(n2)) return r;
    if (len != GWW_HEAD + span1 + 32 + gww_span(form, n2.lo)) return r;
    r.ok = 1; r.form = form; r.pv_len = (uint32_t)n1.lo; r.proof_len = (uint32_t)n2.lo;
    r.pv_at = GWW_HEAD; r.proof_at = GWW_HEAD + span1 + 32;
    return r;
}

}  // namespace zkv

// Loads from caller byte buffers that may have ANY alignment (include/zkv.h: byte-typed buffers carry no alignment contract): the typed
// fast path is taken only behind an address test, everything else goes byte by byte.  Host-compilable so that the byte paths, which a
// freshly allocated buffer never reaches, run under test (tests/host_sim/host_sim_geometry.cpp).
#pragma once
#include <stdint.h>
#include <stddef.h>
#include "zkv_field.h"

namespace zkv {

// k_gateway.hip / k_mixed.hip: a word of a ragged proof or of a 32-byte input
ZKV_HD uint32_t gw_ld4(const uint8_t* p, uint64_t avail) {      // up to 4 bytes, zero padded, any alignment
    if (avail >= 4 && !((uintptr_t)p & 3u)) return *(const uint32_t*)p;
    uint32_t v = 0;
    for (int k = 0; k < 4; k++) if ((uint64_t)k < avail) v |= (uint32_t)p[k] << (8 * k);
    return v;
}
ZKV_HD uint32_t mx_ld4(const uint8_t* p, size_t avail) {      // up to 4 bytes, zero padded, any alignment
    if (avail >= 4 && !((uintptr_t)p & 3u)) return *(const uint32_t*)p;
    uint32_t v = 0;
    for (int k = 0; k < 4; k++) if ((size_t)k < avail) v |= (uint32_t)p[k] << (8 * k);
    return v;
}

// k_wire.hip
// One 32-byte ABI word that must hold a value < 2^32.  `al` (wave-uniform): the word is 4-byte aligned.
struct WordVal { uint32_t v; bool small; };
ZKV_HD WordVal wire_word(const uint8_t* p, bool al) {
    uint32_t hi = 0, last;
    if (al) {
        const uint32_t* q = (const uint32_t*)p;
        uint32_t w0 = q[0], w1 = q[1], w2 = q[2], w3 = q[3], w4 = q[4], w5 = q[5], w6 = q[6];
        hi = w0 | w1 | w2 | w3 | w4 | w5 | w6;
        last = __builtin_bswap32(q[7]);
    } else {
#pragma unroll 4
        for (int k = 0; k < 28; k++) hi |= p[k];
        last = ((uint32_t)p[28] << 24) | ((uint32_t)p[29] << 16) | ((uint32_t)p[30] << 8) | p[31];
    }
    WordVal r; r.v = last; r.small = hi == 0;
    return r;
}

}  // namespace zkv

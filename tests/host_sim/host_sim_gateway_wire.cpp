// Host build of the header arithmetic k_wire_gateway runs on every eth_call request to the SP1 gateway
// (stylus_zkvm_verifiers_amd/csrc/zkv_wire_gateway.h): both calldata forms, offsets, lengths, the exact-total-length test.  TEST ONLY.
#include <stdint.h>
#include <string.h>
#include <stdlib.h>
#include "../../stylus_zkvm_verifiers_amd/csrc/zkv_wire_gateway.h"
using namespace zkv;

// out = {ok, form, pv_len, proof_len, pv_at, proof_at}.  The call is parsed from a private copy of exactly `len` bytes placed `shift`
// bytes past a 16-byte boundary, so a read outside the call is a read outside the allocation; shift 0 takes the aligned word loads.
extern "C" int hsgw_parse(const uint8_t* cd, uint64_t len, uint32_t shift, uint32_t sel_u_be, uint32_t sel_b_be, uint64_t out[6]) {
    uint8_t* raw = (uint8_t*)aligned_alloc(16, (size_t)((len + shift + 15) / 16 * 16 + 16));
    if (!raw) return -1;
    uint8_t* p = raw + shift;
    if (len) memcpy(p, cd, (size_t)len);
    const GwCall c = gww_parse(p, len, (((uintptr_t)p) & 3u) == 0, sel_u_be, sel_b_be);
    out[0] = c.ok; out[1] = c.form; out[2] = c.pv_len; out[3] = c.proof_len; out[4] = c.pv_at; out[5] = c.proof_at;
    free(raw);
    return 0;
}

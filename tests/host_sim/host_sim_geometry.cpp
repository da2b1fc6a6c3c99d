// Host build of the code that first touches the caller's bytes (csrc/zkv_sha256.h, ShaStream of csrc/zkv_plonk.h, csrc/zkv_bytes.h) for
// CPU-side tests.  TEST ONLY: the shipped library runs these functions inside HIP kernels; this file lets `-m "not gpu"` tests drive
// them at the lengths, byte phases and alignments a freshly allocated buffer never presents.
#include <stdint.h>
#include <string.h>
#include "../../stylus_zkvm_verifiers_amd/csrc/zkv_host_vk.h"
#include "../../stylus_zkvm_verifiers_amd/csrc/zkv_plonk.h"
#include "../../stylus_zkvm_verifiers_amd/csrc/zkv_bytes.h"

using namespace zkv;

static void put_digest(const uint32_t h[8], uint8_t* out) {
    for (int i = 0; i < 8; i++) { out[4 * i] = h[i] >> 24; out[4 * i + 1] = h[i] >> 16; out[4 * i + 2] = h[i] >> 8; out[4 * i + 3] = h[i]; }
}

extern "C" {
void hsg_sha256(const uint8_t* m, size_t n, uint8_t* out) { uint32_t h[8]; sha256_bytes(m, n, h); put_digest(h, out); }
// the SP1 signal as k_prep_sp1 forms it from the digest: h[0] &= 0x1fffffff, limbs little-endian
void hsg_sp1_signal(const uint8_t* m, size_t n, uint32_t* limbs) {
    uint32_t h[8]; sha256_bytes(m, n, h);
    h[0] &= 0x1fffffffu;
    for (int j = 0; j < 8; j++) limbs[7 - j] = h[j];
}
// ShaStream fed by a script: ops[i] = 0 one byte, 1 word_be (4 bytes), 2 limbs_be (32 bytes), taken from m in order.  Returns the number
// of message bytes consumed (the caller makes the script cover the message exactly).
size_t hsg_sha_stream(const uint8_t* m, const uint8_t* ops, size_t n_ops, uint8_t* out) {
    ShaStream s; s.init();
    size_t at = 0;
    for (size_t i = 0; i < n_ops; i++) {
        if (ops[i] == 0) { s.byte(m[at]); at += 1; }
        else if (ops[i] == 1) { s.word_be(load_be32(m + at)); at += 4; }
        else { uint32_t l[8]; load_be256(l, m + at); s.limbs_be(l); at += 32; }
    }
    uint32_t h[8]; s.finish(h); put_digest(h, out);
    return at;
}
uint32_t hsg_gw_ld4(const uint8_t* p, uint64_t avail) { return gw_ld4(p, avail); }
uint32_t hsg_mx_ld4(const uint8_t* p, uint64_t avail) { return mx_ld4(p, (size_t)avail); }
// wire_word through the branch `al` selects (al = 1 needs a 4-byte aligned p): out[0] = value of the low four bytes, out[1] = "the upper 28 are zero"
void hsg_wire_word(const uint8_t* p, int al, uint32_t* out) { const WordVal w = wire_word(p, al != 0); out[0] = w.v; out[1] = w.small ? 1u : 0u; }
}

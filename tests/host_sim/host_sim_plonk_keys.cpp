// Host build of the PLONK pre-pairing stage for any key (include/zkv_plonk_keys.h: plonk_prepare with the public inputs read from the
// proof's row, as k_plonk_prep_keys runs it) for CPU-side tests.  TEST ONLY: the shipped library never runs this on the host.
#include <stdint.h>
#include <string.h>
#include "../../stylus_zkvm_verifiers_amd/csrc/zkv_host_vk.h"
#include "../../stylus_zkvm_verifiers_amd/csrc/zkv_plonk.h"

using namespace zkv;

static void wr_be(uint8_t* p, const uint32_t l[8]) { for (int i = 0; i < 8; i++) for (int k = 0; k < 4; k++) p[31 - 4 * i - k] = (uint8_t)(l[i] >> (8 * k)); }

static PlonkKey* key_for(const uint8_t* vk, size_t vk_len) {
    if (vk_len < 7 * 32) return nullptr;
    uint32_t w7[7][8];
    for (int k = 0; k < 7; k++) host::be_to_limbs(w7[k], vk + 32 * k);
    const size_t n_c = w7[5][0];
    if (n_c > 1 || vk_len != 7 * 32 + (8 + n_c) * 64 + 256 || w7[4][0] > PLONK_MAX_PUBLIC) return nullptr;
    static PlonkKeyRaw raw, last; static PlonkKey key; static bool have = false;
    memset(&raw, 0, sizeof raw);
    memcpy(raw.size, w7[0], 32); memcpy(raw.size_inv, w7[1], 32); memcpy(raw.gen, w7[2], 32); memcpy(raw.coset, w7[3], 32);
    raw.nb_public = w7[4][0]; raw.n_c = w7[5][0]; raw.cci = w7[6][0];
    for (size_t p = 0; p < 8 + n_c; p++) { host::be_to_limbs(raw.pts[p][0], vk + 224 + 64 * p); host::be_to_limbs(raw.pts[p][1], vk + 256 + 64 * p); }
    if (!have || memcmp(&raw, &last, sizeof raw) != 0) {     // the tables of a key are built once per key
        plonk_setup_key(raw, key, true); plonk_setup_tables(key);
        last = raw; have = true;
    }
    return &key;
}
extern "C" {
// vk: the serialisation of include/zkv_plonk_keys.h; proof: 24 + 3 n_c words; pub: nb_public x 32 bytes.  Returns -1 for a malformed
// key, 0 when the stage rejects, 1 when it produced the pairing inputs: out = D.x D.y Q.x Q.y (128 bytes, (0,0) = infinity).  The G2
// points are not looked at here (the device judges them with the line tables).
int hspk_prepare(const uint8_t* vk, size_t vk_len, const uint8_t* proof, size_t proof_len, const uint8_t* pub, uint8_t* out128) {
    PlonkKey* kp = key_for(vk, vk_len);
    if (!kp || proof_len != 32 * (24 + 3 * (size_t)kp->n_c)) return -1;
    uint32_t w[27][8];
    memset(w, 0, sizeof w);
    for (size_t k = 0; k < proof_len / 32; k++) host::be_to_limbs(w[k], proof + 32 * k);
    PlonkOut o;
    static uint32_t tabmem[PLONK_TAB_WORDS];
    const TabRef tab = {tabmem};
    const PlonkPubRow row = {pub};
    if (!plonk_prepare(*kp, w, row, o, tab)) return 0;
    memset(out128, 0, 128);
    uint32_t r[8];
    G1A d, q; uint32_t d_inf, q_inf;
    g1j_to_affine(o.d, d, d_inf); g1j_to_affine(o.q, q, q_inf);
    if (!d_inf) { fp_to_raw(r, d.x); wr_be(out128, r); fp_to_raw(r, d.y); wr_be(out128 + 32, r); }
    if (!q_inf) { fp_to_raw(r, q.x); wr_be(out128 + 64, r); fp_to_raw(r, q.y); wr_be(out128 + 96, r); }
    return 1;
}
}

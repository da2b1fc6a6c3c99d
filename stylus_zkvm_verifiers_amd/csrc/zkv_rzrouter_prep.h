// RISC Zero router, keyed routes (include/zkv_risc0_router.h): the front end of one slot of the keyed group --
// verify_integrity_internal (risc0/verifier.rs:146-196) after the selector, which the router's classifier has matched, with the slot's
// route: its key's validity, its control root and control id.  The slot layout of the group is zkv_gset_layout.h's.
// __host__ __device__, so that tests/host_cpp/test_rzrouter_prep.cpp runs the kernel's own body on the CPU (plain and under the sanitizers).
#pragma once
#include "zkv_gwset_prep.h"

namespace zkv {

// The constants of one keyed route: control_root_0 / _1 (the 128-bit halves as verifier.rs:64-66 stores them) and bn254_control_id as
// little-endian limbs, and whether the control id is >= R (every proof of the route then fails at groth16.rs:32).
struct RzrRoute { uint32_t cr0[8], cr1[8], id[8]; uint32_t id_ge_r, pad[3]; };

// What the slot hands to the later stages.  sig: the five public signals (verifier.rs:173-179) as little-endian limbs, where k_gset_msm
// reads them; signals the checks did not reach stay zero.  o: the points, meaningful when flags has FL_ALIVE.
struct RzrSlot { uint8_t status; uint32_t flags; uint32_t sig[5][8]; PrepOut o; };

// The checks in the order of the reference: strict length (abi_decode of 8 static words), then verify_proof_with_key with the route's
// key -- a key with an invalid point fails here, as the precompiles would reject it --, every signal < R (only the control id can
// fail: the other four are 128-bit halves), the point encodings with A negated.
// in_a / in_b: image id and journal digest (verify), or claim digest and nullptr (verify_integrity); any alignment.
ZKV_HD void rzrouter_prep_slot(uint32_t vk_valid, const RzrRoute& rt, const Risc0Consts& k, uint32_t len, const uint8_t* in_a, const uint8_t* in_b,
                               const GwsetRec& rec, RzrSlot& r) {
    r.flags = 0;
#pragma unroll
    for (int b = 0; b < 5; b++) {
#pragma unroll
        for (int q = 0; q < 8; q++) r.sig[b][q] = 0;
    }
    if (len != 260) { r.status = ST_INVALID_PROOF_DATA; return; }
    r.status = ST_VERIFICATION_FAILED;
    if (!vk_valid || rt.id_ge_r) return;
    uint32_t h[8];
    if (in_b) risc0_claim_digest(k, in_a, in_b, h);
    else {
#pragma unroll 1
        for (int j = 0; j < 8; j++) h[j] = load_be32(in_a + 4 * j);
    }
#pragma unroll
    for (int q = 0; q < 8; q++) { r.sig[0][q] = rt.cr0[q]; r.sig[1][q] = rt.cr1[q]; r.sig[4][q] = rt.id[q]; }
    risc0_split_digest(h, r.sig[2], r.sig[3]);
    uint32_t w[8][8];
#pragma unroll 1
    for (int j = 0; j < 8; j++) rec.u256(w[j], 1 + 8 * j);
    if (prep_points(w, true, r.o)) r.flags = r.o.flags;
}

// The in_b of group slot `slot` as rzrouter_prep_slot takes it, chosen per slot: kind is the group's method row (ZKV_METHOD_*), or
// nullptr when the whole call has one method, which in_b then tells (nullptr: verify_integrity).
ZKV_HD const uint8_t* rzrouter_slot_in_b(const uint8_t* kind, const uint8_t* in_b, size_t slot) {
    if (!in_b || (kind && kind[slot] != 0)) return nullptr;
    return in_b + 32 * slot;
}

// Router classifier (k_risc0_router.hip) on the host as well: the column of a seal whose first four bytes are `sel` (big-endian word).
// Columns: 0 = the built-in group (all built-in routes; *inst = which), 1 + k = keyed route k, then not found.  sel[]: the built-in
// routes' selectors, then the keyed routes'.
constexpr int RZR_MAX_ROUTES = 32, RZR_MAX_KEYED = 8;
constexpr int RZR_COL_BUILTIN = 0, RZR_COL_KEYED0 = 1, RZR_COL_NOT_FOUND = 9, RZR_COL_SHORT = 10, RZR_COLS = 11;
ZKV_HD int rzrouter_column(const uint32_t* sel, uint32_t n_builtin, uint32_t n_keyed, uint32_t v, uint32_t* inst) {
    int c = RZR_COL_NOT_FOUND;
    *inst = 0;
#pragma unroll
    for (int r = 0; r < RZR_MAX_ROUTES; r++) {
        if ((uint32_t)r < n_builtin + n_keyed && v == sel[r]) {
            if ((uint32_t)r < n_builtin) { c = RZR_COL_BUILTIN; *inst = (uint32_t)r; }
            else c = RZR_COL_KEYED0 + (int)((uint32_t)r - n_builtin);
        }
    }
    return c;
}

}  // namespace zkv

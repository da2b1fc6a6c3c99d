// Slot layout of a Groth16 key-set batch (zkv_groth16_set_*): plain C++, shared by the C ABI and the host build of
// the tests (tests/host_sim/host_sim_gset_layout.cpp).
//
// The proofs of a batch are partitioned by key; key group k starts at slot start[k], a multiple of the proofs per wavefront of the
// Miller-loop mapping the batch takes (32 on lane pairs, 4 on 16 lanes, 1 on one or two wavefronts per proof), so that every
// wavefront of those kernels holds proofs of one key only.  The slots between a group's last proof and the next group are pad slots:
// they carry no proof.
#pragma once
#include <stddef.h>
#include <stdint.h>

namespace zkv {

// Proofs per wavefront of the Miller mappings, and the lanes-per-proof setting (zkv_ctx_set_lanes_per_proof) each corresponds to.
inline uint32_t gset_align_of_lanes(int lanes) { return lanes == 2 ? 32u : lanes == 16 ? 4u : 1u; }

// start[0 .. n_keys]: group k occupies slots [start[k], start[k] + cnt[k]), padded up to start[k + 1].  Returns the slot count.
inline uint64_t gset_layout(const uint32_t* cnt, uint32_t n_keys, uint32_t align, uint64_t* start) {
    uint64_t s = 0;
    for (uint32_t k = 0; k < n_keys; k++) {
        start[k] = s;
        s += ((uint64_t)cnt[k] + align - 1) / align * align;
    }
    start[n_keys] = s;
    return s;
}

// The mapping of a batch: `lanes` is what the automatic policy (or the caller) picked for the batch size.  An automatic choice steps
// to the next finer mapping (lane pairs -> 16 lanes -> one wavefront per proof) while the padded slot count exceeds 1.25 times the
// proofs; a mapping the caller fixed (fixed != 0) is kept.  Returns the lanes per proof and fills start[] (gset_layout).
inline int gset_choose(const uint32_t* cnt, uint32_t n_keys, int lanes, int fixed, uint64_t* start, uint64_t* slots) {
    uint64_t n = 0;
    for (uint32_t k = 0; k < n_keys; k++) n += cnt[k];
    for (;;) {
        *slots = gset_layout(cnt, n_keys, gset_align_of_lanes(lanes), start);
        if (fixed || 4 * *slots <= 5 * n || gset_align_of_lanes(lanes) == 1) return lanes;
        lanes = lanes == 2 ? 16 : 64;
    }
}

}  // namespace zkv

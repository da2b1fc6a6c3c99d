// Selector demultiplexer skeleton, shared by the SP1 gateway (k_gateway.hip) and the RISC Zero router (k_risc0_router.hip): what the
// count, place and gather kernels of a unit do once its classifier has given every item a column.  Columns [0, ROUTED) take slots,
// the columns from ROUTED on are answered in place.  The unit keeps its span and classifier functions and whatever else a slot
// carries; its __global__ kernels stay its own and call these with their __shared__ counts.  Workgroups are whole wavefronts.
#pragma once
#include "zkv_internal.h"
#include "zkv_bytes.h"

namespace zkv {

// Columns [0, COLS) of one workgroup: wc[k][wave] = items of column k in the wavefront (c < 0: no item on this lane).  Returns the
// ballot of the lane's own column (0 when c is outside [0, COLS)), from which demux_slot ranks the lane.  A __syncthreads() of the
// caller's separates this from the two readers below.
template <int COLS, int WAVES>
__device__ __forceinline__ uint64_t demux_ballots(int c, uint32_t (&wc)[COLS][WAVES]) {
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    uint64_t mine = 0;
#pragma unroll
    for (int k = 0; k < COLS; k++) {
        const uint64_t m = __ballot(c == k);
        if (c == k) mine = m;
        if (lane == 0) wc[k][wave] = (uint32_t)__popcll(m);
    }
    return mine;
}

// The count kernel's result: cnt[block * COLS + k] = items of column k in this workgroup.
template <int COLS, int WAVES>
__device__ __forceinline__ void demux_block_counts(const uint32_t (&wc)[COLS][WAVES], uint32_t* cnt) {
    if (threadIdx.x < COLS) {
        uint32_t t = 0;
        for (int w = 0; w < WAVES; w++) t += wc[threadIdx.x][w];
        cnt[(size_t)blockIdx.x * COLS + threadIdx.x] = t;
    }
}

// The place kernel's slot of an item of routed column c, a stable partition: its rank among the column's items in caller order -- the
// items of the column in earlier workgroups (cnt after the scan, COLS columns per block) and before it in this one -- from the column's
// first slot.  A column may have two regions (the aggregate check on a keyed group, zkv_gset_layout.h gset_agg_slot): the first agg[c]
// items go to astart[c] .., the others to start[c] ..; agg[c] = 0: one region from start[c].
template <int COLS, int ROUTED, int WAVES>
__device__ __forceinline__ uint32_t demux_slot(int c, uint64_t mine, const uint32_t (&wc)[ROUTED][WAVES], const uint32_t* start, const uint32_t* agg,
                                               const uint32_t* astart, const uint32_t* cnt) {
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const uint64_t below = lane ? (~0ull >> (64 - lane)) : 0ull;
    uint32_t r = (uint32_t)__popcll(mine & below);
    for (uint32_t w = 0; w < wave; w++) r += wc[c][w];
    r += cnt[(size_t)blockIdx.x * COLS + c];
    return r < agg[c] ? astart[c] + r : start[c] + (r - agg[c]);
}

// An item no verifier is asked about: answered here, no slot.  recv may be null.
__device__ __forceinline__ void demux_answer(size_t i, uint8_t st, uint32_t sel, uint32_t* pos, uint8_t* status, uint8_t* recv) {
    pos[i] = GW_NONE;
    status[i] = st;
    if (recv) {
        recv[4 * i] = (uint8_t)(sel >> 24); recv[4 * i + 1] = (uint8_t)(sel >> 16);
        recv[4 * i + 2] = (uint8_t)(sel >> 8); recv[4 * i + 3] = (uint8_t)sel;
    }
}

// The true length of an item as a slot carries it: every length a record can hold is told apart, the rest are "too long".
__device__ __forceinline__ uint32_t demux_len32(uint64_t len) { return len > 0xFFFFFFFEull ? 0xFFFFFFFEu : (uint32_t)len; }

// The gather kernel's record, one wavefront per item: the first min(len, rec) bytes of src as rec / 4 dwords, zero padded; any alignment of src.
__device__ __forceinline__ void demux_copy_record(uint32_t* dst, const uint8_t* src, uint64_t len, uint32_t rec, uint32_t lane) {
    if (len > rec) len = rec;
    for (uint32_t w = lane; w < rec / 4; w += 64) {
        const uint64_t at = 4ull * w;
        dst[w] = at < len ? gw_ld4(src + at, len - at) : 0u;
    }
}

}  // namespace zkv

// SP1 gateway, Groth16 routes with caller-supplied keys (include/zkv_sp1_gateway_keys.h): the SP1 front end of one
// slot of the keyed group -- sp1/verifier.rs:58-94 after the selector (the demultiplexer has matched it), with the slot's key.  The slot
// layout of the group is zkv_gset_layout.h's.  __host__ __device__, so that tests/host_cpp/test_gwset_prep.cpp runs the kernel's own body
// on the CPU (plain and under the sanitizers).
#pragma once
#include "zkv_verify.h"
#if defined(__HIPCC__)
#include "zkv_internal.h"
#endif

namespace zkv {

// The 65 words of a compact 260-byte record: a row staged in LDS (words still hold big-endian bytes) or the record itself, byte by byte.
struct GwsetRec {
    const uint32_t* row;        // non-null: the staged row
    const uint8_t* rec;         // otherwise: the record
    ZKV_HD uint32_t word(int k) const { return row ? __builtin_bswap32(row[k]) : load_be32(rec + 4 * k); }
    ZKV_HD void u256(uint32_t limbs[8], int word0) const {
#pragma unroll 1
        for (int j = 0; j < 8; j++) limbs[7 - j] = word(word0 + j);
    }
};

// What the slot hands to the later stages.  sig: the two public signals as little-endian limbs (program vkey, masked SHA-256 of the
// public values); a signal the checks did not reach stays zero.  o: the points, meaningful when flags has FL_ALIVE.
struct GwsetSlot { uint8_t status; uint32_t flags; uint32_t sig[2][8]; PrepOut o; };

// k_prep_sp1's checks in the order of the reference: strict length (verifier.rs:80-82), then verify_proof_with_key with the route's key
// -- a key with an invalid point fails here, as the precompiles would reject it --, program_vkey < R (groth16.rs:32), the hash of the
// public values & (2^253 - 1) (types.rs:34-38; below R, so it has no range check of its own to fail), the point encodings.
// vkey: the 32 bytes of the program vkey, 4-byte aligned (the gateway's compact copy).
ZKV_HD void gwset_prep_slot(uint32_t vk_valid, uint32_t len, const uint32_t* vkey, const uint8_t* pv, size_t pv_len, const GwsetRec& rec, GwsetSlot& r) {
    r.flags = 0;
#pragma unroll
    for (int k = 0; k < 8; k++) { r.sig[0][k] = 0; r.sig[1][k] = 0; }
    if (len != 260) { r.status = ST_INVALID_PROOF_DATA; return; }
    r.status = ST_VERIFICATION_FAILED;
    if (!vk_valid) return;
#pragma unroll
    for (int j = 0; j < 8; j++) r.sig[0][7 - j] = __builtin_bswap32(vkey[j]);       // U256::from_be_bytes(program_vkey)
    if (!raw_lt_r(r.sig[0])) return;
    uint32_t h[8];
    sha256_bytes(pv, pv_len, h);
    h[0] &= 0x1fffffffu;
#pragma unroll
    for (int j = 0; j < 8; j++) r.sig[1][7 - j] = h[j];
    uint32_t w[8][8];
#pragma unroll 1
    for (int j = 0; j < 8; j++) rec.u256(w[j], 1 + 8 * j);
    if (prep_points(w, false, r.o)) r.flags = r.o.flags;
}

// The key (route of the group) of group slot j: the last key whose group starts at or before it -- an empty key starts where the next
// one does, and a pad slot belongs to the key whose group it pads.  start: n_keys first slots (zkv_gset_layout.h gset_layout).
ZKV_HD uint32_t gwset_key_of_slot(const uint32_t* start, uint32_t n_keys, uint32_t j) {
    uint32_t k = 0;
    for (uint32_t q = 1; q < n_keys; q++) if (start[q] <= j) k = q;
    return k;
}
// With the aggregate check on the group (zkv_gset_layout.h route_layout_agg) the group has two regions, each with one start per key:
// group slots below agg_r are the aggregate region (astart), the others the per-proof region (start).  The region is taken from
// wave_slot, the first slot of the lane's 64-slot PREP block: agg_r and every chunk's first slot are multiples of 64, so a block lies in
// one region and the choice between the two start rows stays wave-uniform.  agg_r = 0: gwset_key_of_slot over start.
ZKV_HD uint32_t gwset_key_of_slot2(const uint32_t* astart, const uint32_t* start, uint32_t n_keys, uint32_t agg_r, uint32_t wave_slot, uint32_t j) {
    return gwset_key_of_slot(wave_slot < agg_r ? astart : start, n_keys, j);
}

#if defined(__HIPCC__)
// The PREP kernel of a keyed group (k_gwset_prep, k_rzrouter_prep), one slot per lane: everything around the unit's slot function.
// Records are 260-byte rows from a 4-byte aligned base (the caller's own allocation; every record before the group's is a multiple of 4
// bytes), so the 64 rows of a wavefront are 16,640 contiguous bytes: copied to LDS with coalesced dword loads, every lane then reads its
// own 65 words (row stride 65 dwords: conflict-free), as k_prep_sp1 stages fixed-stride seals.  The address test is wave-uniform; a base
// that fails it is read byte by byte.  Then the key of the slot (skey, for k_gset_msm / k_gset_miller; two regions when the group takes
// the aggregate check: gwset_key_of_slot2), and for a live slot
// slot_fn(chunk, key, slot, record, r) -- the unit's checks, filling a Slot with NSIG signals --, the signals staged as GsetChunk::sig, the
// points where k_gset_msm reads them, flags, status and the (zero) received selector.  Chunk: GwsetChunk or RzrChunk (zkv_internal.h);
// lds: ZKV_BLOCK * 65 words of the kernel's.
// A chunk of the aggregate region is left as k_gset_prep leaves one for k_agg_g1 and the k_gset_agg_* kernels: rows and flags of the live
// slots, g2bad cleared, the signals staged (below r, or the slot is off), every slot's key; a slot the front checks fail is switched off
// (flags 0) and keeps the status written here, which k_gset_agg_mark leaves alone.
template <int NSIG, class Slot, class Chunk, class F>
__device__ __forceinline__ void gwset_prep_lane(const Chunk& c, const Workspace& ws, uint32_t* lds, F slot_fn) {
    const size_t b0 = (size_t)blockIdx.x * ZKV_BLOCK;
    const uint8_t* rows = c.recs + (c.slot0 + b0) * 260;
    const bool staged = !((uintptr_t)c.recs & 3u);
    if (staged) {
        const size_t mm = c.m - b0 < ZKV_BLOCK ? c.m - b0 : ZKV_BLOCK;
        const uint32_t* src = (const uint32_t*)rows;
        const uint32_t total = (uint32_t)mm * 65u;
#pragma unroll 1
        for (uint32_t t = threadIdx.x; t < total; t += ZKV_BLOCK) lds[t] = src[t];
        __syncthreads();
    }
    const size_t j = b0 + threadIdx.x;
    if (j >= c.m) return;
    const size_t slot = c.slot0 + j;
    const uint32_t k = gwset_key_of_slot2(c.astart, c.start, c.n_keys, c.agg_r, (uint32_t)(c.slot0 + b0), (uint32_t)slot);
    c.skey[slot] = k;
    const uint32_t i = c.idx[slot];
    uint32_t flags = 0;
    uint8_t st = ST_VERIFICATION_FAILED;
    if (i != GW_NONE) {                                             // (a pad slot carries nothing: every stage skips it)
        GwsetRec rd;
        rd.row = staged ? lds + threadIdx.x * 65u : nullptr;
        rd.rec = rows + (size_t)threadIdx.x * 260;
        Slot r;
        slot_fn(c, k, slot, rd, r);
#pragma unroll
        for (int b = 0; b < NSIG; b++) {
#pragma unroll
            for (int q = 0; q < 8; q++) c.sig[(size_t)(8 * b + q) * c.sig_cap + j] = r.sig[b][q];
        }
        if (r.flags & FL_ALIVE) {
            ws_st(ws.prep, ws.cap, 0, j, r.o.ax); ws_st(ws.prep, ws.cap, 8, j, r.o.ay);
            ws_st(ws.prep, ws.cap, 16, j, r.o.cx); ws_st(ws.prep, ws.cap, 24, j, r.o.cy);
            ws_st(ws.prep, ws.cap, 32, j, r.o.bx.c0); ws_st(ws.prep, ws.cap, 40, j, r.o.bx.c1);
            ws_st(ws.prep, ws.cap, 48, j, r.o.by.c0); ws_st(ws.prep, ws.cap, 56, j, r.o.by.c1);
        }
        flags = r.flags; st = r.status;
    }
    ws.flags[j] = flags;
    ws.g2bad[j] = 0;
    c.status[slot] = st;
    c.recv[slot] = 0;                                               // the route has the selector: nothing received to report
}
#endif

}  // namespace zkv

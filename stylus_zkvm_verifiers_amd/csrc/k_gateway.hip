// SP1 gateway (include/zkv_sp1_gateway.h): every proof of a batch goes to the route -- the SP1 Groth16 verifier or an SP1 PLONK
// verifier -- whose 4-byte selector begins it, as SP1's on-chain gateway forwards `verify_proof` by the selector.  No reference
// counterpart (parity unpinned); the routes' own statuses are their contexts' ones.
//
// The shape of the mixed-batch demultiplexer (k_mixed.hip), with up to 8 route columns and ragged proofs.  The column counts, the slot
// of a proof, the in-place answers and the record copy are the selector routers' shared skeleton (zkv_demux.h, also under
// k_risc0_router.hip); this unit's own are the spans and the classifier, the public-values locations, the per-route record size and
// the scan:
//   k_gateway_count   per 256-proof block: proofs per route, not found, short, bad calldata (wave ballots + popcounts)
//   k_gateway_scan    exclusive scan of every column over the blocks (one workgroup), totals
//   (the host reads the totals back once and sizes the compact records: route r holds n_r records of 260 or 868 bytes)
//   k_gateway_place   stable partition: slot of every routed proof; short and not-found proofs are answered in place
//   k_gateway_gather  one wavefront per proof: first min(len, record) proof bytes, the 32-byte program vkey; the true length and
//                     the public-values location were written by place
// Proofs arrive as n + 1 contiguous offsets or, from the calldata decoder (k_wire_gateway), as (start, length) records with gaps.
// The statuses come back through k_mixed_return.  All of it is byte traffic beside the pairing; no scratch, no LDS beyond the counts.
#include "zkv_demux.h"

namespace zkv {

constexpr int GW_BLOCK = 256;

// Proof i as (start, length) from a.proofs: a record (k_wire_gateway has bounded it) or the caller's two offsets; false: the offsets run
// backwards or past proof_bytes, the proof is never read.
__device__ __forceinline__ bool gw_span(const GatewayArgs& a, size_t i, uint64_t* start, uint64_t* len) {
    if (a.rec_proof_at) { *start = a.rec_proof_at[i]; *len = a.rec_proof_len[i]; return true; }
    const uint64_t s = a.proof_off[i], e = a.proof_off[i + 1];
    *start = s; *len = e - s;
    return s <= e && e <= a.proof_bytes;
}

// route of proof i (0 .. n_routes - 1), GW_COL_NOT_FOUND, GW_COL_SHORT or (records) GW_COL_BAD; *sel = the selector read (0 when short or
// bad).  Byte loads: a ragged blob has no alignment.
__device__ __forceinline__ int gw_class(const GatewayArgs& a, size_t i, uint32_t* sel) {
    *sel = 0;
    if (a.rec_bad && a.rec_bad[i]) return GW_COL_BAD;
    uint64_t s, len;
    if (!gw_span(a, i, &s, &len) || len < 4) return GW_COL_SHORT;
    const uint8_t* p = a.proofs + s;
    const uint32_t v = ((uint32_t)p[0] << 24) | ((uint32_t)p[1] << 16) | ((uint32_t)p[2] << 8) | p[3];
    *sel = v;
#pragma unroll
    for (int r = 0; r < GW_MAX_ROUTES; r++)
        if ((uint32_t)r < a.n_routes && v == a.sel[r]) return r;
    return GW_COL_NOT_FOUND;
}

__global__ __launch_bounds__(GW_BLOCK) void k_gateway_count(GatewayArgs a) {
    __shared__ uint32_t wc[GW_COLS][GW_BLOCK / 64];
    const size_t i = (size_t)blockIdx.x * GW_BLOCK + threadIdx.x;
    uint32_t sel;
    demux_ballots(i < a.n ? gw_class(a, i, &sel) : -1, wc);
    __syncthreads();
    demux_block_counts(wc, a.cnt);
}

// cnt[b * GW_COLS + k] -> exclusive prefix sums over b in place, per column k; totals[k].  One workgroup.
__global__ __launch_bounds__(1024) void k_gateway_scan(uint32_t blocks, uint32_t* __restrict__ cnt, uint32_t* __restrict__ totals) {
    __shared__ uint32_t part[GW_COLS][1024];
    const uint32_t t = threadIdx.x, per = (blocks + 1023u) / 1024u, lo = t * per, hi = lo + per < blocks ? lo + per : blocks;
    uint32_t s[GW_COLS];
#pragma unroll
    for (int k = 0; k < GW_COLS; k++) s[k] = 0;
    for (uint32_t b = lo; b < hi; b++) {
#pragma unroll
        for (int k = 0; k < GW_COLS; k++) s[k] += cnt[(size_t)b * GW_COLS + k];
    }
#pragma unroll
    for (int k = 0; k < GW_COLS; k++) part[k][t] = s[k];
    __syncthreads();
    for (uint32_t d = 1; d < 1024; d <<= 1) {                       // Hillis-Steele inclusive scan of the 1024 partial sums, every column
        uint32_t v[GW_COLS];
#pragma unroll
        for (int k = 0; k < GW_COLS; k++) v[k] = t >= d ? part[k][t - d] : 0;
        __syncthreads();
#pragma unroll
        for (int k = 0; k < GW_COLS; k++) part[k][t] += v[k];
        __syncthreads();
    }
    uint32_t e[GW_COLS];
#pragma unroll
    for (int k = 0; k < GW_COLS; k++) e[k] = part[k][t] - s[k];
    for (uint32_t b = lo; b < hi; b++) {
#pragma unroll
        for (int k = 0; k < GW_COLS; k++) { const uint32_t c = cnt[(size_t)b * GW_COLS + k]; cnt[(size_t)b * GW_COLS + k] = e[k]; e[k] += c; }
    }
    if (t == 1023) {
#pragma unroll
        for (int k = 0; k < GW_COLS; k++) totals[k] = part[k][1023];
    }
}

__global__ __launch_bounds__(GW_BLOCK) void k_gateway_place(GatewayArgs a) {
    __shared__ uint32_t wc[GW_MAX_ROUTES][GW_BLOCK / 64];
    const size_t i = (size_t)blockIdx.x * GW_BLOCK + threadIdx.x;
    uint32_t sel = 0;
    const int c = i < a.n ? gw_class(a, i, &sel) : -1;
    const uint64_t mine = demux_ballots(c, wc);
    __syncthreads();
    if (c < 0) return;
    if (c >= GW_MAX_ROUTES) {                                       // ZKV_STATUS_INVALID_PROOF_DATA, _BAD_CALLDATA, _ROUTE_NOT_FOUND
        demux_answer(i, c == GW_COL_SHORT ? 4 : c == GW_COL_BAD ? 6 : 8, sel, a.pos, a.status, a.recv);
        return;
    }
    const uint32_t slot = demux_slot<GW_COLS>(c, mine, wc, a.start, a.agg, a.astart, a.cnt);
    a.pos[i] = slot;
    a.idx[slot] = (uint32_t)i;
    uint64_t at, len;
    gw_span(a, i, &at, &len);
    a.c_len[slot] = demux_len32(len);
    if (a.rec_proof_at) { a.c_pvoff[slot] = a.rec_pv_at[i]; a.c_pvlen[slot] = a.rec_pv_len[i]; return; }
    a.c_pvoff[slot] = a.pv_off ? a.pv_off[i] : (uint64_t)i * a.pv_stride;
    a.c_pvlen[slot] = (uint32_t)(a.pv_off ? a.pv_off[i + 1] - a.pv_off[i] : a.pv_stride);
}

// One wavefront per proof (four per workgroup): the route's record stride decides how many words the lanes copy (65 or 217).
__global__ __launch_bounds__(GW_BLOCK) void k_gateway_gather(GatewayArgs a) {
    const size_t i = (size_t)blockIdx.x * (GW_BLOCK / 64) + (threadIdx.x >> 6);
    const uint32_t lane = threadIdx.x & 63u;
    if (i >= a.n) return;
    const uint32_t slot = a.pos[i];
    if (slot == GW_NONE) return;
    // a slot of the keyed group: the group-relative 260-byte row, in either of its regions.  Otherwise the route of the slot: the last
    // route starting at or before it (an empty route starts where the next one does; a keyed route's start lies inside the group)
    uint32_t rec = 260;
    uint32_t* dst;
    if (slot - a.g0 < a.gm) dst = (uint32_t*)(a.c_proofs + a.gb0 + (uint64_t)(slot - a.g0) * 260);
    else {
        uint32_t r = 0;
#pragma unroll
        for (int k = 1; k < GW_MAX_ROUTES; k++) if ((uint32_t)k < a.n_routes && a.start[k] <= slot) r = (uint32_t)k;
        rec = a.rec[r];
        dst = (uint32_t*)(a.c_proofs + a.base[r] + (uint64_t)(slot - a.start[r]) * rec);
    }
    uint64_t at, len;
    gw_span(a, i, &at, &len);
    demux_copy_record(dst, a.proofs + at, len, rec, lane);
    if (lane < 8) ((uint32_t*)a.c_a)[(size_t)slot * 8 + lane] = gw_ld4(a.vkeys + 32 * i + 4 * lane, 4);
}

void launch_gateway_count(const GatewayArgs& a, hipStream_t s) {
    if (!a.n) return;
    const unsigned blocks = (unsigned)((a.n + GW_BLOCK - 1) / GW_BLOCK);
    hipLaunchKernelGGL(k_gateway_count, dim3(blocks), dim3(GW_BLOCK), 0, s, a);
    hipLaunchKernelGGL(k_gateway_scan, dim3(1), dim3(1024), 0, s, blocks, a.cnt, a.totals);
}
void launch_gateway_place(const GatewayArgs& a, hipStream_t s) {
    if (!a.n) return;
    const unsigned blocks = (unsigned)((a.n + GW_BLOCK - 1) / GW_BLOCK);
    hipLaunchKernelGGL(k_gateway_place, dim3(blocks), dim3(GW_BLOCK), 0, s, a);
    const size_t per = GW_BLOCK / 64;
    hipLaunchKernelGGL(k_gateway_gather, dim3((unsigned)((a.n + per - 1) / per)), dim3(GW_BLOCK), 0, s, a);
}

}  // namespace zkv

// SP1 gateway, Groth16 routes with caller-supplied keys (include/zkv_sp1_gateway_keys.h).  The keyed routes of a
// gateway are one Groth16 key set (n_ic = 3, SP1 sign convention); the demultiplexer (k_gateway.hip) has sorted their proofs into the
// set's slot layout (zkv_gset_layout.h: every route starts on a multiple of the proofs per wavefront of the Miller mapping).  This unit
// is the stage between the two: the SP1 front end of k_prep_sp1 per slot with the slot's key, one slot per lane.  It stages the two
// signals where k_gset_msm reads them and writes each slot's key for k_gset_msm / k_gset_miller; the remaining stages are the key sets'.
// Parity unpinned, except that a route holding the reference's own key and hash gives the pinned SP1 statuses.
#include "zkv_internal.h"
#include "zkv_gwset_prep.h"

namespace zkv {

// Records are 260-byte rows from a 4-byte aligned base (the gateway's own allocation; every route's records before the group's are a
// multiple of 4 bytes), so the 64 rows of a wavefront are 16,640 contiguous bytes: copied to LDS with coalesced dword loads, every lane
// then reads its own 65 words (row stride 65 dwords: conflict-free), as k_prep_sp1 stages fixed-stride seals.  The address test is
// wave-uniform; a base that fails it is read byte by byte.
__global__ __launch_bounds__(ZKV_BLOCK) void k_gwset_prep(GwsetChunk c, Workspace ws) {
    __shared__ uint32_t lds[ZKV_BLOCK * 65];
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
    const uint32_t k = gwset_key_of_slot(c.start, c.n_keys, (uint32_t)slot);
    c.skey[slot] = k;
    const uint32_t i = c.idx[slot];
    uint32_t flags = 0;
    uint8_t st = ST_VERIFICATION_FAILED;
    if (i != GW_NONE) {                                             // (a pad slot carries no proof: every stage skips it)
        GwsetRec rd;
        rd.row = staged ? lds + threadIdx.x * 65u : nullptr;
        rd.rec = rows + (size_t)threadIdx.x * 260;
        GwsetSlot r;
        gwset_prep_slot(c.keys[k].tab->vk_valid, c.len[slot], (const uint32_t*)(c.vkeys + 32 * slot), c.pv + c.pvoff[slot], c.pvlen[slot], rd, r);
#pragma unroll
        for (int b = 0; b < 2; b++) {
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
    c.recv[slot] = 0;                                               // the route has the proof's selector: nothing received to report
}
void launch_gwset_prep(const GwsetChunk& c, const Workspace& ws, hipStream_t s) {
    if (!c.m) return;
    hipLaunchKernelGGL(k_gwset_prep, dim3((unsigned)((c.m + ZKV_BLOCK - 1) / ZKV_BLOCK)), dim3(ZKV_BLOCK), 0, s, c, ws);
}

}  // namespace zkv

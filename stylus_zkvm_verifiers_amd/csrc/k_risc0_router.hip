// RISC Zero router (include/zkv_risc0_router.h): every seal of a batch goes to the route -- a built-in-key
// verifier or a verifier with a caller's key -- whose 4-byte selector begins it, as RISC Zero's on-chain router forwards `verify` and
// `verifyIntegrity`.  No reference counterpart (parity unpinned); the routes' own statuses are their verifiers' ones.
//
// Up to 32 selectors and two groups of routes.  The column counts, the slot of a seal, the in-place answers and the record copy are the
// selector routers' shared skeleton (zkv_demux.h, also under k_gateway.hip), the keyed group's PREP kernel is the shared body of
// zkv_gwset_prep.h around rzrouter_prep_slot; this unit's own are the spans and the classifier, the instance of a built-in seal and
// the per-built-in-route counters:
//   k_rzrouter_count   per 256-seal block: seals of the built-in group (all built-in routes together), per keyed route, unknown, short;
//                      and the seals of every built-in route, added to one counter per route (the call's per-route totals), and the
//                      bad-calldata seals (they sit in the short column), added to one counter more
//   k_gateway_scan     (k_gateway.hip, same column count) exclusive scan of every column over the blocks, totals
//   (the host reads the totals back once and lays the slots out: the built-in group first, then the keyed routes padded as a key set)
//   k_rzrouter_place   stable partition: slot of every routed seal; short and unknown seals are answered in place.  A seal of the
//                      built-in group also gets the instance it matched -- the row the verifier-set pipeline takes from its caller --,
//                      and every slot its seal's method byte when the call has a method row
//   k_rzrouter_gather  one wavefront per seal: first min(len, 260) seal bytes and the two 32-byte inputs to the slot's compact record
//   k_rzrouter_prep    the keyed group's PREP, one slot per lane (zkv_rzrouter_prep.h), in front of the key sets' stages
// The built-in group then runs the verifier set's own pipeline on its compact records, the statuses come back through k_mixed_return.
#include "zkv_demux.h"
#include "zkv_rzrouter_prep.h"

namespace zkv {

static_assert(RZR_COLS == GW_COLS, "k_gateway_scan scans GW_COLS columns");
static_assert(RZR_MAX_KEYED == GW_MAX_ROUTES, "RzrChunk::start holds one first slot per keyed route");
__global__ void k_gateway_scan(uint32_t blocks, uint32_t* __restrict__ cnt, uint32_t* __restrict__ totals);      // k_gateway.hip

constexpr int RZR_BLOCK = 256;
constexpr int RZR_ROUTED = RZR_COL_KEYED0 + RZR_MAX_KEYED;      // columns that take slots

// Seal i as (start, length); false: the offsets run backwards or past seal_bytes, the seal is never read.  With a true-length row the
// length may exceed the stride: the slot then holds the seal's first `stride` bytes, and every reader stops there (no route reads more).
__device__ __forceinline__ bool rzr_span(const RzrArgs& a, size_t i, uint64_t* start, uint64_t* len) {
    if (!a.seal_off) { *start = (uint64_t)i * a.stride; *len = a.wire_len ? a.wire_len[i] : a.stride; return true; }
    const uint64_t s = a.seal_off[i], e = a.seal_off[i + 1];
    *start = s; *len = e - s;
    return s <= e && e <= a.seal_bytes;
}
// Column of seal i (zkv_rzrouter_prep.h), *sel = the selector read (0 when short), *inst = the built-in route it matched.  The selector is
// one dword load when every seal starts 4-byte aligned (a wave-uniform test: fixed stride from an aligned base), byte loads otherwise: a
// ragged blob has no alignment.  Only these 4 bytes of a seal are read here, so the seals are not staged in LDS; the gather and the two
// PREP kernels read whole seals, coalesced.
// *bad: the seal is bad calldata -- a method byte above ZKV_METHOD_VERIFY_INTEGRITY, or a request the wire stage could not decode; it
// shares the short column (answered in place, zero selector) and is counted beside it.
__device__ __forceinline__ int rzr_class(const RzrArgs& a, size_t i, uint32_t* sel, uint32_t* inst, bool* bad) {
    *sel = 0; *inst = 0;
    *bad = (a.method && a.method[i] > 1) || (a.wire_len && a.wire_len[i] == 0xFFFFFFFFu);
    if (*bad) return RZR_COL_SHORT;
    uint64_t s, len;
    if (!rzr_span(a, i, &s, &len) || len < 4) return RZR_COL_SHORT;
    const uint8_t* p = a.seals + s;
    uint32_t v;
    if (!a.seal_off && !(((uintptr_t)a.seals | a.stride) & 3u)) v = __builtin_bswap32(*(const uint32_t*)p);
    else v = ((uint32_t)p[0] << 24) | ((uint32_t)p[1] << 16) | ((uint32_t)p[2] << 8) | p[3];
    *sel = v;
    return rzrouter_column(a.sel, a.n_builtin, a.n_keyed, v, inst);
}

__global__ __launch_bounds__(RZR_BLOCK) void k_rzrouter_count(RzrArgs a) {
    __shared__ uint32_t wc[RZR_COLS][RZR_BLOCK / 64];
    const size_t i = (size_t)blockIdx.x * RZR_BLOCK + threadIdx.x;
    uint32_t sel = 0, inst = 0;
    bool bad = false;
    const int c = i < a.n ? rzr_class(a, i, &sel, &inst, &bad) : -1;
    demux_ballots(c, wc);
    const uint64_t mb = __ballot(bad);
    if ((threadIdx.x & 63u) == 0 && mb) atomicAdd(&a.inst_tot[RZR_BAD_WORD], (uint32_t)__popcll(mb));
    // per built-in route: one atomic per wavefront and route that has seals (the slots do not depend on these, only the reported counts)
#pragma unroll 1
    for (uint32_t r = 0; r < a.n_builtin; r++) {
        const uint64_t m = __ballot(c == RZR_COL_BUILTIN && inst == r);
        if ((threadIdx.x & 63u) == 0 && m) atomicAdd(&a.inst_tot[r], (uint32_t)__popcll(m));
    }
    __syncthreads();
    demux_block_counts(wc, a.cnt);
}

__global__ __launch_bounds__(RZR_BLOCK) void k_rzrouter_place(RzrArgs a) {
    __shared__ uint32_t wc[RZR_ROUTED][RZR_BLOCK / 64];
    const size_t i = (size_t)blockIdx.x * RZR_BLOCK + threadIdx.x;
    uint32_t sel = 0, inst = 0;
    bool bad = false;
    const int c = i < a.n ? rzr_class(a, i, &sel, &inst, &bad) : -1;
    const uint64_t mine = demux_ballots(c, wc);
    __syncthreads();
    if (c < 0) return;
    if (c >= RZR_ROUTED) {                                          // ZKV_STATUS_BAD_CALLDATA, ZKV_STATUS_INVALID_PROOF_DATA, ZKV_STATUS_ROUTE_NOT_FOUND
        demux_answer(i, bad ? 6 : c == RZR_COL_SHORT ? 4 : 8, sel, a.pos, a.status, a.recv);
        return;
    }
    const uint32_t slot = demux_slot<RZR_COLS>(c, mine, wc, a.start, a.agg, a.astart, a.cnt);
    a.pos[i] = slot;
    a.idx[slot] = (uint32_t)i;
    uint64_t at, len;
    rzr_span(a, i, &at, &len);
    a.c_len[slot] = demux_len32(len);
    if (a.method) a.c_kind[slot] = a.method[i];
    if (c == RZR_COL_BUILTIN) a.c_inst[slot] = inst;
}

// One wavefront per seal (four per workgroup): 65 record words, then 8 words of in_a and (verify) 8 of in_b.
__global__ __launch_bounds__(RZR_BLOCK) void k_rzrouter_gather(RzrArgs a) {
    const size_t i = (size_t)blockIdx.x * (RZR_BLOCK / 64) + (threadIdx.x >> 6);
    const uint32_t lane = threadIdx.x & 63u;
    if (i >= a.n) return;
    const uint32_t slot = a.pos[i];
    if (slot == GW_NONE) return;
    uint32_t* dst = (uint32_t*)(a.c_seals + (uint64_t)slot * 260);
    uint64_t at, len;
    rzr_span(a, i, &at, &len);
    demux_copy_record(dst, a.seals + at, len, 260, lane);
    if (lane < 8) ((uint32_t*)a.c_a)[(size_t)slot * 8 + lane] = gw_ld4(a.in_a + 32 * i + 4 * lane, 4);
    else if (lane < 16 && a.in_b) ((uint32_t*)a.c_b)[(size_t)slot * 8 + (lane - 8)] = gw_ld4(a.in_b + 32 * i + 4 * (lane - 8), 4);
}

void launch_rzrouter_count(const RzrArgs& a, hipStream_t s) {
    if (!a.n) return;
    const unsigned blocks = (unsigned)((a.n + RZR_BLOCK - 1) / RZR_BLOCK);
    hipLaunchKernelGGL(k_rzrouter_count, dim3(blocks), dim3(RZR_BLOCK), 0, s, a);
    hipLaunchKernelGGL(k_gateway_scan, dim3(1), dim3(1024), 0, s, blocks, a.cnt, a.totals);
}
void launch_rzrouter_place(const RzrArgs& a, hipStream_t s) {
    if (!a.n) return;
    const unsigned blocks = (unsigned)((a.n + RZR_BLOCK - 1) / RZR_BLOCK);
    hipLaunchKernelGGL(k_rzrouter_place, dim3(blocks), dim3(RZR_BLOCK), 0, s, a);
    const size_t per = RZR_BLOCK / 64;
    hipLaunchKernelGGL(k_rzrouter_gather, dim3((unsigned)((a.n + per - 1) / per)), dim3(RZR_BLOCK), 0, s, a);
}

// Keyed group: the shared PREP body (zkv_gwset_prep.h) around the router's slot function.
__global__ __launch_bounds__(ZKV_BLOCK) void k_rzrouter_prep(RzrChunk c, Risc0Consts kc, Workspace ws) {
    __shared__ uint32_t lds[ZKV_BLOCK * 65];
    // (kc is a kernel argument taken by reference: the lambda must stay always_inline, so that the reference folds away and kc stays in SGPRs)
    gwset_prep_lane<5, RzrSlot>(c, ws, lds, [&kc](const RzrChunk& ch, uint32_t k, size_t slot, const GwsetRec& rd, RzrSlot& r) __attribute__((always_inline)) {
        rzrouter_prep_slot(ch.keys[k].tab->vk_valid, ch.routes[k], kc, ch.len[slot], ch.in_a + 32 * slot, rzrouter_slot_in_b(ch.kind, ch.in_b, slot), rd, r);
    });
}
void launch_rzrouter_prep(const RzrChunk& c, const Risc0Consts& k, const Workspace& ws, hipStream_t s) {
    if (!c.m) return;
    hipLaunchKernelGGL(k_rzrouter_prep, dim3((unsigned)((c.m + ZKV_BLOCK - 1) / ZKV_BLOCK)), dim3(ZKV_BLOCK), 0, s, c, k, ws);
}

}  // namespace zkv

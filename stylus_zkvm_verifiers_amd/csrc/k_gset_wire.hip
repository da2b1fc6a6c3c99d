// eth_call batches on a set of deployed Groth16 verifier contracts (include/zkv_groth16_set_wire.h): the front and
// the back of the key-set pipeline, which runs unchanged between them.
//
//   k_gset_wire_decode  one request per lane (zkv_wire_gset.h, the functions the host simulation runs): offsets, the address among the
//                       set's sorted addresses by binary search (at most 10 steps over 32-byte entries: the table of 1,024 contracts is
//                       32 KB and stays in L2), selector and length.  Then the wavefront copies the words of its calls one call after
//                       the other, a dword per lane -- the 256 proof bytes and the N signal words into the rows k_gset_prep reads, with
//                       the test "a signal word >= r" on the way (eight lanes hold one word; two ballots per step).  A lane copying
//                       its own request alone reads with a stride of the request's length: 112 GB/s on 129-IC calls, 7 % of the call
//                       (profiles/groth16_set_wire_ab.txt).  Calldata words sit 4 bytes behind the request's start: whole dwords when
//                       that address is 4-byte aligned, bytes otherwise.
//   k_gset_wire_return  one request per lane: decode verdict, in-field byte and verified byte into the status byte; the four totals by
//                       one ballot per wavefront and one atomic add per non-zero total.
#include "zkv_internal.h"
#include "zkv_wire_gset.h"
#include "../../include/zkv_groth16_set_wire.h"

namespace zkv {

static_assert(GSW_BAD_CALLDATA == ZKV_STATUS_BAD_CALLDATA && GSW_NO_CONTRACT == ZKV_STATUS_NO_CONTRACT, "decode verdicts are status bytes");
constexpr int GSW_BLOCK = 256;

__global__ __launch_bounds__(GSW_BLOCK) void k_gset_wire_decode(GswArgs a) {
    const size_t i = (size_t)blockIdx.x * GSW_BLOCK + threadIdx.x;
    const uint32_t lane = threadIdx.x & 63u;
    const size_t i0 = i - lane;                           // the wavefront's first request
    const bool live = i < a.n;
    GswCall c = {GSW_BAD_CALLDATA, GSW_NONE, 0, 0};
    if (live) c = gsw_resolve(a, i);
    uint32_t big = 0;
    unsigned long long calls = __ballot(live && c.verdict == GSW_CALL);
    while (calls) {                                       // wave-uniform: the calls of the wavefront, one after the other, a dword per lane
        const int j = __ffsll(calls) - 1;
        calls &= calls - 1;
        const uint64_t at = ((uint64_t)(uint32_t)__shfl((int)(c.at >> 32), j) << 32) | (uint32_t)__shfl((int)(uint32_t)c.at, j);
        const uint32_t n_dwords = 8u * (uint32_t)__shfl((int)c.n_sig, j);
        const uint8_t* src = a.cd + at + 4;               // (inside the blob: gsw_resolve saw the whole call there)
        const bool al = (((uintptr_t)src) & 3u) == 0;
        ((uint32_t*)(a.proofs + 256 * (i0 + j)))[lane] = gsw_ld4(src + 4 * lane, al);
        uint32_t* row = (uint32_t*)(a.rows + (size_t)a.sig_stride * (i0 + j));
        bool ge = false;
        for (uint32_t w0 = 0; w0 < n_dwords; w0 += 64) {
            const uint32_t cls = gsw_signal_dword(src + 256, al, row, w0 + lane, n_dwords);
            ge = gsw_any_ge_r(__ballot(cls == 2), __ballot(cls == 1)) || ge;
        }
        if (lane == (uint32_t)j && ge) big = 1;
    }
    if (live) gsw_finish(a, i, c, big);
}
void launch_gset_wire_decode(const GswArgs& a, hipStream_t s) {
    if (!a.n) return;
    hipLaunchKernelGGL(k_gset_wire_decode, dim3((unsigned)((a.n + GSW_BLOCK - 1) / GSW_BLOCK)), dim3(GSW_BLOCK), 0, s, a);
}

__global__ __launch_bounds__(GSW_BLOCK) void k_gset_wire_return(size_t n, const uint8_t* __restrict__ verdict, const uint8_t* __restrict__ ge_r,
                                                                const uint8_t* __restrict__ verified, uint8_t* __restrict__ status,
                                                                unsigned long long* __restrict__ counts) {
    const size_t i = (size_t)blockIdx.x * GSW_BLOCK + threadIdx.x;
    const bool live = i < n;
    uint32_t st = 0xFFu;                                  // (a lane past the batch: no status, no total)
    bool placed = false;
    if (live) {
        const uint32_t v = verdict[i];
        placed = v == GSW_CALL && !ge_r[i];
        st = v != GSW_CALL ? v : ge_r[i] ? (uint32_t)ZKV_STATUS_INPUT_NOT_IN_FIELD : verified[i] ? (uint32_t)ZKV_STATUS_OK : (uint32_t)ZKV_STATUS_VERIFICATION_FAILED;
        status[i] = (uint8_t)st;
    }
    const unsigned long long b0 = __ballot(placed), b1 = __ballot(st == ZKV_STATUS_NO_CONTRACT), b2 = __ballot(st == ZKV_STATUS_BAD_CALLDATA),
                             b3 = __ballot(st == ZKV_STATUS_INPUT_NOT_IN_FIELD);
    if ((threadIdx.x & 63u) == 0) {
        if (b0) atomicAdd(counts + 0, (unsigned long long)__popcll(b0));
        if (b1) atomicAdd(counts + 1, (unsigned long long)__popcll(b1));
        if (b2) atomicAdd(counts + 2, (unsigned long long)__popcll(b2));
        if (b3) atomicAdd(counts + 3, (unsigned long long)__popcll(b3));
    }
}
void launch_gset_wire_return(size_t n, const uint8_t* verdict, const uint8_t* ge_r, const uint8_t* verified, uint8_t* status,
                             unsigned long long* counts, hipStream_t s) {
    if (!n) return;
    hipLaunchKernelGGL(k_gset_wire_return, dim3((unsigned)((n + GSW_BLOCK - 1) / GSW_BLOCK)), dim3(GSW_BLOCK), 0, s, n, verdict, ge_r, verified, status, counts);
}

}  // namespace zkv

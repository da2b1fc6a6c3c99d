// eth_call batches on a set of deployed gnark PLONK verifier contracts (include/zkv_plonk_set_wire.h): the front
// and the back of the PLONK key-set pipeline, which runs unchanged between them.
//
//   k_pset_wire_decode  one request per lane (zkv_wire_pset.h, the functions the host simulation runs): offsets, the address among the
//                       set's sorted addresses by binary search (at most 8 steps over 32-byte entries), the canonical head of
//                       Verify(bytes,uint256[]) and the two length rules N' = nb and Lp = Lkey.  Then the wavefront copies the words of
//                       its calls one call after the other, a dword per lane (the finding of section 11d: a lane copying its own request
//                       alone reads with a stride of the request's length) -- the nb input words and the Lkey proof bytes into the rows
//                       k_pset_prep reads, zeros behind a short proof, with the tests "an input word >= r" and "an opening word >= r" on
//                       the way (eight lanes hold one word; two ballots per step).  Calldata words sit 4 bytes behind the request's
//                       start: whole dwords when that address is 4-byte aligned, bytes otherwise.
//   k_pset_wire_points  one (request, point) per lane over the copied rows: sixteen lanes per request, of which nine or ten test a point
//                       with plonk_g1 (coordinates < p, on the curve or (0, 0)); "bad" is a plain byte store into the request's row,
//                       and the request loses its key.
//   k_pset_wire_return  one request per lane: decode verdict, reason, point byte and verified byte into status and reason; the eight
//                       totals by one ballot per wavefront and one atomic add per non-zero total.
#include "zkv_internal.h"
#include "zkv_wire_pset.h"
#include "../../include/zkv_plonk_set_wire.h"

namespace zkv {

static_assert(PSW_BAD_CALLDATA == ZKV_STATUS_BAD_CALLDATA && PSW_NO_CONTRACT == ZKV_STATUS_NO_CONTRACT, "decode verdicts are status bytes");
static_assert(PSW_R_INPUT_COUNT == ZKV_PLONK_REVERT_INPUT_COUNT && PSW_R_INPUT_RANGE == ZKV_PLONK_REVERT_INPUT_RANGE &&
              PSW_R_PROOF_SIZE == ZKV_PLONK_REVERT_PROOF_SIZE && PSW_R_OPENING_RANGE == ZKV_PLONK_REVERT_OPENING_RANGE &&
              PSW_R_EC == ZKV_PLONK_REVERT_EC_OPERATION, "reasons are the header's");
constexpr int PSW_BLOCK = 256;
constexpr uint32_t PSW_POINT_LANES = 16;                  // lanes per request in k_pset_wire_points (PSW_MAX_POINTS of them work)

__global__ __launch_bounds__(PSW_BLOCK) void k_pset_wire_decode(PswArgs a) {
    const size_t i = (size_t)blockIdx.x * PSW_BLOCK + threadIdx.x;
    const uint32_t lane = threadIdx.x & 63u;
    const size_t i0 = i - lane;                           // the wavefront's first request
    const bool live = i < a.n;
    PswCall c = {PSW_BAD_CALLDATA, PSW_NONE, 0, 0, 0, 0, 0};
    if (live) c = psw_resolve(a, i);
    uint32_t in_ge = 0, op_ge = 0;
    const uint32_t row_dwords = a.proof_stride / 4;
    unsigned long long calls = __ballot(live && c.verdict == PSW_CALL && c.pre != PSW_R_INPUT_COUNT);
    while (calls) {                                       // wave-uniform: the calls of the wavefront, one after the other, a dword per lane
        const int j = __ffsll(calls) - 1;
        calls &= calls - 1;
        const uint64_t at = ((uint64_t)(uint32_t)__shfl((int)(c.at >> 32), j) << 32) | (uint32_t)__shfl((int)(uint32_t)c.at, j);
        const uint32_t nb = (uint32_t)__shfl((int)c.nb, j), n_c = (uint32_t)__shfl((int)c.n_c, j), lp = (uint32_t)__shfl((int)c.lp, j);
        const bool store = __shfl((int)c.pre, j) == (int)PSW_R_NONE;      // both length rules passed: the rows are written
        const uint8_t* cd = a.cd + at;                    // (inside the blob: psw_resolve saw the whole call there)
        const bool al = (((uintptr_t)cd) & 3u) == 0;
        const uint8_t* src = cd + PSW_HEAD + psw_pad32(lp) + 32;
        uint32_t* row = (uint32_t*)(a.rows + (size_t)a.input_stride * (i0 + j));
        const uint32_t n_dwords = 8u * nb;
        bool ge = false;
        for (uint32_t w0 = 0; w0 < n_dwords; w0 += 64) {
            const uint32_t cls = psw_input_dword(src, al, row, store, w0 + lane, n_dwords);
            ge = gsw_any_ge_r(__ballot(cls == 2), __ballot(cls == 1)) || ge;
        }
        if (lane == (uint32_t)j && ge) in_ge = 1;
        if (!store) continue;
        uint32_t* proof = (uint32_t*)(a.proofs + (size_t)a.proof_stride * (i0 + j));
        ge = false;
        for (uint32_t w0 = 0; w0 < row_dwords; w0 += 64) {
            const uint32_t cls = psw_proof_dword(cd + PSW_HEAD, al, proof, w0 + lane, n_c, row_dwords);
            if (w0 >= 64) ge = gsw_any_ge_r(__ballot(cls == 2), __ballot(cls == 1)) || ge;     // (no opening among words 0 .. 7)
        }
        if (lane == (uint32_t)j && ge) op_ge = 1;
    }
    if (live) psw_finish(a, i, c, psw_reason(c, in_ge != 0, op_ge != 0));
}
void launch_pset_wire_decode(const PswArgs& a, hipStream_t s) {
    if (!a.n) return;
    hipLaunchKernelGGL(k_pset_wire_decode, dim3((unsigned)((a.n + PSW_BLOCK - 1) / PSW_BLOCK)), dim3(PSW_BLOCK), 0, s, a);
}

__global__ __launch_bounds__(PSW_BLOCK) void k_pset_wire_points(PswArgs a) {
    const size_t t = (size_t)blockIdx.x * PSW_BLOCK + threadIdx.x;
    const size_t i = t / PSW_POINT_LANES;
    const uint32_t p = (uint32_t)(t % PSW_POINT_LANES);
    if (i < a.n && p < PSW_MAX_POINTS) psw_point(a, i, p);
}
void launch_pset_wire_points(const PswArgs& a, hipStream_t s) {
    if (!a.n) return;
    const size_t per = PSW_BLOCK / PSW_POINT_LANES;
    hipLaunchKernelGGL(k_pset_wire_points, dim3((unsigned)((a.n + per - 1) / per)), dim3(PSW_BLOCK), 0, s, a);
}

__global__ __launch_bounds__(PSW_BLOCK) void k_pset_wire_return(size_t n, const uint8_t* __restrict__ verdict, const uint8_t* __restrict__ reason_in,
                                                                const uint8_t* __restrict__ ec, const uint8_t* __restrict__ verified,
                                                                uint8_t* __restrict__ status, uint8_t* __restrict__ reason,
                                                                unsigned long long* __restrict__ counts) {
    const size_t i = (size_t)blockIdx.x * PSW_BLOCK + threadIdx.x;
    const bool live = i < n;
    uint32_t st = 0xFFu, rs = 0xFFu;                      // (a lane past the batch: no status, no total)
    bool placed = false;
    if (live) {
        const uint32_t v = verdict[i];
        rs = v != PSW_CALL ? PSW_R_NONE : reason_in[i] ? (uint32_t)reason_in[i] : ec[i] ? PSW_R_EC : PSW_R_NONE;
        placed = v == PSW_CALL && rs == PSW_R_NONE;
        st = v != PSW_CALL ? v : rs == PSW_R_INPUT_RANGE ? (uint32_t)ZKV_STATUS_INPUT_NOT_IN_FIELD : rs != PSW_R_NONE ? (uint32_t)ZKV_STATUS_INVALID_PROOF_DATA
           : verified[i] ? (uint32_t)ZKV_STATUS_OK : (uint32_t)ZKV_STATUS_VERIFICATION_FAILED;
        status[i] = (uint8_t)st;
        if (reason) reason[i] = (uint8_t)rs;
    }
    const unsigned long long b0 = __ballot(placed), b1 = __ballot(st == ZKV_STATUS_NO_CONTRACT), b2 = __ballot(st == ZKV_STATUS_BAD_CALLDATA);
    if ((threadIdx.x & 63u) == 0) {
        if (b0) atomicAdd(counts + 0, (unsigned long long)__popcll(b0));
        if (b1) atomicAdd(counts + 1, (unsigned long long)__popcll(b1));
        if (b2) atomicAdd(counts + 2, (unsigned long long)__popcll(b2));
    }
#pragma unroll
    for (uint32_t r = 1; r <= 5; r++) {
        const unsigned long long b = __ballot(rs == r);
        if ((threadIdx.x & 63u) == 0 && b) atomicAdd(counts + 2 + r, (unsigned long long)__popcll(b));
    }
}
void launch_pset_wire_return(size_t n, const uint8_t* verdict, const uint8_t* reason_in, const uint8_t* ec, const uint8_t* verified, uint8_t* status,
                             uint8_t* reason, unsigned long long* counts, hipStream_t s) {
    if (!n) return;
    hipLaunchKernelGGL(k_pset_wire_return, dim3((unsigned)((n + PSW_BLOCK - 1) / PSW_BLOCK)), dim3(PSW_BLOCK), 0, s, n, verdict, reason_in, ec, verified, status,
                       reason, counts);
}

}  // namespace zkv

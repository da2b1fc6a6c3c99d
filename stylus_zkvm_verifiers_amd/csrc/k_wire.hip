// Stage WIRE: eth_call calldata -> fixed-stride verifier inputs.
//
// The deployed shells (examples/risc0-verifier/src/lib.rs, examples/sp1-verifier/src/lib.rs) receive `Vec<u8>` arguments as
// Solidity `uint8[]` (examples/risc0-verifier/examples/interact.rs:36, examples/sp1-verifier/examples/interact.rs:15): one
// 32-byte big-endian word per byte, so a 260-byte seal arrives as 8,452 bytes of calldata.  This stage is the only
// HBM-bound kernel of the library: one wavefront per request streams the calldata with 1 KiB-per-instruction coalesced
// loads, checks that it is the canonical ABI encoding (the router decodes with validation: any other byte string is
// rejected -- unpinned), and compacts the arrays to bytes.
#include "zkv_internal.h"
#include "zkv_bytes.h"
#include "zkv_wire_gateway.h"
#include "zkv_wire_rzrouter.h"

namespace zkv {

constexpr int WIRE_BLOCK = 256;                  // four requests per workgroup
constexpr uint32_t WIRE_BAD = 0xFFFFFFFFu;

// 16 bytes of calldata as four dwords in ABI (big-endian) significance order: w[3] holds the lowest-order bytes.
template <bool AL, bool NT = false>
__device__ __forceinline__ void wire_load16(const uint8_t* __restrict__ p, uint32_t w[4]) {
    if (AL) {
        const uint32_t* q = (const uint32_t*)p;
        if (NT) {
            w[0] = __builtin_nontemporal_load(q); w[1] = __builtin_nontemporal_load(q + 1); w[2] = __builtin_nontemporal_load(q + 2);
            w[3] = __builtin_bswap32(__builtin_nontemporal_load(q + 3));
        } else { w[0] = q[0]; w[1] = q[1]; w[2] = q[2]; w[3] = __builtin_bswap32(q[3]); }
    } else {
        w[0] = load_be32(p); w[1] = load_be32(p + 4); w[2] = load_be32(p + 8); w[3] = load_be32(p + 12);
    }
}

// Streams the `n_el` element words of one uint8[] starting at `el`: every lane pair takes one word (even lane the upper
// 16 bytes, odd lane the lower 16), so one wave-instruction reads 1 KiB of contiguous calldata; on 4-byte-aligned blobs
// eight such loads are issued back to back before any of them is consumed (8 KiB in flight per wave).  Writes the first
// min(n_el, cap) bytes to `dst`; returns false (wave-uniform) when an element is not a uint8.
template <bool AL, bool NT>
__device__ __forceinline__ bool wire_u8_array_t(const uint8_t* __restrict__ el, uint32_t n_el, uint8_t* __restrict__ dst, uint32_t cap, uint32_t lane) {
    const uint32_t half = lane & 1u;
    uint32_t bad = 0, k = lane >> 1;
#pragma unroll 1
    for (; AL && k + 32 * 7 < n_el; k += 32 * 8) {        // unaligned blobs take the one-word loop below only
        uint32_t w[8][4];
#pragma unroll
        for (int j = 0; j < 8; j++) wire_load16<AL, NT>(el + (size_t)32 * (k + 32 * j) + 16 * half, w[j]);
#pragma unroll
        for (int j = 0; j < 8; j++) {
            const uint32_t hi = w[j][0] | w[j][1] | w[j][2];
            if (half) {
                bad |= hi | (w[j][3] & ~0xFFu);
                if (k + 32 * j < cap) dst[k + 32 * j] = (uint8_t)w[j][3];
            } else bad |= hi | w[j][3];
        }
    }
#pragma unroll 1
    for (; k < n_el; k += 32) {
        uint32_t w[4];
        wire_load16<AL, NT>(el + (size_t)32 * k + 16 * half, w);
        const uint32_t hi = w[0] | w[1] | w[2];
        if (half) {
            bad |= hi | (w[3] & ~0xFFu);
            if (k < cap) dst[k] = (uint8_t)w[3];
        } else bad |= hi | w[3];
    }
    return __all(bad == 0) != 0;
}
template <bool NT>
__device__ __forceinline__ bool wire_u8_array(const uint8_t* el, uint32_t n_el, bool al, uint8_t* dst, uint32_t cap, uint32_t lane) {
    return al ? wire_u8_array_t<true, NT>(el, n_el, dst, cap, lane) : wire_u8_array_t<false, NT>(el, n_el, dst, cap, lane);
}

__device__ __forceinline__ void copy32(uint8_t* dst, const uint8_t* src, uint32_t lane) {
    if (lane < 32) dst[lane] = src[lane];
}

// verify(uint8[],bytes32,bytes32) = sel | 0x60 | image_id | journal_digest | L | L element words
// verifyIntegrity(uint8[],bytes32) = sel | 0x40 | claim_digest | L | L element words
template <int BLOCK, bool NT>
__global__ __launch_bounds__(BLOCK) void k_wire_risc0(WireArgs a) {
    const uint32_t lane = threadIdx.x & 63u;
    const size_t i = (size_t)blockIdx.x * (BLOCK / 64) + (threadIdx.x >> 6);
    if (i >= a.n) return;
    const uint64_t o0 = a.off[i], o1 = a.off[i + 1];
    const bool in_blob = o0 <= o1 && o1 <= a.cd_bytes;       // offsets come from the caller: never read outside the blob
    const uint8_t* cd = a.cd + (in_blob ? o0 : 0);
    const uint64_t len = in_blob ? o1 - o0 : 0;
    const bool al = (((uintptr_t)cd) & 3u) == 0;
    uint32_t L = WIRE_BAD, kind = 0;
    if (len >= 4) {
        uint32_t sel = load_be32(cd);
        kind = sel == a.sel_b_be ? 1u : 0u;
        const uint32_t nh = kind ? 2u : 3u;
        const uint8_t* args = cd + 4;
        if ((sel == a.sel_a_be || sel == a.sel_b_be) && len >= 4 + 32ull * nh + 32) {
            WordVal o = wire_word(args, al), n = wire_word(args + 32 * nh, al);
            if (o.small && o.v == 32 * nh && n.small && len == 4 + 32ull * nh + 32 + 32ull * n.v) {
                if (wire_u8_array<NT>(args + 32 * nh + 32, n.v, al, a.seals + i * 260, 260, lane)) L = n.v;
                copy32(a.in_a + 32 * i, args + 32, lane);
                if (!kind) copy32(a.in_b + 32 * i, args + 64, lane);
            }
        }
    }
    if (lane == 0) { a.seal_len[i] = L; a.kind[i] = (uint8_t)kind; }
}

// verifyProof(bytes32,uint8[],uint8[]) = sel | vkey | 0x60 | 0x80 + 32 Lpv | Lpv | Lpv words | Lproof | Lproof words
template <int BLOCK, bool NT>
__global__ __launch_bounds__(BLOCK) void k_wire_sp1(WireArgs a) {
    const uint32_t lane = threadIdx.x & 63u;
    const size_t i = (size_t)blockIdx.x * (BLOCK / 64) + (threadIdx.x >> 6);
    if (i >= a.n) return;
    const uint64_t o0 = a.off[i], o1 = a.off[i + 1];
    const bool in_blob = o0 <= o1 && o1 <= a.cd_bytes;       // offsets come from the caller: never read outside the blob
    const uint8_t* cd = a.cd + (in_blob ? o0 : 0);
    const uint64_t len = in_blob ? o1 - o0 : 0;
    const bool al = (((uintptr_t)cd) & 3u) == 0;
    uint32_t L = WIRE_BAD, lpv = 0;
    const uint64_t pv_at = in_blob ? o0 / 32 : 0; // decoded public values of request i: at most len / 32 bytes
    if (len >= 4 + 96 + 64 && load_be32(cd) == a.sel_a_be) {
        const uint8_t* args = cd + 4;
        WordVal o1 = wire_word(args + 32, al), o2 = wire_word(args + 64, al), n1 = wire_word(args + 96, al);
        if (o1.small && o1.v == 0x60 && n1.small && len >= 4 + 96 + 32 + 32ull * n1.v + 32 && o2.small && o2.v == 0x80ull + 32ull * n1.v) {
            const uint8_t* second = args + 128 + (size_t)32 * n1.v;
            WordVal n2 = wire_word(second, al);
            if (n2.small && len == 4 + 96 + 32 + 32ull * n1.v + 32 + 32ull * n2.v) {
                bool ok = wire_u8_array<NT>(args + 128, n1.v, al, a.pv + pv_at, n1.v, lane);
                ok = wire_u8_array<NT>(second + 32, n2.v, al, a.seals + i * 260, 260, lane) && ok;
                if (ok) { L = n2.v; lpv = n1.v; }
                copy32(a.in_a + 32 * i, args, lane);
            }
        }
    }
    if (lane == 0) { a.seal_len[i] = L; a.pv_off[i] = pv_at; a.pv_len[i] = lpv; }
}

// verifyProof to the SP1 gateway, either calldata form (zkv_wire_gateway.h): the record of request i instead of a fixed slot, since the
// proof may be an 868-byte PLONK one.  Form U streams both arrays as k_wire_sp1 does, into the arena at off[i] / 32: the decoded bytes of
// a request are fewer than a 32nd of its calldata, so requests whose calldata does not overlap do not meet there; the proof copy stops at
// `cap` bytes (the longest record any route reads), the length passed on is the true one.  Form B is already bytes: the wave checks the
// zero padding of both arguments (at most 31 bytes each, lanes 0-30 and 32-62) and the record points into the blob.
template <int BLOCK, bool NT>
__global__ __launch_bounds__(BLOCK) void k_wire_gateway(GwWireArgs a, uint32_t cap) {
    const uint32_t lane = threadIdx.x & 63u;
    const size_t i = (size_t)blockIdx.x * (BLOCK / 64) + (threadIdx.x >> 6);
    if (i >= a.n) return;
    const uint64_t o0 = a.off[i], o1 = a.off[i + 1];
    const bool in_blob = o0 <= o1 && o1 <= a.cd_bytes;       // offsets come from the caller: never read outside the blob
    const uint8_t* cd = a.cd + (in_blob ? o0 : 0);
    const uint64_t len = in_blob ? o1 - o0 : 0;
    const bool al = (((uintptr_t)cd) & 3u) == 0;
    const GwCall h = gww_parse(cd, len, al, a.sel_u_be, a.sel_b_be);     // wave-uniform
    bool ok = h.ok != 0;
    uint64_t pv_at = 0, proof_at = 0;
    if (ok && h.form == GWW_FORM_UINT8_ARRAY) {
        const uint64_t at = o0 / 32;
        uint8_t* dst = a.arena + at;
        ok = wire_u8_array<NT>(cd + h.pv_at, h.pv_len, al, dst, h.pv_len, lane);
        ok = wire_u8_array<NT>(cd + h.proof_at, h.proof_len, al, dst + h.pv_len, cap, lane) && ok;
        pv_at = a.arena_delta + at; proof_at = pv_at + h.pv_len;
    } else if (ok) {
        const uint32_t half = lane >> 5, k = lane & 31u;
        const uint64_t body = half ? h.proof_at : h.pv_at, used = half ? h.proof_len : h.pv_len;
        const uint32_t pad = (uint32_t)(-used & 31u);
        const uint32_t b = k < pad ? cd[body + used + k] : 0u;
        ok = __all(b == 0) != 0;
        pv_at = a.cd_delta + o0 + h.pv_at; proof_at = a.cd_delta + o0 + h.proof_at;
    }
    if (h.ok) copy32(a.vkeys + 32 * i, cd + 4, lane);
    if (lane == 0) {
        a.bad[i] = ok ? 0 : 1;
        a.pv_at[i] = ok ? pv_at : 0; a.pv_len[i] = ok ? h.pv_len : 0;
        a.proof_at[i] = ok ? proof_at : 0; a.proof_len[i] = ok ? h.proof_len : 0;
    }
}

// verify / verifyIntegrity to the RISC Zero router, the four call shapes of zkv_wire_rzrouter.h: the fixed 260-byte slot of request i
// (k_wire_risc0's output: no route reads more than 260 bytes, so a longer seal keeps only its true length) with its inputs and method.
// Form U streams the element words as k_wire_risc0 does.  Form B is already bytes: the wave copies the first min(L, 260) of them -- whole
// dwords when the request and the slots are 4-byte aligned (the body starts a multiple of 4 behind the request), bytes otherwise -- and
// checks the zero padding behind the seal's end, at most 31 bytes, one per lane.  Every position is bounded by rzw_parse: it demands the
// exact total length, and the request itself lies inside the blob.
template <int BLOCK, bool NT>
__global__ __launch_bounds__(BLOCK) void k_wire_rzrouter(RzWireArgs a) {
    const uint32_t lane = threadIdx.x & 63u;
    const size_t i = (size_t)blockIdx.x * (BLOCK / 64) + (threadIdx.x >> 6);
    if (i >= a.n) return;
    const uint64_t o0 = a.off[i], o1 = a.off[i + 1];
    const bool in_blob = o0 <= o1 && o1 <= a.cd_bytes;       // offsets come from the caller: never read outside the blob
    const uint8_t* cd = a.cd + (in_blob ? o0 : 0);
    const uint64_t len = in_blob ? o1 - o0 : 0;
    const bool al = (((uintptr_t)cd) & 3u) == 0;
    const RzwCall h = rzw_parse(cd, len, al, a.sel_be);      // wave-uniform
    bool ok = h.ok != 0;
    uint8_t* slot = a.seals + i * 260;
    if (ok && h.form == GWW_FORM_UINT8_ARRAY) ok = wire_u8_array<NT>(cd + h.seal_at, h.seal_len, al, slot, 260, lane);
    else if (ok) {
        const uint8_t* src = cd + h.seal_at;
        const uint32_t L = h.seal_len, m = L < 260u ? L : 260u;
        uint32_t k = 0;                                      // bytes the dword path has copied
        if (al && !((uintptr_t)a.seals & 3u)) {
            k = m & ~3u;
            for (uint32_t w = lane; w < k / 4; w += 64) {
                const uint32_t* q = (const uint32_t*)src + w;
                ((uint32_t*)slot)[w] = NT ? __builtin_nontemporal_load(q) : *q;
            }
        }
        for (uint32_t t = k + lane; t < m; t += 64) slot[t] = src[t];
        const uint32_t pad = (uint32_t)(-L & 31u);
        const uint32_t b = lane < pad ? src[(uint64_t)L + lane] : 0u;
        ok = __all(b == 0) != 0;
    }
    if (h.ok) {
        copy32(a.in_a + 32 * i, cd + h.a_at, lane);
        if (!h.method) copy32(a.in_b + 32 * i, cd + h.a_at + 32, lane);
    }
    if (lane == 0) {
        a.seal_len[i] = ok ? h.seal_len : WIRE_BAD;
        a.method[i] = ok ? (uint8_t)h.method : 0;
        if (a.call_kind) a.call_kind[i] = ok ? (uint8_t)(2 * h.form + h.method) : (uint8_t)RZW_KIND_BAD;
    }
}

// One wavefront per request, four requests per workgroup, non-temporal loads (each calldata byte is read exactly once).
// Measured on 2^16 verify() requests (554 MB): 4.9 TB/s; a persistent grid-stride grid (3.4-4.5 TB/s), 64- or 512-thread
// workgroups (4.7 TB/s), default-policy loads (4.8 TB/s) and a header-independent slot-streaming form (4.4 TB/s, 98 VGPRs)
// were all slower.
static void wire_dispatch(bool sp1, const WireArgs& a, hipStream_t s) {
    if (!a.n) return;
    const size_t per = WIRE_BLOCK / 64;
    const dim3 grid((unsigned)((a.n + per - 1) / per));
    if (sp1) hipLaunchKernelGGL((k_wire_sp1<WIRE_BLOCK, true>), grid, dim3(WIRE_BLOCK), 0, s, a);
    else hipLaunchKernelGGL((k_wire_risc0<WIRE_BLOCK, true>), grid, dim3(WIRE_BLOCK), 0, s, a);
}
void launch_wire_gateway(const GwWireArgs& a, hipStream_t s) {
    if (!a.n) return;
    const size_t per = WIRE_BLOCK / 64;
    hipLaunchKernelGGL((k_wire_gateway<WIRE_BLOCK, true>), dim3((unsigned)((a.n + per - 1) / per)), dim3(WIRE_BLOCK), 0, s, a, (uint32_t)ZKV_PLONK_PROOF_BYTES);
}
void launch_wire_rzrouter(const RzWireArgs& a, hipStream_t s) {
    if (!a.n) return;
    const size_t per = WIRE_BLOCK / 64;
    hipLaunchKernelGGL((k_wire_rzrouter<WIRE_BLOCK, true>), dim3((unsigned)((a.n + per - 1) / per)), dim3(WIRE_BLOCK), 0, s, a);
}
void launch_wire_risc0(const WireArgs& a, hipStream_t s) { wire_dispatch(false, a, s); }
void launch_wire_sp1(const WireArgs& a, hipStream_t s) { wire_dispatch(true, a, s); }

}  // namespace zkv

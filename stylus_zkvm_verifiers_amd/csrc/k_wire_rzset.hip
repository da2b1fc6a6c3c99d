// Stage WIRE of a RISC Zero router with a set route (include/zkv_risc0_router_set_wire.h): verify /
// verifyIntegrity calldata whose seal may be a set-inclusion seal of any length.  k_wire_rzrouter's shape (k_wire.hip): one wavefront
// per request, four requests per workgroup, offsets checked against the blob's size before any read, non-temporal loads, the header
// arithmetic of rzw_parse.  It writes what that kernel writes -- the 260-byte slot, the true length or 0xFFFFFFFF, the inputs, the
// method, the call kind -- so the router's partition runs on fixed-stride slots through kernels that do not change, and for every
// request one (start, length) record of the WHOLE seal, which k_rzset_front reads (zkv_wire_rzset.h).
//   form B  the record points into the caller's blob; only the slot's 260 bytes are copied, the padding is checked
//   form U  one pass over the element words, a lane pair per word as k_wire.hip's wire_u8_array streams them (that loop has one
//           destination and lives in a unit that must compile to the same object, so this unit has its own): every element is
//           checked, the first 260 bytes go to the slot, and the first rzsw_keep() bytes -- all of a seal with the set selector -- to
//           the arena at rzsw_arena_at(off[i]).  The check never stops, the copies do.
// Parity unpinned: the reference has no router.
#include "zkv_wire_rzset.h"

namespace zkv {

constexpr int RZSW_BLOCK = 256;                  // four requests per workgroup
constexpr uint32_t RZSW_BAD = 0xFFFFFFFFu;

// 16 bytes of calldata as four dwords in ABI (big-endian) significance order: w[3] holds the lowest-order bytes.
template <bool AL>
__device__ __forceinline__ void rzsw_load16(const uint8_t* __restrict__ p, uint32_t w[4]) {
    if (AL) {
        const uint32_t* q = (const uint32_t*)p;
        w[0] = __builtin_nontemporal_load(q); w[1] = __builtin_nontemporal_load(q + 1); w[2] = __builtin_nontemporal_load(q + 2);
        w[3] = __builtin_bswap32(__builtin_nontemporal_load(q + 3));
    } else {
        w[0] = load_be32(p); w[1] = load_be32(p + 4); w[2] = load_be32(p + 8); w[3] = load_be32(p + 12);
    }
}

// The n_el element words of one uint8[] from `el`: every lane pair takes one word (even lane the upper 16 bytes, odd lane the lower 16),
// one wave-instruction reads 1 KiB of contiguous calldata, and on 4-byte aligned requests eight such loads are in flight before the
// first is consumed.  Byte k goes to slot[k] while k < 260 and to arena[k] while k < keep.  false (wave-uniform): an element is no uint8.
template <bool AL>
__device__ __forceinline__ bool rzsw_u8_array_t(const uint8_t* __restrict__ el, uint32_t n_el, uint8_t* __restrict__ arena, uint32_t keep,
                                                uint8_t* __restrict__ slot, uint32_t lane) {
    const uint32_t half = lane & 1u;
    uint32_t bad = 0, k = lane >> 1;
#pragma unroll 1
    for (; AL && k + 32 * 7 < n_el; k += 32 * 8) {
        uint32_t w[8][4];
#pragma unroll
        for (int j = 0; j < 8; j++) rzsw_load16<AL>(el + (size_t)32 * (k + 32 * j) + 16 * half, w[j]);
#pragma unroll
        for (int j = 0; j < 8; j++) {
            const uint32_t hi = w[j][0] | w[j][1] | w[j][2], at = k + 32 * j;
            if (half) {
                bad |= hi | (w[j][3] & ~0xFFu);
                if (at < 260u) slot[at] = (uint8_t)w[j][3];
                if (at < keep) arena[at] = (uint8_t)w[j][3];
            } else bad |= hi | w[j][3];
        }
    }
#pragma unroll 1
    for (; k < n_el; k += 32) {
        uint32_t w[4];
        rzsw_load16<AL>(el + (size_t)32 * k + 16 * half, w);
        const uint32_t hi = w[0] | w[1] | w[2];
        if (half) {
            bad |= hi | (w[3] & ~0xFFu);
            if (k < 260u) slot[k] = (uint8_t)w[3];
            if (k < keep) arena[k] = (uint8_t)w[3];
        } else bad |= hi | w[3];
    }
    return __all(bad == 0) != 0;
}

__device__ __forceinline__ void rzsw_copy32(uint8_t* dst, const uint8_t* src, uint32_t lane) {
    if (lane < 32) dst[lane] = src[lane];
}

// Every position is bounded by rzw_parse: it demands the exact total length, and the request itself lies inside the blob.  The arena
// positions are bounded by zkv_wire_rzset.h's argument.
__global__ __launch_bounds__(RZSW_BLOCK) void k_wire_rzset(RzSetWireArgs a) {
    const uint32_t lane = threadIdx.x & 63u;
    const size_t i = (size_t)blockIdx.x * (RZSW_BLOCK / 64) + (threadIdx.x >> 6);
    if (i >= a.w.n) return;
    const uint64_t o0 = a.w.off[i], o1 = a.w.off[i + 1];
    const bool in_blob = o0 <= o1 && o1 <= a.w.cd_bytes;     // offsets come from the caller: never read outside the blob
    const uint8_t* cd = a.w.cd + (in_blob ? o0 : 0);
    const uint64_t len = in_blob ? o1 - o0 : 0;
    const bool al = (((uintptr_t)cd) & 3u) == 0;
    const RzwCall h = rzw_parse(cd, len, al, a.w.sel_be);    // wave-uniform
    bool ok = h.ok != 0;
    uint8_t* slot = a.w.seals + i * 260;
    uint64_t at = 0;
    if (ok && h.form == GWW_FORM_UINT8_ARRAY) {
        const uint8_t* el = cd + h.seal_at;
        uint32_t first4 = 0;                                 // the low byte of the first four element words
        if (h.seal_len >= 4) first4 = ((uint32_t)el[31] << 24) | ((uint32_t)el[63] << 16) | ((uint32_t)el[95] << 8) | el[127];
        const uint32_t keep = rzsw_keep(h.seal_len, first4, a.set_sel);
        const uint64_t pos = rzsw_arena_at(o0);
        uint8_t* dst = a.arena + pos;
        ok = al ? rzsw_u8_array_t<true>(el, h.seal_len, dst, keep, slot, lane) : rzsw_u8_array_t<false>(el, h.seal_len, dst, keep, slot, lane);
        at = a.arena_delta + pos;
    } else if (ok) {
        const uint8_t* src = cd + h.seal_at;
        const uint32_t L = h.seal_len, m = L < 260u ? L : 260u;
        uint32_t k = 0;                                      // bytes the dword path has copied
        if (al && !((uintptr_t)a.w.seals & 3u)) {
            k = m & ~3u;
            for (uint32_t w = lane; w < k / 4; w += 64) ((uint32_t*)slot)[w] = __builtin_nontemporal_load((const uint32_t*)src + w);
        }
        for (uint32_t t = k + lane; t < m; t += 64) slot[t] = src[t];
        const uint32_t pad = (uint32_t)(-L & 31u);
        const uint32_t b = lane < pad ? src[(uint64_t)L + lane] : 0u;
        ok = __all(b == 0) != 0;
        at = a.cd_delta + o0 + h.seal_at;
    }
    if (h.ok) {
        rzsw_copy32(a.w.in_a + 32 * i, cd + h.a_at, lane);
        if (!h.method) rzsw_copy32(a.w.in_b + 32 * i, cd + h.a_at + 32, lane);
    }
    if (lane == 0) {
        a.w.seal_len[i] = ok ? h.seal_len : RZSW_BAD;
        a.w.method[i] = ok ? (uint8_t)h.method : 0;
        if (a.w.call_kind) a.w.call_kind[i] = ok ? (uint8_t)(2 * h.form + h.method) : (uint8_t)RZW_KIND_BAD;
        RzsSpan sp;
        sp.at = ok ? at : 0; sp.len = ok ? h.seal_len : 0; sp.pad = 0;
        a.span[i] = sp;
    }
}

void launch_wire_rzset(const RzSetWireArgs& a, hipStream_t s) {
    if (!a.w.n) return;
    const size_t per = RZSW_BLOCK / 64;
    hipLaunchKernelGGL(k_wire_rzset, dim3((unsigned)((a.w.n + per - 1) / per)), dim3(RZSW_BLOCK), 0, s, a);
}

}  // namespace zkv

// eth_call calldata of a RISC Zero router with a set route (include/zkv_risc0_router_set_wire.h): what
// k_wire_rzset (k_wire_rzset.hip), the set stage (k_rzrouter_set.hip) and the host (tests/host_sim/host_sim_rzset_wire.cpp) share.  The
// call shapes are zkv_wire_rzrouter.h's and the seal inside a call is zkv_rzrouter_set.h's; this header adds where the whole seal of a
// request lies for the set stage, and which claim digest a set seal's row asks for.  Parity unpinned: the reference has no router.
#pragma once
#include "zkv_rzrouter_set.h"
#include "zkv_wire_rzrouter.h"

namespace zkv {

// Arena of the form U requests: calldata_bytes / 32 + 64 bytes.  The request at blob offset o0 is compacted to arena[rzsw_arena_at(o0) ..),
// a 4-byte aligned position, so that the path of a set seal -- RZS_PATH_AT = 132 bytes into it -- is 4-byte aligned as well and
// k_rzset_hash loads its siblings as dwords.
//   Room.  A form U request of L decoded bytes spans at least 100 + 32 L bytes of calldata ([o0, o1): selector, two or three head words,
//   the length word, L element words), and floor((x + 100) / 32) >= floor(x / 32) + 3 for every x.  So
//       rzsw_arena_at(o0) + L <= floor(o0 / 32) + 3 + L <= floor((o0 + 100 + 32 L) / 32) <= floor(o1 / 32)
//   Disjoint.  A request that begins at o0' >= o1 is placed at or behind floor(o0' / 32) >= floor(o1 / 32): the three bytes that the
//   head of a request is worth pay for the rounding.  Requests whose calldata does not overlap in the blob do not overlap in the arena.
//   Inside.  o1 <= calldata_bytes, so every copy ends at or below calldata_bytes / 32.
ZKV_HD uint64_t rzsw_arena_at(uint64_t o0) { return (o0 / 32 + 3) & ~(uint64_t)3; }
ZKV_HD uint64_t rzsw_arena_bytes(uint64_t calldata_bytes) { return calldata_bytes / 32 + 64; }

// Bytes of a form U seal that are kept: all of a seal that begins with the set selector (the set stage reads paths and root seals of any
// length), the slot's 260 of any other one (no Groth16 route reads more).  first4: the first four decoded bytes, big-endian.
ZKV_HD uint32_t rzsw_keep(uint32_t seal_len, uint32_t first4_be, uint32_t set_sel_be) {
    return seal_len >= 4 && first4_be == set_sel_be ? seal_len : (seal_len < 260u ? seal_len : 260u);
}

}  // namespace zkv

// ---------------------------------------------------------------- the kernel (k_wire_rzset.hip) and its launcher
#if defined(__HIPCC__)
#include "zkv_internal.h"

namespace zkv {

// RzWireArgs' output (slots, true lengths, inputs, methods, call kinds) and one RzsSpan per request.  base: an address at or below both
// the calldata blob and the arena; the spans are distances from it.
struct RzSetWireArgs {
    RzWireArgs w;
    uint32_t set_sel;                                                          // the set selector as a big-endian word
    uint8_t* arena; uint64_t cd_delta, arena_delta;                            // rzsw_arena_bytes(w.cd_bytes); cd - base, arena - base
    RzsSpan* span;                                                             // n
};
void launch_wire_rzset(const RzSetWireArgs& a, hipStream_t s);

}  // namespace zkv
#endif

// Internal interface between the C-ABI translation unit and the kernel translation units.
#pragma once
#include <hip/hip_runtime.h>
#include "zkv_verify.h"

namespace zkv {

// Per-chunk workspace in HBM, struct-of-arrays: word k of proof i lives at base[k * cap + i], so the 64 lanes
// of a wavefront read/write 256 contiguous bytes per word (coalesced).
constexpr int WS_PREP_WORDS = 64 + 8 * MAX_VAR;   // ax ay cx cy (4x8) | bx.c0 bx.c1 by.c0 by.c1 (4x8) | per-proof scalars (MAX_VAR x 8)
// The scalar rows (64 ..) are written by the PREP stage alone and must stay as written until the chunk's last kernel: with GT tables (zkv_gt.h)
// k_finalexp2 cuts its window digits from rows 64 .. 79.
constexpr int WS_NORM_WORDS = 48;   // axs ays lxs lys cxs cys
constexpr int WS_F_WORDS = 96;      // Fp12 Miller value (slot F of the final exponentiation)
constexpr int WS_FE_WORDS = 7 * 96; // cold Fp12 slots of the final exponentiation: E, Y1, Y3, Y4 and the window slots x^3, x^5, x^7
struct Workspace {
    uint32_t* prep; uint32_t* norm; uint32_t* f; uint32_t* fe; uint32_t* flags;
    uint32_t* g2bad;            // 1 = B failed the subgroup check (own word: the check may run beside the MSM, which owns `flags`)
    size_t cap;
    uint8_t* gtag;              // walk-prefix cache (zkv_gt.h): one tag byte per proof, written by k_gt_cache_tag (nullptr in the secondary workspaces)
};

constexpr int ZKV_BLOCK = 64;       // one wavefront per workgroup: one proof per lane, no cross-lane traffic

__device__ __forceinline__ Fp ws_ld(const uint32_t* base, size_t cap, int word0, size_t i) {
    Fp r;
#pragma unroll
    for (int k = 0; k < 8; k++) r.v[k] = base[(size_t)(word0 + k) * cap + i];
    return r;
}
__device__ __forceinline__ void ws_st(uint32_t* base, size_t cap, int word0, size_t i, const Fp& a) {
#pragma unroll
    for (int k = 0; k < 8; k++) base[(size_t)(word0 + k) * cap + i] = a.v[k];
}

struct PrepArgs {
    size_t n;
    const uint8_t* blob;        // seals / proofs
    const uint64_t* off;        // n+1 offsets, or nullptr for fixed stride
    uint32_t stride;            // bytes per record when off == nullptr
    const uint8_t* in32_a;      // risc0: image_ids (or claim digests when in32_b == nullptr); sp1: program vkeys
    const uint8_t* in32_b;      // risc0: journal digests; sp1: unused
    const uint8_t* pv_blob;     // sp1 public values
    const uint64_t* pv_off;     // sp1: n+1 offsets or nullptr
    uint32_t pv_stride;
    uint32_t selector_be;       // expected selector as big-endian word
    uint32_t force_fail;        // context-level VerificationFailed (risc0 bn254_control_id >= R, invalid generic VK)
    uint32_t n_sig;             // generic Groth16 batches: signals per proof (in32_a holds n x n_sig x 32 bytes)
    uint32_t negate_a;          // generic Groth16 batches: VMType::Risc0 negates A
    // wire-layer batches (k_wire.hip decodes calldata into fixed-stride records): per-proof decoded seal length
    // (0xFFFFFFFF = undecodable calldata), per-proof method (1 = verifyIntegrity: in32_a is the claim digest) and
    // per-proof public-values length (pv_off then holds n start offsets).
    const uint32_t* len;
    const uint8_t* kind;
    const uint32_t* pv_len;
    // verifier sets (zkv_risc0_set_*): per-proof instance index; selector and context-level failure come from the table
    const uint32_t* inst; const InstTab* inst_tab; uint32_t n_inst;
    uint32_t* plonk_tab;        // PLONK batches: PLONK_TAB_WORDS words per proof for the per-proof window tables of the MSMs (zkv_plonk.h)
    uint32_t not_initialized;   // wire-layer batches on an un-initialised RISC Zero verifier: decodable calls get InvalidInitialization
    uint8_t* status; uint8_t* recv;
};

// eth_call calldata decode (k_wire.hip): one wavefront per request.
struct WireArgs {
    size_t n;
    const uint8_t* cd;          // calldata blob
    const uint64_t* off;        // n+1 offsets
    uint64_t cd_bytes;          // size of the blob: a request whose offsets leave [0, cd_bytes] or run backwards is never read
    uint32_t sel_a_be, sel_b_be;    // risc0: verify / verifyIntegrity; sp1: verifyProof / unused
    uint8_t* seals;             // n x 260: first min(L, 260) decoded seal / proof bytes
    uint32_t* seal_len;         // n: decoded length L, or 0xFFFFFFFF when the calldata is not a canonical verify call
    uint8_t* in_a; uint8_t* in_b;   // n x 32 each: risc0 image id (claim digest) / journal digest; sp1 program vkey / unused
    uint8_t* kind;              // n: risc0 0 = verify, 1 = verifyIntegrity
    uint8_t* pv; uint64_t* pv_off; uint32_t* pv_len;    // sp1 public values: pv_off[i] = off[i] / 32
};
void launch_wire_risc0(const WireArgs& a, hipStream_t s);
void launch_wire_sp1(const WireArgs& a, hipStream_t s);
// eth_call calldata of the SP1 gateway (k_wire_gateway in k_wire.hip; zkv_wire_gateway.h has the two forms): one record per request,
// its public values and proof as (start, true length) from `base`, an address at or below both the calldata blob and the arena.  Form U
// requests are compacted into the arena (request i at arena[off[i] / 32 ..): public values, then the first min(Lproof, ZKV_PLONK_PROOF_BYTES)
// proof bytes); form B records point into the blob.  A request that is not a canonical call has bad = 1 and zero starts and lengths.
struct GwWireArgs {
    size_t n;
    const uint8_t* cd; const uint64_t* off; uint64_t cd_bytes;                  // as WireArgs
    uint32_t sel_u_be, sel_b_be;                                               // verifyProof(bytes32,uint8[],uint8[]) / verifyProof(bytes32,bytes,bytes)
    uint8_t* arena;                                                            // cd_bytes / 32 + 64 bytes
    uint64_t cd_delta, arena_delta;                                            // cd - base, arena - base
    uint8_t* vkeys;                                                            // n x 32
    uint64_t* pv_at; uint32_t* pv_len; uint64_t* proof_at; uint32_t* proof_len; uint8_t* bad;
};
void launch_wire_gateway(const GwWireArgs& a, hipStream_t s);
// eth_call calldata of the RISC Zero router (k_wire_rzrouter in k_wire.hip; zkv_wire_rzrouter.h has the four call shapes): request i to a
// fixed 260-byte slot with the first min(L, 260) seal bytes, the true L (0xFFFFFFFF: not a canonical call), its two 32-byte inputs and
// its method -- the router's fixed-stride input with a true-length row (RzrArgs::wire_len).
struct RzWireArgs {
    size_t n;
    const uint8_t* cd; const uint64_t* off; uint64_t cd_bytes;                  // as WireArgs
    uint32_t sel_be[4];                                                        // selector of call kind 2 form + method
    uint8_t* seals; uint32_t* seal_len;                                        // n x 260 (4-byte aligned), n
    uint8_t* in_a; uint8_t* in_b;                                              // n x 32 each; in_b is written for verify calls only
    uint8_t* method;                                                           // n: ZKV_METHOD_* (0 for a bad request)
    uint8_t* call_kind;                                                        // n or nullptr: 2 form + method, 255 for a bad request
};
void launch_wire_rzrouter(const RzWireArgs& a, hipStream_t s);

void launch_setup(const VkRaw* d_raw, VkTables* d_tab, hipStream_t s);
void launch_prep_risc0(const PrepArgs& a, const Risc0Consts& k, const Workspace& ws, hipStream_t s);
void launch_prep_sp1(const PrepArgs& a, const Workspace& ws, hipStream_t s);
void launch_prep_groth16(const PrepArgs& a, const Workspace& ws, hipStream_t s);
void launch_setup_msm16(const VkTables* d_tab, const Msm16& m, G1A* tab, uint32_t rows, hipStream_t s);
// skip_vk_x: no window walk -- every vk_x is reported absent (FL_L_INF), A' and C are normalised as always (chunks whose (vk_x, gamma) pair goes
// through the GT tables)
void launch_msm(size_t n, const VkTables* d_tab, const Msm16& m16, const InstTab* inst_tab, const Workspace& ws, hipStream_t s, bool skip_vk_x = false);
void launch_msm_w(size_t n, const VkTables* d_tab, const InstTab* inst_tab, const Workspace& ws, hipStream_t s);
// long keys (n_ic > MAX_IC or ZKV_LONG_KEY=1; LongKey in zkv_verify.h)
void launch_setup_long(const uint32_t* d_ic, uint32_t n_sig, VkTables* d_tab, G1A* tab, uint32_t* win, hipStream_t s);
void launch_prep_groth16_long(const PrepArgs& a, const Workspace& ws, uint32_t* sig, size_t stride, hipStream_t s);
void launch_msm_long(size_t n, uint32_t lanes, const VkTables* d_tab, const LongKey& lk, const Workspace& ws, hipStream_t s);
void launch_vk_x_long(size_t n, uint32_t lanes, const VkTables* d_tab, const LongKey& lk, const uint8_t* sig, uint8_t* out, hipStream_t s);
void launch_status_to_bool(size_t n, uint8_t* status, hipStream_t s);
void launch_setup_instances(const VkRaw* d_raw, const InstConsts& k, const InstRaw* d_in, InstTab* d_out, uint32_t n_inst, hipStream_t s);
void launch_vk_x(size_t n, const VkTables* d_tab, const Msm16& m16, const InstTab* inst_tab, const uint32_t* inst, const uint8_t* sig, uint8_t* out, hipStream_t s);
// lane-pair variants (k_pair.hip): one proof per two lanes, two waves per SIMD
void launch_g2chk2(size_t n, const Workspace& ws, uint8_t* status, hipStream_t s);
// mconst / gt: the chunk leaves the (vk_x, gamma) pair to the context's GT tables (zkv_gt.h; its vk_x stage ran with skip_vk_x) -- the
// Miller loop multiplies the folded constant in, the final exponentiation walks the tables.  Defaults: the Miller path.
constexpr GtTab GT_NONE = {nullptr, nullptr, {0, 0}};
void launch_miller2(size_t n, const VkTables* d_tab, const Workspace& ws, uint8_t* status, hipStream_t s, const uint32_t* mconst = nullptr);
void launch_finalexp2(size_t n, const Workspace& ws, uint8_t* status, hipStream_t s, const GtTab& gt = GT_NONE);
// walk-prefix cache (zkv_gt.h; gt.cache != nullptr): at most one insertion from the chunk's sampled proofs, then the chunk's tag bytes
// (ws.gtag).  Both read the scalar rows and flags PREP wrote and come before launch_finalexp2 on the same stream.
void launch_gt_cache(size_t n, const Workspace& ws, hipStream_t s, const GtTab& gt);
// set-up of the tables (k_gt.hip): the window bases G_i^(2^(20 j)) and the folded constant (one launch, scratch: GT_SETUP_SCRATCH_WORDS
// words), then level L = 1 .. 19 fills entries d = 2^L .. 2^(L+1) - 1 (L = 19: d = 2^19) of every row from entries d / 2
constexpr size_t GT_SETUP_SCRATCH_WORDS = 3 * 12 * 96;
void launch_gt_bases(const VkRaw* d_raw, const VkTables* d_tab, uint32_t* tab, uint32_t* mconst, uint32_t* scratch, uint32_t nw0, uint32_t nw1, hipStream_t s);
void launch_gt_level(uint32_t* tab, uint32_t rows, uint32_t level, hipStream_t s);
// the build's last step: every entry of `rows` windows to its affine torus value, in place (k_gt_torus)
void launch_gt_torus(uint32_t* tab, uint32_t rows, hipStream_t s);
// test only (zkv_diag_gt_read / zkv_diag_gt_product): a stored a back to the full entry; u / conj(u) of the n values in the TMP rows
void launch_gt_diag_expand(const uint32_t* a48, uint32_t* out96, hipStream_t s);
void launch_gt_diag_ratio(size_t n, const uint32_t* tmp, size_t cap, uint32_t* out, uint32_t* scr, hipStream_t s);
// test only (zkv_diag_gt_product): flags alive, Miller value 1 for n lane-pair proofs
void launch_gt_diag_seed(size_t n, const Workspace& ws, hipStream_t s);
// coefficient-parallel small-batch variants (k_wide.hip): one proof per 16 lanes
void launch_miller_w(size_t n, const VkTables* d_tab, const Workspace& ws, hipStream_t s);
void launch_finalexp_w(size_t n, const Workspace& ws, uint8_t* status, hipStream_t s);
// one proof per wavefront (k_wide.hip, four slices of 16 lanes): the smallest chunks
void launch_miller_w64(size_t n, const VkTables* d_tab, const Workspace& ws, hipStream_t s);
void launch_finalexp_w64(size_t n, const Workspace& ws, uint8_t* status, hipStream_t s);
// two wavefronts per proof: one steps the running point and tabulates the lines, the other accumulates f (the very smallest chunks)
void launch_miller_w64d(size_t n, const VkTables* d_tab, const Workspace& ws, uint8_t* status, hipStream_t s);

// mixed batches (k_mixed.hip): per-proof VM tag, device-side demultiplexing into two homogeneous sub-batches
struct MixedArgs {
    size_t n;
    const uint8_t* vm;
    const uint8_t* method;                                                     // n x ZKV_METHOD_*, or nullptr: all verify
    const uint8_t* seals; const uint64_t* seal_off; uint32_t seal_stride;     // ragged (off) or fixed stride
    const uint8_t* in_a;                                                       // n x 32
    const uint8_t* in_b; const uint64_t* b_off; uint32_t b_stride, pv_len;     // ragged (off) or fixed stride + fixed SP1 length
    const uint32_t* cnt; const uint32_t* totals;
    uint32_t* pos; uint32_t* idx;                                              // pos[i] = slot (0xFFFFFFFF: unknown VM / method); idx[slot] = i
    uint8_t* c_seals; uint32_t* c_len; uint8_t* c_a; uint8_t* c_b; uint64_t* c_pvoff; uint32_t* c_pvlen;   // compact records
    uint8_t* c_kind;                                                           // compact RISC Zero method (PrepArgs::kind)
    uint8_t* status; uint8_t* recv;                                            // caller's outputs (unknown-VM proofs are answered here)
};
void launch_mixed_partition(const MixedArgs& a, uint32_t* cnt, uint32_t* totals, hipStream_t s);
void launch_mixed_return(size_t m, const uint32_t* idx, const uint8_t* c_status, const uint8_t* c_recv, uint8_t* status, uint8_t* recv, hipStream_t s);

// SP1 gateway (k_gateway.hip, include/zkv_sp1_gateway.h): every proof goes to the route whose selector begins it.  Count columns:
// routes 0 .. GW_MAX_ROUTES - 1, then GW_COL_NOT_FOUND, GW_COL_SHORT (shorter than 4 bytes, or offsets outside the blob) and GW_COL_BAD
// (record input only: the request was not a canonical call, GwWireArgs::bad).
constexpr int GW_MAX_ROUTES = 8, GW_COL_NOT_FOUND = 8, GW_COL_SHORT = 9, GW_COL_BAD = 10, GW_COLS = 11;
constexpr uint32_t GW_NONE = 0xFFFFFFFFu;
struct GatewayArgs {
    size_t n;
    const uint8_t* proofs; const uint64_t* proof_off; uint64_t proof_bytes;    // ragged proofs; proof_bytes bounds every read
    const uint8_t* vkeys;                                                      // n x 32
    const uint64_t* pv_off; uint64_t pv_stride;                                // public values: n + 1 offsets (ragged) or a fixed stride
    // record input (rec_proof_at set: proof_off, proof_bytes, pv_off and pv_stride are unused): (start, length) per proof, gaps allowed.
    // The records come from k_wire_gateway, which has bounded them; `proofs` and the public-values blob are then its one `base`.
    const uint64_t* rec_proof_at; const uint32_t* rec_proof_len; const uint64_t* rec_pv_at; const uint32_t* rec_pv_len; const uint8_t* rec_bad;
    uint32_t n_routes;
    uint32_t sel[GW_MAX_ROUTES];                                               // route selectors, big-endian words (kernel arguments: SGPRs)
    uint32_t rec[GW_MAX_ROUTES];                                               // record bytes per route: ZKV_SEAL_BYTES or ZKV_PLONK_PROOF_BYTES
    uint32_t start[GW_MAX_ROUTES]; uint64_t base[GW_MAX_ROUTES];               // (place, gather) first slot and record byte offset of each route
    // (place) aggregate check on the keyed group (zkv_gset_layout.h route_layout_agg): the first agg[r] proofs of route r, in caller order,
    // go to slots astart[r] .., the others to start[r] .. (base[r] is that part's); agg[r] = 0: one region.  (gather) the keyed group is
    // slots [g0, g0 + gm), its 260-byte rows from byte gb0, whichever region a slot lies in; gm = 0: no keyed route
    uint32_t agg[GW_MAX_ROUTES], astart[GW_MAX_ROUTES];
    uint32_t g0, gm; uint64_t gb0;
    uint32_t* cnt; uint32_t* totals;                                           // GW_COLS per block (exclusive scan in place), GW_COLS totals
    uint32_t* pos; uint32_t* idx;                                              // pos[i] = slot (GW_NONE: answered in place); idx[slot] = i
    uint8_t* c_proofs; uint32_t* c_len; uint8_t* c_a; uint64_t* c_pvoff; uint32_t* c_pvlen;    // compact records
    uint8_t* status; uint8_t* recv;                                            // caller's outputs (short / not-found proofs answered here)
};
void launch_gateway_count(const GatewayArgs& a, hipStream_t s);     // count + scan: totals[GW_COLS]
void launch_gateway_place(const GatewayArgs& a, hipStream_t s);     // place + gather (start[] / base[] filled from the totals)

// Groth16 key sets (k_gset.hip, k_gset_pair.hip; zkv_gset_layout.h): per-key device record.  tab: the key's VkTables (alpha, beta, gamma,
// delta, IC[0]); its IC[1..] window rows are rows [sig0, sig0 + n_sig) of the set's one row allocation (LongKey layout), and win[sig0 ..]
// their window counts.
struct GsetKey { const VkTables* tab; uint32_t sig0, n_sig, negate, pad; };
constexpr uint32_t GSET_NONE = 0xFFFFFFFFu;      // pad slot (idx) / proof with no key (pos)
struct GsetPart {
    size_t n; uint32_t n_keys, blocks, per_block;   // per_block: proofs per partition block (a multiple of 64)
    const uint32_t* key;                            // caller's key per proof
    uint32_t* cnt;                                  // n_keys x blocks, key-major
    uint32_t* totals;                               // n_keys
    uint32_t* off;                                  // n_keys x blocks: first slot of (key, block)
    uint32_t* idx; uint32_t* skey;                  // per slot: caller index (GSET_NONE: pad) and key
    uint32_t* pos;                                  // per proof: slot (GSET_NONE: key >= n_keys)
};
struct GsetChunk {
    size_t m, slot0;                                // slots [slot0, slot0 + m) of the call
    const uint32_t* idx; const uint32_t* skey;      // whole-call slot tables
    const GsetKey* keys; const G1A* rows; const uint32_t* win;
    const uint8_t* proofs; const uint8_t* signals; uint32_t sig_stride;   // caller rows: 256 bytes / sig_stride bytes per proof
    uint32_t* sig; size_t sig_cap;                  // staged signals: limb k of signal b of slot j at sig[(8 b + k) * sig_cap + j]
    uint8_t* status;                                // m statuses (slot order)
};
void launch_gset_setup(uint32_t n_keys, const VkRaw* d_raw, VkTables* d_tabs, uint32_t n_sig_all, const uint32_t* d_ic, const uint32_t* d_sig_key,
                       G1A* rows, uint32_t* win, hipStream_t s);
void launch_gset_count(const GsetPart& p, hipStream_t s);
void launch_gset_place(const GsetPart& p, const uint64_t* d_start, hipStream_t s);
void launch_gset_prep(const GsetChunk& c, const Workspace& ws, hipStream_t s);
void launch_gset_msm(const GsetChunk& c, uint32_t lanes, const Workspace& ws, hipStream_t s);
void launch_gset_vk_x(size_t n, uint32_t lanes, const uint32_t* key, const GsetKey* keys, const G1A* rows, const uint32_t* win, const uint8_t* sig,
                      uint32_t sig_stride, uint8_t* out, hipStream_t s);
void launch_gset_return(size_t n, const uint32_t* pos, const uint8_t* status, uint8_t* verified, hipStream_t s);
// Miller loops with the key of each wavefront's first slot (k_gset_pair.hip): lanes 2 / 16 / 64 / 128 as zkv_ctx_set_lanes_per_proof
void launch_gset_miller(int lanes, size_t m, const uint32_t* skey, const GsetKey* keys, const Workspace& ws, uint8_t* status, hipStream_t s);
int read_gset_wait_faults(unsigned long long* out);     // k_gset_miller_w64d's counterpart of read_wait_faults
// eth_call calldata of a set of deployed contracts (k_gset_wire.hip; zkv_wire_gset.h has the decode rule and GswArgs): one request per
// lane into the set's ordinary inputs, then, behind the set's pipeline, one lane per request for the status byte and the four totals
// (counts: placed, no contract, bad calldata, signal not in field -- added to, so zeroed by the host).
struct GswArgs;
void launch_gset_wire_decode(const GswArgs& a, hipStream_t s);
void launch_gset_wire_return(size_t n, const uint8_t* verdict, const uint8_t* ge_r, const uint8_t* verified, uint8_t* status,
                             unsigned long long* counts, hipStream_t s);
// eth_call calldata of a set of deployed PLONK contracts (k_pset_wire.hip; zkv_wire_pset.h has the rules and PswArgs): one request per
// lane into the PLONK set's ordinary inputs, the curve test of the copied proofs' points, then, behind the set's pipeline, one lane per
// request for status and reason (may be null) and the eight totals (counts: placed, no contract, bad calldata, reasons 1 .. 5 -- added
// to, so zeroed by the host).
struct PswArgs;
void launch_pset_wire_decode(const PswArgs& a, hipStream_t s);
void launch_pset_wire_points(const PswArgs& a, hipStream_t s);
void launch_pset_wire_return(size_t n, const uint8_t* verdict, const uint8_t* reason_in, const uint8_t* ec, const uint8_t* verified, uint8_t* status,
                             uint8_t* reason, unsigned long long* counts, hipStream_t s);
// SP1 gateway, keyed Groth16 routes (k_gateway_keys.hip; include/zkv_sp1_gateway_keys.h): PREP of slots [slot0, slot0 + m) of the keyed
// group, the gateway's routes with caller keys as one key set.  Every per-slot table is the group's (index 0 = its first slot): the
// demultiplexer's compact outputs -- caller index (GW_NONE: pad slot), 260-byte records, true lengths, program vkeys, (offset, length)
// of the public values in `pv` -- and the outputs: the slot's key (skey, read by k_gset_msm and k_gset_miller), the signals staged as
// GsetChunk::sig, the status and the (zero) received selector.  start[k]: first group slot of key k (zkv_gset_layout.h).  A chunk may be
// one of the aggregate region: the k_gset_agg_* kernels then follow it as they follow k_gset_prep.
struct GwsetChunk {
    size_t m, slot0;
    const uint32_t* idx; uint32_t* skey;
    const uint8_t* recs; const uint32_t* len; const uint8_t* vkeys; const uint64_t* pvoff; const uint32_t* pvlen; const uint8_t* pv;
    uint32_t n_keys; uint32_t start[GW_MAX_ROUTES];
    uint32_t agg_r, astart[GW_MAX_ROUTES];           // aggregate region: group slots [0, agg_r), key k from astart[k]; start[] is then the per-proof region's
    const GsetKey* keys;
    uint32_t* sig; size_t sig_cap;
    uint8_t* status; uint32_t* recv;
};
void launch_gwset_prep(const GwsetChunk& c, const Workspace& ws, hipStream_t s);
// RISC Zero router (k_risc0_router.hip, include/zkv_risc0_router.h; zkv_rzrouter_prep.h has the columns): every seal goes to the route
// whose selector begins it.  The built-in-key routes are ONE column (a verifier set: place writes the instance each seal matched), every
// keyed route has its own (one key set, group k from slot start[1 + k]).
constexpr int RZR_BAD_WORD = 32;                                               // inst_tot[RZR_BAD_WORD]: behind the ZKV_RISC0_ROUTER_MAX_ROUTES route words
struct RzrArgs {
    size_t n;
    const uint8_t* seals; const uint64_t* seal_off; uint64_t seal_bytes;       // ragged seals (seal_bytes bounds every read), or seal_off == nullptr:
    uint32_t stride;                                                           // a fixed stride
    const uint32_t* wire_len;                                                  // fixed stride only, or nullptr: true length of seal i, of which the slot
                                                                               // holds the first min(length, stride) bytes; 0xFFFFFFFF: bad calldata
    const uint8_t* in_a; const uint8_t* in_b;                                  // n x 32 each; in_b == nullptr: verify_integrity, in_a holds claim digests
    const uint8_t* method;                                                     // n x ZKV_METHOD_* (a byte above 1: bad calldata), or nullptr: in_b decides
    uint32_t n_builtin, n_keyed;
    uint32_t sel[32];                                                          // route selectors, big-endian words (kernel arguments: SGPRs)
    uint32_t start[9];                                                         // (place) first slot of the built-in group and of every keyed route
    uint32_t agg[9], astart[9];                                                // (place) aggregate check on the keyed group, as GatewayArgs: the first
                                                                               // agg[c] seals of column c go to slots astart[c] .., the others to start[c] ..
    uint32_t* cnt; uint32_t* totals;                                           // GW_COLS per block (exclusive scan in place), GW_COLS totals
    uint32_t* inst_tot;                                                        // seals per built-in route, then (word RZR_BAD_WORD) the bad-calldata
                                                                               // seals, which the short column counts too (zeroed by the host)
    uint32_t* pos; uint32_t* idx;                                              // pos[i] = slot (GW_NONE: answered in place); idx[slot] = i
    uint8_t* c_seals; uint32_t* c_len; uint8_t* c_a; uint8_t* c_b; uint32_t* c_inst;      // compact records; c_inst: built-in slots only
    uint8_t* c_kind;                                                           // compact method row (method != nullptr only)
    uint8_t* status; uint8_t* recv;                                            // caller's outputs (short / unknown seals answered here)
};
void launch_rzrouter_count(const RzrArgs& a, hipStream_t s);       // count + scan: totals[GW_COLS], inst_tot[n_builtin]
void launch_rzrouter_place(const RzrArgs& a, hipStream_t s);       // place + gather (start[] filled from the totals)
// PREP of slots [slot0, slot0 + m) of the keyed group, as GwsetChunk: every per-slot table is the group's (index 0 = its first slot).
struct RzrRoute;
struct RzrChunk {
    size_t m, slot0;
    const uint32_t* idx; uint32_t* skey;
    const uint8_t* recs; const uint32_t* len; const uint8_t* in_a; const uint8_t* in_b;     // in_b == nullptr: verify_integrity
    const uint8_t* kind;                                                                    // per-slot ZKV_METHOD_*, or nullptr: in_b decides
    uint32_t n_keys; uint32_t start[GW_MAX_ROUTES];
    uint32_t agg_r, astart[GW_MAX_ROUTES];           // as GwsetChunk
    const GsetKey* keys; const RzrRoute* routes;
    uint32_t* sig; size_t sig_cap;
    uint8_t* status; uint32_t* recv;
};
void launch_rzrouter_prep(const RzrChunk& c, const Risc0Consts& k, const Workspace& ws, hipStream_t s);
// Aggregate check on a set (k_gset_agg.hip, k_gset_agg_pair.hip; the layout: zkv_gset_layout.h gset_agg_choose).  psl: pseudo-proof slot per sub-batch.
struct AggTables;
void launch_gset_setup_agg(uint32_t n_keys, const VkRaw* d_raw, const VkTables* d_tabs, AggTables* d_agg, hipStream_t s);
// (k_gset_scan of k_gset.hip with d_zero = K + 1 zero starts, so off[] holds ranks; then k_gset_agg_place with the two-region map)
__global__ void k_gset_scan(GsetPart p, const uint64_t* __restrict__ start);
void launch_gset_agg_place(const GsetPart& p, const uint64_t* d_zero, const uint64_t* d_map, hipStream_t s);
void launch_gset_agg_miller(size_t n, uint32_t g, const uint32_t* skey, const GsetKey* keys, const Workspace& ws, uint8_t* status, hipStream_t s);
void launch_gset_agg_reduce(const GsetChunk& c, uint32_t sub, uint32_t g, const Workspace& ws, const uint32_t* agg, const AggTables* tabs,
                            const Workspace& ws2, uint8_t* status2, const uint32_t* psl, bool park, hipStream_t s);
void launch_gset_agg_combine(const GsetChunk& c, size_t n2, uint32_t wide, const AggTables* tabs, const Workspace& ws2, uint8_t* status2, const uint32_t* psl,
                             hipStream_t s);
void launch_gset_agg_fprod(size_t n, size_t n2, uint32_t sub, uint32_t g, const Workspace& ws, const uint32_t* agg, const Workspace& ws2, const uint32_t* psl,
                           hipStream_t s);
void launch_gset_agg_mark(size_t n, uint32_t sub, uint32_t g, const Workspace& ws, const uint32_t* agg, const uint8_t* status2, const uint32_t* psl,
                          uint8_t* status, unsigned long long* counters, hipStream_t s);

// SP1 PLONK path (k_plonk.hip, zkv_plonk.h)
#ifndef ZKV_PLONK_PROOF_BYTES
#define ZKV_PLONK_PROOF_BYTES 868    /* selector + the 27 words of gnark's MarshalSolidity with one BSB22 commitment */
#endif
struct PlonkKeyRaw; struct PlonkKey;
void launch_plonk_setup(const PlonkKeyRaw* d_raw, PlonkKey* d_key, hipStream_t s);
void launch_plonk_setup_keys(const PlonkKeyRaw* d_raw, PlonkKey* d_key, hipStream_t s);     // any key (k_plonk_keys.hip): include/zkv_plonk_keys.h key rule
void launch_plonk_prep(const PrepArgs& a, const PlonkKey* d_key, const Workspace& ws, hipStream_t s);
void launch_plonk_prep_keys(const PrepArgs& a, const PlonkKey* d_key, const Workspace& ws, hipStream_t s);     // any key, up to 128 public inputs (k_plonk_keys.hip)
// PLONK key sets (k_plonk_set.hip; include/zkv_plonk_set.h): the PlonkKey of every key (grid y = key) and its validity word (PlonkKey.valid
// and the key's VkTables.vk_valid, so after launch_gset_setup on the same stream), and PREP with the key of each 64-slot wavefront
// (zkv_gset_layout.h pset_choose).  Slot j of a chunk is slot slot0 + j of the call; its proof is row idx[] of the caller's rows.
struct PsetChunk {
    size_t m, slot0;                                // slots [slot0, slot0 + m) of the call
    const uint32_t* idx; const uint32_t* skey;      // whole-call slot tables (GsetPart)
    const PlonkKey* keys; const uint32_t* ok;       // the set's keys and their validity words
    const uint8_t* proofs; uint32_t proof_stride;   // caller rows: key's 32 (24 + 3 n_c) bytes first
    const uint8_t* inputs; uint32_t input_stride;   // caller rows: key's nb_public 32-byte words first
    uint32_t* plonk_tab;                            // PLONK_TAB_WORDS words per slot of the chunk
    uint8_t* status;                                // m statuses (slot order)
};
void launch_pset_setup(uint32_t n_keys, const PlonkKeyRaw* d_raw, PlonkKey* d_keys, const VkTables* d_tabs, uint32_t* d_ok, hipStream_t s);
void launch_pset_prep(const PsetChunk& c, const Workspace& ws, hipStream_t s);
// Aggregate check on a PLONK set (k_pset_agg.hip; the layout: zkv_gset_layout.h pset_agg_choose).  psl: pseudo-proof slot per sub-batch of the
// chunk's m slots (m a multiple of max(64, sub)); sub <= 64 here, sub-batches of 128 / 256 slots park 64-slot sums for the combine step.
void launch_pset_agg_reduce(size_t m, uint32_t sub, const Workspace& ws, const uint32_t* agg, const Workspace& ws2, uint8_t* status2, const uint32_t* psl,
                            bool park, hipStream_t s);
void launch_pset_agg_combine(size_t n2, uint32_t wide, const Workspace& ws2, uint8_t* status2, const uint32_t* psl, hipStream_t s);

// k_wide.hip: consumer wavefronts that timed out waiting for their producer on the current device (always 0 unless a wavefront died)
int read_wait_faults(unsigned long long* out);
// multiplication-rate microbenchmark (k_diag.hip)
void launch_diag_mulmod(int kind, unsigned blocks, uint32_t iters, uint32_t* out, unsigned long long* clk, hipStream_t s);
void launch_diag_issue(int kind, unsigned blocks, uint32_t iters, uint32_t* out, unsigned long long* clk, hipStream_t s);
// known-answer harness of the primitives (k_selftest.hip: mapping 0; k_selftest_pair.hip: mappings 1-3; zkv_selftest.h)
void launch_selftest_lane(int op, unsigned waves, const uint32_t* in, uint32_t* out, hipStream_t s);
void launch_selftest_pair(int mapping, int op, unsigned waves, const uint32_t* in, uint32_t* out, hipStream_t s);
void launch_selftest_line_sums(unsigned waves, const uint32_t* in, uint32_t* out, hipStream_t s);

// aggregate check (k_agg.hip, k_pair.hip; zkv_agg.h)
struct AggTables; struct AggSeed;
void launch_setup_agg(const VkRaw* d_raw, const VkTables* d_tab, AggTables* d_agg, hipStream_t s);
void launch_agg_g1(size_t n, const VkTables* d_tab, const InstTab* inst_tab, const Workspace& ws, uint32_t* agg, const AggSeed& seed, bool sums, hipStream_t s);
void launch_agg_reduce(size_t n, uint32_t sub, bool sums, uint32_t g, const VkTables* d_tab, const Workspace& ws, const uint32_t* agg, const AggTables* tab,
                       const Workspace& ws2, uint8_t* status2, bool park, hipStream_t s);
void launch_agg_combine(size_t n64, size_t n2, uint32_t wide, const AggTables* tab, const Workspace& ws2, uint8_t* status2, hipStream_t s);
void launch_agg_miller(size_t n, uint32_t g, const VkTables* d_tab, const Workspace& ws, uint8_t* status, hipStream_t s);
void launch_agg_fprod(size_t n, size_t n2, uint32_t sub, uint32_t g, const Workspace& ws, const uint32_t* agg, const Workspace& ws2, hipStream_t s);
void launch_agg_mark(size_t n, uint32_t sub, uint32_t g, const Workspace& ws, const uint32_t* agg, const uint8_t* status2, uint8_t* status, unsigned long long* counters,
                     uint32_t* idx, hipStream_t s);
void launch_agg_gather(size_t n, const Workspace& ws, const uint32_t* agg, const unsigned long long* counters, const uint32_t* idx, const Workspace& ws3,
                       uint8_t* status3, hipStream_t s);
void launch_agg_plonk_g1(size_t n, const Workspace& ws, uint32_t* agg, const AggSeed& seed, hipStream_t s);
void launch_agg_plonk_norm(size_t n, const Workspace& ws, const uint32_t* agg, const unsigned long long* counters, const uint32_t* idx, const Workspace& ws3,
                           uint8_t* status3, hipStream_t s);
void launch_agg_scatter(size_t n, const unsigned long long* counters, const uint32_t* idx, const uint8_t* status3, uint8_t* status, hipStream_t s);

// precompile-level batches (k_precompile.hip)
void launch_ecadd(size_t n, const uint8_t* in, uint8_t* out, uint8_t* ok, hipStream_t s);
void launch_ecmul(size_t n, const uint8_t* in, uint8_t* out, uint8_t* ok, hipStream_t s);
void launch_pairing(size_t n, uint32_t k, const uint8_t* in, const Workspace& ws, uint8_t* result, uint8_t* ok, hipStream_t s);
uint32_t pairing_group(uint32_t k);      // pairs per call of the one-loop kernel (k_pairing_miller_g), 0 = none: the workspace then needs k slots per call
// the same for small batches of calls: one call per workgroup of two wavefronts (k_wide.hip)
void launch_pairing_w(size_t n, uint32_t k, const uint8_t* in, const Workspace& ws, uint8_t* result, uint8_t* ok, hipStream_t s);

}  // namespace zkv

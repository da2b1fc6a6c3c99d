// C ABI of libzkv_mi355x.so (include/zkv.h): verifier contexts, batch entry points, chunked stage pipeline.
// Host code here only marshals bytes, runs the once-per-context SHA-256 chain (initialize) and enqueues
// kernels; every field/curve/pairing operation runs in the HIP kernels.  No CPU fallback exists.
#include <hip/hip_runtime.h>
#include <algorithm>
#include <condition_variable>
#include <functional>
#include <memory>
#include <mutex>
#include <new>
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <system_error>
#include <thread>
#include <utility>
#include <vector>

#include "../../include/zkv.h"
#include "../../include/zkv_groth16_set.h"
#include "../../include/zkv_groth16_set_wire.h"
#include "../../include/zkv_sp1_gateway.h"
#include "../../include/zkv_sp1_gateway_wire.h"
#include "../../include/zkv_sp1_gateway_keys.h"
#include "../../include/zkv_plonk_keys.h"
#include "../../include/zkv_plonk_set.h"
#include "../../include/zkv_plonk_set_agg.h"
#include "../../include/zkv_plonk_set_wire.h"
#include "../../include/zkv_diag_primitive.h"
#include "../../include/zkv_diag_line_steps.h"
#include "../../include/zkv_diag_prep.h"
#include "../../include/zkv_diag_gt.h"
#include "../../include/zkv_risc0_set_inclusion.h"
#include "../../include/zkv_risc0_router.h"
#include "../../include/zkv_risc0_router_wire.h"
#include "../../include/zkv_risc0_router_set.h"
#include "../../include/zkv_risc0_router_set_wire.h"
#include "zkv_host_abi.h"
#include "zkv_host_vk.h"
#include "zkv_internal.h"
#include "zkv_devmem.h"
#include "zkv_plonk.h"
#include "zkv_agg.h"
#include "zkv_gset_layout.h"
#include "zkv_selftest.h"
#include "zkv_setincl.h"
#include "zkv_rzrouter_prep.h"
#include "zkv_wire_rzrouter.h"
#include "zkv_rzrouter_set.h"
#include "zkv_wire_rzset.h"
#include "zkv_wire_gset.h"
#include "zkv_wire_pset.h"
#include <sys/random.h>

using namespace zkv;

#define ZKV_EXPORT extern "C" __attribute__((visibility("default")))

// ---- Device state of a context.  OWNERSHIP: every device allocation, event and stream of a context is a DevBuf / DevEvent / DevStream
// (zkv_devmem.h) in one of the structs below, which hold nothing but such owners, the plain views kernels take by value
// (Workspace, GtTab, Msm16: filled from the owners beside them) and the sizes and flags that describe them, all with default member
// initialisers.  Releasing a group is assigning it a default-constructed value; a field added here needs no other edit to be released.
// ChunkMem and AggMem are sized as a whole.  The families' structs behind them (one member of CtxDevice each; DESIGN.md "Growth": which
// kind of context uses which) are staging: a call grows what it is about to use, each size beside its buffer's name (grow_all).
//
// Per-chunk buffers, sized by ctx_reserve() for ws.cap proofs in flight.
struct ChunkMem {
    DevBuf<uint32_t> ws_prep, ws_norm, ws_f, ws_fe, ws_flags, ws_g2bad;
    DevBuf<uint8_t> ws_gtag;
    Workspace ws = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, 0};      // view of the seven rows above
    DevBuf<uint8_t> d_a, d_b, d_status, d_recv;
    DevBuf<uint64_t> d_off, d_pvoff;
    DevBuf<uint32_t> d_inst_idx;
    // wire layer (eth_call batches): decoded lengths / methods, the calldata offsets of both buffers
    DevBuf<uint32_t> d_len, d_pvlen;
    DevBuf<uint8_t> d_kind;
    DevBuf<uint64_t> d_cdoff[2];
    DevBuf<uint32_t> d_plonk_tab;                              // per-proof window tables of the PLONK stage (PLONK_TAB_WORDS words per proof in flight)
};
// Buffers of the aggregate check (zkv_agg.h), sized by agg_reserve() with the workspace: per-proof rows, the pseudo-proofs' workspace
// (one per sub-batch) and their statuses; and, for the proofs of failed sub-batches gathered into a dense workspace for the ordinary
// kernels, own PREP rows, flags and statuses (the scratch rows norm, f, fe of ws3 are the chunk workspace's)
struct AggMem {
    DevBuf<uint32_t> d_agg;
    DevBuf<uint32_t> ws2_prep, ws2_norm, ws2_f, ws2_fe, ws2_flags, ws2_g2bad;
    DevBuf<uint8_t> d_status2;
    DevBuf<uint32_t> ws3_prep, ws3_flags, ws3_g2bad;
    DevBuf<uint8_t> d_status3;
    DevBuf<uint32_t> d_agg_idx;
    Workspace ws2 = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, 0};
    Workspace ws3 = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, 0};
    size_t agg_cap = 0;                                        // proofs the buffers above have room for (0: none, the chunk takes the ordinary kernels)
};
// What the three demultiplexers (mixed batches, SP1 gateway, RISC Zero router) all keep: per-block counts, per-column totals, every
// proof's position, the proof of every slot; the compact records, their lengths and first inputs; the slots' statuses and receive words.
struct DemuxMem { DevBuf<uint32_t> cnt, totals, pos, idx, len; DevBuf<uint8_t> recs, a, st, rv; };
// Mixed batches (run_mixed): the compact second inputs, public-value records and method row; h_*: the host call's staging.
struct MixedMem : DemuxMem {
    DevBuf<uint8_t> b, kind; DevBuf<uint64_t> pvoff; DevBuf<uint32_t> pvlen;
    DevBuf<uint8_t> h_vm, h_seals, h_a, h_b, h_st, h_rv, h_method; DevBuf<uint64_t> h_soff, h_boff;
};
// SP1 gateway (run_gateway): the compact public-value records and, for the keyed group, the key of every group slot; h_*: the host
// calls' staging (h_cd, h_cdoff: calldata); w_*: the rows the calldata decoder writes (run_gateway_wire).
struct GatewayMem : DemuxMem {
    DevBuf<uint64_t> pvoff; DevBuf<uint32_t> pvlen, skey;
    DevBuf<uint8_t> h_vk, h_pv, h_proof, h_st, h_rv, h_cd; DevBuf<uint64_t> h_pvoff, h_poff, h_cdoff;
    DevBuf<uint8_t> w_vk, w_bad, w_arena; DevBuf<uint64_t> w_pvat, w_pat; DevBuf<uint32_t> w_pvlen, w_plen;
};
// Section 16's grouping rows, of a set-inclusion context and of a router's set route alike: per claim the root, per root seal its
// representative and job slot, the claim <-> job maps, the four counters, the submitted roots; then the root jobs' rows (records with
// their lengths and inputs, or (keyed inner verifier) proofs and signals with the verdicts known beforehand) and their statuses.
struct SetGroupMem {
    DevBuf<uint32_t> roots, rep, gslot, claim_job, job_claim, cnt; DevBuf<uint8_t> stored;
    DevBuf<uint8_t> rows, ids, jds, proofs, signals, pre, pre_recv, jst, jrv; DevBuf<uint32_t> lens;
};
// RISC Zero router (run_router): per-instance totals, the compact second inputs, instance and method rows, every group slot's key, the
// keyed routes' constants; h_*: the host calls' staging (a calldata batch is decoded into h_a, h_b, h_method); w_*: a calldata batch's
// decoded slots, true lengths and call kinds, and on a router with a set route every request's whole-seal record and the arena of the
// uint8[] requests; s_*, grp: the set route -- claim records, root-seal table, root indices, answers, section 16.
struct RouterMem : DemuxMem {
    DevBuf<uint32_t> itot, inst, skey; DevBuf<uint8_t> b, kind; DevBuf<RzrRoute> routes;
    DevBuf<uint8_t> h_seals, h_a, h_b, h_st, h_rv, h_method; DevBuf<uint64_t> h_off;
    DevBuf<uint8_t> w_seals, w_ck, w_arena; DevBuf<uint32_t> w_len; DevBuf<RzsSpan> w_span;
    DevBuf<RzsRec> s_rec; DevBuf<uint32_t> s_owner, s_ridx, s_diag; DevBuf<uint8_t> s_ans; SetGroupMem grp;
};
// Key sets, Groth16 and PLONK (set_partition .. set_agg_plan): per-block counts, per-key totals, block offsets, every proof's position,
// the proof and key of every slot, the aggregate chunks' pseudo-proof maps; the keys' slot starts (behind the aggregate layout's map).
struct KeySetMem { DevBuf<uint32_t> cnt, totals, off, pos, idx, skey, amap; DevBuf<uint64_t> start; };
// Set-inclusion contexts (run_setincl): section 16's rows; h_*: the host call's staging; diag: zkv_diag_setincl_roots.
struct SetInclMem : SetGroupMem { DevBuf<uint8_t> h_a, h_b, h_paths, h_seals, h_st, h_rv, diag; DevBuf<uint32_t> h_poff, h_ridx, h_slen; };
// Host-buffer batches (run_host_batch): whole-batch staging in HBM, filled by segments on copy_stream while the previous one is verified.
struct HostBatchMem { DevBuf<uint8_t> seals, in_a, in_b, pv; DevBuf<uint64_t> off, pv_off; };
// Host-buffer calls on a key set: the caller's keys, proofs and signal / public-input rows, the verdicts; the vk_x call's points.
struct KeySetHostMem { DevBuf<uint32_t> key; DevBuf<uint8_t> proofs, rows, verdicts, vk_x; };
// eth_call batches on a deployed key set (run_gset_wire): the sorted address table; the rows the decoder writes -- the set's ordinary
// inputs (key, proofs, signal rows), the key each address resolved to, decode verdict and in-field byte --, the verdicts of the pipeline
// and the four totals; h_*: the host call's staging.
struct GsetWireMem {
    DevBuf<GswEntry> tab; DevBuf<uint32_t> key, rkey; DevBuf<uint8_t> proofs, rows, verdict, ge_r, verified; DevBuf<unsigned long long> cnt;
    DevBuf<uint8_t> h_to, h_cd, h_st; DevBuf<uint64_t> h_cdoff;
};
// eth_call batches on a deployed PLONK set (run_pset_wire): the sorted address table; the rows the decoder writes -- the set's ordinary
// inputs (key, proofs, input rows), the key each address resolved to, decode verdict, reason, point count and point byte --, the verdicts
// of the pipeline and the eight totals; h_*: the host call's staging.
struct PsetWireMem {
    DevBuf<PswEntry> tab; DevBuf<uint32_t> key, rkey; DevBuf<uint8_t> proofs, rows, verdict, reason, npt, ec, verified; DevBuf<unsigned long long> cnt;
    DevBuf<uint8_t> h_to, h_cd, h_st, h_rs; DevBuf<uint64_t> h_cdoff;
};
// Grows each buffer to the byte count behind it, in the order given; the first failure ends it.
static int grow_all() { return ZKV_OK; }
template <class T, class... Rest> static int grow_all(DevBuf<T>& buf, size_t bytes, Rest&&... rest) {
    const int rc = buf.grow(bytes);
    return rc != ZKV_OK ? rc : grow_all(rest...);
}
// Everything created lazily for the device (on the first compute call).  ctx_free_device() resets it as a whole.  Buffers come first,
// then events, then streams: the order in which a reset lets them go.
struct CtxDevice : ChunkMem, AggMem {
    bool dev_ready = false;
    DevBuf<VkTables> d_tab;
    DevBuf<G1A> d_msm16;                                       // the vk_x stage's 16-bit window rows (Msm16; empty: 8-bit walk)
    Msm16 m16 = {nullptr, {0, 0, 0, 0, 0}};
    // fixed-base GT tables of the (vk_x, gamma) pairing (zkv_gt.h): built the first time a call can run lane-pair chunks (gt_maybe_build);
    // gt.tab == nullptr: none (ZKV_GT_WINDOW_BITS=0, no room, another kind of context) -- the Miller loop takes the pair
    DevBuf<uint32_t> d_gt, d_gt_const;
    DevBuf<GtCache> d_gt_cache;                                // walk-prefix cache of an SP1 context with tables (zkv_gt.h); ZKV_GT_CACHE=0: none
    GtTab gt = GT_NONE;
    bool gt_tried = false;
    size_t gt_bytes = 0;
    DevBuf<InstTab> d_inst;                                    // ZKV_VM_RISC0_SET: the instances' table
    DevBuf<G1A> d_ltab; DevBuf<uint32_t> d_lwin, d_lsig;       // long key: IC[1..] window rows, their window counts, a chunk's staged signals
    // key sets: one VkTables per key, the per-key records, all keys' IC[1..] window rows in one allocation and their window counts
    DevBuf<VkTables> d_gs_tab; DevBuf<GsetKey> d_gs_key; DevBuf<G1A> d_gs_rows; DevBuf<uint32_t> d_gs_win;
    DevBuf<PlonkKey> d_pkey;
    DevBuf<uint32_t> d_ps_ok;                                  // PLONK set: a validity word per key
    // aggregate check: key tables (one AggTables per key on a set), the counters {sub-batches checked, sub-batches failed}, whether a key can take it
    DevBuf<AggTables> d_agg_tab;
    DevBuf<unsigned long long> d_agg_cnt;
    bool agg_key_ok = false;
    // staging: proofs and public values of a chunk; calldata blobs of the wire layer; whole-batch statuses and receive words
    DevBuf<> d_blob, d_pv, d_cd[2], d_st_all, d_rv_all;
    // the families' staging: host-buffer batches, key-set host calls; demultiplexing, routing, key-set and set-inclusion buffers
    HostBatchMem m_host; KeySetHostMem m_kshost;
    MixedMem m_mixed; GatewayMem m_gw; RouterMem m_rz; KeySetMem m_ks; SetInclMem m_si; GsetWireMem m_gsw; PsetWireMem m_psw;
    DevEvent ev_fork, ev_join;                                 // small chunks: the G2 subgroup check runs beside the MSM (stream `side`)
    DevEvent ev_copied[2], ev_decoded[2];                      // wire layer: H2D of calldata chunk k+1 overlaps the kernels of chunk k
    DevEvent ev[6], ev_wire[2];
    bool wire_timed = false;
    // The workspace is shared by every call on this context, and the *_dev entry points run on caller-chosen streams:
    // each call first makes its stream wait for the previous call's last kernel (ev_done), then records ev_done again.
    DevEvent ev_done;
    bool has_done = false;
    DevEvent ev_seg[2];
    DevStream copy_stream, side, stream;
};

struct zkv_ctx : CtxDevice {
    int vm = 0, device = 0, lanes = 0;       // lanes: 0 = library default, 1 or 2 = lanes per proof for the Fp2-heavy stages
    bool initialized = false, id_ge_r = false;
    uint8_t control_root_0[16] = {0}, control_root_1[16] = {0}, control_id[32] = {0}, selector[4] = {0};
    Risc0Consts consts;
    // ZKV_VM_RISC0_SET: n_inst verifier instances sharing the VK tables and the workspace
    std::vector<InstRaw> inst_raw;
    std::vector<InstTab> inst_host;          // copy of the device table (selectors derived on the device) for the getters
    std::vector<uint8_t> gvk;                // ZKV_VM_GROTH16: the caller's verification key (448 + 64 n_ic bytes)
    uint32_t g_n_ic = 0; bool g_negate = false, vk_invalid = false;
    // long-key path (n_ic > MAX_IC, or ZKV_LONG_KEY=1 at creation): IC[1..] in tables of their own (LongKey) and the staged signals of a chunk
    bool long_key = false;
    // ZKV_VM_GROTH16_SET (zkv_groth16_set.h): the keys back to back in gvk (gs_off[k]: byte offset of key k), their n_ic and sign
    // convention.  A set runs the long-key path (long_key = true, g_n_ic = the largest n_ic: d_lsig stages the signals of a chunk); on the
    // device one VkTables per key, the per-key records, all keys' IC[1..] window rows in one allocation and their window counts.
    std::vector<size_t> gs_off; std::vector<uint32_t> gs_nic; std::vector<uint8_t> gs_neg;
    std::vector<uint32_t> gs_totals; std::vector<uint64_t> gs_start;     // per call: proofs per key, slot layout (zkv_gset_layout.h)
    // aggregate check on a set: which keys can take it (d_agg_tab then holds one AggTables per key), and per call the two-region layout
    // (zkv_gset_layout.h: gset_agg_choose) and every aggregate chunk's pseudo-proof slots (run_gset)
    std::vector<uint8_t> gs_agg_ok; std::vector<uint32_t> gs_agg_n, gs_rest, gs_nsb, gs_amap; std::vector<uint64_t> gs_map, gs_pst;
    // A set of deployed contracts (zkv_groth16_set_wire.h; gsw_tab empty: not one): the address table, ascending, and per key the contract
    // form; the two gnark error selectors, ProofInvalid() and PublicInputNotInField()
    std::vector<GswEntry> gsw_tab; std::vector<uint8_t> gsw_form;
    uint8_t gsw_err[2][4] = {{0}};
    float gt_build_ms = 0;
    size_t last_chunk_n = 0;                                 // proofs of the most recent chunk (zkv_diag_prep.h reads their rows back)
    // ZKV_VM_SP1_PLONK and ZKV_VM_PLONK (zkv_plonk_keys.h): parsed verifying key, the SRS's two G2 points (reference word order) and
    // (SP1) the verifier hash
    PlonkKeyRaw pk_raw; uint8_t pk_g2[256] = {0}, plonk_hash[32] = {0};
    // ZKV_VM_PLONK_SET (zkv_plonk_set.h): every key's parsed header and points, its two G2 points (256 bytes per key in ps_g2), and the
    // largest nb_public and n_c (the row strides).  On the device: the keys' PlonkKey array in d_pkey, one VkTables per key in d_gs_tab
    // with its GsetKey in d_gs_key (what the Groth16 sets' Miller kernels read), and a validity word per key in d_ps_ok.  A call reuses
    // the Groth16 sets' partition buffers (gs_totals, gs_start, m_ks).
    std::vector<PlonkKeyRaw> ps_raw; std::vector<uint8_t> ps_g2; uint32_t ps_nb_max = 0, ps_nc_max = 0;
    // aggregate check on a PLONK set (zkv_plonk_set_agg.h): every key's SRS class and each class's first key (formed at creation), which
    // classes can take the check (read back the first time a call wants it), and per call every class's region (pset_agg_choose)
    std::vector<uint32_t> ps_class, ps_cls_rep; std::vector<uint8_t> ps_cls_ok; std::vector<uint64_t> ps_cbeg, ps_cend;
    // A PLONK set of deployed contracts (zkv_plonk_set_wire.h; psw_tab empty: not one): the address table, ascending
    std::vector<PswEntry> psw_tab;
    // Aggregate check (zkv_agg.h, zkv_ctx_set_aggregate_check): the switch and its policy state (the buffers: AggMem, CtxDevice)
    bool agg_on = false;
    uint32_t agg_sub = 32;                                     // proofs per sub-batch: 16, 32, 64, 128 or 256
    bool agg_auto = false;                                     // enable = 1: the size follows the failure rate seen so far (agg_adapt)
    unsigned long long agg_seen[2] = {0, 0};                   // counters at the last adaptation
    bool agg_resnap = false;                                   // just switched on: the next look only takes the counters as they are
    bool agg_look = false;                                     // one look at the counters per CALL (order_after_previous arms it): a later chunk of the same call
                                                               // could find the previous chunk's k_agg_mark half-way through its two counters
    uint32_t agg_pause = 0, agg_pause_len = 0;                 // automatic mode: chunks still to run WITHOUT the check (too many sub-batches fail), and the length of that pause
    bool agg_os_seed = false;                                  // the secret came from the operating system: it is drawn afresh every AGG_REKEY_CHUNKS chunks
    uint32_t agg_key_age = 0;
    AggSeed agg_seed = {{0, 0, 0, 0, 0, 0, 0, 0}, 0};
    // ZKV_VM_MIXED: one RISC Zero and one SP1 verifier (kid[]) behind a per-proof VM tag
    // Sharded (multi-device) context: `shards` single-device contexts of one verifier behind the ordinary batch entry points
    // (zkv_ctx_create_sharded).  sh[] is the per-shard state of device-resident batches: staging rows on the shard's device, a copy
    // stream (the transfer of piece k + 1 runs behind the kernels of piece k), the shard's compute stream and its events.
    struct ShardDev {
        DevBuf<> row[5], st, rv;
        DevEvent ev_piece[2], ev_done;
        DevStream copy, run;
        bool has_done = false;                                 // ev_done has been recorded: the next call's copies into row[] wait for it
        int peer = 2;                                          // peer access to the source GPU of the last staged batch: 1 granted (direct xGMI copies), 0 refused
                                                               // (the runtime bounces the copies), 2 never needed (same device, or nothing staged yet)
    };
    // One persistent host thread per shard beyond the first (shard 0 runs on the calling thread): created on first use, parked on a
    // condition variable between calls.
    struct ShardWorker {
        std::thread th; std::mutex m; std::condition_variable cv;
        std::function<void()> job; bool busy = false, quit = false;
        void loop() {
            std::unique_lock<std::mutex> lk(m);
            for (;;) {
                cv.wait(lk, [&] { return busy || quit; });
                if (quit) return;
                std::function<void()> j = std::move(job);
                lk.unlock(); j(); lk.lock();
                busy = false; cv.notify_all();
            }
        }
        void submit(std::function<void()> j) { { std::lock_guard<std::mutex> lk(m); job = std::move(j); busy = true; } cv.notify_all(); }
        void wait() { std::unique_lock<std::mutex> lk(m); cv.wait(lk, [&] { return !busy; }); }
    };
    std::vector<std::unique_ptr<ShardWorker>> workers;
    std::mutex pool_mu;                                        // one batch call at a time hands work to the pool
    std::vector<zkv_ctx*> shards;
    std::vector<ShardDev> sh;
    std::vector<DevEvent> ev_in;                         // per source device: "the caller's stream has produced the inputs"
    zkv_ctx* kid[2] = {nullptr, nullptr};
    bool kid_ran[2] = {false, false};        // which sub-batch of the most recent mixed call was non-empty (zkv_ctx_last_stage_ms)
    // ZKV_VM_SP1_GATEWAY (zkv_sp1_gateway.h): the routes' contexts and selectors; which routes ran in the most recent call
    // (zkv_ctx_last_stage_ms) and its per-column proof counts (routes, not found, short, bad calldata)
    // Keyed Groth16 routes (zkv_sp1_gateway_keys.h) are routes [gw_key0, gw_key0 + gw_nkeys): they have no context of their own
    // (gw_route[r] = nullptr) and share gw_group, a Groth16 key set of their keys (n_ic = 3, SP1 sign convention).  gw_hash: 32 bytes per route.
    std::vector<zkv_ctx*> gw_route;
    zkv_ctx* gw_group = nullptr;
    size_t gw_key0 = 0, gw_nkeys = 0;
    std::vector<uint8_t> gw_hash;
    std::vector<uint32_t> gw_sel;
    std::vector<uint8_t> gw_ran;
    uint64_t gw_counts[GW_COLS] = {0};
    // ZKV_VM_RISC0_SETINCL (zkv_risc0_set_inclusion.h): kid[0] is the inner root verifier V -- a RISC Zero context, or (si_keyed) a generic
    // Groth16 context of the caller's key in the RISC Zero convention, whose parameters then sit in control_root_0 / _1, control_id and
    // si_root_sel.  si_roots: the submitted roots, 32 bytes each, ascending; their device copy (m_si.stored) is refreshed by the next
    // batch call after a submission (si_dirty).  m_si holds the workspace and the staging of host-buffer calls.
    bool si_keyed = false, si_dirty = false;
    uint8_t si_id[32] = {0}, si_root_sel[4] = {0}, si_set_sel[4] = {0};
    std::vector<uint8_t> si_roots;
    uint64_t si_counts[3] = {0, 0, 0};
    // ZKV_VM_RISC0_ROUTER (zkv_risc0_router.h): routes [0, rz_nb) are the instances of kid[0], a verifier set; the keyed routes behind them
    // share gw_group, a Groth16 key set of their keys (n_ic = 6, RISC Zero convention), and rz_routes holds their control parameters.
    // gw_sel / gw_hash: selector and key digest per route; kid_ran: which group ran; rz_counts: seals per route, unknown, short.
    size_t rz_nb = 0;
    std::vector<RzrRoute> rz_routes;
    std::vector<uint64_t> rz_counts;
    uint64_t rz_bad = 0;                        // bad-calldata seals of the call rz_counts describes (zkv_risc0_router_last_call_counts)
    // A router with a set route (zkv_risc0_router_set.h): the set route is the last route and is not in gw_sel -- the partition knows the
    // Groth16 routes only.  si_id, si_set_sel, si_roots and si_dirty are the set route's as they are a set-inclusion context's.
    // rzs_counts: seals per route (the set route included), unknown, short; rzs_last: zkv_risc0_router_set_last_counts.
    bool rz_set = false;
    std::vector<uint64_t> rzs_counts;
    uint64_t rzs_last[4] = {0, 0, 0, 0};
    std::mutex mu;
};

// the two PLONK kinds share the device path after the public-input step (prep kernel, G2 line tables, MSM tables, aggregate check)
static inline bool is_plonk(const zkv_ctx* c) { return c->vm == ZKV_VM_SP1_PLONK || c->vm == ZKV_VM_PLONK; }

// Proofs per chunk (= per launch of the stage kernels): ZKV_CHUNK, default 2^20, clamped to [64, 2^26].  The upper clamp is a
// correctness bound, not a tuning choice: the lane-pair kernels address their workspace rows through ONE 32-bit byte offset per lane
// (SoaRef::off = (8 * cap + i) * 4 in k_miller2), which wraps from cap = 2^32 / 36 (about 2^26.8) on; 2^26 proofs per chunk also is
// 248 GB of workspace, i.e. all of one MI355X.
static size_t chunk_capacity() {
    const char* e = getenv("ZKV_CHUNK");
    size_t c = e ? (size_t)strtoull(e, nullptr, 10) : (size_t)1 << 20;      // upper bound: the workspace is sized on demand
    if (c < 64) c = 64;
    if (c > ((size_t)1 << 26)) c = (size_t)1 << 26;
    return (c + 63) & ~(size_t)63;
}
ZKV_EXPORT size_t zkv_chunk_capacity(void) { return chunk_capacity(); }

// Chunks of at most this many proofs take the coefficient-parallel kernels (one proof per 16 lanes).  Measured (RISC Zero,
// tools/small_batch_sweep.sh, profiles/round2_g_small_batch_sweep.txt): 3.4-3.8 ms against 7.8 ms up to 4,096 proofs (one wavefront per
// SIMD), 5.6 against 7.8 ms at 8,192 (two), 7.9 against 7.9 ms from 10,240 on (a second round of wavefronts): above 8,192 the
// lane-pair kernels win because they do a third of the work per proof.
// ZKV_WIDE_BELOW=0 disables the 16-lane kernels.
// Chunks of at most this many proofs run the vk_x stage with one proof per wavefront (k_msm_w: latency instead of throughput).
// ZKV_MSM_WAVE_BELOW=0 disables it.
static size_t msm_wave_below() {
    const char* e = getenv("ZKV_MSM_WAVE_BELOW");
    return e ? (size_t)strtoull(e, nullptr, 10) : (size_t)2048;
}
// Window width of the vk_x stage's fixed-base tables: 16 (default) adds rows of 65,536 entries (4 MB each: SP1 134 MB, RISC Zero 67 MB per
// context) that halve the stage's additions; 8 keeps the L2-resident 8-bit rows only.
static int msm_window_bits() {
    const char* e = getenv("ZKV_MSM_WINDOW_BITS");
    return (e && atoi(e) == 8) ? 8 : 16;
}
static size_t wide_below() {
    const char* e = getenv("ZKV_WIDE_BELOW");
    return e ? (size_t)strtoull(e, nullptr, 10) : (size_t)12288;     // round 4 (profiles/round4_batch_sweep.txt): 16 lanes 6.9-7.2 ms against 7.3 for lane pairs up to here, 8.7 beyond
}
// One lane-pair wavefront holds 32 proofs and a SIMD holds two wavefronts: a launch of up to 32,768 proofs puts one wavefront on
// every SIMD (7.3 ms for the Miller loop and the final exponentiation together), the next 32,768 a second one (10.8 ms for both), and so
// on: T(k layers) grows by 3.5 ms from odd to even k and by 7 ms from even to odd.  A chunk of 32,768 k + r proofs with a small r would
// pay a whole layer for r proofs; instead the last r proofs take the mapping their own number selects (one or two wavefronts per proof,
// 16 lanes per proof: 2-6.4 ms alone):
//  * k odd: the last layer of the others is ONE lane-pair wavefront per SIMD, which issues at 0.74 of the rate of two -- the tail's
//    kernels run BESIDE it on the second stream (234 + 201 VGPRs fit a SIMD together): 33,792 proofs 10.7 -> 7.8 ms (9.7 with the tail
//    after the others), 36,864 10.7 -> 8.0, 40,960 10.7 -> 9.8.  Worth it up to r = ZKV_TAIL_SPLIT_BELOW (default 8,192) for one layer and
//    half of that for three and more, for chunks of up to ZKV_TAIL_SPLIT_MAX proofs (default 2^18: beyond, the odd layer is a few per
//    cent of the launch and the tail disturbs more than it fills);
//  * k even: every SIMD is full, and kernels launched beside would take register space from lane-pair wavefronts at the start and push
//    them into a layer of their own at the end -- the tail runs AFTER the others: 69,632 proofs 18.9 -> 14.2 ms, 135,168 30.0 -> 26.6,
//    263,168 50.3 -> 46.4.  Worth it up to r = ZKV_TAIL_SPLIT_EVEN_BELOW (default 12,288 = the most the 16-lane kernels take: 6.4 ms
//    against the 7 ms of a layer of lone wavefronts), any chunk size.
// ZKV_TAIL_SPLIT_BELOW=0 disables both; ZKV_TAIL_BESIDE=0 runs every tail after the others (profiles/round4_tail_beside.txt).
static bool tail_beside() {
    const char* e = getenv("ZKV_TAIL_BESIDE");
    return !(e && atoi(e) == 0);
}
static size_t tail_split_max() {
    const char* e = getenv("ZKV_TAIL_SPLIT_MAX");
    return e ? (size_t)strtoull(e, nullptr, 10) : ((size_t)1 << 18);
}
static size_t tail_split_below() {
    const char* e = getenv("ZKV_TAIL_SPLIT_BELOW");
    return e ? (size_t)strtoull(e, nullptr, 10) : (size_t)8192;
}
static size_t tail_split_even_below() {
    const char* e = getenv("ZKV_TAIL_SPLIT_EVEN_BELOW");
    return e ? (size_t)strtoull(e, nullptr, 10) : (size_t)12288;
}
// how many proofs at the end of an n-proof chunk take the small-batch mapping (0: none), and whether beside the others or after them
static size_t tail_of_chunk(size_t n, bool* beside) {
    const size_t layer = 32768, k = n / layer, r = n % layer;
    *beside = false;
    if (n <= layer || !r || !tail_split_below()) return 0;
    if (k & 1) { *beside = tail_beside(); return (n <= tail_split_max() && r <= (k == 1 ? tail_split_below() : tail_split_below() / 2)) ? r : 0; }
    return r <= tail_split_even_below() ? r : 0;
}
// The workspace rows of proofs [off, off + ...) of a chunk: word k of proof i sits at base[k * cap + i], so the same capacity with every
// base advanced by `off` elements addresses them as proofs 0, 1, ...
static Workspace ws_from(const Workspace& ws, size_t off) {
    Workspace w = ws;
    w.prep += off; w.norm += off; w.f += off; w.fe += off; w.flags += off; w.g2bad += off; if (w.gtag) w.gtag += off;
    return w;
}
// Chunks of at most this many proofs run the Miller loop and the final exponentiation with ONE PROOF PER WAVEFRONT (k_miller_w64 /
// k_finalexp_w64: four slices of 16 lanes; 1,024 proofs are one wavefront on every SIMD of the chip, 2,048 two).  Measured (RISC Zero,
// profiles/round3_e_latency_threshold_sweep.txt), one proof per wavefront against 16 lanes per proof: 1 proof 2.07 / 3.50 ms, 1,024
// proofs 2.56 / 3.65, 1,536 3.03 / 3.69, 2,048 3.61 / 3.78, 3,072 5.07 / 3.71.  ZKV_WAVE_BELOW=0 disables it.
// Chunks of at most this many proofs give the Miller loop TWO wavefronts per proof (k_miller_w64d: one steps the running point and
// tabulates the line coefficients, the other accumulates f).  Measured (RISC Zero, profiles/round3_j_dual_threshold_sweep.txt), two
// wavefronts against one per proof: 1 proof 1.69 / 2.08 ms, 128 proofs 1.90 / 2.15, 256 1.99 / 2.40, 512 2.10 / 2.49, 768 2.47 / 2.56,
// 1,024 (two wavefronts on every SIMD from the Miller kernel alone) 2.76 / 2.55.  ZKV_DUAL_BELOW=0 disables it.
static size_t dual_below() {
    const char* e = getenv("ZKV_DUAL_BELOW");
    return e ? (size_t)strtoull(e, nullptr, 10) : (size_t)768;
}
static size_t wave_below() {
    const char* e = getenv("ZKV_WAVE_BELOW");
    return e ? (size_t)strtoull(e, nullptr, 10) : (size_t)2048;
}
// The mapping policy, in its one place: lanes per proof of the Miller loop of n proofs on context c -- what the caller fixed
// (zkv_ctx_set_lanes_per_proof), else by the thresholds above: 128 (two wavefronts per proof), 64 (one), 16, or 2 (lane pairs).  Every chunk,
// tail, pseudo-proof batch and Groth16 key-set layout asks here (DESIGN.md section 11b has the table of call sites).
static int miller_lanes(const zkv_ctx* c, size_t n) {
    if (c->lanes) return c->lanes;
    if (n <= dual_below()) return 128;
    if (n <= wave_below()) return 64;
    if (n <= wide_below()) return 16;
    return 2;
}
// The single-key kernels of a mapping (launch_gset_miller is the key-set counterpart).  The final exponentiation has no two-wavefront
// kernel: 128 takes the one-wavefront one.
static void launch_miller_lanes(int lanes, size_t n, const VkTables* tab, const Workspace& ws, uint8_t* status, hipStream_t s) {
    if (lanes == 128) launch_miller_w64d(n, tab, ws, status, s);
    else if (lanes == 64) launch_miller_w64(n, tab, ws, s);
    else if (lanes == 16) launch_miller_w(n, tab, ws, s);
    else launch_miller2(n, tab, ws, status, s);
}
static void launch_finalexp_lanes(int lanes, size_t n, const Workspace& ws, uint8_t* status, hipStream_t s) {
    if (lanes == 2) launch_finalexp2(n, ws, status, s);
    else if (lanes == 16) launch_finalexp_w(n, ws, status, s);
    else launch_finalexp_w64(n, ws, status, s);
}

static bool device_is_gfx950(int dev) {
    hipDeviceProp_t p;
    if (hipGetDeviceProperties(&p, dev) != hipSuccess) return false;
    return strncmp(p.gcnArchName, "gfx950", 6) == 0;
}

ZKV_EXPORT int zkv_device_count(void) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) { (void)hipGetLastError(); return 0; }
    int ok = 0;
    for (int i = 0; i < n; i++) ok += device_is_gfx950(i) ? 1 : 0;
    return ok;
}
ZKV_EXPORT const char* zkv_version(void) { return "zkv-mi355x 0.1 (gfx950)"; }

// (x: a HIP call, or an owner's alloc() / create() -- any status other than 0 = hipSuccess = ZKV_OK)
#define HIP_TRY(x) do { if ((x) != 0) { (void)hipGetLastError(); return ZKV_ERR_HIP; } } while (0)

// Releases every device resource of the context and returns it to the "not set up" state (safe on a partially set-up context).
static void ctx_free_device(zkv_ctx* c) {
    if (!c->dev_ready && !c->stream) return;
    (void)hipSetDevice(c->device);
    static_cast<CtxDevice&>(*c) = CtxDevice();
}

static int gset_device_setup(zkv_ctx* c);
static int pset_device_setup(zkv_ctx* c);
// Lazily creates the streams, the VK tables (set-up kernels) and the events; the per-chunk workspace comes from ctx_reserve().
static int ctx_device_setup(zkv_ctx* c) {
    HIP_TRY(c->stream.create());
    for (auto& e : c->ev) HIP_TRY(e.create());
    for (auto& e : c->ev_wire) HIP_TRY(e.create());
    HIP_TRY(c->ev_done.create(hipEventDisableTiming));
    HIP_TRY(c->side.create());
    HIP_TRY(c->copy_stream.create());
    HIP_TRY(c->ev_fork.create(hipEventDisableTiming));
    HIP_TRY(c->ev_join.create(hipEventDisableTiming));
    for (auto& e : c->ev_seg) HIP_TRY(e.create(hipEventDisableTiming));
    for (int b = 0; b < 2; b++) {
        HIP_TRY(c->ev_copied[b].create(hipEventDisableTiming));
        HIP_TRY(c->ev_decoded[b].create(hipEventDisableTiming));
    }
    if (c->vm == ZKV_VM_GROTH16_SET) return gset_device_setup(c);
    if (c->vm == ZKV_VM_PLONK_SET) return pset_device_setup(c);
    if (c->vm != ZKV_VM_BN254 && c->vm != ZKV_VM_MIXED && c->vm != ZKV_VM_SP1_GATEWAY && c->vm != ZKV_VM_RISC0_SETINCL && c->vm != ZKV_VM_RISC0_ROUTER) {
        VkRaw raw;
        if (c->vm == ZKV_VM_RISC0 || c->vm == ZKV_VM_RISC0_SET) host::fill_vk_risc0(raw, c->control_root_0, c->control_root_1, c->control_id);
        else if (c->vm == ZKV_VM_GROTH16) host::fill_vk_generic(raw, c->gvk.data(), c->long_key ? 1u : c->g_n_ic);   // long key: IC[0] only here
        else if (is_plonk(c)) {
            // the pairing of a PLONK proof has two FIXED pairs: the SRS's [1]_2 and [tau]_2 take the line-table slots of gamma and
            // delta; there is no (alpha, beta) pair (alpha = infinity contributes 1) and no IC points
            memset(&raw, 0, sizeof raw);
            const int perm[4] = {1, 0, 3, 2};
            for (int k = 0; k < 4; k++) { host::be_to_limbs(raw.gamma[k], c->pk_g2 + 32 * perm[k]); host::be_to_limbs(raw.delta[k], c->pk_g2 + 128 + 32 * perm[k]); }
        }
        else host::fill_vk_sp1(raw);
        if (c->id_ge_r) memset(raw.fixed_scalar[5], 0, 32);      // never used: every proof fails the range check first
        // the raw key and the instance parameters are only read by the set-up kernels: scoped, released once those are done
        DevBuf<VkRaw> d_raw;
        DevBuf<> d_par;
        HIP_TRY(d_raw.alloc(sizeof(VkRaw)));
        HIP_TRY(c->d_tab.alloc(sizeof(VkTables)));
        HIP_TRY(hipMemsetAsync(c->d_tab, 0, sizeof(VkTables), c->stream));
        HIP_TRY(hipMemcpyAsync(d_raw, &raw, sizeof raw, hipMemcpyHostToDevice, c->stream));
        launch_setup(d_raw, c->d_tab, c->stream);
        HIP_TRY(hipGetLastError());
        if (c->long_key) {
            // IC[1..n_ic-1]: validity (folded into vk_valid) and window rows, 512 KB per signal; the raw points (d_par) only until set-up is done
            const uint32_t n_sig = c->g_n_ic - 1;
            std::vector<uint32_t> ic((size_t)16 * n_sig);
            for (uint32_t b = 0; b < n_sig; b++) {
                host::be_to_limbs(&ic[16 * (size_t)b], c->gvk.data() + 448 + 64 * (size_t)(b + 1));
                host::be_to_limbs(&ic[16 * (size_t)b + 8], c->gvk.data() + 480 + 64 * (size_t)(b + 1));
            }
            const size_t tab_bytes = (size_t)n_sig * LONG_ROW_ENTRIES * sizeof(G1A);
            HIP_TRY(d_par.alloc(sizeof(uint32_t) * ic.size()));
            HIP_TRY(c->d_ltab.alloc(tab_bytes));
            HIP_TRY(c->d_lwin.alloc(sizeof(uint32_t) * n_sig));
            HIP_TRY(hipMemsetAsync(c->d_ltab, 0, tab_bytes, c->stream));
            HIP_TRY(hipMemcpyAsync(d_par, ic.data(), sizeof(uint32_t) * ic.size(), hipMemcpyHostToDevice, c->stream));
            launch_setup_long(d_par.as<const uint32_t>(), n_sig, c->d_tab, c->d_ltab, c->d_lwin, c->stream);
            HIP_TRY(hipGetLastError());
            HIP_TRY(hipStreamSynchronize(c->stream));        // `ic` is a pageable host buffer about to go out of scope
        }
        // (a long key takes no aggregate check: its chunks run the ordinary per-proof path)
        const bool agg_vm = c->vm == ZKV_VM_RISC0 || c->vm == ZKV_VM_RISC0_SET || c->vm == ZKV_VM_SP1 || (c->vm == ZKV_VM_GROTH16 && !c->long_key);
        if (agg_vm && msm_window_bits() == 16) {
            // 16-bit window rows for the vk_x stage of big batches: 4 MB per row, built from the 8-bit rows k_setup_msm has just written
            Msm16 m = {nullptr, {0, 0, 0, 0, 0}};
            uint32_t rows = 0;
            for (uint32_t b = 0; b < raw.n_var && b < (uint32_t)MAX_VAR; b++) { m.row0[b] = rows; rows += (raw.var_windows[b] + 1) / 2; }
            if (rows && rows <= MSM16_MAX_ROWS) {
                const size_t bytes = (size_t)rows * 65536 * sizeof(G1A);
                if (c->d_msm16.alloc(bytes) == ZKV_OK) {
                    HIP_TRY(hipMemsetAsync(c->d_msm16, 0, bytes, c->stream));
                    launch_setup_msm16(c->d_tab, m, c->d_msm16, rows, c->stream);
                    HIP_TRY(hipGetLastError());
                    m.tab = c->d_msm16;
                    c->m16 = m;
                }                                                // else no room for the rows (many contexts on one device): the 8-bit walk, same results
            }
        }
        if (agg_vm || is_plonk(c)) {
            HIP_TRY(c->d_agg_cnt.alloc(3 * sizeof(unsigned long long)));
            HIP_TRY(hipMemsetAsync(c->d_agg_cnt, 0, 3 * sizeof(unsigned long long), c->stream));
        }
        if (agg_vm) {
            HIP_TRY(c->d_agg_tab.alloc(sizeof(AggTables)));
            launch_setup_agg(d_raw, c->d_tab, c->d_agg_tab, c->stream);
            HIP_TRY(hipGetLastError());
        }
        if (c->vm == ZKV_VM_RISC0_SET) {
            const size_t k = c->inst_raw.size();
            InstConsts ic;
            host::sha256_host((const uint8_t*)"risc0.Groth16ReceiptVerifierParameters", 38, ic.tag);
            host::risc0_vk_digest(ic.vk_digest);
            HIP_TRY(d_par.alloc(sizeof(InstRaw) * k));
            InstRaw* d_in = d_par.as<InstRaw>();
            HIP_TRY(c->d_inst.alloc(sizeof(InstTab) * k));
            HIP_TRY(hipMemcpyAsync(d_in, c->inst_raw.data(), sizeof(InstRaw) * k, hipMemcpyHostToDevice, c->stream));
            launch_setup_instances(d_raw, ic, d_in, c->d_inst, (uint32_t)k, c->stream);
            HIP_TRY(hipGetLastError());
            c->inst_host.resize(k);
            HIP_TRY(hipMemcpyAsync(c->inst_host.data(), c->d_inst, sizeof(InstTab) * k, hipMemcpyDeviceToHost, c->stream));
        }
        if (is_plonk(c)) {
            HIP_TRY(d_par.alloc(sizeof(PlonkKeyRaw)));
            HIP_TRY(c->d_pkey.alloc(sizeof(PlonkKey)));
            HIP_TRY(hipMemcpyAsync(d_par, &c->pk_raw, sizeof(PlonkKeyRaw), hipMemcpyHostToDevice, c->stream));
            if (c->vm == ZKV_VM_PLONK) launch_plonk_setup_keys(d_par.as<const PlonkKeyRaw>(), c->d_pkey, c->stream);
            else launch_plonk_setup(d_par.as<const PlonkKeyRaw>(), c->d_pkey, c->stream);
            HIP_TRY(hipGetLastError());
        }
        HIP_TRY(hipStreamSynchronize(c->stream));
        d_raw.release(); d_par.release();
        uint32_t valid = 0;
        HIP_TRY(hipMemcpy(&valid, &c->d_tab->vk_valid, sizeof valid, hipMemcpyDeviceToHost));
        c->vk_invalid = valid == 0;
        if (c->d_agg_tab) {
            uint32_t ok = 0;
            HIP_TRY(hipMemcpy(&ok, &c->d_agg_tab->ok, sizeof ok, hipMemcpyDeviceToHost));
            c->agg_key_ok = ok != 0;
        }
        if (is_plonk(c)) c->agg_key_ok = !c->vk_invalid;      // (no (alpha, beta) pair: nothing else to tabulate)
        if (c->vm == ZKV_VM_PLONK) {
            // the key's own validity (points, size_inv / generator / coset_shift < R) was judged by k_plonk_setup
            uint32_t kv = 0;
            HIP_TRY(hipMemcpy(&kv, &c->d_pkey->valid, sizeof kv, hipMemcpyDeviceToHost));
            if (!kv) { c->vk_invalid = true; c->agg_key_ok = false; }
        }
    }
    return ZKV_OK;
}
static int ctx_device_init(zkv_ctx* c) {
    if (c->dev_ready) return hipSetDevice(c->device) == hipSuccess ? ZKV_OK : ZKV_ERR_HIP;
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n <= 0) { (void)hipGetLastError(); return ZKV_ERR_NO_DEVICE; }
    if (c->device < 0 || c->device >= n || !device_is_gfx950(c->device)) return ZKV_ERR_NO_DEVICE;
    HIP_TRY(hipSetDevice(c->device));
    const int rc = ctx_device_setup(c);
    if (rc != ZKV_OK) { ctx_free_device(c); return rc; }       // a failed set-up leaves nothing behind; the next call starts over
    c->ws.cap = 0;                                       // per-chunk buffers: ctx_reserve()
    c->dev_ready = true;
    return ZKV_OK;
}

// Per-chunk buffers (3.7 KB of workspace per proof in flight) are sized by the largest batch seen so far, rounded up to a power
// of two, at most ZKV_CHUNK (default 2^20) proofs: a context that only ever verifies single proofs stays small, a 2^20-proof
// batch runs as one chunk (larger launches amortise kernel tails: 4.12 M proofs/s at 2^18 per chunk against 4.00 at 2^17).
// Growing frees the old buffers, which synchronises the device, so work in flight on them has finished.
// Buffers of the aggregate check, sized with the workspace (about 0.9 KB per proof in flight on top of its 3.7 KB): 224 B of rows per proof, one
// pseudo-proof workspace per 16 proofs (the smallest sub-batch), and the dense workspace of the second pass (own PREP rows, flags, statuses, index list).
static int agg_reserve(zkv_ctx* c) {
    if (!c->agg_on || !c->agg_key_ok || c->agg_cap >= c->ws.cap) return ZKV_OK;
    AggMem& g = *c;
    g = AggMem();
    // room for the smallest sub-batch size; a key set pads its pseudo-proofs per key up to 1.25 times (gset_choose in run_gset) and runs
    // its second pass in place (k_gset_agg_mark): no dense workspace, no index list
    const bool set = c->vm == ZKV_VM_GROTH16_SET || c->vm == ZKV_VM_PLONK_SET;     // (a PLONK set pads per SRS class: run_pset)
    const size_t cap = c->ws.cap, cap2 = (cap + 15) / 16 + (set ? (cap + 63) / 64 : 0);
    if (g.d_agg.alloc(sizeof(uint32_t) * WS_AGG_WORDS * cap) || g.ws2_prep.alloc(sizeof(uint32_t) * WS_PREP_WORDS * cap2) ||
        g.ws2_norm.alloc(sizeof(uint32_t) * WS_NORM_WORDS * cap2) || g.ws2_f.alloc(sizeof(uint32_t) * WS_F_WORDS * cap2) ||
        g.ws2_fe.alloc(sizeof(uint32_t) * WS_FE_WORDS * cap2) || g.ws2_flags.alloc(sizeof(uint32_t) * cap2) ||
        g.ws2_g2bad.alloc(sizeof(uint32_t) * cap2) || g.d_status2.alloc(cap2) ||
        (!set && (g.ws3_prep.alloc(sizeof(uint32_t) * WS_PREP_WORDS * cap) || g.ws3_flags.alloc(sizeof(uint32_t) * cap) ||
                  g.ws3_g2bad.alloc(sizeof(uint32_t) * cap) || g.d_status3.alloc(cap) || g.d_agg_idx.alloc(sizeof(uint32_t) * cap)))) {
        // no room for the extra 0.9 KB per proof in flight: the chunk takes the ordinary kernels (enqueue_chunk looks at agg_cap)
        g = AggMem();
        return ZKV_OK;
    }
    g.ws2 = Workspace{g.ws2_prep, g.ws2_norm, g.ws2_f, g.ws2_fe, g.ws2_flags, g.ws2_g2bad, cap2};
    if (!set) g.ws3 = Workspace{g.ws3_prep, c->ws.norm, c->ws.f, c->ws.fe, g.ws3_flags, g.ws3_g2bad, cap};
    g.agg_cap = cap;
    return ZKV_OK;
}
static int ctx_reserve(zkv_ctx* c, size_t want) {
    const size_t limit = chunk_capacity();
    if (want > limit) want = limit;
    if (want <= c->ws.cap) return agg_reserve(c);
    size_t cap = 4096;
    while (cap < want) cap <<= 1;
    if (cap > limit) cap = limit;
    ChunkMem& m = *c;
    m = ChunkMem();
    if (m.ws_prep.alloc(sizeof(uint32_t) * WS_PREP_WORDS * cap) || m.ws_norm.alloc(sizeof(uint32_t) * WS_NORM_WORDS * cap) ||
        m.ws_f.alloc(sizeof(uint32_t) * WS_F_WORDS * cap) || m.ws_fe.alloc(sizeof(uint32_t) * WS_FE_WORDS * cap) ||
        m.ws_flags.alloc(sizeof(uint32_t) * cap) || m.ws_g2bad.alloc(sizeof(uint32_t) * cap) || m.ws_gtag.alloc(cap) ||
        m.d_a.alloc(32 * cap) || m.d_b.alloc(32 * cap) || m.d_status.alloc(cap) || m.d_recv.alloc(4 * cap) ||
        m.d_off.alloc(sizeof(uint64_t) * (cap + 1)) || m.d_pvoff.alloc(sizeof(uint64_t) * (cap + 1)) ||
        m.d_inst_idx.alloc(sizeof(uint32_t) * cap) || m.d_len.alloc(sizeof(uint32_t) * cap) || m.d_pvlen.alloc(sizeof(uint32_t) * cap) ||
        m.d_kind.alloc(cap) || m.d_cdoff[0].alloc(sizeof(uint64_t) * (cap + 1)) || m.d_cdoff[1].alloc(sizeof(uint64_t) * (cap + 1)) ||
        ((is_plonk(c) || c->vm == ZKV_VM_PLONK_SET) && m.d_plonk_tab.alloc(sizeof(uint32_t) * PLONK_TAB_WORDS * cap))) {
        m = ChunkMem();                                      // (at once: the survivors of a failed reserve are of no use to anyone)
        return ZKV_ERR_OOM;
    }
    m.ws = Workspace{m.ws_prep, m.ws_norm, m.ws_f, m.ws_fe, m.ws_flags, m.ws_g2bad, cap, m.ws_gtag};
    return agg_reserve(c);
}
// Fixed-base GT tables (zkv_gt.h) for the (vk_x, gamma) pairing of an SP1 or RISC Zero context: 2^19 entries of 384 bytes per signed 20-bit
// window of each per-proof signal -- SP1 2 x 13 windows = 5.2 GB, RISC Zero 2 x 7 = 2.8 GB per context.  ZKV_GT_WINDOW_BITS=0 switches them
// off; ZKV_GT_MAX_BYTES bounds what a context may take for them.  A context without them (switched off, over the bound, or no room on the
// device) keeps the pair in the Miller loop: same statuses.
// ZKV_GT_WINDOW_BITS: "0" switches the tables off, "20" (the only width built) or unset keeps them; anything else is refused at the first
// call that would build them (ZKV_ERR_INVALID_ARG) rather than read as one of the two.
static int gt_window_bits() {
    const char* e = getenv("ZKV_GT_WINDOW_BITS");
    if (!e || !strcmp(e, "20")) return (int)GT_WINDOW_BITS;
    return !strcmp(e, "0") ? 0 : -1;
}
// ZKV_GT_CACHE: "0" leaves an SP1 context without the walk-prefix cache (zkv_gt.h), anything else or unset keeps it.
static bool gt_cache_wanted() {
    const char* e = getenv("ZKV_GT_CACHE");
    return !e || strcmp(e, "0") != 0;
}
static size_t gt_max_bytes() {
    const char* e = getenv("ZKV_GT_MAX_BYTES");
    return e ? (size_t)strtoull(e, nullptr, 10) : ~(size_t)0;
}
// Built the first time a call of n proofs can run lane-pair chunks (the only kernels that read them), after the workspace: contexts
// that only ever see small batches never pay for them.
// One attempt per context (gt_tried): a context that had no room then keeps the Miller path for its life, and tables once built stay
// until the context is destroyed.
static int gt_maybe_build(zkv_ctx* c, size_t n) {
    if (c->gt_tried || (c->vm != ZKV_VM_SP1 && c->vm != ZKV_VM_RISC0) || c->vk_invalid || !c->d_tab) return ZKV_OK;
    const size_t per = n < chunk_capacity() ? n : chunk_capacity();
    if (!(c->lanes == 2 || (c->lanes == 0 && per > wide_below()))) return ZKV_OK;
    const int bits = gt_window_bits();
    if (bits < 0) return ZKV_ERR_INVALID_ARG;
    c->gt_tried = true;
    if (bits == 0) return ZKV_OK;
    VkRaw raw;
    if (c->vm == ZKV_VM_RISC0) host::fill_vk_risc0(raw, c->control_root_0, c->control_root_1, c->control_id);
    else host::fill_vk_sp1(raw);
    if (raw.n_var != GT_MAX_SIG || !raw.var_windows[0] || !raw.var_windows[1]) return ZKV_OK;
    const uint32_t nw0 = gt_windows(8 * raw.var_windows[0]), nw1 = gt_windows(8 * raw.var_windows[1]), rows = nw0 + nw1;
    if (nw0 > GT_MAX_WINDOWS || nw1 > GT_MAX_WINDOWS) return ZKV_OK;
    const size_t bytes = (size_t)rows * GT_ROW_BYTES;
    if (bytes > gt_max_bytes()) return ZKV_OK;
    DevBuf<VkRaw> d_raw; DevBuf<uint32_t> d_scr;
    DevEvent e0, e1;
    bool ok = c->d_gt.alloc(bytes) == ZKV_OK && c->d_gt_const.alloc(sizeof(uint32_t) * 2 * GT_ENTRY_WORDS) == ZKV_OK &&      // the folded constant, and the loop's start value made of it
              miller_start_exponent_ok() &&                                            // 2^64 h invertible mod r, e its inverse (zkv_verify.h)
              d_raw.alloc(sizeof(VkRaw)) == ZKV_OK && d_scr.alloc(sizeof(uint32_t) * GT_SETUP_SCRATCH_WORDS) == ZKV_OK &&
              e0.create() == ZKV_OK && e1.create() == ZKV_OK;
    if (ok) {
        ok = hipMemcpyAsync(d_raw, &raw, sizeof raw, hipMemcpyHostToDevice, c->stream) == hipSuccess;
        (void)hipEventRecord(e0, c->stream);
        launch_gt_bases(d_raw, c->d_tab, c->d_gt, c->d_gt_const, d_scr, nw0, nw1, c->stream);
        for (uint32_t level = 1; level < GT_WINDOW_BITS; level++) launch_gt_level(c->d_gt, rows, level, c->stream);
        launch_gt_torus(c->d_gt, rows, c->stream);               // every entry to its affine torus value: what the walk multiplies by
        (void)hipEventRecord(e1, c->stream);
        ok = ok && hipGetLastError() == hipSuccess && hipStreamSynchronize(c->stream) == hipSuccess;
        if (ok) (void)hipEventElapsedTime(&c->gt_build_ms, e0, e1);
    }
    (void)hipGetLastError();
    d_raw.release(); d_scr.release();
    if (!ok) {                                                // no room (or a failed launch): the Miller path, same results
        c->d_gt.release(); c->d_gt_const.release();
        return ZKV_OK;
    }
    c->gt = GtTab{c->d_gt, c->d_gt_const, {nw0, nw1}, nullptr};
    c->gt_bytes = bytes;
    // the walk-prefix cache: SP1 only (signal 0 is the program vkey).  No room for its 2 KB: the context walks every window, same results.
    if (c->vm == ZKV_VM_SP1 && gt_cache_wanted()) {
        GtCache head = {};
        head.entries = GT_CACHE_ENTRIES;
        if (c->d_gt_cache.alloc(sizeof(GtCache)) == ZKV_OK && hipMemset(c->d_gt_cache, 0, sizeof(GtCache)) == hipSuccess &&
            hipMemcpy(c->d_gt_cache, &head, 4 * sizeof(uint32_t), hipMemcpyHostToDevice) == hipSuccess) c->gt.cache = c->d_gt_cache;
        else { (void)hipGetLastError(); c->d_gt_cache.release(); }
    }
    return ZKV_OK;
}
// device set-up + buffers for a batch of n
// verify == false: a call that runs no verification kernels (zkv_ctx_vk_x_batch) -- it never reads the GT tables and does not build them
static int ctx_ready(zkv_ctx* c, size_t n, bool verify = true) {
    int rc = ctx_device_init(c);
    if (rc == ZKV_OK) rc = ctx_reserve(c, n ? n : 1);
    if (rc == ZKV_OK && verify) rc = gt_maybe_build(c, n ? n : 1);
    return rc;
}

// Cross-stream ordering of consecutive calls on one context (see zkv_ctx::ev_done).
static int order_after_previous(zkv_ctx* c, hipStream_t s) {
    if (c->has_done) HIP_TRY(hipStreamWaitEvent(s, c->ev_done, 0));
    c->agg_look = true;
    return ZKV_OK;
}
static int mark_done(zkv_ctx* c, hipStream_t s) {
    HIP_TRY(hipEventRecord(c->ev_done, s));
    c->has_done = true;
    return ZKV_OK;
}

// Chunks of at least this many proofs take the aggregate check when it is switched on.  Measured (SP1, tools/bench_aggregate.py,
// profiles/round3_t_aggregate_sizes.txt), aggregate / ordinary, all proofs valid: 2^14 7.4 / 8.2 ms, 2^15 8.0 / 8.4, 2^16 10.7 / 13.4,
// 2^17 16.6 / 24.6, 2^18 29.6 / 47.3, 2^20 104 / 183; one proof in 64 rejected (a fifth of those at the pairing): 2^16 19.1 / 13.4,
// 2^17 25.3 / 24.6, 2^18 40.0 / 47.4, 2^20 121 / 182 -- the pseudo-proofs and the second pass over failed sub-batches each cost a
// kernel latency, which small chunks cannot hide.  ZKV_AGG_MIN overrides.
static size_t agg_min() {
    const char* e = getenv("ZKV_AGG_MIN");
    size_t v = e ? (size_t)strtoull(e, nullptr, 10) : (size_t)131072;
    return v < 64 ? 64 : v;
}
// Proofs per Miller accumulator in the aggregate check (k_agg_miller; 1 = k_miller2, an accumulator per proof).  ZKV_AGG_GROUP overrides;
// a sub-batch must hold at least two groups.
static uint32_t agg_group(uint32_t sub) {
    const char* e = getenv("ZKV_AGG_GROUP");
    uint32_t g = e ? (uint32_t)strtoul(e, nullptr, 10) : 4u;
    if (g != 1 && g != 2 && g != 4 && g != 8) g = 4;
    while (g > 1 && sub / g < 2) g >>= 1;
    return g;
}
// enable = 1 ("automatic"): before a chunk is enqueued, and only if everything enqueued earlier on this context has finished (no
// waiting), the counters tell which fraction of the sub-batches checked since the last look failed; from it the rate p of proofs that
// fail at the pairing, and from p the size for the coming chunks: a failed sub-batch costs its `sub` proofs a second, ordinary
// verification, a sub-batch costs one pseudo-proof: per proof 1 / sub + sub p in units of one verification, least near sub = 1 / sqrt(p).
// Measured (2^20 SP1 proofs): no failures 128 best (87 ms; 91.5 at 64), one proof in 320 failing 16 best (109 ms; 133 at 64).
//
// Switching OFF: at the smallest size a sub-batch that fails costs its 16 proofs the aggregate pass AND the ordinary pass; from about one
// failing sub-batch in three on the check is a net loss (measured: the aggregate pass is ~0.6 of an ordinary one at size 16), and a
// stream of bad proofs would make it a slow-down knob.  Above that rate the following AGG_PAUSE_MIN (then twice as many, up to
// AGG_PAUSE_MAX) chunks run without the check; the chunk after a pause probes again with size 16, and the check stays on once the
// rate has fallen.  Only the automatic mode (enable = 1) does any of this: a caller that fixes the size keeps it.
constexpr uint32_t AGG_PAUSE_MIN = 8, AGG_PAUSE_MAX = 64;
// One look per call, at its start: ev_done is recorded once per call, so a later chunk of the same call could see the event of the
// PREVIOUS call complete while its own earlier chunk is still adding to the two counters.
static void agg_adapt(zkv_ctx* c) {
    if (!c->agg_look) return;
    c->agg_look = false;
    if (!c->agg_auto || !c->has_done || !c->d_agg_cnt || hipEventQuery(c->ev_done) != hipSuccess) { (void)hipGetLastError(); return; }
    unsigned long long v[2];                                   // (on the context's side stream, idle here: waits neither for the caller's streams nor for the
                                                               // host pipeline's segment copies on copy_stream)
    if (hipMemcpyAsync(v, c->d_agg_cnt, sizeof v, hipMemcpyDeviceToHost, c->side) != hipSuccess || hipStreamSynchronize(c->side) != hipSuccess) {
        (void)hipGetLastError();
        return;
    }
    if (c->agg_resnap) { c->agg_seen[0] = v[0]; c->agg_seen[1] = v[1]; c->agg_resnap = false; return; }
    const unsigned long long checked = v[0] - c->agg_seen[0], failed = v[1] - c->agg_seen[1];
    if (checked < 256) return;                                 // too little to go by
    c->agg_seen[0] = v[0]; c->agg_seen[1] = v[1];
    const double f = (double)failed / (double)checked;         // P(a sub-batch of agg_sub proofs holds a failing proof) = 1 - (1 - p)^sub
    const double p = f >= 1.0 ? 1.0 : 1.0 - pow(1.0 - f, 1.0 / (double)c->agg_sub);
    const uint32_t was = c->agg_sub;
    c->agg_sub = p < 1.0 / 32768 ? 128u : p < 1.0 / 4096 ? 64u : p < 1.0 / 1024 ? 32u : 16u;
    // what size 16 would see with this p: 1 - (1 - p)^16
    const double f16 = was == 16u ? f : 1.0 - pow(1.0 - p, 16.0);
    if (f16 > 1.0 / 3.0) {
        c->agg_pause_len = c->agg_pause_len ? (2 * c->agg_pause_len > AGG_PAUSE_MAX ? AGG_PAUSE_MAX : 2 * c->agg_pause_len) : AGG_PAUSE_MIN;
        c->agg_pause = c->agg_pause_len;
        c->agg_sub = 16u;                                     // the probe after the pause
    } else c->agg_pause_len = 0;
}
// Whether this chunk takes the aggregate check (automatic mode: not during a pause).
static bool agg_wanted(zkv_ctx* c) {
    agg_adapt(c);                                             // (once per call: the decision covers this chunk already)
    if (c->agg_auto && c->agg_pause) { c->agg_pause--; return false; }
    return true;
}
// Fresh coefficients for every chunk (the counter), and a fresh SECRET every AGG_REKEY_CHUNKS chunks when the operating system supplied it
// (zkv_ctx_set_aggregate_check with seed32 = NULL): nothing a long-running service has revealed about old coefficients -- timing, say --
// carries over.  A caller-supplied seed is the caller's responsibility (include/zkv.h).
constexpr uint32_t AGG_REKEY_CHUNKS = 1024;
static uint32_t agg_rekey_chunks() {
    const char* e = getenv("ZKV_AGG_REKEY");                    // tests shorten the interval
    const unsigned long v = e ? strtoul(e, nullptr, 10) : 0;
    return v ? (uint32_t)v : AGG_REKEY_CHUNKS;
}
static void agg_next_coefficients(zkv_ctx* c) {
    if (c->agg_os_seed && ++c->agg_key_age >= agg_rekey_chunks()) {
        uint8_t seed[32];
        if (getrandom(seed, 32, 0) == 32) {
            for (int i = 0; i < 8; i++) c->agg_seed.w[i] = ((uint32_t)seed[4 * i] << 24) | ((uint32_t)seed[4 * i + 1] << 16) | ((uint32_t)seed[4 * i + 2] << 8) | seed[4 * i + 3];
            c->agg_key_age = 0;
        }
        volatile uint8_t* wipe = seed;
        for (int i = 0; i < 32; i++) wipe[i] = 0;
    }
    c->agg_seed.call++;
}
// The aggregate check of one chunk (zkv_agg.h), after PREP: per-proof G1 stage and Miller loop of the variable pair only, one
// pseudo-proof per sub-batch through the ordinary Miller loop and final exponentiation, then the ordinary stages once more for the
// proofs of sub-batches that failed, gathered into a dense workspace (the launches cover the whole chunk -- the host does not know how
// many there are -- and wavefronts past the end of the list leave at once).
static void enqueue_agg(zkv_ctx* c, const PrepArgs& a, hipStream_t s, bool timed) {
    agg_adapt(c);
    const uint32_t sub = c->agg_sub, sub64 = sub < 64 ? sub : 64;        // sub-batches of 128 / 256 proofs are summed per 64-proof block first
    const size_t n64 = (a.n + 63) / 64;
    const size_t n2 = sub > 64 ? (a.n + sub - 1) / sub : n64 * (64 / sub);      // the last block counted in full (empty sub-batches switch themselves off)
    // proofs per Miller accumulator: ZKV_AGG_GROUP = 1 (k_miller2), 2, 4 or 8 (k_agg_miller); at most the sub-batch's eighth... see agg_group()
    const uint32_t grp = agg_group(sub64);
    const int lanes2 = miller_lanes(c, n2);                   // the pseudo-proofs' mapping (automatic: the check runs only with c->lanes == 0)
    const InstTab* inst = a.inst ? c->d_inst : nullptr;
    agg_next_coefficients(c);
    // vk_x through summed scalars: one key (no per-proof base) and at most two per-proof signals
    const bool sums = !inst && (c->vm == ZKV_VM_RISC0 || c->vm == ZKV_VM_SP1 || (c->vm == ZKV_VM_GROTH16 && c->g_n_ic >= 1 && c->g_n_ic - 1 <= (uint32_t)AGG_SUM_VARS));
    launch_agg_g1(a.n, c->d_tab, inst, c->ws, c->d_agg, c->agg_seed, sums, s);
    if (timed) { (void)hipEventRecord(c->ev[2], s); (void)hipEventRecord(c->ev[3], s); }
    if (grp > 1) launch_agg_miller(a.n, grp, c->d_tab, c->ws, a.status, s);
    else launch_miller2(a.n, c->d_tab, c->ws, a.status, s);
    launch_agg_reduce(a.n, sub64, sums, grp, c->d_tab, c->ws, c->d_agg, c->d_agg_tab, c->ws2, c->d_status2, sub > 64, s);
    if (sub > 64) launch_agg_combine(n64, n2, sub / 64, c->d_agg_tab, c->ws2, c->d_status2, s);
    launch_miller_lanes(lanes2, n2, c->d_tab, c->ws2, c->d_status2, s);
    if (timed) (void)hipEventRecord(c->ev[4], s);
    launch_agg_fprod(a.n, n2, sub, grp, c->ws, c->d_agg, c->ws2, s);
    launch_finalexp_lanes(lanes2, n2, c->ws2, c->d_status2, s);
    launch_agg_mark(a.n, sub, grp, c->ws, c->d_agg, c->d_status2, a.status, c->d_agg_cnt, c->d_agg_idx, s);
    launch_agg_gather(a.n, c->ws, c->d_agg, c->d_agg_cnt, c->d_agg_idx, c->ws3, c->d_status3, s);
    launch_msm(a.n, c->d_tab, c->m16, inst, c->ws3, s);
    launch_miller2(a.n, c->d_tab, c->ws3, c->d_status3, s);
    launch_finalexp2(a.n, c->ws3, c->d_status3, s);
    launch_agg_scatter(a.n, c->d_agg_cnt, c->d_agg_idx, c->d_status3, a.status, s);
    if (timed) (void)hipEventRecord(c->ev[5], s);
}

// The aggregate check of a PLONK chunk, after the unchanged PREP stage (k_agg_plonk_g1 explains why there is no per-proof Miller loop).
static void enqueue_agg_plonk(zkv_ctx* c, const PrepArgs& a, hipStream_t s, bool timed) {
    agg_adapt(c);
    const uint32_t sub = c->agg_sub, sub64 = sub < 64 ? sub : 64;
    const size_t n64 = (a.n + 63) / 64;
    const size_t n2 = sub > 64 ? (a.n + sub - 1) / sub : n64 * (64 / sub);
    const int lanes2 = miller_lanes(c, n2);
    agg_next_coefficients(c);
    launch_agg_plonk_g1(a.n, c->ws, c->d_agg, c->agg_seed, s);
    if (timed) { (void)hipEventRecord(c->ev[2], s); (void)hipEventRecord(c->ev[3], s); }
    launch_agg_reduce(a.n, sub64, false, 1, c->d_tab, c->ws, c->d_agg, nullptr, c->ws2, c->d_status2, sub > 64, s);
    if (sub > 64) launch_agg_combine(n64, n2, sub / 64, nullptr, c->ws2, c->d_status2, s);
    launch_miller_lanes(lanes2, n2, c->d_tab, c->ws2, c->d_status2, s);
    if (timed) (void)hipEventRecord(c->ev[4], s);
    launch_finalexp_lanes(lanes2, n2, c->ws2, c->d_status2, s);
    launch_agg_mark(a.n, sub, 1, c->ws, c->d_agg, c->d_status2, a.status, c->d_agg_cnt, c->d_agg_idx, s);
    launch_agg_plonk_norm(a.n, c->ws, c->d_agg, c->d_agg_cnt, c->d_agg_idx, c->ws3, c->d_status3, s);
    launch_miller2(a.n, c->d_tab, c->ws3, c->d_status3, s);
    launch_finalexp2(a.n, c->ws3, c->d_status3, s);
    launch_agg_scatter(a.n, c->d_agg_cnt, c->d_agg_idx, c->d_status3, a.status, s);
    if (timed) (void)hipEventRecord(c->ev[5], s);
}

// Long keys (LongKey): the table walk of a chunk of n proofs runs with G lanes per proof -- 64 up to ZKV_MSM_WAVE_BELOW proofs (one proof
// per wavefront, as k_msm_w), 16 below ZKV_LONG_LANE_BELOW (default 2^18: a chunk of fewer proofs has too few wavefronts with one lane
// per proof to fill the chip -- 2^18 proofs are four per SIMD -- while 32 (n_ic - 1) / G additions per lane stay far above the 4 of the
// butterfly), one lane per proof above.  zkv_ctx_set_lanes_per_proof fixes it: 2 -> 1, 16 -> 16, 64 / 128 -> 64.
static uint32_t msm_lanes_long(const zkv_ctx* c, size_t n) {
    if (c->lanes) return c->lanes == 2 ? 1u : c->lanes == 16 ? 16u : 64u;
    if (n <= msm_wave_below()) return 64;
    const char* e = getenv("ZKV_LONG_LANE_BELOW");
    return n < (e ? (size_t)strtoull(e, nullptr, 10) : ((size_t)1 << 18)) ? 16u : 1u;
}
// proofs the staged-signal rows of a long key or a key set have room for (= their row stride): d_lsig holds 32 bytes per signal and proof
static size_t lsig_stride(const zkv_ctx* c) { return c->g_n_ic > 1 ? c->d_lsig.cap() / ((size_t)32 * (c->g_n_ic - 1)) : 0; }
static LongKey long_key_of(const zkv_ctx* c) { return LongKey{c->d_ltab, c->d_lwin, c->d_lsig, lsig_stride(c), c->g_n_ic - 1}; }

// Enqueues the five stages for one chunk (all pointers device-resident).
static void enqueue_chunk(zkv_ctx* c, const PrepArgs& a, hipStream_t s, bool timed) {
    c->last_chunk_n = a.n;
    if (timed) (void)hipEventRecord(c->ev[0], s);
    if (is_plonk(c)) {
        // PLONK: the prep stage does everything up to the two G1 points of the final check (transcript, scalar algebra, MSMs);
        // no per-proof G2 point, so no subgroup check, and no vk_x stage
        PrepArgs ap = a;
        ap.plonk_tab = c->d_plonk_tab;
        if (c->vm == ZKV_VM_PLONK) launch_plonk_prep_keys(ap, c->d_pkey, c->ws, s);
        else launch_plonk_prep(ap, c->d_pkey, c->ws, s);
        if (c->agg_on && c->agg_key_ok && c->agg_cap >= c->ws.cap && c->lanes == 0 && a.n >= agg_min() && agg_wanted(c)) {
            if (timed) (void)hipEventRecord(c->ev[1], s);
            enqueue_agg_plonk(c, a, s, timed);
            return;
        }
        if (timed) { (void)hipEventRecord(c->ev[1], s); (void)hipEventRecord(c->ev[2], s); (void)hipEventRecord(c->ev[3], s); }
        int pl = miller_lanes(c, a.n);
        if (pl == 128) pl = 64;                              // (no variable pair: nothing for a second wavefront to do)
        launch_miller_lanes(pl, a.n, c->d_tab, c->ws, a.status, s);
        if (timed) (void)hipEventRecord(c->ev[4], s);
        launch_finalexp_lanes(pl, a.n, c->ws, a.status, s);
        if (timed) (void)hipEventRecord(c->ev[5], s);
        return;
    }
    if (c->vm == ZKV_VM_RISC0 || c->vm == ZKV_VM_RISC0_SET) launch_prep_risc0(a, c->consts, c->ws, s);
    else if (c->vm == ZKV_VM_GROTH16 && c->long_key) launch_prep_groth16_long(a, c->ws, c->d_lsig, lsig_stride(c), s);
    else if (c->vm == ZKV_VM_GROTH16) launch_prep_groth16(a, c->ws, s);
    else launch_prep_sp1(a, c->ws, s);
    if (timed) (void)hipEventRecord(c->ev[1], s);
    if (c->agg_on && c->agg_key_ok && c->agg_cap >= c->ws.cap && c->lanes == 0 && a.n >= agg_min() && agg_wanted(c)) { enqueue_agg(c, a, s, timed); return; }
    bool tail_runs_beside = false;
    const size_t tail = c->lanes == 0 ? tail_of_chunk(a.n, &tail_runs_beside) : 0;
    if (tail) {
        // all proofs through the vk_x stage, then the Miller loops and final exponentiations of the first a.n - tail proofs on lane pairs and
        // of the last `tail` through their own small-batch mapping (whose Miller kernels leave the subgroup test of B to k_g2chk2)
        const size_t head = a.n - tail;
        const Workspace wt = ws_from(c->ws, head);
        const bool gt = c->gt.tab != nullptr;               // the head's (vk_x, gamma) pairing comes from the GT tables: no window walk for it
        if (c->long_key) launch_msm_long(a.n, msm_lanes_long(c, a.n), c->d_tab, long_key_of(c), c->ws, s);
        else if (gt) {
            launch_msm(head, c->d_tab, c->m16, nullptr, c->ws, s, true);
            launch_msm(tail, c->d_tab, c->m16, nullptr, wt, s);
        }
        else launch_msm(a.n, c->d_tab, c->m16, a.inst ? c->d_inst : nullptr, c->ws, s);
        if (timed) (void)hipEventRecord(c->ev[2], s);
        // the tail's kernels on the second stream beside the lane-pair kernels of the others (odd number of layers), or after them
        // (tail_of_chunk); disjoint workspace rows and status bytes either way
        const bool beside = tail_runs_beside && c->side != nullptr;
        hipStream_t st = beside ? c->side : s;
        if (beside) { (void)hipEventRecord(c->ev_fork, s); (void)hipStreamWaitEvent(c->side, c->ev_fork, 0); }
        launch_g2chk2(tail, wt, a.status + head, st);
        if (timed) (void)hipEventRecord(c->ev[3], s);
        if (gt) launch_gt_cache(head, c->ws, s, c->gt);
        launch_miller2(head, c->d_tab, c->ws, a.status, s, c->gt.mconst);
        const int tl = miller_lanes(c, tail);                // (automatic: a fixed mapping takes no tail split)
        launch_miller_lanes(tl, tail, c->d_tab, wt, a.status + head, st);
        if (timed) (void)hipEventRecord(c->ev[4], s);
        launch_finalexp2(head, c->ws, a.status, s, c->gt);
        launch_finalexp_lanes(tl, tail, wt, a.status + head, st);
        if (beside) { (void)hipEventRecord(c->ev_join, c->side); (void)hipStreamWaitEvent(s, c->ev_join, 0); }
        if (timed) (void)hipEventRecord(c->ev[5], s);
        return;
    }
    // 2 = one proof per lane pair; 16 = one proof per 16 lanes (small chunks); 64 = per wavefront (smaller); 128 = two wavefronts per proof
    // in the Miller loop (smallest)
    const int lanes = miller_lanes(c, a.n);
    const bool wide = lanes != 2;
    const bool gt = !wide && c->gt.tab != nullptr;           // lane pairs with GT tables (zkv_gt.h): no vk_x walk, no (vk_x, gamma) trip in the Miller loop
    // Lane-pair kernels: the Miller loop itself is the subgroup test of B (miller_loop_p), there is no separate check; stage time
    // [2] is then 0.  16-lane kernels (small chunks, most of the chip idle): the check (k_g2chk2) only needs the PREP output and only
    // its verdict (ws.g2bad; the MSM owns ws.flags) is needed, by the final exponentiation, so it runs on a second stream beside the
    // MSM and the Miller loop, which is computed speculatively for the rare proof whose B fails the check (-0.7 ms).
    const bool fork = wide && c->side != nullptr;
    if (fork) {
        (void)hipEventRecord(c->ev_fork, s);
        (void)hipStreamWaitEvent(c->side, c->ev_fork, 0);
        launch_g2chk2(a.n, c->ws, a.status, c->side);
        (void)hipEventRecord(c->ev_join, c->side);
    }
    if (c->long_key) launch_msm_long(a.n, msm_lanes_long(c, a.n), c->d_tab, long_key_of(c), c->ws, s);
    else if (gt) launch_msm(a.n, c->d_tab, c->m16, nullptr, c->ws, s, true);
    else if (a.n <= msm_wave_below()) launch_msm_w(a.n, c->d_tab, a.inst ? c->d_inst : nullptr, c->ws, s);     // one proof per wavefront
    else launch_msm(a.n, c->d_tab, c->m16, a.inst ? c->d_inst : nullptr, c->ws, s);
    if (timed) (void)hipEventRecord(c->ev[2], s);
    if (wide && !fork) launch_g2chk2(a.n, c->ws, a.status, s);
    if (timed) (void)hipEventRecord(c->ev[3], s);
    if (gt) { launch_gt_cache(a.n, c->ws, s, c->gt); launch_miller2(a.n, c->d_tab, c->ws, a.status, s, c->gt.mconst); }
    else launch_miller_lanes(lanes, a.n, c->d_tab, c->ws, a.status, s);
    if (timed) (void)hipEventRecord(c->ev[4], s);
    if (fork) (void)hipStreamWaitEvent(s, c->ev_join, 0);     // the final exponentiation reads the verdict of the subgroup check
    if (gt) launch_finalexp2(a.n, c->ws, a.status, s, c->gt);
    else launch_finalexp_lanes(lanes, a.n, c->ws, a.status, s);
    if (timed) (void)hipEventRecord(c->ev[5], s);
}

// Offsets handed over by the caller must be non-decreasing: the kernels index the blob with them.
static bool offsets_ok(const uint64_t* off, size_t n) {
    for (size_t i = 0; i < n; i++) if (off[i + 1] < off[i]) return false;
    return true;
}
static uint32_t be32_of(const uint8_t* p) { return ((uint32_t)p[0] << 24) | ((uint32_t)p[1] << 16) | ((uint32_t)p[2] << 8) | p[3]; }
static void be32_put(uint8_t* p, uint32_t v) { p[0] = (uint8_t)(v >> 24); p[1] = (uint8_t)(v >> 16); p[2] = (uint8_t)(v >> 8); p[3] = (uint8_t)v; }

// Host-pointer batch driver shared by risc0 verify / verify_integrity / sp1 verify_proof.
//
// The whole batch (at most 2^22 proofs per pass) is staged in HBM; the copies run on the context's copy stream SEGMENT BY SEGMENT
// while the previous segment is being verified: a short first segment (2^16 proofs: its 25 MB cross PCIe in about a millisecond),
// then segments of up to one workspace (2^20 proofs) whose H2D time hides behind the kernels of the segment before.  Statuses
// stay on the device until the pass is done.  Only the first segment's copy and the status D2H are exposed.
static size_t host_first_segment(size_t n, size_t cap) {
    const char* e = getenv("ZKV_HOST_FIRST_SEGMENT");
    size_t v = e ? (size_t)strtoull(e, nullptr, 10) : (size_t)1 << 16;
    if (v < 64) v = 64;
    if (n <= 2 * v) v = n;
    return v < cap ? v : cap;
}
static int run_host_batch(zkv_ctx* c, size_t n, const uint8_t* blob, const uint64_t* off, const uint8_t* in_a, const uint8_t* in_b,
                          const uint8_t* pv_blob, const uint64_t* pv_off, uint8_t* status, uint8_t* recv) {
    if (!c || (n && (!blob || !off || !status || !in_a))) return ZKV_ERR_INVALID_ARG;
    if (n && (!offsets_ok(off, n) || (pv_off && !offsets_ok(pv_off, n)))) return ZKV_ERR_INVALID_ARG;
    if (recv) memset(recv, 0, 4 * n);
    if (c->vm == ZKV_VM_RISC0 && !c->initialized) {              // risc0/verifier.rs:84-86, 99-101
        memset(status, ZKV_STATUS_INVALID_INITIALIZATION, n);
        return ZKV_OK;
    }
    if (!n) return ZKV_OK;
    std::lock_guard<std::mutex> lk(c->mu);
    int rc = ctx_ready(c, n);
    if (rc != ZKV_OK) return rc;
    const char* pe = getenv("ZKV_HOST_PASS");                   // proofs staged per pass (tests shrink it to reach the multi-pass loop)
    const size_t cap = c->ws.cap, pass_max = pe && strtoull(pe, nullptr, 10) ? (size_t)strtoull(pe, nullptr, 10) : (size_t)1 << 22;
    const bool sp1 = c->vm == ZKV_VM_SP1 || c->vm == ZKV_VM_SP1_PLONK;
    if ((rc = order_after_previous(c, c->stream)) != ZKV_OK) return rc;
    std::vector<uint64_t> rel, prel;
    for (size_t p0 = 0; p0 < n; p0 += pass_max) {
        const size_t pn = n - p0 < pass_max ? n - p0 : pass_max;
        const uint64_t s0 = off[p0], sbytes = off[p0 + pn] - s0;
        const uint64_t v0 = sp1 ? pv_off[p0] : 0, vbytes = sp1 ? pv_off[p0 + pn] - v0 : 0;
        // growing a buffer frees the old one, which synchronises the device: everything is sized before the first copy
        HostBatchMem& hb = c->m_host;
        if ((rc = grow_all(hb.seals, (size_t)sbytes + 8, hb.off, 8 * (pn + 1), hb.in_a, 32 * pn)) != ZKV_OK ||
            (in_b && (rc = hb.in_b.grow(32 * pn)) != ZKV_OK) ||
            (sp1 && (rc = grow_all(hb.pv, (size_t)vbytes + 8, hb.pv_off, 8 * (pn + 1))) != ZKV_OK) ||
            (rc = grow_all(c->d_st_all, pn, c->d_rv_all, 4 * pn)) != ZKV_OK) return rc;
        // offsets relative to the pass (the caller's array is used as it is when the pass starts at offset 0)
        const uint64_t* o = off + p0; const uint64_t* po = sp1 ? pv_off + p0 : nullptr;
        if (s0) { rel.resize(pn + 1); for (size_t i = 0; i <= pn; i++) rel[i] = off[p0 + i] - s0; o = rel.data(); }
        if (sp1 && v0) { prel.resize(pn + 1); for (size_t i = 0; i <= pn; i++) prel[i] = pv_off[p0 + i] - v0; po = prel.data(); }
        const size_t first = host_first_segment(pn, cap);
        // ZKV_HOST_TRACE=1 (diagnostic): events around the segments' copies and kernels, printed to stderr after the pass
        const bool trace = getenv("ZKV_HOST_TRACE") != nullptr;
        std::vector<DevEvent> tev;
        auto mark = [&](hipStream_t st) { if (!trace) return; DevEvent e; if (e.create() == ZKV_OK) { (void)hipEventRecord(e, st); tev.push_back(std::move(e)); } };
        mark(c->stream);
        for (size_t base = 0, k = 0; base < pn; k++) {
            // (a third, intermediate segment of 2 * first was measured and dropped: 202.6 against 200.7 ms per 2^20 SP1 proofs,
            // alternating runs on one box)
            const size_t m = k == 0 ? first : (pn - base < cap ? pn - base : cap);
            hipStream_t cs = c->copy_stream;
            HIP_TRY(hipMemcpyAsync(hb.off + base, o + base, 8 * (m + 1), hipMemcpyHostToDevice, cs));
            if (o[base + m] > o[base]) HIP_TRY(hipMemcpyAsync(hb.seals + o[base], blob + s0 + o[base], (size_t)(o[base + m] - o[base]), hipMemcpyHostToDevice, cs));
            HIP_TRY(hipMemcpyAsync(hb.in_a + 32 * base, in_a + 32 * (p0 + base), 32 * m, hipMemcpyHostToDevice, cs));
            if (in_b) HIP_TRY(hipMemcpyAsync(hb.in_b + 32 * base, in_b + 32 * (p0 + base), 32 * m, hipMemcpyHostToDevice, cs));
            if (sp1) {
                HIP_TRY(hipMemcpyAsync(hb.pv_off + base, po + base, 8 * (m + 1), hipMemcpyHostToDevice, cs));
                if (po[base + m] > po[base]) HIP_TRY(hipMemcpyAsync(hb.pv + po[base], pv_blob + v0 + po[base], (size_t)(po[base + m] - po[base]), hipMemcpyHostToDevice, cs));
            }
            HIP_TRY(hipEventRecord(c->ev_seg[k & 1], cs));
            mark(cs);
            HIP_TRY(hipStreamWaitEvent(c->stream, c->ev_seg[k & 1], 0));
            PrepArgs a;
            memset(&a, 0, sizeof a);
            a.n = m; a.blob = hb.seals; a.off = hb.off + base; a.stride = 0;
            a.in32_a = hb.in_a + 32 * base; a.in32_b = in_b ? hb.in_b + 32 * base : nullptr;
            if (sp1) {
                a.pv_blob = hb.pv; a.pv_off = hb.pv_off + base;
                a.selector_be = be32_of(c->vm == ZKV_VM_SP1_PLONK ? c->plonk_hash : host::SP1_VERIFIER_HASH);
                a.force_fail = c->vm == ZKV_VM_SP1_PLONK && c->vk_invalid ? 1u : 0u;
            } else {
                a.selector_be = be32_of(c->selector);
                a.force_fail = c->id_ge_r ? 1u : 0u;
            }
            a.status = c->d_st_all + base; a.recv = c->d_rv_all + 4 * base;
            base += m;
            enqueue_chunk(c, a, c->stream, base >= pn);
            mark(c->stream);
            HIP_TRY(hipGetLastError());
        }
        HIP_TRY(hipMemcpyAsync(status + p0, c->d_st_all, pn, hipMemcpyDeviceToHost, c->stream));
        if (recv) HIP_TRY(hipMemcpyAsync(recv + 4 * p0, c->d_rv_all, 4 * pn, hipMemcpyDeviceToHost, c->stream));
        mark(c->stream);
        HIP_TRY(hipStreamSynchronize(c->stream));            // also: the staging buffers are free for the next pass
        if (trace && tev.size() > 1) {
            fprintf(stderr, "zkv host pass of %zu proofs (first segment %zu): events [start, (copy done, kernels done) per segment, statuses back], ms since start:", pn, first);
            for (size_t i = 1; i < tev.size(); i++) { float ms = 0; (void)hipEventElapsedTime(&ms, tev[0], tev[i]); fprintf(stderr, " %.2f", ms); }
            fprintf(stderr, "\n");
        }
    }
    return ZKV_OK;
}

// Device-pointer fast path (fixed stride), asynchronous on `stream`.
static int run_dev_batch(zkv_ctx* c, size_t n, const uint8_t* d_blob, const uint8_t* d_a, const uint8_t* d_b, const uint8_t* d_pv,
                         size_t pv_len, uint8_t* d_status, uint8_t* d_recv, void* stream) {
    if (!c || (n && (!d_blob || !d_a || !d_status))) return ZKV_ERR_INVALID_ARG;
    std::lock_guard<std::mutex> lk(c->mu);
    int rc = ctx_ready(c, n);
    if (rc != ZKV_OK) return rc;
    hipStream_t s = stream ? (hipStream_t)stream : c->stream;
    if (c->vm == ZKV_VM_RISC0 && !c->initialized) {
        HIP_TRY(hipMemsetAsync(d_status, ZKV_STATUS_INVALID_INITIALIZATION, n, s));
        if (d_recv) HIP_TRY(hipMemsetAsync(d_recv, 0, 4 * n, s));
        return ZKV_OK;
    }
    size_t cap = c->ws.cap;
    if (n && (rc = order_after_previous(c, s)) != ZKV_OK) return rc;
    for (size_t base = 0; base < n; base += cap) {
        size_t m = n - base < cap ? n - base : cap;
        PrepArgs a;
        memset(&a, 0, sizeof a);
        const size_t rec = c->vm == ZKV_VM_SP1_PLONK ? (size_t)ZKV_PLONK_PROOF_BYTES : (size_t)ZKV_SEAL_BYTES;
        a.n = m; a.blob = d_blob + base * rec; a.off = nullptr; a.stride = (uint32_t)rec;
        a.in32_a = d_a + 32 * base; a.in32_b = d_b ? d_b + 32 * base : nullptr;
        if (c->vm == ZKV_VM_SP1 || c->vm == ZKV_VM_SP1_PLONK) {
            a.pv_blob = d_pv + base * pv_len; a.pv_off = nullptr; a.pv_stride = (uint32_t)pv_len;
            a.selector_be = be32_of(c->vm == ZKV_VM_SP1_PLONK ? c->plonk_hash : host::SP1_VERIFIER_HASH);
            a.force_fail = c->vm == ZKV_VM_SP1_PLONK && c->vk_invalid ? 1u : 0u;
        } else {
            a.selector_be = be32_of(c->selector);
            a.force_fail = c->id_ge_r ? 1u : 0u;
        }
        a.status = d_status + base; a.recv = d_recv ? d_recv + 4 * base : nullptr;
        enqueue_chunk(c, a, s, base + cap >= n);
    }
    HIP_TRY(hipGetLastError());
    return n ? mark_done(c, s) : ZKV_OK;
}

// Stage pipeline over m compact records that a device-side front end produced (fixed stride plus the true length, 32-byte inputs,
// public values as (start, length) into one blob): the output format of the calldata decoder, of the mixed-batch demultiplexer and of
// the SP1 gateway.  The stride is 260 bytes, 868 for an SP1 PLONK context.  `kind` (RISC Zero, may be null): per-proof method,
// 1 = verify_integrity.  Asynchronous on `s`.
static int run_records(zkv_ctx* c, size_t m_total, const uint8_t* seals, const uint32_t* len, const uint8_t* in_a, const uint8_t* in_b,
                       const uint8_t* kind, const uint8_t* pv_blob, const uint64_t* pv_start, const uint32_t* pv_len, uint8_t* st, uint8_t* rv, hipStream_t s) {
    if (!m_total) return ZKV_OK;
    std::lock_guard<std::mutex> lk(c->mu);
    int rc = ctx_ready(c, m_total);
    if (rc != ZKV_OK) return rc;
    if ((rc = order_after_previous(c, s)) != ZKV_OK) return rc;
    const size_t cap = c->ws.cap;
    const size_t rec = c->vm == ZKV_VM_SP1_PLONK ? (size_t)ZKV_PLONK_PROOF_BYTES : (size_t)ZKV_SEAL_BYTES;
    for (size_t base = 0; base < m_total; base += cap) {
        const size_t m = m_total - base < cap ? m_total - base : cap;
        PrepArgs a;
        memset(&a, 0, sizeof a);
        a.n = m; a.blob = seals + base * rec; a.stride = (uint32_t)rec; a.len = len + base;
        a.in32_a = in_a + 32 * base;
        if (c->vm == ZKV_VM_SP1) {
            a.pv_blob = pv_blob; a.pv_off = pv_start + base; a.pv_len = pv_len + base;
            a.selector_be = be32_of(host::SP1_VERIFIER_HASH);
        } else if (c->vm == ZKV_VM_SP1_PLONK) {
            a.pv_blob = pv_blob; a.pv_off = pv_start + base; a.pv_len = pv_len + base;
            a.selector_be = be32_of(c->plonk_hash);
            a.force_fail = c->vk_invalid ? 1u : 0u;
        } else {
            a.in32_b = in_b + 32 * base; a.kind = kind ? kind + base : nullptr;
            a.selector_be = be32_of(c->selector);
            a.force_fail = c->id_ge_r ? 1u : 0u;
        }
        a.status = st + base; a.recv = rv ? rv + 4 * base : nullptr;
        enqueue_chunk(c, a, s, base + cap >= m_total);
    }
    HIP_TRY(hipGetLastError());
    return mark_done(c, s);
}

// ------------------------------------------------------------------ sharded (multi-device) contexts (SURVEY 8b `device_mask`, 8e)
// One single-device context per shard behind the ordinary batch entry points; proofs are independent, so a batch splits into
// contiguous ranges and nothing is exchanged between shards.  Host-buffer batches: one host thread per shard calls the single-device
// entry point on its range of the caller's buffers, so every GPU pulls its rows over its own PCIe link (no bounce through a root
// GPU).  Device-resident batches: rows are copied from the GPU that holds them to each shard's GPU with hipMemcpyPeerAsync (one direct
// xGMI link per peer) in two pieces -- the second piece travels behind the first piece's kernels -- and the statuses return the same way.
static inline bool is_sharded(const zkv_ctx* c) { return c && !c->shards.empty(); }
static size_t env_size(const char* name, size_t dflt) {
    const char* e = getenv(name);
    return e && *e ? (size_t)strtoull(e, nullptr, 10) : dflt;
}
// shards that get work: at least ZKV_SHARD_MIN (default 1,024) proofs each -- a single proof stays on one GPU
static size_t shards_used(const zkv_ctx* c, size_t n) {
    size_t mn = env_size("ZKV_SHARD_MIN", 1024);
    if (mn < 1) mn = 1;
    size_t k = (n + mn - 1) / mn;
    if (k < 1) k = 1;
    return k < c->shards.size() ? k : c->shards.size();
}
static inline void shard_range(size_t n, size_t used, size_t k, size_t* lo, size_t* hi) {      // contiguous, remainder to the low shards
    const size_t q = n / used, r = n % used;
    *lo = k * q + (k < r ? k : r);
    *hi = *lo + q + (k < r ? 1 : 0);
}
// per_shard(child, lo, hi) -> ZKV_*; shard 0 runs on the calling thread
// fn(k) for the shards 1 .. used - 1 on their persistent workers and for shard 0 on the calling thread; returns when all are done.
template <class F> static void shard_parallel(zkv_ctx* c, size_t used, F fn) {
    std::lock_guard<std::mutex> pool(c->pool_mu);
    while (c->workers.size() + 1 < used) {
        std::unique_ptr<zkv_ctx::ShardWorker> w(new zkv_ctx::ShardWorker());
        try { w->th = std::thread([p = w.get()] { p->loop(); }); } catch (const std::system_error&) { break; }     // no thread to be had: that shard runs here
        c->workers.push_back(std::move(w));
    }
    const size_t pooled = c->workers.size() + 1 < used ? c->workers.size() + 1 : used;
    for (size_t k = 1; k < pooled; k++) c->workers[k - 1]->submit([&fn, k] { fn(k); });
    fn(0);
    for (size_t k = pooled; k < used; k++) fn(k);
    for (size_t k = 1; k < pooled; k++) c->workers[k - 1]->wait();
}
static void shard_workers_stop(zkv_ctx* c) {
    for (auto& w : c->workers) {
        { std::lock_guard<std::mutex> lk(w->m); w->quit = true; }
        w->cv.notify_all();
        if (w->th.joinable()) w->th.join();
    }
    c->workers.clear();
}
template <class F> static int run_sharded(zkv_ctx* c, size_t n, F per_shard) {
    const size_t used = shards_used(c, n);
    std::vector<int> rc(used, ZKV_OK);
    shard_parallel(c, used, [&](size_t k) { size_t lo, hi; shard_range(n, used, k, &lo, &hi); rc[k] = per_shard(c->shards[k], lo, hi); });
    for (int r : rc) if (r != ZKV_OK) return r;
    return ZKV_OK;
}
static int shard_dev_setup(zkv_ctx::ShardDev& d, int device) {
    if (d.run) return ZKV_OK;
    HIP_TRY(hipSetDevice(device));
    HIP_TRY(d.run.create());
    HIP_TRY(d.copy.create());
    for (auto& e : d.ev_piece) HIP_TRY(e.create(hipEventDisableTiming));
    HIP_TRY(d.ev_done.create(hipEventDisableTiming));
    return ZKV_OK;
}
struct DevRow { const uint8_t* p; size_t stride; };
// child_call(child, m, rows[n_rows <= 5] (device pointers on the child's GPU), status, recv (may be null), stream) -> ZKV_*
template <class F>
static int run_sharded_dev(zkv_ctx* c, size_t n, const DevRow* rows, int n_rows, uint8_t* d_status, uint8_t* d_recv, void* stream, F child_call) {
    if (!n) return ZKV_OK;
    if (n_rows < 1 || n_rows > 5) return ZKV_ERR_INVALID_ARG;
    hipPointerAttribute_t at;
    if (hipPointerGetAttributes(&at, rows[0].p) != hipSuccess) { (void)hipGetLastError(); return ZKV_ERR_INVALID_ARG; }
    const int sdev = at.device;
    int ndev = 0;
    HIP_TRY(hipGetDeviceCount(&ndev));
    if (sdev < 0 || sdev >= ndev) return ZKV_ERR_INVALID_ARG;
    std::lock_guard<std::mutex> lk(c->mu);
    if (c->ev_in.size() < (size_t)ndev) c->ev_in.resize(ndev);
    hipStream_t caller = (hipStream_t)stream;
    if (caller) {                                     // the shards' streams start after what the caller's stream has enqueued so far
        HIP_TRY(hipSetDevice(sdev));
        if (!c->ev_in[sdev]) HIP_TRY(c->ev_in[sdev].create(hipEventDisableTiming));
        HIP_TRY(hipEventRecord(c->ev_in[sdev], caller));
    }
    const size_t used = shards_used(c, n);
    const bool force = env_size("ZKV_SHARD_FORCE_STAGING", 0) != 0;         // tests: take the peer-copy path on a one-GPU box
    // first piece of a staged range: ZKV_SHARD_FIRST_PIECE when set, else half the range for ranges of at least 2^17 proofs (small
    // launches run the stage kernels below their rate, which costs more than the transfer a smaller first piece would hide)
    const size_t first_env = env_size("ZKV_SHARD_FIRST_PIECE", 0);
    std::vector<int> rc(used, ZKV_OK);
    auto one = [&](size_t k) -> int {
        zkv_ctx* kid = c->shards[k];
        zkv_ctx::ShardDev& d = c->sh[k];
        size_t lo, hi; shard_range(n, used, k, &lo, &hi);
        const size_t m = hi - lo;
        if (!m) return ZKV_OK;
        int r = shard_dev_setup(d, kid->device);
        if (r != ZKV_OK) return r;
        HIP_TRY(hipSetDevice(kid->device));
        const bool staged = force || kid->device != sdev;
        if (caller) { HIP_TRY(hipStreamWaitEvent(d.run, c->ev_in[sdev], 0)); HIP_TRY(hipStreamWaitEvent(d.copy, c->ev_in[sdev], 0)); }
        if (staged) {
            if (kid->device != sdev) {                             // direct xGMI copies where the platform allows; the verdict is kept for zkv_ctx_shard_peer_access
                const hipError_t pe = hipDeviceEnablePeerAccess(sdev, 0);
                (void)hipGetLastError();
                d.peer = (pe == hipSuccess || pe == hipErrorPeerAccessAlreadyEnabled) ? 1 : 0;
            }
            // the staging rows are about to be overwritten: not before the previous call's kernels on this shard have read them (that call may
            // have been enqueued on another caller stream, or with none, and still be running)
            if (d.has_done) HIP_TRY(hipStreamWaitEvent(d.copy, d.ev_done, 0));
            for (int j = 0; j < n_rows; j++) if ((r = d.row[j].grow(m * rows[j].stride + 8)) != ZKV_OK) return r;
            if ((r = d.st.grow(m)) != ZKV_OK || (d_recv && (r = d.rv.grow(4 * m)) != ZKV_OK)) return r;
        }
        // two pieces: the first (at most `first` proofs) is what the kernels wait for, the rest travels behind its kernels
        size_t pc[3] = {0, m, m};
        int np = 1;
        const size_t first = first_env ? first_env : (m >= ((size_t)1 << 17) ? m / 2 : 0);
        if (staged && first && m >= 2 * first) { pc[1] = first; np = 2; }
        if (staged) {
            for (int q = 0; q < np; q++) {
                for (int j = 0; j < n_rows; j++)
                    HIP_TRY(hipMemcpyPeerAsync(d.row[j] + pc[q] * rows[j].stride, kid->device, rows[j].p + (lo + pc[q]) * rows[j].stride, sdev,
                                               (pc[q + 1] - pc[q]) * rows[j].stride, d.copy));
                HIP_TRY(hipEventRecord(d.ev_piece[q], d.copy));
            }
        }
        for (int q = 0; q < np; q++) {
            const uint8_t* rp[5] = {nullptr, nullptr, nullptr, nullptr, nullptr};
            for (int j = 0; j < n_rows; j++) rp[j] = (staged ? d.row[j] : rows[j].p + lo * rows[j].stride) + pc[q] * rows[j].stride;
            if (staged) HIP_TRY(hipStreamWaitEvent(d.run, d.ev_piece[q], 0));
            uint8_t* st = (staged ? d.st : d_status + lo) + pc[q];
            uint8_t* rv = d_recv ? (staged ? d.rv : d_recv + 4 * lo) + 4 * pc[q] : nullptr;
            if ((r = child_call(kid, pc[q + 1] - pc[q], rp, st, rv, d.run)) != ZKV_OK) return r;
            HIP_TRY(hipSetDevice(kid->device));
        }
        if (staged) {
            HIP_TRY(hipMemcpyPeerAsync(d_status + lo, sdev, d.st, kid->device, m, d.run));
            if (d_recv) HIP_TRY(hipMemcpyPeerAsync(d_recv + 4 * lo, sdev, d.rv, kid->device, 4 * m, d.run));
        }
        HIP_TRY(hipEventRecord(d.ev_done, d.run));
        d.has_done = true;
        return ZKV_OK;
    };
    shard_parallel(c, used, [&](size_t k) { rc[k] = one(k); });
    for (int r : rc) if (r != ZKV_OK) return r;
    if (caller) {                                     // ... and the caller's stream continues after every shard has delivered its statuses
        HIP_TRY(hipSetDevice(sdev));
        for (size_t k = 0; k < used; k++) { size_t lo, hi; shard_range(n, used, k, &lo, &hi); if (hi > lo) HIP_TRY(hipStreamWaitEvent(caller, c->sh[k].ev_done, 0)); }
    }
    return ZKV_OK;
}
static void shards_free(zkv_ctx* c) {
    shard_workers_stop(c);
    for (size_t k = 0; k < c->sh.size(); k++) {
        zkv_ctx::ShardDev& d = c->sh[k];
        if (!d.run) continue;
        (void)hipSetDevice(c->shards[k]->device);
        (void)hipStreamSynchronize(d.run); (void)hipStreamSynchronize(d.copy);
        d = zkv_ctx::ShardDev();
    }
    c->ev_in.clear();
    for (auto& k : c->shards) { if (k) zkv_ctx_destroy(k); k = nullptr; }
    c->shards.clear(); c->sh.clear();
}
ZKV_EXPORT zkv_ctx* zkv_ctx_create_sharded(zkv_ctx* const* shards, size_t n_shards) {
    if (!shards || !n_shards || n_shards > 64) return nullptr;
    for (size_t k = 0; k < n_shards; k++) {
        const zkv_ctx* s = shards[k];
        if (!s || is_sharded(s) || s->vm != shards[0]->vm) return nullptr;
        for (size_t j = 0; j < k; j++) if (shards[j] == s) return nullptr;
        if (s->vm != ZKV_VM_RISC0 && s->vm != ZKV_VM_SP1 && s->vm != ZKV_VM_MIXED && s->vm != ZKV_VM_GROTH16 && s->vm != ZKV_VM_SP1_PLONK &&
            s->vm != ZKV_VM_PLONK) return nullptr;
        // shards of one verifier: the same parameters everywhere (the host-visible state of shard 0 answers the getters)
        if (!s->initialized || memcmp(s->selector, shards[0]->selector, 4) || memcmp(s->control_id, shards[0]->control_id, 32) ||
            s->gvk != shards[0]->gvk || s->g_n_ic != shards[0]->g_n_ic || s->g_negate != shards[0]->g_negate || s->long_key != shards[0]->long_key ||
            memcmp(s->plonk_hash, shards[0]->plonk_hash, 32)) return nullptr;
        if (is_plonk(s) && (memcmp(&s->pk_raw, &shards[0]->pk_raw, sizeof s->pk_raw) || memcmp(s->pk_g2, shards[0]->pk_g2, sizeof s->pk_g2))) return nullptr;
        if (s->vm == ZKV_VM_MIXED && memcmp(s->kid[0]->selector, shards[0]->kid[0]->selector, 4)) return nullptr;
    }
    zkv_ctx* c = new (std::nothrow) zkv_ctx();
    if (!c) return nullptr;
    const zkv_ctx* s0 = shards[0];
    c->vm = s0->vm; c->device = s0->device; c->initialized = s0->initialized; c->id_ge_r = s0->id_ge_r;
    memcpy(c->control_root_0, s0->control_root_0, 16); memcpy(c->control_root_1, s0->control_root_1, 16);
    memcpy(c->control_id, s0->control_id, 32); memcpy(c->selector, s0->selector, 4);
    c->consts = s0->consts; c->g_n_ic = s0->g_n_ic; c->g_negate = s0->g_negate; c->gvk = s0->gvk; c->long_key = s0->long_key;
    memcpy(c->plonk_hash, s0->plonk_hash, 32);
    c->pk_raw = s0->pk_raw; memcpy(c->pk_g2, s0->pk_g2, sizeof c->pk_g2);
    c->shards.assign(shards, shards + n_shards);
    c->sh.resize(n_shards);
    return c;
}
ZKV_EXPORT size_t zkv_ctx_shard_count(const zkv_ctx* c) { return c ? c->shards.size() : 0; }
ZKV_EXPORT int zkv_ctx_shard_device(const zkv_ctx* c, size_t k) { return c && k < c->shards.size() ? c->shards[k]->device : ZKV_ERR_INVALID_ARG; }
// one shard per set bit of device_mask (bit d = HIP device d), lowest device first
template <class Mk> static zkv_ctx* create_multi(uint64_t device_mask, Mk mk) {
    std::vector<zkv_ctx*> kids;
    for (int d = 0; d < 64; d++) {
        if (!((device_mask >> d) & 1u)) continue;
        zkv_ctx* k = mk(d);
        if (!k) { for (auto* x : kids) zkv_ctx_destroy(x); return nullptr; }
        kids.push_back(k);
    }
    if (kids.empty()) return nullptr;
    zkv_ctx* c = zkv_ctx_create_sharded(kids.data(), kids.size());
    if (!c) for (auto* x : kids) zkv_ctx_destroy(x);
    return c;
}
ZKV_EXPORT zkv_ctx* zkv_risc0_ctx_create_multi(const uint8_t control_root[32], const uint8_t bn254_control_id[32], uint64_t device_mask) {
    if (!control_root || !bn254_control_id) return nullptr;
    return create_multi(device_mask, [&](int d) { return zkv_risc0_ctx_create(control_root, bn254_control_id, d); });
}
ZKV_EXPORT zkv_ctx* zkv_sp1_ctx_create_multi(uint64_t device_mask) { return create_multi(device_mask, [](int d) { return zkv_sp1_ctx_create(d); }); }
ZKV_EXPORT zkv_ctx* zkv_mixed_ctx_create_multi(const uint8_t control_root[32], const uint8_t bn254_control_id[32], uint64_t device_mask) {
    if (!control_root || !bn254_control_id) return nullptr;
    return create_multi(device_mask, [&](int d) { return zkv_mixed_ctx_create(control_root, bn254_control_id, d); });
}
// The end of a host-buffer call: n statuses and (recv != nullptr) received selectors from d_st / d_rv, and the call's wait.
static int return_to_host(const DevBuf<uint8_t>& d_st, const DevBuf<uint8_t>& d_rv, size_t n, uint8_t* status, uint8_t* recv, hipStream_t s) {
    HIP_TRY(hipMemcpyAsync(status, d_st, n, hipMemcpyDeviceToHost, s));
    if (recv) HIP_TRY(hipMemcpyAsync(recv, d_rv, 4 * n, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    return ZKV_OK;
}

// ------------------------------------------------------------------ mixed batches: per-proof VMType (common/types.rs:24-26)
ZKV_EXPORT zkv_ctx* zkv_mixed_ctx_create(const uint8_t control_root[32], const uint8_t bn254_control_id[32], int device) {
    if (!control_root || !bn254_control_id) return nullptr;
    zkv_ctx* c = new (std::nothrow) zkv_ctx();
    if (!c) return nullptr;
    c->vm = ZKV_VM_MIXED; c->device = device; c->initialized = true;
    memset(&c->consts, 0, sizeof c->consts);
    c->kid[0] = zkv_risc0_ctx_create(control_root, bn254_control_id, device);
    c->kid[1] = zkv_sp1_ctx_create(device);
    if (!c->kid[0] || !c->kid[1]) { zkv_ctx_destroy(c); return nullptr; }
    return c;
}
ZKV_EXPORT zkv_ctx* zkv_mixed_ctx_risc0(zkv_ctx* c) { if (is_sharded(c)) c = c->shards[0]; return c && c->vm == ZKV_VM_MIXED ? c->kid[0] : nullptr; }
ZKV_EXPORT zkv_ctx* zkv_mixed_ctx_sp1(zkv_ctx* c) { if (is_sharded(c)) c = c->shards[0]; return c && c->vm == ZKV_VM_MIXED ? c->kid[1] : nullptr; }

// Everything device-resident; `seal_off` / `b_off` select the ragged layout, otherwise fixed strides; `d_method` (may be null: all
// ZKV_METHOD_VERIFY) is the per-proof method.  Synchronises `s` once, after the partition, to learn the two sub-batch sizes.
static int run_mixed(zkv_ctx* c, size_t n, const uint8_t* d_vm, const uint8_t* d_method, const uint8_t* d_seals, const uint64_t* d_seal_off, uint32_t seal_stride,
                     const uint8_t* d_a, const uint8_t* d_b, const uint64_t* d_b_off, uint32_t b_stride, uint32_t pv_len,
                     uint8_t* d_status, uint8_t* d_recv, hipStream_t s) {
    int rc;
    const size_t blocks = (n + 255) / 256;
    MixedMem& mm = c->m_mixed;
    if ((rc = grow_all(mm.cnt, 8 * blocks, mm.totals, 8, mm.pos, 4 * n, mm.idx, 4 * n, mm.recs, (size_t)ZKV_SEAL_BYTES * n, mm.len, 4 * n, mm.a, 32 * n,
                       mm.b, 32 * n, mm.pvoff, 8 * n, mm.pvlen, 4 * n, mm.st, n, mm.rv, 4 * n, mm.kind, n)) != ZKV_OK) return rc;
    if ((rc = order_after_previous(c, s)) != ZKV_OK) return rc;
    MixedArgs a;
    memset(&a, 0, sizeof a);
    a.n = n; a.vm = d_vm; a.method = d_method; a.seals = d_seals; a.seal_off = d_seal_off; a.seal_stride = seal_stride;
    a.in_a = d_a; a.in_b = d_b; a.b_off = d_b_off; a.b_stride = b_stride; a.pv_len = pv_len;
    a.cnt = mm.cnt; a.totals = mm.totals; a.pos = mm.pos; a.idx = mm.idx; a.c_seals = mm.recs; a.c_len = mm.len; a.c_a = mm.a; a.c_b = mm.b;
    a.c_pvoff = mm.pvoff; a.c_pvlen = mm.pvlen; a.c_kind = mm.kind;
    a.status = d_status; a.recv = d_recv;
    launch_mixed_partition(a, mm.cnt, mm.totals, s);
    HIP_TRY(hipGetLastError());
    uint32_t tot[2] = {0, 0};
    HIP_TRY(hipMemcpyAsync(tot, mm.totals, sizeof tot, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    const size_t n0 = tot[0], n1 = tot[1];
    if (n0 + n1 > n) return ZKV_ERR_HIP;
    c->kid_ran[0] = n0 > 0; c->kid_ran[1] = n1 > 0;
    uint8_t *st = mm.st, *rv = mm.rv;
    if ((rc = run_records(c->kid[0], n0, a.c_seals, a.c_len, a.c_a, a.c_b, d_method ? a.c_kind : nullptr, nullptr, nullptr, nullptr, st, rv, s)) != ZKV_OK) return rc;
    if ((rc = run_records(c->kid[1], n1, a.c_seals + ZKV_SEAL_BYTES * n0, a.c_len + n0, a.c_a + 32 * n0, nullptr, nullptr, d_b, a.c_pvoff + n0, a.c_pvlen + n0,
                          st + n0, rv + 4 * n0, s)) != ZKV_OK) return rc;
    HIP_TRY(hipSetDevice(c->device));
    launch_mixed_return(n0 + n1, a.idx, st, rv, d_status, d_recv, s);
    HIP_TRY(hipGetLastError());
    return mark_done(c, s);
}
ZKV_EXPORT int zkv_mixed_verify_call_batch_dev(zkv_ctx* c, size_t n, const uint8_t* d_vm, const uint8_t* d_method, const uint8_t* d_seals,
                                               const uint8_t* d_in_a, const uint8_t* d_in_b, size_t b_stride, size_t pv_len, uint8_t* d_status,
                                               uint8_t* d_recv, void* stream) {
    if (!c || c->vm != ZKV_VM_MIXED) return ZKV_ERR_WRONG_CTX;
    if (n && (!d_vm || !d_seals || !d_in_a || !d_in_b || !d_status || b_stride < 32 || pv_len > b_stride || b_stride > 0xFFFFFFFFu)) return ZKV_ERR_INVALID_ARG;
    if (!n) return ZKV_OK;
    if (n > 0xFFFFFFF0u) return ZKV_ERR_INVALID_ARG;
    if (is_sharded(c)) {
        // the method row travels with the others (one byte per proof); without one the shards get none either
        const DevRow rows[5] = {{d_vm, 1}, {d_seals, ZKV_SEAL_BYTES}, {d_in_a, 32}, {d_in_b, b_stride}, {d_method, 1}};
        return run_sharded_dev(c, n, rows, d_method ? 5 : 4, d_status, d_recv, stream,
                               [&](zkv_ctx* k, size_t m, const uint8_t* const* r, uint8_t* st, uint8_t* rv, hipStream_t s) {
            return zkv_mixed_verify_call_batch_dev(k, m, r[0], d_method ? r[4] : nullptr, r[1], r[2], r[3], b_stride, pv_len, st, rv, s); });
    }
    std::lock_guard<std::mutex> lk(c->mu);
    int rc = ctx_device_init(c);
    if (rc != ZKV_OK) return rc;
    return run_mixed(c, n, d_vm, d_method, d_seals, nullptr, ZKV_SEAL_BYTES, d_in_a, d_in_b, nullptr, (uint32_t)b_stride, (uint32_t)pv_len, d_status,
                     d_recv, stream ? (hipStream_t)stream : c->stream);
}
ZKV_EXPORT int zkv_mixed_verify_batch_dev(zkv_ctx* c, size_t n, const uint8_t* d_vm, const uint8_t* d_seals, const uint8_t* d_in_a, const uint8_t* d_in_b,
                                          size_t b_stride, size_t pv_len, uint8_t* d_status, uint8_t* d_recv, void* stream) {
    return zkv_mixed_verify_call_batch_dev(c, n, d_vm, nullptr, d_seals, d_in_a, d_in_b, b_stride, pv_len, d_status, d_recv, stream);
}
ZKV_EXPORT int zkv_mixed_verify_call_batch(zkv_ctx* c, size_t n, const uint8_t* vm, const uint8_t* method, const uint8_t* seal_blob, const uint64_t* seal_off,
                                           const uint8_t* in_a, const uint8_t* in_b_blob, const uint64_t* in_b_off, uint8_t* status, uint8_t* recv) {
    if (!c || c->vm != ZKV_VM_MIXED) return ZKV_ERR_WRONG_CTX;
    if (n && (!vm || !seal_blob || !seal_off || !in_a || !in_b_blob || !in_b_off || !status)) return ZKV_ERR_INVALID_ARG;
    if (!n) return ZKV_OK;
    if (n > 0xFFFFFFF0u || !offsets_ok(seal_off, n) || !offsets_ok(in_b_off, n)) return ZKV_ERR_INVALID_ARG;
    for (size_t i = 0; i < n; i++)                   // journal_digest is a B256 in the reference (risc0/verifier.rs:82); verify_integrity has none
        if (vm[i] == ZKV_VM_RISC0 && (!method || method[i] == ZKV_METHOD_VERIFY) && in_b_off[i + 1] - in_b_off[i] != 32) return ZKV_ERR_INVALID_ARG;
    if (is_sharded(c))
        return run_sharded(c, n, [&](zkv_ctx* k, size_t lo, size_t hi) {
            return zkv_mixed_verify_call_batch(k, hi - lo, vm + lo, method ? method + lo : nullptr, seal_blob, seal_off + lo, in_a + 32 * lo, in_b_blob,
                                               in_b_off + lo, status + lo, recv ? recv + 4 * lo : nullptr); });
    std::lock_guard<std::mutex> lk(c->mu);
    int rc = ctx_device_init(c);
    if (rc != ZKV_OK) return rc;
    const uint64_t s0 = seal_off[0], sbytes = seal_off[n] - s0, b0 = in_b_off[0], bbytes = in_b_off[n] - b0;
    MixedMem& mm = c->m_mixed;
    if ((rc = grow_all(mm.h_vm, n, mm.h_seals, (size_t)sbytes + 8, mm.h_soff, 8 * (n + 1), mm.h_a, 32 * n, mm.h_b, (size_t)bbytes + 8,
                       mm.h_boff, 8 * (n + 1), mm.h_st, n, mm.h_rv, 4 * n)) != ZKV_OK || (method && (rc = mm.h_method.grow(n)) != ZKV_OK)) return rc;
    hipStream_t s = c->stream;
    if ((rc = order_after_previous(c, s)) != ZKV_OK) return rc;
    std::vector<uint64_t> so(seal_off, seal_off + n + 1), bo(in_b_off, in_b_off + n + 1);
    for (auto& v : so) v -= s0;
    for (auto& v : bo) v -= b0;
    HIP_TRY(hipMemcpyAsync(mm.h_vm, vm, n, hipMemcpyHostToDevice, s));
    if (method) HIP_TRY(hipMemcpyAsync(mm.h_method, method, n, hipMemcpyHostToDevice, s));
    if (sbytes) HIP_TRY(hipMemcpyAsync(mm.h_seals, seal_blob + s0, (size_t)sbytes, hipMemcpyHostToDevice, s));
    HIP_TRY(hipMemcpyAsync(mm.h_soff, so.data(), 8 * (n + 1), hipMemcpyHostToDevice, s));
    HIP_TRY(hipMemcpyAsync(mm.h_a, in_a, 32 * n, hipMemcpyHostToDevice, s));
    if (bbytes) HIP_TRY(hipMemcpyAsync(mm.h_b, in_b_blob + b0, (size_t)bbytes, hipMemcpyHostToDevice, s));
    HIP_TRY(hipMemcpyAsync(mm.h_boff, bo.data(), 8 * (n + 1), hipMemcpyHostToDevice, s));
    if ((rc = run_mixed(c, n, mm.h_vm, method ? mm.h_method : nullptr, mm.h_seals, mm.h_soff, 0, mm.h_a, mm.h_b, mm.h_boff, 0, 0, mm.h_st, mm.h_rv, s)) != ZKV_OK)
        return rc;
    return return_to_host(mm.h_st, mm.h_rv, n, status, recv, s);
}
ZKV_EXPORT int zkv_mixed_verify_batch(zkv_ctx* c, size_t n, const uint8_t* vm, const uint8_t* seal_blob, const uint64_t* seal_off, const uint8_t* in_a,
                                      const uint8_t* in_b_blob, const uint64_t* in_b_off, uint8_t* status, uint8_t* recv) {
    return zkv_mixed_verify_call_batch(c, n, vm, nullptr, seal_blob, seal_off, in_a, in_b_blob, in_b_off, status, recv);
}

// ------------------------------------------------------------------ RISC Zero
ZKV_EXPORT zkv_ctx* zkv_risc0_ctx_new(int device) {
    zkv_ctx* c = new (std::nothrow) zkv_ctx();
    if (!c) return nullptr;
    c->vm = ZKV_VM_RISC0; c->device = device;
    host::risc0_consts(c->consts);
    return c;
}
ZKV_EXPORT int zkv_risc0_initialize(zkv_ctx* c, const uint8_t control_root[32], const uint8_t bn254_control_id[32], uint8_t* status) {
    if (!c || c->vm != ZKV_VM_RISC0 || !control_root || !bn254_control_id) return ZKV_ERR_INVALID_ARG;
    std::lock_guard<std::mutex> lk(c->mu);
    if (c->initialized) { if (status) *status = ZKV_STATUS_ALREADY_INITIALIZED; return ZKV_OK; }   // verifier.rs:63-65
    host::split_digest(control_root, c->control_root_0, c->control_root_1);                        // :67-69
    memcpy(c->control_id, bn254_control_id, 32);                                                   // :70
    host::risc0_selector(control_root, bn254_control_id, c->selector);                             // :71-72
    uint32_t id[8];
    host::be_to_limbs(id, bn254_control_id);
    c->id_ge_r = !raw_lt_r(id);            // such a verifier fails every proof at groth16.rs:32
    c->initialized = true;
    if (status) *status = ZKV_STATUS_OK;
    return ZKV_OK;
}
ZKV_EXPORT zkv_ctx* zkv_risc0_ctx_create(const uint8_t control_root[32], const uint8_t bn254_control_id[32], int device) {
    zkv_ctx* c = zkv_risc0_ctx_new(device);
    if (!c) return nullptr;
    uint8_t st;
    if (zkv_risc0_initialize(c, control_root, bn254_control_id, &st) != ZKV_OK) { delete c; return nullptr; }
    return c;
}
ZKV_EXPORT void zkv_ctx_destroy(zkv_ctx* c) {
    if (!c) return;
    if (is_sharded(c)) shards_free(c);
    for (auto& k : c->kid) { if (k) zkv_ctx_destroy(k); k = nullptr; }
    for (auto* k : c->gw_route) zkv_ctx_destroy(k);
    c->gw_route.clear();
    if (c->gw_group) zkv_ctx_destroy(c->gw_group);
    c->gw_group = nullptr;
    ctx_free_device(c);
    delete c;
}
ZKV_EXPORT int zkv_risc0_get_selector(const zkv_ctx* c, uint8_t out[4]) {
    if (!c || c->vm != ZKV_VM_RISC0) return ZKV_ERR_WRONG_CTX;
    memcpy(out, c->selector, 4); return ZKV_OK;
}
ZKV_EXPORT int zkv_risc0_get_control_root(const zkv_ctx* c, uint8_t out_0[16], uint8_t out_1[16]) {
    if (!c || c->vm != ZKV_VM_RISC0) return ZKV_ERR_WRONG_CTX;
    memcpy(out_0, c->control_root_0, 16); memcpy(out_1, c->control_root_1, 16); return ZKV_OK;
}
ZKV_EXPORT int zkv_risc0_get_bn254_control_id(const zkv_ctx* c, uint8_t out[32]) {
    if (!c || c->vm != ZKV_VM_RISC0) return ZKV_ERR_WRONG_CTX;
    memcpy(out, c->control_id, 32); return ZKV_OK;
}
ZKV_EXPORT int zkv_risc0_get_verifier_key_digest(const zkv_ctx* c, uint8_t out[32]) {
    if (!c || c->vm != ZKV_VM_RISC0) return ZKV_ERR_WRONG_CTX;
    host::risc0_vk_digest(out); return ZKV_OK;
}
ZKV_EXPORT int zkv_risc0_is_initialized(const zkv_ctx* c) { return c && c->vm == ZKV_VM_RISC0 && c->initialized ? 1 : 0; }

ZKV_EXPORT int zkv_risc0_verify_batch(zkv_ctx* c, size_t n, const uint8_t* seal_blob, const uint64_t* seal_off, const uint8_t* image_ids,
                                      const uint8_t* journal_digests, uint8_t* status, uint8_t* recv) {
    if (!c || c->vm != ZKV_VM_RISC0) return ZKV_ERR_WRONG_CTX;
    if (n && (!image_ids || !journal_digests)) return ZKV_ERR_INVALID_ARG;
    if (is_sharded(c)) {
        if (n && (!seal_blob || !seal_off || !status)) return ZKV_ERR_INVALID_ARG;
        return run_sharded(c, n, [&](zkv_ctx* k, size_t lo, size_t hi) {
            return zkv_risc0_verify_batch(k, hi - lo, seal_blob, seal_off + lo, image_ids + 32 * lo, journal_digests + 32 * lo, status + lo, recv ? recv + 4 * lo : nullptr); });
    }
    return run_host_batch(c, n, seal_blob, seal_off, image_ids, journal_digests, nullptr, nullptr, status, recv);
}
ZKV_EXPORT int zkv_risc0_verify_integrity_batch(zkv_ctx* c, size_t n, const uint8_t* seal_blob, const uint64_t* seal_off,
                                                const uint8_t* claim_digests, uint8_t* status, uint8_t* recv) {
    if (!c || c->vm != ZKV_VM_RISC0) return ZKV_ERR_WRONG_CTX;
    if (n && !claim_digests) return ZKV_ERR_INVALID_ARG;
    if (is_sharded(c)) {
        if (n && (!seal_blob || !seal_off || !status)) return ZKV_ERR_INVALID_ARG;
        return run_sharded(c, n, [&](zkv_ctx* k, size_t lo, size_t hi) {
            return zkv_risc0_verify_integrity_batch(k, hi - lo, seal_blob, seal_off + lo, claim_digests + 32 * lo, status + lo, recv ? recv + 4 * lo : nullptr); });
    }
    return run_host_batch(c, n, seal_blob, seal_off, claim_digests, nullptr, nullptr, nullptr, status, recv);
}
ZKV_EXPORT int zkv_risc0_verify(zkv_ctx* c, const uint8_t* seal, size_t seal_len, const uint8_t image_id[32], const uint8_t journal_digest[32],
                                uint8_t* status, uint8_t recv[4]) {
    uint64_t off[2] = {0, seal_len};
    uint8_t dummy = 0;
    if (!seal && seal_len) return ZKV_ERR_INVALID_ARG;
    return zkv_risc0_verify_batch(c, 1, seal ? seal : &dummy, off, image_id, journal_digest, status, recv);
}
ZKV_EXPORT int zkv_risc0_verify_integrity(zkv_ctx* c, const uint8_t* seal, size_t seal_len, const uint8_t claim_digest[32], uint8_t* status,
                                          uint8_t recv[4]) {
    uint64_t off[2] = {0, seal_len};
    uint8_t dummy = 0;
    if (!seal && seal_len) return ZKV_ERR_INVALID_ARG;
    return zkv_risc0_verify_integrity_batch(c, 1, seal ? seal : &dummy, off, claim_digest, status, recv);
}
ZKV_EXPORT int zkv_risc0_verify_batch_dev(zkv_ctx* c, size_t n, const uint8_t* d_seals, const uint8_t* d_image_ids,
                                          const uint8_t* d_journal_digests, uint8_t* d_status, uint8_t* d_recv, void* stream) {
    if (!c || c->vm != ZKV_VM_RISC0) return ZKV_ERR_WRONG_CTX;
    if (n && !d_journal_digests) return ZKV_ERR_INVALID_ARG;
    if (is_sharded(c)) {
        if (n && (!d_seals || !d_image_ids || !d_status)) return ZKV_ERR_INVALID_ARG;
        const DevRow rows[3] = {{d_seals, ZKV_SEAL_BYTES}, {d_image_ids, 32}, {d_journal_digests, 32}};
        return run_sharded_dev(c, n, rows, 3, d_status, d_recv, stream, [&](zkv_ctx* k, size_t m, const uint8_t* const* r, uint8_t* st, uint8_t* rv, hipStream_t s) {
            return zkv_risc0_verify_batch_dev(k, m, r[0], r[1], r[2], st, rv, s); });
    }
    return run_dev_batch(c, n, d_seals, d_image_ids, d_journal_digests, nullptr, 0, d_status, d_recv, stream);
}
// no journal digest row: the prep kernel takes in_a as the claim digest (k_prep_risc0, in32_b == nullptr)
ZKV_EXPORT int zkv_risc0_verify_integrity_batch_dev(zkv_ctx* c, size_t n, const uint8_t* d_seals, const uint8_t* d_claim_digests, uint8_t* d_status,
                                                    uint8_t* d_recv, void* stream) {
    if (!c || c->vm != ZKV_VM_RISC0) return ZKV_ERR_WRONG_CTX;
    if (n && (!d_seals || !d_claim_digests || !d_status)) return ZKV_ERR_INVALID_ARG;
    if (!n) return ZKV_OK;
    if (is_sharded(c)) {
        const DevRow rows[2] = {{d_seals, ZKV_SEAL_BYTES}, {d_claim_digests, 32}};
        return run_sharded_dev(c, n, rows, 2, d_status, d_recv, stream, [&](zkv_ctx* k, size_t m, const uint8_t* const* r, uint8_t* st, uint8_t* rv, hipStream_t s) {
            return zkv_risc0_verify_integrity_batch_dev(k, m, r[0], r[1], st, rv, s); });
    }
    return run_dev_batch(c, n, d_seals, d_claim_digests, nullptr, nullptr, 0, d_status, d_recv, stream);
}

// ------------------------------------------------------------------ RISC Zero verifier sets (many instances, one VK)
ZKV_EXPORT zkv_ctx* zkv_risc0_set_create(size_t n_instances, const uint8_t* control_roots, const uint8_t* bn254_control_ids, int device) {
    if (!n_instances || n_instances > ((size_t)1 << 24) || !control_roots || !bn254_control_ids) return nullptr;
    zkv_ctx* c = new (std::nothrow) zkv_ctx();
    if (!c) return nullptr;
    c->vm = ZKV_VM_RISC0_SET; c->device = device; c->initialized = true;
    host::risc0_consts(c->consts);
    c->inst_raw.resize(n_instances);
    for (size_t i = 0; i < n_instances; i++) {
        memcpy(c->inst_raw[i].control_root, control_roots + 32 * i, 32);
        memcpy(c->inst_raw[i].control_id, bn254_control_ids + 32 * i, 32);
    }
    return c;
}
ZKV_EXPORT size_t zkv_risc0_set_size(const zkv_ctx* c) { return c && c->vm == ZKV_VM_RISC0_SET ? c->inst_raw.size() : 0; }
ZKV_EXPORT int zkv_risc0_set_get_selector(zkv_ctx* c, size_t instance, uint8_t out[4]) {
    if (!c || c->vm != ZKV_VM_RISC0_SET) return ZKV_ERR_WRONG_CTX;
    if (!out || instance >= c->inst_raw.size()) return ZKV_ERR_INVALID_ARG;
    std::lock_guard<std::mutex> lk(c->mu);
    int rc = ctx_device_init(c);                        // selectors are derived by the set-up kernel
    if (rc != ZKV_OK) return rc;
    const uint32_t s = c->inst_host[instance].selector_be;
    out[0] = (uint8_t)(s >> 24); out[1] = (uint8_t)(s >> 16); out[2] = (uint8_t)(s >> 8); out[3] = (uint8_t)s;
    return ZKV_OK;
}
// shared driver: host pointers when `dev` is false (one chunk at a time, synchronous), device pointers otherwise (asynchronous).
// integrity: verify_integrity, `ids` holds the claim digests and `jds` is not read.
static int run_set_batch(zkv_ctx* c, size_t n, const uint32_t* inst, const uint8_t* blob, const uint64_t* off, const uint8_t* ids, const uint8_t* jds,
                         uint8_t* status, uint8_t* recv, bool dev, void* stream, bool integrity = false) {
    if (!c || c->vm != ZKV_VM_RISC0_SET) return ZKV_ERR_WRONG_CTX;
    if (n && (!inst || !blob || (!dev && !off) || !ids || (!integrity && !jds) || !status)) return ZKV_ERR_INVALID_ARG;
    if (n && !dev && !offsets_ok(off, n)) return ZKV_ERR_INVALID_ARG;
    if (!n) return ZKV_OK;
    std::lock_guard<std::mutex> lk(c->mu);
    int rc = ctx_ready(c, n);
    if (rc != ZKV_OK) return rc;
    hipStream_t s = dev && stream ? (hipStream_t)stream : c->stream;
    if ((rc = order_after_previous(c, s)) != ZKV_OK) return rc;
    const size_t cap = c->ws.cap;
    std::vector<uint64_t> rel(dev ? 0 : cap + 1);
    for (size_t base = 0; base < n; base += cap) {
        const size_t m = n - base < cap ? n - base : cap;
        PrepArgs a;
        memset(&a, 0, sizeof a);
        a.n = m; a.inst_tab = c->d_inst; a.n_inst = (uint32_t)c->inst_raw.size();
        if (dev) {
            a.blob = blob + base * ZKV_SEAL_BYTES; a.stride = ZKV_SEAL_BYTES; a.inst = inst + base;
            a.in32_a = ids + 32 * base; a.in32_b = integrity ? nullptr : jds + 32 * base; a.status = status + base; a.recv = recv ? recv + 4 * base : nullptr;
        } else {
            const uint64_t b0 = off[base], bytes = off[base + m] - b0;
            if ((rc = c->d_blob.grow((size_t)bytes + 8)) != ZKV_OK) return rc;
            for (size_t i = 0; i <= m; i++) rel[i] = off[base + i] - b0;
            HIP_TRY(hipMemcpyAsync(c->d_off, rel.data(), sizeof(uint64_t) * (m + 1), hipMemcpyHostToDevice, s));
            if (bytes) HIP_TRY(hipMemcpyAsync(c->d_blob, blob + b0, (size_t)bytes, hipMemcpyHostToDevice, s));
            HIP_TRY(hipMemcpyAsync(c->d_inst_idx, inst + base, sizeof(uint32_t) * m, hipMemcpyHostToDevice, s));
            HIP_TRY(hipMemcpyAsync(c->d_a, ids + 32 * base, 32 * m, hipMemcpyHostToDevice, s));
            if (!integrity) HIP_TRY(hipMemcpyAsync(c->d_b, jds + 32 * base, 32 * m, hipMemcpyHostToDevice, s));
            HIP_TRY(hipStreamSynchronize(s));               // rel[] is reused by the next chunk
            a.blob = c->d_blob; a.off = c->d_off; a.inst = c->d_inst_idx; a.in32_a = c->d_a; a.in32_b = integrity ? nullptr : c->d_b;
            a.status = c->d_status; a.recv = c->d_recv;
        }
        enqueue_chunk(c, a, s, base + cap >= n);
        HIP_TRY(hipGetLastError());
        if (!dev) {
            HIP_TRY(hipMemcpyAsync(status + base, c->d_status, m, hipMemcpyDeviceToHost, s));
            if (recv) HIP_TRY(hipMemcpyAsync(recv + 4 * base, c->d_recv, 4 * m, hipMemcpyDeviceToHost, s));
            HIP_TRY(hipStreamSynchronize(s));
        }
    }
    return dev ? mark_done(c, s) : ZKV_OK;
}
ZKV_EXPORT int zkv_risc0_set_verify_batch(zkv_ctx* c, size_t n, const uint32_t* instance, const uint8_t* seal_blob, const uint64_t* seal_off,
                                          const uint8_t* image_ids, const uint8_t* journal_digests, uint8_t* status, uint8_t* recv) {
    if (recv && n) memset(recv, 0, 4 * n);
    return run_set_batch(c, n, instance, seal_blob, seal_off, image_ids, journal_digests, status, recv, false, nullptr);
}
ZKV_EXPORT int zkv_risc0_set_verify_batch_dev(zkv_ctx* c, size_t n, const uint32_t* d_instance, const uint8_t* d_seals, const uint8_t* d_image_ids,
                                              const uint8_t* d_journal_digests, uint8_t* d_status, uint8_t* d_recv, void* stream) {
    return run_set_batch(c, n, d_instance, d_seals, nullptr, d_image_ids, d_journal_digests, d_status, d_recv, true, stream);
}
ZKV_EXPORT int zkv_risc0_set_verify_integrity_batch(zkv_ctx* c, size_t n, const uint32_t* instance, const uint8_t* seal_blob, const uint64_t* seal_off,
                                                    const uint8_t* claim_digests, uint8_t* status, uint8_t* recv) {
    if (recv && n && c && c->vm == ZKV_VM_RISC0_SET) memset(recv, 0, 4 * n);
    return run_set_batch(c, n, instance, seal_blob, seal_off, claim_digests, nullptr, status, recv, false, nullptr, true);
}
ZKV_EXPORT int zkv_risc0_set_verify_integrity_batch_dev(zkv_ctx* c, size_t n, const uint32_t* d_instance, const uint8_t* d_seals,
                                                        const uint8_t* d_claim_digests, uint8_t* d_status, uint8_t* d_recv, void* stream) {
    return run_set_batch(c, n, d_instance, d_seals, nullptr, d_claim_digests, nullptr, d_status, d_recv, true, stream, true);
}
// compute_vk_x for (instance, claim halves): the per-instance signals come from the device table
ZKV_EXPORT int zkv_risc0_set_vk_x_batch(zkv_ctx* c, size_t n, const uint32_t* instance, const uint8_t* var_signals, uint8_t* out) {
    if (!c || c->vm != ZKV_VM_RISC0_SET) return ZKV_ERR_WRONG_CTX;
    if (n && (!instance || !var_signals || !out)) return ZKV_ERR_INVALID_ARG;
    if (!n) return ZKV_OK;
    for (size_t i = 0; i < n; i++) if (instance[i] >= c->inst_raw.size()) return ZKV_ERR_INVALID_ARG;
    std::lock_guard<std::mutex> lk(c->mu);
    int rc = ctx_ready(c, n);
    if (rc != ZKV_OK) return rc;
    if ((rc = order_after_previous(c, c->stream)) != ZKV_OK) return rc;
    const size_t cap = c->ws.cap;
    for (size_t base = 0; base < n; base += cap) {
        size_t m = n - base < cap ? n - base : cap;
        if ((rc = c->d_blob.grow(m * 64 + 8)) != ZKV_OK) return rc;
        if ((rc = c->d_pv.grow(m * 64 + 8)) != ZKV_OK) return rc;
        HIP_TRY(hipMemcpyAsync(c->d_blob, var_signals + 64 * base, 64 * m, hipMemcpyHostToDevice, c->stream));
        HIP_TRY(hipMemcpyAsync(c->d_inst_idx, instance + base, sizeof(uint32_t) * m, hipMemcpyHostToDevice, c->stream));
        launch_vk_x(m, c->d_tab, c->m16, c->d_inst, c->d_inst_idx, c->d_blob, c->d_pv, c->stream);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipMemcpyAsync(out + 64 * base, c->d_pv, 64 * m, hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(hipStreamSynchronize(c->stream));
    }
    return ZKV_OK;
}

// ------------------------------------------------------------------ SP1
ZKV_EXPORT zkv_ctx* zkv_sp1_ctx_create(int device) {
    zkv_ctx* c = new (std::nothrow) zkv_ctx();
    if (!c) return nullptr;
    c->vm = ZKV_VM_SP1; c->device = device; c->initialized = true;
    memset(&c->consts, 0, sizeof c->consts);
    return c;
}
ZKV_EXPORT int zkv_sp1_verifier_hash(uint8_t out[32]) { memcpy(out, host::SP1_VERIFIER_HASH, 32); return ZKV_OK; }
ZKV_EXPORT const char* zkv_sp1_version(void) { return host::SP1_VERSION; }
ZKV_EXPORT int zkv_sp1_verify_batch(zkv_ctx* c, size_t n, const uint8_t* vkeys, const uint8_t* pv_blob, const uint64_t* pv_off,
                                    const uint8_t* proof_blob, const uint64_t* proof_off, uint8_t* status, uint8_t* recv) {
    if (!c || c->vm != ZKV_VM_SP1) return ZKV_ERR_WRONG_CTX;
    if (n && (!vkeys || !pv_blob || !pv_off)) return ZKV_ERR_INVALID_ARG;
    if (is_sharded(c)) {
        if (n && (!proof_blob || !proof_off || !status)) return ZKV_ERR_INVALID_ARG;
        return run_sharded(c, n, [&](zkv_ctx* k, size_t lo, size_t hi) {
            return zkv_sp1_verify_batch(k, hi - lo, vkeys + 32 * lo, pv_blob, pv_off + lo, proof_blob, proof_off + lo, status + lo, recv ? recv + 4 * lo : nullptr); });
    }
    return run_host_batch(c, n, proof_blob, proof_off, vkeys, nullptr, pv_blob, pv_off, status, recv);
}
ZKV_EXPORT int zkv_sp1_verify_proof(zkv_ctx* c, const uint8_t vkey[32], const uint8_t* pv, size_t pv_len, const uint8_t* proof, size_t proof_len,
                                    uint8_t* status, uint8_t recv[4]) {
    uint64_t poff[2] = {0, proof_len}, voff[2] = {0, pv_len};
    uint8_t dummy = 0;
    if ((!pv && pv_len) || (!proof && proof_len)) return ZKV_ERR_INVALID_ARG;
    return zkv_sp1_verify_batch(c, 1, vkey, pv ? pv : &dummy, voff, proof ? proof : &dummy, poff, status, recv);
}
ZKV_EXPORT int zkv_sp1_verify_batch_dev(zkv_ctx* c, size_t n, const uint8_t* d_vkeys, const uint8_t* d_pv, size_t pv_len, const uint8_t* d_proofs,
                                        uint8_t* d_status, uint8_t* d_recv, void* stream) {
    if (!c || c->vm != ZKV_VM_SP1) return ZKV_ERR_WRONG_CTX;
    if (n && !d_pv) return ZKV_ERR_INVALID_ARG;
    if (is_sharded(c)) {
        if (n && (!d_proofs || !d_vkeys || !d_status)) return ZKV_ERR_INVALID_ARG;
        const DevRow rows[3] = {{d_vkeys, 32}, {d_pv, pv_len}, {d_proofs, ZKV_SEAL_BYTES}};
        return run_sharded_dev(c, n, rows, 3, d_status, d_recv, stream, [&](zkv_ctx* k, size_t m, const uint8_t* const* r, uint8_t* st, uint8_t* rv, hipStream_t s) {
            return zkv_sp1_verify_batch_dev(k, m, r[0], r[1], pv_len, r[2], st, rv, s); });
    }
    return run_dev_batch(c, n, d_proofs, d_vkeys, nullptr, d_pv, pv_len, d_status, d_recv, stream);
}

// ------------------------------------------------------------------ SP1 PLONK (no reference code: parity unpinned)
ZKV_EXPORT zkv_ctx* zkv_sp1_plonk_ctx_create(const uint8_t* vk, size_t vk_len, const uint8_t verifier_hash[32], int device) {
    if (!vk || !verifier_hash || vk_len < 7 * 32) return nullptr;
    uint32_t w[7][8];
    for (int k = 0; k < 7; k++) host::be_to_limbs(w[k], vk + 32 * k);
    auto small = [](const uint32_t* x) { for (int i = 1; i < 8; i++) if (x[i]) return false; return true; };
    // SP1's circuit: two public inputs and exactly one BSB22 commitment (the 27-word proof layout); other shapes are not supported
    if (!small(w[4]) || !small(w[5]) || !small(w[6]) || w[5][0] != 1 || w[4][0] != 2) return nullptr;
    const size_t n_c = w[5][0];
    if (vk_len != 7 * 32 + (8 + n_c) * 64 + 256) return nullptr;
    zkv_ctx* c = new (std::nothrow) zkv_ctx();
    if (!c) return nullptr;
    c->vm = ZKV_VM_SP1_PLONK; c->device = device; c->initialized = true;
    memset(&c->consts, 0, sizeof c->consts);
    memset(&c->pk_raw, 0, sizeof c->pk_raw);
    memcpy(c->pk_raw.size, w[0], 32); memcpy(c->pk_raw.size_inv, w[1], 32); memcpy(c->pk_raw.gen, w[2], 32); memcpy(c->pk_raw.coset, w[3], 32);
    c->pk_raw.nb_public = w[4][0]; c->pk_raw.n_c = w[5][0]; c->pk_raw.cci = w[6][0];
    for (size_t p = 0; p < 8 + n_c; p++) {
        host::be_to_limbs(c->pk_raw.pts[p][0], vk + 224 + 64 * p); host::be_to_limbs(c->pk_raw.pts[p][1], vk + 256 + 64 * p);
    }
    memcpy(c->pk_g2, vk + 224 + 64 * (8 + n_c), 256);
    memcpy(c->plonk_hash, verifier_hash, 32);
    return c;
}
ZKV_EXPORT int zkv_sp1_plonk_verifier_hash(const zkv_ctx* c, uint8_t out[32]) {
    if (!c || c->vm != ZKV_VM_SP1_PLONK) return ZKV_ERR_WRONG_CTX;
    memcpy(out, c->plonk_hash, 32); return ZKV_OK;
}
ZKV_EXPORT int zkv_sp1_plonk_verify_batch(zkv_ctx* c, size_t n, const uint8_t* vkeys, const uint8_t* pv_blob, const uint64_t* pv_off,
                                          const uint8_t* proof_blob, const uint64_t* proof_off, uint8_t* status, uint8_t* recv) {
    if (!c || c->vm != ZKV_VM_SP1_PLONK) return ZKV_ERR_WRONG_CTX;
    if (n && (!vkeys || !pv_blob || !pv_off)) return ZKV_ERR_INVALID_ARG;
    if (is_sharded(c)) {
        if (n && (!proof_blob || !proof_off || !status)) return ZKV_ERR_INVALID_ARG;
        return run_sharded(c, n, [&](zkv_ctx* k, size_t lo, size_t hi) {
            return zkv_sp1_plonk_verify_batch(k, hi - lo, vkeys + 32 * lo, pv_blob, pv_off + lo, proof_blob, proof_off + lo, status + lo, recv ? recv + 4 * lo : nullptr); });
    }
    return run_host_batch(c, n, proof_blob, proof_off, vkeys, nullptr, pv_blob, pv_off, status, recv);
}
ZKV_EXPORT int zkv_sp1_plonk_verify_proof(zkv_ctx* c, const uint8_t vkey[32], const uint8_t* pv, size_t pv_len, const uint8_t* proof, size_t proof_len,
                                          uint8_t* status, uint8_t recv[4]) {
    uint64_t poff[2] = {0, proof_len}, voff[2] = {0, pv_len};
    uint8_t dummy = 0;
    if ((!pv && pv_len) || (!proof && proof_len)) return ZKV_ERR_INVALID_ARG;
    return zkv_sp1_plonk_verify_batch(c, 1, vkey, pv ? pv : &dummy, voff, proof ? proof : &dummy, poff, status, recv);
}
ZKV_EXPORT int zkv_sp1_plonk_verify_batch_dev(zkv_ctx* c, size_t n, const uint8_t* d_vkeys, const uint8_t* d_pv, size_t pv_len, const uint8_t* d_proofs,
                                              uint8_t* d_status, uint8_t* d_recv, void* stream) {
    if (!c || c->vm != ZKV_VM_SP1_PLONK) return ZKV_ERR_WRONG_CTX;
    if (n && !d_pv) return ZKV_ERR_INVALID_ARG;
    if (is_sharded(c)) {
        if (n && (!d_proofs || !d_vkeys || !d_status)) return ZKV_ERR_INVALID_ARG;
        const DevRow rows[3] = {{d_vkeys, 32}, {d_pv, pv_len}, {d_proofs, ZKV_PLONK_PROOF_BYTES}};
        return run_sharded_dev(c, n, rows, 3, d_status, d_recv, stream, [&](zkv_ctx* k, size_t m, const uint8_t* const* r, uint8_t* st, uint8_t* rv, hipStream_t s) {
            return zkv_sp1_plonk_verify_batch_dev(k, m, r[0], r[1], pv_len, r[2], st, rv, s); });
    }
    return run_dev_batch(c, n, d_proofs, d_vkeys, nullptr, d_pv, pv_len, d_status, d_recv, stream);
}

// ------------------------------------------------------------------ selector routers: what the SP1 gateway and the RISC Zero router share
// Two routes with one selector: the router could not tell them apart.
static bool selectors_distinct(const std::vector<uint32_t>& sel) {
    for (size_t k = 0; k < sel.size(); k++)
        for (size_t j = 0; j < k; j++) if (sel[j] == sel[k]) return false;
    return true;
}
// The revert data of a custom error with one bytes4 argument, `signature` = "Name(bytes4)": its selector, then the bytes4 left-aligned in a word.
static int abi_encode_error_bytes4(const char* signature, const uint8_t arg[4], uint8_t* out) {
    memset(out, 0, 36);
    host::fn_selector(signature, out);
    memcpy(out + 4, arg, 4);
    return 36;
}
// A ragged host blob of n items to the device: the bytes [off[0], off[n]) to d_blob, the n + 1 offsets rebased to zero to d_off;
// *bytes = the byte count.  `rebased` holds the offsets until the caller has synchronised `s`.
static int stage_ragged(DevBuf<uint8_t>& d_blob, DevBuf<uint64_t>& d_off, const uint8_t* blob, const uint64_t* off, size_t n, std::vector<uint64_t>* rebased,
                        hipStream_t s, uint64_t* bytes) {
    const uint64_t o0 = off[0];
    *bytes = off[n] - o0;
    const int rc = grow_all(d_blob, (size_t)*bytes + 8, d_off, 8 * (n + 1));
    if (rc != ZKV_OK) return rc;
    rebased->assign(off, off + n + 1);
    for (auto& v : *rebased) v -= o0;
    if (*bytes) HIP_TRY(hipMemcpyAsync(d_blob, blob + o0, (size_t)*bytes, hipMemcpyHostToDevice, s));
    HIP_TRY(hipMemcpyAsync(d_off, rebased->data(), 8 * (n + 1), hipMemcpyHostToDevice, s));
    return ZKV_OK;
}
// The per-proof stages of one chunk of key-set slots (run_gset's per-proof region, the keyed groups of the two routers): `prep` launches
// the caller's PREP kernel for the chunk, the remaining stages are the key sets'.  The last chunk of a call records the six stage events.
template <class Prep>
static int gset_proof_stages(zkv_ctx* g, const GsetChunk& ch, int lanes, bool timed, hipStream_t s, Prep prep) {
    const size_t m = ch.m;
    if (timed) (void)hipEventRecord(g->ev[0], s);
    prep();
    if (timed) (void)hipEventRecord(g->ev[1], s);
    launch_gset_msm(ch, msm_lanes_long(g, m), g->ws, s);
    if (timed) (void)hipEventRecord(g->ev[2], s);
    if (lanes != 2) launch_g2chk2(m, g->ws, ch.status, s);       // (the lane-pair Miller loop is the subgroup test itself)
    if (timed) (void)hipEventRecord(g->ev[3], s);
    launch_gset_miller(lanes, m, ch.skey + ch.slot0, g->d_gs_key, g->ws, ch.status, s);
    if (timed) (void)hipEventRecord(g->ev[4], s);
    launch_finalexp_lanes(lanes, m, g->ws, ch.status, s);
    if (timed) (void)hipEventRecord(g->ev[5], s);
    HIP_TRY(hipGetLastError());
    return ZKV_OK;
}
// The keyed group of a router (DESIGN.md sections 12d, 12f, 17): the M padded slots the demultiplexer has filled, verified in one pass for
// all keys of the key set g -- prep(ch) fills and launches the caller's PREP record for the chunk, then the key sets' stages, chunk by
// chunk as run_gset runs them (no tail split).  idx, skey, st: the group's slot tables (index 0 = its first slot).  The set's own buffers
// (its keys, staged signals, workspace) are read after groth16_ready, which may have made them: a PREP record takes them from the chunk it
// is handed (keyed_prep_chunk), never from g before the call.  g->mu is held by the caller.
// The aggregate check on the group (zkv_ctx_set_aggregate_check on the front end, under the key sets' rules): keyed_group_begin decides
// whether the call takes it -- before the slots are laid out, the device has seen the count kernel only -- and names the capable keys
// for route_layout_agg; run_keyed_group then runs the set's aggregate sequence over the aggregate region [0, ka.R) with the caller's PREP
// (chunks ending on multiples of the unit), and the per-proof chunks from ka.R on.
static int groth16_ready(zkv_ctx* c, size_t n, size_t* chunk);
static bool gset_agg_tables(zkv_ctx* c);
struct GsetAggChunk { size_t base, m, n2, off; uint64_t slots; int lanes; };       // (set_agg_plan)
static int set_agg_plan(zkv_ctx* c, const uint64_t* beg, const uint64_t* end, const uint32_t* rep, uint32_t n_regions, uint64_t R, size_t capa,
                        uint32_t sub, std::vector<GsetAggChunk>* plan, hipStream_t s);
template <class Prep>
static void enqueue_gset_agg(zkv_ctx* c, const GsetChunk& ch, const GsetAggChunk& g, const uint32_t* skey, const uint32_t* d_amap, uint32_t sub,
                             hipStream_t s, bool timed, Prep prep);
struct KeyedAgg {
    const uint8_t* capable = nullptr;               // per key of the group: can take the check (null: this call does not)
    uint32_t sub = 0;                               // proofs per sub-batch of this call
    uint64_t R = 0;                                 // the aggregate region the layout gave: group slots [0, R), key k from astart[k]
    uint64_t astart[ROUTE_MAX_COLS + 1] = {};
};
// tot: the K keyed columns' totals, `placed` their sum.  *lanes: the mapping of the per-proof slots, as route_layout_agg takes it.
static int keyed_group_begin(zkv_ctx* g, const uint32_t* tot, size_t K, size_t placed, hipStream_t s, KeyedAgg* ka, int* lanes) {
    *ka = KeyedAgg();
    *lanes = miller_lanes(g, placed);
    if (!placed) return ZKV_OK;
    size_t cap = 0;
    int rc = groth16_ready(g, placed, &cap);
    if (rc != ZKV_OK) return rc;
    if ((rc = order_after_previous(g, s)) != ZKV_OK) return rc;
    if (!(g->agg_on && g->lanes == 0 && placed >= agg_min() && gset_agg_tables(g) && agg_wanted(g))) return ZKV_OK;
    // the workspace for any layout of these proofs (at most 31 pad slots per key) and, now that the tables have made agg_key_ok, the
    // aggregate buffers beside it: nothing grows once the slots are laid out
    if ((rc = groth16_ready(g, placed + 31 * K, &cap)) != ZKV_OK) return rc;
    const uint32_t unit = gset_agg_unit(g->agg_sub);
    if (g->agg_cap < g->ws.cap || cap < unit) return ZKV_OK;                     // (the aggregate buffers could not be allocated)
    size_t rest = 0;
    for (size_t k = 0; k < K; k++) rest += g->gs_agg_ok[k] ? tot[k] % unit : tot[k];
    ka->capable = g->gs_agg_ok.data(); ka->sub = g->agg_sub;
    *lanes = miller_lanes(g, rest);
    return ZKV_OK;
}
template <class Prep>
static int run_keyed_group(zkv_ctx* g, size_t M, int lanes, const KeyedAgg& ka, const uint32_t* idx, const uint32_t* skey, uint8_t* st, hipStream_t s, Prep prep) {
    if (!M) return ZKV_OK;
    size_t cap = 0;
    int rc = groth16_ready(g, M, &cap);            // (with the check engaged keyed_group_begin has sized the buffers already: nothing grows here)
    if (rc != ZKV_OK) return rc;
    auto chunk = [&](size_t base, size_t m) {
        GsetChunk ch;
        memset(&ch, 0, sizeof ch);
        ch.m = m; ch.slot0 = base; ch.idx = idx; ch.skey = skey;
        ch.keys = g->d_gs_key; ch.rows = g->d_gs_rows; ch.win = g->d_gs_win;
        ch.sig = g->d_lsig; ch.sig_cap = lsig_stride(g); ch.status = st + base;
        return ch;
    };
    const size_t R = (size_t)ka.R;
    if (R) {
        // one region per key, the keys back to back, as run_gset passes them
        const uint32_t unit = gset_agg_unit(ka.sub);
        std::vector<GsetAggChunk> plan;
        if ((rc = set_agg_plan(g, ka.astart, ka.astart + 1, nullptr, (uint32_t)g->gs_nic.size(), R, cap / unit * unit, ka.sub, &plan, s)) != ZKV_OK) return rc;
        for (const GsetAggChunk& a : plan) {
            const GsetChunk ch = chunk(a.base, a.m);
            enqueue_gset_agg(g, ch, a, skey + a.base, g->m_ks.amap, ka.sub, s, M == R && a.base + a.m >= R, [&] { prep(ch); });
            HIP_TRY(hipGetLastError());
        }
    }
    for (size_t base = R; base < M; base += cap) {
        const size_t m = M - base < cap ? M - base : cap;
        const GsetChunk ch = chunk(base, m);
        if ((rc = gset_proof_stages(g, ch, lanes, base + cap >= M, s, [&] { prep(ch); })) != ZKV_OK) return rc;
    }
    return mark_done(g, s);
}
// What a keyed group's PREP record (GwsetChunk, RzrChunk) shares with the chunk's GsetChunk
template <class Chunk>
static void keyed_prep_chunk(Chunk* pc, const GsetChunk& ch) {
    pc->m = ch.m; pc->slot0 = ch.slot0; pc->keys = ch.keys; pc->sig = ch.sig; pc->sig_cap = ch.sig_cap;
}
// The statuses of a router call back to the caller's order: one k_mixed_return per run of live slots (zkv_gset_layout.h route_layout).
static void route_return(const RouteLayout& L, const uint32_t* idx, const uint8_t* st, const uint8_t* rv, uint8_t* d_status, uint8_t* d_recv, hipStream_t s) {
    for (uint32_t q = 0; q < L.n_runs; q++) {
        const size_t lo = (size_t)L.run_at[q];
        launch_mixed_return((size_t)L.run_n[q], idx + lo, st + lo, rv + 4 * lo, d_status, d_recv, s);
    }
}

// ------------------------------------------------------------------ SP1 gateway (zkv_sp1_gateway.h; no reference counterpart: parity unpinned)
// Up to ZKV_SP1_GATEWAY_MAX_ROUTES SP1 verifiers behind one context; every proof goes to the route whose selector begins it.  The routes
// are ordinary SP1 / SP1 PLONK contexts owned by the gateway: the device front end (k_gateway.hip) sorts a batch into their compact
// records, each non-empty route runs its own stage pipeline on them (run_records), and the statuses go back to the caller's order.
ZKV_EXPORT zkv_ctx* zkv_sp1_gateway_create_keyed(int groth16, size_t n_keys, const uint8_t* const* vk_words, const uint8_t* verifier_hash,
                                                 size_t n_plonk, const uint8_t* const* plonk_vk, const size_t* plonk_vk_len,
                                                 const uint8_t* plonk_verifier_hash, int device) {
    if ((groth16 != 0 && groth16 != 1) || n_plonk > ZKV_SP1_GATEWAY_MAX_ROUTES || n_keys > ZKV_SP1_GATEWAY_MAX_ROUTES ||
        groth16 + n_keys + n_plonk == 0 || groth16 + n_keys + n_plonk > ZKV_SP1_GATEWAY_MAX_ROUTES) return nullptr;
    if (n_plonk && (!plonk_vk || !plonk_vk_len || !plonk_verifier_hash)) return nullptr;
    if (n_keys && (!vk_words || !verifier_hash)) return nullptr;
    std::vector<uint32_t> sel;
    std::vector<uint8_t> hash;
    if (groth16) { sel.push_back(be32_of(host::SP1_VERIFIER_HASH)); hash.insert(hash.end(), host::SP1_VERIFIER_HASH, host::SP1_VERIFIER_HASH + 32); }
    for (size_t k = 0; k < n_keys; k++) {
        if (!vk_words[k]) return nullptr;
        sel.push_back(be32_of(verifier_hash + 32 * k));
        hash.insert(hash.end(), verifier_hash + 32 * k, verifier_hash + 32 * k + 32);
    }
    for (size_t k = 0; k < n_plonk; k++) {
        if (!plonk_vk[k]) return nullptr;
        sel.push_back(be32_of(plonk_verifier_hash + 32 * k));
        hash.insert(hash.end(), plonk_verifier_hash + 32 * k, plonk_verifier_hash + 32 * k + 32);
    }
    if (!selectors_distinct(sel)) return nullptr;
    zkv_ctx* c = new (std::nothrow) zkv_ctx();
    if (!c) return nullptr;
    c->vm = ZKV_VM_SP1_GATEWAY; c->device = device; c->initialized = true;
    memset(&c->consts, 0, sizeof c->consts);
    c->gw_sel = sel; c->gw_hash = hash;
    if (groth16) {
        zkv_ctx* r = zkv_sp1_ctx_create(device);
        if (!r) { zkv_ctx_destroy(c); return nullptr; }
        c->gw_route.push_back(r);
    }
    if (n_keys) {                                                  // one key set for all of them: its points are judged on the device (vk_valid per key)
        const std::vector<size_t> n_ic(n_keys, 3);
        const std::vector<int> vm(n_keys, ZKV_VM_SP1);
        c->gw_group = zkv_groth16_set_create(n_keys, vk_words, n_ic.data(), vm.data(), device);
        if (!c->gw_group) { zkv_ctx_destroy(c); return nullptr; }
        c->gw_key0 = c->gw_route.size(); c->gw_nkeys = n_keys;
        c->gw_route.insert(c->gw_route.end(), n_keys, nullptr);
    }
    for (size_t k = 0; k < n_plonk; k++) {
        zkv_ctx* r = zkv_sp1_plonk_ctx_create(plonk_vk[k], plonk_vk_len[k], plonk_verifier_hash + 32 * k, device);
        if (!r) { zkv_ctx_destroy(c); return nullptr; }
        c->gw_route.push_back(r);
    }
    c->gw_ran.assign(c->gw_route.size(), 0);
    return c;
}
ZKV_EXPORT zkv_ctx* zkv_sp1_gateway_create(int groth16, size_t n_plonk, const uint8_t* const* plonk_vk, const size_t* plonk_vk_len,
                                           const uint8_t* plonk_verifier_hash, int device) {
    return zkv_sp1_gateway_create_keyed(groth16, 0, nullptr, nullptr, n_plonk, plonk_vk, plonk_vk_len, plonk_verifier_hash, device);
}
// a route of the keyed group (no context of its own)
static inline bool gw_keyed(const zkv_ctx* c, size_t r) { return r >= c->gw_key0 && r < c->gw_key0 + c->gw_nkeys; }
ZKV_EXPORT int zkv_sp1_gateway_route_verifier_hash(const zkv_ctx* c, size_t r, uint8_t out[32]) {
    if (!c || c->vm != ZKV_VM_SP1_GATEWAY) return ZKV_ERR_WRONG_CTX;
    if (r >= c->gw_route.size() || !out) return ZKV_ERR_INVALID_ARG;
    memcpy(out, c->gw_hash.data() + 32 * r, 32);
    return ZKV_OK;
}
ZKV_EXPORT size_t zkv_sp1_gateway_route_count(const zkv_ctx* c) { return c && c->vm == ZKV_VM_SP1_GATEWAY ? c->gw_route.size() : 0; }
ZKV_EXPORT int zkv_sp1_gateway_route(const zkv_ctx* c, size_t r, uint8_t selector[4], int* vm) {
    if (!c || c->vm != ZKV_VM_SP1_GATEWAY) return ZKV_ERR_WRONG_CTX;
    if (r >= c->gw_route.size()) return ZKV_ERR_INVALID_ARG;
    if (selector) be32_put(selector, c->gw_sel[r]);
    if (vm) *vm = gw_keyed(c, r) ? ZKV_VM_SP1 : c->gw_route[r]->vm;
    return ZKV_OK;
}
ZKV_EXPORT zkv_ctx* zkv_sp1_gateway_route_ctx(zkv_ctx* c, size_t r) {
    return c && c->vm == ZKV_VM_SP1_GATEWAY && r < c->gw_route.size() ? c->gw_route[r] : nullptr;
}
// route of a proof of `len` bytes starting with p: 0 .. R - 1, GW_COL_NOT_FOUND or GW_COL_SHORT (the kernels' gw_class on the host)
static int gateway_route_of(const zkv_ctx* c, const uint8_t* p, size_t len) {
    if (len < 4) return GW_COL_SHORT;
    const uint32_t sel = be32_of(p);
    for (size_t k = 0; k < c->gw_sel.size(); k++) if (c->gw_sel[k] == sel) return (int)k;
    return GW_COL_NOT_FOUND;
}
ZKV_EXPORT int zkv_sp1_gateway_verify_proof(zkv_ctx* c, const uint8_t vkey[32], const uint8_t* pv, size_t pv_len, const uint8_t* proof, size_t proof_len,
                                            uint8_t* status, uint8_t recv[4]) {
    if (!c || c->vm != ZKV_VM_SP1_GATEWAY) return ZKV_ERR_WRONG_CTX;
    if (!vkey || !status || (!pv && pv_len) || (!proof && proof_len)) return ZKV_ERR_INVALID_ARG;
    const int col = gateway_route_of(c, proof, proof_len);
    uint8_t rv[4] = {0, 0, 0, 0};
    if (col < GW_MAX_ROUTES && gw_keyed(c, (size_t)col)) {       // the keyed group has no single-proof path: a batch of one
        const uint64_t poff[2] = {0, proof_len}, voff[2] = {0, pv_len};
        const uint8_t zero = 0;
        return zkv_sp1_gateway_verify_batch(c, 1, vkey, pv ? pv : &zero, voff, proof, poff, status, recv);
    }
    if (col < GW_MAX_ROUTES) {
        zkv_ctx* k = c->gw_route[col];
        const int rc = k->vm == ZKV_VM_SP1 ? zkv_sp1_verify_proof(k, vkey, pv, pv_len, proof, proof_len, status, rv)
                                           : zkv_sp1_plonk_verify_proof(k, vkey, pv, pv_len, proof, proof_len, status, rv);
        if (rc != ZKV_OK) return rc;
    } else if (col == GW_COL_NOT_FOUND) {
        *status = ZKV_STATUS_ROUTE_NOT_FOUND;
        memcpy(rv, proof, 4);
    } else *status = ZKV_STATUS_INVALID_PROOF_DATA;                // sp1/verifier.rs:64
    if (recv) memcpy(recv, rv, 4);
    std::lock_guard<std::mutex> lk(c->mu);
    for (auto& v : c->gw_counts) v = 0;
    c->gw_counts[col] = 1;
    for (size_t k = 0; k < c->gw_ran.size(); k++) c->gw_ran[k] = (int)k == col;
    return ZKV_OK;
}

// Everything device-resident: ragged proofs (offsets bounded by proof_bytes on the device); public values ragged (d_pv_off) or at a
// fixed stride.  Or, from the calldata decoder, `recs`: (start, length) records of proofs and public values from one base address, which
// d_proofs and d_pv then both are, and bad-calldata marks.  Synchronises `s` once, after the count, to size the compact records and learn
// the routes' sub-batch sizes.
static int run_gateway(zkv_ctx* c, size_t n, const uint8_t* d_vkeys, const uint8_t* d_proofs, const uint64_t* d_proof_off, uint64_t proof_bytes,
                       const uint8_t* d_pv, const uint64_t* d_pv_off, uint64_t pv_stride, uint8_t* d_status, uint8_t* d_recv, hipStream_t s,
                       const GwWireArgs* recs = nullptr) {
    int rc;
    const size_t blocks = (n + 255) / 256, R = c->gw_route.size(), K = c->gw_nkeys, key0 = c->gw_key0;
    // slots: one per routed proof, and up to 31 pad slots behind every keyed route (its successor starts on a wavefront of the Miller
    // mapping).  With the aggregate check on the keyed group the bound is the same: the aggregate region pads nothing, and every route's
    // per-proof part is padded as the whole route was (zkv_gset_layout.h route_layout_agg).
    const size_t ns = n + 32 * K;
    GatewayMem& gm = c->m_gw;                                     // (the compact records are sized behind the count)
    if ((rc = grow_all(gm.cnt, 4 * GW_COLS * blocks, gm.totals, 4 * GW_COLS, gm.pos, 4 * n, gm.idx, 4 * ns, gm.len, 4 * ns, gm.a, 32 * ns,
                       gm.pvoff, 8 * ns, gm.pvlen, 4 * ns, gm.st, ns, gm.rv, 4 * ns)) != ZKV_OK || (K && (rc = gm.skey.grow(4 * ns)) != ZKV_OK)) return rc;
    if ((rc = order_after_previous(c, s)) != ZKV_OK) return rc;
    GatewayArgs a;
    memset(&a, 0, sizeof a);
    a.n = n; a.proofs = d_proofs; a.proof_off = d_proof_off; a.proof_bytes = proof_bytes; a.vkeys = d_vkeys; a.pv_off = d_pv_off; a.pv_stride = pv_stride;
    if (recs) { a.rec_proof_at = recs->proof_at; a.rec_proof_len = recs->proof_len; a.rec_pv_at = recs->pv_at; a.rec_pv_len = recs->pv_len; a.rec_bad = recs->bad; }
    a.n_routes = (uint32_t)R;
    for (size_t r = 0; r < R; r++) {
        a.sel[r] = c->gw_sel[r];
        a.rec[r] = c->gw_route[r] && c->gw_route[r]->vm == ZKV_VM_SP1_PLONK ? ZKV_PLONK_PROOF_BYTES : ZKV_SEAL_BYTES;
    }
    a.cnt = gm.cnt; a.totals = gm.totals; a.pos = gm.pos; a.idx = gm.idx; a.c_len = gm.len; a.c_a = gm.a; a.c_pvoff = gm.pvoff; a.c_pvlen = gm.pvlen;
    a.status = d_status; a.recv = d_recv;
    if (K) HIP_TRY(hipMemsetAsync(a.idx, 0xFF, 4 * ns, s));      // pad slots: GW_NONE
    launch_gateway_count(a, s);
    HIP_TRY(hipGetLastError());
    uint32_t tot[GW_COLS];
    HIP_TRY(hipMemcpyAsync(tot, gm.totals, sizeof tot, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    // The layout (zkv_gset_layout.h route_layout).  A route with a context of its own takes one slot per proof; the keyed routes take the
    // key sets' layout (gset_choose: the mapping their proofs would take, stepped to a finer one while the padding exceeds 1.25 times).
    size_t routed = 0, placed = 0;
    for (size_t r = 0; r < R; r++) routed += tot[r];
    for (size_t k = 0; k < K; k++) placed += tot[key0 + k];
    std::unique_lock<std::mutex> glk;
    if (K) glk = std::unique_lock<std::mutex>(c->gw_group->mu);
    // whether the group takes the aggregate check is decided here, before the layout: the layout then has two regions (route_layout_agg)
    KeyedAgg ka;
    int glanes = 0;
    if (K && (rc = keyed_group_begin(c->gw_group, tot + key0, K, placed, s, &ka, &glanes)) != ZKV_OK) return rc;
    RouteLayout L;
    RouteAggLayout A;
    route_layout_agg(tot, (uint32_t)R, (uint32_t)key0, (uint32_t)K, a.rec, glanes, K && c->gw_group->lanes != 0, ka.capable, ka.sub, &L, &A);
    ka.R = A.R;
    for (size_t k = 0; k <= K; k++) ka.astart[k] = A.astart[k];
    for (size_t r = 0; r < R; r++) { a.start[r] = L.start[r]; a.base[r] = L.base[r]; }
    for (size_t k = 0; k < K; k++) { a.agg[key0 + k] = A.agg[k]; a.astart[key0 + k] = (uint32_t)(L.g0 + A.astart[k]); }
    a.g0 = (uint32_t)L.g0; a.gm = (uint32_t)L.m; a.gb0 = L.b0;
    if (routed + tot[GW_COL_NOT_FOUND] + tot[GW_COL_SHORT] + tot[GW_COL_BAD] != n || L.slots > ns) return ZKV_ERR_HIP;
    if ((rc = gm.recs.grow((size_t)L.bytes + 8)) != ZKV_OK) return rc;
    a.c_proofs = gm.recs;
    for (size_t r = 0; r < R; r++) { c->gw_counts[r] = tot[r]; c->gw_ran[r] = tot[r] > 0; }
    for (size_t r = R; r < GW_MAX_ROUTES; r++) c->gw_counts[r] = 0;
    c->gw_counts[GW_COL_NOT_FOUND] = tot[GW_COL_NOT_FOUND]; c->gw_counts[GW_COL_SHORT] = tot[GW_COL_SHORT]; c->gw_counts[GW_COL_BAD] = tot[GW_COL_BAD];
    launch_gateway_place(a, s);
    HIP_TRY(hipGetLastError());
    uint8_t *st = gm.st, *rv = gm.rv;
    for (size_t r = 0; r < R; r++) {
        if (gw_keyed(c, r)) continue;
        const size_t j = a.start[r];
        if ((rc = run_records(c->gw_route[r], tot[r], a.c_proofs + a.base[r], a.c_len + j, a.c_a + 32 * j, nullptr, nullptr, d_pv, a.c_pvoff + j,
                              a.c_pvlen + j, st + j, rv + 4 * j, s)) != ZKV_OK) return rc;
    }
    if (K) {                                                       // the keyed group: k_gwset_prep with the slot's key, then the key sets' stages
        const size_t G0 = (size_t)L.g0;
        zkv_ctx* g = c->gw_group;
        GwsetChunk pc;
        memset(&pc, 0, sizeof pc);
        pc.idx = a.idx + G0; pc.skey = gm.skey;
        pc.recs = a.c_proofs + L.b0; pc.len = a.c_len + G0; pc.vkeys = a.c_a + 32 * G0; pc.pvoff = a.c_pvoff + G0; pc.pvlen = a.c_pvlen + G0; pc.pv = d_pv;
        pc.n_keys = (uint32_t)K;
        for (size_t k = 0; k < K; k++) { pc.start[k] = (uint32_t)L.gstart[k]; pc.astart[k] = (uint32_t)A.astart[k]; }
        pc.agg_r = (uint32_t)A.R;
        pc.status = st + G0; pc.recv = (uint32_t*)(rv + 4 * G0);
        if ((rc = run_keyed_group(g, (size_t)L.m, L.lanes, ka, pc.idx, pc.skey, pc.status, s, [&](const GsetChunk& ch) {
                keyed_prep_chunk(&pc, ch);
                launch_gwset_prep(pc, g->ws, s); })) != ZKV_OK) return rc;
    }
    HIP_TRY(hipSetDevice(c->device));
    // (a keyed route may end in pad slots; a gateway without keyed routes is one run)
    route_return(L, a.idx, st, rv, d_status, d_recv, s);
    HIP_TRY(hipGetLastError());
    return mark_done(c, s);
}
ZKV_EXPORT int zkv_sp1_gateway_verify_batch_dev(zkv_ctx* c, size_t n, const uint8_t* d_vkeys, const uint8_t* d_pv, size_t pv_len,
                                                const uint8_t* d_proofs, const uint64_t* d_proof_off, uint64_t proof_bytes,
                                                uint8_t* d_status, uint8_t* d_recv, void* stream) {
    if (!c || c->vm != ZKV_VM_SP1_GATEWAY) return ZKV_ERR_WRONG_CTX;
    if (n && (!d_vkeys || !d_pv || !d_proofs || !d_proof_off || !d_status)) return ZKV_ERR_INVALID_ARG;
    if (!n) return ZKV_OK;
    if (n > 0xFFFFFFF0u || pv_len > 0xFFFFFFFFu) return ZKV_ERR_INVALID_ARG;
    std::lock_guard<std::mutex> lk(c->mu);
    int rc = ctx_device_init(c);
    if (rc != ZKV_OK) return rc;
    return run_gateway(c, n, d_vkeys, d_proofs, d_proof_off, proof_bytes, d_pv, nullptr, pv_len, d_status, d_recv, stream ? (hipStream_t)stream : c->stream);
}
ZKV_EXPORT int zkv_sp1_gateway_verify_batch(zkv_ctx* c, size_t n, const uint8_t* vkeys, const uint8_t* pv_blob, const uint64_t* pv_off,
                                            const uint8_t* proof_blob, const uint64_t* proof_off, uint8_t* status, uint8_t* recv) {
    if (!c || c->vm != ZKV_VM_SP1_GATEWAY) return ZKV_ERR_WRONG_CTX;
    if (n && (!vkeys || !pv_blob || !pv_off || !proof_blob || !proof_off || !status)) return ZKV_ERR_INVALID_ARG;
    if (!n) return ZKV_OK;
    if (n > 0xFFFFFFF0u || !offsets_ok(proof_off, n) || !offsets_ok(pv_off, n)) return ZKV_ERR_INVALID_ARG;
    for (size_t i = 0; i < n; i++) if (pv_off[i + 1] - pv_off[i] > 0xFFFFFFFFu) return ZKV_ERR_INVALID_ARG;
    std::lock_guard<std::mutex> lk(c->mu);
    int rc = ctx_device_init(c);
    if (rc != ZKV_OK) return rc;
    GatewayMem& gm = c->m_gw;
    if ((rc = grow_all(gm.h_vk, 32 * n, gm.h_st, n, gm.h_rv, 4 * n)) != ZKV_OK) return rc;
    hipStream_t s = c->stream;
    if ((rc = order_after_previous(c, s)) != ZKV_OK) return rc;
    std::vector<uint64_t> so, vo;
    uint64_t sbytes = 0, vbytes = 0;
    HIP_TRY(hipMemcpyAsync(gm.h_vk, vkeys, 32 * n, hipMemcpyHostToDevice, s));
    if ((rc = stage_ragged(gm.h_pv, gm.h_pvoff, pv_blob, pv_off, n, &vo, s, &vbytes)) != ZKV_OK ||
        (rc = stage_ragged(gm.h_proof, gm.h_poff, proof_blob, proof_off, n, &so, s, &sbytes)) != ZKV_OK) return rc;
    if ((rc = run_gateway(c, n, gm.h_vk, gm.h_proof, gm.h_poff, sbytes, gm.h_pv, gm.h_pvoff, 0, gm.h_st, gm.h_rv, s)) != ZKV_OK) return rc;
    return return_to_host(gm.h_st, gm.h_rv, n, status, recv, s);
}
ZKV_EXPORT int zkv_sp1_gateway_last_route_counts(zkv_ctx* c, uint64_t* out) {
    if (!c || c->vm != ZKV_VM_SP1_GATEWAY) return ZKV_ERR_WRONG_CTX;
    if (!out) return ZKV_ERR_INVALID_ARG;
    std::lock_guard<std::mutex> lk(c->mu);
    const size_t R = c->gw_route.size();
    for (size_t r = 0; r < R; r++) out[r] = c->gw_counts[r];
    out[R] = c->gw_counts[GW_COL_NOT_FOUND]; out[R + 1] = c->gw_counts[GW_COL_SHORT];
    return ZKV_OK;
}
ZKV_EXPORT int zkv_sp1_gateway_status_abi_encode(const zkv_ctx* c, uint8_t status, const uint8_t received[4], uint8_t out[68]) {
    if (!c || c->vm != ZKV_VM_SP1_GATEWAY) return ZKV_ERR_WRONG_CTX;
    if (!out) return ZKV_ERR_INVALID_ARG;
    if (status == ZKV_STATUS_ROUTE_NOT_FOUND) return received ? abi_encode_error_bytes4("RouteNotFound(bytes4)", received, out) : ZKV_ERR_INVALID_ARG;
    uint8_t expected[4];
    be32_put(expected, c->gw_sel[0]);
    return zkv_status_abi_encode(ZKV_VM_SP1, status, received, expected, out);
}

// ------------------------------------------------------------------ RISC Zero router (zkv_risc0_router.h; no reference counterpart: parity unpinned)
// Up to ZKV_RISC0_ROUTER_MAX_ROUTES RISC Zero Groth16 verifiers behind one context; every seal goes to the route whose selector begins
// it.  The built-in-key routes are ONE verifier set (kid[0], a ZKV_VM_RISC0_SET context whose instances are the routes), the keyed routes
// ONE Groth16 key set (gw_group: n_ic = 6, RISC Zero convention).  The device front end (k_risc0_router.hip) sorts a batch into the two
// groups' compact records; the built-in group runs the verifier set's own stage pipeline with the instance row the front end wrote, the
// keyed group k_rzrouter_prep and then the key sets' stages, and the statuses go back to the caller's order.
// gw_sel: every route's selector (built-in routes first); gw_hash: 32 bytes per route, its key's digest; kid_ran: which group ran.
ZKV_EXPORT zkv_ctx* zkv_risc0_router_create(size_t n_builtin, const uint8_t* control_roots, const uint8_t* bn254_control_ids, size_t n_keyed,
                                            const uint8_t* const* vk_words, const uint8_t* keyed_control_roots, const uint8_t* keyed_control_ids, int device) {
    if (n_builtin > ZKV_RISC0_ROUTER_MAX_ROUTES || n_keyed > ZKV_RISC0_ROUTER_MAX_KEYED || n_builtin + n_keyed == 0 ||
        n_builtin + n_keyed > ZKV_RISC0_ROUTER_MAX_ROUTES) return nullptr;
    if (n_builtin && (!control_roots || !bn254_control_ids)) return nullptr;
    if (n_keyed && (!vk_words || !keyed_control_roots || !keyed_control_ids)) return nullptr;
    std::vector<uint32_t> sel;
    std::vector<uint8_t> dig;
    std::vector<RzrRoute> routes(n_keyed);
    uint8_t d[32], s4[4];
    host::risc0_vk_digest(d);
    for (size_t k = 0; k < n_builtin; k++) {
        host::risc0_selector_with(control_roots + 32 * k, bn254_control_ids + 32 * k, d, s4);
        sel.push_back(be32_of(s4));
        dig.insert(dig.end(), d, d + 32);
    }
    for (size_t k = 0; k < n_keyed; k++) {
        if (!vk_words[k]) return nullptr;
        const uint8_t *root = keyed_control_roots + 32 * k, *id = keyed_control_ids + 32 * k;
        host::risc0_vk_digest_words(vk_words[k], 6, d);
        host::risc0_selector_with(root, id, d, s4);
        sel.push_back(be32_of(s4));
        dig.insert(dig.end(), d, d + 32);
        // control_root_0 / _1 as initialize stores them (verifier.rs:64-66), the control id as it is; all as little-endian limbs
        uint8_t lo[16], hi[16], w[32];
        host::split_digest(root, lo, hi);
        RzrRoute& rt = routes[k];
        memset(&rt, 0, sizeof rt);
        memset(w, 0, 32); memcpy(w + 16, lo, 16); host::be_to_limbs(rt.cr0, w);
        memset(w, 0, 32); memcpy(w + 16, hi, 16); host::be_to_limbs(rt.cr1, w);
        host::be_to_limbs(rt.id, id);
        rt.id_ge_r = raw_lt_r(rt.id) ? 0u : 1u;
    }
    if (!selectors_distinct(sel)) return nullptr;
    zkv_ctx* c = new (std::nothrow) zkv_ctx();
    if (!c) return nullptr;
    c->vm = ZKV_VM_RISC0_ROUTER; c->device = device; c->initialized = true;
    host::risc0_consts(c->consts);
    c->gw_sel = sel; c->gw_hash = dig; c->rz_routes = routes; c->rz_nb = n_builtin;
    c->rz_counts.assign(sel.size() + 2, 0);
    if (n_builtin) {
        c->kid[0] = zkv_risc0_set_create(n_builtin, control_roots, bn254_control_ids, device);
        if (!c->kid[0]) { zkv_ctx_destroy(c); return nullptr; }
    }
    if (n_keyed) {                                                 // one key set for all of them: its points are judged on the device (vk_valid per key)
        const std::vector<size_t> n_ic(n_keyed, 6);
        const std::vector<int> vm(n_keyed, ZKV_VM_RISC0);
        c->gw_group = zkv_groth16_set_create(n_keyed, vk_words, n_ic.data(), vm.data(), device);
        if (!c->gw_group) { zkv_ctx_destroy(c); return nullptr; }
    }
    return c;
}
ZKV_EXPORT size_t zkv_risc0_router_route_count(const zkv_ctx* c) { return c && c->vm == ZKV_VM_RISC0_ROUTER ? c->gw_sel.size() + (c->rz_set ? 1 : 0) : 0; }
ZKV_EXPORT int zkv_risc0_router_route(const zkv_ctx* c, size_t r, uint8_t selector[4], int* keyed) {
    if (!c || c->vm != ZKV_VM_RISC0_ROUTER) return ZKV_ERR_WRONG_CTX;
    if (c->rz_set && r == c->gw_sel.size()) {                     // the set route (zkv_risc0_router_set.h): the last one
        if (selector) memcpy(selector, c->si_set_sel, 4);
        if (keyed) *keyed = 2;
        return ZKV_OK;
    }
    if (r >= c->gw_sel.size()) return ZKV_ERR_INVALID_ARG;
    if (selector) be32_put(selector, c->gw_sel[r]);
    if (keyed) *keyed = r >= c->rz_nb ? 1 : 0;
    return ZKV_OK;
}
ZKV_EXPORT int zkv_risc0_router_route_verifier_key_digest(const zkv_ctx* c, size_t r, uint8_t out[32]) {
    if (!c || c->vm != ZKV_VM_RISC0_ROUTER) return ZKV_ERR_WRONG_CTX;
    if (r >= c->gw_sel.size() || !out) return ZKV_ERR_INVALID_ARG;
    memcpy(out, c->gw_hash.data() + 32 * r, 32);
    return ZKV_OK;
}

// The built-in group: m compact records from the front end through the verifier set's pipeline (run_set_batch's chunks, with the true
// lengths and the instance row on the device).  kind: the method row, or nullptr: one method, in_b == nullptr being verify_integrity.
static int run_router_builtin(zkv_ctx* c, size_t m_total, const uint8_t* seals, const uint32_t* len, const uint32_t* inst, const uint8_t* in_a,
                              const uint8_t* in_b, const uint8_t* kind, uint8_t* st, uint8_t* rv, hipStream_t s) {
    if (!m_total) return ZKV_OK;
    std::lock_guard<std::mutex> lk(c->mu);
    int rc = ctx_ready(c, m_total);
    if (rc != ZKV_OK) return rc;
    if ((rc = order_after_previous(c, s)) != ZKV_OK) return rc;
    const size_t cap = c->ws.cap;
    for (size_t base = 0; base < m_total; base += cap) {
        const size_t m = m_total - base < cap ? m_total - base : cap;
        PrepArgs a;
        memset(&a, 0, sizeof a);
        a.n = m; a.blob = seals + base * ZKV_SEAL_BYTES; a.stride = ZKV_SEAL_BYTES; a.len = len + base;
        a.inst = inst + base; a.inst_tab = c->d_inst; a.n_inst = (uint32_t)c->inst_raw.size();
        a.in32_a = in_a + 32 * base; a.in32_b = in_b ? in_b + 32 * base : nullptr;
        a.kind = kind ? kind + base : nullptr;
        a.status = st + base; a.recv = rv + 4 * base;
        enqueue_chunk(c, a, s, base + cap >= m_total);
    }
    HIP_TRY(hipGetLastError());
    return mark_done(c, s);
}
// Everything device-resident: ragged seals (offsets bounded by seal_bytes on the device) or, d_seal_off == nullptr, a fixed stride of 260.
// d_b == nullptr: verify_integrity, d_a holds the claim digests.  d_method: the per-seal method row (d_b is then set), or nullptr.
// d_wire_len (fixed stride only): the true lengths of decoded calldata.  Synchronises `s` once, after the count, to lay the slots out and
// learn the groups' sub-batch sizes.
static int run_router(zkv_ctx* c, size_t n, const uint8_t* d_seals, const uint64_t* d_seal_off, uint64_t seal_bytes, const uint8_t* d_a, const uint8_t* d_b,
                      uint8_t* d_status, uint8_t* d_recv, hipStream_t s, const uint8_t* d_method = nullptr, const uint32_t* d_wire_len = nullptr) {
    int rc;
    const size_t blocks = (n + 255) / 256, R = c->gw_sel.size(), NB = c->rz_nb, K = R - NB;
    // slots: one per routed seal, and up to 31 pad slots behind every keyed route (its successor starts on a wavefront of the Miller mapping);
    // the same bound with the aggregate check on the keyed group (run_gateway)
    const size_t ns = n + 32 * K;
    RouterMem& rm = c->m_rz;
    if ((rc = grow_all(rm.cnt, 4 * GW_COLS * blocks, rm.totals, 4 * GW_COLS, rm.itot, 4 * (RZR_BAD_WORD + 1), rm.pos, 4 * n, rm.idx, 4 * ns,
                       rm.recs, (size_t)ZKV_SEAL_BYTES * ns + 8, rm.len, 4 * ns, rm.a, 32 * ns, rm.b, 32 * ns, rm.inst, 4 * ns, rm.st, ns, rm.rv, 4 * ns,
                       rm.skey, 4 * ns)) != ZKV_OK || (d_method && (rc = rm.kind.grow(ns)) != ZKV_OK)) return rc;
    if ((rc = order_after_previous(c, s)) != ZKV_OK) return rc;
    if (K && !rm.routes) {                                         // the keyed routes' constants, once
        if ((rc = rm.routes.grow(sizeof(RzrRoute) * K)) != ZKV_OK) return rc;
        HIP_TRY(hipMemcpy(rm.routes, c->rz_routes.data(), sizeof(RzrRoute) * K, hipMemcpyHostToDevice));
    }
    RzrArgs a;
    memset(&a, 0, sizeof a);
    a.n = n; a.seals = d_seals; a.seal_off = d_seal_off; a.seal_bytes = seal_bytes; a.stride = ZKV_SEAL_BYTES; a.in_a = d_a; a.in_b = d_b;
    a.method = d_method; a.wire_len = d_wire_len; a.c_kind = d_method ? rm.kind : nullptr;
    a.n_builtin = (uint32_t)NB; a.n_keyed = (uint32_t)K;
    for (size_t r = 0; r < R; r++) a.sel[r] = c->gw_sel[r];
    a.cnt = rm.cnt; a.totals = rm.totals; a.inst_tot = rm.itot; a.pos = rm.pos; a.idx = rm.idx;
    a.c_seals = rm.recs; a.c_len = rm.len; a.c_a = rm.a; a.c_b = rm.b; a.c_inst = rm.inst;
    a.status = d_status; a.recv = d_recv;
    HIP_TRY(hipMemsetAsync(a.inst_tot, 0, 4 * (RZR_BAD_WORD + 1), s));
    if (K) HIP_TRY(hipMemsetAsync(a.idx, 0xFF, 4 * ns, s));       // pad slots: GW_NONE
    launch_rzrouter_count(a, s);
    HIP_TRY(hipGetLastError());
    uint32_t tot[GW_COLS], itot[RZR_BAD_WORD + 1];                 // (the routes' words, then the bad-calldata word)
    HIP_TRY(hipMemcpyAsync(tot, rm.totals, sizeof tot, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipMemcpyAsync(itot, rm.itot, sizeof itot, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    // The layout (zkv_gset_layout.h route_layout).  The built-in group takes one slot per seal from slot 0; the keyed routes take the key
    // sets' layout behind it (gset_choose: the mapping their seals would take, stepped to a finer one while the padding exceeds 1.25 times).
    const size_t n0 = tot[RZR_COL_BUILTIN];
    size_t placed = 0;
    for (size_t k = 0; k < K; k++) placed += tot[RZR_COL_KEYED0 + k];
    const size_t routed = n0 + placed;
    std::unique_lock<std::mutex> glk;
    if (K) glk = std::unique_lock<std::mutex>(c->gw_group->mu);
    uint32_t rec[RZR_COL_KEYED0 + RZR_MAX_KEYED];
    for (uint32_t& v : rec) v = ZKV_SEAL_BYTES;
    KeyedAgg ka;                                                   // (the aggregate check on the keyed group: decided before the layout, as run_gateway does)
    int glanes = 0;
    if (K && (rc = keyed_group_begin(c->gw_group, tot + RZR_COL_KEYED0, K, placed, s, &ka, &glanes)) != ZKV_OK) return rc;
    RouteLayout L;
    RouteAggLayout A;
    route_layout_agg(tot, (uint32_t)(RZR_COL_KEYED0 + K), RZR_COL_KEYED0, (uint32_t)K, rec, glanes, K && c->gw_group->lanes != 0, ka.capable, ka.sub, &L, &A);
    ka.R = A.R;
    for (size_t k = 0; k <= K; k++) ka.astart[k] = A.astart[k];
    for (size_t q = 0; q < RZR_COL_KEYED0 + K; q++) a.start[q] = L.start[q];
    for (size_t k = 0; k < K; k++) { a.agg[RZR_COL_KEYED0 + k] = A.agg[k]; a.astart[RZR_COL_KEYED0 + k] = (uint32_t)(L.g0 + A.astart[k]); }
    uint64_t isum = 0;
    for (size_t r = 0; r < NB; r++) isum += itot[r];
    const uint32_t n_bad = itot[RZR_BAD_WORD];                     // in the short column
    if (routed + tot[RZR_COL_NOT_FOUND] + tot[RZR_COL_SHORT] != n || L.slots > ns || isum != n0 || n_bad > tot[RZR_COL_SHORT]) return ZKV_ERR_HIP;
    launch_rzrouter_place(a, s);
    HIP_TRY(hipGetLastError());
    uint8_t *st = rm.st, *rv = rm.rv;
    if (n0 && (rc = run_router_builtin(c->kid[0], n0, a.c_seals, a.c_len, a.c_inst, a.c_a, d_b ? a.c_b : nullptr, a.c_kind, st, rv, s)) != ZKV_OK) return rc;
    if (routed > n0) {                                             // the keyed group: k_rzrouter_prep with the slot's route, then the key sets' stages
        const size_t G0 = (size_t)L.g0;
        zkv_ctx* g = c->gw_group;
        RzrChunk pc;
        memset(&pc, 0, sizeof pc);
        pc.idx = a.idx + G0; pc.skey = rm.skey;
        pc.recs = a.c_seals + L.b0; pc.len = a.c_len + G0; pc.in_a = a.c_a + 32 * G0; pc.in_b = a.in_b ? a.c_b + 32 * G0 : nullptr;
        pc.kind = a.c_kind ? a.c_kind + G0 : nullptr;
        pc.n_keys = (uint32_t)K;
        for (size_t k = 0; k < K; k++) { pc.start[k] = (uint32_t)L.gstart[k]; pc.astart[k] = (uint32_t)A.astart[k]; }
        pc.agg_r = (uint32_t)A.R;
        pc.routes = rm.routes;
        pc.status = st + G0; pc.recv = (uint32_t*)(rv + 4 * G0);
        if ((rc = run_keyed_group(g, (size_t)L.m, L.lanes, ka, pc.idx, pc.skey, pc.status, s, [&](const GsetChunk& ch) {
                keyed_prep_chunk(&pc, ch);
                launch_rzrouter_prep(pc, c->consts, g->ws, s); })) != ZKV_OK) return rc;
    }
    HIP_TRY(hipSetDevice(c->device));
    route_return(L, a.idx, st, rv, d_status, d_recv, s);                 // (a keyed route may end in pad slots)
    HIP_TRY(hipGetLastError());
    if ((rc = mark_done(c, s)) != ZKV_OK) return rc;
    // the counts of the most recent call: only a call that enqueued everything replaces them
    for (size_t r = 0; r < NB; r++) c->rz_counts[r] = itot[r];
    for (size_t k = 0; k < K; k++) c->rz_counts[NB + k] = tot[RZR_COL_KEYED0 + k];
    c->rz_counts[R] = tot[RZR_COL_NOT_FOUND]; c->rz_counts[R + 1] = tot[RZR_COL_SHORT] - n_bad; c->rz_bad = n_bad;
    c->kid_ran[0] = n0 > 0; c->kid_ran[1] = routed > n0;
    return ZKV_OK;
}
ZKV_EXPORT int zkv_risc0_router_verify_batch_dev(zkv_ctx* c, size_t n, const uint8_t* d_seals, const uint8_t* d_image_ids, const uint8_t* d_journal_digests,
                                                 uint8_t* d_status, uint8_t* d_recv, void* stream) {
    if (!c || c->vm != ZKV_VM_RISC0_ROUTER || c->rz_set) return ZKV_ERR_WRONG_CTX;      // (a set seal has no fixed stride: zkv_risc0_router_verify_ragged_dev)
    if (n && (!d_seals || !d_image_ids || !d_status)) return ZKV_ERR_INVALID_ARG;
    if (!n) return ZKV_OK;
    if (n > 0xFFFFFFF0u / ZKV_SEAL_BYTES) return ZKV_ERR_INVALID_ARG;
    std::lock_guard<std::mutex> lk(c->mu);
    int rc = ctx_device_init(c);
    if (rc != ZKV_OK) return rc;
    return run_router(c, n, d_seals, nullptr, 0, d_image_ids, d_journal_digests, d_status, d_recv, stream ? (hipStream_t)stream : c->stream);
}
// host buffers: in_b == nullptr selects verify_integrity; method: the per-seal method row (in_b is then set), or nullptr
static int run_router_set(zkv_ctx* c, size_t n, const uint8_t* d_seals, const uint64_t* d_seal_off, uint64_t seal_bytes, const uint8_t* d_a, const uint8_t* d_b,
                          uint8_t* d_status, uint8_t* d_recv, hipStream_t s, uint32_t fp_mask, uint32_t* d_diag, const uint8_t* d_method = nullptr,
                          const RzWireArgs* wire = nullptr, const RzsSpan* d_span = nullptr);
static int router_host_batch(zkv_ctx* c, size_t n, const uint8_t* seal_blob, const uint64_t* seal_off, const uint8_t* in_a, const uint8_t* in_b,
                             uint8_t* status, uint8_t* recv, const uint8_t* method = nullptr) {
    if (n > 0xFFFFFFF0u / ZKV_SEAL_BYTES || !offsets_ok(seal_off, n)) return ZKV_ERR_INVALID_ARG;
    std::lock_guard<std::mutex> lk(c->mu);
    int rc = ctx_device_init(c);
    if (rc != ZKV_OK) return rc;
    RouterMem& rm = c->m_rz;
    if ((rc = grow_all(rm.h_a, 32 * n, rm.h_b, 32 * n, rm.h_st, n, rm.h_rv, 4 * n)) != ZKV_OK || (method && (rc = rm.h_method.grow(n)) != ZKV_OK)) return rc;
    hipStream_t s = c->stream;
    if ((rc = order_after_previous(c, s)) != ZKV_OK) return rc;
    std::vector<uint64_t> so;
    uint64_t sbytes = 0;
    if ((rc = stage_ragged(rm.h_seals, rm.h_off, seal_blob, seal_off, n, &so, s, &sbytes)) != ZKV_OK) return rc;
    HIP_TRY(hipMemcpyAsync(rm.h_a, in_a, 32 * n, hipMemcpyHostToDevice, s));
    if (in_b) HIP_TRY(hipMemcpyAsync(rm.h_b, in_b, 32 * n, hipMemcpyHostToDevice, s));
    if (method) HIP_TRY(hipMemcpyAsync(rm.h_method, method, n, hipMemcpyHostToDevice, s));
    if (c->rz_set) rc = run_router_set(c, n, rm.h_seals, rm.h_off, sbytes, rm.h_a, in_b ? rm.h_b : nullptr, rm.h_st, rm.h_rv, s, 0xFFFFFFFFu, nullptr,
                                       method ? rm.h_method : nullptr);
    else rc = run_router(c, n, rm.h_seals, rm.h_off, sbytes, rm.h_a, in_b ? rm.h_b : nullptr, rm.h_st, rm.h_rv, s, method ? rm.h_method : nullptr);
    if (rc != ZKV_OK) return rc;
    return return_to_host(rm.h_st, rm.h_rv, n, status, recv, s);
}
ZKV_EXPORT int zkv_risc0_router_verify_batch(zkv_ctx* c, size_t n, const uint8_t* seal_blob, const uint64_t* seal_off, const uint8_t* image_ids,
                                             const uint8_t* journal_digests, uint8_t* status, uint8_t* recv) {
    if (!c || c->vm != ZKV_VM_RISC0_ROUTER) return ZKV_ERR_WRONG_CTX;
    if (n && (!seal_blob || !seal_off || !image_ids || !journal_digests || !status)) return ZKV_ERR_INVALID_ARG;
    if (!n) return ZKV_OK;
    return router_host_batch(c, n, seal_blob, seal_off, image_ids, journal_digests, status, recv);
}
ZKV_EXPORT int zkv_risc0_router_verify_integrity_batch(zkv_ctx* c, size_t n, const uint8_t* seal_blob, const uint64_t* seal_off, const uint8_t* claim_digests,
                                                       uint8_t* status, uint8_t* recv) {
    if (!c || c->vm != ZKV_VM_RISC0_ROUTER) return ZKV_ERR_WRONG_CTX;
    if (n && (!seal_blob || !seal_off || !claim_digests || !status)) return ZKV_ERR_INVALID_ARG;
    if (!n) return ZKV_OK;
    return router_host_batch(c, n, seal_blob, seal_off, claim_digests, nullptr, status, recv);
}
ZKV_EXPORT int zkv_risc0_router_verify(zkv_ctx* c, const uint8_t* seal, size_t seal_len, const uint8_t image_id[32], const uint8_t journal_digest[32],
                                       uint8_t* status, uint8_t recv[4]) {
    const uint64_t off[2] = {0, seal_len};
    const uint8_t dummy = 0;
    if (!seal && seal_len) return ZKV_ERR_INVALID_ARG;
    return zkv_risc0_router_verify_batch(c, 1, seal ? seal : &dummy, off, image_id, journal_digest, status, recv);
}
ZKV_EXPORT int zkv_risc0_router_verify_integrity(zkv_ctx* c, const uint8_t* seal, size_t seal_len, const uint8_t claim_digest[32], uint8_t* status,
                                                 uint8_t recv[4]) {
    const uint64_t off[2] = {0, seal_len};
    const uint8_t dummy = 0;
    if (!seal && seal_len) return ZKV_ERR_INVALID_ARG;
    return zkv_risc0_router_verify_integrity_batch(c, 1, seal ? seal : &dummy, off, claim_digest, status, recv);
}
ZKV_EXPORT int zkv_risc0_router_last_route_counts(zkv_ctx* c, uint64_t* out) {
    if (!c || c->vm != ZKV_VM_RISC0_ROUTER) return ZKV_ERR_WRONG_CTX;
    if (!out) return ZKV_ERR_INVALID_ARG;
    std::lock_guard<std::mutex> lk(c->mu);
    const std::vector<uint64_t>& v = c->rz_set ? c->rzs_counts : c->rz_counts;
    for (size_t r = 0; r < v.size(); r++) out[r] = v[r];
    return ZKV_OK;
}
ZKV_EXPORT int zkv_risc0_router_status_abi_encode(const zkv_ctx* c, uint8_t status, const uint8_t received[4], uint8_t out[68]) {
    if (!c || c->vm != ZKV_VM_RISC0_ROUTER) return ZKV_ERR_WRONG_CTX;
    if (!out) return ZKV_ERR_INVALID_ARG;
    if (status == ZKV_STATUS_ROUTE_NOT_FOUND) return received ? abi_encode_error_bytes4("SelectorUnknown(bytes4)", received, out) : ZKV_ERR_INVALID_ARG;
    uint8_t expected[4];
    be32_put(expected, c->gw_sel[0]);
    return zkv_status_abi_encode(ZKV_VM_RISC0, status, received, expected, out);
}

// ------------------------------------------------------------------ on-chain wire layer (eth_call batches)
ZKV_EXPORT int zkv_abi_function_selector(const char* signature, uint8_t out[4]) {
    if (!signature || !out) return ZKV_ERR_INVALID_ARG;
    host::fn_selector(signature, out);
    return ZKV_OK;
}
ZKV_EXPORT size_t zkv_risc0_encode_verify_call(const uint8_t* seal, size_t seal_len, const uint8_t image_id[32], const uint8_t journal_digest[32],
                                               uint8_t* out, size_t cap) {
    const size_t need = 4 + 96 + 32 * (seal_len + 1);
    if (!out || cap < need || (seal_len && !seal) || !image_id || !journal_digest) return need;
    memcpy(out, host::selectors().risc0[host::R0_VERIFY], 4);
    host::abi_word_u32(out + 4, 0x60); memcpy(out + 36, image_id, 32); memcpy(out + 68, journal_digest, 32);
    host::abi_u8_array(out + 100, seal, seal_len);
    return need;
}
ZKV_EXPORT size_t zkv_risc0_encode_verify_integrity_call(const uint8_t* seal, size_t seal_len, const uint8_t claim_digest[32], uint8_t* out, size_t cap) {
    const size_t need = 4 + 64 + 32 * (seal_len + 1);
    if (!out || cap < need || (seal_len && !seal) || !claim_digest) return need;
    memcpy(out, host::selectors().risc0[host::R0_VERIFY_INTEGRITY], 4);
    host::abi_word_u32(out + 4, 0x40); memcpy(out + 36, claim_digest, 32);
    host::abi_u8_array(out + 68, seal, seal_len);
    return need;
}
ZKV_EXPORT size_t zkv_sp1_encode_verify_proof_call(const uint8_t program_vkey[32], const uint8_t* pv, size_t pv_len, const uint8_t* proof, size_t proof_len,
                                                   uint8_t* out, size_t cap) {
    const size_t need = 4 + 96 + 32 * (pv_len + 1) + 32 * (proof_len + 1);
    if (!out || cap < need || (pv_len && !pv) || (proof_len && !proof) || !program_vkey) return need;
    memcpy(out, host::selectors().sp1[host::SP1_VERIFY_PROOF], 4);
    memcpy(out + 4, program_vkey, 32); host::abi_word_u32(out + 36, 0x60); host::abi_word_u32(out + 68, 0x80 + 32 * (uint64_t)pv_len);
    size_t k = host::abi_u8_array(out + 100, pv, pv_len);
    host::abi_u8_array(out + 100 + k, proof, proof_len);
    return need;
}

// Return / revert data of a verify-class call from its status (success: `true` word for RISC Zero, nothing for SP1).
static void verify_returndata(const zkv_ctx* c, uint8_t st, const uint8_t* recv, uint8_t* out, uint32_t* out_len, uint8_t* reverted) {
    if (st == ZKV_STATUS_OK) {
        *reverted = 0;
        if (c->vm == ZKV_VM_RISC0) { host::abi_word_u32(out, 1); *out_len = 32; } else *out_len = 0;
        return;
    }
    *reverted = 1;
    if (st == ZKV_STATUS_BAD_CALLDATA) { *out_len = 0; return; }
    int k = zkv_status_abi_encode(c->vm, st, recv, c->vm == ZKV_VM_RISC0 ? c->selector : host::SP1_VERIFIER_HASH, out);
    *out_len = k > 0 ? (uint32_t)k : 0;
}
// Calls the device left as BAD_CALLDATA: either one of the constant-size methods (answered here) or really undecodable.
static void host_method(const zkv_ctx* c, const uint8_t* cd, size_t len, uint8_t* out, uint32_t* out_len, uint8_t* reverted) {
    *out_len = 0; *reverted = 1;
    if (len < 4) return;
    const host::Selectors& S = host::selectors();
    if (c->vm == ZKV_VM_RISC0) {
        int k = -1;
        for (int i = 0; i < host::R0_COUNT; i++) if (!memcmp(S.risc0[i], cd, 4)) k = i;
        if (k < 0 || k == host::R0_VERIFY || k == host::R0_VERIFY_INTEGRITY) return;
        if (k == host::R0_INITIALIZE) {                      // eth_call simulates the transaction; nothing is stored
            if (len != 4 + 64) return;
            if (c->initialized) *out_len = (uint32_t)zkv_status_abi_encode(ZKV_VM_RISC0, ZKV_STATUS_ALREADY_INITIALIZED, nullptr, nullptr, out);
            else *reverted = 0;
            return;
        }
        if (len != 4) return;
        *reverted = 0; *out_len = 32;
        if (k == host::R0_IS_INITIALIZED) host::abi_word_u32(out, c->initialized ? 1 : 0);
        else if (k == host::R0_GET_SELECTOR) host::abi_word_left(out, c->selector, 4);
        else if (k == host::R0_GET_CONTROL_ROOT) { host::abi_word_left(out, c->control_root_0, 16); host::abi_word_left(out + 32, c->control_root_1, 16); *out_len = 64; }
        else if (k == host::R0_GET_BN254_CONTROL_ID) memcpy(out, c->control_id, 32);
        else host::risc0_vk_digest(out);
    } else {
        int k = -1;
        for (int i = 0; i < host::SP1_COUNT; i++) if (!memcmp(S.sp1[i], cd, 4)) k = i;
        if (k <= host::SP1_VERIFY_PROOF || len != 4) return;
        *reverted = 0;
        if (k == host::SP1_FN_VERIFIER_HASH) { memcpy(out, host::SP1_VERIFIER_HASH, 32); *out_len = 32; return; }
        const size_t vl = strlen(host::SP1_VERSION);
        host::abi_word_u32(out, 0x20); host::abi_word_u32(out + 32, vl); memset(out + 64, 0, 32); memcpy(out + 64, host::SP1_VERSION, vl);
        *out_len = 96;
    }
}

// Decode + verify one chunk whose calldata and offsets are already on the device.
static int enqueue_wire_chunk(zkv_ctx* c, size_t m, const uint8_t* d_cd, const uint64_t* d_cdoff, uint64_t cd_bytes, uint8_t* d_status, uint8_t* d_recv,
                              hipStream_t s, bool timed, hipEvent_t decoded = nullptr) {
    int rc;
    if ((rc = c->d_blob.grow(m * ZKV_SEAL_BYTES + 8)) != ZKV_OK) return rc;
    if (c->vm == ZKV_VM_SP1 && (rc = c->d_pv.grow((size_t)(cd_bytes / 32) + 64)) != ZKV_OK) return rc;
    const host::Selectors& S = host::selectors();
    WireArgs w;
    memset(&w, 0, sizeof w);
    w.n = m; w.cd = d_cd; w.off = d_cdoff; w.cd_bytes = cd_bytes;
    w.seals = c->d_blob; w.seal_len = c->d_len; w.in_a = c->d_a; w.in_b = c->d_b; w.kind = c->d_kind;
    w.pv = c->d_pv; w.pv_off = c->d_pvoff; w.pv_len = c->d_pvlen;
    if (timed) (void)hipEventRecord(c->ev_wire[0], s);
    if (c->vm == ZKV_VM_RISC0) {
        w.sel_a_be = be32_of(S.risc0[host::R0_VERIFY]); w.sel_b_be = be32_of(S.risc0[host::R0_VERIFY_INTEGRITY]);
        launch_wire_risc0(w, s);
    } else {
        w.sel_a_be = be32_of(S.sp1[host::SP1_VERIFY_PROOF]);
        launch_wire_sp1(w, s);
    }
    if (timed) { (void)hipEventRecord(c->ev_wire[1], s); c->wire_timed = true; }
    if (decoded) (void)hipEventRecord(decoded, s);           // the calldata buffer may be overwritten from here on
    PrepArgs a;
    memset(&a, 0, sizeof a);
    a.n = m; a.blob = c->d_blob; a.off = nullptr; a.stride = ZKV_SEAL_BYTES; a.len = c->d_len;
    a.in32_a = c->d_a;
    if (c->vm == ZKV_VM_RISC0) {
        a.in32_b = c->d_b; a.kind = c->d_kind;
        a.selector_be = be32_of(c->selector);
        a.force_fail = c->id_ge_r ? 1u : 0u;
        a.not_initialized = c->initialized ? 0u : 1u;
    } else {
        a.pv_blob = c->d_pv; a.pv_off = c->d_pvoff; a.pv_len = c->d_pvlen;
        a.selector_be = be32_of(host::SP1_VERIFIER_HASH);
    }
    a.status = d_status; a.recv = d_recv;
    enqueue_chunk(c, a, s, timed);
    return ZKV_OK;
}

// Host calldata: 8-12 KB per proof cross PCIe, as much time as the verification itself.  Chunks of at most 2^16 requests
// (enough lanes to fill the chip) are double-buffered: the H2D copy of chunk k+1 runs on its own stream while chunk k is
// decoded and verified; statuses stay on the device until the whole batch is done, so the host never waits inside the loop.
static size_t wire_host_chunk(size_t cap) {
    const char* e = getenv("ZKV_WIRE_HOST_CHUNK");
    size_t v = e ? (size_t)strtoull(e, nullptr, 10) : (size_t)1 << 16;
    if (v < 1) v = 1;
    return v < cap ? v : cap;
}
static int run_eth_call_batch(zkv_ctx* c, size_t n, const uint8_t* blob, const uint64_t* off, uint8_t* reverted, uint8_t* returndata,
                              uint32_t* returndata_len, uint8_t* status) {
    if (!c || (n && (!blob || !off || !reverted || !returndata || !returndata_len))) return ZKV_ERR_INVALID_ARG;
    if (!n) return ZKV_OK;
    if (!offsets_ok(off, n)) return ZKV_ERR_INVALID_ARG;
    std::lock_guard<std::mutex> lk(c->mu);
    int rc = ctx_ready(c, n);
    if (rc != ZKV_OK) return rc;
    if ((rc = order_after_previous(c, c->stream)) != ZKV_OK) return rc;
    const size_t chunk = wire_host_chunk(c->ws.cap);
    if ((rc = c->d_st_all.grow(n)) != ZKV_OK || (rc = c->d_rv_all.grow(4 * n)) != ZKV_OK) return rc;
    uint64_t max_bytes = 0;
    for (size_t base = 0; base < n; base += chunk) {
        size_t m = n - base < chunk ? n - base : chunk;
        uint64_t bytes = off[base + m] - off[base];
        if (bytes > max_bytes) max_bytes = bytes;
    }
    // all device buffers are sized before the loop: growing one frees it, which synchronises the device
    for (int b = 0; b < 2; b++)
        if ((n > chunk || b == 0) && (rc = c->d_cd[b].grow((size_t)max_bytes + 8)) != ZKV_OK) return rc;
    if ((rc = c->d_blob.grow(chunk * ZKV_SEAL_BYTES + 8)) != ZKV_OK) return rc;
    if (c->vm == ZKV_VM_SP1 && (rc = c->d_pv.grow((size_t)(max_bytes / 32) + 64)) != ZKV_OK) return rc;
    std::vector<uint64_t> rel[2];
    size_t k = 0;
    for (size_t base = 0; base < n; base += chunk, k++) {
        const size_t m = n - base < chunk ? n - base : chunk;
        const int b = (int)(k & 1);
        const uint64_t b0 = off[base], bytes = off[base + m] - b0;
        if (k >= 2) HIP_TRY(hipStreamWaitEvent(c->copy_stream, c->ev_decoded[b], 0));     // chunk k-2 has been decoded out of this buffer
        HIP_TRY(hipStreamSynchronize(c->copy_stream));                                    // rel[b] of chunk k-2 is no longer being read
        rel[b].resize(m + 1);
        for (size_t i = 0; i <= m; i++) rel[b][i] = off[base + i] - b0;
        HIP_TRY(hipMemcpyAsync(c->d_cdoff[b], rel[b].data(), sizeof(uint64_t) * (m + 1), hipMemcpyHostToDevice, c->copy_stream));
        if (bytes) HIP_TRY(hipMemcpyAsync(c->d_cd[b], blob + b0, (size_t)bytes, hipMemcpyHostToDevice, c->copy_stream));
        HIP_TRY(hipEventRecord(c->ev_copied[b], c->copy_stream));
        HIP_TRY(hipStreamWaitEvent(c->stream, c->ev_copied[b], 0));
        if ((rc = enqueue_wire_chunk(c, m, c->d_cd[b], c->d_cdoff[b], bytes, c->d_st_all + base, c->d_rv_all + 4 * base, c->stream,
                                     base + chunk >= n, c->ev_decoded[b])) != ZKV_OK) return rc;
        HIP_TRY(hipGetLastError());
    }
    std::vector<uint8_t> st(n), rv(4 * n);
    HIP_TRY(hipMemcpyAsync(st.data(), c->d_st_all, n, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipMemcpyAsync(rv.data(), c->d_rv_all, 4 * n, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    HIP_TRY(hipStreamSynchronize(c->copy_stream));
    for (size_t i = 0; i < n; i++) {
        uint8_t* out = returndata + i * ZKV_RETURNDATA_STRIDE;
        if (st[i] == ZKV_STATUS_BAD_CALLDATA) host_method(c, blob + off[i], (size_t)(off[i + 1] - off[i]), out, &returndata_len[i], &reverted[i]);
        else verify_returndata(c, st[i], rv.data() + 4 * i, out, &returndata_len[i], &reverted[i]);
        if (status) status[i] = st[i];
    }
    return ZKV_OK;
}
ZKV_EXPORT int zkv_risc0_eth_call_batch(zkv_ctx* c, size_t n, const uint8_t* calldata_blob, const uint64_t* calldata_off, uint8_t* reverted,
                                        uint8_t* returndata, uint32_t* returndata_len, uint8_t* status) {
    if (!c || c->vm != ZKV_VM_RISC0) return ZKV_ERR_WRONG_CTX;
    if (is_sharded(c)) {
        if (n && (!calldata_blob || !calldata_off || !reverted || !returndata || !returndata_len)) return ZKV_ERR_INVALID_ARG;
        return run_sharded(c, n, [&](zkv_ctx* k, size_t lo, size_t hi) {
            return zkv_risc0_eth_call_batch(k, hi - lo, calldata_blob, calldata_off + lo, reverted + lo, returndata + lo * ZKV_RETURNDATA_STRIDE, returndata_len + lo, status ? status + lo : nullptr); });
    }
    return run_eth_call_batch(c, n, calldata_blob, calldata_off, reverted, returndata, returndata_len, status);
}
ZKV_EXPORT int zkv_sp1_eth_call_batch(zkv_ctx* c, size_t n, const uint8_t* calldata_blob, const uint64_t* calldata_off, uint8_t* reverted,
                                      uint8_t* returndata, uint32_t* returndata_len, uint8_t* status) {
    if (!c || c->vm != ZKV_VM_SP1) return ZKV_ERR_WRONG_CTX;
    if (is_sharded(c)) {
        if (n && (!calldata_blob || !calldata_off || !reverted || !returndata || !returndata_len)) return ZKV_ERR_INVALID_ARG;
        return run_sharded(c, n, [&](zkv_ctx* k, size_t lo, size_t hi) {
            return zkv_sp1_eth_call_batch(k, hi - lo, calldata_blob, calldata_off + lo, reverted + lo, returndata + lo * ZKV_RETURNDATA_STRIDE, returndata_len + lo, status ? status + lo : nullptr); });
    }
    return run_eth_call_batch(c, n, calldata_blob, calldata_off, reverted, returndata, returndata_len, status);
}
// Device-resident calldata: verify-class calls only, statuses stay on the device.
ZKV_EXPORT int zkv_eth_call_batch_dev(zkv_ctx* c, size_t n, const uint8_t* d_calldata, const uint64_t* d_calldata_off, uint64_t calldata_bytes,
                                      uint8_t* d_status, uint8_t* d_recv, void* stream) {
    if (is_sharded(c)) c = c->shards[0];                 // calldata offsets are absolute into one blob: this entry point stays on one GPU
    if (!c || (c->vm != ZKV_VM_RISC0 && c->vm != ZKV_VM_SP1)) return ZKV_ERR_WRONG_CTX;
    if (n && (!d_calldata || !d_calldata_off || !d_status)) return ZKV_ERR_INVALID_ARG;
    if (!n) return ZKV_OK;
    std::lock_guard<std::mutex> lk(c->mu);
    int rc = ctx_ready(c, n);
    if (rc != ZKV_OK) return rc;
    hipStream_t s = stream ? (hipStream_t)stream : c->stream;
    const size_t cap = c->ws.cap;
    if ((rc = order_after_previous(c, s)) != ZKV_OK) return rc;
    for (size_t base = 0; base < n; base += cap) {
        size_t m = n - base < cap ? n - base : cap;
        // offsets are absolute into d_calldata, so chunks share the blob pointer; the public-values scratch is sized for the whole blob
        if ((rc = enqueue_wire_chunk(c, m, d_calldata, d_calldata_off + base, calldata_bytes, d_status + base, d_recv ? d_recv + 4 * base : nullptr, s,
                                     base + cap >= n)) != ZKV_OK) return rc;
    }
    HIP_TRY(hipGetLastError());
    return mark_done(c, s);
}
ZKV_EXPORT int zkv_eth_call_returndata(const zkv_ctx* c, uint8_t status, const uint8_t recv_selector[4], uint8_t out[ZKV_RETURNDATA_STRIDE],
                                       uint32_t* out_len, uint8_t* reverted) {
    static const uint8_t zero[4] = {0, 0, 0, 0};
    if (!c || !out || !out_len || !reverted || (c->vm != ZKV_VM_RISC0 && c->vm != ZKV_VM_SP1) || status > ZKV_STATUS_BAD_CALLDATA) return ZKV_ERR_INVALID_ARG;
    verify_returndata(c, status, recv_selector ? recv_selector : zero, out, out_len, reverted);
    return ZKV_OK;
}
ZKV_EXPORT int zkv_ctx_last_wire_ms(zkv_ctx* c, float* out_ms) {
    if (is_sharded(c)) c = c->shards[0];
    if (!c || !out_ms) return ZKV_ERR_INVALID_ARG;
    if (!c->dev_ready || !c->wire_timed) return ZKV_ERR_NO_DEVICE;
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(hipEventSynchronize(c->ev_wire[1]));
    HIP_TRY(hipEventElapsedTime(out_ms, c->ev_wire[0], c->ev_wire[1]));
    return ZKV_OK;
}

// ------------------------------------------------------------------ SP1 gateway: eth_call batches (zkv_sp1_gateway_wire.h; parity unpinned)
// verifyProof calls to the gateway in either calldata form: k_wire_gateway turns every request into a record, the demultiplexer takes the
// records instead of offsets, and everything after it is the decoded-input path.
static const uint8_t* gateway_bytes_selector() {
    static const struct Sel { uint8_t b[4]; Sel() { host::fn_selector("verifyProof(bytes32,bytes,bytes)", b); } } s;
    return s.b;
}
ZKV_EXPORT size_t zkv_sp1_gateway_encode_verify_proof_call(int form, const uint8_t program_vkey[32], const uint8_t* pv, size_t pv_len, const uint8_t* proof,
                                                           size_t proof_len, uint8_t* out, size_t cap) {
    if (form == ZKV_CALLDATA_FORM_UINT8_ARRAY) return zkv_sp1_encode_verify_proof_call(program_vkey, pv, pv_len, proof, proof_len, out, cap);
    if (form != ZKV_CALLDATA_FORM_BYTES) return 0;
    const size_t pv_pad = (pv_len + 31) & ~(size_t)31, proof_pad = (proof_len + 31) & ~(size_t)31;
    const size_t need = 4 + 96 + 32 + pv_pad + 32 + proof_pad;
    if (!out || cap < need || (pv_len && !pv) || (proof_len && !proof) || !program_vkey) return need;
    memset(out, 0, need);
    memcpy(out, gateway_bytes_selector(), 4);
    memcpy(out + 4, program_vkey, 32); host::abi_word_u32(out + 36, 0x60); host::abi_word_u32(out + 68, 0x80 + (uint64_t)pv_pad);
    host::abi_word_u32(out + 100, pv_len);
    if (pv_len) memcpy(out + 132, pv, pv_len);
    host::abi_word_u32(out + 132 + pv_pad, proof_len);
    if (proof_len) memcpy(out + 164 + pv_pad, proof, proof_len);
    return need;
}
ZKV_EXPORT int zkv_sp1_gateway_eth_call_returndata(const zkv_ctx* c, uint8_t status, const uint8_t recv_selector[4], uint8_t out[ZKV_RETURNDATA_STRIDE],
                                                   uint32_t* out_len, uint8_t* reverted) {
    static const uint8_t zero[4] = {0, 0, 0, 0};
    if (!c || c->vm != ZKV_VM_SP1_GATEWAY) return ZKV_ERR_WRONG_CTX;
    if (!out || !out_len || !reverted) return ZKV_ERR_INVALID_ARG;
    *out_len = 0;
    if (status == ZKV_STATUS_OK) { *reverted = 0; return ZKV_OK; }      // verifyProof returns nothing
    *reverted = 1;
    if (status == ZKV_STATUS_BAD_CALLDATA) return ZKV_OK;               // the router could not decode the call: empty revert data
    const int k = zkv_sp1_gateway_status_abi_encode(c, status, recv_selector ? recv_selector : zero, out);
    if (k < 0) return k;
    *out_len = (uint32_t)k;
    return ZKV_OK;
}
// Calldata and its n + 1 offsets on the device.  The decode is enqueued in front of the count, so the call synchronises where run_gateway does.
static int run_gateway_wire(zkv_ctx* c, size_t n, const uint8_t* d_cd, const uint64_t* d_off, uint64_t cd_bytes, uint8_t* d_status, uint8_t* d_recv, hipStream_t s) {
    int rc;
    GatewayMem& gm = c->m_gw;
    if ((rc = grow_all(gm.w_vk, 32 * n, gm.w_pvat, 8 * n, gm.w_pvlen, 4 * n, gm.w_pat, 8 * n, gm.w_plen, 4 * n, gm.w_bad, n,
                       gm.w_arena, (size_t)(cd_bytes / 32) + 64)) != ZKV_OK) return rc;
    if ((rc = order_after_previous(c, s)) != ZKV_OK) return rc;
    GwWireArgs w;
    memset(&w, 0, sizeof w);
    w.n = n; w.cd = d_cd; w.off = d_off; w.cd_bytes = cd_bytes;
    w.sel_u_be = be32_of(host::selectors().sp1[host::SP1_VERIFY_PROOF]); w.sel_b_be = be32_of(gateway_bytes_selector());
    w.arena = gm.w_arena; w.vkeys = gm.w_vk; w.pv_at = gm.w_pvat; w.pv_len = gm.w_pvlen; w.proof_at = gm.w_pat; w.proof_len = gm.w_plen; w.bad = gm.w_bad;
    // one base address for the records: the lower of the two buffers, so that every start is a plain non-negative distance
    const uintptr_t pc = (uintptr_t)d_cd, pa = (uintptr_t)w.arena, base = pc < pa ? pc : pa;
    w.cd_delta = pc - base; w.arena_delta = pa - base;
    (void)hipEventRecord(c->ev_wire[0], s);
    launch_wire_gateway(w, s);
    (void)hipEventRecord(c->ev_wire[1], s);
    c->wire_timed = true;
    HIP_TRY(hipGetLastError());
    return run_gateway(c, n, w.vkeys, (const uint8_t*)base, nullptr, 0, (const uint8_t*)base, nullptr, 0, d_status, d_recv, s, &w);
}
ZKV_EXPORT int zkv_sp1_gateway_eth_call_batch_dev(zkv_ctx* c, size_t n, const uint8_t* d_calldata, const uint64_t* d_calldata_off, uint64_t calldata_bytes,
                                                  uint8_t* d_status, uint8_t* d_recv, void* stream) {
    if (!c || c->vm != ZKV_VM_SP1_GATEWAY) return ZKV_ERR_WRONG_CTX;
    if (n && (!d_calldata || !d_calldata_off || !d_status)) return ZKV_ERR_INVALID_ARG;
    if (!n) return ZKV_OK;
    if (n > 0xFFFFFFF0u) return ZKV_ERR_INVALID_ARG;
    std::lock_guard<std::mutex> lk(c->mu);
    int rc = ctx_device_init(c);
    if (rc != ZKV_OK) return rc;
    return run_gateway_wire(c, n, d_calldata, d_calldata_off, calldata_bytes, d_status, d_recv, stream ? (hipStream_t)stream : c->stream);
}
ZKV_EXPORT int zkv_sp1_gateway_eth_call_batch(zkv_ctx* c, size_t n, const uint8_t* blob, const uint64_t* off, uint8_t* reverted, uint8_t* returndata,
                                              uint32_t* returndata_len, uint8_t* status) {
    if (!c || c->vm != ZKV_VM_SP1_GATEWAY) return ZKV_ERR_WRONG_CTX;
    if (n && (!blob || !off || !reverted || !returndata || !returndata_len)) return ZKV_ERR_INVALID_ARG;
    if (!n) return ZKV_OK;
    if (n > 0xFFFFFFF0u || !offsets_ok(off, n)) return ZKV_ERR_INVALID_ARG;
    std::vector<uint8_t> st(n), rv(4 * n);
    {
        std::lock_guard<std::mutex> lk(c->mu);
        int rc = ctx_device_init(c);
        if (rc != ZKV_OK) return rc;
        const uint64_t b0 = off[0], bytes = off[n] - b0;
        GatewayMem& gm = c->m_gw;
        if ((rc = grow_all(gm.h_cd, (size_t)bytes + 8, gm.h_cdoff, 8 * (n + 1), gm.h_st, n, gm.h_rv, 4 * n)) != ZKV_OK) return rc;
        hipStream_t s = c->stream;
        if ((rc = order_after_previous(c, s)) != ZKV_OK) return rc;
        std::vector<uint64_t> rel(off, off + n + 1);
        for (auto& v : rel) v -= b0;
        if (bytes) HIP_TRY(hipMemcpyAsync(gm.h_cd, blob + b0, (size_t)bytes, hipMemcpyHostToDevice, s));
        HIP_TRY(hipMemcpyAsync(gm.h_cdoff, rel.data(), 8 * (n + 1), hipMemcpyHostToDevice, s));
        HIP_TRY(hipStreamSynchronize(s));                        // `rel` is a pageable host buffer
        if ((rc = run_gateway_wire(c, n, gm.h_cd, gm.h_cdoff, bytes, gm.h_st, gm.h_rv, s)) != ZKV_OK ||
            (rc = return_to_host(gm.h_st, gm.h_rv, n, st.data(), rv.data(), s)) != ZKV_OK) return rc;
    }
    for (size_t i = 0; i < n; i++) {
        const int rc = zkv_sp1_gateway_eth_call_returndata(c, st[i], rv.data() + 4 * i, returndata + i * ZKV_RETURNDATA_STRIDE, &returndata_len[i], &reverted[i]);
        if (rc != ZKV_OK) return rc;
        if (status) status[i] = st[i];
    }
    return ZKV_OK;
}
ZKV_EXPORT int zkv_sp1_gateway_last_call_counts(zkv_ctx* c, uint64_t* out) {
    if (!c || c->vm != ZKV_VM_SP1_GATEWAY) return ZKV_ERR_WRONG_CTX;
    if (!out) return ZKV_ERR_INVALID_ARG;
    std::lock_guard<std::mutex> lk(c->mu);
    const size_t R = c->gw_route.size();
    for (size_t r = 0; r < R; r++) out[r] = c->gw_counts[r];
    out[R] = c->gw_counts[GW_COL_NOT_FOUND]; out[R + 1] = c->gw_counts[GW_COL_SHORT]; out[R + 2] = c->gw_counts[GW_COL_BAD];
    return ZKV_OK;
}

// ------------------------------------------------------------------ RISC Zero router: per-seal methods and eth_call batches (zkv_risc0_router_wire.h; parity unpinned)
// verify / verifyIntegrity calls to the router in either calldata form: k_wire_rzrouter turns every request into a fixed 260-byte slot, its
// true length, its inputs and its method; the router takes the slots as a fixed-stride batch with a true-length row and a method row, and
// everything after the count is the decoded-input path.
ZKV_EXPORT int zkv_risc0_router_verify_call_batch_dev(zkv_ctx* c, size_t n, const uint8_t* d_method, const uint8_t* d_seals, const uint8_t* d_in_a,
                                                      const uint8_t* d_in_b, uint8_t* d_status, uint8_t* d_recv, void* stream) {
    if (!c || c->vm != ZKV_VM_RISC0_ROUTER || c->rz_set) return ZKV_ERR_WRONG_CTX;
    if (n && (!d_seals || !d_in_a || !d_in_b || !d_status)) return ZKV_ERR_INVALID_ARG;
    if (!n) return ZKV_OK;
    if (n > 0xFFFFFFF0u / ZKV_SEAL_BYTES) return ZKV_ERR_INVALID_ARG;
    std::lock_guard<std::mutex> lk(c->mu);
    int rc = ctx_device_init(c);
    if (rc != ZKV_OK) return rc;
    return run_router(c, n, d_seals, nullptr, 0, d_in_a, d_in_b, d_status, d_recv, stream ? (hipStream_t)stream : c->stream, d_method);
}
ZKV_EXPORT int zkv_risc0_router_verify_call_batch(zkv_ctx* c, size_t n, const uint8_t* method, const uint8_t* seal_blob, const uint64_t* seal_off,
                                                  const uint8_t* in_a, const uint8_t* in_b, uint8_t* status, uint8_t* recv) {
    if (!c || c->vm != ZKV_VM_RISC0_ROUTER || c->rz_set) return ZKV_ERR_WRONG_CTX;
    if (n && (!seal_blob || !seal_off || !in_a || !in_b || !status)) return ZKV_ERR_INVALID_ARG;
    if (!n) return ZKV_OK;
    return router_host_batch(c, n, seal_blob, seal_off, in_a, in_b, status, recv, method);
}

// The four selectors, index 2 form + method (zkv_wire_rzrouter.h): the Stylus shell's uint8[] signatures, then IRiscZeroVerifier's.
static const uint8_t* router_call_selector(int kind) {
    static const struct Sels { uint8_t b[RZW_KINDS][4]; Sels() {
        host::fn_selector("verify(uint8[],bytes32,bytes32)", b[0]); host::fn_selector("verifyIntegrity(uint8[],bytes32)", b[1]);
        host::fn_selector("verify(bytes,bytes32,bytes32)", b[2]); host::fn_selector("verifyIntegrity((bytes,bytes32))", b[3]); } } s;
    return s.b[kind];
}
// sel | head words | L | the seal packed and zero padded: form B of either method (kind 2 or 3)
static size_t router_encode_bytes(int kind, const uint8_t* seal, size_t seal_len, const uint8_t* a, const uint8_t* b, uint8_t* out, size_t cap) {
    const size_t pad = (seal_len + 31) & ~(size_t)31, need = 4 + 96 + 32 + pad;
    if (!out || cap < need || (seal_len && !seal) || !a || (kind == 2 && !b)) return need;
    memset(out, 0, need);
    memcpy(out, router_call_selector(kind), 4);
    if (kind == 2) { host::abi_word_u32(out + 4, 0x60); memcpy(out + 36, a, 32); memcpy(out + 68, b, 32); }
    else { host::abi_word_u32(out + 4, 0x20); host::abi_word_u32(out + 36, 0x40); memcpy(out + 68, a, 32); }
    host::abi_word_u32(out + 100, seal_len);
    if (seal_len) memcpy(out + 132, seal, seal_len);
    return need;
}
ZKV_EXPORT size_t zkv_risc0_router_encode_verify_call(int form, const uint8_t* seal, size_t seal_len, const uint8_t image_id[32],
                                                      const uint8_t journal_digest[32], uint8_t* out, size_t cap) {
    if (form == ZKV_CALLDATA_FORM_UINT8_ARRAY) return zkv_risc0_encode_verify_call(seal, seal_len, image_id, journal_digest, out, cap);
    if (form != ZKV_CALLDATA_FORM_BYTES) return 0;
    return router_encode_bytes(2, seal, seal_len, image_id, journal_digest, out, cap);
}
ZKV_EXPORT size_t zkv_risc0_router_encode_verify_integrity_call(int form, const uint8_t* seal, size_t seal_len, const uint8_t claim_digest[32], uint8_t* out,
                                                                size_t cap) {
    if (form == ZKV_CALLDATA_FORM_UINT8_ARRAY) return zkv_risc0_encode_verify_integrity_call(seal, seal_len, claim_digest, out, cap);
    if (form != ZKV_CALLDATA_FORM_BYTES) return 0;
    return router_encode_bytes(3, seal, seal_len, claim_digest, nullptr, out, cap);
}
ZKV_EXPORT int zkv_risc0_router_eth_call_returndata(const zkv_ctx* c, uint8_t status, const uint8_t recv_selector[4], uint8_t call_kind,
                                                    uint8_t out[ZKV_RETURNDATA_STRIDE], uint32_t* out_len, uint8_t* reverted) {
    static const uint8_t zero[4] = {0, 0, 0, 0};
    if (!c || c->vm != ZKV_VM_RISC0_ROUTER) return ZKV_ERR_WRONG_CTX;
    if (!out || !out_len || !reverted) return ZKV_ERR_INVALID_ARG;
    *out_len = 0;
    if (status == ZKV_STATUS_BAD_CALLDATA) { *reverted = 1; return ZKV_OK; }      // the router could not decode the call: empty revert data
    if (call_kind >= RZW_KINDS) return ZKV_ERR_INVALID_ARG;                       // every other status belongs to a decoded call
    if (status == ZKV_STATUS_OK) {                                               // the Stylus shells return `true`, Solidity's verify nothing
        *reverted = 0;
        if (call_kind < 2) { host::abi_word_u32(out, 1); *out_len = 32; }
        return ZKV_OK;
    }
    *reverted = 1;
    const int k = zkv_risc0_router_status_abi_encode(c, status, recv_selector ? recv_selector : zero, out);
    if (k < 0) return k;
    *out_len = (uint32_t)k;
    return ZKV_OK;
}
// Calldata and its n + 1 offsets on the device.  The decode is enqueued in front of the count, so the call synchronises where run_router does.
// d_ck: the caller's call-kind row, or nullptr.
static int run_router_wire(zkv_ctx* c, size_t n, const uint8_t* d_cd, const uint64_t* d_off, uint64_t cd_bytes, uint8_t* d_status, uint8_t* d_recv,
                           uint8_t* d_ck, hipStream_t s) {
    int rc;
    RouterMem& rm = c->m_rz;
    if ((rc = grow_all(rm.w_seals, (size_t)ZKV_SEAL_BYTES * n + 8, rm.w_len, 4 * n, rm.h_a, 32 * n, rm.h_b, 32 * n, rm.h_method, n)) != ZKV_OK) return rc;
    if ((rc = order_after_previous(c, s)) != ZKV_OK) return rc;
    RzWireArgs w;
    memset(&w, 0, sizeof w);
    w.n = n; w.cd = d_cd; w.off = d_off; w.cd_bytes = cd_bytes;
    for (int k = 0; k < RZW_KINDS; k++) w.sel_be[k] = be32_of(router_call_selector(k));
    w.seals = rm.w_seals; w.seal_len = rm.w_len; w.in_a = rm.h_a; w.in_b = rm.h_b; w.method = rm.h_method;
    w.call_kind = d_ck;
    (void)hipEventRecord(c->ev_wire[0], s);
    launch_wire_rzrouter(w, s);
    (void)hipEventRecord(c->ev_wire[1], s);
    c->wire_timed = true;
    HIP_TRY(hipGetLastError());
    return run_router(c, n, w.seals, nullptr, 0, w.in_a, w.in_b, d_status, d_recv, s, w.method, w.seal_len);
}
ZKV_EXPORT int zkv_risc0_router_eth_call_batch_dev(zkv_ctx* c, size_t n, const uint8_t* d_calldata, const uint64_t* d_calldata_off, uint64_t calldata_bytes,
                                                   uint8_t* d_status, uint8_t* d_recv, uint8_t* d_call_kind, void* stream) {
    if (!c || c->vm != ZKV_VM_RISC0_ROUTER || c->rz_set) return ZKV_ERR_WRONG_CTX;
    if (n && (!d_calldata || !d_calldata_off || !d_status)) return ZKV_ERR_INVALID_ARG;
    if (!n) return ZKV_OK;
    if (n > 0xFFFFFFF0u / ZKV_SEAL_BYTES) return ZKV_ERR_INVALID_ARG;
    std::lock_guard<std::mutex> lk(c->mu);
    int rc = ctx_device_init(c);
    if (rc != ZKV_OK) return rc;
    return run_router_wire(c, n, d_calldata, d_calldata_off, calldata_bytes, d_status, d_recv, d_call_kind, stream ? (hipStream_t)stream : c->stream);
}
ZKV_EXPORT int zkv_risc0_router_eth_call_batch(zkv_ctx* c, size_t n, const uint8_t* blob, const uint64_t* off, uint8_t* reverted, uint8_t* returndata,
                                               uint32_t* returndata_len, uint8_t* status) {
    if (!c || c->vm != ZKV_VM_RISC0_ROUTER || c->rz_set) return ZKV_ERR_WRONG_CTX;
    if (n && (!blob || !off || !reverted || !returndata || !returndata_len)) return ZKV_ERR_INVALID_ARG;
    if (!n) return ZKV_OK;
    if (n > 0xFFFFFFF0u / ZKV_SEAL_BYTES || !offsets_ok(off, n)) return ZKV_ERR_INVALID_ARG;
    std::vector<uint8_t> st(n), rv(4 * n), ck(n);
    {
        std::lock_guard<std::mutex> lk(c->mu);
        int rc = ctx_device_init(c);
        if (rc != ZKV_OK) return rc;
        RouterMem& rm = c->m_rz;
        if ((rc = grow_all(rm.h_st, n, rm.h_rv, 4 * n, rm.w_ck, n)) != ZKV_OK) return rc;
        hipStream_t s = c->stream;
        if ((rc = order_after_previous(c, s)) != ZKV_OK) return rc;
        std::vector<uint64_t> rel;
        uint64_t bytes = 0;
        if ((rc = stage_ragged(rm.h_seals, rm.h_off, blob, off, n, &rel, s, &bytes)) != ZKV_OK) return rc;
        if ((rc = run_router_wire(c, n, rm.h_seals, rm.h_off, bytes, rm.h_st, rm.h_rv, rm.w_ck, s)) != ZKV_OK) return rc;
        HIP_TRY(hipMemcpyAsync(ck.data(), rm.w_ck, n, hipMemcpyDeviceToHost, s));
        if ((rc = return_to_host(rm.h_st, rm.h_rv, n, st.data(), rv.data(), s)) != ZKV_OK) return rc;
    }
    for (size_t i = 0; i < n; i++) {
        const int rc = zkv_risc0_router_eth_call_returndata(c, st[i], rv.data() + 4 * i, ck[i], returndata + i * ZKV_RETURNDATA_STRIDE, &returndata_len[i], &reverted[i]);
        if (rc != ZKV_OK) return rc;
        if (status) status[i] = st[i];
    }
    return ZKV_OK;
}
ZKV_EXPORT int zkv_risc0_router_last_call_counts(zkv_ctx* c, uint64_t* out) {
    if (!c || c->vm != ZKV_VM_RISC0_ROUTER || c->rz_set) return ZKV_ERR_WRONG_CTX;
    if (!out) return ZKV_ERR_INVALID_ARG;
    std::lock_guard<std::mutex> lk(c->mu);
    const size_t R = c->rz_counts.size();
    for (size_t r = 0; r < R; r++) out[r] = c->rz_counts[r];
    out[R] = c->rz_bad;
    return ZKV_OK;
}

// ------------------------------------------------------------------ precompile-level batches
ZKV_EXPORT zkv_ctx* zkv_bn254_ctx_create(int device) {
    zkv_ctx* c = new (std::nothrow) zkv_ctx();
    if (!c) return nullptr;
    c->vm = ZKV_VM_BN254; c->device = device; c->initialized = true;
    memset(&c->consts, 0, sizeof c->consts);
    return c;
}
// kind 0 = ecAdd (128 -> 64), 1 = ecMul (96 -> 64), 2 = ecPairing (k*192 -> result byte)
static int run_precompile(zkv_ctx* c, int kind, size_t n, size_t k, const uint8_t* in, uint8_t* out, uint8_t* ok) {
    if (!c || c->vm != ZKV_VM_BN254) return ZKV_ERR_WRONG_CTX;
    if (n && (!in || !out || !ok)) return ZKV_ERR_INVALID_ARG;
    if (!n) return ZKV_OK;
    std::lock_guard<std::mutex> lk(c->mu);
    const bool resident = kind == 2 && pairing_group((uint32_t)k) && n > dual_below();
    int rc = ctx_ready(c, resident ? n * k : n);
    if (rc != ZKV_OK) return rc;
    const size_t in_sz = kind == 0 ? 128 : kind == 1 ? 96 : 192 * k, out_sz = kind == 2 ? 1 : 64;
    // ecPairing calls of 2 .. 8 pairs keep all their pairs resident (one Miller loop per call, launch_pairing): k workspace slots per call
    const size_t cap = resident ? c->ws.cap / k : c->ws.cap;
    if ((rc = order_after_previous(c, c->stream)) != ZKV_OK) return rc;
    for (size_t base = 0; base < n; base += cap) {
        size_t m = n - base < cap ? n - base : cap;
        if ((rc = c->d_blob.grow(m * in_sz + 8)) != ZKV_OK) return rc;
        if ((rc = c->d_pv.grow(m * out_sz + 8)) != ZKV_OK) return rc;
        if (in_sz) HIP_TRY(hipMemcpyAsync(c->d_blob, in + base * in_sz, m * in_sz, hipMemcpyHostToDevice, c->stream));
        if (kind == 0) launch_ecadd(m, c->d_blob, c->d_pv, c->d_status, c->stream);
        else if (kind == 1) launch_ecmul(m, c->d_blob, c->d_pv, c->d_status, c->stream);
        else if (m <= dual_below()) launch_pairing_w(m, (uint32_t)k, c->d_blob, c->ws, c->d_pv, c->d_status, c->stream);      // few calls: latency
        else launch_pairing(m, (uint32_t)k, c->d_blob, c->ws, c->d_pv, c->d_status, c->stream);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipMemcpyAsync(out + base * out_sz, c->d_pv, m * out_sz, hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(hipMemcpyAsync(ok + base, c->d_status, m, hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(hipStreamSynchronize(c->stream));
    }
    return ZKV_OK;
}
ZKV_EXPORT int zkv_bn254_ecadd_batch(zkv_ctx* c, size_t n, const uint8_t* in, uint8_t* out, uint8_t* ok) { return run_precompile(c, 0, n, 0, in, out, ok); }
ZKV_EXPORT int zkv_bn254_ecmul_batch(zkv_ctx* c, size_t n, const uint8_t* in, uint8_t* out, uint8_t* ok) { return run_precompile(c, 1, n, 0, in, out, ok); }
// The ecPairing seam with calldata, results and verdicts resident in HBM: enqueued on the caller's stream (or the context's), no copy,
// no synchronisation.
ZKV_EXPORT int zkv_bn254_pairing_batch_dev(zkv_ctx* c, size_t n, size_t k, const uint8_t* d_in, uint8_t* d_result, uint8_t* d_ok, void* stream) {
    if (!c || c->vm != ZKV_VM_BN254) return ZKV_ERR_WRONG_CTX;
    if (k > 64 || (n && (!d_result || !d_ok || (k && !d_in)))) return ZKV_ERR_INVALID_ARG;
    if (!n) return ZKV_OK;
    std::lock_guard<std::mutex> lk(c->mu);
    const bool resident = pairing_group((uint32_t)k) && n > dual_below();
    int rc = ctx_ready(c, resident ? n * k : n);
    if (rc != ZKV_OK) return rc;
    hipStream_t s = stream ? (hipStream_t)stream : c->stream;
    if ((rc = order_after_previous(c, s)) != ZKV_OK) return rc;
    const size_t cap = resident ? c->ws.cap / k : c->ws.cap;
    for (size_t base = 0; base < n; base += cap) {
        const size_t m = n - base < cap ? n - base : cap;
        const uint8_t* in = k ? d_in + base * 192 * k : d_in;
        if (m <= dual_below()) launch_pairing_w(m, (uint32_t)k, in, c->ws, d_result + base, d_ok + base, s);
        else launch_pairing(m, (uint32_t)k, in, c->ws, d_result + base, d_ok + base, s);
        HIP_TRY(hipGetLastError());
    }
    return mark_done(c, s);
}
ZKV_EXPORT int zkv_bn254_pairing_batch(zkv_ctx* c, size_t n, size_t k, const uint8_t* in, uint8_t* result, uint8_t* ok) {
    if (k > 64) return ZKV_ERR_INVALID_ARG;
    uint8_t dummy = 0;
    return run_precompile(c, 2, n, k, k ? in : &dummy, result, ok);
}

// ------------------------------------------------------------------ Groth16 core, arbitrary verification key
// Long keys stage the signals of a chunk (32 bytes per signal and proof) next to the workspace: the chunk is capped so that they stay within
// LONG_STAGE_BYTES (2^17 proofs at 128 signals).
constexpr size_t LONG_STAGE_BYTES = (size_t)512 << 20;
static size_t long_chunk(const zkv_ctx* c) {
    const size_t per = 32 * (size_t)(c->g_n_ic - 1), cap = chunk_capacity();
    size_t lim = 64;
    while (lim < cap && 2 * lim * per <= LONG_STAGE_BYTES) lim *= 2;
    return lim < cap ? lim : cap;
}
// device set-up and buffers for a generic-key batch of n proofs; returns the proofs per chunk through *chunk
static int groth16_ready(zkv_ctx* c, size_t n, size_t* chunk) {
    if (!c->long_key) {
        const int rc = ctx_ready(c, n);
        *chunk = c->ws.cap;
        return rc;
    }
    const size_t lc = long_chunk(c);
    int rc = ctx_ready(c, n < lc ? n : lc);
    if (rc != ZKV_OK) return rc;
    const size_t need = c->ws.cap < lc ? c->ws.cap : lc;
    if (lsig_stride(c) < need && (rc = c->d_lsig.alloc((size_t)32 * (c->g_n_ic - 1) * need)) != ZKV_OK) return rc;
    *chunk = need;
    return ZKV_OK;
}
ZKV_EXPORT zkv_ctx* zkv_groth16_ctx_create(const uint8_t* vk_words, size_t n_ic, int vm_type, int device) {
    if (!vk_words || n_ic < 1 || n_ic > ZKV_GROTH16_MAX_IC || (vm_type != ZKV_VM_RISC0 && vm_type != ZKV_VM_SP1)) return nullptr;
    zkv_ctx* c = new (std::nothrow) zkv_ctx();
    if (!c) return nullptr;
    c->vm = ZKV_VM_GROTH16; c->device = device; c->initialized = true;
    memset(&c->consts, 0, sizeof c->consts);
    try { c->gvk.assign(vk_words, vk_words + 448 + 64 * n_ic); } catch (const std::bad_alloc&) { delete c; return nullptr; }
    c->g_n_ic = (uint32_t)n_ic; c->g_negate = vm_type == ZKV_VM_RISC0;
    const char* e = getenv("ZKV_LONG_KEY");                  // A/B knob: keys with n_ic <= MAX_IC through the long-key path as well
    c->long_key = n_ic > (size_t)MAX_IC || (n_ic >= 2 && e && atoi(e) == 1);
    return c;
}
ZKV_EXPORT int zkv_groth16_verify_batch(zkv_ctx* c, size_t n, const uint8_t* proofs, const uint8_t* signals, uint8_t* verified) {
    if (!c || c->vm != ZKV_VM_GROTH16) return ZKV_ERR_WRONG_CTX;
    const uint32_t n_sig = c->g_n_ic - 1;
    if (n && (!proofs || !verified || (n_sig && !signals))) return ZKV_ERR_INVALID_ARG;
    if (!n) return ZKV_OK;
    if (is_sharded(c))
        return run_sharded(c, n, [&](zkv_ctx* k, size_t lo, size_t hi) {
            return zkv_groth16_verify_batch(k, hi - lo, proofs + 256 * lo, n_sig ? signals + (size_t)32 * n_sig * lo : signals, verified + lo); });
    std::lock_guard<std::mutex> lk(c->mu);
    size_t cap = 0;
    int rc = groth16_ready(c, n, &cap);
    if (rc != ZKV_OK) return rc;
    if ((rc = order_after_previous(c, c->stream)) != ZKV_OK) return rc;
    for (size_t base = 0; base < n; base += cap) {
        size_t m = n - base < cap ? n - base : cap;
        if ((rc = c->d_blob.grow(m * 256 + 8)) != ZKV_OK) return rc;
        if ((rc = c->d_pv.grow(m * 32 * n_sig + 8)) != ZKV_OK) return rc;
        HIP_TRY(hipMemcpyAsync(c->d_blob, proofs + 256 * base, 256 * m, hipMemcpyHostToDevice, c->stream));
        if (n_sig) HIP_TRY(hipMemcpyAsync(c->d_pv, signals + (size_t)32 * n_sig * base, (size_t)32 * n_sig * m, hipMemcpyHostToDevice, c->stream));
        PrepArgs a;
        memset(&a, 0, sizeof a);
        a.n = m; a.blob = c->d_blob; a.in32_a = c->d_pv; a.n_sig = n_sig; a.negate_a = c->g_negate ? 1u : 0u;
        a.force_fail = c->vk_invalid ? 1u : 0u;
        a.status = c->d_status; a.recv = nullptr;
        enqueue_chunk(c, a, c->stream, true);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipMemcpyAsync(verified + base, c->d_status, m, hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(hipStreamSynchronize(c->stream));
        for (size_t i = 0; i < m; i++) verified[base + i] = verified[base + i] == ZKV_STATUS_OK ? 1 : 0;
    }
    return ZKV_OK;
}
ZKV_EXPORT int zkv_groth16_verify_batch_dev(zkv_ctx* c, size_t n, const uint8_t* d_proofs, const uint8_t* d_signals, uint8_t* d_verified, void* stream) {
    if (!c || c->vm != ZKV_VM_GROTH16) return ZKV_ERR_WRONG_CTX;
    const uint32_t n_sig = c->g_n_ic - 1;
    if (n && (!d_proofs || !d_verified || (n_sig && !d_signals))) return ZKV_ERR_INVALID_ARG;
    if (!n) return ZKV_OK;
    if (is_sharded(c)) {
        const DevRow rows[2] = {{d_proofs, 256}, {d_signals, (size_t)32 * n_sig}};
        return run_sharded_dev(c, n, rows, n_sig ? 2 : 1, d_verified, nullptr, stream, [&](zkv_ctx* k, size_t m, const uint8_t* const* r, uint8_t* st, uint8_t*, hipStream_t s) {
            return zkv_groth16_verify_batch_dev(k, m, r[0], n_sig ? r[1] : nullptr, st, s); });
    }
    std::lock_guard<std::mutex> lk(c->mu);
    size_t cap = 0;
    int rc = groth16_ready(c, n, &cap);
    if (rc != ZKV_OK) return rc;
    hipStream_t s = stream ? (hipStream_t)stream : c->stream;
    if ((rc = order_after_previous(c, s)) != ZKV_OK) return rc;
    for (size_t base = 0; base < n; base += cap) {
        const size_t m = n - base < cap ? n - base : cap;
        PrepArgs a;
        memset(&a, 0, sizeof a);
        a.n = m; a.blob = d_proofs + 256 * base; a.in32_a = n_sig ? d_signals + (size_t)32 * n_sig * base : nullptr;
        a.n_sig = n_sig; a.negate_a = c->g_negate ? 1u : 0u; a.force_fail = c->vk_invalid ? 1u : 0u;
        a.status = d_verified + base; a.recv = nullptr;
        enqueue_chunk(c, a, s, base + cap >= n);
        launch_status_to_bool(m, d_verified + base, s);
    }
    HIP_TRY(hipGetLastError());
    return mark_done(c, s);
}

// ------------------------------------------------------------------ PLONK core, any key (zkv_plonk_keys.h)
// No reference counterpart: parity unpinned.  The SP1 PLONK context's device path with the public inputs read from a per-proof row.
static size_t plonk_proof_bytes(const zkv_ctx* c) { return (size_t)32 * (24 + 3 * c->pk_raw.n_c); }
// Host batches stage the public inputs of a chunk (32 nb_public bytes per proof) next to the proofs: at most LONG_STAGE_BYTES per chunk.
static size_t plonk_host_chunk(const zkv_ctx* c) {
    const size_t per = 32 * (size_t)c->pk_raw.nb_public, cap = chunk_capacity();
    if (!per) return cap;
    size_t lim = 64;
    while (lim < cap && 2 * lim * per <= LONG_STAGE_BYTES) lim *= 2;
    return lim < cap ? lim : cap;
}
// device set-up and buffers for a batch of n proofs; the proofs per chunk of a host batch through *chunk
static int plonk_ready(zkv_ctx* c, size_t n, size_t* chunk) {
    const size_t hc = plonk_host_chunk(c);
    const int rc = ctx_ready(c, n < hc ? n : hc);
    *chunk = c->ws.cap < hc ? c->ws.cap : hc;
    return rc;
}
// A key in zkv_plonk_keys.h's layout: false on its rules (length, n_c > 1, nb_public > MAX, oversized header words)
static bool plonk_parse_key(const uint8_t* vk, size_t vk_len, PlonkKeyRaw& raw, uint8_t g2[256]) {
    if (!vk || vk_len < 7 * 32) return false;
    uint32_t w[7][8];
    for (int k = 0; k < 7; k++) host::be_to_limbs(w[k], vk + 32 * k);
    auto below = [](const uint32_t* x, int limbs) { for (int i = limbs; i < 8; i++) if (x[i]) return false; return true; };
    // size < 2^64; nb_public, n_c and cci one limb each (the SP1 parser reads limb 0 alone; this one checks the others)
    if (!below(w[0], 2) || !below(w[4], 1) || !below(w[5], 1) || !below(w[6], 1)) return false;
    if (w[5][0] > 1 || w[4][0] > ZKV_PLONK_MAX_PUBLIC) return false;
    const size_t n_c = w[5][0];
    if (vk_len != 7 * 32 + (8 + n_c) * 64 + 256) return false;
    memset(&raw, 0, sizeof raw);
    memcpy(raw.size, w[0], 32); memcpy(raw.size_inv, w[1], 32); memcpy(raw.gen, w[2], 32); memcpy(raw.coset, w[3], 32);
    raw.nb_public = w[4][0]; raw.n_c = w[5][0]; raw.cci = w[6][0];
    for (size_t p = 0; p < 8 + n_c; p++) {
        host::be_to_limbs(raw.pts[p][0], vk + 224 + 64 * p); host::be_to_limbs(raw.pts[p][1], vk + 256 + 64 * p);
    }
    memcpy(g2, vk + 224 + 64 * (8 + n_c), 256);
    return true;
}
ZKV_EXPORT zkv_ctx* zkv_plonk_ctx_create(const uint8_t* vk, size_t vk_len, int device) {
    PlonkKeyRaw raw;
    uint8_t g2[256];
    if (!plonk_parse_key(vk, vk_len, raw, g2)) return nullptr;
    zkv_ctx* c = new (std::nothrow) zkv_ctx();
    if (!c) return nullptr;
    c->vm = ZKV_VM_PLONK; c->device = device; c->initialized = true;
    memset(&c->consts, 0, sizeof c->consts);
    c->pk_raw = raw;
    memcpy(c->pk_g2, g2, 256);
    return c;
}
ZKV_EXPORT int zkv_plonk_key_shape(const zkv_ctx* c, size_t* nb_public, size_t* n_commitments, size_t* proof_bytes) {
    if (!c || c->vm != ZKV_VM_PLONK) return ZKV_ERR_WRONG_CTX;
    if (nb_public) *nb_public = c->pk_raw.nb_public;
    if (n_commitments) *n_commitments = c->pk_raw.n_c;
    if (proof_bytes) *proof_bytes = plonk_proof_bytes(c);
    return ZKV_OK;
}
static PrepArgs plonk_args(const zkv_ctx* c, size_t m, const uint8_t* proofs, const uint8_t* pub, uint8_t* status) {
    PrepArgs a;
    memset(&a, 0, sizeof a);
    a.n = m; a.blob = proofs; a.stride = (uint32_t)plonk_proof_bytes(c);
    a.in32_a = pub; a.n_sig = c->pk_raw.nb_public;
    a.force_fail = c->vk_invalid ? 1u : 0u;
    a.status = status; a.recv = nullptr;
    return a;
}
ZKV_EXPORT int zkv_plonk_verify_batch(zkv_ctx* c, size_t n, const uint8_t* proofs, const uint8_t* public_inputs, uint8_t* verified) {
    if (!c || c->vm != ZKV_VM_PLONK) return ZKV_ERR_WRONG_CTX;
    const size_t pb = plonk_proof_bytes(c), pin = (size_t)32 * c->pk_raw.nb_public;
    if (n && (!proofs || !verified || (pin && !public_inputs))) return ZKV_ERR_INVALID_ARG;
    if (!n) return ZKV_OK;
    if (is_sharded(c))
        return run_sharded(c, n, [&](zkv_ctx* k, size_t lo, size_t hi) {
            return zkv_plonk_verify_batch(k, hi - lo, proofs + pb * lo, pin ? public_inputs + pin * lo : public_inputs, verified + lo); });
    std::lock_guard<std::mutex> lk(c->mu);
    size_t cap = 0;
    int rc = plonk_ready(c, n, &cap);
    if (rc != ZKV_OK) return rc;
    if ((rc = order_after_previous(c, c->stream)) != ZKV_OK) return rc;
    for (size_t base = 0; base < n; base += cap) {
        const size_t m = n - base < cap ? n - base : cap;
        if ((rc = c->d_blob.grow(m * pb + 8)) != ZKV_OK) return rc;
        if ((rc = c->d_pv.grow(m * pin + 8)) != ZKV_OK) return rc;
        HIP_TRY(hipMemcpyAsync(c->d_blob, proofs + pb * base, pb * m, hipMemcpyHostToDevice, c->stream));
        if (pin) HIP_TRY(hipMemcpyAsync(c->d_pv, public_inputs + pin * base, pin * m, hipMemcpyHostToDevice, c->stream));
        const PrepArgs a = plonk_args(c, m, c->d_blob, c->d_pv, c->d_status);
        enqueue_chunk(c, a, c->stream, true);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipMemcpyAsync(verified + base, c->d_status, m, hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(hipStreamSynchronize(c->stream));
        for (size_t i = 0; i < m; i++) verified[base + i] = verified[base + i] == ZKV_STATUS_OK ? 1 : 0;
    }
    return mark_done(c, c->stream);
}
ZKV_EXPORT int zkv_plonk_verify_batch_dev(zkv_ctx* c, size_t n, const uint8_t* d_proofs, const uint8_t* d_public_inputs, uint8_t* d_verified, void* stream) {
    if (!c || c->vm != ZKV_VM_PLONK) return ZKV_ERR_WRONG_CTX;
    const size_t pb = plonk_proof_bytes(c), pin = (size_t)32 * c->pk_raw.nb_public;
    if (n && (!d_proofs || !d_verified || (pin && !d_public_inputs))) return ZKV_ERR_INVALID_ARG;
    if (!n) return ZKV_OK;
    if (is_sharded(c)) {
        const DevRow rows[2] = {{d_proofs, pb}, {d_public_inputs, pin}};
        return run_sharded_dev(c, n, rows, pin ? 2 : 1, d_verified, nullptr, stream, [&](zkv_ctx* k, size_t m, const uint8_t* const* r, uint8_t* st, uint8_t*, hipStream_t s) {
            return zkv_plonk_verify_batch_dev(k, m, r[0], pin ? r[1] : nullptr, st, s); });
    }
    std::lock_guard<std::mutex> lk(c->mu);
    int rc = ctx_ready(c, n);
    if (rc != ZKV_OK) return rc;
    const size_t cap = c->ws.cap;
    hipStream_t s = stream ? (hipStream_t)stream : c->stream;
    if ((rc = order_after_previous(c, s)) != ZKV_OK) return rc;
    for (size_t base = 0; base < n; base += cap) {
        const size_t m = n - base < cap ? n - base : cap;
        const PrepArgs a = plonk_args(c, m, d_proofs + pb * base, pin ? d_public_inputs + pin * base : nullptr, d_verified + base);
        enqueue_chunk(c, a, s, base + cap >= n);
        launch_status_to_bool(m, d_verified + base, s);
    }
    HIP_TRY(hipGetLastError());
    return mark_done(c, s);
}

// ------------------------------------------------------------------ Groth16 key sets (zkv_groth16_set.h)
// Set-up of every key in six launches whatever the number of keys (k_gset.hip): VkTables per key (alpha, beta, gamma, delta and IC[0]:
// 3.6 MB, most of it the unused short-key rows of the struct) and 512 KB of window rows per signal.
static int gset_device_setup(zkv_ctx* c) {
    const uint32_t K = (uint32_t)c->gs_nic.size();
    std::vector<VkRaw> raw(K);
    std::vector<GsetKey> keys(K);
    std::vector<uint32_t> ic, sig_key;
    uint32_t S = 0;
    for (uint32_t k = 0; k < K; k++) {
        const uint8_t* w = c->gvk.data() + c->gs_off[k];
        host::fill_vk_generic(raw[k], w, 1u);                 // IC[0] only: IC[1..] take the window rows
        const uint32_t n_sig = c->gs_nic[k] - 1;
        keys[k] = GsetKey{nullptr, S, n_sig, c->gs_neg[k] ? 1u : 0u, 0u};
        for (uint32_t b = 0; b < n_sig; b++) {
            ic.resize(ic.size() + 16);
            host::be_to_limbs(&ic[ic.size() - 16], w + 448 + 64 * (size_t)(b + 1));
            host::be_to_limbs(&ic[ic.size() - 8], w + 480 + 64 * (size_t)(b + 1));
            sig_key.push_back(k);
        }
        S += n_sig;
    }
    HIP_TRY(c->d_gs_tab.alloc(sizeof(VkTables) * K));
    HIP_TRY(hipMemsetAsync(c->d_gs_tab, 0, sizeof(VkTables) * K, c->stream));
    for (uint32_t k = 0; k < K; k++) keys[k].tab = c->d_gs_tab + k;
    HIP_TRY(c->d_gs_key.alloc(sizeof(GsetKey) * K));
    HIP_TRY(hipMemcpyAsync(c->d_gs_key, keys.data(), sizeof(GsetKey) * K, hipMemcpyHostToDevice, c->stream));
    // the raw keys and points are only read by the set-up kernels: scoped, released after the synchronisation below
    DevBuf<VkRaw> d_raw;
    DevBuf<uint32_t> d_ic, d_sig_key;
    HIP_TRY(d_raw.alloc(sizeof(VkRaw) * K));
    HIP_TRY(hipMemcpyAsync(d_raw, raw.data(), sizeof(VkRaw) * K, hipMemcpyHostToDevice, c->stream));
    if (S) {
        const size_t tab_bytes = (size_t)S * LONG_ROW_ENTRIES * sizeof(G1A);
        HIP_TRY(c->d_gs_rows.alloc(tab_bytes));
        HIP_TRY(c->d_gs_win.alloc(sizeof(uint32_t) * S));
        HIP_TRY(hipMemsetAsync(c->d_gs_rows, 0, tab_bytes, c->stream));
        HIP_TRY(d_ic.alloc(sizeof(uint32_t) * ic.size()));
        HIP_TRY(d_sig_key.alloc(sizeof(uint32_t) * S));
        HIP_TRY(hipMemcpyAsync(d_ic, ic.data(), sizeof(uint32_t) * ic.size(), hipMemcpyHostToDevice, c->stream));
        HIP_TRY(hipMemcpyAsync(d_sig_key, sig_key.data(), sizeof(uint32_t) * S, hipMemcpyHostToDevice, c->stream));
    }
    launch_gset_setup(K, d_raw, c->d_gs_tab, S, d_ic, d_sig_key, c->d_gs_rows, c->d_gs_win, c->stream);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(c->stream));                // the host vectors above go out of scope
    return ZKV_OK;
}
ZKV_EXPORT zkv_ctx* zkv_groth16_set_create(size_t n_keys, const uint8_t* const* vk_words, const size_t* n_ic, const int* vm_type, int device) {
    if (n_keys < 1 || n_keys > ZKV_GROTH16_SET_MAX_KEYS || !vk_words || !n_ic || !vm_type) return nullptr;
    size_t bytes = 0, max_ic = 1;
    for (size_t k = 0; k < n_keys; k++) {
        if (!vk_words[k] || n_ic[k] < 1 || n_ic[k] > ZKV_GROTH16_MAX_IC || (vm_type[k] != ZKV_VM_RISC0 && vm_type[k] != ZKV_VM_SP1)) return nullptr;
        bytes += 448 + 64 * n_ic[k];
        if (n_ic[k] > max_ic) max_ic = n_ic[k];
    }
    zkv_ctx* c = new (std::nothrow) zkv_ctx();
    if (!c) return nullptr;
    c->vm = ZKV_VM_GROTH16_SET; c->device = device; c->initialized = true;
    memset(&c->consts, 0, sizeof c->consts);
    try {
        c->gvk.reserve(bytes);
        for (size_t k = 0; k < n_keys; k++) {
            c->gs_off.push_back(c->gvk.size());
            c->gvk.insert(c->gvk.end(), vk_words[k], vk_words[k] + 448 + 64 * n_ic[k]);
            c->gs_nic.push_back((uint32_t)n_ic[k]);
            c->gs_neg.push_back(vm_type[k] == ZKV_VM_RISC0 ? 1 : 0);
        }
    } catch (const std::bad_alloc&) { delete c; return nullptr; }
    c->g_n_ic = (uint32_t)max_ic; c->long_key = true;
    return c;
}
ZKV_EXPORT size_t zkv_groth16_set_size(const zkv_ctx* c) { return c && c->vm == ZKV_VM_GROTH16_SET ? c->gs_nic.size() : 0; }
ZKV_EXPORT size_t zkv_groth16_set_signal_stride(const zkv_ctx* c) { return c && c->vm == ZKV_VM_GROTH16_SET ? (size_t)32 * (c->g_n_ic - 1) : 0; }
ZKV_EXPORT int zkv_groth16_set_key_n_ic(const zkv_ctx* c, size_t key) {
    if (!c || c->vm != ZKV_VM_GROTH16_SET) return ZKV_ERR_WRONG_CTX;
    return key < c->gs_nic.size() ? (int)c->gs_nic[key] : ZKV_ERR_INVALID_ARG;
}
// Aggregate check on a set: every key's AggTables (k_setup_agg's contents, 0.53 MB per key) in d_agg_tab and which keys can take the check,
// built the first time a call wants the check -- not at set creation, so a set that never uses it does not grow -- and the counters.
// false: no key can, or no room (the call then runs the per-proof path).
static bool gset_agg_tables(zkv_ctx* c) {
    if (c->d_agg_tab) return c->agg_key_ok;
    const uint32_t K = (uint32_t)c->gs_nic.size();
    std::vector<VkRaw> raw(K);
    for (uint32_t k = 0; k < K; k++) host::fill_vk_generic(raw[k], c->gvk.data() + c->gs_off[k], 1u);
    DevBuf<VkRaw> d_raw;
    if (c->d_agg_tab.alloc(sizeof(AggTables) * K) || d_raw.alloc(sizeof(VkRaw) * K) ||
        (!c->d_agg_cnt && (c->d_agg_cnt.alloc(3 * sizeof(unsigned long long)) ||
                           hipMemset(c->d_agg_cnt, 0, 3 * sizeof(unsigned long long)) != hipSuccess))) {
        (void)hipGetLastError();
        c->d_agg_tab.release();
        return false;
    }
    std::vector<uint32_t> ok(K);
    bool good = hipMemcpyAsync(d_raw, raw.data(), sizeof(VkRaw) * K, hipMemcpyHostToDevice, c->stream) == hipSuccess;
    if (good) {
        launch_gset_setup_agg(K, d_raw, c->d_gs_tab, c->d_agg_tab, c->stream);
        good = hipGetLastError() == hipSuccess;
        for (uint32_t k = 0; k < K && good; k++)
            good = hipMemcpyAsync(&ok[k], &c->d_agg_tab[k].ok, sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream) == hipSuccess;
        good = good && hipStreamSynchronize(c->stream) == hipSuccess;
    }
    if (!good) { (void)hipGetLastError(); c->d_agg_tab.release(); return false; }
    c->gs_agg_ok.assign(K, 0);
    c->agg_key_ok = false;
    for (uint32_t k = 0; k < K; k++) { c->gs_agg_ok[k] = ok[k] ? 1 : 0; c->agg_key_ok = c->agg_key_ok || ok[k]; }
    return c->agg_key_ok;
}
// ---- The steps of a call that both kinds of key set take (run_gset, run_pset: each keeps its own layout choice, placement and stages).
// Partition: the proofs counted per key, block by block; the per-key totals come back to the host (gs_totals: the call's one
// synchronisation) and *placed is their sum.  The buffers: KeySetMem.
static int set_partition(zkv_ctx* c, size_t n, uint32_t K, const uint32_t* d_key, hipStream_t s, GsetPart* p, size_t* placed) {
    memset(p, 0, sizeof *p);
    p->n = n; p->n_keys = K;
    size_t per = (n + 255) / 256;                            // at most 256 partition blocks of a multiple of 64 proofs
    per = (per + 63) / 64 * 64;
    p->per_block = (uint32_t)per; p->blocks = (uint32_t)((n + per - 1) / per);
    const size_t kb = (size_t)K * p->blocks;
    KeySetMem& ks = c->m_ks;
    const int rc = grow_all(ks.cnt, 4 * kb, ks.totals, 4 * (size_t)K, ks.off, 4 * kb, ks.pos, 4 * n, ks.start, 8 * ((size_t)K + 1));
    if (rc != ZKV_OK) return rc;
    p->key = d_key; p->cnt = ks.cnt; p->totals = ks.totals; p->off = ks.off; p->pos = ks.pos;
    HIP_TRY(hipMemsetAsync(p->totals, 0, 4 * (size_t)K, s));
    launch_gset_count(*p, s);
    HIP_TRY(hipGetLastError());
    c->gs_totals.resize(K); c->gs_start.resize((size_t)K + 1);
    HIP_TRY(hipMemcpyAsync(c->gs_totals.data(), p->totals, 4 * (size_t)K, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    *placed = 0;
    for (uint32_t k = 0; k < K; k++) *placed += c->gs_totals[k];
    return ZKV_OK;
}
// Slot buffers of a layout of M slots: the proof of every slot, its key and its status byte.
static int set_slot_buffers(zkv_ctx* c, size_t M, GsetPart* p, hipStream_t s) {
    const int rc = grow_all(c->m_ks.idx, 4 * M + 4, c->m_ks.skey, 4 * M + 4, c->d_st_all, M + 1);
    if (rc != ZKV_OK) return rc;
    p->idx = c->m_ks.idx; p->skey = c->m_ks.skey;
    HIP_TRY(hipMemsetAsync(p->idx, 0xFF, 4 * M + 4, s));     // pad slots: GSET_NONE
    HIP_TRY(hipMemsetAsync(p->skey, 0, 4 * M + 4, s));       // (and key 0: a slot's key is only read for live slots, this keeps any read in the set)
    return ZKV_OK;
}
// The aggregate chunks of the aggregate region [0, R), `capa` slots each, and their pseudo-proof maps (zkv_gset_layout.h
// gset_agg_chunk_plan, whose regions the caller passes on): chunk g's map is in gs_amap from word g.off -- psl (sub-batch -> pseudo slot, n2
// words), then the key of every pseudo slot (slots words) -- and all of gs_amap goes to m_ks.amap in one copy.
// (GsetAggChunk: declared with run_keyed_group, which plans the keyed group of a router the same way)
static int set_agg_plan(zkv_ctx* c, const uint64_t* beg, const uint64_t* end, const uint32_t* rep, uint32_t n_regions, uint64_t R, size_t capa,
                        uint32_t sub, std::vector<GsetAggChunk>* plan, hipStream_t s) {
    c->gs_amap.clear();
    c->gs_nsb.assign(n_regions, 0); c->gs_pst.resize((size_t)n_regions + 1);
    for (size_t base = 0; base < R; base += capa) {
        const size_t m = R - base < capa ? (size_t)R - base : capa;
        GsetAggChunk g{base, m, m / sub, c->gs_amap.size(), 0, 0};
        c->gs_amap.resize(g.off + 2 * g.n2 + 31 * (size_t)n_regions, 0);      // (the most the padding can take; cut to the slots below)
        uint32_t* psl = c->gs_amap.data() + g.off;
        g.lanes = gset_agg_chunk_plan(beg, end, rep, n_regions, base, m, sub, miller_lanes(c, g.n2), c->ws2.cap, c->gs_nsb.data(), c->gs_pst.data(),
                                      psl, psl + g.n2, &g.slots);
        c->gs_amap.resize(g.off + g.n2 + g.slots);
        plan->push_back(g);
    }
    const int rc = c->m_ks.amap.grow(4 * c->gs_amap.size() + 4);
    if (rc != ZKV_OK) return rc;
    HIP_TRY(hipMemcpyAsync(c->m_ks.amap, c->gs_amap.data(), 4 * c->gs_amap.size(), hipMemcpyHostToDevice, s));
    return ZKV_OK;
}
// The verdicts back to the caller's order (a call that placed no proof still records the six stage events).
static int set_return(zkv_ctx* c, size_t n, size_t M, const GsetPart& p, uint8_t* d_verified, hipStream_t s) {
    if (!M) for (int e = 0; e < 6; e++) (void)hipEventRecord(c->ev[e], s);
    launch_gset_return(n, p.pos, c->d_st_all, d_verified, s);
    HIP_TRY(hipGetLastError());
    return ZKV_OK;
}
// Slots [base, base + m) of a Groth16 set's layout as one chunk
static GsetChunk gset_chunk_of(const zkv_ctx* c, const GsetPart& p, const uint8_t* d_proofs, const uint8_t* d_signals, size_t base, size_t m) {
    GsetChunk ch;
    memset(&ch, 0, sizeof ch);
    ch.m = m; ch.slot0 = base; ch.idx = p.idx; ch.skey = p.skey;
    ch.keys = c->d_gs_key; ch.rows = c->d_gs_rows; ch.win = c->d_gs_win;
    ch.proofs = d_proofs; ch.signals = d_signals; ch.sig_stride = 32 * (c->g_n_ic - 1);
    ch.sig = c->d_lsig; ch.sig_cap = lsig_stride(c); ch.status = c->d_st_all + base;
    return ch;
}
// The aggregate check of one chunk of a set's aggregate region (zkv_agg.h; k_gset_agg.hip): PREP (`prep` launches it: the set's own
// k_gset_prep, or the PREP kernel of a router's keyed group, as in gset_proof_stages), the coefficients and r A', r C, the
// Miller loop of the variable pair, one pseudo-proof per sub-batch with its key's gamma / delta lines and ML(alpha, beta), the product of the
// proofs' Miller values into it, its final exponentiation, the verdicts, and the per-proof kernels once more over the proofs of the
// sub-batches that failed (in place: k_gset_agg_mark).
template <class Prep>
static void enqueue_gset_agg(zkv_ctx* c, const GsetChunk& ch, const GsetAggChunk& g, const uint32_t* skey, const uint32_t* d_amap, uint32_t sub,
                             hipStream_t s, bool timed, Prep prep) {
    const size_t m = ch.m;
    const uint32_t sub64 = sub < 64 ? sub : 64, grp = agg_group(sub64);
    const uint32_t* psl = d_amap + g.off;
    const uint32_t* skey2 = psl + g.n2;
    if (timed) (void)hipEventRecord(c->ev[0], s);
    prep();
    if (timed) (void)hipEventRecord(c->ev[1], s);
    agg_next_coefficients(c);
    launch_agg_g1(m, c->d_gs_tab, nullptr, c->ws, c->d_agg, c->agg_seed, true, s);      // (reads no key: the set's tables have n_var = 0)
    if (timed) { (void)hipEventRecord(c->ev[2], s); (void)hipEventRecord(c->ev[3], s); }
    if (grp > 1) launch_gset_agg_miller(m, grp, skey, c->d_gs_key, c->ws, ch.status, s);
    else launch_gset_miller(2, m, skey, c->d_gs_key, c->ws, ch.status, s);
    (void)hipMemsetAsync(c->ws2.flags, 0, sizeof(uint32_t) * g.slots, s);     // pad slots of the pseudo-proofs: no proof
    launch_gset_agg_reduce(ch, sub64, grp, c->ws, c->d_agg, c->d_agg_tab, c->ws2, c->d_status2, psl, sub > 64, s);
    if (sub > 64) launch_gset_agg_combine(ch, g.n2, sub / 64, c->d_agg_tab, c->ws2, c->d_status2, psl, s);
    launch_gset_miller(g.lanes, (size_t)g.slots, skey2, c->d_gs_key, c->ws2, c->d_status2, s);
    if (timed) (void)hipEventRecord(c->ev[4], s);
    launch_gset_agg_fprod(m, g.n2, sub, grp, c->ws, c->d_agg, c->ws2, psl, s);
    launch_finalexp_lanes(g.lanes, (size_t)g.slots, c->ws2, c->d_status2, s);
    launch_gset_agg_mark(m, sub, grp, c->ws, c->d_agg, c->d_status2, psl, ch.status, c->d_agg_cnt, s);
    launch_gset_msm(ch, msm_lanes_long(c, m), c->ws, s);
    launch_gset_miller(2, m, skey, c->d_gs_key, c->ws, ch.status, s);       // (lane pairs: the subgroup test of B included)
    launch_finalexp2(m, c->ws, ch.status, s);
    if (timed) (void)hipEventRecord(c->ev[5], s);
}
// One call of n proofs, every buffer on the device, enqueued on s (c->mu held, device set up).  Partition (count per block; the per-key
// totals come back to the host, which lays the groups out; place), then the stages chunk by chunk over the slots, then the verdicts back
// to the caller's order.  Chunks of a set take no tail split (tail_of_chunk): every slot of a chunk runs the one mapping of the call.
static int run_gset(zkv_ctx* c, size_t n, const uint32_t* d_key, const uint8_t* d_proofs, const uint8_t* d_signals, uint8_t* d_verified, hipStream_t s) {
    const uint32_t K = (uint32_t)c->gs_nic.size();
    GsetPart p;
    size_t placed = 0;
    int rc;
    if ((rc = set_partition(c, n, K, d_key, s, &p, &placed)) != ZKV_OK) return rc;
    // The aggregate check (a fixed mapping, a small call or no capable key: none): the aggregate region [0, R) and the per-proof region
    // (zkv_gset_layout.h gset_agg_choose); R = 0 falls back to the one-region layout below.
    bool agg = c->agg_on && c->lanes == 0 && placed >= agg_min() && gset_agg_tables(c) && agg_wanted(c);
    const uint32_t sub = c->agg_sub, unit = gset_agg_unit(sub);
    uint64_t slots = 0, R = 0;
    int lanes = 0;
    size_t cap = 0;
    if (agg) {
        c->gs_agg_n.resize(K); c->gs_rest.resize(K); c->gs_map.assign(3 * ((size_t)K + 1), 0);
        size_t rest = 0;
        for (uint32_t k = 0; k < K; k++) rest += c->gs_agg_ok[k] ? c->gs_totals[k] % unit : c->gs_totals[k];
        lanes = gset_agg_choose(c->gs_totals.data(), c->gs_agg_ok.data(), K, sub, miller_lanes(c, rest), 0, c->gs_agg_n.data(), c->gs_map.data(),
                                c->gs_rest.data(), c->gs_map.data() + K + 1, &R, &slots);
        for (uint32_t k = 0; k < K; k++) c->gs_map[2 * ((size_t)K + 1) + k] = c->gs_agg_n[k];
        if ((rc = groth16_ready(c, (size_t)slots, &cap)) != ZKV_OK) return rc;
        agg = R > 0 && c->agg_cap >= c->ws.cap && cap >= unit;       // (the aggregate buffers could be allocated)
    }
    if (!agg) {
        R = 0;
        lanes = gset_choose(c->gs_totals.data(), K, miller_lanes(c, placed), c->lanes != 0, c->gs_start.data(), &slots);
    }
    const size_t M = (size_t)slots;
    if ((rc = groth16_ready(c, M ? M : 1, &cap)) != ZKV_OK) return rc;     // (growing frees buffers, which synchronises the device)
    if ((rc = set_slot_buffers(c, M, &p, s)) != ZKV_OK) return rc;
    if (agg) {
        if ((rc = c->m_ks.start.grow(8 * (c->gs_map.size() + K + 1))) != ZKV_OK) return rc;
        HIP_TRY(hipMemsetAsync(c->m_ks.start + c->gs_map.size(), 0, 8 * ((size_t)K + 1), s));      // zero starts: k_gset_scan gives ranks
        HIP_TRY(hipMemcpyAsync(c->m_ks.start, c->gs_map.data(), 8 * c->gs_map.size(), hipMemcpyHostToDevice, s));
        launch_gset_agg_place(p, c->m_ks.start + c->gs_map.size(), c->m_ks.start, s);
    } else {
        HIP_TRY(hipMemcpyAsync(c->m_ks.start, c->gs_start.data(), 8 * ((size_t)K + 1), hipMemcpyHostToDevice, s));
        launch_gset_place(p, c->m_ks.start, s);
    }
    HIP_TRY(hipGetLastError());
    if (agg) {
        // aggregate chunks end on multiples of the unit, so no sub-batch and no 64-proof block straddles two of them; a region per key:
        // the keys lie back to back (astart[k + 1] = astart[k] + agg[k]) and stand for themselves
        std::vector<GsetAggChunk> plan;
        if ((rc = set_agg_plan(c, c->gs_map.data(), c->gs_map.data() + 1, nullptr, K, R, cap / unit * unit, sub, &plan, s)) != ZKV_OK) return rc;
        for (const GsetAggChunk& g : plan) {
            const GsetChunk ch = gset_chunk_of(c, p, d_proofs, d_signals, g.base, g.m);
            enqueue_gset_agg(c, ch, g, p.skey + g.base, c->m_ks.amap, sub, s, M == R && g.base + g.m >= R, [&] { launch_gset_prep(ch, c->ws, s); });
            HIP_TRY(hipGetLastError());
        }
    }
    for (size_t base = R; base < M; base += cap) {
        const size_t m = M - base < cap ? M - base : cap;
        const GsetChunk ch = gset_chunk_of(c, p, d_proofs, d_signals, base, m);
        if ((rc = gset_proof_stages(c, ch, lanes, base + cap >= M, s, [&] { launch_gset_prep(ch, c->ws, s); })) != ZKV_OK) return rc;
    }
    return set_return(c, n, M, p, d_verified, s);
}
ZKV_EXPORT int zkv_groth16_set_verify_batch_dev(zkv_ctx* c, size_t n, const uint32_t* d_key, const uint8_t* d_proofs, const uint8_t* d_signals,
                                                uint8_t* d_verified, void* stream) {
    if (!c || c->vm != ZKV_VM_GROTH16_SET) return ZKV_ERR_WRONG_CTX;
    if (n && (!d_key || !d_proofs || !d_verified || (c->g_n_ic > 1 && !d_signals))) return ZKV_ERR_INVALID_ARG;
    if (!n) return ZKV_OK;
    std::lock_guard<std::mutex> lk(c->mu);
    size_t cap = 0;
    int rc = groth16_ready(c, n, &cap);
    if (rc != ZKV_OK) return rc;
    hipStream_t s = stream ? (hipStream_t)stream : c->stream;
    if ((rc = order_after_previous(c, s)) != ZKV_OK) return rc;
    if ((rc = run_gset(c, n, d_key, d_proofs, d_signals, d_verified, s)) != ZKV_OK) return rc;
    return mark_done(c, s);
}
ZKV_EXPORT int zkv_groth16_set_verify_batch(zkv_ctx* c, size_t n, const uint32_t* key, const uint8_t* proofs, const uint8_t* signals, uint8_t* verified) {
    if (!c || c->vm != ZKV_VM_GROTH16_SET) return ZKV_ERR_WRONG_CTX;
    const size_t stride = (size_t)32 * (c->g_n_ic - 1);
    if (n && (!key || !proofs || !verified || (stride && !signals))) return ZKV_ERR_INVALID_ARG;
    if (!n) return ZKV_OK;
    std::lock_guard<std::mutex> lk(c->mu);
    size_t cap = 0;
    int rc = groth16_ready(c, n, &cap);
    if (rc != ZKV_OK) return rc;
    if ((rc = order_after_previous(c, c->stream)) != ZKV_OK) return rc;
    KeySetHostMem& hb = c->m_kshost;                           // the whole batch in HBM: keys, proofs, signals and the verdicts
    if ((rc = grow_all(hb.key, 4 * n, hb.proofs, 256 * n, hb.rows, stride * n + 8, hb.verdicts, n)) != ZKV_OK) return rc;
    HIP_TRY(hipMemcpyAsync(hb.key, key, 4 * n, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipMemcpyAsync(hb.proofs, proofs, 256 * n, hipMemcpyHostToDevice, c->stream));
    if (stride) HIP_TRY(hipMemcpyAsync(hb.rows, signals, stride * n, hipMemcpyHostToDevice, c->stream));
    if ((rc = run_gset(c, n, hb.key, hb.proofs, hb.rows, hb.verdicts, c->stream)) != ZKV_OK) return rc;
    HIP_TRY(hipMemcpyAsync(verified, hb.verdicts, n, hipMemcpyDeviceToHost, c->stream));
    if ((rc = mark_done(c, c->stream)) != ZKV_OK) return rc;
    HIP_TRY(hipStreamSynchronize(c->stream));
    return ZKV_OK;
}
ZKV_EXPORT int zkv_groth16_set_vk_x_batch(zkv_ctx* c, size_t n, const uint32_t* key, const uint8_t* signals, uint8_t* out) {
    if (!c || c->vm != ZKV_VM_GROTH16_SET) return ZKV_ERR_WRONG_CTX;
    const size_t stride = (size_t)32 * (c->g_n_ic - 1);
    if (n && (!key || !out || (stride && !signals))) return ZKV_ERR_INVALID_ARG;
    for (size_t i = 0; i < n; i++) if (key[i] >= c->gs_nic.size()) return ZKV_ERR_INVALID_ARG;
    if (!n) return ZKV_OK;
    std::lock_guard<std::mutex> lk(c->mu);
    size_t cap = 0;
    int rc = groth16_ready(c, n, &cap);
    if (rc != ZKV_OK) return rc;
    if ((rc = order_after_previous(c, c->stream)) != ZKV_OK) return rc;
    KeySetHostMem& hb = c->m_kshost;
    if ((rc = grow_all(hb.key, 4 * n, hb.rows, stride * n + 8, hb.vk_x, 64 * n)) != ZKV_OK) return rc;
    HIP_TRY(hipMemcpyAsync(hb.key, key, 4 * n, hipMemcpyHostToDevice, c->stream));
    if (stride) HIP_TRY(hipMemcpyAsync(hb.rows, signals, stride * n, hipMemcpyHostToDevice, c->stream));
    launch_gset_vk_x(n, msm_lanes_long(c, n), hb.key, c->d_gs_key, c->d_gs_rows, c->d_gs_win, hb.rows, (uint32_t)stride, hb.vk_x, c->stream);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(out, hb.vk_x, 64 * n, hipMemcpyDeviceToHost, c->stream));
    if ((rc = mark_done(c, c->stream)) != ZKV_OK) return rc;
    HIP_TRY(hipStreamSynchronize(c->stream));
    return ZKV_OK;
}

// ------------------------------------------------------------------ Groth16 key sets of deployed contracts: eth_call batches
// (zkv_groth16_set_wire.h; parity unpinned).  k_gset_wire_decode turns every request into a row of the set's
// ordinary inputs, run_gset runs on those rows as it runs on a caller's, and k_gset_wire_return merges its verdicts with the decoder's.
static bool gsw_signature(int form, size_t n_sig, char out[96]) {
    if ((form != ZKV_G16_FORM_SNARKJS && form != ZKV_G16_FORM_GNARK) || n_sig < 1 || n_sig >= ZKV_GROTH16_MAX_IC) return false;
    snprintf(out, 96, form == ZKV_G16_FORM_SNARKJS ? "verifyProof(uint256[2],uint256[2][2],uint256[2],uint256[%zu])" : "verifyProof(uint256[8],uint256[%zu])", n_sig);
    return true;
}
ZKV_EXPORT int zkv_groth16_set_call_selector(int form, size_t n_signals, uint8_t out[4]) {
    char sig[96];
    if (!out || !gsw_signature(form, n_signals, sig)) return ZKV_ERR_INVALID_ARG;
    host::fn_selector(sig, out);
    return ZKV_OK;
}
static bool is_deployed_set(const zkv_ctx* c) { return c && c->vm == ZKV_VM_GROTH16_SET && !c->gsw_tab.empty(); }
ZKV_EXPORT zkv_ctx* zkv_groth16_set_create_deployed(size_t n_keys, const uint8_t* const* vk_words, const size_t* n_ic, const int* vm_type,
                                                    const uint8_t* addresses, const uint8_t* form, int device) {
    if (!addresses || !form) return nullptr;
    zkv_ctx* c = zkv_groth16_set_create(n_keys, vk_words, n_ic, vm_type, device);
    if (!c) return nullptr;
    try {
        c->gsw_tab.resize(n_keys);
        c->gsw_form.assign(form, form + n_keys);
    } catch (const std::bad_alloc&) { delete c; return nullptr; }
    bool ok = true;
    for (size_t k = 0; k < n_keys && ok; k++) {
        GswEntry& e = c->gsw_tab[k];
        for (int j = 0; j < 5; j++) e.addr[j] = be32_of(addresses + 20 * k + 4 * j);
        e.key = (uint32_t)k; e.sel_be = 0; e.n_sig = GSW_NONE;           // (n_ic = 1: no method)
        ok = form[k] == ZKV_G16_FORM_SNARKJS || form[k] == ZKV_G16_FORM_GNARK;
        uint8_t sel[4];
        if (ok && n_ic[k] > 1) {
            (void)zkv_groth16_set_call_selector(form[k], n_ic[k] - 1, sel);
            e.sel_be = be32_of(sel); e.n_sig = (uint32_t)(n_ic[k] - 1);
        }
    }
    std::sort(c->gsw_tab.begin(), c->gsw_tab.end(), [](const GswEntry& a, const GswEntry& b) { return gsw_addr_cmp(a.addr, b.addr) < 0; });
    for (size_t k = 1; k < n_keys && ok; k++) ok = gsw_addr_cmp(c->gsw_tab[k - 1].addr, c->gsw_tab[k].addr) != 0;
    if (!ok) { delete c; return nullptr; }
    host::fn_selector("ProofInvalid()", c->gsw_err[0]);
    host::fn_selector("PublicInputNotInField()", c->gsw_err[1]);
    return c;
}
ZKV_EXPORT int zkv_groth16_set_eth_call_returndata(const zkv_ctx* c, uint32_t key, uint8_t status, uint8_t out[ZKV_RETURNDATA_STRIDE], uint32_t* out_len,
                                                   uint8_t* reverted) {
    if (!is_deployed_set(c)) return ZKV_ERR_WRONG_CTX;
    if (!out || !out_len || !reverted) return ZKV_ERR_INVALID_ARG;
    *out_len = 0;
    if (status == ZKV_STATUS_NO_CONTRACT) { *reverted = 0; return ZKV_OK; }             // an address without code: success, no data
    if (status == ZKV_STATUS_BAD_CALLDATA) { *reverted = 1; return ZKV_OK; }            // the contract's dispatcher reverts with no data
    if ((status != ZKV_STATUS_OK && status != ZKV_STATUS_VERIFICATION_FAILED && status != ZKV_STATUS_INPUT_NOT_IN_FIELD) || key >= c->gsw_form.size())
        return ZKV_ERR_INVALID_ARG;
    if (c->gsw_form[key] == ZKV_G16_FORM_SNARKJS) {                                     // returns (bool), whatever went wrong
        *reverted = 0; *out_len = 32;
        memset(out, 0, 32);
        out[31] = status == ZKV_STATUS_OK ? 1 : 0;
        return ZKV_OK;
    }
    *reverted = status == ZKV_STATUS_OK ? 0 : 1;
    if (status != ZKV_STATUS_OK) { memcpy(out, c->gsw_err[status == ZKV_STATUS_INPUT_NOT_IN_FIELD ? 1 : 0], 4); *out_len = 4; }
    return ZKV_OK;
}
// Addresses, calldata and its n + 1 offsets on the device (c->mu held).  The decode is enqueued in front of the partition, so the call
// synchronises where run_gset does; d_key: the resolved keys go there (the host call passes its own row).
static int run_gset_wire(zkv_ctx* c, size_t n, const uint8_t* d_to, const uint8_t* d_cd, const uint64_t* d_off, uint64_t cd_bytes, uint8_t* d_status,
                         uint32_t* d_key, hipStream_t s) {
    size_t cap = 0;
    int rc = groth16_ready(c, n, &cap);
    if (rc != ZKV_OK) return rc;
    GsetWireMem& gm = c->m_gsw;
    const size_t stride = (size_t)32 * (c->g_n_ic - 1);
    if ((rc = grow_all(gm.key, 4 * n, gm.rkey, d_key ? 0 : 4 * n, gm.proofs, 256 * n, gm.rows, stride * n + 8, gm.verdict, n, gm.ge_r, n, gm.verified, n,
                       gm.cnt, 4 * sizeof(unsigned long long))) != ZKV_OK) return rc;
    if (!gm.tab) {                                               // once per device set-up: the table is the context's own, sorted at creation
        if ((rc = gm.tab.alloc(sizeof(GswEntry) * c->gsw_tab.size())) != ZKV_OK) return rc;
        HIP_TRY(hipMemcpy(gm.tab, c->gsw_tab.data(), sizeof(GswEntry) * c->gsw_tab.size(), hipMemcpyHostToDevice));
    }
    if ((rc = order_after_previous(c, s)) != ZKV_OK) return rc;
    HIP_TRY(hipMemsetAsync(gm.cnt, 0, 4 * sizeof(unsigned long long), s));
    GswArgs w;
    memset(&w, 0, sizeof w);
    w.n = n; w.to = d_to; w.cd = d_cd; w.off = d_off; w.cd_bytes = cd_bytes;
    w.tab = gm.tab; w.n_tab = (uint32_t)c->gsw_tab.size();
    w.key = gm.key; w.rkey = d_key ? d_key : (uint32_t*)gm.rkey; w.proofs = gm.proofs; w.rows = gm.rows; w.sig_stride = (uint32_t)stride;
    w.verdict = gm.verdict; w.ge_r = gm.ge_r;
    (void)hipEventRecord(c->ev_wire[0], s);
    launch_gset_wire_decode(w, s);
    (void)hipEventRecord(c->ev_wire[1], s);
    c->wire_timed = true;
    HIP_TRY(hipGetLastError());
    if ((rc = run_gset(c, n, gm.key, gm.proofs, gm.rows, gm.verified, s)) != ZKV_OK) return rc;
    launch_gset_wire_return(n, gm.verdict, gm.ge_r, gm.verified, d_status, gm.cnt, s);
    HIP_TRY(hipGetLastError());
    return mark_done(c, s);
}
ZKV_EXPORT int zkv_groth16_set_eth_call_batch_dev(zkv_ctx* c, size_t n, const uint8_t* d_to, const uint8_t* d_calldata, const uint64_t* d_calldata_off,
                                                  uint64_t calldata_bytes, uint8_t* d_status, uint32_t* d_key, void* stream) {
    if (!is_deployed_set(c)) return ZKV_ERR_WRONG_CTX;
    if (n && (!d_to || !d_calldata || !d_calldata_off || !d_status)) return ZKV_ERR_INVALID_ARG;
    if (!n) return ZKV_OK;
    if (n > 0xFFFFFFF0u) return ZKV_ERR_INVALID_ARG;
    std::lock_guard<std::mutex> lk(c->mu);
    int rc = ctx_device_init(c);
    if (rc != ZKV_OK) return rc;
    return run_gset_wire(c, n, d_to, d_calldata, d_calldata_off, calldata_bytes, d_status, d_key, stream ? (hipStream_t)stream : c->stream);
}
ZKV_EXPORT int zkv_groth16_set_eth_call_batch(zkv_ctx* c, size_t n, const uint8_t* to, const uint8_t* blob, const uint64_t* off, uint8_t* reverted,
                                              uint8_t* returndata, uint32_t* returndata_len, uint8_t* status) {
    if (!is_deployed_set(c)) return ZKV_ERR_WRONG_CTX;
    if (n && (!to || !blob || !off || !reverted || !returndata || !returndata_len)) return ZKV_ERR_INVALID_ARG;
    if (!n) return ZKV_OK;
    if (n > 0xFFFFFFF0u) return ZKV_ERR_INVALID_ARG;
    std::vector<uint8_t> st(n);
    std::vector<uint32_t> key(n);
    {
        std::lock_guard<std::mutex> lk(c->mu);
        int rc = ctx_device_init(c);
        if (rc != ZKV_OK) return rc;
        const uint64_t bytes = off[n];                           // the blob; a request may still run backwards or past it
        GsetWireMem& gm = c->m_gsw;
        if ((rc = grow_all(gm.h_to, 20 * n, gm.h_cd, (size_t)bytes + 8, gm.h_cdoff, 8 * (n + 1), gm.h_st, n, gm.rkey, 4 * n)) != ZKV_OK) return rc;
        hipStream_t s = c->stream;
        if ((rc = order_after_previous(c, s)) != ZKV_OK) return rc;
        HIP_TRY(hipMemcpyAsync(gm.h_to, to, 20 * n, hipMemcpyHostToDevice, s));
        if (bytes) HIP_TRY(hipMemcpyAsync(gm.h_cd, blob, (size_t)bytes, hipMemcpyHostToDevice, s));
        HIP_TRY(hipMemcpyAsync(gm.h_cdoff, off, 8 * (n + 1), hipMemcpyHostToDevice, s));
        if ((rc = run_gset_wire(c, n, gm.h_to, gm.h_cd, gm.h_cdoff, bytes, gm.h_st, gm.rkey, s)) != ZKV_OK) return rc;
        HIP_TRY(hipMemcpyAsync(st.data(), gm.h_st, n, hipMemcpyDeviceToHost, s));
        HIP_TRY(hipMemcpyAsync(key.data(), gm.rkey, 4 * n, hipMemcpyDeviceToHost, s));
        HIP_TRY(hipStreamSynchronize(s));
    }
    for (size_t i = 0; i < n; i++) {
        const int rc = zkv_groth16_set_eth_call_returndata(c, key[i], st[i], returndata + i * ZKV_RETURNDATA_STRIDE, &returndata_len[i], &reverted[i]);
        if (rc != ZKV_OK) return rc;
        if (status) status[i] = st[i];
    }
    return ZKV_OK;
}
ZKV_EXPORT int zkv_groth16_set_last_call_counts(zkv_ctx* c, uint64_t out[4]) {
    if (!is_deployed_set(c)) return ZKV_ERR_WRONG_CTX;
    if (!out) return ZKV_ERR_INVALID_ARG;
    std::lock_guard<std::mutex> lk(c->mu);
    memset(out, 0, 4 * sizeof(uint64_t));
    if (!c->dev_ready || !c->m_gsw.cnt || !c->has_done) return ZKV_OK;       // no eth_call batch has run
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(hipEventSynchronize(c->ev_done));
    HIP_TRY(hipMemcpy(out, c->m_gsw.cnt, 4 * sizeof(uint64_t), hipMemcpyDeviceToHost));
    return ZKV_OK;
}

// ------------------------------------------------------------------ PLONK key sets (zkv_plonk_set.h)
// No reference counterpart: parity unpinned.  The Groth16 sets' partition by key with 64-slot key groups (zkv_gset_layout.h pset_choose),
// PREP with the key of each wavefront (k_plonk_set.hip), the Groth16 sets' Miller loops with every key's [1]_2 / [tau]_2 in the gamma /
// delta slots of its VkTables, the single-key final exponentiation, and the Groth16 sets' return to the caller's order.
static size_t pset_proof_stride(const zkv_ctx* c) { return (size_t)32 * (24 + 3 * c->ps_nc_max); }
static size_t pset_input_stride(const zkv_ctx* c) { return (size_t)32 * c->ps_nb_max; }
// Host batches stage the public inputs of a chunk next to the proofs: at most LONG_STAGE_BYTES, sized by the set's largest nb_public.
static size_t pset_host_chunk(const zkv_ctx* c) {
    const size_t per = pset_input_stride(c), cap = chunk_capacity();
    if (!per) return cap;
    size_t lim = 64;
    while (lim < cap && 2 * lim * per <= LONG_STAGE_BYTES) lim *= 2;
    return lim < cap ? lim : cap;
}
// Set-up of every key whatever K is: the VkTables of its two G2 points (k_gset.hip's kernels, grid y = key; the VkRaw the single-key PLONK
// path builds), then its PlonkKey (24 MB) and validity word (k_plonk_set.hip).
static int pset_device_setup(zkv_ctx* c) {
    const uint32_t K = (uint32_t)c->ps_raw.size();
    std::vector<VkRaw> raw(K);
    std::vector<GsetKey> keys(K);
    for (uint32_t k = 0; k < K; k++) {
        memset(&raw[k], 0, sizeof raw[k]);
        const uint8_t* g2 = c->ps_g2.data() + 256 * (size_t)k;
        const int perm[4] = {1, 0, 3, 2};
        for (int q = 0; q < 4; q++) { host::be_to_limbs(raw[k].gamma[q], g2 + 32 * perm[q]); host::be_to_limbs(raw[k].delta[q], g2 + 128 + 32 * perm[q]); }
    }
    HIP_TRY(c->d_gs_tab.alloc(sizeof(VkTables) * K));
    HIP_TRY(hipMemsetAsync(c->d_gs_tab, 0, sizeof(VkTables) * K, c->stream));
    for (uint32_t k = 0; k < K; k++) keys[k] = GsetKey{c->d_gs_tab + k, 0u, 0u, 0u, 0u};
    HIP_TRY(c->d_gs_key.alloc(sizeof(GsetKey) * K));
    HIP_TRY(hipMemcpyAsync(c->d_gs_key, keys.data(), sizeof(GsetKey) * K, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(c->d_pkey.alloc(sizeof(PlonkKey) * K));
    HIP_TRY(c->d_ps_ok.alloc(sizeof(uint32_t) * K));
    // the raw keys are only read by the set-up kernels: scoped, released after the synchronisation below
    DevBuf<VkRaw> d_raw;
    DevBuf<PlonkKeyRaw> d_pk;
    HIP_TRY(d_raw.alloc(sizeof(VkRaw) * K));
    HIP_TRY(d_pk.alloc(sizeof(PlonkKeyRaw) * K));
    HIP_TRY(hipMemcpyAsync(d_raw, raw.data(), sizeof(VkRaw) * K, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipMemcpyAsync(d_pk, c->ps_raw.data(), sizeof(PlonkKeyRaw) * K, hipMemcpyHostToDevice, c->stream));
    launch_gset_setup(K, d_raw, c->d_gs_tab, 0, nullptr, nullptr, nullptr, nullptr, c->stream);
    launch_pset_setup(K, d_pk, c->d_pkey, c->d_gs_tab, c->d_ps_ok, c->stream);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(c->stream));                // the host vectors above go out of scope
    return ZKV_OK;
}
ZKV_EXPORT zkv_ctx* zkv_plonk_set_create(size_t n_keys, const uint8_t* const* vk_bytes, const size_t* vk_len, int device) {
    if (n_keys < 1 || n_keys > ZKV_PLONK_SET_MAX_KEYS || !vk_bytes || !vk_len) return nullptr;
    std::vector<PlonkKeyRaw> raw;
    std::vector<uint8_t> g2;
    try {
        raw.resize(n_keys);
        g2.resize(256 * n_keys);
    } catch (const std::bad_alloc&) { return nullptr; }
    uint32_t nb_max = 0, nc_max = 0;
    for (size_t k = 0; k < n_keys; k++) {
        if (!plonk_parse_key(vk_bytes[k], vk_len[k], raw[k], g2.data() + 256 * k)) return nullptr;
        if (raw[k].nb_public > nb_max) nb_max = raw[k].nb_public;
        if (raw[k].n_c > nc_max) nc_max = raw[k].n_c;
    }
    zkv_ctx* c = new (std::nothrow) zkv_ctx();
    if (!c) return nullptr;
    c->vm = ZKV_VM_PLONK_SET; c->device = device; c->initialized = true;
    memset(&c->consts, 0, sizeof c->consts);
    try {
        c->ps_class.resize(n_keys); c->ps_cls_rep.resize(n_keys);
        c->ps_cls_rep.resize(pset_srs_classes(g2.data(), (uint32_t)n_keys, c->ps_class.data(), c->ps_cls_rep.data()));
    } catch (const std::bad_alloc&) { delete c; return nullptr; }
    c->ps_raw = std::move(raw); c->ps_g2 = std::move(g2);
    c->ps_nb_max = nb_max; c->ps_nc_max = nc_max;
    return c;
}
// (zkv_plonk_set_agg.h) host only: the classes were formed at creation
ZKV_EXPORT int zkv_plonk_set_srs_classes(const zkv_ctx* c, uint32_t* class_of_key, size_t* n_classes) {
    if (!c || c->vm != ZKV_VM_PLONK_SET) return ZKV_ERR_WRONG_CTX;
    if (class_of_key) for (size_t k = 0; k < c->ps_class.size(); k++) class_of_key[k] = c->ps_class[k];
    if (n_classes) *n_classes = c->ps_cls_rep.size();
    return ZKV_OK;
}
ZKV_EXPORT size_t zkv_plonk_set_size(const zkv_ctx* c) { return c && c->vm == ZKV_VM_PLONK_SET ? c->ps_raw.size() : 0; }
ZKV_EXPORT size_t zkv_plonk_set_proof_stride(const zkv_ctx* c) { return c && c->vm == ZKV_VM_PLONK_SET ? pset_proof_stride(c) : 0; }
ZKV_EXPORT size_t zkv_plonk_set_input_stride(const zkv_ctx* c) { return c && c->vm == ZKV_VM_PLONK_SET ? pset_input_stride(c) : 0; }
ZKV_EXPORT int zkv_plonk_set_key_shape(const zkv_ctx* c, size_t key, size_t* nb_public, size_t* n_commitments, size_t* proof_bytes) {
    if (!c || c->vm != ZKV_VM_PLONK_SET) return ZKV_ERR_WRONG_CTX;
    if (key >= c->ps_raw.size()) return ZKV_ERR_INVALID_ARG;
    const PlonkKeyRaw& r = c->ps_raw[key];
    if (nb_public) *nb_public = r.nb_public;
    if (n_commitments) *n_commitments = r.n_c;
    if (proof_bytes) *proof_bytes = (size_t)32 * (24 + 3 * r.n_c);
    return ZKV_OK;
}
// Aggregate check on a PLONK set (zkv_plonk_set_agg.h).  Which SRS classes can take it -- the VkTables.vk_valid of
// each class's first key, i.e. its two G2 points passed the set-up validation -- and the counters, the first time a call wants the check: a
// set that never uses it allocates nothing.  false: no class can, or no room (the call then runs the per-proof path).
static bool pset_agg_classes(zkv_ctx* c) {
    if (c->d_agg_cnt) return c->agg_key_ok;
    const uint32_t n_cls = (uint32_t)c->ps_cls_rep.size();
    std::vector<uint32_t> ok(n_cls, 0);
    bool good = true;
    for (uint32_t q = 0; q < n_cls && good; q++)
        good = hipMemcpy(&ok[q], &c->d_gs_tab[c->ps_cls_rep[q]].vk_valid, sizeof(uint32_t), hipMemcpyDeviceToHost) == hipSuccess;
    if (!good || c->d_agg_cnt.alloc(3 * sizeof(unsigned long long)) ||
        hipMemset(c->d_agg_cnt, 0, 3 * sizeof(unsigned long long)) != hipSuccess) {
        (void)hipGetLastError();
        c->d_agg_cnt.release();
        return false;
    }
    c->ps_cls_ok.assign(n_cls, 0);
    c->agg_key_ok = false;
    for (uint32_t q = 0; q < n_cls; q++) { c->ps_cls_ok[q] = ok[q] ? 1 : 0; c->agg_key_ok = c->agg_key_ok || ok[q]; }
    return c->agg_key_ok;
}
// Slots [base, base + m) of a PLONK set's layout as one chunk
static PsetChunk pset_chunk_of(const zkv_ctx* c, const GsetPart& p, const uint8_t* d_proofs, const uint8_t* d_inputs, size_t base, size_t m) {
    PsetChunk ch;
    memset(&ch, 0, sizeof ch);
    ch.m = m; ch.slot0 = base; ch.idx = p.idx; ch.skey = p.skey;
    ch.keys = c->d_pkey; ch.ok = c->d_ps_ok;
    ch.proofs = d_proofs; ch.proof_stride = (uint32_t)pset_proof_stride(c);
    ch.inputs = d_inputs; ch.input_stride = (uint32_t)pset_input_stride(c);
    ch.plonk_tab = c->d_plonk_tab; ch.status = c->d_st_all + base;
    return ch;
}
// The aggregate check of one chunk of a PLONK set's aggregate region: PREP unchanged, the coefficients and r_i D_i, r_i (-Q_i)
// (k_agg_plonk_g1: no per-proof Miller loop), one pseudo-proof per sub-batch with its class's [1]_2 / [tau]_2 lines, its final
// exponentiation, the verdicts, and the per-proof kernels once more over the proofs of the sub-batches that failed -- in place, on the
// proofs' own points (k_agg_plonk_g1 leaves PREP's rows in ws.norm alone), so the verdict is the per-proof one.
static void enqueue_pset_agg(zkv_ctx* c, const PsetChunk& ch, const GsetAggChunk& g, const uint32_t* skey, const uint32_t* d_amap, uint32_t sub,
                             hipStream_t s, bool timed) {
    const size_t m = ch.m;
    const uint32_t sub64 = sub < 64 ? sub : 64;
    const uint32_t* psl = d_amap + g.off;
    const uint32_t* skey2 = psl + g.n2;
    if (timed) (void)hipEventRecord(c->ev[0], s);
    launch_pset_prep(ch, c->ws, s);
    if (timed) (void)hipEventRecord(c->ev[1], s);
    agg_next_coefficients(c);
    launch_agg_plonk_g1(m, c->ws, c->d_agg, c->agg_seed, s);
    if (timed) { (void)hipEventRecord(c->ev[2], s); (void)hipEventRecord(c->ev[3], s); }
    (void)hipMemsetAsync(c->ws2.flags, 0, sizeof(uint32_t) * g.slots, s);     // pad slots of the pseudo-proofs: no proof
    launch_pset_agg_reduce(m, sub64, c->ws, c->d_agg, c->ws2, c->d_status2, psl, sub > 64, s);
    if (sub > 64) launch_pset_agg_combine(g.n2, sub / 64, c->ws2, c->d_status2, psl, s);
    launch_gset_miller(g.lanes, (size_t)g.slots, skey2, c->d_gs_key, c->ws2, c->d_status2, s);
    if (timed) (void)hipEventRecord(c->ev[4], s);
    launch_finalexp_lanes(g.lanes, (size_t)g.slots, c->ws2, c->d_status2, s);
    launch_gset_agg_mark(m, sub, 1, c->ws, c->d_agg, c->d_status2, psl, ch.status, c->d_agg_cnt, s);
    launch_gset_miller(2, m, skey, c->d_gs_key, c->ws, ch.status, s);
    launch_finalexp2(m, c->ws, ch.status, s);
    if (timed) (void)hipEventRecord(c->ev[5], s);
}
// One call of n proofs, every buffer on the device, enqueued on s (c->mu held, device set up).  Partition by key (count; the per-key totals
// come back to the host, which lays the groups out on 64-slot boundaries and picks the Miller mapping; place), then the stages chunk by
// chunk over the slots, then the verdicts back to the caller's order.  No G2 subgroup check (a PLONK proof has no G2 point).  With the
// aggregate check (automatic mapping, at least ZKV_AGG_MIN proofs placed, a capable SRS class) the groups are ordered class by class
// (pset_agg_choose): slots [0, R) take enqueue_pset_agg, the classes that cannot take the check follow on the per-proof path.
static int run_pset(zkv_ctx* c, size_t n, const uint32_t* d_key, const uint8_t* d_proofs, const uint8_t* d_inputs, uint8_t* d_verified, hipStream_t s) {
    const uint32_t K = (uint32_t)c->ps_raw.size();
    GsetPart p;
    size_t placed = 0;
    int rc;
    if ((rc = set_partition(c, n, K, d_key, s, &p, &placed)) != ZKV_OK) return rc;
    bool agg = c->agg_on && c->lanes == 0 && placed >= agg_min() && pset_agg_classes(c) && agg_wanted(c);
    const uint32_t sub = c->agg_sub, n_cls = (uint32_t)c->ps_cls_rep.size();
    uint64_t slots = 0, R = 0;
    int lanes = 0;
    if (agg) {
        c->ps_cbeg.assign(n_cls, 0); c->ps_cend.assign(n_cls, 0);
        lanes = pset_agg_choose(c->gs_totals.data(), c->ps_class.data(), K, c->ps_cls_ok.data(), n_cls, sub, 0, wave_below(), wide_below(),
                                c->gs_start.data(), c->ps_cbeg.data(), c->ps_cend.data(), &R, &slots);
        if ((rc = ctx_ready(c, slots ? (size_t)slots : 1)) != ZKV_OK) return rc;
        agg = R > 0 && c->agg_cap >= c->ws.cap && pset_agg_chunk_slots(c->ws.cap, sub) > 0;       // (the aggregate buffers could be allocated)
    }
    if (!agg) { R = 0; lanes = pset_choose(c->gs_totals.data(), K, c->lanes, wave_below(), wide_below(), c->gs_start.data(), &slots); }
    const size_t M = (size_t)slots;
    if ((rc = ctx_ready(c, M ? M : 1)) != ZKV_OK) return rc;     // (growing frees buffers, which synchronises the device)
    if ((rc = set_slot_buffers(c, M, &p, s)) != ZKV_OK) return rc;
    HIP_TRY(hipMemcpyAsync(c->m_ks.start, c->gs_start.data(), 8 * ((size_t)K + 1), hipMemcpyHostToDevice, s));
    launch_gset_place(p, c->m_ks.start, s);
    HIP_TRY(hipGetLastError());
    const size_t cap = c->ws.cap;                            // (a power of two >= 4,096 or ZKV_CHUNK, a multiple of 64: chunks keep the 64-slot groups)
    if (agg) {
        // aggregate chunks end on multiples of max(64, sub), so no sub-batch straddles two of them; a region per class, through the
        // class's first key, whose line tables are those of every key of the class; a class that cannot take the check: no region
        for (uint32_t q = 0; q < n_cls; q++) if (!c->ps_cls_ok[q]) c->ps_cend[q] = c->ps_cbeg[q];
        std::vector<GsetAggChunk> plan;
        if ((rc = set_agg_plan(c, c->ps_cbeg.data(), c->ps_cend.data(), c->ps_cls_rep.data(), n_cls, R, (size_t)pset_agg_chunk_slots(cap, sub), sub,
                               &plan, s)) != ZKV_OK) return rc;
        for (const GsetAggChunk& g : plan) {
            enqueue_pset_agg(c, pset_chunk_of(c, p, d_proofs, d_inputs, g.base, g.m), g, p.skey + g.base, c->m_ks.amap, sub, s,
                             M == R && g.base + g.m >= R);
            HIP_TRY(hipGetLastError());
        }
    }
    for (size_t base = (size_t)R; base < M; base += cap) {
        const size_t m = M - base < cap ? M - base : cap;
        const bool timed = base + cap >= M;
        const PsetChunk ch = pset_chunk_of(c, p, d_proofs, d_inputs, base, m);
        if (timed) (void)hipEventRecord(c->ev[0], s);
        launch_pset_prep(ch, c->ws, s);
        if (timed) { (void)hipEventRecord(c->ev[1], s); (void)hipEventRecord(c->ev[2], s); (void)hipEventRecord(c->ev[3], s); }
        launch_gset_miller(lanes, m, p.skey + base, c->d_gs_key, c->ws, ch.status, s);
        if (timed) (void)hipEventRecord(c->ev[4], s);
        launch_finalexp_lanes(lanes, m, c->ws, ch.status, s);
        if (timed) (void)hipEventRecord(c->ev[5], s);
        HIP_TRY(hipGetLastError());
    }
    return set_return(c, n, M, p, d_verified, s);
}
ZKV_EXPORT int zkv_plonk_set_verify_batch_dev(zkv_ctx* c, size_t n, const uint32_t* d_key, const uint8_t* d_proofs, const uint8_t* d_public_inputs,
                                              uint8_t* d_verified, void* stream) {
    if (!c || c->vm != ZKV_VM_PLONK_SET) return ZKV_ERR_WRONG_CTX;
    if (n && (!d_key || !d_proofs || !d_verified || (pset_input_stride(c) && !d_public_inputs))) return ZKV_ERR_INVALID_ARG;
    if (!n) return ZKV_OK;
    std::lock_guard<std::mutex> lk(c->mu);
    int rc = ctx_ready(c, n);
    if (rc != ZKV_OK) return rc;
    hipStream_t s = stream ? (hipStream_t)stream : c->stream;
    if ((rc = order_after_previous(c, s)) != ZKV_OK) return rc;
    if ((rc = run_pset(c, n, d_key, d_proofs, d_public_inputs, d_verified, s)) != ZKV_OK) return rc;
    return mark_done(c, s);
}
ZKV_EXPORT int zkv_plonk_set_verify_batch(zkv_ctx* c, size_t n, const uint32_t* key, const uint8_t* proofs, const uint8_t* public_inputs, uint8_t* verified) {
    if (!c || c->vm != ZKV_VM_PLONK_SET) return ZKV_ERR_WRONG_CTX;
    const size_t ps = pset_proof_stride(c), is = pset_input_stride(c);
    if (n && (!key || !proofs || !verified || (is && !public_inputs))) return ZKV_ERR_INVALID_ARG;
    if (!n) return ZKV_OK;
    std::lock_guard<std::mutex> lk(c->mu);
    const size_t hc = pset_host_chunk(c);
    int rc = ctx_ready(c, n < hc ? n : hc);
    if (rc != ZKV_OK) return rc;
    if ((rc = order_after_previous(c, c->stream)) != ZKV_OK) return rc;
    KeySetHostMem& hb = c->m_kshost;                           // chunks of the caller's order staged in HBM: keys, proofs, public inputs and the verdicts
    for (size_t base = 0; base < n; base += hc) {
        const size_t m = n - base < hc ? n - base : hc;
        if ((rc = grow_all(hb.key, 4 * m, hb.proofs, ps * m, hb.rows, is * m + 8, hb.verdicts, m)) != ZKV_OK) return rc;
        HIP_TRY(hipMemcpyAsync(hb.key, key + base, 4 * m, hipMemcpyHostToDevice, c->stream));
        HIP_TRY(hipMemcpyAsync(hb.proofs, proofs + ps * base, ps * m, hipMemcpyHostToDevice, c->stream));
        if (is) HIP_TRY(hipMemcpyAsync(hb.rows, public_inputs + is * base, is * m, hipMemcpyHostToDevice, c->stream));
        if ((rc = run_pset(c, m, hb.key, hb.proofs, is ? hb.rows : nullptr, hb.verdicts, c->stream)) != ZKV_OK) return rc;
        HIP_TRY(hipMemcpyAsync(verified + base, hb.verdicts, m, hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(hipStreamSynchronize(c->stream));
    }
    return mark_done(c, c->stream);
}

// ------------------------------------------------------------------ PLONK key sets of deployed contracts: eth_call batches
// (zkv_plonk_set_wire.h; parity unpinned).  k_pset_wire_decode turns every request into a row of the set's ordinary
// inputs, k_pset_wire_points takes the key from a request with a point the precompiles refuse, run_pset runs on those rows as it runs on
// a caller's, and k_pset_wire_return merges its verdicts with the classification.
static const uint8_t* psw_selector() {
    static const struct Sel { uint8_t b[2][4]; Sel() { host::fn_selector("Verify(bytes,uint256[])", b[0]); host::fn_selector("Error(string)", b[1]); } } s;
    return &s.b[0][0];
}
ZKV_EXPORT int zkv_plonk_set_call_selector(uint8_t out[4]) {
    if (!out) return ZKV_ERR_INVALID_ARG;
    memcpy(out, psw_selector(), 4);
    return ZKV_OK;
}
static bool is_deployed_pset(const zkv_ctx* c) { return c && c->vm == ZKV_VM_PLONK_SET && !c->psw_tab.empty(); }
ZKV_EXPORT zkv_ctx* zkv_plonk_set_create_deployed(size_t n_keys, const uint8_t* const* vk_bytes, const size_t* vk_len, const uint8_t* addresses, int device) {
    if (!addresses) return nullptr;
    zkv_ctx* c = zkv_plonk_set_create(n_keys, vk_bytes, vk_len, device);
    if (!c) return nullptr;
    try { c->psw_tab.resize(n_keys); } catch (const std::bad_alloc&) { delete c; return nullptr; }
    for (size_t k = 0; k < n_keys; k++) {
        PswEntry& e = c->psw_tab[k];
        for (int j = 0; j < 5; j++) e.addr[j] = be32_of(addresses + 20 * k + 4 * j);
        e.key = (uint32_t)k; e.nb = c->ps_raw[k].nb_public; e.n_c = c->ps_raw[k].n_c;
    }
    std::sort(c->psw_tab.begin(), c->psw_tab.end(), [](const PswEntry& a, const PswEntry& b) { return gsw_addr_cmp(a.addr, b.addr) < 0; });
    for (size_t k = 1; k < n_keys; k++)
        if (gsw_addr_cmp(c->psw_tab[k - 1].addr, c->psw_tab[k].addr) == 0) { delete c; return nullptr; }
    return c;
}
ZKV_EXPORT int zkv_plonk_set_eth_call_returndata(uint8_t status, uint8_t reason, uint8_t out[ZKV_PLONK_RETURNDATA_STRIDE], uint32_t* out_len, uint8_t* reverted) {
    if (!out || !out_len || !reverted) return ZKV_ERR_INVALID_ARG;
    static const char* const MSG[6] = {"", "wrong number of public inputs", "inputs are bigger than r", "wrong proof size", "openings bigger than r",
                                       "error ec operation"};
    *out_len = 0;
    if (reason == ZKV_PLONK_REVERT_NONE) {
        if (status == ZKV_STATUS_NO_CONTRACT) { *reverted = 0; return ZKV_OK; }         // an address without code: success, no data
        if (status == ZKV_STATUS_BAD_CALLDATA) { *reverted = 1; return ZKV_OK; }        // the contract's dispatcher or ABI decoder reverts with no data
        if (status != ZKV_STATUS_OK && status != ZKV_STATUS_VERIFICATION_FAILED) return ZKV_ERR_INVALID_ARG;
        *reverted = 0; *out_len = 32;                                                   // returns (bool)
        memset(out, 0, 32);
        out[31] = status == ZKV_STATUS_OK ? 1 : 0;
        return ZKV_OK;
    }
    if (reason > ZKV_PLONK_REVERT_EC_OPERATION ||
        status != (reason == ZKV_PLONK_REVERT_INPUT_RANGE ? ZKV_STATUS_INPUT_NOT_IN_FIELD : ZKV_STATUS_INVALID_PROOF_DATA)) return ZKV_ERR_INVALID_ARG;
    const size_t len = strlen(MSG[reason]);                                             // Error(string): selector, offset 0x20, length, the message padded to 32
    memset(out, 0, 100);
    memcpy(out, psw_selector() + 4, 4);
    out[35] = 0x20; out[67] = (uint8_t)len;
    memcpy(out + 68, MSG[reason], len);
    *reverted = 1; *out_len = 100;
    return ZKV_OK;
}
// Addresses, calldata and its n + 1 offsets on the device (c->mu held, device set up and ordered after the previous call).  Decode and
// point test are enqueued in front of the partition, so the call synchronises where run_pset does; d_key: the resolved keys go there.
static int run_pset_wire(zkv_ctx* c, size_t n, const uint8_t* d_to, const uint8_t* d_cd, const uint64_t* d_off, uint64_t cd_bytes, uint8_t* d_status,
                         uint8_t* d_reason, uint32_t* d_key, hipStream_t s) {
    int rc;
    PsetWireMem& pm = c->m_psw;
    const size_t ps = pset_proof_stride(c), is = pset_input_stride(c);
    if ((rc = grow_all(pm.key, 4 * n, pm.rkey, d_key ? 0 : 4 * n, pm.proofs, ps * n, pm.rows, is * n + 8, pm.verdict, n, pm.reason, n, pm.npt, n, pm.ec, n,
                       pm.verified, n, pm.cnt, 8 * sizeof(unsigned long long))) != ZKV_OK) return rc;
    if (!pm.tab) {                                               // once per device set-up: the table is the context's own, sorted at creation
        if ((rc = pm.tab.alloc(sizeof(PswEntry) * c->psw_tab.size())) != ZKV_OK) return rc;
        HIP_TRY(hipMemcpy(pm.tab, c->psw_tab.data(), sizeof(PswEntry) * c->psw_tab.size(), hipMemcpyHostToDevice));
    }
    HIP_TRY(hipMemsetAsync(pm.cnt, 0, 8 * sizeof(unsigned long long), s));
    PswArgs w;
    memset(&w, 0, sizeof w);
    w.n = n; w.to = d_to; w.cd = d_cd; w.off = d_off; w.cd_bytes = cd_bytes;
    w.tab = pm.tab; w.n_tab = (uint32_t)c->psw_tab.size(); w.sel_be = be32_of(psw_selector());
    w.key = pm.key; w.rkey = d_key ? d_key : (uint32_t*)pm.rkey; w.proofs = pm.proofs; w.proof_stride = (uint32_t)ps; w.rows = pm.rows; w.input_stride = (uint32_t)is;
    w.verdict = pm.verdict; w.reason = pm.reason; w.npt = pm.npt; w.ec = pm.ec;
    (void)hipEventRecord(c->ev_wire[0], s);
    launch_pset_wire_decode(w, s);
    launch_pset_wire_points(w, s);
    (void)hipEventRecord(c->ev_wire[1], s);
    c->wire_timed = true;
    HIP_TRY(hipGetLastError());
    if ((rc = run_pset(c, n, pm.key, pm.proofs, is ? (const uint8_t*)pm.rows : nullptr, pm.verified, s)) != ZKV_OK) return rc;
    launch_pset_wire_return(n, pm.verdict, pm.reason, pm.ec, pm.verified, d_status, d_reason, pm.cnt, s);
    HIP_TRY(hipGetLastError());
    return mark_done(c, s);
}
ZKV_EXPORT int zkv_plonk_set_eth_call_batch_dev(zkv_ctx* c, size_t n, const uint8_t* d_to, const uint8_t* d_calldata, const uint64_t* d_calldata_off,
                                                uint64_t calldata_bytes, uint8_t* d_status, uint8_t* d_reason, uint32_t* d_key, void* stream) {
    if (!is_deployed_pset(c)) return ZKV_ERR_WRONG_CTX;
    if (n && (!d_to || !d_calldata || !d_calldata_off || !d_status)) return ZKV_ERR_INVALID_ARG;
    if (!n) return ZKV_OK;
    if (n > 0xFFFFFFF0u) return ZKV_ERR_INVALID_ARG;
    std::lock_guard<std::mutex> lk(c->mu);
    int rc = ctx_ready(c, n);
    if (rc != ZKV_OK) return rc;
    hipStream_t s = stream ? (hipStream_t)stream : c->stream;
    if ((rc = order_after_previous(c, s)) != ZKV_OK) return rc;
    return run_pset_wire(c, n, d_to, d_calldata, d_calldata_off, calldata_bytes, d_status, d_reason, d_key, s);
}
ZKV_EXPORT int zkv_plonk_set_eth_call_batch(zkv_ctx* c, size_t n, const uint8_t* to, const uint8_t* blob, const uint64_t* off, uint8_t* reverted,
                                            uint8_t* returndata, uint32_t* returndata_len, uint8_t* status, uint8_t* reason) {
    if (!is_deployed_pset(c)) return ZKV_ERR_WRONG_CTX;
    if (n && (!to || !blob || !off || !reverted || !returndata || !returndata_len)) return ZKV_ERR_INVALID_ARG;
    if (!n) return ZKV_OK;
    if (n > 0xFFFFFFF0u) return ZKV_ERR_INVALID_ARG;
    std::vector<uint8_t> st(n), rs(n);
    {
        std::lock_guard<std::mutex> lk(c->mu);
        int rc = ctx_ready(c, n);
        if (rc != ZKV_OK) return rc;
        const uint64_t bytes = off[n];                           // the blob; a request may still run backwards or past it
        PsetWireMem& pm = c->m_psw;
        if ((rc = grow_all(pm.h_to, 20 * n, pm.h_cd, (size_t)bytes + 8, pm.h_cdoff, 8 * (n + 1), pm.h_st, n, pm.h_rs, n)) != ZKV_OK) return rc;
        hipStream_t s = c->stream;
        if ((rc = order_after_previous(c, s)) != ZKV_OK) return rc;
        HIP_TRY(hipMemcpyAsync(pm.h_to, to, 20 * n, hipMemcpyHostToDevice, s));
        if (bytes) HIP_TRY(hipMemcpyAsync(pm.h_cd, blob, (size_t)bytes, hipMemcpyHostToDevice, s));
        HIP_TRY(hipMemcpyAsync(pm.h_cdoff, off, 8 * (n + 1), hipMemcpyHostToDevice, s));
        if ((rc = run_pset_wire(c, n, pm.h_to, pm.h_cd, pm.h_cdoff, bytes, pm.h_st, pm.h_rs, nullptr, s)) != ZKV_OK) return rc;
        HIP_TRY(hipMemcpyAsync(st.data(), pm.h_st, n, hipMemcpyDeviceToHost, s));
        HIP_TRY(hipMemcpyAsync(rs.data(), pm.h_rs, n, hipMemcpyDeviceToHost, s));
        HIP_TRY(hipStreamSynchronize(s));
    }
    for (size_t i = 0; i < n; i++) {
        const int rc = zkv_plonk_set_eth_call_returndata(st[i], rs[i], returndata + i * ZKV_PLONK_RETURNDATA_STRIDE, &returndata_len[i], &reverted[i]);
        if (rc != ZKV_OK) return rc;
        if (status) status[i] = st[i];
        if (reason) reason[i] = rs[i];
    }
    return ZKV_OK;
}
ZKV_EXPORT int zkv_plonk_set_last_call_counts(zkv_ctx* c, uint64_t out[8]) {
    if (!is_deployed_pset(c)) return ZKV_ERR_WRONG_CTX;
    if (!out) return ZKV_ERR_INVALID_ARG;
    std::lock_guard<std::mutex> lk(c->mu);
    memset(out, 0, 8 * sizeof(uint64_t));
    if (!c->dev_ready || !c->m_psw.cnt || !c->has_done) return ZKV_OK;       // no eth_call batch has run
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(hipEventSynchronize(c->ev_done));
    HIP_TRY(hipMemcpy(out, c->m_psw.cnt, 8 * sizeof(uint64_t), hipMemcpyDeviceToHost));
    return ZKV_OK;
}

// ------------------------------------------------------------------ Groth16 core pieces
ZKV_EXPORT int zkv_ctx_vk_x_batch(zkv_ctx* c, size_t n, const uint8_t* var_signals, uint8_t* out) {
    if (is_sharded(c)) c = c->shards[0];
    if (!c || c->vm == ZKV_VM_BN254 || c->vm == ZKV_VM_RISC0_SET || c->vm == ZKV_VM_MIXED || c->vm == ZKV_VM_SP1_PLONK || c->vm == ZKV_VM_GROTH16_SET ||
        c->vm == ZKV_VM_SP1_GATEWAY || c->vm == ZKV_VM_PLONK || c->vm == ZKV_VM_PLONK_SET || c->vm == ZKV_VM_RISC0_SETINCL || c->vm == ZKV_VM_RISC0_ROUTER)
        return ZKV_ERR_WRONG_CTX;
    if (c->vm == ZKV_VM_RISC0 && !c->initialized) return ZKV_ERR_INVALID_ARG;
    if (n && (!var_signals || !out)) return ZKV_ERR_INVALID_ARG;
    if (!n) return ZKV_OK;
    // per-proof signals: two for the RISC Zero / SP1 keys, all n_ic - 1 for a generic key (k_vk_x reads n_var x 32 bytes per proof)
    const size_t sig = 32 * (size_t)(c->vm == ZKV_VM_GROTH16 ? c->g_n_ic - 1 : 2);
    std::lock_guard<std::mutex> lk(c->mu);
    size_t cap = 0;
    int rc = c->vm == ZKV_VM_GROTH16 ? groth16_ready(c, n, &cap) : ctx_ready(c, n, false);
    if (rc != ZKV_OK) return rc;
    if (c->vm != ZKV_VM_GROTH16) cap = c->ws.cap;
    if ((rc = order_after_previous(c, c->stream)) != ZKV_OK) return rc;
    for (size_t base = 0; base < n; base += cap) {
        size_t m = n - base < cap ? n - base : cap;
        if ((rc = c->d_blob.grow(m * sig + 8)) != ZKV_OK) return rc;
        if ((rc = c->d_pv.grow(m * 64 + 8)) != ZKV_OK) return rc;
        if (sig) HIP_TRY(hipMemcpyAsync(c->d_blob, var_signals + sig * base, sig * m, hipMemcpyHostToDevice, c->stream));
        if (c->long_key) launch_vk_x_long(m, msm_lanes_long(c, m), c->d_tab, long_key_of(c), c->d_blob, c->d_pv, c->stream);
        else launch_vk_x(m, c->d_tab, c->m16, nullptr, nullptr, c->d_blob, c->d_pv, c->stream);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipMemcpyAsync(out + 64 * base, c->d_pv, 64 * m, hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(hipStreamSynchronize(c->stream));
    }
    return ZKV_OK;
}

// ------------------------------------------------------------------ diagnostics: multiplication-rate and issue-rate microbenchmarks
// shared driver of the two microbenchmarks: `issue` selects k_diag_issue (64 instructions per loop trip and lane) over k_diag_mulmod
// (four primitive calls per trip; kind 1 counts two multiplications per call)
static int run_diag(int device, bool issue, int kind, int waves_per_simd, uint32_t iters, double* per_s, double* shader_clock_ghz) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n <= 0) { (void)hipGetLastError(); return ZKV_ERR_NO_DEVICE; }
    if (device < 0 || device >= n || !device_is_gfx950(device)) return ZKV_ERR_NO_DEVICE;
    HIP_TRY(hipSetDevice(device));
    hipDeviceProp_t p;
    HIP_TRY(hipGetDeviceProperties(&p, device));
    const unsigned blocks = (unsigned)p.multiProcessorCount * 4u * (unsigned)waves_per_simd;      // one 64-lane workgroup per wave slot
    DevBuf<uint32_t> d_out; DevBuf<unsigned long long> d_clk;
    DevEvent e0, e1;
    float ms = 0;
    unsigned long long clk[2] = {0, 0};
    auto launch = [&](uint32_t it) { if (issue) launch_diag_issue(kind, blocks, it, d_out, d_clk, nullptr); else launch_diag_mulmod(kind, blocks, it, d_out, d_clk, nullptr); };
    auto measure = [&]() -> bool {
        if (d_out.alloc((size_t)blocks * 64 * 4) || d_clk.alloc(16) || e0.create() || e1.create()) return false;
        launch(iters / 8 + 1);                                                             // warm-up (code fetch, clocks)
        if (hipDeviceSynchronize() != hipSuccess || hipEventRecord(e0, nullptr) != hipSuccess) return false;
        launch(iters);
        return hipEventRecord(e1, nullptr) == hipSuccess && hipEventSynchronize(e1) == hipSuccess &&
               hipEventElapsedTime(&ms, e0, e1) == hipSuccess && hipMemcpy(clk, d_clk, 16, hipMemcpyDeviceToHost) == hipSuccess;
    };
    if (!measure()) { (void)hipGetLastError(); return ZKV_ERR_HIP; }
    *per_s = (double)blocks * 64.0 * (issue ? 64.0 : 4.0 * (kind == 1 ? 2.0 : 1.0)) * (double)iters / ((double)ms * 1e-3);
    if (shader_clock_ghz) *shader_clock_ghz = clk[1] ? 0.1 * (double)clk[0] / (double)clk[1] : 0.0;     // s_memrealtime ticks at 100 MHz
    return ZKV_OK;
}
ZKV_EXPORT int zkv_diag_mulmod_rate(int device, int kind, int waves_per_simd, uint32_t iters, double* mulmods_per_s, double* shader_clock_ghz) {
    if (kind < 0 || kind > 4 || waves_per_simd < 1 || waves_per_simd > 8 || !iters || !mulmods_per_s) return ZKV_ERR_INVALID_ARG;
    return run_diag(device, false, kind, waves_per_simd, iters, mulmods_per_s, shader_clock_ghz);
}
ZKV_EXPORT int zkv_diag_issue_rate(int device, int kind, int waves_per_simd, uint32_t iters, double* lane_instr_per_s, double* shader_clock_ghz) {
    if (kind < 0 || kind > 2 || waves_per_simd < 1 || waves_per_simd > 8 || !iters || !lane_instr_per_s) return ZKV_ERR_INVALID_ARG;
    return run_diag(device, true, kind, waves_per_simd, iters, lane_instr_per_s, shader_clock_ghz);
}

// Known-answer harness of the arithmetic primitives (zkv_selftest.h): every argument is checked here, before anything is allocated or
// launched; the batch is padded to whole wavefronts (lane pairs, 16-lane groups) with zero operands whose results are discarded.
ZKV_EXPORT int zkv_diag_primitive(int device, int mapping, int op, size_t n, const uint32_t* in, uint32_t* out) {
    int iw = 0, ow = 0;
    if (!selftest_io(mapping, op, &iw, &ow) || n == 0 || n > ZKV_DIAG_PRIMITIVE_MAX_CASES || !in || !out) return ZKV_ERR_INVALID_ARG;
    int nd = 0;
    if (hipGetDeviceCount(&nd) != hipSuccess || nd <= 0) { (void)hipGetLastError(); return ZKV_ERR_NO_DEVICE; }
    if (device < 0 || device >= nd || !device_is_gfx950(device)) return ZKV_ERR_NO_DEVICE;
    HIP_TRY(hipSetDevice(device));
    const size_t per = (size_t)selftest_cases_per_wave(mapping), waves = (n + per - 1) / per, padded = waves * per;
    DevBuf<uint32_t> d_in, d_out;
    if (d_in.alloc(padded * (size_t)iw * 4) || d_out.alloc(padded * (size_t)ow * 4)) return ZKV_ERR_OOM;
    bool ok = hipMemset(d_in, 0, padded * (size_t)iw * 4) == hipSuccess && hipMemcpy(d_in, in, n * (size_t)iw * 4, hipMemcpyHostToDevice) == hipSuccess;
    if (ok) {
        if (mapping == 0) launch_selftest_lane(op, (unsigned)waves, d_in, d_out, nullptr);
        else launch_selftest_pair(mapping, op, (unsigned)waves, d_in, d_out, nullptr);
        ok = hipGetLastError() == hipSuccess && hipDeviceSynchronize() == hipSuccess &&
             hipMemcpy(out, d_out, n * (size_t)ow * 4, hipMemcpyDeviceToHost) == hipSuccess;
    }
    if (!ok) { (void)hipGetLastError(); return ZKV_ERR_HIP; }
    return ZKV_OK;
}

// The line steps of k_miller2 as column sums (zkv_diag_line_steps.h; selftest_line_sums): checked and padded like zkv_diag_primitive.
static_assert(ZKV_DIAG_LINE_STEPS_IN == 192 && ZKV_DIAG_LINE_STEPS_OUT == 624, "zkv_diag_line_steps.h documents the rows of selftest_line_sums");
ZKV_EXPORT int zkv_diag_line_steps(int device, size_t n, const uint32_t* in, uint32_t* out) {
    if (n == 0 || n > ZKV_DIAG_PRIMITIVE_MAX_CASES || !in || !out) return ZKV_ERR_INVALID_ARG;
    int nd = 0;
    if (hipGetDeviceCount(&nd) != hipSuccess || nd <= 0) { (void)hipGetLastError(); return ZKV_ERR_NO_DEVICE; }
    if (device < 0 || device >= nd || !device_is_gfx950(device)) return ZKV_ERR_NO_DEVICE;
    HIP_TRY(hipSetDevice(device));
    const size_t iw = ZKV_DIAG_LINE_STEPS_IN, ow = ZKV_DIAG_LINE_STEPS_OUT, waves = (n + 31) / 32, padded = waves * 32;
    DevBuf<uint32_t> d_in, d_out;
    if (d_in.alloc(padded * iw * 4) || d_out.alloc(padded * ow * 4)) return ZKV_ERR_OOM;
    bool ok = hipMemset(d_in, 0, padded * iw * 4) == hipSuccess && hipMemcpy(d_in, in, n * iw * 4, hipMemcpyHostToDevice) == hipSuccess;
    if (ok) {
        launch_selftest_line_sums((unsigned)waves, d_in, d_out, nullptr);
        ok = hipGetLastError() == hipSuccess && hipDeviceSynchronize() == hipSuccess &&
             hipMemcpy(out, d_out, n * ow * 4, hipMemcpyDeviceToHost) == hipSuccess;
    }
    if (!ok) { (void)hipGetLastError(); return ZKV_ERR_HIP; }
    return ZKV_OK;
}

// ------------------------------------------------------------------ zkv_diag_prep.h: what PREP stored for the vk_x stage (TEST ONLY)
static_assert(ZKV_DIAG_PREP_SIGNALS == MAX_VAR, "zkv_diag_prep.h documents MAX_VAR signal rows");
ZKV_EXPORT int zkv_diag_prep_signals(zkv_ctx* c, size_t n, uint32_t* signals, uint32_t* flags) {
    if (!c || !signals || !flags || n == 0) return ZKV_ERR_INVALID_ARG;
    if (is_sharded(c) || (c->vm != ZKV_VM_RISC0 && c->vm != ZKV_VM_SP1) || c->agg_on) return ZKV_ERR_INVALID_ARG;
    int nd = 0;
    if (hipGetDeviceCount(&nd) != hipSuccess || nd <= 0) { (void)hipGetLastError(); return ZKV_ERR_NO_DEVICE; }
    if (c->device < 0 || c->device >= nd || !device_is_gfx950(c->device)) return ZKV_ERR_NO_DEVICE;
    std::lock_guard<std::mutex> lk(c->mu);
    if (!c->dev_ready || !c->ws.prep || n > c->last_chunk_n || n > c->ws.cap) return ZKV_ERR_INVALID_ARG;
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(hipDeviceSynchronize());                         // the call may have run on a stream of the caller's
    const size_t rows = (size_t)8 * MAX_VAR;
    std::vector<uint32_t> t(rows * n);
    HIP_TRY(hipMemcpy2D(t.data(), 4 * n, c->ws.prep + (size_t)64 * c->ws.cap, 4 * c->ws.cap, 4 * n, rows, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(flags, c->ws.flags, 4 * n, hipMemcpyDeviceToHost));
    for (size_t j = 0; j < n; j++)
        for (size_t r = 0; r < rows; r++) signals[j * rows + r] = t[r * n + j];
    return ZKV_OK;
}

// ------------------------------------------------------------------ shared
ZKV_EXPORT int zkv_ctx_vm(const zkv_ctx* c) { return c ? c->vm : ZKV_ERR_INVALID_ARG; }
ZKV_EXPORT int zkv_ctx_set_lanes_per_proof(zkv_ctx* c, int lanes) {
    if (!c || (lanes != 0 && lanes != 2 && lanes != 16 && lanes != 64 && lanes != 128)) return ZKV_ERR_INVALID_ARG;
    if (is_sharded(c)) { for (auto* k : c->shards) { const int rc = zkv_ctx_set_lanes_per_proof(k, lanes); if (rc != ZKV_OK) return rc; } return ZKV_OK; }
    if (c->vm == ZKV_VM_MIXED) {                         // the two verifiers behind the tag run the stages
        for (auto* k : c->kid) { const int rc = zkv_ctx_set_lanes_per_proof(k, lanes); if (rc != ZKV_OK) return rc; }
    }
    if (c->vm == ZKV_VM_RISC0_SETINCL) { const int rc = zkv_ctx_set_lanes_per_proof(c->kid[0], lanes); if (rc != ZKV_OK) return rc; }   // the root jobs run there
    if (c->vm == ZKV_VM_RISC0_ROUTER && c->kid[0]) { const int rc = zkv_ctx_set_lanes_per_proof(c->kid[0], lanes); if (rc != ZKV_OK) return rc; }   // the built-in group
    for (auto* k : c->gw_route) { if (!k) continue; const int rc = zkv_ctx_set_lanes_per_proof(k, lanes); if (rc != ZKV_OK) return rc; }
    if (c->gw_group) { const int rc = zkv_ctx_set_lanes_per_proof(c->gw_group, lanes); if (rc != ZKV_OK) return rc; }
    std::lock_guard<std::mutex> lk(c->mu);
    c->lanes = lanes;
    return ZKV_OK;
}
// Diagnostics of the GT tables (zkv_gt.h; include/zkv_diag_gt.h).  info: {built, windows of signal 0, of signal 1, table bytes, build time in
// microseconds, build attempted}.  read: the 96 words of one entry in full Fp12 form (Montgomery form, R = 2^261, values below 2p; g0 g1 g2 h0 h1
// h2, (c0, c1) each; rebuilt from the stored torus value, k_gt_diag_expand) -- signal 0 / 1, window, digit magnitude d = 1 .. 2^19 --, or with
// signal < 0 the folded Miller constant as stored.
ZKV_EXPORT int zkv_diag_gt_info(zkv_ctx* c, uint64_t* out6) {
    if (!c || !out6) return ZKV_ERR_INVALID_ARG;
    std::lock_guard<std::mutex> lk(c->mu);
    out6[0] = c->gt.tab ? 1 : 0; out6[1] = c->gt.nw[0]; out6[2] = c->gt.nw[1]; out6[3] = c->gt_bytes;
    out6[4] = (uint64_t)(c->gt_build_ms * 1000.0f); out6[5] = c->gt_tried ? 1 : 0;
    return ZKV_OK;
}
ZKV_EXPORT int zkv_diag_gt_read(zkv_ctx* c, int signal, uint32_t window, uint32_t d, uint32_t* out96) {
    if (!c || !out96) return ZKV_ERR_INVALID_ARG;
    std::lock_guard<std::mutex> lk(c->mu);
    if (!c->gt.tab) return ZKV_ERR_INVALID_ARG;
    if (hipSetDevice(c->device) != hipSuccess) return ZKV_ERR_HIP;
    const uint32_t* src = c->gt.mconst;
    if (signal >= 0) {
        if (signal >= (int)GT_MAX_SIG || window >= c->gt.nw[signal] || d < 1 || d > GT_ROW_ENTRIES) return ZKV_ERR_INVALID_ARG;
        src = c->gt.tab + gt_row_word((signal ? c->gt.nw[0] : 0u) + window) + gt_entry_offset(d) / 4;
    }
    if (signal < 0) { HIP_TRY(hipMemcpy(out96, src, sizeof(uint32_t) * GT_ENTRY_WORDS, hipMemcpyDeviceToHost)); return ZKV_OK; }
    // an entry is stored as its affine torus value a (zkv_gt.h): the full Fp12 is reconstructed from it on the device
    DevBuf<uint32_t> d_out;
    HIP_TRY(d_out.alloc(sizeof(uint32_t) * GT_ENTRY_WORDS));
    launch_gt_diag_expand(src, d_out, c->stream);
    const bool ok = hipGetLastError() == hipSuccess && hipStreamSynchronize(c->stream) == hipSuccess &&
                    hipMemcpy(out96, d_out, sizeof(uint32_t) * GT_ENTRY_WORDS, hipMemcpyDeviceToHost) == hipSuccess;
    if (!ok) { (void)hipGetLastError(); return ZKV_ERR_HIP; }
    return ZKV_OK;
}
// cache: {valid entries, insertions so far, entries the cache holds} of the walk-prefix cache; all 0 for a context without one.
ZKV_EXPORT int zkv_diag_gt_cache(zkv_ctx* c, uint64_t* out3) {
    if (!c || !out3) return ZKV_ERR_INVALID_ARG;
    std::lock_guard<std::mutex> lk(c->mu);
    out3[0] = out3[1] = out3[2] = 0;
    if (!c->gt.cache) return ZKV_OK;
    if (hipSetDevice(c->device) != hipSuccess) return ZKV_ERR_HIP;
    uint32_t head[4 + GT_CACHE_ENTRIES];
    if (hipDeviceSynchronize() != hipSuccess || hipMemcpy(head, c->gt.cache, sizeof head, hipMemcpyDeviceToHost) != hipSuccess) { (void)hipGetLastError(); return ZKV_ERR_HIP; }
    for (uint32_t e = 0; e < GT_CACHE_ENTRIES; e++) out3[0] += head[4 + e] ? 1 : 0;
    out3[1] = head[1]; out3[2] = head[2];
    return ZKV_OK;
}
// product: what k_finalexp2's table walk makes of given scalars.  The n proofs get the Miller value 1 (k_gt_diag_seed), so the kernel's
// program exponentiates 1 to 1, the walk carries u with M = u / conj(u) over the selected rows and leaves u in the slot TMP (slot 8 of
// ws.fe); M is formed from it (k_gt_diag_ratio, one inversion per proof) and read back.  The kernel and its launch are the ones the verify
// path uses.
ZKV_EXPORT int zkv_diag_gt_product(zkv_ctx* c, size_t n, const uint32_t* scalars, uint32_t* out) {
    if (!c || !n || !scalars || !out) return ZKV_ERR_INVALID_ARG;
    std::lock_guard<std::mutex> lk(c->mu);
    if (!c->gt.tab || n > c->ws.cap) return ZKV_ERR_INVALID_ARG;
    for (size_t i = 0; i < n; i++) for (uint32_t sig = 0; sig < GT_MAX_SIG; sig++) {        // below 2^(20 nw - 1): the top window takes the last carry
        const uint32_t top = GT_WINDOW_BITS * c->gt.nw[sig] - 1u;
        for (uint32_t b = top; b < 256; b++) if ((scalars[(i * GT_MAX_SIG + sig) * 8 + (b >> 5)] >> (b & 31u)) & 1u) return ZKV_ERR_INVALID_ARG;
    }
    if (hipSetDevice(c->device) != hipSuccess) return ZKV_ERR_HIP;
    int rc = order_after_previous(c, c->stream);
    if (rc != ZKV_OK) return rc;
    constexpr size_t SW = 8 * GT_MAX_SIG;
    std::vector<uint32_t> rows(SW * n), res((size_t)GT_ENTRY_WORDS * n);
    for (size_t i = 0; i < n; i++) for (size_t k = 0; k < SW; k++) rows[k * n + i] = scalars[i * SW + k];
    DevBuf<uint8_t> d_st;
    DevBuf<uint32_t> d_m;                                        // M and the scratch of k_gt_diag_ratio, 96 n words each
    HIP_TRY(d_st.alloc(n));
    HIP_TRY(d_m.alloc(sizeof(uint32_t) * 2 * GT_ENTRY_WORDS * n));
    const size_t cap = c->ws.cap;
    bool ok = hipMemcpy2DAsync(c->ws.prep + 64 * cap, cap * 4, rows.data(), n * 4, n * 4, SW, hipMemcpyHostToDevice, c->stream) == hipSuccess;
    if (ok) {
        launch_gt_diag_seed(n, c->ws, c->stream);
        launch_gt_cache(n, c->ws, c->stream, c->gt);               // the stages of a verify call: the cached path is what is read back
        launch_finalexp2(n, c->ws, d_st, c->stream, c->gt);
        launch_gt_diag_ratio(n, c->ws.fe + (size_t)(96 * 6) * cap, cap, d_m, d_m + (size_t)GT_ENTRY_WORDS * n, c->stream);
        ok = hipGetLastError() == hipSuccess &&
             hipMemcpyAsync(res.data(), d_m, sizeof(uint32_t) * GT_ENTRY_WORDS * n, hipMemcpyDeviceToHost, c->stream) == hipSuccess &&
             hipStreamSynchronize(c->stream) == hipSuccess;
    }
    if (!ok) { (void)hipGetLastError(); return ZKV_ERR_HIP; }
    for (size_t i = 0; i < n; i++) for (size_t k = 0; k < GT_ENTRY_WORDS; k++) out[i * GT_ENTRY_WORDS + k] = res[k * n + i];
    return ZKV_OK;
}
// The keyed group of a gateway or router (gw_group, a Groth16 key set): its secret is derived from the front end's seed as the routes'
// are -- SHA-256(seed | index), with index 255, which no route has -- or drawn from the operating system (seed = nullptr).
constexpr uint8_t AGG_GROUP_SEED_INDEX = 255;
ZKV_EXPORT int zkv_ctx_set_aggregate_check(zkv_ctx* c, int enable, const uint8_t* seed32);
static int set_group_aggregate_check(zkv_ctx* group, int enable, const uint8_t* seed) {
    if (!enable || !seed) return zkv_ctx_set_aggregate_check(group, enable, nullptr);
    uint8_t buf[33], sk[32];
    memcpy(buf, seed, 32); buf[32] = AGG_GROUP_SEED_INDEX;
    host::sha256_host(buf, 33, sk);
    const int rc = zkv_ctx_set_aggregate_check(group, enable, sk);
    { volatile uint8_t* w = sk; for (int i = 0; i < 32; i++) w[i] = 0; }
    { volatile uint8_t* w = buf; for (int i = 0; i < 33; i++) w[i] = 0; }
    return rc;
}
// Aggregate check on / off (zkv_agg.h).  seed32 = nullptr draws the 32 secret bytes from the operating system.
ZKV_EXPORT int zkv_ctx_set_aggregate_check(zkv_ctx* c, int enable, const uint8_t* seed32) {
    if (!c || (enable != 0 && enable != 1 && enable != 16 && enable != 32 && enable != 64 && enable != 128 && enable != 256)) return ZKV_ERR_INVALID_ARG;
    uint8_t seed[32];
    if (enable) {
        if (seed32) memcpy(seed, seed32, 32);
        else if (getrandom(seed, 32, 0) != 32) return ZKV_ERR_INVALID_ARG;
    }
    if (is_sharded(c)) {                                 // every shard its own seed, derived from this one (or drawn afresh)
        for (size_t k = 0; k < c->shards.size(); k++) {
            uint8_t sk[32];
            if (enable && seed32) { uint8_t buf[36]; memcpy(buf, seed, 32); buf[32] = (uint8_t)(k >> 24); buf[33] = (uint8_t)(k >> 16); buf[34] = (uint8_t)(k >> 8); buf[35] = (uint8_t)k; host::sha256_host(buf, 36, sk); }
            const int rc = zkv_ctx_set_aggregate_check(c->shards[k], enable, enable && seed32 ? sk : nullptr);
            { volatile uint8_t* w = sk; for (int i = 0; i < 32; i++) w[i] = 0; }
            if (rc != ZKV_OK) return rc;
        }
        return ZKV_OK;
    }
    if (c->vm == ZKV_VM_MIXED || c->vm == ZKV_VM_SP1_GATEWAY) {
        const size_t nk = c->vm == ZKV_VM_MIXED ? 2 : c->gw_route.size();
        for (size_t k = 0; k < nk; k++) {
            if (c->vm == ZKV_VM_SP1_GATEWAY && !c->gw_route[k]) continue;      // a keyed route: its group follows the loop
            uint8_t sk[32];
            if (enable && seed32) { uint8_t buf[33]; memcpy(buf, seed, 32); buf[32] = (uint8_t)k; host::sha256_host(buf, 33, sk); }
            const int rc = zkv_ctx_set_aggregate_check(c->vm == ZKV_VM_MIXED ? c->kid[k] : c->gw_route[k], enable, enable && seed32 ? sk : nullptr);
            { volatile uint8_t* w = sk; for (int i = 0; i < 32; i++) w[i] = 0; }
            if (rc != ZKV_OK) return rc;
        }
        if (c->vm == ZKV_VM_SP1_GATEWAY && c->gw_group) {   // the keyed group: a secret of its own, under an index no route has
            const int rc = set_group_aggregate_check(c->gw_group, enable, seed32 ? seed : nullptr);
            if (rc != ZKV_OK) return rc;
        }
        return ZKV_OK;
    }
    if (c->vm == ZKV_VM_RISC0_ROUTER) {                  // the built-in group with the seed itself, the keyed group with one derived from it
        int rc = c->kid[0] ? zkv_ctx_set_aggregate_check(c->kid[0], enable, enable && seed32 ? seed : nullptr) : ZKV_OK;
        if (rc == ZKV_OK && c->gw_group) rc = set_group_aggregate_check(c->gw_group, enable, seed32 ? seed : nullptr);
        { volatile uint8_t* w = seed; for (int i = 0; i < 32; i++) w[i] = 0; }
        return rc;
    }
    if (c->vm != ZKV_VM_RISC0 && c->vm != ZKV_VM_RISC0_SET && c->vm != ZKV_VM_SP1 && c->vm != ZKV_VM_GROTH16 && c->vm != ZKV_VM_SP1_PLONK &&
        c->vm != ZKV_VM_GROTH16_SET && c->vm != ZKV_VM_PLONK && c->vm != ZKV_VM_PLONK_SET)
        return enable ? ZKV_ERR_INVALID_ARG : ZKV_OK;
    {
        std::lock_guard<std::mutex> lk(c->mu);
        c->agg_on = enable != 0;
        if (enable) {
            c->agg_auto = enable == 1; c->agg_sub = enable == 1 ? 32u : (uint32_t)enable;
            c->agg_resnap = c->dev_ready;                       // counters of earlier runs (other sizes) are not this setting's evidence; a fresh context starts from zero
            if (!c->dev_ready) c->agg_seen[0] = c->agg_seen[1] = 0;
            c->agg_pause = c->agg_pause_len = 0;
            c->agg_os_seed = seed32 == nullptr; c->agg_key_age = 0;
            for (int i = 0; i < 8; i++) c->agg_seed.w[i] = be32_of(seed + 4 * i);
        }
    }
    volatile uint8_t* wipe = seed;                              // the secret does not stay on this stack
    for (int i = 0; i < 32; i++) wipe[i] = 0;
    return ZKV_OK;
}
// {sub-batches checked, sub-batches that failed and were verified proof by proof} since the context was set up; the calling thread
// must have synchronised with the batches it wants counted.
ZKV_EXPORT int zkv_ctx_aggregate_counters(zkv_ctx* c, uint64_t out[2]) {
    if (!c || !out) return ZKV_ERR_INVALID_ARG;
    out[0] = out[1] = 0;
    if (is_sharded(c) || c->vm == ZKV_VM_MIXED || c->vm == ZKV_VM_SP1_GATEWAY) {
        const size_t nk = is_sharded(c) ? c->shards.size() : c->vm == ZKV_VM_MIXED ? 2 : c->gw_route.size();
        for (size_t k = 0; k < nk; k++) {
            if (!is_sharded(c) && c->vm == ZKV_VM_SP1_GATEWAY && !c->gw_route[k]) continue;
            uint64_t o[2];
            const int rc = zkv_ctx_aggregate_counters(is_sharded(c) ? c->shards[k] : c->vm == ZKV_VM_MIXED ? c->kid[k] : c->gw_route[k], o);
            if (rc != ZKV_OK) return rc;
            out[0] += o[0]; out[1] += o[1];
        }
        if (!is_sharded(c) && c->vm == ZKV_VM_SP1_GATEWAY && c->gw_group) {      // the keyed group's
            uint64_t o[2];
            const int rc = zkv_ctx_aggregate_counters(c->gw_group, o);
            if (rc != ZKV_OK) return rc;
            out[0] += o[0]; out[1] += o[1];
        }
        return ZKV_OK;
    }
    if (c->vm == ZKV_VM_RISC0_ROUTER) {                  // the built-in group's and the keyed group's
        for (zkv_ctx* k : {c->kid[0], c->gw_group}) {
            if (!k) continue;
            uint64_t o[2];
            const int rc = zkv_ctx_aggregate_counters(k, o);
            if (rc != ZKV_OK) return rc;
            out[0] += o[0]; out[1] += o[1];
        }
        return ZKV_OK;
    }
    std::lock_guard<std::mutex> lk(c->mu);
    if (!c->dev_ready || !c->d_agg_cnt) return ZKV_OK;
    HIP_TRY(hipSetDevice(c->device));
    unsigned long long v[2];
    HIP_TRY(hipMemcpy(v, c->d_agg_cnt, sizeof v, hipMemcpyDeviceToHost));
    out[0] = v[0]; out[1] = v[1];
    return ZKV_OK;
}
ZKV_EXPORT int zkv_diag_device_memory(uint64_t out[2]) {
    if (!out) return ZKV_ERR_INVALID_ARG;
    out[0] = g_dev_live_allocs.load(std::memory_order_relaxed); out[1] = g_dev_live_bytes.load(std::memory_order_relaxed);
    return ZKV_OK;
}
ZKV_EXPORT int zkv_diag_wait_faults(int device, uint64_t* out) {
    if (!out) return ZKV_ERR_INVALID_ARG;
    *out = 0;
    if (device < 0 || device >= zkv_device_count()) return ZKV_ERR_NO_DEVICE;
    HIP_TRY(hipSetDevice(device));
    unsigned long long v = 0;
    if (zkv::read_wait_faults(&v) != 0) return ZKV_ERR_HIP;
    unsigned long long g = 0;                            // the key-set Miller kernel counts its own (k_gset_pair.hip)
    if (zkv::read_gset_wait_faults(&g) != 0) return ZKV_ERR_HIP;
    *out = v + g;
    return ZKV_OK;
}
ZKV_EXPORT int zkv_ctx_shard_peer_access(zkv_ctx* c, size_t shard) {
    if (!c || !is_sharded(c) || shard >= c->sh.size()) return ZKV_ERR_INVALID_ARG;
    std::lock_guard<std::mutex> lk(c->mu);
    return c->sh[shard].peer;
}
ZKV_EXPORT int zkv_host_register(void* ptr, size_t bytes) {
    if (!ptr || !bytes) return ZKV_ERR_INVALID_ARG;
    if (zkv_device_count() < 1) return ZKV_ERR_NO_DEVICE;
    HIP_TRY(hipHostRegister(ptr, bytes, hipHostRegisterPortable));
    return ZKV_OK;
}
ZKV_EXPORT int zkv_host_unregister(void* ptr) {
    if (!ptr) return ZKV_ERR_INVALID_ARG;
    if (zkv_device_count() < 1) return ZKV_ERR_NO_DEVICE;
    HIP_TRY(hipHostUnregister(ptr));
    return ZKV_OK;
}
ZKV_EXPORT int zkv_ctx_reserve(zkv_ctx* c, size_t n) {
    if (!c) return ZKV_ERR_INVALID_ARG;
    if (is_sharded(c)) {                                 // every shard for its share of an n-proof batch
        const size_t used = shards_used(c, n ? n : 1);
        for (size_t k = 0; k < used; k++) { size_t lo, hi; shard_range(n ? n : 1, used, k, &lo, &hi); const int rc = zkv_ctx_reserve(c->shards[k], hi - lo); if (rc != ZKV_OK) return rc; }
        return ZKV_OK;
    }
    if (c->vm == ZKV_VM_MIXED) {                         // either VM may own the whole batch
        int rc = zkv_ctx_reserve(c->kid[0], n);
        if (rc == ZKV_OK) rc = zkv_ctx_reserve(c->kid[1], n);
        if (rc != ZKV_OK) return rc;
        std::lock_guard<std::mutex> lk(c->mu);
        return ctx_device_init(c);
    }
    if (c->vm == ZKV_VM_RISC0_SETINCL) {                 // the inner verifier for n root jobs; the hash workspace grows with the calls
        const int rc = zkv_ctx_reserve(c->kid[0], n);
        if (rc != ZKV_OK) return rc;
        std::lock_guard<std::mutex> lk(c->mu);
        return ctx_device_init(c);
    }
    if (c->vm == ZKV_VM_RISC0_ROUTER) {                  // either group may own the whole batch
        if (c->kid[0]) { const int rc = zkv_ctx_reserve(c->kid[0], n); if (rc != ZKV_OK) return rc; }
        if (c->gw_group) { const int rc = zkv_ctx_reserve(c->gw_group, n); if (rc != ZKV_OK) return rc; }
        std::lock_guard<std::mutex> lk(c->mu);
        return ctx_device_init(c);
    }
    if (c->vm == ZKV_VM_SP1_GATEWAY) {                   // any route may own the whole batch
        for (auto* k : c->gw_route) { if (!k) continue; const int rc = zkv_ctx_reserve(k, n); if (rc != ZKV_OK) return rc; }
        if (c->gw_group) { const int rc = zkv_ctx_reserve(c->gw_group, n); if (rc != ZKV_OK) return rc; }
        std::lock_guard<std::mutex> lk(c->mu);
        return ctx_device_init(c);
    }
    std::lock_guard<std::mutex> lk(c->mu);
    size_t chunk;
    if (c->vm == ZKV_VM_PLONK) return plonk_ready(c, n, &chunk);
    return c->vm == ZKV_VM_GROTH16 || c->vm == ZKV_VM_GROTH16_SET ? groth16_ready(c, n, &chunk) : ctx_ready(c, n);
}
ZKV_EXPORT int zkv_ctx_synchronize(zkv_ctx* c) {
    if (!c) return ZKV_ERR_INVALID_ARG;
    if (is_sharded(c)) {                                 // every shard's device, and the shards' own streams (status copies back to the source GPU)
        for (size_t k = 0; k < c->shards.size(); k++) {
            const int rc = zkv_ctx_synchronize(c->shards[k]);
            if (rc != ZKV_OK) return rc;
            if (c->sh[k].run) { HIP_TRY(hipSetDevice(c->shards[k]->device)); HIP_TRY(hipStreamSynchronize(c->sh[k].run)); }
        }
        return ZKV_OK;
    }
    // a mixed context has work in flight as soon as ANY of its three contexts is set up (an all-SP1 batch never touches the RISC Zero child)
    bool any = c->dev_ready || ((c->vm == ZKV_VM_MIXED || c->vm == ZKV_VM_RISC0_SETINCL || c->vm == ZKV_VM_RISC0_ROUTER) && ((c->kid[0] && c->kid[0]->dev_ready) || (c->kid[1] && c->kid[1]->dev_ready)));
    for (auto* k : c->gw_route) any = any || (k && k->dev_ready);
    any = any || (c->gw_group && c->gw_group->dev_ready);
    if (!any) return ZKV_OK;
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(hipDeviceSynchronize());
    return ZKV_OK;
}
ZKV_EXPORT int zkv_ctx_last_stage_ms(zkv_ctx* c, float out_ms[5]) {
    if (!c || !out_ms) return ZKV_ERR_INVALID_ARG;
    if (is_sharded(c)) return zkv_ctx_last_stage_ms(c->shards[0], out_ms);          // shards run side by side: shard 0 stands for all
    if (c->vm == ZKV_VM_MIXED) {
        // the two sub-batches run one after the other: stage times add up.  Only the children that ran in the MOST RECENT mixed call
        // count (an unused child is either not set up or still holds the event times of an earlier batch).
        for (int i = 0; i < 5; i++) out_ms[i] = 0.0f;
        for (int k = 0; k < 2; k++) {
            if (!c->kid_ran[k]) continue;
            float a[5];
            const int rc = zkv_ctx_last_stage_ms(c->kid[k], a);
            if (rc != ZKV_OK) return rc;
            for (int i = 0; i < 5; i++) out_ms[i] += a[i];
        }
        return ZKV_OK;
    }
    if (c->vm == ZKV_VM_RISC0_SETINCL) {                 // [0]: k_setincl_hash of the last chunk; [1..4]: the inner verifier's stages of the last root jobs
        std::lock_guard<std::mutex> lk(c->mu);
        if (!c->dev_ready || !c->si_counts[0]) return ZKV_ERR_NO_DEVICE;
        float a[5] = {0, 0, 0, 0, 0};
        if (c->si_counts[1]) { const int rc = zkv_ctx_last_stage_ms(c->kid[0], a); if (rc != ZKV_OK) return rc; }
        HIP_TRY(hipSetDevice(c->device));
        HIP_TRY(hipEventSynchronize(c->ev[1]));
        HIP_TRY(hipEventElapsedTime(&out_ms[0], c->ev[0], c->ev[1]));
        for (int i = 1; i < 5; i++) out_ms[i] = a[i];
        return ZKV_OK;
    }
    if (c->vm == ZKV_VM_RISC0_ROUTER) {                  // the two groups run one after the other: stage times add up
        bool ran = false;
        for (int i = 0; i < 5; i++) out_ms[i] = 0.0f;
        for (int k = 0; k < 2; k++) {
            if (!c->kid_ran[k]) continue;
            float a[5];
            const int rc = zkv_ctx_last_stage_ms(k == 0 ? c->kid[0] : c->gw_group, a);
            if (rc != ZKV_OK) return rc;
            for (int i = 0; i < 5; i++) out_ms[i] += a[i];
            ran = true;
        }
        return ran ? ZKV_OK : ZKV_ERR_NO_DEVICE;
    }
    if (c->vm == ZKV_VM_SP1_GATEWAY) {                   // routes run one after the other, as the mixed context's children
        bool ran = false;
        for (int i = 0; i < 5; i++) out_ms[i] = 0.0f;
        bool group = false;                              // the keyed routes ran as one pass: their group counts once
        for (size_t k = 0; k < c->gw_route.size(); k++) {
            if (!c->gw_ran[k] || (!c->gw_route[k] && group)) continue;
            if (!c->gw_route[k]) group = true;
            float a[5];
            const int rc = zkv_ctx_last_stage_ms(c->gw_route[k] ? c->gw_route[k] : c->gw_group, a);
            if (rc != ZKV_OK) return rc;
            for (int i = 0; i < 5; i++) out_ms[i] += a[i];
            ran = true;
        }
        return ran ? ZKV_OK : ZKV_ERR_NO_DEVICE;
    }
    if (!c->dev_ready) return ZKV_ERR_NO_DEVICE;
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(hipEventSynchronize(c->ev[5]));
    for (int i = 0; i < 5; i++) HIP_TRY(hipEventElapsedTime(&out_ms[i], c->ev[i], c->ev[i + 1]));
    return ZKV_OK;
}
ZKV_EXPORT int zkv_status_abi_encode(int vm, uint8_t status, const uint8_t received[4], const uint8_t expected[4], uint8_t out[68]) {
    // keccak-256 selectors of the reference's Solidity custom errors
    static const uint8_t sel[5][4] = {{0, 0, 0, 0}, {0x43, 0x9c, 0xc0, 0xcd}, {0xf9, 0x2e, 0xe8, 0xa9}, {0x0d, 0xc1, 0x49, 0xf0}, {0xe3, 0xe9, 0x43, 0x26}};
    static const uint8_t mism[2][4] = {{0xb8, 0xb3, 0x8d, 0x4c}, {0x98, 0x80, 0x66, 0xa1}};
    if (vm == ZKV_VM_SP1_PLONK) vm = ZKV_VM_SP1;           // same ISp1Verifier errors
    if (!out || (vm != ZKV_VM_RISC0 && vm != ZKV_VM_SP1)) return ZKV_ERR_INVALID_ARG;
    if (status == ZKV_STATUS_OK) return 0;
    if (status == ZKV_STATUS_SELECTOR_MISMATCH) {
        if (!received || !expected) return ZKV_ERR_INVALID_ARG;
        memset(out, 0, 68);
        memcpy(out, mism[vm], 4); memcpy(out + 4, received, 4); memcpy(out + 36, expected, 4);
        return 68;
    }
    if (status > ZKV_STATUS_SELECTOR_MISMATCH) return ZKV_ERR_INVALID_ARG;
    memcpy(out, sel[status], 4);
    return 4;
}

// ------------------------------------------------------------------ RISC Zero set-inclusion receipts (zkv_risc0_set_inclusion.h)
// No reference counterpart: parity unpinned.  k_setincl.hip hashes the paths and forms the root jobs; the jobs run on the inner context.
constexpr size_t SETINCL_CHUNK = (size_t)1 << 20;
// Section 16's grouping rows in a chunk's record, as they are now (after their grows).
static void setgroup_chunk_view(const SetGroupMem& g, SetinclChunk* ch) {
    ch->stored = g.stored; ch->roots = g.roots; ch->rep = g.rep; ch->gslot = g.gslot; ch->claim_job = g.claim_job; ch->job_claim = g.job_claim;
    ch->counters = g.cnt;
}
// The rows of nj root jobs, grown, in a job record: records with lengths and inputs or, for a keyed inner verifier, proofs and signals.
// (Growing frees the old buffer, which waits for the device: the previous chunk's scatter has read its rows by then.)
static int setgroup_job_rows(SetGroupMem& g, size_t nj, bool keyed, SetinclJobs* jb) {
    const size_t rec = keyed ? 0 : nj, key = keyed ? nj : 0;
    const int rc = grow_all(g.rows, 260 * rec, g.lens, 4 * rec, g.ids, 32 * rec, g.jds, 32 * rec, g.proofs, 256 * key, g.signals, 160 * key, g.pre, key,
                            g.pre_recv, 4 * key, g.jst, nj, g.jrv, 4 * nj);
    if (rc != ZKV_OK) return rc;
    jb->rows = g.rows; jb->lens = g.lens; jb->ids = g.ids; jb->jds = g.jds; jb->st = g.jst; jb->rv = g.jrv;
    jb->proofs = g.proofs; jb->signals = g.signals; jb->pre = g.pre; jb->pre_recv = g.pre_recv;
    return ZKV_OK;
}

static void setincl_set_selector(const uint8_t id[32], uint8_t out[4]) {
    uint8_t tag[32], d[32];
    host::sha256_host((const uint8_t*)"risc0.SetInclusionReceiptVerifierParameters", 43, tag);
    host::tagged_struct(tag, id, 1, d);
    memcpy(out, d, 4);
}
static zkv_ctx* setincl_new(zkv_ctx* inner, const uint8_t control_root[32], const uint8_t control_id[32], const uint8_t id[32], int device) {
    if (!inner) return nullptr;
    zkv_ctx* c = new (std::nothrow) zkv_ctx();
    if (!c) { zkv_ctx_destroy(inner); return nullptr; }
    c->vm = ZKV_VM_RISC0_SETINCL; c->device = device; c->initialized = true;
    c->kid[0] = inner;
    host::risc0_consts(c->consts);
    host::split_digest(control_root, c->control_root_0, c->control_root_1);
    memcpy(c->control_id, control_id, 32);
    memcpy(c->si_id, id, 32);
    setincl_set_selector(id, c->si_set_sel);
    return c;
}
ZKV_EXPORT zkv_ctx* zkv_risc0_setincl_create(const uint8_t control_root[32], const uint8_t bn254_control_id[32], const uint8_t set_builder_image_id[32],
                                             int device) {
    if (!control_root || !bn254_control_id || !set_builder_image_id) return nullptr;
    zkv_ctx* c = setincl_new(zkv_risc0_ctx_create(control_root, bn254_control_id, device), control_root, bn254_control_id, set_builder_image_id, device);
    if (c) memcpy(c->si_root_sel, c->kid[0]->selector, 4);
    return c;
}
ZKV_EXPORT zkv_ctx* zkv_risc0_setincl_create_keyed(const uint8_t* vk_words, const uint8_t root_selector[4], const uint8_t control_root[32],
                                                   const uint8_t bn254_control_id[32], const uint8_t set_builder_image_id[32], int device) {
    if (!vk_words || !root_selector || !control_root || !bn254_control_id || !set_builder_image_id) return nullptr;
    zkv_ctx* c = setincl_new(zkv_groth16_ctx_create(vk_words, 6, ZKV_VM_RISC0, device), control_root, bn254_control_id, set_builder_image_id, device);
    if (c) { c->si_keyed = true; memcpy(c->si_root_sel, root_selector, 4); }
    return c;
}
ZKV_EXPORT int zkv_risc0_setincl_get_selector(const zkv_ctx* c, uint8_t out[4]) {
    if (!c || c->vm != ZKV_VM_RISC0_SETINCL) return ZKV_ERR_WRONG_CTX;
    if (!out) return ZKV_ERR_INVALID_ARG;
    memcpy(out, c->si_set_sel, 4);
    return ZKV_OK;
}
// position of `root` in the sorted table, *found = it is there
static size_t setincl_find(const zkv_ctx* c, const uint8_t root[32], bool* found) {
    size_t lo = 0, hi = c->si_roots.size() / 32;
    *found = false;
    while (lo < hi) {
        const size_t mid = (lo + hi) / 2;
        const int r = memcmp(root, c->si_roots.data() + 32 * mid, 32);
        if (r == 0) { *found = true; return mid; }
        if (r < 0) hi = mid; else lo = mid + 1;
    }
    return lo;
}
ZKV_EXPORT int zkv_risc0_setincl_has_root(zkv_ctx* c, const uint8_t root[32]) {
    if (!c || c->vm != ZKV_VM_RISC0_SETINCL) return ZKV_ERR_WRONG_CTX;
    if (!root) return ZKV_ERR_INVALID_ARG;
    std::lock_guard<std::mutex> lk(c->mu);
    bool found;
    (void)setincl_find(c, root, &found);
    return found ? 1 : 0;
}
// the five signals of V for (ID, sha256(ID || root)) in the keyed mode, 32-byte big-endian words (risc0/verifier.rs:128-144)
static void setincl_host_signals(const zkv_ctx* c, const uint8_t jd[32], uint8_t sig[160]) {
    uint32_t h[8];
    risc0_claim_digest(c->consts, c->si_id, jd, h);
    uint8_t d[32], lo[16], hi[16];
    for (int q = 0; q < 8; q++) be32_put(d + 4 * q, h[q]);
    host::split_digest(d, lo, hi);
    memset(sig, 0, 160);
    memcpy(sig + 16, c->control_root_0, 16); memcpy(sig + 48, c->control_root_1, 16);
    memcpy(sig + 80, lo, 16); memcpy(sig + 112, hi, 16);
    memcpy(sig + 128, c->control_id, 32);
}
ZKV_EXPORT int zkv_risc0_setincl_submit_root(zkv_ctx* c, const uint8_t root[32], const uint8_t* seal, size_t seal_len, uint8_t* status, uint8_t recv[4]) {
    if (!c || c->vm != ZKV_VM_RISC0_SETINCL) return ZKV_ERR_WRONG_CTX;
    if (!root || !status || (!seal && seal_len)) return ZKV_ERR_INVALID_ARG;
    uint8_t msg[64], jd[32], rv[4] = {0, 0, 0, 0}, st = ZKV_STATUS_VERIFICATION_FAILED;
    memcpy(msg, c->si_id, 32); memcpy(msg + 32, root, 32);
    host::sha256_host(msg, 64, jd);
    int rc = ZKV_OK;
    if (!c->si_keyed) rc = zkv_risc0_verify(c->kid[0], seal, seal_len, c->si_id, jd, &st, rv);
    else if (seal_len < 4) st = ZKV_STATUS_INVALID_PROOF_DATA;
    else if (memcmp(seal, c->si_root_sel, 4)) { st = ZKV_STATUS_SELECTOR_MISMATCH; memcpy(rv, seal, 4); }
    else if (seal_len != ZKV_SEAL_BYTES) st = ZKV_STATUS_INVALID_PROOF_DATA;
    else {
        uint8_t sig[160], v = 0;
        setincl_host_signals(c, jd, sig);
        rc = zkv_groth16_verify_batch(c->kid[0], 1, seal + 4, sig, &v);
        st = v ? ZKV_STATUS_OK : ZKV_STATUS_VERIFICATION_FAILED;
    }
    if (rc != ZKV_OK) return rc;
    *status = st;
    if (recv) memcpy(recv, rv, 4);
    if (st != ZKV_STATUS_OK) return ZKV_OK;
    std::lock_guard<std::mutex> lk(c->mu);
    bool found;
    const size_t at = setincl_find(c, root, &found);
    if (found) return ZKV_OK;
    if (c->si_roots.size() / 32 >= ZKV_SETINCL_MAX_ROOTS) return ZKV_ERR_INVALID_ARG;
    try { c->si_roots.insert(c->si_roots.begin() + 32 * at, root, root + 32); } catch (const std::bad_alloc&) { return ZKV_ERR_OOM; }
    c->si_dirty = true;
    return ZKV_OK;
}

// Everything device-resident.  d_b = nullptr: integrity.  d_slen = nullptr: every root seal is 260 bytes.  d_ridx = nullptr with diag: hash only.
// Synchronises `s` once per chunk (the job count).  The caller holds c->mu and has initialised the device.
static int run_setincl(zkv_ctx* c, size_t n, const uint8_t* d_a, const uint8_t* d_b, const uint8_t* d_paths, const uint32_t* d_poff, size_t n_sib,
                       const uint32_t* d_ridx, size_t m, const uint8_t* d_seals, const uint32_t* d_slen, uint8_t* d_status, uint8_t* d_recv, uint8_t* d_diag,
                       hipStream_t s) {
    int rc;
    const size_t cap = n < SETINCL_CHUNK ? n : SETINCL_CHUNK;
    SetGroupMem& g = c->m_si;
    if ((rc = grow_all(g.roots, 32 * cap, g.rep, 4 * (m + 1), g.gslot, 4 * (m + 1), g.claim_job, 4 * cap, g.job_claim, 4 * cap, g.cnt, 16,
                       g.stored, (size_t)32 * ZKV_SETINCL_MAX_ROOTS)) != ZKV_OK) return rc;
    if (c->si_dirty) {                                   // a root was submitted since the last call: nothing of this context is in flight after the wait
        HIP_TRY(hipDeviceSynchronize());
        if (!c->si_roots.empty()) HIP_TRY(hipMemcpy(g.stored, c->si_roots.data(), c->si_roots.size(), hipMemcpyHostToDevice));
        c->si_dirty = false;
    }
    if ((rc = order_after_previous(c, s)) != ZKV_OK) return rc;
    HIP_TRY(hipMemsetAsync(g.cnt, 0, 16, s));
    if (!d_diag) { c->si_counts[0] = n; c->si_counts[1] = 0; c->si_counts[2] = 0; }
    for (size_t base = 0; base < n; base += cap) {
        const size_t mc = n - base < cap ? n - base : cap;
        SetinclChunk ch;
        memset(&ch, 0, sizeof ch);
        ch.n = (uint32_t)mc; ch.m = (uint32_t)m; ch.n_siblings = (uint32_t)n_sib; ch.n_stored = (uint32_t)(c->si_roots.size() / 32);
        ch.in_a = d_a + 32 * base; ch.in_b = d_b ? d_b + 32 * base : nullptr;
        ch.paths = d_paths; ch.path_off = d_poff + base; ch.root_idx = d_ridx ? d_ridx + base : nullptr;
        ch.seals = d_seals; ch.seal_len = d_slen;
        for (int q = 0; q < 8; q++) ch.id_be[q] = be32_of(c->si_id + 4 * q);
        setgroup_chunk_view(g, &ch);
        ch.status = d_status ? d_status + base : nullptr; ch.recv = d_recv ? d_recv + 4 * base : nullptr;
        ch.diag_roots = d_diag ? d_diag + 32 * base : nullptr;
        if (d_diag) { launch_setincl_hash(ch, c->consts, s); HIP_TRY(hipGetLastError()); continue; }
        HIP_TRY(hipMemsetAsync(ch.rep, 0xFF, 4 * (m + 1), s));
        HIP_TRY(hipMemsetAsync(g.cnt, 0, 4, s));
        HIP_TRY(hipEventRecord(c->ev[0], s));                       // zkv_ctx_last_stage_ms [0]: the hash kernel of the last chunk
        launch_setincl_hash(ch, c->consts, s);
        HIP_TRY(hipEventRecord(c->ev[1], s));
        launch_setincl_group(ch, s);
        HIP_TRY(hipGetLastError());
        uint32_t nj = 0;
        HIP_TRY(hipMemcpyAsync(&nj, g.cnt, 4, hipMemcpyDeviceToHost, s));
        HIP_TRY(hipStreamSynchronize(s));
        if (nj > mc) return ZKV_ERR_HIP;
        c->si_counts[1] += nj;
        SetinclJobs jb;
        memset(&jb, 0, sizeof jb);
        jb.n_jobs = nj; jb.keyed = c->si_keyed ? 1u : 0u; jb.selector_be = be32_of(c->si_root_sel);
        if (nj) {
            if ((rc = setgroup_job_rows(g, nj, c->si_keyed, &jb)) != ZKV_OK) return rc;
            memcpy(jb.fixed[0] + 16, c->control_root_0, 16); memcpy(jb.fixed[1] + 16, c->control_root_1, 16); memcpy(jb.fixed[2], c->control_id, 32);
            launch_setincl_jobs(ch, jb, c->consts, s);
            HIP_TRY(hipGetLastError());
            if (c->si_keyed) rc = zkv_groth16_verify_batch_dev(c->kid[0], nj, jb.proofs, jb.signals, g.jst, s);
            else rc = run_records(c->kid[0], nj, jb.rows, jb.lens, jb.ids, jb.jds, nullptr, nullptr, nullptr, nullptr, g.jst, g.jrv, s);
            if (rc != ZKV_OK) return rc;
            HIP_TRY(hipSetDevice(c->device));
        }
        launch_setincl_scatter(ch, jb, s);
        HIP_TRY(hipGetLastError());
    }
    return mark_done(c, s);
}
static int setincl_dev_call(zkv_ctx* c, size_t n, const uint8_t* d_a, const uint8_t* d_b, const uint8_t* d_paths, const uint32_t* d_poff, size_t n_sib,
                            const uint32_t* d_ridx, size_t m, const uint8_t* d_seals, uint8_t* d_status, uint8_t* d_recv, void* stream) {
    if (!c || c->vm != ZKV_VM_RISC0_SETINCL) return ZKV_ERR_WRONG_CTX;
    if (n && (!d_a || !d_poff || !d_ridx || !d_status || (n_sib && !d_paths) || (m && !d_seals))) return ZKV_ERR_INVALID_ARG;
    if (!n) return ZKV_OK;
    if (n > 0xFFFFFFF0u || m > ((size_t)1 << 24) || n_sib > 0xFFFFFFFFu) return ZKV_ERR_INVALID_ARG;
    std::lock_guard<std::mutex> lk(c->mu);
    int rc = ctx_device_init(c);
    if (rc != ZKV_OK) return rc;
    return run_setincl(c, n, d_a, d_b, d_paths, d_poff, n_sib, d_ridx, m, d_seals, nullptr, d_status, d_recv, nullptr, stream ? (hipStream_t)stream : c->stream);
}
ZKV_EXPORT int zkv_risc0_setincl_verify_batch_dev(zkv_ctx* c, size_t n, const uint8_t* d_image_ids, const uint8_t* d_journal_digests, const uint8_t* d_path_blob,
                                                  const uint32_t* d_path_off, size_t n_siblings, const uint32_t* d_root_idx, size_t m,
                                                  const uint8_t* d_root_seals, uint8_t* d_status, uint8_t* d_recv, void* stream) {
    return setincl_dev_call(c, n, d_image_ids, d_journal_digests, d_path_blob, d_path_off, n_siblings, d_root_idx, m, d_root_seals, d_status, d_recv, stream);
}
// Host buffers: staged whole, one device-resident run, statuses copied back.  in_b = nullptr: integrity.  diag_out: hash only (blob_shift
// places the path blob off its aligned base).
static int setincl_host_call(zkv_ctx* c, size_t n, const uint8_t* in_a, const uint8_t* in_b, bool integrity, const uint8_t* path_blob, const uint32_t* path_off,
                             const uint32_t* root_idx, size_t m, const uint8_t* seal_blob, const uint64_t* seal_off, uint8_t* status, uint8_t* recv,
                             uint8_t* diag_out, size_t blob_shift) {
    if (!c || c->vm != ZKV_VM_RISC0_SETINCL) return ZKV_ERR_WRONG_CTX;
    if (n && (!in_a || (!integrity && !in_b) || !path_off || (!diag_out && (!root_idx || !status)) || (m && (!seal_blob || !seal_off)))) return ZKV_ERR_INVALID_ARG;
    if (!n) return ZKV_OK;
    if (n > 0xFFFFFFF0u || m > ((size_t)1 << 24) || blob_shift > 31 || (m && !offsets_ok(seal_off, m))) return ZKV_ERR_INVALID_ARG;
    for (size_t i = 0; i < n; i++) if (path_off[i + 1] < path_off[i]) return ZKV_ERR_INVALID_ARG;
    const uint32_t o0 = path_off[0];
    const size_t n_sib = path_off[n] - o0;
    if (n_sib && !path_blob) return ZKV_ERR_INVALID_ARG;
    std::lock_guard<std::mutex> lk(c->mu);
    int rc = ctx_device_init(c);
    if (rc != ZKV_OK) return rc;
    std::vector<uint32_t> po, sl;
    std::vector<uint8_t> rows;
    try {
        po.assign(path_off, path_off + n + 1);
        for (auto& v : po) v -= o0;
        sl.resize(m + 1); rows.assign((size_t)ZKV_SEAL_BYTES * (m + 1), 0);
        for (size_t j = 0; j < m; j++) {
            const uint64_t len = seal_off[j + 1] - seal_off[j];
            sl[j] = len > 0xFFFFFFFEu ? 0xFFFFFFFEu : (uint32_t)len;
            memcpy(rows.data() + ZKV_SEAL_BYTES * j, seal_blob + seal_off[j], len < ZKV_SEAL_BYTES ? (size_t)len : (size_t)ZKV_SEAL_BYTES);
        }
    } catch (const std::bad_alloc&) { return ZKV_ERR_OOM; }
    SetInclMem& si = c->m_si;
    if ((rc = grow_all(si.h_a, 32 * n, si.h_b, integrity ? 0 : 32 * n, si.h_paths, 32 * n_sib + 256 + 32, si.h_poff, 4 * (n + 1), si.h_ridx, 4 * n,
                       si.h_seals, rows.size(), si.h_slen, 4 * sl.size(), si.h_st, n, si.h_rv, 4 * n)) != ZKV_OK || (diag_out && (rc = si.diag.grow(32 * n)) != ZKV_OK)) return rc;
    hipStream_t s = c->stream;
    if ((rc = order_after_previous(c, s)) != ZKV_OK) return rc;
    uint8_t* d_paths = (uint8_t*)(((uintptr_t)si.h_paths.as<uint8_t>() + 255u) & ~(uintptr_t)255u) + blob_shift;
    HIP_TRY(hipMemcpyAsync(si.h_a, in_a, 32 * n, hipMemcpyHostToDevice, s));
    if (!integrity) HIP_TRY(hipMemcpyAsync(si.h_b, in_b, 32 * n, hipMemcpyHostToDevice, s));
    if (n_sib) HIP_TRY(hipMemcpyAsync(d_paths, path_blob + 32 * (size_t)o0, 32 * n_sib, hipMemcpyHostToDevice, s));
    HIP_TRY(hipMemcpyAsync(si.h_poff, po.data(), 4 * (n + 1), hipMemcpyHostToDevice, s));
    if (!diag_out) {
        HIP_TRY(hipMemcpyAsync(si.h_ridx, root_idx, 4 * n, hipMemcpyHostToDevice, s));
        HIP_TRY(hipMemcpyAsync(si.h_seals, rows.data(), rows.size(), hipMemcpyHostToDevice, s));
        HIP_TRY(hipMemcpyAsync(si.h_slen, sl.data(), 4 * sl.size(), hipMemcpyHostToDevice, s));
    }
    HIP_TRY(hipStreamSynchronize(s));                    // the staging vectors are pageable host memory
    rc = run_setincl(c, n, si.h_a, integrity ? nullptr : si.h_b, d_paths, si.h_poff, n_sib, diag_out ? nullptr : si.h_ridx, m, si.h_seals, si.h_slen,
                     diag_out ? nullptr : si.h_st, diag_out ? nullptr : si.h_rv, diag_out ? si.diag : nullptr, s);
    if (rc != ZKV_OK) return rc;
    if (!diag_out) return return_to_host(si.h_st, si.h_rv, n, status, recv, s);
    HIP_TRY(hipMemcpyAsync(diag_out, si.diag, 32 * n, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    return ZKV_OK;
}
ZKV_EXPORT int zkv_risc0_setincl_verify_batch(zkv_ctx* c, size_t n, const uint8_t* image_ids, const uint8_t* journal_digests, const uint8_t* path_blob,
                                              const uint32_t* path_off, const uint32_t* root_idx, size_t m, const uint8_t* root_seal_blob,
                                              const uint64_t* root_seal_off, uint8_t* status, uint8_t* recv) {
    return setincl_host_call(c, n, image_ids, journal_digests, false, path_blob, path_off, root_idx, m, root_seal_blob, root_seal_off, status, recv, nullptr, 0);
}
ZKV_EXPORT int zkv_risc0_setincl_verify_integrity_batch(zkv_ctx* c, size_t n, const uint8_t* claim_digests, const uint8_t* path_blob, const uint32_t* path_off,
                                                        const uint32_t* root_idx, size_t m, const uint8_t* root_seal_blob, const uint64_t* root_seal_off,
                                                        uint8_t* status, uint8_t* recv) {
    return setincl_host_call(c, n, claim_digests, nullptr, true, path_blob, path_off, root_idx, m, root_seal_blob, root_seal_off, status, recv, nullptr, 0);
}
ZKV_EXPORT int zkv_diag_setincl_roots(zkv_ctx* c, size_t n, const uint8_t* image_ids, const uint8_t* journal_digests, const uint8_t* path_blob,
                                      const uint32_t* path_off, size_t blob_shift, uint8_t* out_roots) {
    if (n && !out_roots) return ZKV_ERR_INVALID_ARG;
    return setincl_host_call(c, n, image_ids, journal_digests, journal_digests == nullptr, path_blob, path_off, nullptr, 0, nullptr, nullptr, nullptr, nullptr,
                             out_roots, blob_shift);
}
ZKV_EXPORT int zkv_risc0_setincl_last_counts(zkv_ctx* c, uint64_t out[3]) {
    if (!c || c->vm != ZKV_VM_RISC0_SETINCL) return ZKV_ERR_WRONG_CTX;
    if (!out) return ZKV_ERR_INVALID_ARG;
    std::lock_guard<std::mutex> lk(c->mu);
    out[0] = c->si_counts[0]; out[1] = c->si_counts[1]; out[2] = 0;
    if (!c->dev_ready || !c->m_si.cnt) return ZKV_OK;
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(hipDeviceSynchronize());
    uint32_t v[2] = {0, 0};
    HIP_TRY(hipMemcpy(v, c->m_si.cnt, sizeof v, hipMemcpyDeviceToHost));
    out[2] = v[1];
    return ZKV_OK;
}

// The on-chain form: set_selector || abi.encode(Seal{bytes32[] path; bytes rootSeal}).
ZKV_EXPORT size_t zkv_risc0_setincl_seal_encode(const zkv_ctx* c, const uint8_t* path, size_t path_len, const uint8_t* root_seal, size_t root_seal_len,
                                                uint8_t* out, size_t cap) {
    if (!c || c->vm != ZKV_VM_RISC0_SETINCL || (path_len && !path) || (root_seal_len && !root_seal) || path_len > 0xFFFFFFu || root_seal_len > 0xFFFFFFFFu) return 0;
    const size_t padded = (root_seal_len + 31) / 32 * 32, total = 4 + 32 + 64 + 32 + 32 * path_len + 32 + padded;
    if (!out || cap < total) return total;
    memset(out, 0, total);
    memcpy(out, c->si_set_sel, 4);
    uint8_t* b = out + 4;
    host::abi_word_u32(b, 0x20);
    host::abi_word_u32(b + 32, 0x40);
    host::abi_word_u32(b + 64, 0x60 + 32 * path_len);
    host::abi_word_u32(b + 96, path_len);
    if (path_len) memcpy(b + 128, path, 32 * path_len);
    uint8_t* r = b + 128 + 32 * path_len;
    host::abi_word_u32(r, root_seal_len);
    if (root_seal_len) memcpy(r + 32, root_seal, root_seal_len);
    return total;
}
// a 32-byte big-endian word that fits 32 bits
static bool setincl_word(const uint8_t* p, uint64_t* v) {
    for (int k = 0; k < 28; k++) if (p[k]) return false;
    *v = be32_of(p + 28);
    return true;
}
ZKV_EXPORT int zkv_risc0_setincl_seal_decode(const zkv_ctx* c, const uint8_t* seal, size_t seal_len, uint8_t* status, uint8_t recv[4], size_t* path_at,
                                             size_t* path_len, size_t* root_seal_at, size_t* root_seal_len) {
    if (!c || c->vm != ZKV_VM_RISC0_SETINCL) return ZKV_ERR_WRONG_CTX;
    if (!status || !path_at || !path_len || !root_seal_at || !root_seal_len || (!seal && seal_len)) return ZKV_ERR_INVALID_ARG;
    *path_at = *path_len = *root_seal_at = *root_seal_len = 0;
    if (recv) memset(recv, 0, 4);
    *status = ZKV_STATUS_INVALID_PROOF_DATA;
    if (seal_len < 4) return ZKV_OK;
    if (memcmp(seal, c->si_set_sel, 4)) { *status = ZKV_STATUS_SELECTOR_MISMATCH; if (recv) memcpy(recv, seal, 4); return ZKV_OK; }
    const uint8_t* b = seal + 4;
    const uint64_t blen = seal_len - 4;
    uint64_t w0, w1, w2, k, len;
    if (blen < 160 || blen % 32) return ZKV_OK;                     // the shortest body: 0x20, two offsets, two length words
    if (!setincl_word(b, &w0) || w0 != 0x20 || !setincl_word(b + 32, &w1) || w1 != 0x40 || !setincl_word(b + 96, &k)) return ZKV_OK;
    if (k > (blen - 160) / 32) return ZKV_OK;                       // the path must leave room for the root seal's length word
    if (!setincl_word(b + 64, &w2) || w2 != 0x60 + 32 * k) return ZKV_OK;
    const uint8_t* r = b + 128 + 32 * k;
    if (!setincl_word(r, &len)) return ZKV_OK;
    const uint64_t padded = (len + 31) / 32 * 32;
    if (blen != 160 + 32 * k + padded) return ZKV_OK;               // nothing missing, nothing trailing
    for (uint64_t q = len; q < padded; q++) if (r[32 + q]) return ZKV_OK;    // clean padding
    *status = ZKV_STATUS_OK;
    *path_at = 4 + 128; *path_len = (size_t)k; *root_seal_at = (size_t)(4 + 128 + 32 * k + 32); *root_seal_len = (size_t)len;
    return ZKV_OK;
}

// ------------------------------------------------------------------ RISC Zero router with a set route (zkv_risc0_router_set.h)
// No reference counterpart: parity unpinned.  A set-inclusion seal is decoded on the device (k_rzrouter_set.hip), its root seal is
// verified by the router itself: the root jobs are 260-byte rows that go through run_router as a batch of their own.
ZKV_EXPORT zkv_ctx* zkv_risc0_router_create_with_set(size_t n_builtin, const uint8_t* control_roots, const uint8_t* bn254_control_ids, size_t n_keyed,
                                                     const uint8_t* const* vk_words, const uint8_t* keyed_control_roots, const uint8_t* keyed_control_ids,
                                                     const uint8_t set_builder_image_id[32], int device) {
    if (!set_builder_image_id || n_builtin > ZKV_RISC0_ROUTER_MAX_ROUTES || n_keyed > ZKV_RISC0_ROUTER_MAX_ROUTES ||
        n_builtin + n_keyed + 1 > ZKV_RISC0_ROUTER_MAX_ROUTES) return nullptr;      // the set route counts
    zkv_ctx* c = zkv_risc0_router_create(n_builtin, control_roots, bn254_control_ids, n_keyed, vk_words, keyed_control_roots, keyed_control_ids, device);
    if (!c) return nullptr;
    memcpy(c->si_id, set_builder_image_id, 32);
    setincl_set_selector(set_builder_image_id, c->si_set_sel);
    for (const uint32_t v : c->gw_sel) if (v == be32_of(c->si_set_sel)) { zkv_ctx_destroy(c); return nullptr; }
    c->rz_set = true;
    c->rzs_counts.assign(c->gw_sel.size() + 3, 0);
    return c;
}
ZKV_EXPORT int zkv_risc0_router_set_selector(const zkv_ctx* c, uint8_t out[4]) {
    if (!c || c->vm != ZKV_VM_RISC0_ROUTER || !c->rz_set) return ZKV_ERR_WRONG_CTX;
    if (!out) return ZKV_ERR_INVALID_ARG;
    memcpy(out, c->si_set_sel, 4);
    return ZKV_OK;
}
ZKV_EXPORT int zkv_risc0_router_set_has_root(zkv_ctx* c, const uint8_t root[32]) {
    if (!c || c->vm != ZKV_VM_RISC0_ROUTER || !c->rz_set) return ZKV_ERR_WRONG_CTX;
    if (!root) return ZKV_ERR_INVALID_ARG;
    std::lock_guard<std::mutex> lk(c->mu);
    bool found;
    (void)setincl_find(c, root, &found);
    return found ? 1 : 0;
}
ZKV_EXPORT int zkv_risc0_router_set_submit_root(zkv_ctx* c, const uint8_t root[32], const uint8_t* seal, size_t seal_len, uint8_t* status, uint8_t recv[4]) {
    if (!c || c->vm != ZKV_VM_RISC0_ROUTER || !c->rz_set) return ZKV_ERR_WRONG_CTX;
    if (!root || !status || (!seal && seal_len)) return ZKV_ERR_INVALID_ARG;
    uint8_t msg[64], jd[32], rv[4] = {0, 0, 0, 0}, st = ZKV_STATUS_VERIFICATION_FAILED;
    memcpy(msg, c->si_id, 32); memcpy(msg + 32, root, 32);
    host::sha256_host(msg, 64, jd);
    const int rc = zkv_risc0_router_verify(c, seal, seal_len, c->si_id, jd, &st, rv);      // V is the router
    if (rc != ZKV_OK) return rc;
    *status = st;
    if (recv) memcpy(recv, rv, 4);
    if (st != ZKV_STATUS_OK) return ZKV_OK;
    std::lock_guard<std::mutex> lk(c->mu);
    bool found;
    const size_t at = setincl_find(c, root, &found);
    if (found) return ZKV_OK;
    if (c->si_roots.size() / 32 >= ZKV_SETINCL_MAX_ROOTS) return ZKV_ERR_INVALID_ARG;
    try { c->si_roots.insert(c->si_roots.begin() + 32 * at, root, root + 32); } catch (const std::bad_alloc&) { return ZKV_ERR_OOM; }
    c->si_dirty = true;
    return ZKV_OK;
}
ZKV_EXPORT int zkv_risc0_router_set_last_counts(zkv_ctx* c, uint64_t out[4]) {
    if (!c || c->vm != ZKV_VM_RISC0_ROUTER || !c->rz_set) return ZKV_ERR_WRONG_CTX;
    if (!out) return ZKV_ERR_INVALID_ARG;
    std::lock_guard<std::mutex> lk(c->mu);
    for (int k = 0; k < 4; k++) out[k] = c->rzs_last[k];
    return ZKV_OK;
}

// Everything device-resident, ragged seals; the caller holds c->mu and has initialised the device.  Per chunk of 2^20 seals: the front
// and identity kernels, the hash and section 16's grouping; the chunk's four counters come back with the next synchronisation -- for the
// first chunk that is run_router's own (the caller's seals are partitioned once, for the whole call; a set seal is a seal of an unknown
// selector there and is answered again by the scatter, behind it in the stream), for a later chunk one of its own.  The root jobs then
// run through run_router as a batch of 260-byte rows with true lengths.  Two synchronisations for a call of one chunk that has root
// jobs: the direct seals' route counts (with the job count), the jobs' route counts.
// d_diag (diagnostic): stop behind the identity kernel of the one chunk and write every claim's representative.
// d_method: the per-seal method row (d_b is then set), or nullptr.  wire, d_span (decoded calldata, zkv_wire_rzset.h; d_seal_off is then
// nullptr): the partition takes the decoder's fixed-stride slots with their true lengths, the set stage every request's record, a
// distance from d_seals.  Chunk bases apply to the records as they do to the offsets.
static int run_router_set(zkv_ctx* c, size_t n, const uint8_t* d_seals, const uint64_t* d_seal_off, uint64_t seal_bytes, const uint8_t* d_a, const uint8_t* d_b,
                          uint8_t* d_status, uint8_t* d_recv, hipStream_t s, uint32_t fp_mask, uint32_t* d_diag, const uint8_t* d_method,
                          const RzWireArgs* wire, const RzsSpan* d_span) {
    int rc;
    const size_t cap = n < SETINCL_CHUNK ? n : SETINCL_CHUNK, R = c->gw_sel.size();
    size_t table = 64;
    while (table < 2 * cap) table <<= 1;
    RouterMem& rm = c->m_rz; SetGroupMem& g = rm.grp;
    if ((rc = grow_all(rm.s_rec, sizeof(RzsRec) * cap, rm.s_owner, 4 * table, rm.s_ridx, 4 * cap, g.rep, 4 * table, g.gslot, 4 * table, g.claim_job, 4 * cap,
                       g.job_claim, 4 * cap, rm.s_ans, cap, g.cnt, 16, g.roots, 32 * cap, g.stored, (size_t)32 * ZKV_SETINCL_MAX_ROOTS)) != ZKV_OK) return rc;
    if (c->si_dirty) {                                   // a root was submitted since the last call: nothing of this context is in flight after the wait
        HIP_TRY(hipDeviceSynchronize());
        if (!c->si_roots.empty()) HIP_TRY(hipMemcpy(g.stored, c->si_roots.data(), c->si_roots.size(), hipMemcpyHostToDevice));
        c->si_dirty = false;
    }
    if ((rc = order_after_previous(c, s)) != ZKV_OK) return rc;
    HIP_TRY(hipMemsetAsync(g.cnt, 0, 16, s));
    uint32_t seen[4] = {0, 0, 0, 0};
    uint64_t jobs = 0, direct_bad = 0;
    std::vector<uint64_t> direct;
    for (size_t base = 0; base < n; base += cap) {
        const size_t mc = n - base < cap ? n - base : cap;
        SetinclChunk ch;
        memset(&ch, 0, sizeof ch);
        ch.n = (uint32_t)mc; ch.m = (uint32_t)table; ch.n_stored = (uint32_t)(c->si_roots.size() / 32);
        ch.in_a = d_a + 32 * base; ch.in_b = d_b ? d_b + 32 * base : nullptr;
        ch.root_idx = rm.s_ridx;
        for (int q = 0; q < 8; q++) ch.id_be[q] = be32_of(c->si_id + 4 * q);
        setgroup_chunk_view(g, &ch);
        ch.status = d_status ? d_status + base : nullptr; ch.recv = d_recv ? d_recv + 4 * base : nullptr;
        RzsArgs a;
        memset(&a, 0, sizeof a);
        a.seals = d_seals; a.seal_off = d_seal_off ? d_seal_off + base : nullptr; a.seal_bytes = seal_bytes;
        if (wire) { a.span = d_span + base; a.wire_len = wire->seal_len + base; }
        a.method = d_method ? d_method + base : nullptr;
        a.set_sel = be32_of(c->si_set_sel); a.table = (uint32_t)table; a.fp_mask = fp_mask;
        a.rec = rm.s_rec; a.owner = rm.s_owner; a.root_idx = rm.s_ridx; a.ans = rm.s_ans;
        HIP_TRY(hipMemsetAsync(a.owner, 0xFF, 4 * table, s));
        HIP_TRY(hipMemsetAsync(ch.rep, 0xFF, 4 * table, s));
        HIP_TRY(hipMemsetAsync(g.cnt, 0, 4, s));
        launch_rzset_front(ch, a, s);
        if (d_diag) {
            launch_rzset_reps(ch, a, d_diag, s);
            HIP_TRY(hipGetLastError());
            return mark_done(c, s);
        }
        launch_rzset_hash(ch, a, c->consts, s);
        launch_setincl_group(ch, s);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipMemcpyAsync(seen, g.cnt, sizeof seen, hipMemcpyDeviceToHost, s));
        if (base == 0) {
            if (wire) rc = run_router(c, n, wire->seals, nullptr, 0, d_a, d_b, d_status, d_recv, s, d_method, wire->seal_len);
            else rc = run_router(c, n, d_seals, d_seal_off, seal_bytes, d_a, d_b, d_status, d_recv, s, d_method);
            if (rc != ZKV_OK) { (void)hipStreamSynchronize(s); return rc; }      // (the copy into `seen` may still be in flight)
            direct = c->rz_counts; direct_bad = c->rz_bad;                       // (the root jobs' partitions write both again)
        } else HIP_TRY(hipStreamSynchronize(s));
        const uint32_t nj = seen[0];
        if (nj > mc) return ZKV_ERR_HIP;
        jobs += nj;
        SetinclJobs jb;
        memset(&jb, 0, sizeof jb);
        jb.n_jobs = nj;
        if (nj) {
            if ((rc = setgroup_job_rows(g, nj, false, &jb)) != ZKV_OK) return rc;
            launch_rzset_jobs(ch, a, jb, s);
            HIP_TRY(hipGetLastError());
            // root jobs are `verify` calls of the router on (S, ID, sha256(ID || root)): the rows enter its partition with their true lengths
            if ((rc = run_router(c, nj, jb.rows, nullptr, 0, jb.ids, jb.jds, g.jst, g.jrv, s, nullptr, jb.lens)) != ZKV_OK) return rc;
        }
        launch_rzset_scatter(ch, a, jb, s);
        HIP_TRY(hipGetLastError());
    }
    if ((rc = mark_done(c, s)) != ZKV_OK) return rc;
    // the counts of the call: the Groth16 routes' are the caller's direct seals (not the root jobs); the set seals were seals of an
    // unknown selector to the partition
    if (direct.size() != R + 2 || direct[R] < seen[2]) return ZKV_ERR_HIP;
    c->rz_counts = direct; c->rz_bad = direct_bad;
    for (size_t r = 0; r < R; r++) c->rzs_counts[r] = direct[r];
    c->rzs_counts[R] = seen[2]; c->rzs_counts[R + 1] = direct[R] - seen[2]; c->rzs_counts[R + 2] = direct[R + 1];
    c->rzs_last[0] = seen[2]; c->rzs_last[1] = seen[3]; c->rzs_last[2] = jobs; c->rzs_last[3] = seen[1];
    return ZKV_OK;
}
ZKV_EXPORT int zkv_risc0_router_verify_ragged_dev(zkv_ctx* c, size_t n, const uint8_t* d_seal_blob, const uint64_t* d_seal_off, uint64_t blob_bytes,
                                                  const uint8_t* d_image_ids, const uint8_t* d_journal_digests, uint8_t* d_status, uint8_t* d_recv, void* stream) {
    if (!c || c->vm != ZKV_VM_RISC0_ROUTER) return ZKV_ERR_WRONG_CTX;
    if (n && (!d_seal_off || !d_image_ids || !d_status || (blob_bytes && !d_seal_blob))) return ZKV_ERR_INVALID_ARG;
    if (!n) return ZKV_OK;
    if (n > 0xFFFFFFF0u / ZKV_SEAL_BYTES) return ZKV_ERR_INVALID_ARG;
    std::lock_guard<std::mutex> lk(c->mu);
    int rc = ctx_device_init(c);
    if (rc != ZKV_OK) return rc;
    hipStream_t s = stream ? (hipStream_t)stream : c->stream;
    if (c->rz_set) return run_router_set(c, n, d_seal_blob, d_seal_off, blob_bytes, d_image_ids, d_journal_digests, d_status, d_recv, s, 0xFFFFFFFFu, nullptr);
    return run_router(c, n, d_seal_blob, d_seal_off, blob_bytes, d_image_ids, d_journal_digests, d_status, d_recv, s);
}
// Test only: the front and identity kernels alone on host buffers, the fingerprint ANDed with fp_mask (0: every claim starts at slot 0
// and probes linearly).  out_rep[i]: the representative of claim i's root seal, 0xFFFFFFFF for a seal that names none.
ZKV_EXPORT int zkv_diag_rzset_groups(zkv_ctx* c, size_t n, const uint8_t* seal_blob, const uint64_t* seal_off, size_t blob_shift, uint32_t fp_mask,
                                     uint32_t* out_rep) {
    if (!c || c->vm != ZKV_VM_RISC0_ROUTER || !c->rz_set) return ZKV_ERR_WRONG_CTX;
    if (n && (!seal_blob || !seal_off || !out_rep)) return ZKV_ERR_INVALID_ARG;
    if (!n) return ZKV_OK;
    if (n > SETINCL_CHUNK || blob_shift > 31 || !offsets_ok(seal_off, n)) return ZKV_ERR_INVALID_ARG;
    std::lock_guard<std::mutex> lk(c->mu);
    int rc = ctx_device_init(c);
    if (rc != ZKV_OK) return rc;
    const uint64_t o0 = seal_off[0], bytes = seal_off[n] - o0;
    std::vector<uint64_t> so;
    try { so.assign(seal_off, seal_off + n + 1); } catch (const std::bad_alloc&) { return ZKV_ERR_OOM; }
    for (auto& v : so) v -= o0;
    RouterMem& rm = c->m_rz;
    if ((rc = grow_all(rm.h_seals, (size_t)bytes + 256 + 32, rm.h_off, 8 * (n + 1), rm.s_diag, 4 * n)) != ZKV_OK) return rc;
    hipStream_t s = c->stream;
    if ((rc = order_after_previous(c, s)) != ZKV_OK) return rc;
    uint8_t* d_blob = (uint8_t*)(((uintptr_t)rm.h_seals.as<uint8_t>() + 255u) & ~(uintptr_t)255u) + blob_shift;
    if (bytes) HIP_TRY(hipMemcpyAsync(d_blob, seal_blob + o0, (size_t)bytes, hipMemcpyHostToDevice, s));
    HIP_TRY(hipMemcpyAsync(rm.h_off, so.data(), 8 * (n + 1), hipMemcpyHostToDevice, s));
    HIP_TRY(hipStreamSynchronize(s));                    // the staging vector is pageable host memory
    if ((rc = run_router_set(c, n, d_blob, rm.h_off, bytes, nullptr, nullptr, nullptr, nullptr, s, fp_mask, rm.s_diag)) != ZKV_OK) return rc;
    HIP_TRY(hipMemcpyAsync(out_rep, rm.s_diag, 4 * n, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    return ZKV_OK;
}

// ------------------------------------------------------------------ RISC Zero router with a set route: per-seal methods and eth_call batches
// (zkv_risc0_router_set_wire.h; parity unpinned).  The entry points of zkv_risc0_router_wire.h for seals of any
// length, valid on every router.  Without a set route they are the ragged twins of those calls: the decoded-input call is run_router on
// offsets with a method row, the calldata call is run_router_wire as it is.  With one, k_wire_rzset writes k_wire_rzrouter's slots for
// the partition and, beside them, every request's whole-seal record for the set stage (run_router_set).
ZKV_EXPORT int zkv_risc0_router_verify_call_ragged_dev(zkv_ctx* c, size_t n, const uint8_t* d_method, const uint8_t* d_seal_blob, const uint64_t* d_seal_off,
                                                       uint64_t blob_bytes, const uint8_t* d_in_a, const uint8_t* d_in_b, uint8_t* d_status, uint8_t* d_recv,
                                                       void* stream) {
    if (!c || c->vm != ZKV_VM_RISC0_ROUTER) return ZKV_ERR_WRONG_CTX;
    if (n && (!d_seal_off || !d_in_a || !d_in_b || !d_status || (blob_bytes && !d_seal_blob))) return ZKV_ERR_INVALID_ARG;
    if (!n) return ZKV_OK;
    if (n > 0xFFFFFFF0u / ZKV_SEAL_BYTES) return ZKV_ERR_INVALID_ARG;
    std::lock_guard<std::mutex> lk(c->mu);
    int rc = ctx_device_init(c);
    if (rc != ZKV_OK) return rc;
    hipStream_t s = stream ? (hipStream_t)stream : c->stream;
    if (c->rz_set) return run_router_set(c, n, d_seal_blob, d_seal_off, blob_bytes, d_in_a, d_in_b, d_status, d_recv, s, 0xFFFFFFFFu, nullptr, d_method);
    return run_router(c, n, d_seal_blob, d_seal_off, blob_bytes, d_in_a, d_in_b, d_status, d_recv, s, d_method);
}
ZKV_EXPORT int zkv_risc0_router_verify_call_ragged(zkv_ctx* c, size_t n, const uint8_t* method, const uint8_t* seal_blob, const uint64_t* seal_off,
                                                   const uint8_t* in_a, const uint8_t* in_b, uint8_t* status, uint8_t* recv) {
    if (!c || c->vm != ZKV_VM_RISC0_ROUTER) return ZKV_ERR_WRONG_CTX;
    if (n && (!seal_blob || !seal_off || !in_a || !in_b || !status)) return ZKV_ERR_INVALID_ARG;
    if (!n) return ZKV_OK;
    return router_host_batch(c, n, seal_blob, seal_off, in_a, in_b, status, recv, method);
}
// Calldata and its n + 1 offsets on the device, a router with a set route.  The decode is enqueued in front of the first count, so the
// call synchronises where run_router_set does.  One base address for the records: the lower of the blob and the arena, so that every
// start is a plain non-negative distance (as run_gateway_wire).
static int run_router_set_wire(zkv_ctx* c, size_t n, const uint8_t* d_cd, const uint64_t* d_off, uint64_t cd_bytes, uint8_t* d_status, uint8_t* d_recv,
                               uint8_t* d_ck, hipStream_t s) {
    int rc;
    RouterMem& rm = c->m_rz;
    if ((rc = grow_all(rm.w_seals, (size_t)ZKV_SEAL_BYTES * n + 8, rm.w_len, 4 * n, rm.h_a, 32 * n, rm.h_b, 32 * n, rm.h_method, n, rm.w_span, sizeof(RzsSpan) * n,
                       rm.w_arena, (size_t)rzsw_arena_bytes(cd_bytes))) != ZKV_OK) return rc;
    if ((rc = order_after_previous(c, s)) != ZKV_OK) return rc;
    RzSetWireArgs w;
    memset(&w, 0, sizeof w);
    w.w.n = n; w.w.cd = d_cd; w.w.off = d_off; w.w.cd_bytes = cd_bytes;
    for (int k = 0; k < RZW_KINDS; k++) w.w.sel_be[k] = be32_of(router_call_selector(k));
    w.w.seals = rm.w_seals; w.w.seal_len = rm.w_len; w.w.in_a = rm.h_a; w.w.in_b = rm.h_b; w.w.method = rm.h_method;
    w.w.call_kind = d_ck;
    w.set_sel = be32_of(c->si_set_sel); w.arena = rm.w_arena; w.span = rm.w_span;
    const uintptr_t pc = (uintptr_t)d_cd, pa = (uintptr_t)w.arena, base = pc < pa ? pc : pa;
    w.cd_delta = pc - base; w.arena_delta = pa - base;
    (void)hipEventRecord(c->ev_wire[0], s);
    launch_wire_rzset(w, s);
    (void)hipEventRecord(c->ev_wire[1], s);
    c->wire_timed = true;
    HIP_TRY(hipGetLastError());
    return run_router_set(c, n, (const uint8_t*)base, nullptr, 0, w.w.in_a, w.w.in_b, d_status, d_recv, s, 0xFFFFFFFFu, nullptr, w.w.method, &w.w, w.span);
}
ZKV_EXPORT int zkv_risc0_router_eth_call_ragged_dev(zkv_ctx* c, size_t n, const uint8_t* d_calldata, const uint64_t* d_calldata_off, uint64_t calldata_bytes,
                                                    uint8_t* d_status, uint8_t* d_recv, uint8_t* d_call_kind, void* stream) {
    if (!c || c->vm != ZKV_VM_RISC0_ROUTER) return ZKV_ERR_WRONG_CTX;
    if (n && (!d_calldata || !d_calldata_off || !d_status)) return ZKV_ERR_INVALID_ARG;
    if (!n) return ZKV_OK;
    if (n > 0xFFFFFFF0u / ZKV_SEAL_BYTES) return ZKV_ERR_INVALID_ARG;
    std::lock_guard<std::mutex> lk(c->mu);
    int rc = ctx_device_init(c);
    if (rc != ZKV_OK) return rc;
    hipStream_t s = stream ? (hipStream_t)stream : c->stream;
    if (c->rz_set) return run_router_set_wire(c, n, d_calldata, d_calldata_off, calldata_bytes, d_status, d_recv, d_call_kind, s);
    return run_router_wire(c, n, d_calldata, d_calldata_off, calldata_bytes, d_status, d_recv, d_call_kind, s);
}
ZKV_EXPORT int zkv_risc0_router_eth_call_ragged(zkv_ctx* c, size_t n, const uint8_t* blob, const uint64_t* off, uint8_t* reverted, uint8_t* returndata,
                                                uint32_t* returndata_len, uint8_t* status) {
    if (!c || c->vm != ZKV_VM_RISC0_ROUTER) return ZKV_ERR_WRONG_CTX;
    if (n && (!blob || !off || !reverted || !returndata || !returndata_len)) return ZKV_ERR_INVALID_ARG;
    if (!n) return ZKV_OK;
    if (n > 0xFFFFFFF0u / ZKV_SEAL_BYTES || !offsets_ok(off, n)) return ZKV_ERR_INVALID_ARG;
    std::vector<uint8_t> st(n), rv(4 * n), ck(n);
    {
        std::lock_guard<std::mutex> lk(c->mu);
        int rc = ctx_device_init(c);
        if (rc != ZKV_OK) return rc;
        RouterMem& rm = c->m_rz;
        if ((rc = grow_all(rm.h_st, n, rm.h_rv, 4 * n, rm.w_ck, n)) != ZKV_OK) return rc;
        hipStream_t s = c->stream;
        if ((rc = order_after_previous(c, s)) != ZKV_OK) return rc;
        std::vector<uint64_t> rel;
        uint64_t bytes = 0;
        if ((rc = stage_ragged(rm.h_seals, rm.h_off, blob, off, n, &rel, s, &bytes)) != ZKV_OK) return rc;
        if (c->rz_set) rc = run_router_set_wire(c, n, rm.h_seals, rm.h_off, bytes, rm.h_st, rm.h_rv, rm.w_ck, s);
        else rc = run_router_wire(c, n, rm.h_seals, rm.h_off, bytes, rm.h_st, rm.h_rv, rm.w_ck, s);
        if (rc != ZKV_OK) return rc;
        HIP_TRY(hipMemcpyAsync(ck.data(), rm.w_ck, n, hipMemcpyDeviceToHost, s));
        if ((rc = return_to_host(rm.h_st, rm.h_rv, n, st.data(), rv.data(), s)) != ZKV_OK) return rc;
    }
    for (size_t i = 0; i < n; i++) {
        const int rc = zkv_risc0_router_eth_call_returndata(c, st[i], rv.data() + 4 * i, ck[i], returndata + i * ZKV_RETURNDATA_STRIDE, &returndata_len[i], &reverted[i]);
        if (rc != ZKV_OK) return rc;
        if (status) status[i] = st[i];
    }
    return ZKV_OK;
}
ZKV_EXPORT int zkv_risc0_router_last_ragged_call_counts(zkv_ctx* c, uint64_t* out) {
    if (!c || c->vm != ZKV_VM_RISC0_ROUTER) return ZKV_ERR_WRONG_CTX;
    if (!out) return ZKV_ERR_INVALID_ARG;
    std::lock_guard<std::mutex> lk(c->mu);
    const std::vector<uint64_t>& v = c->rz_set ? c->rzs_counts : c->rz_counts;
    for (size_t r = 0; r < v.size(); r++) out[r] = v[r];
    out[v.size()] = c->rz_bad;
    return ZKV_OK;
}

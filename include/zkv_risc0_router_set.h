/*
 * zkv_risc0_router_set.h -- RISC Zero verifier router with a set route: set-inclusion seals arrive at the router like any other seal,
 * are decoded on the device, and their root seals are verified by whichever route the root seal's own selector names.
 *
 * On chain the RiscZeroSetVerifier is registered in the RiscZeroVerifierRouter under its own selector, and its inner VERIFIER is the
 * router itself.  A router created here holds the routes of zkv_risc0_router_create plus ONE set route: the last route, selector
 * set_selector(ID) as zkv_risc0_setincl_get_selector derives it (ID = the set-builder image id).  Companion of zkv_risc0_router.h and
 * zkv_risc0_set_inclusion.h (same library, same conventions, same codes); DESIGN.md section 17b describes the device path.
 *
 * PARITY UNPINNED: the reference holds no router and no set verifier.  Agreement is between tests/risc0_router_set_model.py, a host
 * build of the header arithmetic (csrc/zkv_rzrouter_set.h) and the device.
 *
 * Rules, per seal, in the caller's order:
 *   - shorter than 4 bytes, an unknown selector, the selector of a Groth16 route: exactly as zkv_risc0_router.h says.
 *   - the set selector in front of a body that is not the canonical abi.encode(Seal{bytes32[] path; bytes rootSeal}) (the encoding of
 *     zkv_risc0_set_inclusion.h; tests/set_inclusion_model.py abi_decode_seal is the definition): ZKV_STATUS_INVALID_PROOF_DATA, zero
 *     received selector.
 *   - library limits, answered ZKV_STATUS_INVALID_PROOF_DATA with no hashing and no pairing: a path deeper than ZKV_SETINCL_MAX_DEPTH,
 *     and a root seal that itself begins with the set selector (on chain that would recurse; nested sets are not followed here).
 *   - a canonical body with an empty root seal: ZKV_STATUS_OK iff root_i is among the submitted roots, else
 *     ZKV_STATUS_VERIFICATION_FAILED.
 *   - a canonical body with a root seal S: status and received selector are exactly those of the router's own
 *     verify(S, ID, sha256(ID || root_i)), root_i as in zkv_risc0_set_inclusion.h from the claim digest (ReceiptClaim::ok(...) for
 *     `verify` calls, given for `verify_integrity` calls): ZKV_STATUS_ROUTE_NOT_FOUND with S's first four bytes, INVALID_PROOF_DATA
 *     for an S of 1 - 3 or other than 260 bytes, every verdict of a built-in or keyed route.  Root jobs are always `verify` calls.
 * Claims whose root seals are byte-identical, with equal length, form a group: the lowest-index claim is its representative and its
 * root is verified once; a claim whose root differs from the representative's (a straggler) is verified on its own.  Every status
 * therefore is the per-claim one, and an honest batch pays one pairing per distinct root seal.  Batches run in chunks of 2^20 seals; a
 * group that spans chunks is verified once per chunk.
 *
 * On a router WITH a set route:
 *   - zkv_ctx_vm stays ZKV_VM_RISC0_ROUTER; zkv_risc0_router_route_count includes the set route; zkv_risc0_router_route reports it
 *     with *keyed = 2; zkv_risc0_router_route_verifier_key_digest returns ZKV_ERR_INVALID_ARG for it (it has no key).
 *   - zkv_risc0_router_verify, _verify_integrity, _verify_batch and _verify_integrity_batch stage their buffers and take the device
 *     path of zkv_risc0_router_verify_ragged_dev.
 *   - zkv_risc0_router_last_route_counts reports the set route's direct seals under its index (route_count + 2 words in all); the
 *     Groth16 routes' counts cover the caller's direct seals only, not the root jobs.
 *   - OUT OF SCOPE, answered ZKV_ERR_WRONG_CTX: zkv_risc0_router_verify_batch_dev (a fixed stride of 260 bytes cannot hold a set
 *     seal), zkv_risc0_router_verify_call_batch and _verify_call_batch_dev (the per-seal method row) and the calldata entry points
 *     of zkv_risc0_router_wire.h (zkv_risc0_router_eth_call_batch, _eth_call_batch_dev, and zkv_risc0_router_last_call_counts, which
 *     describes them).  On a router without a set route nothing changes.  Calldata and the per-seal method row for seals of any
 *     length, on every router, are the entry points of zkv_risc0_router_set_wire.h (new names: the ones above keep refusing).
 * Device scratch on top of zkv_risc0_router.h's: per seal of a chunk 69 bytes (claim record, root, slot, job tables, answer) and 24
 * bytes of table (2 slots per seal, three words each); per root job 333 bytes.
 */
#ifndef ZKV_RISC0_ROUTER_SET_H
#define ZKV_RISC0_ROUTER_SET_H
#include "zkv_risc0_router.h"
#include "zkv_risc0_set_inclusion.h"

#ifdef __cplusplus
extern "C" {
#endif

/* The router of zkv_risc0_router_create (same arguments, same meaning) plus the set route of set_builder_image_id.  The set route is
 * the last route and counts towards ZKV_RISC0_ROUTER_MAX_ROUTES.  NULL where zkv_risc0_router_create returns NULL (a router needs a
 * Groth16 route), on a NULL image id, on more than ZKV_RISC0_ROUTER_MAX_ROUTES routes in all, and where the set selector equals
 * another route's selector. */
zkv_ctx* zkv_risc0_router_create_with_set(size_t n_builtin, const uint8_t* control_roots, const uint8_t* bn254_control_ids,
                                          size_t n_keyed, const uint8_t* const* vk_words, const uint8_t* keyed_control_roots,
                                          const uint8_t* keyed_control_ids, const uint8_t set_builder_image_id[32], int device);
/* The set route's selector; ZKV_ERR_WRONG_CTX on a router without a set route. */
int zkv_risc0_router_set_selector(const zkv_ctx* ctx, uint8_t out[4]);

/* Everything resident in device memory, seals of ANY length: seal i = d_seal_blob[d_seal_off[i] .. d_seal_off[i + 1]), n + 1 offsets
 * (uint64_t, naturally aligned); the blob may have any alignment.  No offset is followed beyond blob_bytes: a seal whose offsets run
 * backwards or leave the blob is ZKV_STATUS_INVALID_PROOF_DATA and is never read.  d_journal_digests = NULL selects verify_integrity
 * with the claim digests in the first row.  Valid on EVERY router: without a set route it is the ragged twin of
 * zkv_risc0_router_verify_batch_dev and synchronises `stream` (NULL: the context's) once, as that call does.  With a set route it
 * synchronises `stream` TWICE for a batch of up to 2^20 seals that holds root jobs -- once behind the count of the caller's seals
 * (the number of root jobs comes back with the route counts), once behind the count of the root jobs -- and once more for every
 * further chunk of 2^20 seals, whose job count has its own wait; the verification itself is asynchronous. */
int zkv_risc0_router_verify_ragged_dev(zkv_ctx* ctx, size_t n, const uint8_t* d_seal_blob, const uint64_t* d_seal_off, uint64_t blob_bytes,
                                       const uint8_t* d_image_ids, const uint8_t* d_journal_digests, uint8_t* d_status,
                                       uint8_t* d_recv_selector, void* stream);

/* zkv_risc0_setincl_submit_root and zkv_risc0_setincl_has_root with V = the router: *status = the router's verify(seal, ID,
 * sha256(ID || root)), the root is remembered when that is ZKV_STATUS_OK; at most ZKV_SETINCL_MAX_ROOTS roots (beyond: ZKV_ERR_INVALID_ARG,
 * nothing is remembered).  ZKV_ERR_WRONG_CTX on a router without a set route. */
int zkv_risc0_router_set_submit_root(zkv_ctx* ctx, const uint8_t root[32], const uint8_t* seal, size_t seal_len, uint8_t* status,
                                     uint8_t recv_selector[4]);
int zkv_risc0_router_set_has_root(zkv_ctx* ctx, const uint8_t root[32]);
/* The most recent call that returned ZKV_OK: out[0] seals with the set selector, out[1] distinct root seals among their claims (per
 * chunk), out[2] root jobs actually run (groups and stragglers, over all chunks), out[3] stored-root lookups. */
int zkv_risc0_router_set_last_counts(zkv_ctx* ctx, uint64_t out[4]);

/* ------------------------------------------------------------------ diagnostics
 * Test only: the front and identity kernels alone on host buffers (at most 2^20 seals, staged blob_shift (0 .. 31) bytes past a 256-byte
 * aligned device address), with every root seal's fingerprint ANDed with fp_mask before it picks a table slot: 0 makes every claim
 * collide and probe linearly.  out_rep[i] = the representative (lowest seal index carrying the same root-seal bytes) of seal i, or
 * 0xFFFFFFFF for a seal that is no claim with a root seal.  No seal is verified. */
int zkv_diag_rzset_groups(zkv_ctx* ctx, size_t n, const uint8_t* seal_blob, const uint64_t* seal_off, size_t blob_shift, uint32_t fp_mask,
                          uint32_t* out_rep);

#ifdef __cplusplus
}
#endif
#endif /* ZKV_RISC0_ROUTER_SET_H */

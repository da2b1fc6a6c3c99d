/*
 * zkv_risc0_router.h -- RISC Zero verifier router: one context that sends every seal of a batch, on the device, to the Groth16 verifier
 * whose 4-byte selector begins the seal.
 *
 * On chain a RiscZeroVerifierRouter holds one Groth16 verifier per zkVM release and forwards `verify` / `verifyIntegrity` by the seal's
 * selector; every release has its own (control_root, bn254_control_id) and sometimes its own verification key.  A router context holds
 * up to ZKV_RISC0_ROUTER_MAX_ROUTES such verifiers ("routes") of two kinds:
 *   - built-in-key routes: a (control_root, bn254_control_id) pair on the key of risc0/crypto.rs -- exactly the instances of a verifier
 *     set (zkv_risc0_set_create), with the selector derived as there;
 *   - keyed routes, at most ZKV_RISC0_ROUTER_MAX_KEYED: a caller-supplied key with n_ic = 6 (ZKV_RISC0_KEY_BYTES bytes in
 *     zkv_groth16_ctx_create's layout, RISC Zero convention: A is negated, the key is stored as given) and its own (control_root,
 *     bn254_control_id).  The selector is DERIVED, not supplied: calculate_selector (risc0/verifier.rs:128-144) with
 *     compute_verifier_key_digest (risc0/crypto.rs:136-195) evaluated over the caller's key words.  A keyed route that holds the
 *     reference's own key and a real proof's control parameters therefore derives the reference's selector.
 * Route order: the built-in routes in order, then the keyed routes in order.
 * Companion of zkv.h (same library, same conventions, same ZKV_OK / ZKV_ERR_* codes); DESIGN.md section 17 describes the device path.
 *
 * PARITY UNPINNED for the routing itself: the reference holds no router.  ZKV_STATUS_ROUTE_NOT_FOUND and its ABI encoding have no
 * reference counterpart.  A seal routed to a built-in route gets exactly the pinned RISC Zero statuses of that verifier; a keyed route
 * holding the reference's key is reference-pinned through its derived selector; any other keyed route is three-way agreement (spec
 * model, C oracle, device) only.
 *
 * Routing rules (per seal, in the caller's order):
 *   - seal shorter than 4 bytes: ZKV_STATUS_INVALID_PROOF_DATA with a zero received selector (this project's definition: every route
 *     would answer so, risc0/verifier.rs:151); handled in place, it takes no slot and reaches no verifier.
 *   - no route has the seal's selector: ZKV_STATUS_ROUTE_NOT_FOUND (value 8, as in zkv_sp1_gateway.h), received selector = the seal's
 *     first four bytes; handled in place.  Its revert bytes are RISC Zero's SelectorUnknown(bytes4).
 *   - selector of route r: status and received selector are EXACTLY those of route r's IRiscZeroVerifier::verify / verify_integrity
 *     (risc0/verifier.rs:78-104, 146-196): a built-in route answers what a zkv_risc0_ctx_create context with its parameters answers
 *     (a control id out of range included: the verifier-set instance's behaviour), a keyed route what the same verifier with the
 *     caller's key and the derived selector answers -- a length other than 260 gives ZKV_STATUS_INVALID_PROOF_DATA; a key with an
 *     invalid point, a control id >= R, a malformed point or a failed pairing gives ZKV_STATUS_VERIFICATION_FAILED; the received
 *     selector is zero.  ZKV_STATUS_SELECTOR_MISMATCH therefore never comes out of a router.
 *
 * Context-wide calls: zkv_ctx_destroy, _synchronize, _reserve, _set_lanes_per_proof and _last_stage_ms forward to both groups (the
 * built-in routes are one verifier set, the keyed routes one key set) and keep their meaning; zkv_ctx_last_stage_ms sums the groups
 * that ran in the most recent call.  zkv_ctx_vm returns ZKV_VM_RISC0_ROUTER.  zkv_ctx_set_aggregate_check reaches both groups: the
 * built-in group with seed32 itself, the keyed group under the key sets' rules (zkv_groth16_set.h) with a secret of its own,
 * SHA-256(seed32 | 255), or drawn from the operating system -- only with the automatic mapping, from ZKV_AGG_MIN seals on the keyed
 * routes in one call, for routes whose key is valid with alpha and beta finite; a sub-batch holds seals of one route only, a failed
 * sub-batch is verified again seal by seal, and statuses and received selectors are those of the per-proof path, byte for byte.
 * zkv_ctx_aggregate_counters sums the two groups.  No GT tables for the keyed group.  A router is
 * single-device: zkv_ctx_create_sharded refuses it, and every batch entry point of another kind returns ZKV_ERR_WRONG_CTX on it.
 *
 * Device scratch of a batch call, on top of the two groups' own workspaces: 349 bytes per seal (compact 260-byte record, the two
 * 32-byte inputs, length, instance, slot tables and slot key, status, received selector); host-buffer calls also stage the caller's
 * buffers in device memory.  Device memory per keyed route: one VkTables (2,644,456 bytes) and five signals' 8-bit window rows of
 * 524,288 bytes each -- 5,265,896 bytes; per built-in route one 80-byte instance record beside the one shared key.
 * Alignment: byte-typed buffers (uint8_t*), host or device, may have any alignment; uint64_t* arguments need their natural one.
 */
#ifndef ZKV_RISC0_ROUTER_H
#define ZKV_RISC0_ROUTER_H
#include "zkv.h"

#ifdef __cplusplus
extern "C" {
#endif

#define ZKV_VM_RISC0_ROUTER 12
#define ZKV_RISC0_ROUTER_MAX_ROUTES 32
#define ZKV_RISC0_ROUTER_MAX_KEYED 8
#define ZKV_RISC0_KEY_BYTES 832        /* a key with n_ic = 6 in zkv_groth16_ctx_create's layout: 448 + 64 * 6 */
#ifndef ZKV_STATUS_ROUTE_NOT_FOUND
#define ZKV_STATUS_ROUTE_NOT_FOUND 8   /* routers only: RiscZeroVerifierRouter's SelectorUnknown(bytes4) here -- no reference counterpart */
#endif

/* n_builtin built-in-key routes (control_roots, bn254_control_ids: n_builtin x 32 bytes each, as zkv_risc0_set_create), then n_keyed
 * keyed routes (vk_words[k]: ZKV_RISC0_KEY_BYTES bytes; keyed_control_roots, keyed_control_ids: n_keyed x 32 bytes).  A count of zero
 * lets its pointers be NULL.  NULL on: no route at all, more than ZKV_RISC0_ROUTER_MAX_ROUTES routes, more than
 * ZKV_RISC0_ROUTER_MAX_KEYED keyed routes, NULL pointers, two equal selectors among all routes (the router could not tell them apart).
 * A keyed key that holds an invalid point is ACCEPTED and fails every proof of its own route only (ZKV_STATUS_VERIFICATION_FAILED), as in
 * key sets.  The device is set up lazily. */
zkv_ctx* zkv_risc0_router_create(size_t n_builtin, const uint8_t* control_roots, const uint8_t* bn254_control_ids,
                                 size_t n_keyed, const uint8_t* const* vk_words, const uint8_t* keyed_control_roots,
                                 const uint8_t* keyed_control_ids, int device);
size_t   zkv_risc0_router_route_count(const zkv_ctx* ctx);     /* 0 for a context that is not a router */
/* selector (4 bytes) of route r and whether it is a keyed route (1) or a built-in-key route (0); ZKV_ERR_INVALID_ARG past the routes */
int      zkv_risc0_router_route(const zkv_ctx* ctx, size_t r, uint8_t selector[4], int* keyed);
/* compute_verifier_key_digest of route r's key (the built-in key's digest for a built-in route); ZKV_ERR_INVALID_ARG past the routes */
int      zkv_risc0_router_route_verifier_key_digest(const zkv_ctx* ctx, size_t r, uint8_t out[32]);

/* One seal with the trait shapes of IRiscZeroVerifier; it runs as a batch of one.  status / recv_selector as for the batch calls. */
int zkv_risc0_router_verify(zkv_ctx* ctx, const uint8_t* seal, size_t seal_len, const uint8_t image_id[32], const uint8_t journal_digest[32],
                            uint8_t* status, uint8_t recv_selector[4]);
int zkv_risc0_router_verify_integrity(zkv_ctx* ctx, const uint8_t* seal, size_t seal_len, const uint8_t claim_digest[32], uint8_t* status,
                                      uint8_t recv_selector[4]);
/* Host buffers, ragged seals as in zkv_risc0_verify_batch (seal i = seal_blob[seal_off[i] .. seal_off[i+1]); recv_selector n x 4, may be
 * NULL).  The buffers are staged in device memory and take the device-resident path. */
int zkv_risc0_router_verify_batch(zkv_ctx* ctx, size_t n, const uint8_t* seal_blob, const uint64_t* seal_off, const uint8_t* image_ids,
                                  const uint8_t* journal_digests, uint8_t* status, uint8_t* recv_selector);
int zkv_risc0_router_verify_integrity_batch(zkv_ctx* ctx, size_t n, const uint8_t* seal_blob, const uint64_t* seal_off,
                                            const uint8_t* claim_digests, uint8_t* status, uint8_t* recv_selector);
/* Everything resident in device memory, enqueued on `stream` (NULL: the context's): seals at a fixed stride of ZKV_SEAL_BYTES (260),
 * n x 32 image ids, n x 32 journal digests.  d_journal_digests = NULL selects verify_integrity with the claim digests in the first row
 * (the convention of zkv_risc0_setincl_verify_batch_dev).  The call reads the per-route seal counts back once (a synchronisation with
 * `stream` after the count); the verification itself is asynchronous. */
int zkv_risc0_router_verify_batch_dev(zkv_ctx* ctx, size_t n, const uint8_t* d_seals, const uint8_t* d_image_ids,
                                      const uint8_t* d_journal_digests, uint8_t* d_status, uint8_t* d_recv_selector, void* stream);
/* Seal counts of the most recent call that returned ZKV_OK (a call that fails leaves them as they were): out[r] for route
 * r < route_count, then out[route_count] = selector unknown, out[route_count + 1] = shorter than 4 bytes. */
int zkv_risc0_router_last_route_counts(zkv_ctx* ctx, uint64_t* out /* route_count + 2 */);
/* ABI revert data of a router status (unpinned): ZKV_STATUS_ROUTE_NOT_FOUND gives 36 bytes, the SelectorUnknown(bytes4) selector
 * (keccak-256 of the signature, zkv_abi_function_selector) followed by the received selector left-aligned in one 32-byte word.  Every
 * other status gives what zkv_status_abi_encode(ZKV_VM_RISC0, status, received, <route 0's selector>, out) gives.  Returns the length,
 * or ZKV_ERR_*. */
int zkv_risc0_router_status_abi_encode(const zkv_ctx* ctx, uint8_t status, const uint8_t received[4], uint8_t out[68]);

#ifdef __cplusplus
}
#endif
#endif /* ZKV_RISC0_ROUTER_H */

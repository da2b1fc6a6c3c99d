/*
 * zkv_sp1_gateway_keys.h -- SP1 gateway: Groth16 routes with caller-supplied keys.
 *
 * SP1's on-chain gateway holds one verifier per SP1 release, and every release has its own Groth16 verification key and VERIFIER_HASH.
 * zkv_sp1_gateway_create knows one Groth16 release, the built-in v5.0.0 key.  This companion of zkv_sp1_gateway.h (same library, same
 * conventions) adds Groth16 routes whose key and verifier hash the caller supplies ("keyed routes"), beside the built-in route and the
 * PLONK routes.  Every batch entry point of zkv_sp1_gateway.h and zkv_sp1_gateway_wire.h serves them with no new call:
 * zkv_sp1_gateway_verify_proof (a single proof on a keyed route runs as a batch of one), _verify_batch, _verify_batch_dev, the two
 * eth_call entry points, _last_route_counts, _last_call_counts and _status_abi_encode.  DESIGN.md section 12d describes the device path:
 * the keyed routes of one gateway are verified in ONE pass, as one Groth16 key set whose key is uniform per wavefront.
 *
 * Statuses of a keyed route are sp1/verifier.rs:58-111 with that route's hash and key: a length other than 260 gives
 * ZKV_STATUS_INVALID_PROOF_DATA; program_vkey >= R, a malformed point or a failed pairing gives ZKV_STATUS_VERIFICATION_FAILED; the
 * received selector is zero.  Proofs shorter than 4 bytes and unknown selectors are answered by the gateway as before.
 *
 * PARITY: a keyed route that holds the reference's own SP1 key and hash (sp1/crypto.rs) is reference-pinned on ACCEPT and gives the
 * pinned SP1 statuses.  PARITY UNPINNED for every other key: three-way agreement (spec model, C oracle, device) only.
 *
 * Context-wide calls: zkv_ctx_reserve, _synchronize, _set_lanes_per_proof and _last_stage_ms forward to the keyed routes as to any
 * route.  zkv_ctx_set_aggregate_check reaches the keyed routes too: together they take the check under the key sets' rules
 * (zkv_groth16_set.h) -- only with the automatic mapping, from ZKV_AGG_MIN proofs on the keyed routes in one call, for routes whose key
 * is valid with alpha and beta finite; a sub-batch holds proofs of one route only, a failed sub-batch is verified again proof by proof,
 * and statuses and received selectors are those of the per-proof path, byte for byte.  Their secret is their own: SHA-256(seed32 | 255),
 * the derivation of the routes' secrets under an index no route has, or 32 bytes from the operating system (re-drawn as for any
 * context).  zkv_ctx_aggregate_counters includes their sub-batches in its sums.  No GT tables for them; a sharded gateway does not exist.
 *
 * Device memory per keyed route: one VkTables (2,644,456 bytes, most of it the unused short-key rows of the struct) and two signals' 8-bit
 * window rows of 524,288 bytes each -- 3,693,032 bytes; the workspace of the keyed routes is one, shared, and sized by their proofs in flight.
 */
#ifndef ZKV_SP1_GATEWAY_KEYS_H
#define ZKV_SP1_GATEWAY_KEYS_H
#include "zkv_sp1_gateway.h"

#ifdef __cplusplus
extern "C" {
#endif

#define ZKV_SP1_GROTH16_KEY_BYTES 640   /* a key with n_ic = 3 in zkv_groth16_ctx_create's layout: 448 + 64 * 3 */

/* zkv_sp1_gateway_create with n_keys keyed Groth16 routes.  Route order: the built-in v5.0.0 route if groth16 = 1, then the keyed routes
 * in order, then the PLONK routes in order.  vk_words[k]: ZKV_SP1_GROTH16_KEY_BYTES bytes in zkv_groth16_ctx_create's layout with
 * n_ic = 3, verified as VMType::Sp1: A is not negated, and beta, gamma, delta are stored negated as sp1/crypto.rs stores them.
 * verifier_hash: n_keys x 32 bytes; the first four bytes of each are the route's selector.  n_keys = 0 (vk_words and verifier_hash may
 * then be NULL) gives what zkv_sp1_gateway_create gives.  NULL on: what zkv_sp1_gateway_create refuses, more than
 * ZKV_SP1_GATEWAY_MAX_ROUTES routes in total, two equal selectors among all three kinds of route, NULL pointers.  A key that holds an
 * invalid point is ACCEPTED and fails every proof of its own route only (ZKV_STATUS_VERIFICATION_FAILED), as in key sets. */
zkv_ctx* zkv_sp1_gateway_create_keyed(int groth16, size_t n_keys, const uint8_t* const* vk_words, const uint8_t* verifier_hash,
                                      size_t n_plonk, const uint8_t* const* plonk_vk, const size_t* plonk_vk_len,
                                      const uint8_t* plonk_verifier_hash, int device);
/* The 32-byte verifier hash of route r, whatever its kind; ZKV_ERR_INVALID_ARG past the routes.  zkv_sp1_gateway_route reports
 * ZKV_VM_SP1 for a keyed route; zkv_sp1_gateway_route_ctx returns NULL for it, because the keyed routes share one internal context. */
int zkv_sp1_gateway_route_verifier_hash(const zkv_ctx* ctx, size_t r, uint8_t out[32]);

#ifdef __cplusplus
}
#endif
#endif /* ZKV_SP1_GATEWAY_KEYS_H */

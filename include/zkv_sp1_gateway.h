/*
 * zkv_sp1_gateway.h -- SP1 gateway: one context that routes every proof of a batch, on the device, to the SP1 verifier whose
 * 4-byte selector begins the proof.
 *
 * SP1's on-chain entry point is a gateway that reads the first 4 bytes of `proof_bytes` and forwards
 * `ISp1Verifier::verify_proof(program_vkey, public_values, proof_bytes)` to the verifier registered for them.  A gateway context
 * holds up to ZKV_SP1_GATEWAY_MAX_ROUTES such verifiers ("routes"): optionally the built-in SP1 v5.0.0 Groth16 verifier
 * (zkv_sp1_ctx_create) and any number of SP1 PLONK verifiers (zkv_sp1_plonk_ctx_create, one per key and verifier hash).
 * Companion of zkv.h (same library, same conventions, same ZKV_OK / ZKV_ERR_* codes); DESIGN.md section 12 describes the device path.
 * zkv_sp1_gateway_wire.h adds eth_call batches (raw `verifyProof` calldata) on a gateway.
 *
 * PARITY UNPINNED: the reference holds no gateway and no PLONK code.  ZKV_STATUS_ROUTE_NOT_FOUND and its ABI encoding, and every
 * PLONK status, have no reference counterpart; a proof routed to the Groth16 route gets exactly the pinned SP1 statuses.
 *
 * Routing rules (per proof, in the caller's order):
 *   - proof shorter than 4 bytes: ZKV_STATUS_INVALID_PROOF_DATA with a zero received selector (sp1/verifier.rs:64); handled in place,
 *     it takes no slot and reaches no verifier.  Device-resident batches: a proof whose offsets run backwards or past `proof_bytes` is
 *     never read and is answered the same way.
 *   - no route has the proof's selector: ZKV_STATUS_ROUTE_NOT_FOUND, received selector = those 4 bytes; handled in place.
 *   - selector of route r: route r's own status and received selector, from its full check order -- the length check included (a
 *     260-byte Groth16 proof that carries a PLONK route's selector gets that route's ZKV_STATUS_INVALID_PROOF_DATA).  The demultiplexer
 *     passes the true length through and decides nothing itself.
 *
 * Context-wide calls forward to every route and keep their meaning: zkv_ctx_destroy, _synchronize, _reserve, _set_lanes_per_proof,
 * _set_aggregate_check (every route its own secret, derived from seed32 or drawn afresh) and _aggregate_counters (summed).
 * zkv_ctx_last_stage_ms sums the routes that ran in the most recent call.  zkv_ctx_vm returns ZKV_VM_SP1_GATEWAY.
 * A gateway is single-device: zkv_ctx_create_sharded refuses it, zkv_ctx_vk_x_batch and every SP1 / PLONK entry point of zkv.h
 * return ZKV_ERR_WRONG_CTX on it.  zkv_status_abi_encode is unchanged (status 8 stays ZKV_ERR_INVALID_ARG there).
 *
 * Device scratch of a batch call, on top of the routes' own workspaces: sum over routes of n_r x record_r (260 bytes per Groth16-route
 * proof, 868 per PLONK-route proof) plus 61 bytes per proof; host-buffer calls also stage the caller's buffers in device memory.
 * Alignment: byte-typed buffers (uint8_t*), host or device, may have any alignment; uint32_t* / uint64_t* arguments need their natural one.
 */
#ifndef ZKV_SP1_GATEWAY_H
#define ZKV_SP1_GATEWAY_H
#include "zkv.h"

#ifdef __cplusplus
extern "C" {
#endif

#define ZKV_VM_SP1_GATEWAY 8
#define ZKV_SP1_GATEWAY_MAX_ROUTES 8
#define ZKV_STATUS_ROUTE_NOT_FOUND 8   /* gateway only: SP1VerifierGateway's RouteNotFound(bytes4) -- no reference counterpart */

/* groth16 = 1 adds the built-in SP1 v5.0.0 Groth16 verifier as route 0 (0: none); then one route per PLONK key, in order, in
 * zkv_sp1_plonk_ctx_create's layout, with its verifier hash (plonk_verifier_hash: n_plonk x 32 bytes).  NULL on: groth16 not 0 / 1,
 * no route at all, more than ZKV_SP1_GATEWAY_MAX_ROUTES, a PLONK key zkv_sp1_plonk_ctx_create refuses, two routes with equal 4-byte
 * selectors (a PLONK hash whose prefix is the Groth16 selector included), NULL pointers.  The device is set up lazily. */
zkv_ctx* zkv_sp1_gateway_create(int groth16, size_t n_plonk, const uint8_t* const* plonk_vk, const size_t* plonk_vk_len,
                                const uint8_t* plonk_verifier_hash, int device);
size_t   zkv_sp1_gateway_route_count(const zkv_ctx* ctx);     /* 0 for a context that is not a gateway */
/* selector (4 bytes) and kind (ZKV_VM_SP1 for the Groth16 route, ZKV_VM_SP1_PLONK) of route r; ZKV_ERR_INVALID_ARG past the routes */
int      zkv_sp1_gateway_route(const zkv_ctx* ctx, size_t r, uint8_t selector[4], int* vm);
/* route r's own context, owned by the gateway: for its getters (zkv_sp1_plonk_verifier_hash, ...).  NULL past the routes. */
zkv_ctx* zkv_sp1_gateway_route_ctx(zkv_ctx* ctx, size_t r);

/* One proof, routed on the host to the route's single-proof entry point.  status / recv_selector as for zkv_sp1_verify_proof. */
int zkv_sp1_gateway_verify_proof(zkv_ctx* ctx, const uint8_t vkey[32], const uint8_t* pv, size_t pv_len, const uint8_t* proof, size_t proof_len,
                                 uint8_t* status, uint8_t recv_selector[4]);
/* Host buffers, ragged as in zkv_sp1_verify_batch (recv_selector n x 4, may be NULL).  The buffers are staged in device memory and
 * take the device-resident path. */
int zkv_sp1_gateway_verify_batch(zkv_ctx* ctx, size_t n, const uint8_t* program_vkeys, const uint8_t* pv_blob, const uint64_t* pv_off,
                                 const uint8_t* proof_blob, const uint64_t* proof_off, uint8_t* status, uint8_t* recv_selector);
/* Device-resident, enqueued on `stream` (NULL: the context's).  Proofs RAGGED: proof i = d_proofs[d_proof_off[i] .. d_proof_off[i+1]),
 * the n + 1 offsets in device memory, proof_bytes = size of d_proofs (the bounds of every read); public values at a fixed pv_len stride
 * as in zkv_sp1_verify_batch_dev.  The call reads the per-route proof counts back once (a synchronisation with `stream` after the
 * count); the verification itself is asynchronous. */
int zkv_sp1_gateway_verify_batch_dev(zkv_ctx* ctx, size_t n, const uint8_t* d_vkeys, const uint8_t* d_pv, size_t pv_len,
                                     const uint8_t* d_proofs, const uint64_t* d_proof_off, uint64_t proof_bytes,
                                     uint8_t* d_status, uint8_t* d_recv_selector, void* stream);
/* Proof counts of the most recent call: out[r] for route r < route_count, then out[route_count] = route not found,
 * out[route_count + 1] = shorter than 4 bytes (or unreadable). */
int zkv_sp1_gateway_last_route_counts(zkv_ctx* ctx, uint64_t* out /* route_count + 2 */);
/* ABI revert data of a gateway status (unpinned): ZKV_STATUS_ROUTE_NOT_FOUND gives 36 bytes, the RouteNotFound(bytes4) selector
 * (keccak-256 of the signature, zkv_abi_function_selector) followed by the received selector left-aligned in one 32-byte word.
 * Every other status gives what zkv_status_abi_encode(ZKV_VM_SP1, status, received, <route 0's selector>, out) gives (a gateway
 * never reports SELECTOR_MISMATCH: the route it picks has the proof's selector).  Returns the length, or ZKV_ERR_*. */
int zkv_sp1_gateway_status_abi_encode(const zkv_ctx* ctx, uint8_t status, const uint8_t received[4], uint8_t out[68]);

#ifdef __cplusplus
}
#endif
#endif /* ZKV_SP1_GATEWAY_H */

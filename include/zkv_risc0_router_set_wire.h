/*
 * zkv_risc0_router_set_wire.h -- eth_call batches and a method per seal on a RISC Zero router WITH a set route: raw `verify` /
 * `verifyIntegrity` calldata whose seal may be a set-inclusion seal of any length, and the decoded-input call with ragged seals and a
 * method per seal.  Calldata layer, partition, set stage and root jobs all run on the device.  Companion of zkv_risc0_router_wire.h (the
 * calldata rules) and zkv_risc0_router_set.h (the set route); DESIGN.md section 17c describes the device path.
 *
 * PARITY UNPINNED: the reference holds no router and no set verifier.  Agreement is between tests/risc0_router_set_wire_model.py (the
 * composition of the two companions' models), a host build of the header arithmetic (csrc/zkv_wire_rzrouter.h, zkv_rzrouter_set.h,
 * zkv_wire_rzset.h) and the device.
 *
 * The entry points of zkv_risc0_router_wire.h answer ZKV_ERR_WRONG_CTX on a router with a set route and keep doing so; the ones below
 * are valid on EVERY router, as zkv_risc0_router_verify_ragged_dev is.  On a router without a set route they answer exactly what
 * zkv_risc0_router_eth_call_batch[_dev] and zkv_risc0_router_verify_call_batch answer (zkv_risc0_router_verify_call_ragged_dev is the
 * ragged twin of zkv_risc0_router_verify_call_batch_dev).
 *
 * Rules, per request, in the caller's order:
 *   Calldata.  The four call shapes of zkv_risc0_router_wire.h and its canonical-only rule.  A request that is not a canonical call --
 *     another function selector, fewer than 4 bytes, an offset word other than the shape's, a length word of 2^32 or more, a missing or
 *     trailing byte, a uint8[] element above 255, a non-zero padding byte -- is ZKV_STATUS_BAD_CALLDATA with a zero received selector,
 *     empty revert data and call kind ZKV_RISC0_ROUTER_CALL_KIND_BAD.  It takes no slot, reaches no route, is not a set seal, is not
 *     hashed and starts no root job.  A method byte above ZKV_METHOD_VERIFY_INTEGRITY in the decoded-input calls is treated the same
 *     way.  EVERY uint8[] element of a seal is checked, whatever the seal's length and whatever route it goes to, and every padding
 *     byte.  Offsets that run backwards or past the blob: the request is never read (ZKV_STATUS_BAD_CALLDATA; a seal of the
 *     decoded-input calls: ZKV_STATUS_INVALID_PROOF_DATA).
 *   The seal inside a canonical call.  Exactly zkv_risc0_router_set.h's rules: shorter than 4 bytes, an unknown selector, the selector
 *     of a Groth16 route as zkv_risc0_router.h says; the set selector in front of a body that is not the canonical abi.encode(Seal) is
 *     ZKV_STATUS_INVALID_PROOF_DATA -- NOT bad calldata: the calldata layer and the seal layer keep their own verdicts --; a path deeper
 *     than ZKV_SETINCL_MAX_DEPTH and a root seal that begins with the set selector are the library limits
 *     (ZKV_STATUS_INVALID_PROOF_DATA, no hashing, no pairing); an empty root seal looks up the submitted roots; a root seal S gets the
 *     router's own verify(S, ID, sha256(ID || root)).
 *   Method per claim.  For a set seal, a `verify` row derives the claim digest ReceiptClaim::ok(image_id, journal_digest) from its two
 *     inputs, a `verifyIntegrity` row takes in_a as the claim digest -- per row, within one batch.  Root jobs are always `verify` calls.
 *   Grouping.  Bytes decide, method and calldata form do not: claims whose root seals are byte-identical form one group even if one
 *     arrived in uint8[] form and one in bytes form, or one through verify and one through verifyIntegrity.  Stragglers, chunks of 2^20
 *     requests and "a group that spans chunks is verified once per chunk" are zkv_risc0_router_set.h's.
 *
 * Synchronisation: the decode is enqueued on `stream` in front of the first count; the calls wait where
 * zkv_risc0_router_verify_ragged_dev waits on the same router, and not once more.
 *
 * OVERLAPPING REQUESTS (the warning of zkv_sp1_gateway_wire.h): a uint8[] request is compacted into an arena near a 32nd of its blob
 * offset.  Requests whose calldata does not overlap in the blob do not overlap there; two uint8[] requests whose calldata DOES overlap in
 * the blob may see each other's decoded bytes.  Hand in requests that do not overlap.
 *
 * Device scratch on a router with a set route, on top of zkv_risc0_router_set.h's: 346 bytes per request (zkv_risc0_router_wire.h's
 * 330 and a 16-byte record of where the whole seal lies) and an arena of calldata_bytes / 32 + 64 bytes.  A bytes-form seal is read
 * where it lies in the caller's blob; nothing but its 260-byte slot is copied.
 */
#ifndef ZKV_RISC0_ROUTER_SET_WIRE_H
#define ZKV_RISC0_ROUTER_SET_WIRE_H
#include "zkv_risc0_router_set.h"
#include "zkv_risc0_router_wire.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Decoded inputs with a method per seal, seals of ANY length, everything in device memory: the blob and offsets of
 * zkv_risc0_router_verify_ragged_dev, the method row and inputs of zkv_risc0_router_verify_call_batch_dev (d_method = NULL: all
 * ZKV_METHOD_VERIFY; d_in_b is never NULL and is not read for verifyIntegrity rows; d_recv_selector may be NULL). */
int zkv_risc0_router_verify_call_ragged_dev(zkv_ctx* ctx, size_t n, const uint8_t* d_method, const uint8_t* d_seal_blob,
                                            const uint64_t* d_seal_off, uint64_t blob_bytes, const uint8_t* d_in_a, const uint8_t* d_in_b,
                                            uint8_t* d_status, uint8_t* d_recv_selector, void* stream);
/* Host buffers, staged in device memory: zkv_risc0_router_verify_call_batch's arguments. */
int zkv_risc0_router_verify_call_ragged(zkv_ctx* ctx, size_t n, const uint8_t* method, const uint8_t* seal_blob, const uint64_t* seal_off,
                                        const uint8_t* in_a, const uint8_t* in_b, uint8_t* status, uint8_t* recv_selector);
/* zkv_risc0_router_eth_call_batch_dev's arguments: n + 1 offsets in device memory, calldata_bytes = size of d_calldata,
 * d_recv_selector (n x 4) and d_call_kind (n bytes) may be NULL. */
int zkv_risc0_router_eth_call_ragged_dev(zkv_ctx* ctx, size_t n, const uint8_t* d_calldata, const uint64_t* d_calldata_off,
                                         uint64_t calldata_bytes, uint8_t* d_status, uint8_t* d_recv_selector, uint8_t* d_call_kind,
                                         void* stream);
/* Host buffers, the signature and the ZKV_RETURNDATA_STRIDE layout of zkv_risc0_router_eth_call_batch; status may be NULL.  The return
 * data of one status: zkv_risc0_router_eth_call_returndata, which answers on any router. */
int zkv_risc0_router_eth_call_ragged(zkv_ctx* ctx, size_t n, const uint8_t* calldata_blob, const uint64_t* calldata_off, uint8_t* reverted,
                                     uint8_t* returndata, uint32_t* returndata_len, uint8_t* status);
/* The most recent router call that returned ZKV_OK, route_count + 3 words (zkv_risc0_router_route_count counts the set route): every
 * route's seals -- the set route under its own index with its direct seals, as zkv_risc0_router_last_route_counts reports them on a
 * router with a set route --, unknown selector, decoded seals shorter than 4 bytes, bad calldata (bad method bytes and undecodable
 * requests).  zkv_risc0_router_set_last_counts and zkv_ctx_last_wire_ms describe the calls above too. */
int zkv_risc0_router_last_ragged_call_counts(zkv_ctx* ctx, uint64_t* out /* route_count + 3 */);

#ifdef __cplusplus
}
#endif
#endif /* ZKV_RISC0_ROUTER_SET_WIRE_H */

/*
 * zkv_risc0_router_wire.h -- eth_call batches on a RISC Zero router: raw `verify` / `verifyIntegrity` calldata, both methods and seals of
 * several releases mixed, decoded and routed on the device; and the decoded-input call with a method per seal that it rests on.
 * Companion of zkv_risc0_router.h (same library, same conventions); DESIGN.md section 17a describes the device path.
 *
 * PARITY UNPINNED: the reference holds no router.  The calldata rules below are those of zkv.h's wire layer (canonical encodings only),
 * applied to the router's two methods; a decoded call gets exactly what zkv_risc0_router_verify_call_batch gives its arguments.
 *
 * Two calldata forms and two methods, chosen per request by the 4-byte function selector (keccak-256 of the signature,
 * zkv_abi_function_selector); pad32 rounds up to a multiple of 32:
 *   ZKV_CALLDATA_FORM_UINT8_ARRAY -- what a Stylus shell's `Vec<u8>` looks like, one 32-byte word per byte (zkv.h's encoders):
 *       verify(uint8[],bytes32,bytes32)   sel | 0x60 | image_id | journal_digest | L | L element words
 *       verifyIntegrity(uint8[],bytes32)  sel | 0x40 | claim_digest | L | L element words
 *   ZKV_CALLDATA_FORM_BYTES -- IRiscZeroVerifier's Solidity ABI, as a deployed RiscZeroVerifierRouter is called:
 *       verify(bytes,bytes32,bytes32)     sel | 0x60 | image_id | journal_digest | L | seal, zeros to pad32(L)           (selector ab750e75)
 *       verifyIntegrity((bytes,bytes32))  sel | 0x20 | 0x40 | claim_digest | L | seal, zeros to pad32(L)                 (selector 1599ead5)
 * Anything else reverts with empty return data and ZKV_STATUS_BAD_CALLDATA (zero received selector): another selector -- the router's own
 * addVerifier / removeVerifier / getVerifier are not simulated -- or fewer than 4 bytes, an offset word other than the ones above, a
 * length word of 2^32 or more, a uint8[] element above 255, a non-zero padding byte, a missing or a trailing byte.  A bad request takes no
 * slot and reaches no route.  The decoded length is passed on as it is: the routes decide about it (zkv_risc0_router.h, routing rules).
 *
 * Device scratch, on top of zkv_risc0_router_verify_batch_dev's: 330 bytes per request (the decoded 260-byte slot -- no route reads more
 * of a seal --, true length, two inputs, method, compact method); the calldata itself is read once and not copied.
 */
#ifndef ZKV_RISC0_ROUTER_WIRE_H
#define ZKV_RISC0_ROUTER_WIRE_H
#include "zkv_risc0_router.h"

#ifdef __cplusplus
extern "C" {
#endif

#ifndef ZKV_CALLDATA_FORM_UINT8_ARRAY
#define ZKV_CALLDATA_FORM_UINT8_ARRAY 0
#define ZKV_CALLDATA_FORM_BYTES 1
#endif
#define ZKV_RISC0_ROUTER_CALL_KIND_BAD 255     /* call kind of a request that is not a canonical call; otherwise 2 * form + method */

/* Decoded inputs with a method per seal (ZKV_METHOD_*; method = NULL: all ZKV_METHOD_VERIFY): in_a is the image id of a verify row or the
 * claim digest of a verifyIntegrity row, in_b (n x 32, never NULL) the journal digest, not read for verifyIntegrity rows -- as
 * zkv_mixed_verify_call_batch.  Any other method byte: ZKV_STATUS_BAD_CALLDATA with a zero received selector, answered in place (no slot,
 * no route).  Everything else as zkv_risc0_router_verify_batch (ragged host seals) and zkv_risc0_router_verify_batch_dev (device-resident,
 * seals at a stride of ZKV_SEAL_BYTES, one synchronisation with `stream` after the count). */
int zkv_risc0_router_verify_call_batch(zkv_ctx* ctx, size_t n, const uint8_t* method, const uint8_t* seal_blob, const uint64_t* seal_off,
                                       const uint8_t* in_a, const uint8_t* in_b, uint8_t* status, uint8_t* recv_selector);
int zkv_risc0_router_verify_call_batch_dev(zkv_ctx* ctx, size_t n, const uint8_t* d_method, const uint8_t* d_seals, const uint8_t* d_in_a,
                                           const uint8_t* d_in_b, uint8_t* d_status, uint8_t* d_recv_selector, void* stream);

/* Canonical calldata of verify(seal, image_id, journal_digest) / verifyIntegrity(Receipt(seal, claim_digest)) in `form`.  Return the
 * needed length, like the other encoders (`out` is written only when cap is at least that; NULL out just asks); 0 for a form that does
 * not exist.  ZKV_CALLDATA_FORM_UINT8_ARRAY gives zkv_risc0_encode_verify_call / zkv_risc0_encode_verify_integrity_call's bytes. */
size_t zkv_risc0_router_encode_verify_call(int form, const uint8_t* seal, size_t seal_len, const uint8_t image_id[32],
                                           const uint8_t journal_digest[32], uint8_t* out, size_t cap);
size_t zkv_risc0_router_encode_verify_integrity_call(int form, const uint8_t* seal, size_t seal_len, const uint8_t claim_digest[32], uint8_t* out,
                                                     size_t cap);
/* Host buffers, the signature and the ZKV_RETURNDATA_STRIDE layout of zkv_risc0_eth_call_batch: request i = calldata_blob[calldata_off[i] ..
 * calldata_off[i+1]).  The buffers are staged in device memory and take the device-resident path.  status may be NULL. */
int zkv_risc0_router_eth_call_batch(zkv_ctx* ctx, size_t n, const uint8_t* calldata_blob, const uint64_t* calldata_off, uint8_t* reverted,
                                    uint8_t* returndata, uint32_t* returndata_len, uint8_t* status);
/* Device-resident, enqueued on `stream` (NULL: the context's): the n + 1 offsets in device memory, calldata_bytes = size of d_calldata (a
 * request whose offsets run backwards or past it is never read and gets ZKV_STATUS_BAD_CALLDATA).  d_recv_selector (n x 4) and
 * d_call_kind (n bytes: 2 * form + method, ZKV_RISC0_ROUTER_CALL_KIND_BAD for bad calldata -- the return data of a status depends on the
 * form) may be NULL.  The decode is enqueued in front of the count; the call synchronises where zkv_risc0_router_verify_batch_dev does,
 * once, after the count. */
int zkv_risc0_router_eth_call_batch_dev(zkv_ctx* ctx, size_t n, const uint8_t* d_calldata, const uint64_t* d_calldata_off, uint64_t calldata_bytes,
                                        uint8_t* d_status, uint8_t* d_recv_selector, uint8_t* d_call_kind, void* stream);
/* Return / revert data of one status: ZKV_STATUS_OK is not reverted, with one `true` word in form UINT8_ARRAY (the Stylus shells of zkv.h)
 * and no data in form BYTES (Solidity's verify returns nothing); ZKV_STATUS_BAD_CALLDATA is reverted with no data, whatever the call kind;
 * every other status is reverted with what zkv_risc0_router_status_abi_encode gives (its errors are passed on).  ZKV_ERR_INVALID_ARG for
 * a call kind above 3 with any status but ZKV_STATUS_BAD_CALLDATA. */
int zkv_risc0_router_eth_call_returndata(const zkv_ctx* ctx, uint8_t status, const uint8_t recv_selector[4], uint8_t call_kind,
                                         uint8_t out[ZKV_RETURNDATA_STRIDE], uint32_t* out_len, uint8_t* reverted);
/* zkv_risc0_router_last_route_counts with one more column: out[route_count + 2] = bad calldata (bad method bytes and undecodable
 * requests; out[route_count + 1] holds the decoded seals shorter than 4 bytes alone).  zkv_ctx_last_wire_ms gives the decode time of the
 * most recent eth_call batch on the router. */
int zkv_risc0_router_last_call_counts(zkv_ctx* ctx, uint64_t* out /* route_count + 3 */);

#ifdef __cplusplus
}
#endif
#endif /* ZKV_RISC0_ROUTER_WIRE_H */

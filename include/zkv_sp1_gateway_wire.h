/*
 * zkv_sp1_gateway_wire.h -- eth_call batches on an SP1 gateway: raw `verifyProof` calldata, Groth16 and PLONK proofs mixed, decoded and
 * routed on the device.  Companion of zkv_sp1_gateway.h (same library, same conventions); DESIGN.md section 12c describes the device path.
 *
 * PARITY UNPINNED: the reference holds no gateway, no PLONK code and no router.  The calldata rules below are those of zkv.h's wire
 * layer (canonical encodings only), applied to the gateway's one method; a decoded call gets exactly what zkv_sp1_gateway_verify_batch
 * gives its three arguments.
 *
 * Two calldata forms, chosen per request by the 4-byte function selector (keccak-256 of the signature, zkv_abi_function_selector):
 *   ZKV_CALLDATA_FORM_UINT8_ARRAY  verifyProof(bytes32,uint8[],uint8[]) -- what a Stylus shell's `Vec<u8>` looks like, one 32-byte word per
 *       byte: sel | vkey | 0x60 | 0x80 + 32 Lpv | Lpv | Lpv words | Lproof | Lproof words
 *   ZKV_CALLDATA_FORM_BYTES        verifyProof(bytes32,bytes,bytes) -- ISP1Verifier's Solidity ABI, packed bytes padded with zeros to 32:
 *       sel | vkey | 0x60 | 0x80 + pad32(Lpv) | Lpv | pv, padding | Lproof | proof, padding          (pad32 rounds up to a multiple of 32)
 * Anything else reverts with empty return data and ZKV_STATUS_BAD_CALLDATA (zero received selector): another selector -- the gateway's
 * own routes / addRoute / freezeRoute are not simulated -- or fewer than 4 bytes, an offset other than the ones above, a length word of
 * 2^32 or more, a uint8[] element above 255, a non-zero padding byte, a missing or a trailing byte.  A bad request takes no slot and
 * reaches no route.  Lengths are passed on as they are: the routes decide about them (zkv_sp1_gateway.h, routing rules).
 *
 * Device scratch, on top of zkv_sp1_gateway_verify_batch_dev's: 57 bytes per request and a 32nd of the calldata (form UINT8_ARRAY
 * requests are compacted there; form BYTES requests are read where they lie).  Requests of one device-resident batch should not overlap
 * in the blob: two form UINT8_ARRAY requests whose calldata overlaps may see each other's decoded bytes.
 */
#ifndef ZKV_SP1_GATEWAY_WIRE_H
#define ZKV_SP1_GATEWAY_WIRE_H
#include "zkv_sp1_gateway.h"

#ifdef __cplusplus
extern "C" {
#endif

#define ZKV_CALLDATA_FORM_UINT8_ARRAY 0
#define ZKV_CALLDATA_FORM_BYTES 1

/* Canonical calldata of verifyProof(program_vkey, public_values, proof_bytes) in `form`.  Returns the needed length, like the other
 * encoders (`out` is written only when cap is at least that; NULL out just asks); 0 for a form that does not exist. */
size_t zkv_sp1_gateway_encode_verify_proof_call(int form, const uint8_t program_vkey[32], const uint8_t* pv, size_t pv_len, const uint8_t* proof,
                                                size_t proof_len, uint8_t* out, size_t cap);
/* Host buffers, the signature and the ZKV_RETURNDATA_STRIDE layout of zkv_sp1_eth_call_batch: request i = calldata_blob[calldata_off[i] ..
 * calldata_off[i+1]).  The buffers are staged in device memory and take the device-resident path.  status may be NULL. */
int zkv_sp1_gateway_eth_call_batch(zkv_ctx* ctx, size_t n, const uint8_t* calldata_blob, const uint64_t* calldata_off, uint8_t* reverted,
                                   uint8_t* returndata, uint32_t* returndata_len, uint8_t* status);
/* Device-resident, enqueued on `stream` (NULL: the context's): the n + 1 offsets in device memory, calldata_bytes = size of d_calldata (a
 * request whose offsets run backwards or past it is never read and gets ZKV_STATUS_BAD_CALLDATA).  d_recv_selector (n x 4) may be NULL.
 * Synchronises where zkv_sp1_gateway_verify_batch_dev does, once, after the count. */
int zkv_sp1_gateway_eth_call_batch_dev(zkv_ctx* ctx, size_t n, const uint8_t* d_calldata, const uint64_t* d_calldata_off, uint64_t calldata_bytes,
                                       uint8_t* d_status, uint8_t* d_recv_selector, void* stream);
/* Return / revert data of one status: ZKV_STATUS_OK is not reverted and has no data (verifyProof returns nothing), ZKV_STATUS_BAD_CALLDATA
 * is reverted with no data, every other status is reverted with what zkv_sp1_gateway_status_abi_encode gives (its errors are passed on). */
int zkv_sp1_gateway_eth_call_returndata(const zkv_ctx* ctx, uint8_t status, const uint8_t recv_selector[4], uint8_t out[ZKV_RETURNDATA_STRIDE],
                                        uint32_t* out_len, uint8_t* reverted);
/* zkv_sp1_gateway_last_route_counts with one more column: out[route_count + 2] = bad calldata (always 0 after a decoded-input call).
 * zkv_ctx_last_wire_ms gives the decode time of the most recent eth_call batch on the gateway. */
int zkv_sp1_gateway_last_call_counts(zkv_ctx* ctx, uint64_t* out /* route_count + 3 */);

#ifdef __cplusplus
}
#endif
#endif /* ZKV_SP1_GATEWAY_WIRE_H */

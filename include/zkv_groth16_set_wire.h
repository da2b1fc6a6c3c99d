/*
 * zkv_groth16_set_wire.h -- eth_call batches on a Groth16 key set whose keys are deployed verifier contracts: raw `verifyProof` calldata,
 * each request addressed to a contract, resolved, decoded and verified on the device.  Companion of zkv_groth16_set.h (same library, same
 * conventions); DESIGN.md section 11d describes the device path.
 *
 * PARITY UNPINNED: the reference holds no generic contract shell.  The two contract forms below are the Solidity verifiers that snarkjs
 * and gnark export, one contract per circuit; a decoded call gets exactly what zkv_groth16_set_verify_batch gives its key, proof and
 * signals.  Canonical encodings only, as in every other wire layer of this library: the arguments are static arrays, so the one canonical
 * encoding of a call is its selector followed by exactly 8 + N words.  The gnark error names are as the gnark template words them.
 *
 * Forms (the contract's N is its key's n_ic - 1; the selector is keccak-256 of the signature with N in decimal, derived at creation):
 *   ZKV_G16_FORM_SNARKJS  verifyProof(uint256[2],uint256[2][2],uint256[2],uint256[N]) returns (bool).  Never reverts on a bad proof: a
 *       signal >= r, a point the precompiles refuse and a failed pairing all return false.
 *   ZKV_G16_FORM_GNARK    verifyProof(uint256[8],uint256[N]), returns nothing.  Reverts PublicInputNotInField() when a signal is >= r
 *       (checked first) and ProofInvalid() otherwise.
 * Both have one body: the eight proof words in the order of the EVM precompiles, then the N signal words -- the 256-byte proof and the
 * signal row of zkv_groth16_set_verify_batch, so decoding moves bytes and interprets none.  vm_type keeps its meaning (who negates A) and
 * is independent of the form.  A key with n_ic = 1 has no callable method (uint256[0] is not a Solidity type).
 *
 * The rules of request i, in this order:
 *   1. offsets that run backwards or past the calldata: ZKV_STATUS_BAD_CALLDATA, the request is never read (no key is resolved);
 *   2. to[i] is none of the set's addresses: ZKV_STATUS_NO_CONTRACT -- not reverted, empty return data, what an eth_call to an address
 *      without code answers;
 *   3. fewer than 4 bytes, a selector other than the key's, a length other than 4 + 32 (8 + N) (a byte missing or trailing), or a key
 *      with n_ic = 1: ZKV_STATUS_BAD_CALLDATA, reverted with empty data;
 *   4. a signal word >= r: ZKV_STATUS_INPUT_NOT_IN_FIELD, whatever the proof words hold, as in both contracts;
 *   5. otherwise the request is placed: ZKV_STATUS_OK or ZKV_STATUS_VERIFICATION_FAILED, as zkv_groth16_set_verify_batch decides.
 * A request that is not placed takes no slot and reaches no verifier.
 *
 * Return data by the key's form:             OK                        VERIFICATION_FAILED               INPUT_NOT_IN_FIELD
 *   snarkjs                                  not reverted, word 1      not reverted, word 0              not reverted, word 0
 *   gnark                                    not reverted, empty       reverted, ProofInvalid()          reverted, PublicInputNotInField()
 *
 * Device scratch, on top of zkv_groth16_set_verify_batch_dev's: 267 bytes per request and one signal row
 * (zkv_groth16_set_signal_stride) per request, plus 32 bytes per contract.
 */
#ifndef ZKV_GROTH16_SET_WIRE_H
#define ZKV_GROTH16_SET_WIRE_H
#include "zkv_groth16_set.h"

#ifdef __cplusplus
extern "C" {
#endif

#define ZKV_G16_FORM_SNARKJS 0
#define ZKV_G16_FORM_GNARK 1
#define ZKV_STATUS_NO_CONTRACT 9           /* deployed sets only: no contract at the address (not reverted, empty return data) */
#define ZKV_STATUS_INPUT_NOT_IN_FIELD 10   /* deployed sets only: a public signal >= r (gnark: PublicInputNotInField())          */

/* zkv_groth16_set_create with a 20-byte contract address and a form per key.  The result is an ordinary key set (zkv_ctx_vm answers
 * ZKV_VM_GROTH16_SET, every call of zkv_groth16_set.h works on it) that also answers the calls below; on a set made by
 * zkv_groth16_set_create those return ZKV_ERR_WRONG_CTX.  NULL on what zkv_groth16_set_create refuses, a NULL pointer, two keys with
 * one address, or a form that does not exist.  One key may be listed twice under two addresses. */
zkv_ctx* zkv_groth16_set_create_deployed(size_t n_keys, const uint8_t* const* vk_words, const size_t* n_ic, const int* vm_type,
                                         const uint8_t* addresses /* n_keys x 20 */, const uint8_t* form /* n_keys */, int device);
/* The function selector of a form's verifyProof with n_signals public signals (1 .. ZKV_GROTH16_MAX_IC - 1), derived as
 * zkv_abi_function_selector derives it.  Host only.  ZKV_ERR_INVALID_ARG for another form or count. */
int zkv_groth16_set_call_selector(int form, size_t n_signals, uint8_t out[4]);
/* Host buffers: request i = calldata_blob[calldata_off[i] .. calldata_off[i+1]) to the contract at to[20 i ..]; the blob is
 * calldata_blob[0 .. calldata_off[n]), so a request can run backwards or past it (rule 1).  The buffers are staged in device memory and
 * take the device-resident path.  reverted[n], returndata (n x ZKV_RETURNDATA_STRIDE) and returndata_len[n] as in zkv_eth_call_batch;
 * status may be NULL. */
int zkv_groth16_set_eth_call_batch(zkv_ctx* ctx, size_t n, const uint8_t* to, const uint8_t* calldata_blob, const uint64_t* calldata_off,
                                   uint8_t* reverted, uint8_t* returndata, uint32_t* returndata_len, uint8_t* status);
/* Device-resident, enqueued on `stream` (NULL: the context's): addresses, calldata and the n + 1 offsets in device memory,
 * calldata_bytes = size of d_calldata.  d_status[n] receives ZKV_STATUS_*; d_key (n x uint32, may be NULL) the key each address resolved
 * to, 0xFFFFFFFF where no contract answered or (rule 1) none was looked up.  Synchronises where zkv_groth16_set_verify_batch_dev does,
 * once, and at no other point. */
int zkv_groth16_set_eth_call_batch_dev(zkv_ctx* ctx, size_t n, const uint8_t* d_to, const uint8_t* d_calldata, const uint64_t* d_calldata_off,
                                       uint64_t calldata_bytes, uint8_t* d_status, uint32_t* d_key, void* stream);
/* Return / revert data of one status of a request that resolved to `key` (the table above).  ZKV_STATUS_NO_CONTRACT and
 * ZKV_STATUS_BAD_CALLDATA need no key (any value).  ZKV_ERR_INVALID_ARG for a status a deployed set does not report, or a key past the
 * set with a status that needs one.  Host only. */
int zkv_groth16_set_eth_call_returndata(const zkv_ctx* ctx, uint32_t key, uint8_t status, uint8_t out[ZKV_RETURNDATA_STRIDE], uint32_t* out_len,
                                        uint8_t* reverted);
/* Requests of the most recent eth_call batch: out = {placed, no contract, bad calldata, signal not in field}; zeros before the first.
 * Waits for that batch.  zkv_ctx_last_wire_ms gives its decode time. */
int zkv_groth16_set_last_call_counts(zkv_ctx* ctx, uint64_t out[4]);

#ifdef __cplusplus
}
#endif
#endif /* ZKV_GROTH16_SET_WIRE_H */

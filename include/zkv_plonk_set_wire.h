/*
 * zkv_plonk_set_wire.h -- eth_call batches on a PLONK key set whose keys are deployed gnark verifier contracts (one PlonkVerifier.sol per
 * circuit, each at its own address): raw `Verify` calldata, each request addressed to a contract, resolved, decoded, classified and
 * verified on the device, and answered with the contract's own return or revert data.  Companion of zkv_plonk_set.h (same library, same
 * conventions); DESIGN.md section 14b describes the device path.
 *
 * PARITY UNPINNED: the reference holds no PLONK code and no contract shell.  The contract is gnark's Solidity PLONK verifier,
 *   Verify(bytes proof, uint256[] public_inputs) returns (bool)
 * Both arguments are dynamic; only the canonical encoding passes, as in every other wire layer of this library:
 *   sel | 0x40 | 0x60 + pad32(Lp) | Lp | proof, zero padded to 32 | N' | N' words          4 + 96 + pad32(Lp) + 32 + 32 N' bytes
 * The proof bytes are the 32 (24 + 3 n_c) bytes of zkv_plonk_keys.h's layout and the input words the public-input row of
 * zkv_plonk_set_verify_batch, so a decoded call gets exactly what that call gives its key, proof row and input row.
 *
 * The rules of request i, in this order (nb, n_c and Lkey = 32 (24 + 3 n_c) belong to the resolved key):
 *   1. offsets that run backwards or past the calldata: ZKV_STATUS_BAD_CALLDATA, the request is never read (no key is resolved);
 *   2. to[i] is none of the set's addresses: ZKV_STATUS_NO_CONTRACT -- not reverted, empty return data, what an eth_call to an address
 *      without code answers;
 *   3. not the canonical encoding -- fewer than 4 + 128 bytes, another selector, an offset word other than shown, Lp or N' >= 2^32, an
 *      N' word outside the request, a total length other than shown (a byte missing or trailing): ZKV_STATUS_BAD_CALLDATA, reverted with
 *      empty data.  Padding bytes are not inspected: a request is only ever placed with Lp = 768 or 864, which has none.  A key with
 *      nb = 0 is callable, with an empty array;
 *   4. the contract's sanity checks in gnark's order, each reverting with its Error(string):
 *        N' != nb                                                     ZKV_PLONK_REVERT_INPUT_COUNT    "wrong number of public inputs"
 *        an input word >= r (only the nb words are ever looked at)    ZKV_PLONK_REVERT_INPUT_RANGE    "inputs are bigger than r"
 *        Lp != Lkey                                                   ZKV_PLONK_REVERT_PROOF_SIZE     "wrong proof size"
 *        proof word 12-16, 19 or (n_c = 1) 24 >= r                    ZKV_PLONK_REVERT_OPENING_RANGE  "openings bigger than r"
 *   5. one of the proof's points -- L R O H0 H1 H2 Z H_zeta H_zeta_omega at words 0 2 4 6 8 10 17 20 22, and the BSB22 commitment at
 *      word 25 when n_c = 1 -- is no input of the EC precompiles (a coordinate >= p, or off the curve; (0, 0) is infinity and passes):
 *      ZKV_PLONK_REVERT_EC_OPERATION "error ec operation";
 *   6. otherwise the request is placed: ZKV_STATUS_OK (not reverted, the word 1) or ZKV_STATUS_VERIFICATION_FAILED (not reverted, the
 *      word 0), as zkv_plonk_set_verify_batch decides.  An invalid key answers 0 for all its placed requests.  The zero-denominator
 *      cases of zkv_plonk_keys.h answer the word 0; what the contract does there (a modular inverse of zero) is not modelled.
 * A request that is not placed takes no slot and reaches no verifier.
 *
 * Two bytes per request: the status and the reason.  No new ZKV_STATUS_* number: the contract's revert causes travel in the reason.
 *   reason 2        ZKV_STATUS_INPUT_NOT_IN_FIELD (zkv_groth16_set_wire.h)
 *   reason 1 3 4 5  ZKV_STATUS_INVALID_PROOF_DATA
 *   reason 0        every other status (OK, VERIFICATION_FAILED, BAD_CALLDATA, NO_CONTRACT)
 * Revert data of a reason: 08c379a0 (Error(string)) | 0x20 | length | the message, zero padded to 32 -- 100 bytes each.
 *
 * Not modelled: gnark template versions with another proof layout, n_c > 1, addresses added after creation, proxies, and the reverts
 * "error pairing" / "error mod exp", which cannot occur with a valid key.
 *
 * Device scratch, on top of zkv_plonk_set_verify_batch_dev's: per request one proof row (zkv_plonk_set_proof_stride), one input row
 * (zkv_plonk_set_input_stride) and 13 bytes, plus 32 bytes per contract.
 */
#ifndef ZKV_PLONK_SET_WIRE_H
#define ZKV_PLONK_SET_WIRE_H
#include "zkv_plonk_set.h"
#include "zkv_groth16_set_wire.h"   /* ZKV_STATUS_NO_CONTRACT (9), ZKV_STATUS_INPUT_NOT_IN_FIELD (10) */

#ifdef __cplusplus
extern "C" {
#endif

#define ZKV_PLONK_REVERT_NONE 0
#define ZKV_PLONK_REVERT_INPUT_COUNT 1       /* Error("wrong number of public inputs")  29 bytes */
#define ZKV_PLONK_REVERT_INPUT_RANGE 2       /* Error("inputs are bigger than r")       24 bytes */
#define ZKV_PLONK_REVERT_PROOF_SIZE 3        /* Error("wrong proof size")               16 bytes */
#define ZKV_PLONK_REVERT_OPENING_RANGE 4     /* Error("openings bigger than r")         22 bytes */
#define ZKV_PLONK_REVERT_EC_OPERATION 5      /* Error("error ec operation")             18 bytes */
#define ZKV_PLONK_RETURNDATA_STRIDE 128      /* Error(string) with a message of up to 32 bytes is 100 bytes */

/* zkv_plonk_set_create with a 20-byte contract address per key.  The result is an ordinary PLONK set (zkv_ctx_vm answers
 * ZKV_VM_PLONK_SET, every call of zkv_plonk_set.h works on it) that also answers the calls below; on a set made by zkv_plonk_set_create
 * those return ZKV_ERR_WRONG_CTX.  NULL on what zkv_plonk_set_create refuses, a NULL pointer, or two keys with one address.  One key may
 * be listed twice under two addresses. */
zkv_ctx* zkv_plonk_set_create_deployed(size_t n_keys, const uint8_t* const* vk_bytes, const size_t* vk_len, const uint8_t* addresses /* n_keys x 20 */,
                                       int device);
/* The function selector of Verify(bytes,uint256[]), derived as zkv_abi_function_selector derives it.  Host only. */
int zkv_plonk_set_call_selector(uint8_t out[4]);
/* Host buffers: request i = calldata_blob[calldata_off[i] .. calldata_off[i+1]) to the contract at to[20 i ..]; the blob is
 * calldata_blob[0 .. calldata_off[n]), so a request can run backwards or past it (rule 1).  The buffers are staged in device memory and
 * take the device-resident path.  reverted[n], returndata (n x ZKV_PLONK_RETURNDATA_STRIDE) and returndata_len[n]; status and reason
 * (n bytes each) may be NULL. */
int zkv_plonk_set_eth_call_batch(zkv_ctx* ctx, size_t n, const uint8_t* to, const uint8_t* calldata_blob, const uint64_t* calldata_off,
                                 uint8_t* reverted, uint8_t* returndata, uint32_t* returndata_len, uint8_t* status, uint8_t* reason);
/* Device-resident, enqueued on `stream` (NULL: the context's): addresses, calldata and the n + 1 offsets in device memory,
 * calldata_bytes = size of d_calldata.  d_status[n] receives ZKV_STATUS_*; d_reason (n bytes, may be NULL) ZKV_PLONK_REVERT_*; d_key
 * (n x uint32, may be NULL) the key each address resolved to, 0xFFFFFFFF where no contract answered or (rule 1) none was looked up.
 * Synchronises where zkv_plonk_set_verify_batch_dev does, once, and at no other point. */
int zkv_plonk_set_eth_call_batch_dev(zkv_ctx* ctx, size_t n, const uint8_t* d_to, const uint8_t* d_calldata, const uint64_t* d_calldata_off,
                                     uint64_t calldata_bytes, uint8_t* d_status, uint8_t* d_reason, uint32_t* d_key, void* stream);
/* Return / revert data of one (status, reason) pair.  Host only, no context.  ZKV_ERR_INVALID_ARG for a pair a deployed PLONK set never
 * reports, or a NULL pointer. */
int zkv_plonk_set_eth_call_returndata(uint8_t status, uint8_t reason, uint8_t out[ZKV_PLONK_RETURNDATA_STRIDE], uint32_t* out_len, uint8_t* reverted);
/* Requests of the most recent eth_call batch: out = {placed, no contract, bad calldata, reason 1, reason 2, reason 3, reason 4,
 * reason 5}; zeros before the first.  Waits for that batch.  zkv_ctx_last_wire_ms gives the time of its decode and point kernels. */
int zkv_plonk_set_last_call_counts(zkv_ctx* ctx, uint64_t out[8]);

#ifdef __cplusplus
}
#endif
#endif /* ZKV_PLONK_SET_WIRE_H */

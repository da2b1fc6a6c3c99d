/*
 * zkv_diag_prep.h -- read-back of the public signals the PREP stage derived.  TEST ONLY: no verification path uses it.
 *
 * The SHA-256 chains of the first kernel (SP1: sha256(public_values) & (2^253 - 1); RISC Zero: the two halves of the claim digest) are
 * otherwise visible only through ACCEPT / REJECT.  This reader copies out what the shipped kernel stored for the vk_x stage; it launches
 * nothing and no verify kernel knows of it.  Companion of zkv.h (same library, same ZKV_OK / ZKV_ERR_* codes).
 */
#ifndef ZKV_DIAG_PREP_H
#define ZKV_DIAG_PREP_H
#include "zkv.h"

#ifdef __cplusplus
extern "C" {
#endif

#define ZKV_DIAG_PREP_SIGNALS 5          /* signal rows per proof (RISC Zero and SP1 fill the first two) */

/* Synchronous.  After a batch call on a single-device RISC Zero or SP1 Groth16 context (also the child contexts of a mixed batch,
 * zkv_mixed_ctx_risc0 / zkv_mixed_ctx_sp1, and the Groth16 route of a gateway, zkv_sp1_gateway_route_ctx: proof j of a child is the
 * j-th proof of the batch that went to it, the partition being stable), waits for that call and copies out, for the first n proofs of
 * its MOST RECENT CHUNK (ZKV_CHUNK proofs; a batch of at most one chunk is its own last chunk):
 *   flags[j]                         the proof's flags word as the stages left it; 0 = PREP rejected the proof before or at point
 *                                    validation and stored NO signals for it (the row then holds an earlier proof's values);
 *   signals[(5 j + b) * 8 + k]       limb k (little-endian uint32, raw integer, not Montgomery) of signal b of proof j:
 *                                    SP1: b = 0 the program vkey, b = 1 the public-values digest; RISC Zero: b = 0, 1 the low and high
 *                                    128 bits of the byte-reversed claim digest; the other rows are zero.
 * ZKV_ERR_INVALID_ARG (checked on the host before anything else): NULL ctx or buffer, a context that is not ZKV_VM_RISC0 / ZKV_VM_SP1,
 * a sharded context, a context with the aggregate check switched on (its chunks keep other rows), n = 0, or -- once a device is known
 * to be there -- n beyond the last chunk's proof count.  ZKV_ERR_NO_DEVICE without a gfx950 device. */
int zkv_diag_prep_signals(zkv_ctx* ctx, size_t n, uint32_t* signals, uint32_t* flags);

#ifdef __cplusplus
}
#endif
#endif /* ZKV_DIAG_PREP_H */

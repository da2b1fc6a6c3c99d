/*
 * zkv_groth16_set.h -- Groth16 key sets: many verification keys behind one context, the key chosen per proof.
 *
 * The batch form of `Groth16Verifier::verify_proof_with_key(vm_type, &vk, proof, signals)` (common/groth16.rs:23-49) with a key
 * per proof: proof i is verified against key key[i] of the set.  Companion of zkv.h (same library, same conventions, same
 * ZKV_OK / ZKV_ERR_* codes); DESIGN.md section 11 describes the device pipeline.
 *
 *   - A set is immutable and single-device (zkv_ctx_create_sharded refuses it).  zkv_ctx_vm returns ZKV_VM_GROTH16_SET.
 *   - zkv_ctx_destroy / _synchronize / _reserve / _set_lanes_per_proof / _last_stage_ms work as on other contexts.
 *   - zkv_ctx_set_aggregate_check works on a set as on other contexts: enable = 1 automatic size, 16 / 32 / 64 / 128 / 256 a fixed
 *     size, 0 off; the same secret and rekey rules.  zkv_ctx_aggregate_counters counts the set's sub-batches (checked, and failed then
 *     verified proof by proof).  The check engages for a call only when the mapping is automatic (lanes 0), the call places at least
 *     ZKV_AGG_MIN proofs and the aggregate buffers could be allocated; otherwise the call runs the per-proof path unchanged.
 *     A key is aggregate-capable when it is valid and alpha and beta are finite; all proofs of other keys, and of keys past the set,
 *     take the per-proof path or answer 0 as without the check.  Every sub-batch holds proofs of one key (the equation uses that key's
 *     alpha, beta, gamma and delta).  Statuses are the per-proof ones.  The first call with the check on allocates every key's
 *     aggregate tables: about 0.53 MB per key (0.5 GB for 1,024 keys), plus 224 B of rows per proof in flight and the pseudo-proofs'
 *     workspace; with the check off (the default) nothing is allocated.
 *   - Proofs are 256 bytes each, as for zkv_groth16_verify_batch.  Signals are rows of zkv_groth16_set_signal_stride bytes:
 *     the first n_ic[k] - 1 32-byte big-endian words of row i are proof i's signals; the words after them are never read.
 * Alignment: byte-typed buffers (uint8_t*), host or device, may have any alignment; uint32_t* / uint64_t* arguments need their natural one.
 */
#ifndef ZKV_GROTH16_SET_H
#define ZKV_GROTH16_SET_H
#include "zkv.h"

#ifdef __cplusplus
extern "C" {
#endif

#define ZKV_VM_GROTH16_SET 7
#define ZKV_GROTH16_SET_MAX_KEYS 1024

/* vk_words[k]: key k in zkv_groth16_ctx_create's layout; 1 <= n_ic[k] <= ZKV_GROTH16_MAX_IC; vm_type[k] = ZKV_VM_RISC0 / ZKV_VM_SP1.
 * NULL on any bad argument (0 or > MAX keys, n_ic out of range, bad vm_type, NULL pointers).  Copies the keys; the device is set up
 * lazily (about 3.6 MB of tables per key plus 512 KB per signal). */
zkv_ctx* zkv_groth16_set_create(size_t n_keys, const uint8_t* const* vk_words, const size_t* n_ic, const int* vm_type, int device);
size_t   zkv_groth16_set_size(const zkv_ctx* ctx);            /* number of keys; 0 for a context that is not a set */
size_t   zkv_groth16_set_signal_stride(const zkv_ctx* ctx);   /* bytes per proof in `signals` = 32 * (max_k n_ic[k] - 1), may be 0 */
int      zkv_groth16_set_key_n_ic(const zkv_ctx* ctx, size_t key);    /* n_ic of key `key`, ZKV_ERR_INVALID_ARG past the set */

/* verified[i] = verify_proof_with_key(vm_type[k], vk[k], proof i, first n_ic[k] - 1 signals of row i) for k = key[i] < n_keys;
 * 0 for key[i] >= n_keys (never handed to a verifier).  Signal words past n_ic[k] - 1 in a row are ignored, whatever their value. */
int zkv_groth16_set_verify_batch(zkv_ctx* ctx, size_t n, const uint32_t* key, const uint8_t* proofs, const uint8_t* signals, uint8_t* verified);
/* The same with every buffer in device memory, enqueued on `stream` (NULL: the context's).  The call reads the per-key proof counts
 * back once (a synchronisation with `stream` up to the partition); the verification itself is asynchronous. */
int zkv_groth16_set_verify_batch_dev(zkv_ctx* ctx, size_t n, const uint32_t* d_key, const uint8_t* d_proofs, const uint8_t* d_signals,
                                     uint8_t* d_verified, void* stream);
/* compute_vk_x (groth16.rs:51-58) of row i under key key[i]: out[i] = 64 bytes (x, y big-endian; (0, 0) = infinity).
 * ZKV_ERR_INVALID_ARG when any key[i] >= n_keys. */
int zkv_groth16_set_vk_x_batch(zkv_ctx* ctx, size_t n, const uint32_t* key, const uint8_t* signals, uint8_t* out /* n x 64 */);

#ifdef __cplusplus
}
#endif
#endif /* ZKV_GROTH16_SET_H */

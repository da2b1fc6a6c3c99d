/*
 * zkv_plonk_set.h -- PLONK key sets: many gnark BN254 PLONK keys behind one context, the key chosen per proof.
 *
 * The batch form of zkv_plonk_verify_batch (zkv_plonk_keys.h) with a key per proof: proof i is verified against key key[i] of the set.
 * Companion of zkv.h (same library, same conventions, same ZKV_OK / ZKV_ERR_* codes); DESIGN.md section 14 describes the device path.
 * PARITY UNPINNED BY CONSTRUCTION: the reference holds no PLONK code; every verdict is oracle/plonk_model.py's plonk_verify.
 *
 *   - Every key is in zkv_plonk_ctx_create's layout and obeys its rules (992 or 1,056 bytes to match n_c, n_c <= 1, nb_public <=
 *     ZKV_PLONK_MAX_PUBLIC, ...).  A key holding an invalid point or a size_inv / generator / coset_shift >= R is accepted, and every
 *     proof against it answers 0; the other keys' proofs are unaffected.
 *   - A set is immutable and single-device (zkv_ctx_create_sharded refuses it).  zkv_ctx_vm returns ZKV_VM_PLONK_SET.
 *   - zkv_ctx_destroy / _synchronize / _reserve / _set_lanes_per_proof / _last_stage_ms work as on other contexts.
 *   - zkv_ctx_set_aggregate_check works on a set: sub-batches run across the keys of one SRS (keys with equal [1]_2 | [tau]_2 bytes);
 *     zkv_plonk_set_agg.h states the contract.  Before the first call that engages it zkv_ctx_aggregate_counters is {0, 0}.
 *   - zkv_ctx_vk_x_batch and every other kind's entry points return ZKV_ERR_WRONG_CTX on a set, and the entry points below return it
 *     on every other kind.
 *   - Proofs are rows of zkv_plonk_set_proof_stride bytes: row i holds key[i]'s 32 (24 + 3 n_c) proof bytes (zkv_plonk_keys.h's layout)
 *     first; the bytes after them are never read.  Public inputs are rows of zkv_plonk_set_input_stride bytes: the first nb_public
 *     32-byte big-endian words of row i are proof i's inputs; the words after them are never read.
 *   - Device memory: about 24 MB per key (the key points' window tables: 6.2 GB for 256 keys) and 3.6 MB of line tables per key, set
 *     up lazily on the first batch or zkv_ctx_reserve; per proof in flight 3.7 KB of workspace and 3.75 KB of MSM tables, and per
 *     call the slot tables of the partition by key.
 * Alignment: byte-typed buffers (uint8_t*), host or device, may have any alignment; uint32_t* / uint64_t* arguments need their natural one.
 */
#ifndef ZKV_PLONK_SET_H
#define ZKV_PLONK_SET_H
#include "zkv.h"

#ifdef __cplusplus
extern "C" {
#endif

#define ZKV_VM_PLONK_SET 10
#define ZKV_PLONK_SET_MAX_KEYS 256

/* vk_bytes[k], vk_len[k]: key k in zkv_plonk_ctx_create's layout.  NULL when n_keys is 0 or above ZKV_PLONK_SET_MAX_KEYS, a pointer is
 * NULL, or any key breaks zkv_plonk_ctx_create's rules.  Copies the keys; the device is set up lazily. */
zkv_ctx* zkv_plonk_set_create(size_t n_keys, const uint8_t* const* vk_bytes, const size_t* vk_len, int device);
size_t   zkv_plonk_set_size(const zkv_ctx* ctx);           /* number of keys; 0 for a context that is not a PLONK set */
size_t   zkv_plonk_set_proof_stride(const zkv_ctx* ctx);   /* bytes per proof row = 32 (24 + 3 max_k n_c[k]): 768 or 864 */
size_t   zkv_plonk_set_input_stride(const zkv_ctx* ctx);   /* bytes per public-input row = 32 max_k nb_public[k]; may be 0 */
/* nb_public, n_c and proof length in bytes of key `key` (any pointer may be NULL); ZKV_ERR_INVALID_ARG past the set. */
int      zkv_plonk_set_key_shape(const zkv_ctx* ctx, size_t key, size_t* nb_public, size_t* n_commitments, size_t* proof_bytes);

/* verified[i] = plonk_verify(key key[i], proof row i, public-input row i) for key[i] < n_keys; 0 for key[i] >= n_keys.  `public_inputs`
 * may be NULL when the input stride is 0.  Synchronous; the inputs are staged in chunks of at most 512 MB of public inputs. */
int zkv_plonk_set_verify_batch(zkv_ctx* ctx, size_t n, const uint32_t* key, const uint8_t* proofs, const uint8_t* public_inputs,
                               uint8_t* verified);
/* The same with every buffer in device memory, enqueued on `stream` (NULL: the context's).  The call reads the per-key proof counts
 * back once (a synchronisation with `stream` up to the partition); the verification itself is asynchronous. */
int zkv_plonk_set_verify_batch_dev(zkv_ctx* ctx, size_t n, const uint32_t* d_key, const uint8_t* d_proofs, const uint8_t* d_public_inputs,
                                   uint8_t* d_verified, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* ZKV_PLONK_SET_H */

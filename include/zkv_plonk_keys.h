/*
 * zkv_plonk_keys.h -- PLONK core for any gnark BN254 verifying key: up to 128 public inputs, with or without one BSB22 commitment.
 *
 * The PLONK counterpart of zkv_groth16_ctx_create: the caller's key, the caller's public inputs, a verdict per proof.  Companion of
 * zkv.h (same library, same conventions, same ZKV_OK / ZKV_ERR_* codes); DESIGN.md section 13 describes the device path.
 * PARITY UNPINNED BY CONSTRUCTION: the reference holds no PLONK code; the algorithm is gnark's published BN254 PLONK verifier, restated
 * in oracle/plonk_model.py (plonk_verify), which defines every verdict below.
 *
 * Key: the layout of zkv_sp1_plonk_ctx_create (zkv.h), 32-byte big-endian words: size | size_inv | generator | coset_shift | nb_public |
 * n_c | cci (commitment constraint index), then S1 S2 S3 Ql Qr Qm Qo Qk (G1 x, y), then Qcp only when n_c = 1, then [1]_2 and [tau]_2
 * (EIP-197 order).  992 bytes for n_c = 0, 1,056 for n_c = 1.  zkv_plonk_ctx_create returns NULL when the length does not match n_c,
 * n_c > 1, nb_public > ZKV_PLONK_MAX_PUBLIC, size >= 2^64, cci >= 2^32, or a high limb of nb_public / n_c / cci is nonzero.
 * nb_public = 0 is allowed.  A key holding an invalid point (G1 not a precompile input, G2 off the curve or outside the subgroup) or a
 * size_inv / generator / coset_shift >= R is accepted, and every proof against it answers 0 (as for SP1 PLONK keys).
 *
 * Proof: the MarshalSolidity words without a selector, 24 + 3 n_c words = 768 or 864 bytes:
 *   L R O H0 H1 H2 (words 0-11) | l r o s1 s2 (12-16) | Z (17-18) | zu (19) | H_zeta (20-21) | H_zeta_omega (22-23)
 *   | n_c = 1 only: qcp(zeta) (24) and the BSB22 commitment (25-26).
 * Public inputs: nb_public 32-byte big-endian words per proof.
 *
 * Verdict 1 exactly when plonk_verify accepts.  0 when: a public input >= R; a scalar word (12-16, 19, and 24 when n_c = 1) >= R; a point
 * coordinate >= P or a point off the curve ((0, 0) is infinity); a zero denominator -- zeta = 1, zeta = omega^i for some i < nb_public,
 * or (n_c = 1) zeta = omega^(nb_public + cci); the pairing check fails.  With n_c = 0 no word past 23 exists and none is read.
 *
 *   - zkv_ctx_vm returns ZKV_VM_PLONK.  zkv_ctx_destroy / _synchronize / _reserve / _set_lanes_per_proof / _set_aggregate_check /
 *     _aggregate_counters / _last_stage_ms work as on SP1 PLONK contexts (the aggregate check engages under the same conditions).
 *   - zkv_ctx_vk_x_batch and every SP1, SP1 PLONK and gateway entry point return ZKV_ERR_WRONG_CTX on this kind, and the entry points
 *     below return it on every other kind.
 *   - zkv_ctx_create_sharded accepts shards of this kind with identical keys; batches split by range.
 *   - Device memory: about 24 MB per context (the key points' window tables) plus the line tables of the two G2 points; per proof in
 *     flight 3.7 KB of workspace and 3.75 KB of MSM tables (7.5 KB), and for host batches the staged proofs and public inputs
 *     (proof_bytes + 32 nb_public bytes).  Host batches run in chunks of at most 512 MB of staged public inputs (2^17 proofs at 128
 *     inputs); device batches in chunks of the workspace (default up to 2^20 proofs, ZKV_CHUNK).
 * Alignment: byte-typed buffers (uint8_t*), host or device, may have any alignment; uint32_t* / uint64_t* arguments need their natural one.
 */
#ifndef ZKV_PLONK_KEYS_H
#define ZKV_PLONK_KEYS_H
#include "zkv.h"

#ifdef __cplusplus
extern "C" {
#endif

#define ZKV_VM_PLONK 9
#define ZKV_PLONK_MAX_PUBLIC 128

/* Copies the key; the device is set up lazily, on the first batch or zkv_ctx_reserve.  NULL on the rules above. */
zkv_ctx* zkv_plonk_ctx_create(const uint8_t* vk_bytes, size_t vk_len, int device);
/* nb_public, n_c and the proof length in bytes (32 (24 + 3 n_c)); any pointer may be NULL.  ZKV_ERR_WRONG_CTX on another kind. */
int      zkv_plonk_key_shape(const zkv_ctx* ctx, size_t* nb_public, size_t* n_commitments, size_t* proof_bytes);
/* proofs: n x proof_bytes; public_inputs: n x nb_public x 32 bytes big-endian (may be NULL when nb_public = 0); verified[i] = 1 / 0.
 * Synchronous. */
int zkv_plonk_verify_batch(zkv_ctx* ctx, size_t n, const uint8_t* proofs, const uint8_t* public_inputs, uint8_t* verified);
/* The same with every buffer in device memory, enqueued on `stream` (NULL: the context's); no synchronisation. */
int zkv_plonk_verify_batch_dev(zkv_ctx* ctx, size_t n, const uint8_t* d_proofs, const uint8_t* d_public_inputs,
                               uint8_t* d_verified, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* ZKV_PLONK_KEYS_H */

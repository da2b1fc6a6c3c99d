/*
 * zkv_risc0_set_inclusion.h -- RISC Zero set-inclusion receipts: many claims behind one root seal.
 *
 * In RISC Zero's aggregation flow (the set-builder guest, `RiscZeroSetVerifier` on chain) ONE Groth16 seal proves a Merkle root, and each
 * of the claims under it carries only a keccak-256 Merkle path to that root.  The root seal travels with the claim, or it was submitted
 * once and the root is remembered.  This companion of zkv.h (same library, same conventions) verifies batches of such claims: the paths
 * are hashed on the device, one claim per lane, the claims that share a root seal share one pairing check, and the root checks run on the
 * library's own RISC Zero / generic Groth16 contexts.  DESIGN.md section 16 describes the device path.
 *
 * PARITY UNPINNED: the reference holds no set verifier.  The rules below are this project's definition, modelled on RISC Zero's Solidity
 * set verifier and OpenZeppelin's MerkleProof.processProof; agreement is between tests/set_inclusion_model.py, a host build of the device
 * math (csrc/zkv_setincl.h) and the device.
 *
 * Rules.  ID = the set-builder image id (32 bytes, fixed at creation).  V = the inner root verifier, a `RiscZeroVerifier`
 * (risc0/verifier.rs) with (control_root, bn254_control_id).
 *   claim_digest = ReceiptClaim::ok(image_id, journal_digest).digest() (risc0/types.rs:44-94) for `verify`, given for `verify_integrity`
 *   leaf         = keccak256("LEAF_TAG" || claim_digest)                       (8 ASCII bytes + 32)
 *   node(a, b)   = keccak256(min(a, b) || max(a, b))                            (32-byte big-endian integers; equal values allowed)
 *   root_i       = fold of node over claim i's path from its leaf; a path of depth 0 gives root_i = leaf
 *   - a claim that names root seal S: status and received selector are exactly those of V.verify(S, ID, sha256(ID || root_i));
 *   - a claim that names no root seal (root index ZKV_SETINCL_STORED): ZKV_STATUS_OK if root_i is among the submitted roots of the
 *     context, else ZKV_STATUS_VERIFICATION_FAILED;
 *   - library limits, answered ZKV_STATUS_INVALID_PROOF_DATA without any seal being verified for the claim: a path deeper than
 *     ZKV_SETINCL_MAX_DEPTH, a root index >= m that is not ZKV_SETINCL_STORED (and, in the device-resident call, path offsets that run
 *     backwards or leave the blob).
 * Claims that name the same root seal are grouped: the lowest-index claim naming it is the group's representative and its root is verified
 * once; a claim whose root differs from its representative's (a "straggler") is verified on its own with the same seal and its own root.
 * Every status therefore is the per-claim one whatever the caller files under one seal, and an honest batch pays one pairing check per
 * root seal.  Batches run in chunks of at most 2^20 claims; a group that spans chunks is verified once per chunk.
 *
 * On-chain form of a set-inclusion seal: set_selector || abi.encode(Seal{bytes32[] path; bytes rootSeal}), where
 * set_selector = first 4 bytes of tagged_struct(sha256("risc0.SetInclusionReceiptVerifierParameters"), [ID]) (risc0/crypto.rs
 * tagged_struct).  The body is the word 0x20, the two offsets (0x40 and 0x60 + 32 * len(path)), the path (length word + elements), the
 * root seal (length word + bytes zero-padded to a word).  Only this canonical encoding decodes.
 *
 * Generic calls of zkv.h on a set-inclusion context: zkv_ctx_destroy, zkv_ctx_synchronize, zkv_ctx_vm, zkv_ctx_reserve and
 * zkv_ctx_set_lanes_per_proof (both forwarded to the inner verifier) and zkv_ctx_last_stage_ms ([0]: the hash kernel of the most recent
 * chunk, [1] .. [4]: those stages of the inner verifier's most recent root jobs, zero when the call ran none) work; every batch entry point of another kind returns ZKV_ERR_WRONG_CTX.  Single-device: a set-inclusion context cannot be sharded.
 */
#ifndef ZKV_RISC0_SET_INCLUSION_H
#define ZKV_RISC0_SET_INCLUSION_H
#include "zkv.h"

#ifdef __cplusplus
extern "C" {
#endif

#define ZKV_VM_RISC0_SETINCL 11
#define ZKV_SETINCL_MAX_DEPTH 64
#define ZKV_SETINCL_STORED 0xFFFFFFFFu      /* root index of a claim whose root is looked up among the submitted roots */
#define ZKV_SETINCL_MAX_ROOTS 4096          /* submitted roots a context keeps */

/* The inner verifier is a built-in RISC Zero context (the key of risc0/crypto.rs:16-89).  NULL on NULL pointers. */
zkv_ctx* zkv_risc0_setincl_create(const uint8_t control_root[32], const uint8_t bn254_control_id[32],
                                  const uint8_t set_builder_image_id[32], int device);
/* The same rules with a caller-supplied Groth16 key for the root proofs (forks, dev-mode keys, tests that need valid root proofs):
 * vk_words is a key with n_ic = 6 in the layout and word order of the generic-key creator of zkv.h (832 bytes), verified in the RISC Zero
 * convention (A negated); root_selector is what V.get_selector would answer.  The front checks of V (length, selector) are made by the
 * job kernel, the five signals are the control-root halves, the two halves of the claim digest and the control id; a failing pairing,
 * a malformed point or a signal >= R give ZKV_STATUS_VERIFICATION_FAILED.  A key holding an invalid point is accepted and fails every root. */
zkv_ctx* zkv_risc0_setincl_create_keyed(const uint8_t* vk_words, const uint8_t root_selector[4], const uint8_t control_root[32],
                                        const uint8_t bn254_control_id[32], const uint8_t set_builder_image_id[32], int device);

/* `verify` over a batch, host buffers.  Claim i: image_ids / journal_digests n x 32 bytes; its path is siblings
 * path_off[i] .. path_off[i + 1] of path_blob (32 bytes each; n + 1 ascending offsets in SIBLING units, else ZKV_ERR_INVALID_ARG);
 * root_idx[i] names root seal j < m, or is ZKV_SETINCL_STORED.  Root seal j = root_seal_blob[root_seal_off[j] .. root_seal_off[j + 1])
 * (any length: V answers a seal that is not 260 bytes as `RiscZeroVerifier` does); m may be 0 (the two pointers may then be NULL).
 * status[n] receives ZKV_STATUS_*; recv_selector (n x 4, may be NULL) the selector found in the root seal for SELECTOR_MISMATCH entries
 * (zero otherwise).  At most 2^24 root seals and 2^32 - 1 siblings per call. */
int zkv_risc0_setincl_verify_batch(zkv_ctx* ctx, size_t n, const uint8_t* image_ids, const uint8_t* journal_digests,
                                   const uint8_t* path_blob, const uint32_t* path_off, const uint32_t* root_idx, size_t m,
                                   const uint8_t* root_seal_blob, const uint64_t* root_seal_off, uint8_t* status, uint8_t* recv_selector);
/* `verify_integrity` over a batch: the claim digests are given. */
int zkv_risc0_setincl_verify_integrity_batch(zkv_ctx* ctx, size_t n, const uint8_t* claim_digests,
                                             const uint8_t* path_blob, const uint32_t* path_off, const uint32_t* root_idx, size_t m,
                                             const uint8_t* root_seal_blob, const uint64_t* root_seal_off, uint8_t* status, uint8_t* recv_selector);
/* Everything resident in HBM (device pointers): d_root_seals holds m rows of ZKV_SEAL_BYTES bytes, d_path_blob n_siblings x 32 bytes (no
 * claim's offsets are followed beyond it).  d_journal_digests = NULL selects `verify_integrity`, d_image_ids then holds the claim digests.
 * `stream` is a hipStream_t (NULL = the context's own).  NOT fully asynchronous: the call SYNCHRONISES ITS STREAM once per chunk of 2^20
 * claims, after the hash and grouping kernels, to read the chunk's job count (4 bytes) back; the root jobs, the scatter of their statuses
 * and everything of the last chunk after that point are enqueued without waiting -- the stream or zkv_ctx_synchronize tells when
 * d_status / d_recv_selector are written. */
int zkv_risc0_setincl_verify_batch_dev(zkv_ctx* ctx, size_t n, const uint8_t* d_image_ids, const uint8_t* d_journal_digests,
                                       const uint8_t* d_path_blob, const uint32_t* d_path_off, size_t n_siblings, const uint32_t* d_root_idx,
                                       size_t m, const uint8_t* d_root_seals, uint8_t* d_status, uint8_t* d_recv_selector, void* stream);

/* *status = V.verify(seal, ID, sha256(ID || root)); the root is remembered when that is ZKV_STATUS_OK (resubmitting a remembered root
 * is ZKV_STATUS_OK again).  recv_selector (may be NULL) as above.  A context keeps at most ZKV_SETINCL_MAX_ROOTS roots: beyond that
 * the call returns ZKV_ERR_INVALID_ARG and remembers nothing.  Blocks until the seal is verified. */
int zkv_risc0_setincl_submit_root(zkv_ctx* ctx, const uint8_t root[32], const uint8_t* seal, size_t seal_len, uint8_t* status,
                                  uint8_t recv_selector[4]);
/* 1 / 0: the root has been submitted; negative on a wrong context */
int zkv_risc0_setincl_has_root(zkv_ctx* ctx, const uint8_t root[32]);
/* set_selector of the on-chain form */
int zkv_risc0_setincl_get_selector(const zkv_ctx* ctx, uint8_t out[4]);
/* Counts of the most recent batch call: out[0] claims, out[1] root-seal verifications actually run (jobs: groups and stragglers, over
 * all chunks), out[2] stored-root lookups.  Synchronises the device. */
int zkv_risc0_setincl_last_counts(zkv_ctx* ctx, uint64_t out[3]);

/* Host only.  The on-chain form of one seal: returns the length needed; writes only when out != NULL and cap is large enough. */
size_t zkv_risc0_setincl_seal_encode(const zkv_ctx* ctx, const uint8_t* path, size_t path_len, const uint8_t* root_seal, size_t root_seal_len,
                                     uint8_t* out, size_t cap);
/* Host only.  *status = ZKV_STATUS_INVALID_PROOF_DATA for a seal shorter than 4 bytes or one whose body is not the canonical encoding,
 * ZKV_STATUS_SELECTOR_MISMATCH (recv_selector = its first 4 bytes) for another selector, else ZKV_STATUS_OK with the path as path_len
 * siblings from byte path_at of `seal` and the root seal as root_seal_len bytes from byte root_seal_at (nothing is copied). */
int zkv_risc0_setincl_seal_decode(const zkv_ctx* ctx, const uint8_t* seal, size_t seal_len, uint8_t* status, uint8_t recv_selector[4],
                                  size_t* path_at, size_t* path_len, size_t* root_seal_at, size_t* root_seal_len);

/* ------------------------------------------------------------------ diagnostics
 * Test only: runs the hash kernel alone on host buffers (arguments as the host batch calls; journal_digests = NULL: the first row holds
 * claim digests) and returns root_i, n x 32 bytes -- 32 zero bytes for a claim past ZKV_SETINCL_MAX_DEPTH, which is never read.  The
 * path blob is staged blob_shift (0 .. 31) bytes past a 256-byte aligned device address, so that both load paths of the kernel can be
 * reached.  No seal is verified. */
int zkv_diag_setincl_roots(zkv_ctx* ctx, size_t n, const uint8_t* image_ids, const uint8_t* journal_digests, const uint8_t* path_blob,
                           const uint32_t* path_off, size_t blob_shift, uint8_t* out_roots);

#ifdef __cplusplus
}
#endif
#endif /* ZKV_RISC0_SET_INCLUSION_H */

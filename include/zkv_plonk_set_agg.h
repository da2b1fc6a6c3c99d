/*
 * zkv_plonk_set_agg.h -- the aggregate check on PLONK key sets, shared by every key of one SRS.
 *
 * Companion of zkv_plonk_set.h (same library, same conventions, same ZKV_OK / ZKV_ERR_* codes); DESIGN.md section 14a describes the device
 * path.  PARITY UNPINNED BY CONSTRUCTION: the reference holds no PLONK code; every verdict is oracle/plonk_model.py's plonk_verify, with
 * the check on as with it off.
 *
 * A PLONK key gives the pairing equation e(D, [1]_2) e(-Q, [tau]_2) == 1 nothing but its two G2 points, and those are the SRS: keys whose
 * [1]_2 | [tau]_2 bytes (the last 256 of the key) are equal form an SRS CLASS, and a sub-batch may hold proofs of any keys of one class.
 *
 *   - zkv_ctx_set_aggregate_check (zkv.h) on a PLONK set: a call verifies the pairing equation per sub-batch of 16 ... 256 slots under
 *     secret 128-bit coefficients, every sub-batch inside one class; a failed sub-batch is verified again proof by proof on the proofs'
 *     own points.  The verdicts are the ones the call gives with the check off (up to 2^-128 over the coefficients).  Everything per proof
 *     that is not the pairing equation stays per proof and deterministic: transcript, range and curve checks, MSMs, zero denominators,
 *     invalid keys.
 *   - It engages when the check is on, the Miller mapping is automatic (zkv_ctx_set_lanes_per_proof 0) and the call -- for the host entry:
 *     the staged chunk -- places at least ZKV_AGG_MIN proofs (environment, default 131072).  Otherwise the call runs the per-proof path and
 *     the counters do not move.  Host entry and device entry (caller's stream) both take it.
 *   - Classes are formed at zkv_plonk_set_create by byte equality.  A class is CAPABLE when its two G2 points pass the set-up validation.
 *     Keys of a class that is not capable take the per-proof path (and answer 0).  A key with valid G2 points but an invalid point or
 *     header word of its own keeps answering 0 without PREP and contributes nothing to any sum.
 *   - Layout: key groups stay on 64-slot boundaries, ordered class by class; every class region starts on a multiple of A = max(64, sub)
 *     slots, and a sub-batch is `sub` consecutive slots of a class region whatever keys they belong to.  Pad slots, proofs PREP rejected,
 *     proofs of failed keys and key indices past the set are dead lanes: they contribute nothing and keep their status.  With many small
 *     keys most lanes are pads (256 keys x 16 proofs: three quarters); the sums skip them.  A sub-batch with nothing alive is switched
 *     off (it still counts as checked).
 *   - Coefficients, re-keying of an OS-drawn secret, the zero-coefficient rule, the automatic sub-batch size and the meaning of
 *     zkv_ctx_aggregate_counters ([0] sub-batches checked, [1] sub-batches failed) are those of zkv.h; a fresh coefficient set per chunk.
 *   - Device memory: a set that never switches the check on allocates nothing more.  With it on, from the first call that engages: 224 B
 *     per slot in flight (the scaled points), one pseudo-proof workspace (3.7 KB) per 16 slots plus one per 64 for the per-class padding,
 *     24 bytes of counters, and per call 4 bytes per sub-batch and per pseudo-proof slot.  No dense second-pass workspace: the second pass
 *     runs in place.
 *   - zkv_ctx_last_stage_ms keeps returning five stage times: PREP, the per-proof G1 stage, 0, the sums and the pseudo-proofs' Miller
 *     loops, and their final exponentiation with the verdicts and the second pass.
 *   - Damaged batches: a batch with one bad proof in 64 fails most sub-batches and pays both passes; switch the check off, or use
 *     enable = 1 (automatic), which pauses the check while too many sub-batches fail.  DESIGN.md section 14a has the measurements.
 *   - Out of scope: sharded sets, sets inside the gateway, n_c > 1, sharing the 3.6 MB line tables between keys of one class.
 */
#ifndef ZKV_PLONK_SET_AGG_H
#define ZKV_PLONK_SET_AGG_H
#include "zkv_plonk_set.h"

#ifdef __cplusplus
extern "C" {
#endif

/* The SRS classes of a PLONK set: class_of_key[k] (zkv_plonk_set_size entries) is key k's class, classes numbered by first appearance in
 * key order; *n_classes their number.  Either pointer may be NULL.  Host only: needs no device.  ZKV_ERR_WRONG_CTX on every other kind of
 * context.  Keys of one capable class share sub-batches. */
int zkv_plonk_set_srs_classes(const zkv_ctx* ctx, uint32_t* class_of_key, size_t* n_classes);

#ifdef __cplusplus
}
#endif
#endif /* ZKV_PLONK_SET_AGG_H */

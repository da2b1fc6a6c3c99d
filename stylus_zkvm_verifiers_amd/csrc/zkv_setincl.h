// RISC Zero set-inclusion receipts (include/zkv_risc0_set_inclusion.h): keccak-256 Merkle paths, one claim per lane.
// The rules are this project's definition (PARITY UNPINNED: the reference holds no set verifier), modelled on RISC Zero's Solidity set
// verifier and OpenZeppelin's MerkleProof.processProof:
//   leaf = keccak256("LEAF_TAG" || claim_digest)        40 bytes, one permutation
//   node(a, b) = keccak256(min(a, b) || max(a, b))       64 bytes, one permutation (below the 136-byte rate); the 32 bytes compare as
//                                                        big-endian integers, equal values allowed
//   root = fold of node over the path from the leaf; the root's journal digest is sha256(ID || root).
// The functions are ZKV_HD: tests/host_cpp/test_setincl.cpp runs the identical code on the CPU.
//
// A 32-byte keccak value is held as eight 32-bit words in keccak's own (little-endian) byte order: d[j] = bytes 4j .. 4j + 3, so
// (d[2k], d[2k + 1]) are the two halves of lane k and no byte moves between a digest and the next state.  The state is 25 lanes of two
// 32-bit halves; every index below is a compile-time constant once the round body is unrolled, so the state lives in 50 VGPRs and the
// rotations become v_alignbit_b32 pairs (a rotation by 32 is a renaming), chi and the xor trees of theta v_bitop3_b32.  The 24 rounds are a rolled loop (ZKV_KECCAK_UNROLL rounds per
// trip, default 1): one round is about 1.5 KB of code (188 VALU instructions), all 24 are 33 KB per copy of the permutation against a 64 KB
// instruction cache, and the loop costs a few scalar instructions a round.  Measured on 2^20 claims at depth 20:
// 1 round per trip 2.33 ms, 2: 2.41, 4: 2.48, 24: 2.53.  The round constant is wave-uniform: one scalar load per round.
#pragma once
#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#include "zkv_verify.h"
#endif
#include "zkv_sha256.h"

#ifndef ZKV_KECCAK_UNROLL
#define ZKV_KECCAK_UNROLL 1
#endif

namespace zkv {

constexpr uint32_t SETINCL_MAX_DEPTH = 64;          // ZKV_SETINCL_MAX_DEPTH
constexpr uint32_t SETINCL_STORED = 0xFFFFFFFFu;    // ZKV_SETINCL_STORED: the claim names no root seal, its root is looked up
constexpr uint32_t SETINCL_MAX_ROOTS = 4096;        // submitted roots a context keeps

// iota constants, (low, high) halves of round r at [2r], [2r + 1]
ZKV_TABLE uint32_t KECCAK_RC32[48] = {
    0x00000001u, 0x00000000u, 0x00008082u, 0x00000000u, 0x0000808Au, 0x80000000u, 0x80008000u, 0x80000000u, 0x0000808Bu, 0x00000000u,
    0x80000001u, 0x00000000u, 0x80008081u, 0x80000000u, 0x00008009u, 0x80000000u, 0x0000008Au, 0x00000000u, 0x00000088u, 0x00000000u,
    0x80008009u, 0x00000000u, 0x8000000Au, 0x00000000u, 0x8000808Bu, 0x00000000u, 0x0000008Bu, 0x80000000u, 0x00008089u, 0x80000000u,
    0x00008003u, 0x80000000u, 0x00008002u, 0x80000000u, 0x00000080u, 0x80000000u, 0x0000800Au, 0x00000000u, 0x8000000Au, 0x80000000u,
    0x80008081u, 0x80000000u, 0x00008080u, 0x80000000u, 0x80000001u, 0x00000000u, 0x80008008u, 0x80000000u};

struct KeccakState { uint32_t lo[25], hi[25]; };    // lane x + 5 y at index x + 5 y

// (lo, hi) rotated left by N as a 64-bit value, N a compile-time constant
template <int N> ZKV_HD void keccak_rotl(uint32_t lo, uint32_t hi, uint32_t& rlo, uint32_t& rhi) {
    if (N == 0) { rlo = lo; rhi = hi; }
    else if (N == 32) { rlo = hi; rhi = lo; }
    else if (N < 32) { rlo = (lo << (N & 31)) | (hi >> ((32 - N) & 31)); rhi = (hi << (N & 31)) | (lo >> ((32 - N) & 31)); }
    else { rlo = (hi << ((N - 32) & 31)) | (lo >> ((64 - N) & 31)); rhi = (lo << ((N - 32) & 31)) | (hi >> ((64 - N) & 31)); }
}

// a ^ b ^ c.  gfx950 has no v_xor3_b32; its three-input v_bitop3_b32 (truth table 0x96) is what the compiler already picks for chi, but it
// leaves chains of xors as two-input instructions, so the parity trees of theta name it.
ZKV_HD uint32_t keccak_xor3(uint32_t a, uint32_t b, uint32_t c) {
#if defined(__HIP_DEVICE_COMPILE__) && defined(__gfx950__)
    return __builtin_amdgcn_bitop3_b32(a, b, c, 0x96);
#else
    return a ^ b ^ c;
#endif
}

// rho + pi of one lane: B[y, 2x + 3y] = rot(A[x, y], r[x, y])
#define ZKV_KECCAK_RP(X, Y, R) keccak_rotl<R>(s.lo[X + 5 * Y], s.hi[X + 5 * Y], b.lo[Y + 5 * ((2 * X + 3 * Y) % 5)], b.hi[Y + 5 * ((2 * X + 3 * Y) % 5)])

ZKV_HD void keccak_round(KeccakState& s, uint32_t rc_lo, uint32_t rc_hi) {
    uint32_t cl[5], ch[5];
#pragma unroll
    for (int x = 0; x < 5; x++) {                                   // theta: column parities
        cl[x] = keccak_xor3(keccak_xor3(s.lo[x], s.lo[x + 5], s.lo[x + 10]), s.lo[x + 15], s.lo[x + 20]);
        ch[x] = keccak_xor3(keccak_xor3(s.hi[x], s.hi[x + 5], s.hi[x + 10]), s.hi[x + 15], s.hi[x + 20]);
    }
#pragma unroll
    for (int x = 0; x < 5; x++) {                                   // lane ^= C[x - 1] ^ rot(C[x + 1], 1): one three-input xor per half
        uint32_t rl, rh;
        keccak_rotl<1>(cl[(x + 1) % 5], ch[(x + 1) % 5], rl, rh);
#pragma unroll
        for (int y = 0; y < 25; y += 5) { s.lo[y + x] = keccak_xor3(s.lo[y + x], cl[(x + 4) % 5], rl); s.hi[y + x] = keccak_xor3(s.hi[y + x], ch[(x + 4) % 5], rh); }
    }
    KeccakState b;
    ZKV_KECCAK_RP(0, 0, 0);  ZKV_KECCAK_RP(1, 0, 1);  ZKV_KECCAK_RP(2, 0, 62); ZKV_KECCAK_RP(3, 0, 28); ZKV_KECCAK_RP(4, 0, 27);
    ZKV_KECCAK_RP(0, 1, 36); ZKV_KECCAK_RP(1, 1, 44); ZKV_KECCAK_RP(2, 1, 6);  ZKV_KECCAK_RP(3, 1, 55); ZKV_KECCAK_RP(4, 1, 20);
    ZKV_KECCAK_RP(0, 2, 3);  ZKV_KECCAK_RP(1, 2, 10); ZKV_KECCAK_RP(2, 2, 43); ZKV_KECCAK_RP(3, 2, 25); ZKV_KECCAK_RP(4, 2, 39);
    ZKV_KECCAK_RP(0, 3, 41); ZKV_KECCAK_RP(1, 3, 45); ZKV_KECCAK_RP(2, 3, 15); ZKV_KECCAK_RP(3, 3, 21); ZKV_KECCAK_RP(4, 3, 8);
    ZKV_KECCAK_RP(0, 4, 18); ZKV_KECCAK_RP(1, 4, 2);  ZKV_KECCAK_RP(2, 4, 61); ZKV_KECCAK_RP(3, 4, 56); ZKV_KECCAK_RP(4, 4, 14);
#pragma unroll
    for (int y = 0; y < 25; y += 5) {                               // chi
#pragma unroll
        for (int x = 0; x < 5; x++) {
            s.lo[y + x] = b.lo[y + x] ^ (~b.lo[y + (x + 1) % 5] & b.lo[y + (x + 2) % 5]);
            s.hi[y + x] = b.hi[y + x] ^ (~b.hi[y + (x + 1) % 5] & b.hi[y + (x + 2) % 5]);
        }
    }
    s.lo[0] ^= rc_lo; s.hi[0] ^= rc_hi;                             // iota
}
#undef ZKV_KECCAK_RP

ZKV_HD void keccak_f1600(KeccakState& s) {
#pragma unroll ZKV_KECCAK_UNROLL
    for (int r = 0; r < 24; r++) keccak_round(s, KECCAK_RC32[2 * r], KECCAK_RC32[2 * r + 1]);
}

// one-block keccak-256 of the first `words` state words (a whole number of 32-bit words, fewer than 34): pad10*1 of Ethereum's keccak
// (domain byte 0x01), the digest is lanes 0 .. 3
template <int WORDS> ZKV_HD void keccak256_block(KeccakState& s, uint32_t out[8]) {
    static_assert(WORDS < 33, "one block of the 136-byte rate");
#pragma unroll
    for (int k = (WORDS + 1) / 2; k < 25; k++) { s.lo[k] = 0; s.hi[k] = 0; }
    if (WORDS & 1) s.hi[WORDS / 2] = 1u; else s.lo[WORDS / 2] = 1u;
    s.hi[16] ^= 0x80000000u;
    keccak_f1600(s);
#pragma unroll
    for (int k = 0; k < 4; k++) { out[2 * k] = s.lo[k]; out[2 * k + 1] = s.hi[k]; }
}

// keccak-256 of a message of fewer than 136 bytes at any alignment (known-answer vectors; the Merkle hashes use the word forms below)
ZKV_HD void keccak256_short(const uint8_t* msg, uint32_t len, uint32_t out[8]) {
    KeccakState s;
#pragma unroll
    for (int k = 0; k < 25; k++) { s.lo[k] = 0; s.hi[k] = 0; }
#pragma unroll
    for (int k = 0; k < 17; k++) {
        uint32_t lo = 0, hi = 0;
#pragma unroll
        for (int b = 0; b < 4; b++) {
            const uint32_t p = 8u * k + b, q = p + 4;
            lo |= (p < len ? (uint32_t)msg[p] : (p == len ? 1u : 0u)) << (8 * b);
            hi |= (q < len ? (uint32_t)msg[q] : (q == len ? 1u : 0u)) << (8 * b);
        }
        s.lo[k] = lo; s.hi[k] = hi;
    }
    s.hi[16] ^= 0x80000000u;
    keccak_f1600(s);
#pragma unroll
    for (int k = 0; k < 4; k++) { out[2 * k] = s.lo[k]; out[2 * k + 1] = s.hi[k]; }
}

// keccak256("LEAF_TAG" || claim_digest): claim_be = the digest as SHA-256 leaves it (big-endian words, h[0] first)
ZKV_HD void setincl_leaf(const uint32_t claim_be[8], uint32_t out[8]) {
    KeccakState s;
    s.lo[0] = 0x4641454Cu; s.hi[0] = 0x4741545Fu;                   // "LEAF" "_TAG"
#pragma unroll
    for (int k = 0; k < 4; k++) { s.lo[1 + k] = __builtin_bswap32(claim_be[2 * k]); s.hi[1 + k] = __builtin_bswap32(claim_be[2 * k + 1]); }
    keccak256_block<10>(s, out);
}

// a < b as 32-byte big-endian integers
ZKV_HD bool setincl_less(const uint32_t a[8], const uint32_t b[8]) {
    bool lt = false, decided = false;
#pragma unroll
    for (int j = 0; j < 8; j++) {
        const uint32_t x = __builtin_bswap32(a[j]), y = __builtin_bswap32(b[j]);
        lt = decided ? lt : x < y;
        decided = decided || x != y;
    }
    return lt;
}

// keccak256(min(a, b) || max(a, b)); out may be a or b
ZKV_HD void setincl_node(const uint32_t a[8], const uint32_t b[8], uint32_t out[8]) {
    const bool a_first = !setincl_less(b, a);
    KeccakState s;
#pragma unroll
    for (int k = 0; k < 4; k++) {
        s.lo[k] = a_first ? a[2 * k] : b[2 * k];         s.hi[k] = a_first ? a[2 * k + 1] : b[2 * k + 1];
        s.lo[4 + k] = a_first ? b[2 * k] : a[2 * k];     s.hi[4 + k] = a_first ? b[2 * k + 1] : a[2 * k + 1];
    }
    keccak256_block<16>(s, out);
}

// sibling k of a path from a byte pointer of any alignment
struct SiblingBytes {
    const uint8_t* p;
    ZKV_HD void operator()(uint32_t k, uint32_t s[8]) const {
        const uint8_t* q = p + 32 * (size_t)k;
#pragma unroll
        for (int j = 0; j < 8; j++) s[j] = (uint32_t)q[4 * j] | ((uint32_t)q[4 * j + 1] << 8) | ((uint32_t)q[4 * j + 2] << 16) | ((uint32_t)q[4 * j + 3] << 24);
    }
};

// cur = fold of node over the `depth` siblings that `load` yields; sibling k + 1 is loaded before permutation k, so its latency hides
// behind the 24 rounds.  depth = 0 leaves cur as it is.
template <class LOAD> ZKV_HD void setincl_walk(uint32_t cur[8], uint32_t depth, const LOAD& load) {
    uint32_t sib[8], nxt[8];
    if (depth) load(0, sib);
#pragma unroll 1
    for (uint32_t k = 0; k < depth; k++) {
        if (k + 1 < depth) load(k + 1, nxt);
        setincl_node(cur, sib, cur);
#pragma unroll
        for (int j = 0; j < 8; j++) sib[j] = nxt[j];
    }
}

// sha256(ID || root), a 64-byte message: id_be = ID as big-endian words, root = keccak words
ZKV_HD void setincl_root_journal(const uint32_t id_be[8], const uint32_t root[8], uint32_t h[8]) {
    uint32_t w[16];
    sha256_init(h);
#pragma unroll
    for (int j = 0; j < 8; j++) { w[j] = id_be[j]; w[8 + j] = __builtin_bswap32(root[j]); }
    sha256_compress(h, w);
    w[0] = 0x80000000u;
#pragma unroll
    for (int j = 1; j < 15; j++) w[j] = 0;
    w[15] = 64u * 8u;
    sha256_compress(h, w);
}

// ---------------------------------------------------------------- kernels (k_setincl.hip) and their host-side launchers
#if defined(__HIPCC__)
// claim_job values besides a job slot
constexpr uint32_t SETINCL_DONE = 0xFFFFFFFFu;      // answered by the hash kernel (library limit, stored-root lookup)
constexpr uint32_t SETINCL_MEMBER = 0xFFFFFFFEu;    // its root equals its representative's: the group's job answers it
constexpr uint32_t SETINCL_PENDING = 0xFFFFFFFDu;   // hashed, not yet grouped

// One chunk of claims.  in_a / in_b / path_off / root_idx / status / recv point at the chunk's first claim; `paths` is the call's whole
// blob and path_off holds n + 1 offsets into it in sibling units, none beyond n_siblings (a claim whose offsets run backwards, leave
// the blob or span more than SETINCL_MAX_DEPTH siblings is never read: INVALID_PROOF_DATA).
struct SetinclChunk {
    uint32_t n, m, n_siblings, n_stored;
    const uint8_t* in_a; const uint8_t* in_b;           // n x 32: image ids + journal digests, or claim digests + nullptr (integrity)
    const uint8_t* paths; const uint32_t* path_off;
    const uint32_t* root_idx;                           // nullptr (diagnostic): hash only
    const uint8_t* seals; const uint32_t* seal_len;     // m rows of 260 bytes; true lengths, or nullptr: all 260
    const uint8_t* stored;                              // n_stored submitted roots, 32 bytes each, ascending as big-endian integers
    uint32_t id_be[8];                                  // the set-builder image id as big-endian words
    uint32_t* roots;                                    // 8 words per claim
    uint32_t* rep; uint32_t* gslot;                     // per root seal: lowest claim naming it (0xFFFFFFFF: none), its job slot
    uint32_t* claim_job; uint32_t* job_claim;           // per claim: slot / SETINCL_*; per slot: its claim
    uint32_t* counters;                                 // [0] jobs of this chunk, [1] stored-root lookups of the call
    uint8_t* status; uint8_t* recv;
    uint8_t* diag_roots;                                // diagnostic: n x 32 root bytes (zero for a claim that is never read)
};
// The job rows of a chunk.  Built-in inner verifier: the records of the RISC Zero stage pipeline (260-byte row, true length, ID, journal
// digest) and its statuses / received selectors.  Keyed: the front checks are made here (pre: status, or 0xFF = verify), the rows are
// Groth16 proofs and five signals, `st` holds the verdict 1 / 0.
struct SetinclJobs {
    uint32_t n_jobs, keyed, selector_be, pad;
    uint8_t* rows; uint32_t* lens; uint8_t* ids; uint8_t* jds;
    uint8_t* proofs; uint8_t* signals; uint8_t* pre; uint8_t* pre_recv;
    uint8_t fixed[3][32];                               // keyed signals 0, 1, 4: control root halves, control id
    const uint8_t* st; const uint8_t* rv;
};
void launch_setincl_hash(const SetinclChunk& c, const Risc0Consts& k, hipStream_t s);
void launch_setincl_group(const SetinclChunk& c, hipStream_t s);
void launch_setincl_jobs(const SetinclChunk& c, const SetinclJobs& j, const Risc0Consts& k, hipStream_t s);
void launch_setincl_scatter(const SetinclChunk& c, const SetinclJobs& j, hipStream_t s);
#endif

}  // namespace zkv

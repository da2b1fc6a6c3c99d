// RISC Zero set-inclusion receipts (include/zkv_risc0_set_inclusion.h; the math: zkv_setincl.h).  Parity unpinned.
//   k_setincl_hash     one claim per lane: claim digest (SHA-256 chain unless the method is integrity), leaf, path walk -> root; answers
//                      the library limits and the stored-root claims, elects each root seal's representative (lowest claim naming it)
//   k_setincl_group    a claim whose root differs from its representative's is a straggler: representatives and stragglers take a job slot
//   k_setincl_jobs     one job per lane: the seal gathered to a row, ID and sha256(ID || root) beside it (keyed: front checks, proof, signals)
//   k_setincl_scatter  job status and received selector back to every claim of the group or straggler
// Job slots come from an atomic counter, so their order varies from run to run; every claim reads its own job's answer, so statuses do not.
#include "zkv_setincl.h"

namespace zkv {

constexpr int SETINCL_BLOCK = 64;       // one wavefront per workgroup, as the other one-item-per-lane kernels

// sibling k of a path in a 16-byte aligned blob: two 16-byte loads
struct SiblingQuads {
    const uint4* p;
    __device__ __forceinline__ void operator()(uint32_t k, uint32_t s[8]) const {
        const uint4 a = p[2 * (size_t)k], b = p[2 * (size_t)k + 1];
        s[0] = a.x; s[1] = a.y; s[2] = a.z; s[3] = a.w; s[4] = b.x; s[5] = b.y; s[6] = b.z; s[7] = b.w;
    }
};

// -1 / 0 / 1: root against a table entry (32 bytes, 4-byte aligned) as big-endian integers
__device__ __forceinline__ int setincl_cmp(const uint32_t root[8], const uint32_t* entry) {
    int r = 0;
#pragma unroll
    for (int j = 7; j >= 0; j--) {
        const uint32_t x = __builtin_bswap32(root[j]), y = __builtin_bswap32(entry[j]);
        r = x < y ? -1 : (x > y ? 1 : r);
    }
    return r;
}

__device__ __forceinline__ void put_recv(uint8_t* recv, size_t i, uint32_t v) {
    if (!recv) return;
    recv[4 * i] = (uint8_t)(v >> 24); recv[4 * i + 1] = (uint8_t)(v >> 16); recv[4 * i + 2] = (uint8_t)(v >> 8); recv[4 * i + 3] = (uint8_t)v;
}

__global__ __launch_bounds__(SETINCL_BLOCK) void k_setincl_hash(SetinclChunk c, Risc0Consts k) {
    const uint32_t i = blockIdx.x * SETINCL_BLOCK + threadIdx.x;
    const bool active = i < c.n;
    const bool diag = c.root_idx == nullptr;
    uint32_t o0 = 0, o1 = 0, idx = SETINCL_STORED;
    if (active) { o0 = c.path_off[i]; o1 = c.path_off[i + 1]; if (!diag) idx = c.root_idx[i]; }
    const bool stored = idx == SETINCL_STORED;
    // library limits: such a claim is never read and takes no pairing
    const bool bad = o1 < o0 || o1 > c.n_siblings || o1 - o0 > SETINCL_MAX_DEPTH || (!stored && idx >= c.m);
    uint32_t root[8];
#pragma unroll
    for (int j = 0; j < 8; j++) root[j] = 0;
    if (active && !bad) {
        uint32_t h[8];
        if (c.in_b) risc0_claim_digest(k, c.in_a + 32 * (size_t)i, c.in_b + 32 * (size_t)i, h);
        else {
#pragma unroll 1
            for (int j = 0; j < 8; j++) h[j] = load_be32(c.in_a + 32 * (size_t)i + 4 * j);
        }
        setincl_leaf(h, root);
        const uint8_t* path = c.paths + 32 * (size_t)o0;
        if (!((uintptr_t)c.paths & 15u)) setincl_walk(root, o1 - o0, SiblingQuads{(const uint4*)path});      // wave-uniform test of the blob base
        else setincl_walk(root, o1 - o0, SiblingBytes{path});
    }
    if (diag) {
        if (active) {
#pragma unroll
            for (int j = 0; j < 8; j++)
#pragma unroll
                for (int b = 0; b < 4; b++) c.diag_roots[32 * (size_t)i + 4 * j + b] = (uint8_t)(root[j] >> (8 * b));
        }
        return;
    }
    bool grouped = false;
    if (active) {
        uint4* dst = (uint4*)(c.roots + 8 * (size_t)i);
        dst[0] = make_uint4(root[0], root[1], root[2], root[3]);
        dst[1] = make_uint4(root[4], root[5], root[6], root[7]);
        if (bad) { c.status[i] = ST_INVALID_PROOF_DATA; put_recv(c.recv, i, 0); c.claim_job[i] = SETINCL_DONE; }
        else if (stored) {
            uint32_t lo = 0, hi = c.n_stored;
            bool found = false;
#pragma unroll 1
            while (lo < hi) {
                const uint32_t mid = (lo + hi) >> 1;
                const int r = setincl_cmp(root, (const uint32_t*)c.stored + 8 * (size_t)mid);
                if (r == 0) { found = true; break; }
                if (r < 0) hi = mid; else lo = mid + 1;
            }
            c.status[i] = found ? ST_OK : ST_VERIFICATION_FAILED; put_recv(c.recv, i, 0); c.claim_job[i] = SETINCL_DONE;
        } else { c.claim_job[i] = SETINCL_PENDING; grouped = true; }
    }
    // stored-root lookups of the call: one atomic per wavefront
    const unsigned long long looked = __ballot(active && !bad && stored);
    if (looked && threadIdx.x == 0) atomicAdd(&c.counters[1], (uint32_t)__popcll(looked));
    // representative of root seal j: the lowest claim naming it.  Lanes hold ascending claims, so the first lane naming j speaks for the
    // wavefront; the value only ever falls, so a plain read that already shows a lower claim saves the atomic.
    bool want = grouped;
#pragma unroll 1
    for (;;) {
        const unsigned long long mask = __ballot(want);
        if (!mask) break;
        const int leader = __ffsll((long long)mask) - 1;
        const uint32_t jj = (uint32_t)__shfl((int)idx, leader);
        if (want && idx == jj) {
            if ((int)threadIdx.x == leader && __atomic_load_n(&c.rep[jj], __ATOMIC_RELAXED) > i) atomicMin(&c.rep[jj], i);
            want = false;
        }
    }
}

__global__ __launch_bounds__(SETINCL_BLOCK) void k_setincl_group(SetinclChunk c) {
    const uint32_t i = blockIdx.x * SETINCL_BLOCK + threadIdx.x;
    if (i >= c.n || c.claim_job[i] != SETINCL_PENDING) return;
    const uint32_t j = c.root_idx[i], r = c.rep[j];
    bool own = i == r;
    if (!own) {
        const uint4* a = (const uint4*)(c.roots + 8 * (size_t)i);
        const uint4* b = (const uint4*)(c.roots + 8 * (size_t)r);
        const uint4 a0 = a[0], a1 = a[1], b0 = b[0], b1 = b[1];
        own = a0.x != b0.x || a0.y != b0.y || a0.z != b0.z || a0.w != b0.w || a1.x != b1.x || a1.y != b1.y || a1.z != b1.z || a1.w != b1.w;   // a straggler
    }
    if (!own) { c.claim_job[i] = SETINCL_MEMBER; return; }
    const uint32_t slot = atomicAdd(&c.counters[0], 1u);            // at most n: every claim takes at most one slot
    c.job_claim[slot] = i;
    c.claim_job[i] = slot;
    if (i == r) c.gslot[j] = slot;
}

__device__ __forceinline__ void put_be32(uint8_t* p, uint32_t v) { p[0] = (uint8_t)(v >> 24); p[1] = (uint8_t)(v >> 16); p[2] = (uint8_t)(v >> 8); p[3] = (uint8_t)v; }

__global__ __launch_bounds__(SETINCL_BLOCK) void k_setincl_jobs(SetinclChunk c, SetinclJobs jb, Risc0Consts k) {
    const uint32_t s = blockIdx.x * SETINCL_BLOCK + threadIdx.x;
    if (s >= jb.n_jobs) return;
    const uint32_t i = c.job_claim[s], j = c.root_idx[i];
    const uint8_t* seal = c.seals + 260 * (size_t)j;
    const uint32_t len = c.seal_len ? c.seal_len[j] : 260u, have = len < 260u ? len : 260u;
    uint32_t root[8], jd[8];
#pragma unroll
    for (int q = 0; q < 8; q++) root[q] = c.roots[8 * (size_t)i + q];
    setincl_root_journal(c.id_be, root, jd);
    if (!jb.keyed) {
        uint8_t* row = jb.rows + 260 * (size_t)s;
#pragma unroll 1
        for (uint32_t b = 0; b < 260u; b++) row[b] = b < have ? seal[b] : (uint8_t)0;
        jb.lens[s] = len;
#pragma unroll 1
        for (int q = 0; q < 8; q++) { put_be32(jb.ids + 32 * (size_t)s + 4 * q, c.id_be[q]); put_be32(jb.jds + 32 * (size_t)s + 4 * q, jd[q]); }
        return;
    }
    // keyed: Risc0Verifier._verify_integrity_internal's front checks (risc0/verifier.rs:146-179) with the caller's selector
    uint8_t pre = 0xFF;
    uint32_t rv = 0;
    if (len < 4) pre = ST_INVALID_PROOF_DATA;
    else {
        const uint32_t sel = load_be32(seal);
        if (sel != jb.selector_be) { pre = ST_SELECTOR_MISMATCH; rv = sel; }
        else if (len != 260u) pre = ST_INVALID_PROOF_DATA;
    }
    jb.pre[s] = pre;
    put_be32(jb.pre_recv + 4 * (size_t)s, rv);
    uint8_t* proof = jb.proofs + 256 * (size_t)s;
#pragma unroll 1
    for (uint32_t b = 0; b < 256u; b++) proof[b] = pre == 0xFF ? seal[4 + b] : (uint8_t)0;
    // signals (risc0/verifier.rs:128-144): control root halves, the halves of the claim digest of (ID, sha256(ID || root)), control id
    uint32_t h[8];
    uint8_t idb[32], jdb[32];
#pragma unroll
    for (int q = 0; q < 8; q++) { put_be32(idb + 4 * q, c.id_be[q]); put_be32(jdb + 4 * q, jd[q]); }
    risc0_claim_digest(k, idb, jdb, h);
    uint8_t* sig = jb.signals + 160 * (size_t)s;
#pragma unroll 1
    for (int b = 0; b < 32; b++) { sig[b] = jb.fixed[0][b]; sig[32 + b] = jb.fixed[1][b]; sig[128 + b] = jb.fixed[2][b]; }
    // split_digest (risc0/crypto.rs:95-110): the digest's bytes reversed; low half = bytes 15 .. 0, high half = bytes 31 .. 16
#pragma unroll 1
    for (int b = 0; b < 16; b++) {
        sig[64 + b] = 0; sig[96 + b] = 0;
        const int lo_b = 15 - b, hi_b = 31 - b;
        sig[64 + 16 + b] = (uint8_t)(h[lo_b >> 2] >> (24 - 8 * (lo_b & 3)));
        sig[96 + 16 + b] = (uint8_t)(h[hi_b >> 2] >> (24 - 8 * (hi_b & 3)));
    }
}

__global__ __launch_bounds__(SETINCL_BLOCK) void k_setincl_scatter(SetinclChunk c, SetinclJobs jb) {
    const uint32_t i = blockIdx.x * SETINCL_BLOCK + threadIdx.x;
    if (i >= c.n) return;
    uint32_t slot = c.claim_job[i];
    if (slot == SETINCL_DONE) return;
    if (slot == SETINCL_MEMBER) slot = c.gslot[c.root_idx[i]];
    if (slot >= jb.n_jobs) { c.status[i] = ST_VERIFICATION_FAILED; put_recv(c.recv, i, 0); return; }     // (cannot happen: fail closed)
    uint8_t st; uint32_t rv;
    if (jb.keyed) {
        const uint8_t pre = jb.pre[slot];
        st = pre != 0xFF ? pre : (jb.st[slot] ? ST_OK : ST_VERIFICATION_FAILED);
        rv = load_be32(jb.pre_recv + 4 * (size_t)slot);
    } else { st = jb.st[slot]; rv = load_be32(jb.rv + 4 * (size_t)slot); }
    c.status[i] = st;
    put_recv(c.recv, i, rv);
}

static unsigned setincl_blocks(uint32_t n) { return (n + SETINCL_BLOCK - 1) / SETINCL_BLOCK; }
void launch_setincl_hash(const SetinclChunk& c, const Risc0Consts& k, hipStream_t s) {
    if (c.n) hipLaunchKernelGGL(k_setincl_hash, dim3(setincl_blocks(c.n)), dim3(SETINCL_BLOCK), 0, s, c, k);
}
void launch_setincl_group(const SetinclChunk& c, hipStream_t s) {
    if (c.n) hipLaunchKernelGGL(k_setincl_group, dim3(setincl_blocks(c.n)), dim3(SETINCL_BLOCK), 0, s, c);
}
void launch_setincl_jobs(const SetinclChunk& c, const SetinclJobs& j, const Risc0Consts& k, hipStream_t s) {
    if (j.n_jobs) hipLaunchKernelGGL(k_setincl_jobs, dim3(setincl_blocks(j.n_jobs)), dim3(SETINCL_BLOCK), 0, s, c, j, k);
}
void launch_setincl_scatter(const SetinclChunk& c, const SetinclJobs& j, hipStream_t s) {
    if (c.n) hipLaunchKernelGGL(k_setincl_scatter, dim3(setincl_blocks(c.n)), dim3(SETINCL_BLOCK), 0, s, c, j);
}

}  // namespace zkv

// RISC Zero router, set route (include/zkv_risc0_router_set.h; the header arithmetic and the identity pair:
// zkv_rzrouter_set.h).  A set-inclusion seal arrives at the router in its on-chain form, is taken apart here, and its root seal goes
// back into the router's own partition as a 260-byte job row.  Parity unpinned.
//   k_rzset_front    one seal per lane, found by rzs_span (a pair of offsets, or the record of decoded calldata): a seal with the set
//                    selector is parsed (rzs_parse); malformed bodies and the library limits (a path past SETINCL_MAX_DEPTH, a root
//                    seal that begins with the set selector) are answered, the others leave a claim record.  Seals of other selectors
//                    are not touched: the router's partition (k_rzrouter_count ...) reads them where they lie
//   k_rzset_ident    one claim per wavefront: the claim's root seal finds its slot in an open-addressed table (fingerprint, then bytes)
//                    and lowers the slot's representative; the slot is section 16's root index
//   k_rzset_hash     one claim per lane: claim digest (derived or given, per row where the batch has a method row), leaf and path walk
//                    from the blob, the stored-root lookup of an empty root seal
//   (k_setincl_group of k_setincl.hip: representatives and stragglers take job slots)
//   k_rzset_jobs     one job per lane: the root seal copied to a 260-byte row, its true length, ID and sha256(ID || root) beside it
//   (the rows run through run_router as a batch of their own)
//   k_rzset_scatter  every set seal's status and received selector: the answer kept by the front end, or its job's
// No lane waits for another one: a claim that loses the compare-and-swap of a slot reads the winner's record, which the front kernel
// wrote in an earlier launch, and the winner's bytes, which lie in the caller's input; the probe loop ends after `table` slots.
#include "zkv_rzrouter_set.h"

namespace zkv {

constexpr int RZS_BLOCK = 256;          // front, identity, scatter: a few loads per seal
constexpr int RZS_HASH_BLOCK = 64;      // hash, jobs: one wavefront per workgroup, as k_setincl.hip

__device__ __forceinline__ void rzs_put_be32(uint8_t* p, uint32_t v) { p[0] = (uint8_t)(v >> 24); p[1] = (uint8_t)(v >> 16); p[2] = (uint8_t)(v >> 8); p[3] = (uint8_t)v; }

// Seal i of the chunk as (start, length) from a.seals, the only place that knows offsets from records (k_rzset_front is its only caller:
// every later kernel takes absolute positions from RzsRec).  false: the set stage never reads the seal and it is no set seal -- offsets
// that run backwards or past seal_bytes (the partition answers a short seal), a request that is not a canonical call, a method byte
// above ZKV_METHOD_VERIFY_INTEGRITY (the partition answers bad calldata).
__device__ __forceinline__ bool rzs_span(const RzsArgs& a, uint32_t i, uint64_t* start, uint64_t* len) {
    if (a.method && a.method[i] > 1) return false;
    if (!a.seal_off) {
        const RzsSpan sp = a.span[i];
        *start = sp.at; *len = sp.len;
        return a.wire_len[i] != 0xFFFFFFFFu;
    }
    const uint64_t s = a.seal_off[i], e = a.seal_off[i + 1];
    *start = s; *len = e - s;
    return s <= e && e <= a.seal_bytes;
}

__global__ __launch_bounds__(RZS_BLOCK) void k_rzset_front(SetinclChunk c, RzsArgs a) {
    const uint32_t i = blockIdx.x * RZS_BLOCK + threadIdx.x;
    bool set = false;
    if (i < c.n) {
        uint64_t s, len;
        uint32_t job = RZS_JOB_NOT_SET;
        if (rzs_span(a, i, &s, &len)) {
            const uint8_t* p = a.seals + s;
            const RzsSeal r = rzs_parse(p, len, !((uintptr_t)p & 3u), a.set_sel);
            if (r.kind != RZS_NOT_SET) {
                set = true;
                job = SETINCL_DONE;
                // library limits: no hashing and no pairing for such a claim
                const bool nested = r.kind == RZS_CLAIM && r.root_len >= 4 && load_be32(p + r.root_at) == a.set_sel;
                if (r.kind == RZS_CLAIM && r.depth <= SETINCL_MAX_DEPTH && !nested) {
                    RzsRec rec;
                    rec.path_at = s + RZS_PATH_AT; rec.root_at = s + r.root_at; rec.depth = r.depth; rec.root_len = r.root_len;
                    a.rec[i] = rec;
                    job = SETINCL_PENDING;
                } else a.ans[i] = ST_INVALID_PROOF_DATA;
            }
        }
        c.claim_job[i] = job;
    }
    const unsigned long long m = __ballot(set);
    if (m && (threadIdx.x & 63u) == 0) atomicAdd(&c.counters[2], (uint32_t)__popcll(m));
}

// One wavefront per claim: the lanes read the root seal's words side by side (a lane per claim would read 64 cache lines per load, the
// seals lie a kilobyte apart), the fingerprint is combined across the wavefront, lane 0 takes or reads the slot, and the comparison with
// an occupant's bytes again is a word per lane.  Every branch around a cross-lane operation is wave-uniform.
__global__ __launch_bounds__(RZS_BLOCK) void k_rzset_ident(SetinclChunk c, RzsArgs a) {
    const uint32_t i = blockIdx.x * (RZS_BLOCK / 64) + (threadIdx.x >> 6), lane = threadIdx.x & 63u;
    if (i >= c.n || c.claim_job[i] != SETINCL_PENDING) return;
    const RzsRec me = a.rec[i];
    if (!me.root_len) return;
    const uint8_t* mine = a.seals + me.root_at;
    const uint32_t take = rzs_fp_take(me.root_len);
    uint32_t acc = 0;
    for (uint32_t w = lane; 4 * w < take; w += 64) acc ^= rzs_fp_word(gw_ld4(mine + 4 * w, take - 4 * w), w);
#pragma unroll
    for (int d = 32; d; d >>= 1) acc ^= (uint32_t)__shfl_xor((int)acc, d);
    const uint32_t mask = a.table - 1;
    uint32_t slot = rzs_fp_finish(acc, me.root_len) & a.fp_mask & mask;
    bool placed = false, took = false;
#pragma unroll 1
    for (uint32_t t = 0; t < a.table && !placed; t++) {
        uint32_t o = 0;
        if (lane == 0) {
            o = __atomic_load_n(&a.owner[slot], __ATOMIC_RELAXED);
            if (o == RZS_EMPTY) {
                o = atomicCAS(&a.owner[slot], RZS_EMPTY, i);
                if (o == RZS_EMPTY) { o = i; took = true; }
            }
        }
        o = (uint32_t)__shfl((int)o, 0);
        bool same = o == i;
        if (!same) {                                                 // the occupant's bytes decide, never the fingerprint
            const RzsRec ot = a.rec[o];
            bool diff = ot.root_len != me.root_len;
            const uint8_t* theirs = a.seals + ot.root_at;
            const uint64_t len = me.root_len;
            for (uint64_t at = 4ull * lane; at < len && !diff; at += 256) diff = gw_ld4(mine + at, len - at) != gw_ld4(theirs + at, len - at);
            same = !__any(diff);
        }
        if (same) {
            // (the representative only ever falls: a plain read that already shows a lower claim saves the atomic)
            if (lane == 0) { a.root_idx[i] = slot; if (__atomic_load_n(&c.rep[slot], __ATOMIC_RELAXED) > i) atomicMin(&c.rep[slot], i); }
            placed = true;
        } else slot = (slot + 1) & mask;
    }
    if (lane == 0) {
        if (!placed) { c.claim_job[i] = SETINCL_DONE; a.ans[i] = ST_VERIFICATION_FAILED; }      // (cannot happen, table >= 2 n: fail closed)
        if (took) atomicAdd(&c.counters[3], 1u);
    }
}

// sibling k of a path anywhere in the blob: eight dword loads where the path is 4-byte aligned, byte loads elsewhere; only the loads
// diverge when the lanes of a wavefront differ, the permutation is shared
struct SiblingAt {
    const uint8_t* p; bool al;
    __device__ __forceinline__ void operator()(uint32_t k, uint32_t s[8]) const {
        const uint8_t* q = p + 32 * (size_t)k;
        if (al) {
            const uint32_t* w = (const uint32_t*)q;
#pragma unroll
            for (int j = 0; j < 8; j++) s[j] = w[j];
        } else SiblingBytes{p}(k, s);
    }
};

// -1 / 0 / 1: root against a table entry (32 bytes, 4-byte aligned) as big-endian integers
__device__ __forceinline__ int rzs_cmp(const uint32_t root[8], const uint32_t* entry) {
    int r = 0;
#pragma unroll
    for (int j = 7; j >= 0; j--) {
        const uint32_t x = __builtin_bswap32(root[j]), y = __builtin_bswap32(entry[j]);
        r = x < y ? -1 : (x > y ? 1 : r);
    }
    return r;
}

__global__ __launch_bounds__(RZS_HASH_BLOCK) void k_rzset_hash(SetinclChunk c, RzsArgs a, Risc0Consts k) {
    const uint32_t i = blockIdx.x * RZS_HASH_BLOCK + threadIdx.x;
    bool looked = false;
    if (i < c.n && c.claim_job[i] == SETINCL_PENDING) {
        const RzsRec me = a.rec[i];
        uint32_t h[8], root[8];
        if (!rzs_claim_given(a.method, c.in_b != nullptr, i)) risc0_claim_digest(k, c.in_a + 32 * (size_t)i, c.in_b + 32 * (size_t)i, h);
        else {
#pragma unroll 1
            for (int j = 0; j < 8; j++) h[j] = load_be32(c.in_a + 32 * (size_t)i + 4 * j);
        }
        setincl_leaf(h, root);
        const uint8_t* path = a.seals + me.path_at;
        setincl_walk(root, me.depth, SiblingAt{path, !((uintptr_t)path & 3u)});
        uint4* dst = (uint4*)(c.roots + 8 * (size_t)i);
        dst[0] = make_uint4(root[0], root[1], root[2], root[3]);
        dst[1] = make_uint4(root[4], root[5], root[6], root[7]);
        if (!me.root_len) {                                          // no root seal: the root must have been submitted
            uint32_t lo = 0, hi = c.n_stored;
            bool found = false;
#pragma unroll 1
            while (lo < hi) {
                const uint32_t mid = (lo + hi) >> 1;
                const int r = rzs_cmp(root, (const uint32_t*)c.stored + 8 * (size_t)mid);
                if (r == 0) { found = true; break; }
                if (r < 0) hi = mid; else lo = mid + 1;
            }
            a.ans[i] = found ? ST_OK : ST_VERIFICATION_FAILED;
            c.claim_job[i] = SETINCL_DONE;
            looked = true;
        }
    }
    const unsigned long long m = __ballot(looked);
    if (m && threadIdx.x == 0) atomicAdd(&c.counters[1], (uint32_t)__popcll(m));
}

__global__ __launch_bounds__(RZS_HASH_BLOCK) void k_rzset_jobs(SetinclChunk c, RzsArgs a, SetinclJobs jb) {
    const uint32_t s = blockIdx.x * RZS_HASH_BLOCK + threadIdx.x;
    if (s >= jb.n_jobs) return;
    const uint32_t i = c.job_claim[s];
    const RzsRec me = a.rec[i];
    const uint8_t* seal = a.seals + me.root_at;
    const uint32_t have = me.root_len < 260u ? me.root_len : 260u;
    uint32_t* row = (uint32_t*)(jb.rows + 260 * (size_t)s);          // 260 = 4 x 65: every row is dword aligned
#pragma unroll 1
    for (uint32_t w = 0; w < 65u; w++) row[w] = 4 * w < have ? gw_ld4(seal + 4 * w, have - 4 * w) : 0u;
    jb.lens[s] = me.root_len > 0xFFFFFFFEu ? 0xFFFFFFFEu : me.root_len;      // (0xFFFFFFFF is RzrArgs::wire_len's bad-calldata mark)
    uint32_t root[8], jd[8];
#pragma unroll
    for (int q = 0; q < 8; q++) root[q] = c.roots[8 * (size_t)i + q];
    setincl_root_journal(c.id_be, root, jd);
#pragma unroll 1
    for (int q = 0; q < 8; q++) { rzs_put_be32(jb.ids + 32 * (size_t)s + 4 * q, c.id_be[q]); rzs_put_be32(jb.jds + 32 * (size_t)s + 4 * q, jd[q]); }
}

__global__ __launch_bounds__(RZS_BLOCK) void k_rzset_scatter(SetinclChunk c, RzsArgs a, SetinclJobs jb) {
    const uint32_t i = blockIdx.x * RZS_BLOCK + threadIdx.x;
    if (i >= c.n) return;
    uint32_t slot = c.claim_job[i];
    if (slot == RZS_JOB_NOT_SET) return;                             // the router's partition has answered it
    uint8_t st = ST_VERIFICATION_FAILED;
    uint32_t rv = 0;
    if (slot == SETINCL_DONE) st = a.ans[i];
    else {
        if (slot == SETINCL_MEMBER) slot = c.gslot[a.root_idx[i]];
        if (slot < jb.n_jobs) { st = jb.st[slot]; rv = load_be32(jb.rv + 4 * (size_t)slot); }      // (else cannot happen: fail closed)
    }
    c.status[i] = st;
    if (c.recv) rzs_put_be32(c.recv + 4 * (size_t)i, rv);
}

__global__ __launch_bounds__(RZS_BLOCK) void k_rzset_reps(SetinclChunk c, RzsArgs a, uint32_t* __restrict__ out) {
    const uint32_t i = blockIdx.x * RZS_BLOCK + threadIdx.x;
    if (i >= c.n) return;
    out[i] = c.claim_job[i] == SETINCL_PENDING && a.rec[i].root_len ? c.rep[a.root_idx[i]] : RZS_EMPTY;
}

static unsigned rzs_blocks(uint32_t n, int block) { return (n + block - 1) / block; }
void launch_rzset_front(const SetinclChunk& c, const RzsArgs& a, hipStream_t s) {
    if (!c.n) return;
    hipLaunchKernelGGL(k_rzset_front, dim3(rzs_blocks(c.n, RZS_BLOCK)), dim3(RZS_BLOCK), 0, s, c, a);
    hipLaunchKernelGGL(k_rzset_ident, dim3(rzs_blocks(c.n, RZS_BLOCK / 64)), dim3(RZS_BLOCK), 0, s, c, a);
}
void launch_rzset_hash(const SetinclChunk& c, const RzsArgs& a, const Risc0Consts& k, hipStream_t s) {
    if (c.n) hipLaunchKernelGGL(k_rzset_hash, dim3(rzs_blocks(c.n, RZS_HASH_BLOCK)), dim3(RZS_HASH_BLOCK), 0, s, c, a, k);
}
void launch_rzset_jobs(const SetinclChunk& c, const RzsArgs& a, const SetinclJobs& j, hipStream_t s) {
    if (j.n_jobs) hipLaunchKernelGGL(k_rzset_jobs, dim3(rzs_blocks(j.n_jobs, RZS_HASH_BLOCK)), dim3(RZS_HASH_BLOCK), 0, s, c, a, j);
}
void launch_rzset_scatter(const SetinclChunk& c, const RzsArgs& a, const SetinclJobs& j, hipStream_t s) {
    if (c.n) hipLaunchKernelGGL(k_rzset_scatter, dim3(rzs_blocks(c.n, RZS_BLOCK)), dim3(RZS_BLOCK), 0, s, c, a, j);
}
void launch_rzset_reps(const SetinclChunk& c, const RzsArgs& a, uint32_t* out, hipStream_t s) {
    if (c.n) hipLaunchKernelGGL(k_rzset_reps, dim3(rzs_blocks(c.n, RZS_BLOCK)), dim3(RZS_BLOCK), 0, s, c, a, out);
}

}  // namespace zkv

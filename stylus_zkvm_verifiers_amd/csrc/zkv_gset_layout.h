// Slot layout of a Groth16 key-set batch (zkv_groth16_set_*): plain C++, shared by the C ABI and the host build of
// the tests (tests/host_sim/host_sim_gset_layout.cpp).
//
// The proofs of a batch are partitioned by key; key group k starts at slot start[k], a multiple of the proofs per wavefront of the
// Miller-loop mapping the batch takes (32 on lane pairs, 4 on 16 lanes, 1 on one or two wavefronts per proof), so that every
// wavefront of those kernels holds proofs of one key only.  The slots between a group's last proof and the next group are pad slots:
// they carry no proof.
#pragma once
#include <stddef.h>
#include <stdint.h>

namespace zkv {

// Proofs per wavefront of the Miller mappings, and the lanes-per-proof setting (zkv_ctx_set_lanes_per_proof) each corresponds to.
inline uint32_t gset_align_of_lanes(int lanes) { return lanes == 2 ? 32u : lanes == 16 ? 4u : 1u; }

// start[0 .. n_keys]: group k occupies slots [start[k], start[k] + cnt[k]), padded up to start[k + 1].  Returns the slot count.
inline uint64_t gset_layout(const uint32_t* cnt, uint32_t n_keys, uint32_t align, uint64_t* start) {
    uint64_t s = 0;
    for (uint32_t k = 0; k < n_keys; k++) {
        start[k] = s;
        s += ((uint64_t)cnt[k] + align - 1) / align * align;
    }
    start[n_keys] = s;
    return s;
}

// The mapping of a batch: `lanes` is what the automatic policy (or the caller) picked for the batch size.  An automatic choice steps
// to the next finer mapping (lane pairs -> 16 lanes -> one wavefront per proof) while the padded slot count exceeds 1.25 times the
// proofs; a mapping the caller fixed (fixed != 0) is kept.  Returns the lanes per proof and fills start[] (gset_layout).
inline int gset_choose(const uint32_t* cnt, uint32_t n_keys, int lanes, int fixed, uint64_t* start, uint64_t* slots) {
    uint64_t n = 0;
    for (uint32_t k = 0; k < n_keys; k++) n += cnt[k];
    for (;;) {
        *slots = gset_layout(cnt, n_keys, gset_align_of_lanes(lanes), start);
        if (fixed || 4 * *slots <= 5 * n || gset_align_of_lanes(lanes) == 1) return lanes;
        lanes = lanes == 2 ? 16 : 64;
    }
}

// Selector routers (the SP1 gateway and the RISC Zero router; DESIGN.md sections 12d and 17): the slots and compact records of one call.
// The demultiplexer counts the items of n_cols routed columns, tot[c] each with records of rec[c] bytes.  Columns [key0, key0 + n_keyed)
// are the keyed routes: together one key set, laid out by gset_choose from the mapping `lanes` their items would take (`fixed`: the
// caller's own choice, kept), so every keyed column starts on gset_align_of_lanes slots of the group's first slot and may end in pad
// slots; their records are rec[key0] bytes each, pad slots included.  Every other column takes one slot per item.  Columns lie in
// column order, slots and bytes back to back.
constexpr uint32_t ROUTE_MAX_COLS = 16;
struct RouteLayout {
    uint32_t start[ROUTE_MAX_COLS];                 // first slot of column c
    uint64_t base[ROUTE_MAX_COLS];                  // byte offset of its first record
    uint64_t g0, b0, m, gstart[ROUTE_MAX_COLS + 1]; // keyed group: first slot, byte offset, slots (pads included), first slot of every key in the group
    int lanes;                                      // ... and its Miller mapping (0 without keyed columns)
    uint64_t slots, bytes;                          // of the call
    uint32_t n_runs;                                // runs of live slots that lie back to back, in slot order: [run_at[q], run_at[q] + run_n[q])
    uint64_t run_at[ROUTE_MAX_COLS], run_n[ROUTE_MAX_COLS];
};
inline void route_layout(const uint32_t* tot, uint32_t n_cols, uint32_t key0, uint32_t n_keyed, const uint32_t* rec, int lanes, int fixed, RouteLayout* L) {
    uint64_t slots = 0, bytes = 0;
    L->g0 = L->b0 = L->m = 0; L->lanes = 0; L->n_runs = 0;
    for (uint32_t k = 0; k <= ROUTE_MAX_COLS; k++) L->gstart[k] = 0;
    for (uint32_t c = 0; c < n_cols; c++) {
        if (n_keyed && c == key0) {
            L->lanes = gset_choose(tot + key0, n_keyed, lanes, fixed, L->gstart, &L->m);
            L->g0 = slots; L->b0 = bytes;
        }
        if (c >= key0 && c < key0 + n_keyed) {
            L->start[c] = (uint32_t)(L->g0 + L->gstart[c - key0]); L->base[c] = L->b0 + (uint64_t)rec[key0] * L->gstart[c - key0];
            if (c + 1 == key0 + n_keyed) { slots = L->g0 + L->m; bytes = L->b0 + (uint64_t)rec[key0] * L->m; }
        } else {
            L->start[c] = (uint32_t)slots; L->base[c] = bytes;
            slots += tot[c]; bytes += (uint64_t)tot[c] * rec[c];
        }
        if (!tot[c]) continue;
        if (L->n_runs && L->run_at[L->n_runs - 1] + L->run_n[L->n_runs - 1] == L->start[c]) L->run_n[L->n_runs - 1] += tot[c];
        else { L->run_at[L->n_runs] = L->start[c]; L->run_n[L->n_runs] = tot[c]; L->n_runs++; }
    }
    L->slots = slots; L->bytes = bytes;
}

// PLONK key sets (zkv_plonk_set_*).  PREP runs one proof per lane, so every key group starts on a multiple of 64
// slots (one PREP wavefront); every Miller wavefront (32, 4 or 1 proofs) then holds one key as well.  The Miller mapping is the single-key
// PLONK policy of enqueue_chunk applied to the n placed proofs: one wavefront per proof at or below wave_below or when the caller fixed
// 64 / 128, 16 lanes at or below wide_below or when fixed to 16, lane pairs otherwise (fixed = 0: automatic).  No two-wavefront
// kernel (PLONK has no variable pair for a second wavefront to step) and no stepping to finer mappings (they do not reduce 64-slot
// padding).  Returns the lanes per proof (2, 16 or 64) and fills start[] (gset_layout, align 64).
inline int pset_choose(const uint32_t* cnt, uint32_t n_keys, int fixed, uint64_t wave_below, uint64_t wide_below, uint64_t* start, uint64_t* slots) {
    uint64_t n = 0;
    for (uint32_t k = 0; k < n_keys; k++) n += cnt[k];
    *slots = gset_layout(cnt, n_keys, 64, start);
    if (fixed == 64 || fixed == 128 || (!fixed && n <= wave_below)) return 64;
    if (fixed == 16 || (!fixed && n <= wide_below)) return 16;
    return 2;
}

// Aggregate check on a key set (zkv_ctx_set_aggregate_check).  Sub-batches must hold proofs of one key, and the
// aggregate Miller kernel deals a 64-proof block out to its lane pairs, so the unit of the aggregate region is A = max(64, sub) proofs.
// A capable key k (valid, alpha and beta finite) puts its first floor(cnt[k] / A) * A proofs, in caller order, into the aggregate region
// [0, R): the keys back to back, no pad slots.  Its other proofs and every proof of a key that cannot take the check go to the per-proof
// region [R, slots), laid out by gset_choose.
inline uint32_t gset_agg_unit(uint32_t sub) { return sub > 64u ? sub : 64u; }
// agg[k]: proofs of key k in the aggregate region, from slot astart[k]; rest[k]: its others, from slot pstart[k] (absolute; pstart[n_keys] =
// slots).  Returns the per-proof region's Miller mapping (gset_choose with `lanes`, `fixed`); *agg_slots = R.
inline int gset_agg_choose(const uint32_t* cnt, const uint8_t* capable, uint32_t n_keys, uint32_t sub, int lanes, int fixed, uint32_t* agg,
                           uint64_t* astart, uint32_t* rest, uint64_t* pstart, uint64_t* agg_slots, uint64_t* slots) {
    const uint32_t unit = gset_agg_unit(sub);
    uint64_t r = 0;
    for (uint32_t k = 0; k < n_keys; k++) {
        agg[k] = capable[k] ? cnt[k] / unit * unit : 0u;
        rest[k] = cnt[k] - agg[k];
        astart[k] = r;
        r += agg[k];
    }
    astart[n_keys] = r;
    *agg_slots = r;
    const int l = gset_choose(rest, n_keys, lanes, fixed, pstart, slots);
    for (uint32_t k = 0; k <= n_keys; k++) pstart[k] += r;
    *slots += r;
    return l;
}
// The slot of the proof of rank `rank` (in caller order) among key k's proofs
inline uint64_t gset_agg_slot(uint32_t k, uint32_t rank, const uint32_t* agg, const uint64_t* astart, const uint64_t* pstart) {
    return rank < agg[k] ? astart[k] + rank : pstart[k] + (rank - agg[k]);
}

// Selector routers with the aggregate check on their keyed group: route_layout with the keyed block laid out by
// gset_agg_choose over the keyed columns' totals.  capable[k]: keyed route k can take the check (null: the check does not engage);
// `lanes`: the mapping the items of the per-proof region would take.  The block [g0, g0 + m) is then two regions: the aggregate region
// [g0, g0 + R), every capable key's first floor(tot / A) * A items back to back, no pad slots, and behind it the per-proof region, the
// rests by gset_choose.  R and every agg[k] are multiples of A = gset_agg_unit(sub) >= 64, so every 64-slot block and every sub-batch of
// the aggregate region lies inside one key.  Records stay rows of rec[key0] bytes: group slot j at b0 + rec[key0] * j.  The columns
// before and after the block are route_layout's.  In L, a keyed column's start, base and gstart are those of its per-proof part
// (gstart[k] = pstart[k] >= R); the live runs: the aggregate region is one run, which the first non-empty per-proof part continues
// (it starts at slot R), so there are never more runs than non-empty columns.  With R = 0 -- no capable key holds A items -- L is
// route_layout's result bit for bit, and pstart = gstart.
// Slot bound: the aggregate region pads nothing and gset_choose pads every key's rest to at most 32 slots, so the call takes at most
// n + 31 * n_keyed slots, as without the check.
struct RouteAggLayout {
    uint64_t R;                                     // slots of the aggregate region (0: one region, the check does not engage)
    uint32_t agg[ROUTE_MAX_COLS], rest[ROUTE_MAX_COLS];        // keyed route k: items in the aggregate region, and the others
    uint64_t astart[ROUTE_MAX_COLS + 1], pstart[ROUTE_MAX_COLS + 1];      // their first group slots (gset_agg_choose; index 0 = slot g0)
};
inline void route_layout_agg(const uint32_t* tot, uint32_t n_cols, uint32_t key0, uint32_t n_keyed, const uint32_t* rec, int lanes, int fixed,
                             const uint8_t* capable, uint32_t sub, RouteLayout* L, RouteAggLayout* A) {
    const uint32_t unit = gset_agg_unit(sub);
    A->R = 0;
    for (uint32_t k = 0; k < ROUTE_MAX_COLS; k++) { A->agg[k] = 0; A->rest[k] = k < n_keyed ? tot[key0 + k] : 0; }
    for (uint32_t k = 0; k <= ROUTE_MAX_COLS; k++) A->astart[k] = A->pstart[k] = 0;
    uint64_t r = 0;
    if (capable) for (uint32_t k = 0; k < n_keyed; k++) if (capable[k]) r += tot[key0 + k] / unit * unit;
    if (!r) {
        route_layout(tot, n_cols, key0, n_keyed, rec, lanes, fixed, L);
        for (uint32_t k = 0; k <= n_keyed; k++) A->pstart[k] = L->gstart[k];
        return;
    }
    uint64_t slots = 0, bytes = 0;
    L->g0 = L->b0 = L->m = 0; L->lanes = 0; L->n_runs = 0;
    for (uint32_t k = 0; k <= ROUTE_MAX_COLS; k++) L->gstart[k] = 0;
    auto run = [L](uint64_t at, uint64_t n) {
        if (!n) return;
        if (L->n_runs && L->run_at[L->n_runs - 1] + L->run_n[L->n_runs - 1] == at) L->run_n[L->n_runs - 1] += n;
        else { L->run_at[L->n_runs] = at; L->run_n[L->n_runs] = n; L->n_runs++; }
    };
    for (uint32_t c = 0; c < n_cols; c++) {
        if (c == key0) {
            L->lanes = gset_agg_choose(tot + key0, capable, n_keyed, sub, lanes, fixed, A->agg, A->astart, A->rest, A->pstart, &A->R, &L->m);
            for (uint32_t k = 0; k <= n_keyed; k++) L->gstart[k] = A->pstart[k];
            L->g0 = slots; L->b0 = bytes;
            run(L->g0, A->R);
        }
        if (c >= key0 && c < key0 + n_keyed) {
            L->start[c] = (uint32_t)(L->g0 + L->gstart[c - key0]); L->base[c] = L->b0 + (uint64_t)rec[key0] * L->gstart[c - key0];
            if (c + 1 == key0 + n_keyed) { slots = L->g0 + L->m; bytes = L->b0 + (uint64_t)rec[key0] * L->m; }
            run(L->start[c], A->rest[c - key0]);
        } else {
            L->start[c] = (uint32_t)slots; L->base[c] = bytes;
            slots += tot[c]; bytes += (uint64_t)tot[c] * rec[c];
            run(L->start[c], tot[c]);
        }
    }
    L->slots = slots; L->bytes = bytes;
}

// Aggregate check on a PLONK key set (zkv_plonk_set_agg.h).  A PLONK key gives the pairing check nothing but its two
// G2 points, so a sub-batch may hold proofs of any keys of one SRS class (keys with the same [1]_2 | [tau]_2 bytes): cls[k] is key k's class,
// capable[c] whether class c's points passed the set-up validation.  Key groups stay on 64-slot boundaries (PREP wavefronts stay
// key-uniform) but are ordered class by class, the capable classes first, and every class region starts on a multiple of
// A = gset_agg_unit(sub) slots: a sub-batch is `sub` consecutive slots of a class region whatever keys they belong to, pad slots included as
// dead lanes, and no sub-batch spans two classes.  Slots [0, R) are the capable classes' regions (the aggregate region), [R, slots) those of
// the other classes (per-proof path).  A class without proofs takes no slots.
// start[k]: first slot of key k's group (NOT monotone in k; start[n_keys] = slots); cbeg[c], cend[c]: class c's region (cend a multiple of A).
// Returns the per-proof region's Miller mapping (pset_choose's policy applied to its proofs); *agg_slots = R.
inline int pset_agg_choose(const uint32_t* cnt, const uint32_t* cls, uint32_t n_keys, const uint8_t* capable, uint32_t n_cls, uint32_t sub, int fixed,
                           uint64_t wave_below, uint64_t wide_below, uint64_t* start, uint64_t* cbeg, uint64_t* cend, uint64_t* agg_slots, uint64_t* slots) {
    const uint64_t unit = gset_agg_unit(sub);
    for (uint32_t c = 0; c < n_cls; c++) cend[c] = 0;
    for (uint32_t k = 0; k < n_keys; k++) cend[cls[k]] += ((uint64_t)cnt[k] + 63) / 64 * 64;       // the class's slots before rounding up to A
    uint64_t s = 0, rest = 0;
    for (int pass = 0; pass < 2; pass++) {                      // capable classes, then the others, each in class order
        for (uint32_t c = 0; c < n_cls; c++) {
            if ((capable[c] != 0) != (pass == 0)) continue;
            cbeg[c] = s;
            s += (cend[c] + unit - 1) / unit * unit;
        }
        if (pass == 0) *agg_slots = s;
    }
    *slots = s;
    for (uint32_t c = 0; c < n_cls; c++) cend[c] = cbeg[c];     // running first free slot of the class
    for (uint32_t k = 0; k < n_keys; k++) {
        start[k] = cend[cls[k]];
        cend[cls[k]] += ((uint64_t)cnt[k] + 63) / 64 * 64;
        if (!capable[cls[k]]) rest += cnt[k];
    }
    start[n_keys] = s;
    for (uint32_t c = 0; c < n_cls; c++) cend[c] = cbeg[c] + (cend[c] - cbeg[c] + unit - 1) / unit * unit;
    if (fixed == 64 || fixed == 128 || (!fixed && rest <= wave_below)) return 64;
    if (fixed == 16 || (!fixed && rest <= wide_below)) return 16;
    return 2;
}
// SRS classes of a PLONK set: class_of[k] numbered by first appearance in key order, by byte equality of the 256 G2 bytes (g2: 256 bytes per
// key); rep[c]: the first key of class c (rep may be null).  Returns the number of classes.
inline uint32_t pset_srs_classes(const uint8_t* g2, uint32_t n_keys, uint32_t* class_of, uint32_t* rep) {
    uint32_t n_cls = 0;
    for (uint32_t k = 0; k < n_keys; k++) {
        uint32_t c = n_cls;
        for (uint32_t j = 0; j < k; j++) {
            bool eq = true;
            for (uint32_t b = 0; b < 256 && eq; b++) eq = g2[256 * (size_t)j + b] == g2[256 * (size_t)k + b];
            if (eq) { c = class_of[j]; break; }
        }
        class_of[k] = c;
        if (c == n_cls) { if (rep) rep[n_cls] = k; n_cls++; }
    }
    return n_cls;
}
// Where aggregate chunks over [0, R) end when the workspace holds `cap` slots: multiples of A, so no sub-batch straddles two chunks
// (0: the workspace is smaller than one unit and the call takes the per-proof path).
inline uint64_t pset_agg_chunk_slots(uint64_t cap, uint32_t sub) { return cap / gset_agg_unit(sub) * gset_agg_unit(sub); }

// The pseudo-proofs of one aggregate chunk [base, base + m) of either kind of set: one per sub-batch of `sub` slots, n2 = m / sub of them.
// Region q is the slots [beg[q], end[q]) whose sub-batches take the line tables of key rep[q] (rep = null: key q): a Groth16 set passes
// one region per key (astart[k], astart[k] + agg[k]), a PLONK set one per SRS class (cbeg, cend, the class's first key), an incapable
// class as an empty region.  Regions are disjoint, and begin and end on multiples of `sub` as do the chunks.  The pseudo-proofs are laid out
// per region and padded to the proofs per wavefront of the Miller mapping, as the proofs themselves: gset_choose over the regions'
// sub-batch counts, starting from `lanes` (the mapping n2 proofs would take); when the padded slots exceed `cap`, the pseudo-workspace's
// capacity, one wavefront per pseudo-proof, which pads nothing.
// Fills nsb[q] (sub-batches of region q in the chunk), pst[0 .. n_regions] (region q's pseudo slots are [pst[q], pst[q + 1])), psl[t] (the
// slot of the chunk's sub-batch t, for every t of a region; the others are left alone) and skey2[0 .. *slots) (rep of the region of every
// pseudo slot, pad slots included); skey2 needs room for n2 + 31 * n_regions words.  Returns the lanes per pseudo-proof.
inline int gset_agg_chunk_plan(const uint64_t* beg, const uint64_t* end, const uint32_t* rep, uint32_t n_regions, uint64_t base, uint64_t m,
                               uint32_t sub, int lanes, uint64_t cap, uint32_t* nsb, uint64_t* pst, uint32_t* psl, uint32_t* skey2, uint64_t* slots) {
    for (uint32_t q = 0; q < n_regions; q++) {
        const uint64_t lo = beg[q] > base ? beg[q] : base, hi = end[q] < base + m ? end[q] : base + m;
        nsb[q] = hi > lo ? (uint32_t)((hi - lo) / sub) : 0u;
    }
    lanes = gset_choose(nsb, n_regions, lanes, 0, pst, slots);
    if (*slots > cap) lanes = gset_choose(nsb, n_regions, 64, 1, pst, slots);
    for (uint32_t q = 0; q < n_regions; q++) {
        if (!nsb[q]) continue;
        const uint64_t sb0 = ((beg[q] > base ? beg[q] : base) - base) / sub;
        for (uint32_t t = 0; t < nsb[q]; t++) psl[sb0 + t] = (uint32_t)(pst[q] + t);
        for (uint64_t w = pst[q]; w < pst[q + 1]; w++) skey2[w] = rep ? rep[q] : q;
    }
    return lanes;
}

}  // namespace zkv

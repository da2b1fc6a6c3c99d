// Host build of the class layout of the aggregate check on PLONK key sets (csrc/zkv_gset_layout.h: pset_agg_choose, pset_srs_classes,
// pset_agg_chunk_slots) for tests/test_plonk_key_sets_aggregate_host.py.  TEST ONLY.
#include <stdint.h>
#include "../../stylus_zkvm_verifiers_amd/csrc/zkv_gset_layout.h"
using namespace zkv;

extern "C" int hpa_choose(const uint32_t* cnt, const uint32_t* cls, uint32_t n_keys, const uint8_t* capable, uint32_t n_cls, uint32_t sub, int fixed,
                          uint64_t wave_below, uint64_t wide_below, uint64_t* start, uint64_t* cbeg, uint64_t* cend, uint64_t* agg_slots, uint64_t* slots) {
    return pset_agg_choose(cnt, cls, n_keys, capable, n_cls, sub, fixed, wave_below, wide_below, start, cbeg, cend, agg_slots, slots);
}
extern "C" uint32_t hpa_classes(const uint8_t* g2, uint32_t n_keys, uint32_t* class_of, uint32_t* rep) { return pset_srs_classes(g2, n_keys, class_of, rep); }
extern "C" uint64_t hpa_chunk_slots(uint64_t cap, uint32_t sub) { return pset_agg_chunk_slots(cap, sub); }

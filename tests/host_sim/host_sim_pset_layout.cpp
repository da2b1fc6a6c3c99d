// Host build of the PLONK key-set slot layout (csrc/zkv_gset_layout.h pset_choose) for tests/test_plonk_key_sets_host.py.
#include "../../stylus_zkvm_verifiers_amd/csrc/zkv_gset_layout.h"

extern "C" int hsp_choose(const uint32_t* cnt, uint32_t n_keys, int fixed, uint64_t wave_below, uint64_t wide_below, uint64_t* start, uint64_t* slots) {
    return zkv::pset_choose(cnt, n_keys, fixed, wave_below, wide_below, start, slots);
}

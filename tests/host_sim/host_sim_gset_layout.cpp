// Host build of the key-set slot layout (csrc/zkv_gset_layout.h) for tests/test_groth16_key_sets_host.py.
#include "../../stylus_zkvm_verifiers_amd/csrc/zkv_gset_layout.h"

extern "C" int hsg_choose(const uint32_t* cnt, uint32_t n_keys, int lanes, int fixed, uint64_t* start, uint64_t* slots) {
    return zkv::gset_choose(cnt, n_keys, lanes, fixed, start, slots);
}

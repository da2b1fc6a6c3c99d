// Host build of the known-answer harness (stylus_zkvm_verifiers_amd/csrc/zkv_selftest.h), one value per lane: the same case bodies
// k_selftest.hip runs, compiled with g++.  TEST ONLY.
#define ZKV_SELFTEST_BODIES 1
#include <stddef.h>
#include <stdint.h>
#include "../../stylus_zkvm_verifiers_amd/csrc/zkv_selftest.h"
using namespace zkv;

// hs_selftest(0, op, n, in, out): what zkv_diag_primitive(device, 0, op, n, in, out) returns on the device; -1 for an unknown op
extern "C" int hs_selftest(int mapping, int op, size_t n, const uint32_t* in, uint32_t* out) {
    int iw = 0, ow = 0;
    if (mapping != 0 || !selftest_io(mapping, op, &iw, &ow)) return -1;
    for (size_t i = 0; i < n; i++) selftest_lane(op, in + i * (size_t)iw, out + i * (size_t)ow);
    return 0;
}
// the (in, out) words per case of (mapping, op) as selftest_io states them; -1 for a pair this build does not run
extern "C" int hs_selftest_io(int mapping, int op, int* in_w, int* out_w) {
    return (mapping != 0 || !selftest_io(mapping, op, in_w, out_w)) ? -1 : 0;
}

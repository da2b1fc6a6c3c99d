// Known-answer harness, one value per lane (zkv_selftest.h, mapping 0): the primitives of k_prep, k_msm, k_plonk, k_precompile and the
// aggregate check, compiled with the shipped flags.  TEST ONLY (zkv_diag_primitive).
#define ZKV_SELFTEST_BODIES 1
#include "zkv_internal.h"
#include "zkv_selftest.h"

namespace zkv {

// one case per lane; the host pads the batch to whole wavefronts
__global__ __launch_bounds__(64) void k_selftest_lane(int op, int in_w, int out_w, const uint32_t* __restrict__ in, uint32_t* __restrict__ out) {
    const size_t i = (size_t)blockIdx.x * 64 + threadIdx.x;
    selftest_lane(op, in + i * (size_t)in_w, out + i * (size_t)out_w);
}

void launch_selftest_lane(int op, unsigned waves, const uint32_t* in, uint32_t* out, hipStream_t s) {
    int iw = 0, ow = 0;
    selftest_io(0, op, &iw, &ow);
    hipLaunchKernelGGL(k_selftest_lane, dim3(waves), dim3(64), 0, s, op, iw, ow, in, out);
}

}  // namespace zkv

// Known-answer harness, lane pairs and wide groups (zkv_selftest.h, mappings 1-3): the ZKV_PAIRED primitives of k_miller2, k_finalexp2
// and the precompile pairing with their operands exchanged between the two lanes of a pair, and the Fp12 routines of k_wide.hip with
// one case per 16 lanes (four per wavefront) or per wavefront.  TEST ONLY (zkv_diag_primitive).
#define ZKV_PAIRED 1
#define ZKV_SELFTEST_BODIES 1
#include "zkv_internal.h"
#include "zkv_selftest.h"

namespace zkv {

// one case per lane pair, 32 per wavefront; every lane has its own column of the LDS block (slots a, b, d and the L9 accumulator)
__global__ __launch_bounds__(64) void k_selftest_pair(int op, int in_w, int out_w, const uint32_t* __restrict__ in, uint32_t* __restrict__ out) {
    __shared__ uint32_t lds[(144 + 54) * 64];
    const size_t i = (size_t)blockIdx.x * 32 + (threadIdx.x >> 1);
    selftest_pair(op, in + i * (size_t)in_w, out + i * (size_t)out_w, lds + threadIdx.x);
}
// the line steps of k_miller2 as column sums (selftest_line_sums), one case per lane pair; f and T in the columns k_selftest_pair gives them
__global__ __launch_bounds__(64) void k_selftest_line_sums(const uint32_t* __restrict__ in, uint32_t* __restrict__ out) {
    __shared__ uint32_t lds[(48 + 24) * 64];
    const size_t i = (size_t)blockIdx.x * 32 + (threadIdx.x >> 1);
    selftest_line_sums(in + i * (size_t)ST_LINE_SUMS_IN, out + i * (size_t)ST_LINE_SUMS_OUT, lds + threadIdx.x);
}
// one case per 16 S lanes, the group's slots as in k_wide.hip (pair q = (lane >> 1) & 7, pairs 6 and 7 shadow 0 and 1; slice = lane bits 4-5)
template <int S>
__device__ __forceinline__ void selftest_wide_body(int op, int in_w, int out_w, const uint32_t* in, uint32_t* out, uint32_t* lds) {
    constexpr int GROUP = 16 * S;
    const uint32_t g = threadIdx.x / GROUP;
    WL w;
    w.q = (int)((threadIdx.x >> 1) & 7u);
    if (w.q >= 6) w.q -= 6;
    w.s = (int)((threadIdx.x % GROUP) >> 4);
    const size_t i = (size_t)blockIdx.x * (64 / GROUP) + g;
    selftest_wide<S>(op, in + i * (size_t)in_w, out + i * (size_t)out_w, lds + g * ST_WIDE_SLOT, w);
}
__global__ __launch_bounds__(64) void k_selftest_wide_s1(int op, int in_w, int out_w, const uint32_t* __restrict__ in, uint32_t* __restrict__ out) {
    __shared__ uint32_t lds[4 * ST_WIDE_SLOT];
    selftest_wide_body<1>(op, in_w, out_w, in, out, lds);
}
__global__ __launch_bounds__(64) void k_selftest_wide_s4(int op, int in_w, int out_w, const uint32_t* __restrict__ in, uint32_t* __restrict__ out) {
    __shared__ uint32_t lds[ST_WIDE_SLOT];
    selftest_wide_body<4>(op, in_w, out_w, in, out, lds);
}

void launch_selftest_pair(int mapping, int op, unsigned waves, const uint32_t* in, uint32_t* out, hipStream_t s) {
    int iw = 0, ow = 0;
    selftest_io(mapping, op, &iw, &ow);
    if (mapping == 1) hipLaunchKernelGGL(k_selftest_pair, dim3(waves), dim3(64), 0, s, op, iw, ow, in, out);
    else if (mapping == 2) hipLaunchKernelGGL(k_selftest_wide_s1, dim3(waves), dim3(64), 0, s, op, iw, ow, in, out);
    else hipLaunchKernelGGL(k_selftest_wide_s4, dim3(waves), dim3(64), 0, s, op, iw, ow, in, out);
}
void launch_selftest_line_sums(unsigned waves, const uint32_t* in, uint32_t* out, hipStream_t s) {
    hipLaunchKernelGGL(k_selftest_line_sums, dim3(waves), dim3(64), 0, s, in, out);
}

}  // namespace zkv

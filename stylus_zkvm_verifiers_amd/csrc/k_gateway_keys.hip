// SP1 gateway, Groth16 routes with caller-supplied keys (include/zkv_sp1_gateway_keys.h).  The keyed routes of a
// gateway are one Groth16 key set (n_ic = 3, SP1 sign convention); the demultiplexer (k_gateway.hip) has sorted their proofs into the
// set's slot layout (zkv_gset_layout.h: every route starts on a multiple of the proofs per wavefront of the Miller mapping).  This unit
// is the stage between the two: the SP1 front end of k_prep_sp1 per slot with the slot's key, one slot per lane.  It stages the two
// signals where k_gset_msm reads them and writes each slot's key for k_gset_msm / k_gset_miller; the remaining stages are the key sets'.
// Everything around the slot function -- record staging, key of slot, pad slots, the stores -- is gwset_prep_lane (zkv_gwset_prep.h),
// which the RISC Zero router's PREP kernel shares.
// Parity unpinned, except that a route holding the reference's own key and hash gives the pinned SP1 statuses.
#include "zkv_internal.h"
#include "zkv_gwset_prep.h"

namespace zkv {

__global__ __launch_bounds__(ZKV_BLOCK) void k_gwset_prep(GwsetChunk c, Workspace ws) {
    __shared__ uint32_t lds[ZKV_BLOCK * 65];
    gwset_prep_lane<2, GwsetSlot>(c, ws, lds, [](const GwsetChunk& ch, uint32_t k, size_t slot, const GwsetRec& rd, GwsetSlot& r) __attribute__((always_inline)) {
        gwset_prep_slot(ch.keys[k].tab->vk_valid, ch.len[slot], (const uint32_t*)(ch.vkeys + 32 * slot), ch.pv + ch.pvoff[slot], ch.pvlen[slot], rd, r);
    });
}
void launch_gwset_prep(const GwsetChunk& c, const Workspace& ws, hipStream_t s) {
    if (!c.m) return;
    hipLaunchKernelGGL(k_gwset_prep, dim3((unsigned)((c.m + ZKV_BLOCK - 1) / ZKV_BLOCK)), dim3(ZKV_BLOCK), 0, s, c, ws);
}

}  // namespace zkv

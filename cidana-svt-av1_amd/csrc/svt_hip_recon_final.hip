// svt_hip_recon_final.hip — svt_hip_recon_final_frame: the reconstruction of the final block list of every superblock of a picture
// (recon_clear_kernel, recon_bin_kernel and recon_final_kernel<0 .. 3>, kernel_recon_final.h): six launches on one stream.
// The checks, the scratch layout and the launch shapes are recon_final_plan.h's, the block and transform sizes av1_geom.h's.
#include <stddef.h>

#include "host_common.h"
#include "kernel_recon_final.h"

using namespace svtdev;
using namespace svthost;

static_assert(sizeof(svt_hip_md_decision) == 4 * RF_DEC_WORDS && offsetof(svt_hip_md_decision, eob) == 4 * RF_DEC_EOB01 &&
              offsetof(svt_hip_md_decision, tx_type) == 4 * RF_DEC_TX_TYPE, "recon_bin_kernel reads the record as eighteen words");
static_assert(RF_COUNTER_BYTES >= 4 * SVT_TX_SIZES_ALL && RF_COUNTER_BYTES % 16 == 0, "the counters, then the 16-byte items");

extern "C" size_t svt_hip_recon_final_scratch_bytes(uint32_t nsb) { return recon_final_scratch_bytes(nsb); }

extern "C" int svt_hip_recon_final_frame(const svt_hip_recon_final_args* a, void* stream) {
    if (int rc = require_init()) return rc;
    if (int rc = recon_final_check(a)) return rc;
    hipStream_t s = (hipStream_t)stream;
    const bool stream_out = a->d_sb_qcoeff[0] != nullptr;
    ReconBinDesc B{};
    B.final_blk = (const uint32_t*)a->d_final; B.final_count = a->d_final_count; B.decision = (const uint32_t*)a->d_decision;
    B.status = a->d_status; B.coeff_offset = a->d_coeff_offset;
    B.counters = (uint32_t*)a->d_scratch; B.items = (uint4*)((char*)a->d_scratch + RF_COUNTER_BYTES);
    B.nsb = a->nsb; B.nsrc = a->nsrc; B.planes = (uint32_t)a->planes; B.stream = stream_out; B.ngroups = a->ngroups;
    ReconFinalDesc R{};
    R.counters = B.counters; R.items = B.items; R.nsb = a->nsb; R.ngroups = (uint32_t)a->ngroups; R.planes = (uint32_t)a->planes; R.stream = stream_out;
    for (int p = 0; p < a->planes; p++) {
        B.width[p] = a->width[p]; B.height[p] = a->height[p];
        R.recon[p] = a->d_recon[p]; R.stride[p] = a->stride[p]; R.width[p] = a->width[p]; R.height[p] = a->height[p]; R.sbq[p] = a->d_sb_qcoeff[p];
    }
    for (int g = 0; g < a->ngroups; g++) {
        const svt_hip_recon_final_group& G = a->groups[g];
        B.g[g].src_first = G.src_first; B.g[g].nblocks = G.nblocks; B.g[g].bsize = (uint8_t)G.bsize; B.g[g].tx_type_uv = (uint8_t)G.tx_type_uv;
        R.g[g].nblocks = G.nblocks;
        R.g[g].txs = (uint32_t)bsize_tx(G.bsize) | (uint32_t)bsize_tx_uv(G.bsize) << 8 | (uint32_t)bsize_tx_uv(G.bsize) << 16;
        for (int p = 0; p < a->planes; p++) { R.g[g].pred[p] = G.d_best_pred[p]; R.g[g].dq[p] = G.d_best_dqcoeff[p]; R.g[g].q[p] = stream_out ? G.d_best_qcoeff[p] : nullptr; }
    }
    hipLaunchKernelGGL(recon_clear_kernel, dim3(1), dim3(64), 0, s, B.counters);
    hipLaunchKernelGGL(recon_bin_kernel, dim3(recon_final_bin_grid(a->nsb)), dim3(RF_BIN_THREADS), 0, s, B);
    if (int rc = launch_status("recon_final bin")) return rc;
    if (g_tune_recon_final_bin_only) return SVT_HIP_OK;                    // (a measuring probe: the planes are not written)
    hipLaunchKernelGGL(recon_final_kernel<3>, dim3(recon_final_class_grid(3, a->nsb)), dim3(RfClass<3>::WAVES * 64), 0, s, R);      // the long workgroups first
    hipLaunchKernelGGL(recon_final_kernel<2>, dim3(recon_final_class_grid(2, a->nsb)), dim3(RfClass<2>::WAVES * 64), 0, s, R);
    hipLaunchKernelGGL(recon_final_kernel<1>, dim3(recon_final_class_grid(1, a->nsb)), dim3(RfClass<1>::WAVES * 64), 0, s, R);
    hipLaunchKernelGGL(recon_final_kernel<0>, dim3(recon_final_class_grid(0, a->nsb)), dim3(RfClass<0>::WAVES * 64), 0, s, R);
    return launch_status("recon_final");
}

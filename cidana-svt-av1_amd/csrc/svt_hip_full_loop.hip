// svt_hip_full_loop.hip — svt_hip_full_loop_frame: the fused luma mode-decision full loop (full_loop_kernel, kernel_full_loop.h), one
// launch per register class and per FL_MAX_GROUPS groups.  What is left here: the group-table fill and the launches (full_loop_enqueue);
// the argument check is md_plan.h's.
#include "host_common.h"
#include "kernel_full_loop.h"

using namespace svtdev;
using namespace svthost;

template <int CLS>
static int full_loop_launch(const FullLoopDesc& fd, uint32_t wgs, hipStream_t s) {
    hipLaunchKernelGGL((full_loop_kernel<CLS>), dim3(wgs), dim3(FullLoopClass<CLS>::THREADS), 0, s, fd);
    return launch_status("full_loop");
}

int svthost::full_loop_enqueue(const svt_hip_full_loop_group* groups, int ngroups, int flavour, const svt_hip_qrows& q, hipStream_t s) {
    QParams qps[3];
    for (int ls = 0; ls < 3; ls++) qps[ls] = make_qparams(q, ls);
    // the 64x64 class first, the small sizes last: the long workgroups start early
    for (int cls = 2; cls >= 0; cls--) {
        GroupTable<FullLoopDesc, FL_MAX_GROUPS> tab;
        tab.desc.avx2 = flavour == SVT_HIP_FLAVOUR_AVX2;
        auto launch = [&](const FullLoopDesc& fd, uint32_t total) -> int {
            return cls == 2 ? full_loop_launch<2>(fd, total, s) : (cls == 1 ? full_loop_launch<1>(fd, total, s) : full_loop_launch<0>(fd, total, s));
        };
        for (int g = 0; g < ngroups; g++) {
            const svt_hip_full_loop_group& G = groups[g];
            if (G.nblocks == 0 || tx_class_of(G.tx_size) != cls) continue;
            const uint32_t per_wg = tx_staged_blocks_per_wg(G.tx_size);
            FullLoopGroupDev* D = tab.add((G.nblocks + per_wg - 1) / per_wg, launch);
            if (!D) return tab.rc;
            D->src = (const uint8_t*)G.d_src; D->pred = (const uint8_t*)G.d_pred; D->src_xy = G.d_src_xy; D->pred_xy = G.d_pred_xy;
            D->iscan = G.d_iscan; D->dist = (unsigned long long*)G.d_dist; D->eob = G.d_eob; D->qcoeff = G.d_qcoeff; D->dqcoeff = G.d_dqcoeff;
            D->src_stride = G.src_stride; D->pred_stride = G.pred_stride; D->nblocks = G.nblocks;
            D->tx_size = G.tx_size; D->ntypes = G.ntypes;
            memcpy(D->types, G.tx_types, sizeof(D->types));
            D->qp = qps[tx_log_scale(G.tx_size)];
        }
        if (int rc = tab.flush(launch)) return rc;
    }
    return SVT_HIP_OK;
}

extern "C" int svt_hip_full_loop_frame(const svt_hip_full_loop_group* groups, int ngroups, int flavour, const int16_t* zbin,
                                       const int16_t* round, const int16_t* quant, const int16_t* quant_shift, const int16_t* dequant,
                                       void* stream) {
    const svt_hip_qrows q = {zbin, round, quant, quant_shift, dequant};
    if (int rc = require_init()) return rc;
    if (int rc = full_loop_check(groups, ngroups, flavour, q)) return rc;
    return full_loop_enqueue(groups, ngroups, flavour, q, (hipStream_t)stream);
}

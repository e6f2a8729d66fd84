// svt_hip_full_loop.hip — svt_hip_full_loop_frame: the fused luma mode-decision full loop (full_loop_kernel, kernel_full_loop.h), one
// launch per register class and per FL_MAX_GROUPS groups.
#include "host_common.h"
#include "kernel_full_loop.h"

using namespace svtdev;
using namespace svthost;

int svthost::full_loop_check(const svt_hip_full_loop_group* groups, int ngroups, int flavour, const int16_t* zbin, const int16_t* round,
                             const int16_t* quant, const int16_t* quant_shift, const int16_t* dequant) {
    if (ngroups < 0 || (ngroups > 0 && !groups)) return set_err(SVT_HIP_ERR_INVALID, "NULL group list");
    if (flavour != SVT_HIP_FLAVOUR_C && flavour != SVT_HIP_FLAVOUR_AVX2) return set_err(SVT_HIP_ERR_INVALID, "flavour %d", flavour);
    if (!zbin || !round || !quant || !quant_shift || !dequant) return set_err(SVT_HIP_ERR_INVALID, "NULL quantiser table");
    for (int i = 0; i < 2; i++) {
        const int qs = quant_shift[i];
        if (qs <= 0 || (qs & (qs - 1))) return set_err(SVT_HIP_ERR_INVALID, "quant_shift[%d] = %d is not a power of two", i, qs);
        if (dequant[i] < 0 || round[i] < 0) return set_err(SVT_HIP_ERR_INVALID, "negative quantiser table entry");
    }
    for (int ls = 0; ls < 3; ls++)
        if (!quant_params(zbin, round, quant, quant_shift, dequant, ls).fast_ok)
            return set_err(SVT_HIP_ERR_INVALID, "quantiser table outside the one-product quantiser's range (log_scale %d)", ls);
    for (int g = 0; g < ngroups; g++) {
        const svt_hip_full_loop_group& G = groups[g];
        if (int rc = group_types_check(g, G.tx_size, G.ntypes, G.tx_types)) return rc;
        if (G.nblocks == 0) continue;
        if (G.nblocks > 0x7fffffffu) return set_err(SVT_HIP_ERR_INVALID, "group %d: nblocks too large", g);
        if (!G.d_src || !G.d_pred || !G.d_iscan || !G.d_dist || !G.d_eob) return set_err(SVT_HIP_ERR_INVALID, "group %d: NULL member", g);
        if (((uintptr_t)G.d_iscan & 7) || ((uintptr_t)G.d_dist & 15) || ((uintptr_t)G.d_qcoeff & 15) || ((uintptr_t)G.d_dqcoeff & 15))
            return set_err(SVT_HIP_ERR_INVALID, "group %d: misaligned buffer (d_iscan 8 bytes, d_dist / d_qcoeff / d_dqcoeff 16 bytes)", g);
        if ((G.d_src_xy && G.src_stride < (uint32_t)kTxW[G.tx_size]) || (G.d_pred_xy && G.pred_stride < (uint32_t)kTxW[G.tx_size]))
            return set_err(SVT_HIP_ERR_INVALID, "group %d: plane stride below the block width", g);
    }
    return SVT_HIP_OK;
}

template <int CLS>
static int full_loop_launch(const FullLoopDesc& fd, uint32_t wgs, hipStream_t s) {
    hipLaunchKernelGGL((full_loop_kernel<CLS>), dim3(wgs), dim3(FullLoopClass<CLS>::THREADS), 0, s, fd);
    return launch_status("full_loop");
}

extern "C" int svt_hip_full_loop_frame(const svt_hip_full_loop_group* groups, int ngroups, int flavour, const int16_t* zbin,
                                       const int16_t* round, const int16_t* quant, const int16_t* quant_shift, const int16_t* dequant,
                                       void* stream) {
    if (int rc = require_init()) return rc;
    if (int rc = full_loop_check(groups, ngroups, flavour, zbin, round, quant, quant_shift, dequant)) return rc;
    hipStream_t s = (hipStream_t)stream;
    QParams qps[3];
    for (int ls = 0; ls < 3; ls++) qps[ls] = quant_params(zbin, round, quant, quant_shift, dequant, ls);
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
            const uint32_t per_wg = staged_blocks_per_wg(G.tx_size);
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

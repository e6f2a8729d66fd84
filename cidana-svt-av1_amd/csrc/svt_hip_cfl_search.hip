// svt_hip_cfl_search.hip — the CfL alpha search of mode decision (kernel_cfl_search.h): svt_hip_cfl_search_frame, the table (one
// cfl_search_kernel launch per CFS_MAX_GROUPS groups, then svt_hip_coeff_rate_frame's launches over the candidates in the scratch);
// svt_hip_cfl_decide_frame, cfl_rd_pick_alpha's walk (one launch per CFD_MAX_GROUPS groups); svt_hip_cfl_pick_frame, both on one stream
// as host composition, the tables the caller does not keep in the scratch.  What is left here: the two kernels' group-table fills and
// launches (search_enqueue, decide_enqueue) and the entry points; the checks, the scratch layouts and the stages' groups are md_plan.h's.
#include "host_common.h"
#include "kernel_cfl_search.h"

using namespace svtdev;
using namespace svthost;

static_assert(sizeof(svt_hip_cfl_decision) == 32 && alignof(svt_hip_cfl_decision) == 8, "cfl_decide_kernel stores the record as four words");
static_assert(SVT_HIP_CFL_NALPHA == CFS_NALPHA, "svt_hip_dsp.h");

static int search_enqueue(const svt_hip_cfl_search_group* groups, int ngroups, int flavour, const svt_hip_qrows* q_cb, const svt_hip_qrows* q_cr,
                   const std::vector<svt_hip_coeff_rate_group>& cr, hipStream_t s) {
    GroupTable<CflSearchDesc, CFS_MAX_GROUPS> tab;
    tab.desc.avx2 = flavour == SVT_HIP_FLAVOUR_AVX2;
    tab.desc.qp[0] = make_qparams(*q_cb, 0);
    tab.desc.qp[1] = make_qparams(*q_cr, 0);
    auto launch = [&](const CflSearchDesc& fd, uint32_t total) -> int {
        hipLaunchKernelGGL(cfl_search_kernel, dim3(total), dim3(FullLoopClass<0>::THREADS), 0, s, fd);
        return launch_status("cfl_search");
    };
    for (int g = 0; g < ngroups; g++) {
        const svt_hip_cfl_search_group& G = groups[g];
        if (G.nblocks == 0) continue;
        // a workgroup's waves take (blocks, plane) units: half as many blocks as a staged body's workgroup
        const uint32_t per_wg = tx_staged_blocks_per_wg(G.tx_size) / 2;
        CflSearchGroupDev* D = tab.add((G.nblocks + per_wg - 1) / per_wg, launch);
        if (!D) return tab.rc;
        const svt_hip_coeff_rate_group& C = cr[(size_t)g];
        D->luma = G.d_luma_recon; D->xy = G.d_xy; D->iscan = G.d_iscan;
        for (int p = 0; p < 2; p++) {
            D->src[p] = G.d_src[p]; D->pred[p] = G.d_pred[p]; D->skip_ctx[p] = G.d_txb_skip_ctx[p]; D->dc_ctx[p] = G.d_dc_sign_ctx[p];
            D->src_stride[p] = G.src_stride[p]; D->pred_stride[p] = G.pred_stride[p];
        }
        D->dist = (unsigned long long*)G.d_dist; D->eob = G.d_eob;
        D->qcoeff = (int32_t*)C.d_qcoeff; D->skip_out = (uint8_t*)C.d_txb_skip_ctx; D->dc_out = (uint8_t*)C.d_dc_sign_ctx;
        D->luma_stride = G.luma_stride; D->nblocks = G.nblocks; D->tx_size = G.tx_size; D->tx_type = G.tx_type;
    }
    if (int rc = tab.flush(launch)) return rc;
    return coeff_rate_enqueue(cr.data(), ngroups, s);
}

static int decide_enqueue(const svt_hip_cfl_decide_group* groups, int ngroups, hipStream_t s) {
    GroupTable<CflDecideDesc, CFD_MAX_GROUPS> tab;
    auto launch = [&](const CflDecideDesc& fd, uint32_t total) -> int {
        hipLaunchKernelGGL(cfl_decide_kernel, dim3(total), dim3(CFD_THREADS), 0, s, fd);
        return launch_status("cfl_decide");
    };
    for (int g = 0; g < ngroups; g++) {
        const svt_hip_cfl_decide_group& G = groups[g];
        if (G.nblocks == 0) continue;
        CflDecideGroupDev* D = tab.add((G.nblocks + CFD_THREADS - 1) / CFD_THREADS, launch);
        if (!D) return tab.rc;
        D->dist = (const unsigned long long*)G.d_dist; D->bits = (const unsigned long long*)G.d_bits; D->alpha_rate = G.d_alpha_rate;
        D->cfl_mode_bits = G.d_cfl_mode_bits; D->dc_mode_bits = G.d_dc_mode_bits; D->decision = (unsigned long long*)G.d_decision;
        D->alpha_cb = G.d_alpha_q3_cb; D->alpha_cr = G.d_alpha_q3_cr; D->nblocks = G.nblocks; D->lambda = G.lambda;
    }
    return tab.flush(launch);
}

extern "C" size_t svt_hip_cfl_search_scratch_bytes(const svt_hip_cfl_search_group* groups, int ngroups) {
    return scratch_bytes_of(cfl_search_walk, groups, ngroups);
}

extern "C" int svt_hip_cfl_search_frame(const svt_hip_cfl_search_group* groups, int ngroups, int flavour, const svt_hip_qrows* q_cb,
                                        const svt_hip_qrows* q_cr, void* d_scratch, size_t scratch_bytes, void* stream) {
    if (int rc = require_init()) return rc;
    CflStages st;
    if (int rc = plan_stages(cfl_search_walk, groups, ngroups, d_scratch, scratch_bytes, &st)) return rc;
    if (int rc = cfl_search_check(groups, ngroups, flavour, q_cb, q_cr)) return rc;
    if (int rc = coeff_rate_check(st.cr.data(), ngroups)) return rc;
    return search_enqueue(groups, ngroups, flavour, q_cb, q_cr, st.cr, (hipStream_t)stream);
}

extern "C" int svt_hip_cfl_decide_frame(const svt_hip_cfl_decide_group* groups, int ngroups, void* stream) {
    if (int rc = require_init()) return rc;
    if (int rc = cfl_decide_check(groups, ngroups)) return rc;
    return decide_enqueue(groups, ngroups, (hipStream_t)stream);
}

extern "C" size_t svt_hip_cfl_pick_scratch_bytes(const svt_hip_cfl_pick_group* groups, int ngroups) {
    return scratch_bytes_of(cfl_pick_walk, groups, ngroups);
}

extern "C" int svt_hip_cfl_pick_frame(const svt_hip_cfl_pick_group* groups, int ngroups, int flavour, const svt_hip_qrows* q_cb,
                                      const svt_hip_qrows* q_cr, void* d_scratch, size_t scratch_bytes, void* stream) {
    if (int rc = require_init()) return rc;
    CflStages st;
    if (int rc = plan_stages(cfl_pick_walk, groups, ngroups, d_scratch, scratch_bytes, &st)) return rc;
    // both stages' arguments before the first launch
    if (int rc = cfl_search_check(st.sg.data(), ngroups, flavour, q_cb, q_cr)) return rc;
    if (int rc = coeff_rate_check(st.cr.data(), ngroups)) return rc;
    if (int rc = cfl_decide_check(st.dg.data(), ngroups)) return rc;
    if (int rc = search_enqueue(st.sg.data(), ngroups, flavour, q_cb, q_cr, st.cr, (hipStream_t)stream)) return rc;
    return decide_enqueue(st.dg.data(), ngroups, (hipStream_t)stream);
}

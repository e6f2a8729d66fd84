// svt_hip_inter_fast.hip — svt_hip_inter_fast_pick_frame: fast cost of the inter candidates, the N best of the combined list, their order
// and the survivors' records (inter_pick_kernel, kernel_inter_fast_pick.h), one launch per non-empty group;
// svt_hip_inter_fast_search_frame, the whole inter fast search as host composition: distortion-only prediction -> pick -> prediction of
// the survivors -> the intra survivors' predictions copied in, on one stream.  The checks, the scratch layout and the stages' groups are
// inter_fast_plan.h's; what is left here is the kernel arguments and the launches.
#include "host_common.h"
#include "inter_fast_plan.h"
#include "kernel_inter_fast_pick.h"

using namespace svtdev;
using namespace svthost;

static_assert(sizeof(svt_hip_inter_blk) == 16 && sizeof(svt_hip_inter_cand) == 16 && sizeof(svt_hip_inter_fast_blk) == 16,
              "inter_pick_kernel reads the records as four words");
static_assert(offsetof(svt_hip_inter_blk, mv) == 4 && offsetof(svt_hip_inter_blk, pred_direction) == 12, "svt_hip_inter_blk layout");
static_assert(offsetof(svt_hip_inter_cand, mode_ctx) == 8 && offsetof(svt_hip_inter_cand, pred_mode) == 10 && offsetof(svt_hip_inter_cand, drl_index) == 12 &&
              offsetof(svt_hip_inter_cand, flags) == 15, "svt_hip_inter_cand layout");
static_assert(offsetof(svt_hip_inter_fast_blk, comp_ref_p) == 4 && offsetof(svt_hip_inter_fast_blk, comp_bwdref_p) == 7 &&
              offsetof(svt_hip_inter_fast_blk, single_ref_p) == 9 && offsetof(svt_hip_inter_fast_blk, has_uv) == 15, "svt_hip_inter_fast_blk layout");
static_assert(sizeof(svt_hip_inter_fast_rates) == IFP_RATE_WORDS * sizeof(int32_t), "inter_pick_kernel stages the tables as words");
static_assert(offsetof(svt_hip_inter_fast_rates, newMvModeFacBits) == IFP_NEWMV * 4 && offsetof(svt_hip_inter_fast_rates, zeroMvModeFacBits) == IFP_ZEROMV * 4 &&
              offsetof(svt_hip_inter_fast_rates, refMvModeFacBits) == IFP_REFMV * 4 && offsetof(svt_hip_inter_fast_rates, drlModeFacBits) == IFP_DRL * 4 &&
              offsetof(svt_hip_inter_fast_rates, interCompoundModeFacBits) == IFP_COMPMODE * 4 && offsetof(svt_hip_inter_fast_rates, singleRefFacBits) == IFP_SINGLE * 4 &&
              offsetof(svt_hip_inter_fast_rates, compRefTypeFacBits) == IFP_CRT * 4 && offsetof(svt_hip_inter_fast_rates, compRefFacBits) == IFP_CREF * 4 &&
              offsetof(svt_hip_inter_fast_rates, compBwdRefFacBits) == IFP_CBWD * 4 && offsetof(svt_hip_inter_fast_rates, compInterFacBits) == IFP_CINTER * 4 &&
              offsetof(svt_hip_inter_fast_rates, motionModeFacBits) == IFP_MM * 4 && offsetof(svt_hip_inter_fast_rates, motionModeFacBits1) == IFP_MM1 * 4 &&
              offsetof(svt_hip_inter_fast_rates, intraInterFacBits) == IFP_II * 4 && offsetof(svt_hip_inter_fast_rates, nmv_vec_cost) == IFP_JOINT * 4,
              "svt_hip_inter_fast_rates layout");
static_assert(SVT_HIP_MV_VALS == IFP_MV_VALS, "svt_hip_dsp.h");
static_assert(sizeof(InterFastPickDev) <= 4000, "kernel arguments");

static int inter_fast_pick_enqueue(const svt_hip_inter_fast_pick_group* groups, int ngroups, int metric, hipStream_t s) {
    for (int g = 0; g < ngroups; g++) {
        const svt_hip_inter_fast_pick_group& G = groups[g];
        if (G.nblocks == 0) continue;
        InterFastPickDev D;
        memset(&D, 0, sizeof(D));
        D.blk = (const uint32_t*)G.d_blk; D.cand_in = (const uint32_t*)G.d_cand_in; D.ctx = (const uint32_t*)G.d_ctx;
        D.rates = (const int32_t*)G.d_rates; D.mv_cost = G.d_mv_cost;
        D.dist = (const unsigned long long*)G.d_dist; D.dist_cb = (const unsigned long long*)G.d_dist_cb; D.dist_cr = (const unsigned long long*)G.d_dist_cr;
        D.intra_cost = (const unsigned long long*)G.d_intra_cost; D.intra_rate = G.d_intra_rate;
        D.cand_out = G.d_cand; D.sorted = G.d_sorted; D.cost = (unsigned long long*)G.d_cost; D.rate = G.d_rate;
        D.ref_fast_cost = (unsigned long long*)G.d_ref_fast_cost; D.all_cost = (unsigned long long*)G.d_all_cost;
        D.blk_out = (uint32_t*)G.d_blk_out; D.cand_rec_out = (uint32_t*)G.d_cand_out; D.src_xy_out = G.d_src_xy_out;
        D.nblocks = G.nblocks; D.lambda = G.lambda; D.qstep = (uint32_t)(G.ac_dequant_q3 >> 3);
        const int ncand = G.ninter + G.nintra, n = fast_n(G.nfl, ncand);
        D.ninter = (uint8_t)G.ninter; D.nintra = (uint8_t)G.nintra; D.n = (uint8_t)n; D.nbuf = (uint8_t)fast_nbuf(n, ncand);
        D.ssd = metric == SVT_HIP_FAST_SSD; D.bsize = (uint8_t)G.bsize;
        D.nlog2_y = kNumPelsLog2[G.bsize]; D.nlog2_uv = kNumPelsLog2[G.bsize_uv];
        D.comp_inter = G.reference_mode_select != 0 && (kBsizeW[G.bsize] < kBsizeH[G.bsize] ? kBsizeW[G.bsize] : kBsizeH[G.bsize]) >= 8;
        D.switchable_motion_mode = G.switchable_motion_mode != 0;
        D.bpw = (uint8_t)pick_bpw(G.nblocks, g_num_cu);
        const uint32_t per_wg = (uint32_t)(FW_WAVES * D.bpw), wgs = (G.nblocks + per_wg - 1) / per_wg;
        hipLaunchKernelGGL(inter_pick_kernel, dim3(wgs), dim3(FW_THREADS), 0, s, D);
        if (int rc = launch_status("inter_fast_pick")) return rc;
    }
    return SVT_HIP_OK;
}

extern "C" int svt_hip_inter_fast_pick_frame(const svt_hip_inter_fast_pick_group* groups, int ngroups, int metric, void* stream) {
    if (int rc = require_init()) return rc;
    if (int rc = inter_fast_pick_check(groups, ngroups, metric)) return rc;
    return inter_fast_pick_enqueue(groups, ngroups, metric, (hipStream_t)stream);
}

// ---- the whole inter fast search -----------------------------------------------------------------------------------------------------
extern "C" size_t svt_hip_inter_fast_search_scratch_bytes(const svt_hip_inter_fast_search_group* groups, int ngroups) {
    return inter_fast_search_scratch_bytes(groups, ngroups);
}

extern "C" int svt_hip_inter_fast_search_frame(const svt_hip_inter_fast_search_group* groups, int ngroups, uint32_t pic_width, uint32_t pic_height,
                                               int bd, int metric, void* d_scratch, size_t scratch_bytes, void* stream) {
    hipStream_t s = (hipStream_t)stream;
    if (int rc = require_init()) return rc;
    InterFastStages st;
    if (int rc = inter_fast_search_plan(groups, ngroups, pic_width, pic_height, bd, metric, d_scratch, scratch_bytes, &st)) return rc;
    // (svt_hip_inter_pred_frame checks its groups once more: they were accepted above, before the first launch)
    if (int rc = svt_hip_inter_pred_frame(st.dist.data(), (int)st.dist.size(), pic_width, pic_height, bd, metric, stream)) return rc;
    if (int rc = inter_fast_pick_enqueue(st.pick.data(), (int)st.pick.size(), metric, s)) return rc;
    if (int rc = svt_hip_inter_pred_frame(st.pred.data(), (int)st.pred.size(), pic_width, pic_height, bd, metric, stream)) return rc;
    for (const InterFastGather& T : st.gather) {
        InterFastGatherDev D{T.d_cand, (const uint4*)T.d_intra_pred, (uint4*)T.d_pred_out, T.n, T.ninter, T.nintra, T.quads};
        hipLaunchKernelGGL(inter_fast_gather_kernel, dim3(T.nblocks * T.n), dim3(64), 0, s, D);
        if (int rc = launch_status("inter_fast_gather")) return rc;
    }
    return SVT_HIP_OK;
}

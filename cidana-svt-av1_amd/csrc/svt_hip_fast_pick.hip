// svt_hip_fast_pick.hip — svt_hip_fast_pick_frame: fast cost, the N best and their order per block, the survivors' predictions gathered
// (fast_pick_kernel, kernel_fast_pick.h), one launch per non-empty group; svt_hip_intra_fast_search_frame, the whole intra fast search
// as host composition: fast loop (luma, Cb, Cr) -> pick on one stream, the arrays the caller does not keep in a scratch.
// What is left here: the pick's kernel arguments and launches (fast_pick_enqueue) and the entry points; the checks, the scratch layout,
// the stages' groups and the pick's counts (fast_n, fast_nbuf, pick_bpw) are md_plan.h's.
#include "host_common.h"
#include "kernel_fast_pick.h"

using namespace svtdev;
using namespace svthost;

static_assert(sizeof(svt_hip_fast_pick_blk) == 8, "fast_pick_kernel loads the record as one word");
static_assert(sizeof(svt_hip_fast_rates) == FP_RATE_WORDS * sizeof(int32_t), "fast_pick_kernel stages the tables as words");
static_assert(offsetof(svt_hip_fast_rates, mbModeFacBits) == FP_MB * 4 && offsetof(svt_hip_fast_rates, intraUVmodeFacBits) == FP_UV * 4 &&
              offsetof(svt_hip_fast_rates, angleDeltaFacBits) == FP_ANG * 4 && offsetof(svt_hip_fast_rates, skipModeFacBits) == FP_SKIP * 4 &&
              offsetof(svt_hip_fast_rates, intraInterFacBits) == FP_II * 4, "svt_hip_fast_rates layout");
static_assert(sizeof(FastPickDev) <= 4000, "kernel arguments");
static_assert(kPickMaxBpw == FW_MAX_BPW, "md_plan.h / kernel_fast_walk.h: both pick kernels take pick_bpw's blocks per wave");

static int fast_pick_enqueue(const svt_hip_fast_pick_group* groups, int ngroups, int metric, hipStream_t s) {
    for (int g = 0; g < ngroups; g++) {
        const svt_hip_fast_pick_group& G = groups[g];
        if (G.nblocks == 0) continue;
        const int w = kTxW[G.tx_size], h = kTxH[G.tx_size];
        FastPickDev D;
        memset(&D, 0, sizeof(D));
        D.dist = (const unsigned long long*)G.d_dist; D.dist_cb = (const unsigned long long*)G.d_dist_cb; D.dist_cr = (const unsigned long long*)G.d_dist_cr;
        D.blk = (const unsigned long long*)G.d_blk; D.rates = (const int32_t*)G.d_rates; D.pred = G.d_pred; D.src_xy = G.d_src_xy;
        D.cand_out = G.d_cand; D.sorted = G.d_sorted; D.cost = (unsigned long long*)G.d_cost; D.rate = G.d_rate;
        D.ref_fast_cost = (unsigned long long*)G.d_ref_fast_cost; D.all_cost = (unsigned long long*)G.d_all_cost;
        D.pred_out = G.d_pred_out; D.src_xy_out = G.d_src_xy_out;
        D.nblocks = G.nblocks; D.lambda = G.lambda; D.intrabc_bits = G.intrabc_bits; D.qstep = (uint32_t)(G.ac_dequant_q3 >> 3);
        for (int c = 0; c < G.ncand; c++) {
            const int um = G.uv_modes[c] == 13 ? 0 : G.uv_modes[c];              // UV_CFL_PRED is costed as UV_DC_PRED
            D.cand[c] = (uint16_t)(G.modes[c] | ((G.angle_deltas[c] + 3) << 4) | (um << 8) | ((G.uv_angle_deltas[c] + 3) << 12));
        }
        const int n = fast_n(G.nfl, G.ncand);
        D.ncand = (uint8_t)G.ncand; D.n = (uint8_t)n; D.nbuf = (uint8_t)fast_nbuf(n, G.ncand);
        D.ssd = metric == SVT_HIP_FAST_SSD; D.slice_is_intra = G.slice_is_intra != 0; D.use_angle_delta = G.use_angle_delta != 0;
        D.cfl_allowed = w <= 32 && h <= 32; D.size_group = kSizeGroup[G.bsize];
        D.nlog2_y = kNumPelsLog2[G.bsize]; D.nlog2_uv = kNumPelsLog2[G.bsize_uv];
        D.ql = (uint8_t)(log2_of(w * h) - 4);
        D.bpw = (uint8_t)pick_bpw(G.nblocks, g_num_cu);
        const uint32_t per_wg = (uint32_t)(FW_WAVES * D.bpw), wgs = (G.nblocks + per_wg - 1) / per_wg;
        hipLaunchKernelGGL(fast_pick_kernel, dim3(wgs), dim3(FW_THREADS), 0, s, D);
        if (int rc = launch_status("fast_pick")) return rc;
    }
    return SVT_HIP_OK;
}

extern "C" int svt_hip_fast_pick_frame(const svt_hip_fast_pick_group* groups, int ngroups, int metric, void* stream) {
    if (int rc = require_init()) return rc;
    if (int rc = fast_pick_check(groups, ngroups, metric)) return rc;
    return fast_pick_enqueue(groups, ngroups, metric, (hipStream_t)stream);
}

// ---- the whole intra fast search: fast loop (luma, Cb, Cr) -> pick ---------------------------------------------------------------
extern "C" size_t svt_hip_intra_fast_search_scratch_bytes(const svt_hip_intra_fast_search_group* groups, int ngroups) {
    return scratch_bytes_of(fast_search_walk, groups, ngroups);
}

extern "C" int svt_hip_intra_fast_search_frame(const svt_hip_intra_fast_search_group* groups, int ngroups, int metric, int flavour,
                                               void* d_scratch, size_t scratch_bytes, void* stream) {
    hipStream_t s = (hipStream_t)stream;
    if (int rc = require_init()) return rc;
    FastSearchStages st;
    if (int rc = plan_stages(fast_search_walk, groups, ngroups, d_scratch, scratch_bytes, &st)) return rc;
    // every stage's arguments before the first launch
    if (int rc = fast_loop_check(st.fl.data(), ngroups, metric, flavour)) return rc;
    if (int rc = fast_loop_check(st.flc.data(), (int)st.flc.size(), metric, flavour)) return rc;
    if (int rc = fast_pick_check(st.fp.data(), ngroups, metric)) return rc;
    if (int rc = fast_loop_enqueue(st.fl.data(), ngroups, metric, flavour, s)) return rc;
    if (int rc = fast_loop_enqueue(st.flc.data(), (int)st.flc.size(), metric, flavour, s)) return rc;
    return fast_pick_enqueue(st.fp.data(), ngroups, metric, s);
}

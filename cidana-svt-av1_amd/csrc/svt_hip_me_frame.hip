// svt_hip_me_frame.hip — svt_hip_motion_estimate_frame: MotionEstimateLcu for every SB of a picture (or of a stack of pictures
// under one parameter set) in three launches (kernel_me_frame.h): prologue (HME levels, best region, CheckZeroZeroCenter, search
// area), full-pel search, bi-prediction + me_results rows.  svt_hip_motion_estimate_subpel_frame: the same with use_subpel_flag = 1 -
// prologue, search, then the two sub-pel launches of svt_hip_me_subpel.hip (refinement, bi-prediction on fractional vectors).
#include "host_common.h"
#include "kernel_me_frame.h"
#include "me_subpel_plan.h"

using namespace svtdev;
using namespace svthost;

static_assert(sizeof(svt_hip_me_frame_params) == 116, "svt_hip_me_frame_params layout");
static_assert(sizeof(svt_hip_me_pyramid) == 88, "svt_hip_me_pyramid layout");

extern "C" size_t svt_hip_motion_estimate_frame_scratch_bytes(const svt_hip_me_frame_params* params, uint32_t n_pictures) {
    MeFramePlan pl;
    if (me_frame_plan(params, pl) != SVT_HIP_OK) return 0;
    return me_frame_scratch(pl, n_pictures ? n_pictures : 1);
}

// Both whole-picture calls: the checks and the plan (me_subpel_plan.h, me_plan.h), then the launches.  subpel: use_subpel_flag = 1 - after
// the search the result rows are refined to quarter-pel and the bi-prediction runs on the fractional vectors (svt_hip_me_subpel.hip);
// sp = its enables (NULL: all on).
static int me_frame_enqueue(const svt_hip_me_pyramid* src, const svt_hip_me_pyramid* ref0, const svt_hip_me_pyramid* ref1, const svt_hip_me_frame_params* params,
                            bool subpel, const svt_hip_me_subpel_params* sp, uint32_t n_pictures, uint32_t* d_best_sad, uint32_t* d_best_mv,
                            int16_t* d_area_origin, uint32_t* d_bipred_sad, svt_hip_me_result* d_results, void* d_scratch, size_t scratch_bytes, void* stream) {
    if (int rc = require_init()) return rc;
    MeFramePlan pl;
    if (int rc = me_frame_check(src, ref0, ref1, params, subpel, sp, n_pictures, d_best_sad, d_best_mv, d_area_origin, d_bipred_sad, d_results, d_scratch,
                                scratch_bytes, pl))
        return rc;
    if (n_pictures == 0) return SVT_HIP_OK;
    const svt_hip_me_frame_params& P = *params;

    MeFrameDev d;
    memset(&d, 0, sizeof(d));
    const svt_hip_me_pyramid* refs[2] = {ref0, ref1};
    for (int k = 0; k < 3; k++) {
        if (k > 0 && !pl.level_on[2 - k]) continue;
        const MePlaneAt at = me_plane_at(src, k, n_pictures);
        d.src[k] = at.p; d.src_stride[k] = at.stride; d.src_pitch[k] = at.pitch;
        for (int l = 0; l < pl.nl; l++) {
            const MePlaneAt rt = me_plane_at(refs[l], k, n_pictures);
            d.ref[l][k] = rt.p; d.ref_stride[l][k] = rt.stride; d.ref_pitch[l][k] = rt.pitch;
        }
    }
    static_assert(sizeof(d.hme) == sizeof(pl.hme) && sizeof(HmeParams) == sizeof(svt_hip_hme_params), "layout");
    memcpy(d.hme, pl.hme, sizeof(d.hme));
    d.setup.picture_width = P.picture_width; d.setup.picture_height = P.picture_height;
    d.setup.ref_width = P.picture_width; d.setup.ref_height = P.picture_height;
    d.setup.search_area_width = P.search_area_width; d.setup.search_area_height = P.search_area_height;
    d.setup.regions_w = P.number_hme_search_region_in_width; d.setup.regions_h = P.number_hme_search_region_in_height;
    d.setup.second_best = 0;
    d.setup.zz_check = pl.zz_check;
    for (int l = 0; l < 2; l++) { d.hme_list[l] = pl.hme_list[l]; d.second_best[l] = pl.second_best[l]; }
    for (int lv = 0; lv < 3; lv++) d.level_on[lv] = pl.level_on[lv];
    d.nreg = pl.nreg; d.last_level = pl.last_level;
    d.nlists = pl.nl; d.npus = P.max_number_of_pus_per_sb;
    d.nsbx = pl.nsbx; d.nsb = pl.nsb;
    d.hme_wpitch = pl.hme_wpitch;
    d.area = (int16_t*)d_scratch;
    d.area_origin = d_area_origin;
    d.best_sad = d_best_sad; d.best_mv = d_best_mv;

    const hipStream_t s = (hipStream_t)stream;
    const dim3 grid(pl.nsb, (uint32_t)pl.nl, n_pictures);
    hipLaunchKernelGGL(me_frame_prologue_kernel, grid, dim3(ME_THREADS), pl.hme_win.lds, s, d);
    if (int rc = launch_status("me_frame_prologue")) return rc;
    auto* search = pl.nsq ? me_frame_search_kernel<true> : me_frame_search_kernel<false>;
    hipLaunchKernelGGL(search, grid, dim3(ME_THREADS), pl.search.lds, s, d, pl.max_w, pl.max_h, P.flavour, pl.search.wpitch, pl.search.pair_off);
    if (int rc = launch_status("me_frame_search")) return rc;
    if (subpel) {
        if (int rc = me_subpel_enqueue_refine(src, ref0, ref1, params, sp, n_pictures, d_best_sad, d_best_mv, nullptr, nullptr, s)) return rc;
        return me_subpel_enqueue_bipred(src, ref0, ref1, params, n_pictures, d_best_sad, d_best_mv, d_bipred_sad, d_results, s);
    }
    static_assert(sizeof(MeResult) == sizeof(svt_hip_me_result), "layout");
    hipLaunchKernelGGL(me_frame_bipred_kernel, dim3(pl.nsb, 1, n_pictures), dim3(ME_THREADS), 0, s, d, pl.bipred_all, pl.sub_sad, me_pu_map(), d_bipred_sad,
                       reinterpret_cast<MeResult*>(d_results));
    return launch_status("me_frame_bipred");
}

extern "C" int svt_hip_motion_estimate_frame(const svt_hip_me_pyramid* src, const svt_hip_me_pyramid* ref0, const svt_hip_me_pyramid* ref1,
                                             const svt_hip_me_frame_params* params, uint32_t n_pictures, uint32_t* d_best_sad, uint32_t* d_best_mv,
                                             int16_t* d_area_origin, uint32_t* d_bipred_sad, svt_hip_me_result* d_results, void* d_scratch,
                                             size_t scratch_bytes, void* stream) {
    return me_frame_enqueue(src, ref0, ref1, params, false, nullptr, n_pictures, d_best_sad, d_best_mv, d_area_origin, d_bipred_sad, d_results, d_scratch,
                            scratch_bytes, stream);
}

extern "C" size_t svt_hip_motion_estimate_subpel_frame_scratch_bytes(const svt_hip_me_frame_params* params, uint32_t n_pictures) {
    if (me_subpel_frame_check(params) != SVT_HIP_OK) return 0;
    return svt_hip_motion_estimate_frame_scratch_bytes(params, n_pictures);
}

extern "C" int svt_hip_motion_estimate_subpel_frame(const svt_hip_me_pyramid* src, const svt_hip_me_pyramid* ref0, const svt_hip_me_pyramid* ref1,
                                                    const svt_hip_me_frame_params* params, const svt_hip_me_subpel_params* subpel, uint32_t n_pictures,
                                                    uint32_t* d_best_sad, uint32_t* d_best_mv, int16_t* d_area_origin, uint32_t* d_bipred_sad,
                                                    svt_hip_me_result* d_results, void* d_scratch, size_t scratch_bytes, void* stream) {
    return me_frame_enqueue(src, ref0, ref1, params, true, subpel, n_pictures, d_best_sad, d_best_mv, d_area_origin, d_bipred_sad, d_results, d_scratch,
                            scratch_bytes, stream);
}

// svt_hip_me_subpel.hip — sub-pel motion estimation (kernel_me_subpel.h): svt_hip_me_subpel_frame, the refinement stage alone; the two
// launches that svt_hip_motion_estimate_subpel_frame (svt_hip_me_frame.hip) puts behind the full-pel search; svt_hip_me_subpel_planes, the
// interpolation by itself; svt_hip_me_subpel_check, the stage's checks without a device (me_subpel_plan.h).
#include "host_common.h"
#include "kernel_me_subpel.h"

using namespace svtdev;
using namespace svthost;

static_assert(sizeof(svt_hip_me_subpel_params) == 20, "svt_hip_me_subpel_params layout");

static MeSubpelDev me_subpel_dev(const svt_hip_me_pyramid* src, const svt_hip_me_pyramid* ref0, const svt_hip_me_pyramid* ref1, const svt_hip_me_frame_params& P,
                                 const svt_hip_me_subpel_params* sp, uint32_t n_pictures) {
    MeSubpelDev d;
    memset(&d, 0, sizeof(d));
    d.nlists = P.slice_type == SVT_HIP_SLICE_P ? 1 : 2;
    const svt_hip_me_pyramid* refs[2] = {ref0, d.nlists == 2 ? ref1 : nullptr};
    d.src = src->d_plane[0] + (size_t)src->origin_y[0] * src->stride[0] + src->origin_x[0];
    d.src_stride = src->stride[0];
    d.src_pitch = n_pictures > 1 ? src->pitch[0] : 0;
    for (int l = 0; l < d.nlists; l++) {
        d.ref[l] = refs[l]->d_plane[0] + (size_t)refs[l]->origin_y[0] * refs[l]->stride[0] + refs[l]->origin_x[0];
        d.ref_stride[l] = refs[l]->stride[0];
        d.ref_pitch[l] = n_pictures > 1 ? refs[l]->pitch[0] : 0;
    }
    d.width = P.picture_width; d.height = P.picture_height;
    d.npus = P.max_number_of_pus_per_sb;
    d.method = P.fractional_search_method;
    d.f64 = sp ? sp->fractional_search64x64 : 1;
    d.h32 = sp ? sp->enable_half_pel32x32 : 1; d.h16 = sp ? sp->enable_half_pel16x16 : 1; d.h8 = sp ? sp->enable_half_pel8x8 : 1;
    d.qp = sp ? sp->enable_quarter_pel : 1;
    d.no8 = P.cu8x8_mode == 1 ? 1 : 0;                   // disable8x8CuInMeFlag = cu8x8_mode == CU_8x8_MODE_1 (:8205)
    d.nsbx = (uint32_t)(P.picture_width + 63) / 64;
    d.nsb = d.nsbx * ((uint32_t)(P.picture_height + 63) / 64);
    return d;
}

int svthost::me_subpel_enqueue_refine(const svt_hip_me_pyramid* src, const svt_hip_me_pyramid* ref0, const svt_hip_me_pyramid* ref1,
                                      const svt_hip_me_frame_params* params, const svt_hip_me_subpel_params* sp, uint32_t n_pictures, uint32_t* d_best_sad,
                                      uint32_t* d_best_mv, uint32_t* d_best_ssd, uint8_t* d_half_dir, hipStream_t s) {
    const MeSubpelDev d = me_subpel_dev(src, ref0, ref1, *params, sp, n_pictures);
    hipLaunchKernelGGL(me_subpel_refine_kernel, dim3(d.nsb, (uint32_t)d.nlists, n_pictures), dim3(ME_SP_THREADS), 0, s, d, d_best_sad, d_best_mv, d_best_ssd,
                       d_half_dir);
    return launch_status("me_subpel_refine");
}

int svthost::me_subpel_enqueue_bipred(const svt_hip_me_pyramid* src, const svt_hip_me_pyramid* ref0, const svt_hip_me_pyramid* ref1,
                                      const svt_hip_me_frame_params* params, uint32_t n_pictures, const uint32_t* d_best_sad, const uint32_t* d_best_mv,
                                      uint32_t* d_bipred_sad, svt_hip_me_result* d_results, hipStream_t s) {
    const svt_hip_me_frame_params& P = *params;
    const MeSubpelDev d = me_subpel_dev(src, ref0, ref1, P, nullptr, n_pictures);
    static_assert(sizeof(MeResult) == sizeof(svt_hip_me_result), "layout");
    const int bipred_all = (P.cu8x8_mode == 0 || P.max_number_of_pus_per_sb == SVT_HIP_ME_PUS_ALL) ? 1 : 0;
    hipLaunchKernelGGL(me_subpel_bipred_kernel, dim3(d.nsb, 1, n_pictures), dim3(ME_SP_THREADS), 0, s, d, bipred_all, P.fractional_search_method == 0 ? 1 : 0,
                       me_pu_map(), d_best_sad, d_best_mv, d_bipred_sad, reinterpret_cast<MeResult*>(d_results));
    return launch_status("me_subpel_bipred");
}

extern "C" int svt_hip_me_subpel_check(const svt_hip_me_pyramid* src, const svt_hip_me_pyramid* ref0, const svt_hip_me_pyramid* ref1,
                                       const svt_hip_me_frame_params* params, const svt_hip_me_subpel_params* subpel, uint32_t n_pictures,
                                       const uint32_t* d_best_sad, const uint32_t* d_best_mv, const uint32_t* d_best_ssd, const uint8_t* d_half_dir) {
    return me_subpel_check(src, ref0, ref1, params, subpel, n_pictures, d_best_sad, d_best_mv, d_best_ssd, d_half_dir);
}

extern "C" int svt_hip_me_subpel_frame(const svt_hip_me_pyramid* src, const svt_hip_me_pyramid* ref0, const svt_hip_me_pyramid* ref1,
                                       const svt_hip_me_frame_params* params, const svt_hip_me_subpel_params* subpel, uint32_t n_pictures,
                                       uint32_t* d_best_sad, uint32_t* d_best_mv, uint32_t* d_best_ssd, uint8_t* d_half_dir, void* stream) {
    if (int rc = require_init()) return rc;
    if (int rc = me_subpel_check(src, ref0, ref1, params, subpel, n_pictures, d_best_sad, d_best_mv, d_best_ssd, d_half_dir)) return rc;
    if (n_pictures == 0) return SVT_HIP_OK;
    return me_subpel_enqueue_refine(src, ref0, ref1, params, subpel, n_pictures, d_best_sad, d_best_mv, d_best_ssd, d_half_dir, (hipStream_t)stream);
}

extern "C" int svt_hip_me_subpel_planes(const svt_hip_me_pyramid* ref, int32_t picture_width, int32_t picture_height, int32_t x0, int32_t y0, uint32_t w,
                                        uint32_t h, uint8_t* d_planes, void* stream) {
    if (int rc = require_init()) return rc;
    if (int rc = me_subpel_planes_check(ref, picture_width, picture_height, x0, y0, w, h, d_planes)) return rc;
    const uint8_t* p = ref->d_plane[0] + (size_t)ref->origin_y[0] * ref->stride[0] + ref->origin_x[0];
    hipLaunchKernelGGL(me_subpel_planes_kernel, dim3((w * h + 255) / 256), dim3(256), 0, (hipStream_t)stream, p, ref->stride[0], x0, y0, w, h, d_planes);
    return launch_status("me_subpel_planes");
}

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
    const MeGeom g = me_geom(P);
    const MeSubpelScalars sc = me_subpel_scalars(P, sp);
    const svt_hip_me_pyramid* refs[2] = {ref0, ref1};
    const MePlaneAt at = me_plane_at(src, 0, n_pictures);
    d.src = at.p; d.src_stride = at.stride; d.src_pitch = at.pitch;
    for (int l = 0; l < g.nl; l++) {
        const MePlaneAt rt = me_plane_at(refs[l], 0, n_pictures);
        d.ref[l] = rt.p; d.ref_stride[l] = rt.stride; d.ref_pitch[l] = rt.pitch;
    }
    d.width = P.picture_width; d.height = P.picture_height;
    d.nlists = g.nl; d.npus = P.max_number_of_pus_per_sb;
    d.method = P.fractional_search_method;
    d.f64 = sc.f64; d.h32 = sc.h32; d.h16 = sc.h16; d.h8 = sc.h8; d.qp = sc.qp; d.no8 = sc.no8;
    d.nsbx = g.nsbx; d.nsb = g.nsb;
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
    const MeBipredSwitches b = me_bipred_switches(P);
    hipLaunchKernelGGL(me_subpel_bipred_kernel, dim3(d.nsb, 1, n_pictures), dim3(ME_SP_THREADS), 0, s, d, b.all_pus, b.sub_sad, me_pu_map(), d_best_sad, d_best_mv,
                       d_bipred_sad, reinterpret_cast<MeResult*>(d_results));
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
    const MePlaneAt at = me_plane_at(ref, 0, 1);
    hipLaunchKernelGGL(me_subpel_planes_kernel, dim3(me_subpel_planes_grid(w, h)), dim3(256), 0, (hipStream_t)stream, at.p, at.stride, x0, y0, w, h, d_planes);
    return launch_status("me_subpel_planes");
}

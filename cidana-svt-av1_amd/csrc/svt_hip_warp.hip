// svt_hip_warp.hip — svt_hip_warp_fit_frame and svt_hip_warp_pred_frame: the local warp model of every (block, candidate) and the warped
// prediction with the distortion fused in (kernel_warp.h).  The checks and the tiling are warp_plan.h's; what is left here is the
// launches, one per WP_MAX_GROUPS non-empty groups: both kernels take the block size at run time.
#include "host_common.h"
#include "kernel_warp.h"

using namespace svtdev;
using namespace svthost;

static_assert(SVT_HIP_INTER_PRED_MAX_GROUPS == WP_MAX_GROUPS, "svt_hip_dsp.h");
static_assert(sizeof(svt_hip_inter_blk) == 16 && alignof(svt_hip_inter_blk) == 2, "the kernels read x | y << 16 and mv[0] as two words");

extern "C" int svt_hip_warp_fit_frame(const svt_hip_warp_fit_group* groups, int ngroups, void* stream) {
    if (int rc = require_init()) return rc;
    if (int rc = warp_fit_check(groups, ngroups)) return rc;
    const hipStream_t s = (hipStream_t)stream;
    return warp_fit_enqueue(groups, ngroups, [&](const WarpFitDesc& fd, uint32_t total) -> int {
        hipLaunchKernelGGL(warp_fit_kernel, dim3(total), dim3(WP_THREADS), 0, s, fd);
        return launch_status("warp_fit");
    });
}

extern "C" int svt_hip_warp_pred_frame(const svt_hip_warp_pred_group* groups, int ngroups, uint32_t pic_width, uint32_t pic_height, int bd, int metric,
                                       void* stream) {
    if (int rc = require_init()) return rc;
    if (int rc = warp_pred_check(groups, ngroups, pic_width, pic_height, bd, metric)) return rc;
    const hipStream_t s = (hipStream_t)stream;
    return warp_pred_enqueue(groups, ngroups, pic_width, pic_height, bd, metric, [&](const WarpPredDesc& fd, uint32_t total) -> int {
        if (bd == 8) hipLaunchKernelGGL(warp_pred_kernel<uint8_t>, dim3(total), dim3(WP_THREADS), 0, s, fd);
        else hipLaunchKernelGGL(warp_pred_kernel<uint16_t>, dim3(total), dim3(WP_THREADS), 0, s, fd);
        return launch_status("warp_pred");
    });
}

extern "C" void svt_hip_warp_tables(int16_t* filter, uint16_t* div_lut) {
    if (filter)
        for (int r = 0; r < svtwarp::kWarpRows; r++)
            for (int k = 0; k < 8; k++) filter[r * 8 + k] = svtwarp::kWarpFilter.t[r][k];
    if (div_lut)
        for (int i = 0; i <= 256; i++) div_lut[i] = svtwarp::kDivLut.v[i];
}

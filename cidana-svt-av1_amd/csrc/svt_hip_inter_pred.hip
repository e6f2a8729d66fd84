// svt_hip_inter_pred.hip — svt_hip_inter_pred_frame: AV1 translational inter prediction with the distortion fused in
// (kernel_inter_pred.h).  The checks and the tiling are inter_plan.h's; what is left here is the launch itself, one
// per IP_MAX_GROUPS non-empty groups: the kernel takes the block size at run time, so every group of a call shares one register class.
#include "host_common.h"
#include "kernel_inter_pred.h"

using namespace svtdev;
using namespace svthost;

static_assert(sizeof(svt_hip_inter_blk) == 16 && alignof(svt_hip_inter_blk) == 2, "inter_pred_kernel reads the record as four words");
static_assert(sizeof(svt_hip_inter_pred_group) == 88, "svt_hip_inter_pred_group layout");
static_assert(SVT_HIP_INTER_PRED_MAX_GROUPS == IP_MAX_GROUPS, "svt_hip_dsp.h");
static_assert(SVT_HIP_UNI_PRED_LIST_0 == 0 && SVT_HIP_UNI_PRED_LIST_1 == 1 && SVT_HIP_BI_PRED == 2, "inter_pred_kernel's pred_direction");

extern "C" int svt_hip_inter_pred_frame(const svt_hip_inter_pred_group* groups, int ngroups, uint32_t pic_width, uint32_t pic_height, int bd,
                                        int metric, void* stream) {
    if (int rc = require_init()) return rc;
    if (int rc = inter_pred_check(groups, ngroups, pic_width, pic_height, bd, metric)) return rc;
    const hipStream_t s = (hipStream_t)stream;
    return inter_pred_enqueue(groups, ngroups, pic_width, pic_height, bd, metric, [&](const InterPredDesc& fd, uint32_t total) -> int {
        if (bd == 8) hipLaunchKernelGGL(inter_pred_kernel<uint8_t>, dim3(total), dim3(IP_THREADS), 0, s, fd);
        else hipLaunchKernelGGL(inter_pred_kernel<uint16_t>, dim3(total), dim3(IP_THREADS), 0, s, fd);
        return launch_status("inter_pred");
    });
}

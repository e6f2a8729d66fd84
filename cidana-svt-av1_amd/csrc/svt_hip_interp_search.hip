// svt_hip_interp_search.hip — the interpolation filter search of mode decision (kernel_interp_search.h): svt_hip_interp_sse_frame, the
// table of nine SSEs per block and plane; svt_hip_interp_decide_frame, the reference's walk over it; svt_hip_interp_search_frame, both on
// one stream as host composition with the table in the caller's scratch.  The checks, the scratch layout and the launch lists are
// interp_plan.h's; what is left here is the launches themselves.
#include "host_common.h"
#include "kernel_interp_search.h"

using namespace svtdev;
using namespace svthost;

static_assert(sizeof(svt_hip_interp_decision) == 32 && alignof(svt_hip_interp_decision) == 8, "interp_decide_kernel stores the record as four words");
static_assert(offsetof(svt_hip_interp_decision, switchable_rate) == 4 && offsetof(svt_hip_interp_decision, rd) == 8 &&
              offsetof(svt_hip_interp_decision, skip_sse_sb) == 16 && offsetof(svt_hip_interp_decision, skip_txfm_sb) == 24, "svt_hip_interp_decision layout");
static_assert(sizeof(svt_hip_inter_blk) == 16 && offsetof(svt_hip_inter_blk, filter_x) == 13 && offsetof(svt_hip_inter_blk, filter_y) == 14,
              "interp_decide_kernel fills the filter bytes of the record's fourth word");

static int sse_enqueue(const svt_hip_interp_sse_group* groups, int ngroups, uint32_t pic_width, uint32_t pic_height, int use_uv, hipStream_t s) {
    return interp_sse_enqueue(groups, ngroups, pic_width, pic_height, use_uv, [&](const InterpSseDesc& fd, uint32_t total) -> int {
        hipLaunchKernelGGL(interp_sse_kernel, dim3(total), dim3(IP_THREADS), 0, s, fd);
        return launch_status("interp_sse");
    });
}

static int decide_enqueue(const svt_hip_interp_decide_group* groups, int ngroups, const svt_hip_interp_params& prm, hipStream_t s) {
    return interp_decide_enqueue(groups, ngroups, prm, [&](const InterpDecideDesc& fd, uint32_t total) -> int {
        hipLaunchKernelGGL(interp_decide_kernel, dim3(total), dim3(ID_THREADS), 0, s, fd);
        return launch_status("interp_decide");
    });
}

extern "C" int svt_hip_interp_sse_frame(const svt_hip_interp_sse_group* groups, int ngroups, uint32_t pic_width, uint32_t pic_height, int bd,
                                        int use_uv, void* stream) {
    if (int rc = require_init()) return rc;
    if (int rc = interp_sse_check(groups, ngroups, pic_width, pic_height, bd, use_uv)) return rc;
    return sse_enqueue(groups, ngroups, pic_width, pic_height, use_uv, (hipStream_t)stream);
}

extern "C" int svt_hip_interp_decide_frame(const svt_hip_interp_decide_group* groups, int ngroups, const svt_hip_interp_params* params, void* stream) {
    if (int rc = require_init()) return rc;
    if (int rc = interp_decide_check(groups, ngroups, params)) return rc;
    return decide_enqueue(groups, ngroups, *params, (hipStream_t)stream);
}

extern "C" size_t svt_hip_interp_search_scratch_bytes(const svt_hip_interp_search_group* groups, int ngroups, int use_uv) {
    return interp_search_scratch_bytes(groups, ngroups, use_uv);
}

extern "C" int svt_hip_interp_search_frame(const svt_hip_interp_search_group* groups, int ngroups, uint32_t pic_width, uint32_t pic_height, int bd,
                                           const svt_hip_interp_params* params, void* d_scratch, size_t scratch_bytes, void* stream) {
    if (int rc = require_init()) return rc;
    // the tables carved, then both stages' arguments before the first launch
    InterpStages st;
    if (int rc = interp_search_plan(groups, ngroups, params, d_scratch, scratch_bytes, &st)) return rc;
    if (int rc = interp_sse_check(st.sg.data(), ngroups, pic_width, pic_height, bd, params->use_uv, true))   // only an empty group is left without a table
        return rc;
    if (int rc = interp_decide_check(st.dg.data(), ngroups, params, true)) return rc;
    if (int rc = sse_enqueue(st.sg.data(), ngroups, pic_width, pic_height, params->use_uv, (hipStream_t)stream)) return rc;
    return decide_enqueue(st.dg.data(), ngroups, *params, (hipStream_t)stream);
}

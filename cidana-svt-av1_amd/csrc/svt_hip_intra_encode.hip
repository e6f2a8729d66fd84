// svt_hip_intra_encode.hip — svt_hip_intra_encode_frame: the intra encode pass in coding order (ie_prepass_kernel, ie_walk_kernel<0 .. 3>,
// ie_finish_kernel, kernel_intra_encode.h).  The checks, the scratch layout, the steps and the schedule of launches inside a step are
// intra_encode_plan.h's.  A translation unit of its own: the walkers inline every encode body once more, and next to the other
// instantiations of those bodies the compiler's inlining budget changes (svt_hip_frame.hip).
#include <stddef.h>

#include "host_common.h"
#include "kernel_intra_encode.h"

using namespace svtdev;
using namespace svthost;

static_assert(sizeof(svt_hip_intra_enc_blk) == 8 && offsetof(svt_hip_intra_enc_blk, mode) == 1 && offsetof(svt_hip_intra_enc_blk, angle_delta) == 2 &&
              offsetof(svt_hip_intra_enc_blk, uv_mode) == 3 && offsetof(svt_hip_intra_enc_blk, cfl_alpha_idx) == 4 && offsetof(svt_hip_intra_enc_blk, cfl_alpha_signs) == 5 &&
              offsetof(svt_hip_intra_enc_blk, tx_type) == 6 && offsetof(svt_hip_intra_enc_blk, tx_type_uv) == 7, "svt_hip_intra_enc_blk as two words");
static_assert(sizeof(svt_hip_intra_enc_result) == 8 && offsetof(svt_hip_intra_enc_result, tx_type) == 6, "svt_hip_intra_enc_result as two words");

extern "C" size_t svt_hip_intra_encode_scratch_bytes(uint32_t npics, uint32_t nsb) { return intra_encode_scratch_bytes(npics, nsb); }
extern "C" size_t svt_hip_intra_encode_tables_bytes(void) { return IE_TABLE_BYTES; }
extern "C" int svt_hip_intra_encode_launches(uint32_t sb_cols, uint32_t sb_rows, int planes) { return intra_encode_launches(sb_cols, sb_rows, planes); }

extern "C" int svt_hip_intra_encode_tables_fill(void* host) {
    if (!host) return set_err(SVT_HIP_ERR_INVALID, "NULL table");
    int16_t* out = (int16_t*)host;
    int16_t scan[1024], iscan[1024];
    for (int t = 0; t < SVT_TX_SIZES_ALL; t++)
        for (int ty = 0; ty < 16; ty++) {
            int16_t* o = out + ie_iscan_first(t) + (size_t)ty * ie_ncoeff(t);
            if (tx_type_ok(t, ty)) {
                if (svt_hip_get_scan(t, ty, scan, iscan) < 0) return set_err(SVT_HIP_ERR_INVALID, "no scan for size %d type %d", t, ty);
                memcpy(o, iscan, ie_ncoeff(t) * sizeof(int16_t));
            } else {
                memset(o, 0, ie_ncoeff(t) * sizeof(int16_t));
            }
        }
    return SVT_HIP_OK;
}

template <int KIND>
static void launch_walk(const IeDesc& D, uint32_t step, uint32_t r_first, uint32_t rows, uint32_t plane_first, uint32_t nplanes, hipStream_t s) {
    hipLaunchKernelGGL(ie_walk_kernel<KIND>, dim3(rows, D.npics, nplanes), dim3(IE_THREADS), 0, s, D, step, r_first, plane_first);
}
static void launch_kind(int kind, const IeDesc& D, uint32_t step, uint32_t r_first, uint32_t rows, uint32_t plane_first, uint32_t nplanes, hipStream_t s) {
    switch (kind) {
    case 0: launch_walk<0>(D, step, r_first, rows, plane_first, nplanes, s); break;
    case 1: launch_walk<1>(D, step, r_first, rows, plane_first, nplanes, s); break;
    case 2: launch_walk<2>(D, step, r_first, rows, plane_first, nplanes, s); break;
    default: launch_walk<3>(D, step, r_first, rows, plane_first, nplanes, s); break;
    }
}

extern "C" int svt_hip_intra_encode_frame(const svt_hip_intra_encode_args* a, void* stream) {
    if (int rc = require_init()) return rc;
    if (int rc = intra_encode_check(a)) return rc;
    hipStream_t s = (hipStream_t)stream;
    const int planes = intra_encode_planes(a);
    IeDesc D{};
    D.final_blk = (const uint32_t*)a->d_final; D.final_count = a->d_final_count; D.blk = (const uint2*)a->d_blk;
    D.status = a->d_status; D.coeff_offset = a->d_coeff_offset; D.result = (uint2*)a->d_result; D.scratch = (char*)a->d_scratch; D.iscan = a->d_tables;
    D.npics = a->npics; D.sb_cols = a->sb_cols; D.sb_rows = a->sb_rows; D.nsb = a->sb_cols * a->sb_rows; D.sb_pitch = intra_encode_sb_pitch(a);
    D.nsrc = a->nsrc; D.blk_pitch = a->blk_pitch; D.planes = (uint32_t)planes;
    for (int p = 0; p < planes; p++) {
        D.src[p] = a->d_src[p]; D.recon[p] = a->d_recon[p]; D.sbq[p] = a->d_sb_qcoeff[p];
        D.src_pitch[p] = a->src_pic_pitch[p]; D.recon_pitch[p] = a->recon_pic_pitch[p];
        D.src_stride[p] = a->src_stride[p]; D.stride[p] = a->stride[p]; D.width[p] = a->width[p]; D.height[p] = a->height[p];
    }
    for (int ls = 0; ls < 3; ls++) {
        D.qp[0][ls] = make_qparams(*a->q_luma, ls);
        D.qp[1][ls] = make_qparams(planes == 3 ? *a->q_chroma : *a->q_luma, ls);
    }
    const uint32_t units = a->npics * D.nsb;
    hipLaunchKernelGGL(ie_prepass_kernel, dim3((units + 3) / 4), dim3(256), 0, s, D);
    if (int rc = launch_status("intra_encode pre-pass")) return rc;
    const uint32_t steps = intra_encode_steps(a->sb_cols, a->sb_rows);
    for (uint32_t step = 0; step < steps; step++) {
        uint32_t r_first = 0;
        const uint32_t rows = intra_encode_step_rows(a->sb_cols, a->sb_rows, step, &r_first);
        if (rows == 0) continue;                                                // (a grid of one column: the odd steps are empty)
        for (int i = 0; i < IE_LUMA_LAUNCHES; i++) launch_kind(kIeLumaSchedule[i], D, step, r_first, rows, 0, 1, s);
        if (planes == 3)
            for (int i = 0; i < IE_CHROMA_LAUNCHES; i++) launch_kind(kIeChromaSchedule[i], D, step, r_first, rows, 1, 2, s);
        if (int rc = launch_status("intra_encode step")) return rc;
    }
    hipLaunchKernelGGL(ie_finish_kernel, dim3((units + 3) / 4), dim3(256), 0, s, D);
    return launch_status("intra_encode");
}

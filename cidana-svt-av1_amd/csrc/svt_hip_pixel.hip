// svt_hip_pixel.hip — entry points of the pixel / search family of libsvt_hip_dsp.so (include/svt_hip_dsp.h): SAD, SSE,
// residual, SAD search, ME multi-size search, coefficient-domain distortion and their drop-ins.
#include "host_common.h"
#include "kernel_me.h"
#include "kernel_pixel.h"
#include "me_plan.h"
#include "pixel_plan.h"

using namespace svtdev;
using namespace svthost;

// mode 0 SAD, 1 SSE, 2 averaging SAD (kernel_pixel.h); a_shift = 2: four references per source block (x4d); needs_offs: pixel_plan.h
static int sad_sse_common(int mode, int needs_offs, const uint8_t* a, uint32_t as, size_t ap, const uint32_t* a_offs, int a_shift,
                          const uint8_t* b, uint32_t bs, size_t bp, const uint32_t* b_offs, const uint8_t* c, uint32_t cst,
                          size_t cp, uint32_t w, uint32_t h, void* out, size_t n, void* stream) {
    if (int rc = require_init()) return rc;
    if (n == 0) return SVT_HIP_OK;
    SadSsePlan p;
    if (int rc = sad_sse_plan(p, mode, needs_offs, a_shift, a, a_offs, b, b_offs, c, out, w, h, n)) return rc;
#define SADL(M) hipLaunchKernelGGL((sad_sse_kernel<M>), dim3(p.grid), dim3(256), 0, (hipStream_t)stream, a, as, ap, a_offs, a_shift, b, bs, bp, \
                                   b_offs, c, cst, cp, w, h, out, p.n)
    switch (p.mode) {
    case SAD_MODE_SSE: SADL(1); break;
    case SAD_MODE_AVG: SADL(2); break;
    default: SADL(0); break;
    }
#undef SADL
    return launch_status(p.name);
}
extern "C" int svt_hip_sad_batch(const uint8_t* d_src, uint32_t src_stride, size_t src_block_pitch,
                                 const uint8_t* d_ref, uint32_t ref_stride, size_t ref_block_pitch, uint32_t width,
                                 uint32_t height, uint32_t* d_out, size_t nblocks, void* stream) {
    return sad_sse_common(0, 0, d_src, src_stride, src_block_pitch, nullptr, 0, d_ref, ref_stride, ref_block_pitch, nullptr, nullptr, 0, 0,
                          width, height, d_out, nblocks, stream);
}
extern "C" int svt_hip_sse_batch(const uint8_t* d_a, uint32_t a_stride, size_t a_block_pitch, const uint8_t* d_b,
                                 uint32_t b_stride, size_t b_block_pitch, uint32_t width, uint32_t height,
                                 uint64_t* d_out, size_t nblocks, void* stream) {
    return sad_sse_common(1, 0, d_a, a_stride, a_block_pitch, nullptr, 0, d_b, b_stride, b_block_pitch, nullptr, nullptr, 0, 0, width, height,
                          d_out, nblocks, stream);
}
extern "C" int svt_hip_sad_planes_batch(const uint8_t* d_src_plane, uint32_t src_stride, const uint32_t* d_src_offsets,
                                        const uint8_t* d_ref_plane, uint32_t ref_stride, const uint32_t* d_ref_offsets,
                                        uint32_t width, uint32_t height, uint32_t* d_out, size_t nblocks, void* stream) {
    return sad_sse_common(0, SAD_NEEDS_A_OFFS | SAD_NEEDS_B_OFFS, d_src_plane, src_stride, 0, d_src_offsets, 0, d_ref_plane, ref_stride, 0, d_ref_offsets, nullptr, 0, 0, width,
                          height, d_out, nblocks, stream);
}
extern "C" int svt_hip_sad_x4d_batch(const uint8_t* d_src, uint32_t src_stride, size_t src_block_pitch,
                                     const uint32_t* d_src_offsets, const uint8_t* d_ref_plane, uint32_t ref_stride,
                                     const uint32_t* d_ref_offsets, uint32_t width, uint32_t height, uint32_t* d_out,
                                     size_t nblocks, void* stream) {
    return sad_sse_common(0, SAD_NEEDS_B_OFFS, d_src, src_stride, src_block_pitch, d_src_offsets, 2, d_ref_plane, ref_stride, 0, d_ref_offsets, nullptr, 0, 0,
                          width, height, d_out, nblocks, stream);
}
extern "C" int svt_hip_sad_avg_batch(const uint8_t* d_src, uint32_t src_stride, size_t src_block_pitch, const uint8_t* d_ref1,
                                     uint32_t ref1_stride, size_t ref1_block_pitch, const uint8_t* d_ref2,
                                     uint32_t ref2_stride, size_t ref2_block_pitch, uint32_t width, uint32_t height,
                                     uint32_t* d_out, size_t nblocks, void* stream) {
    return sad_sse_common(2, 0, d_src, src_stride, src_block_pitch, nullptr, 0, d_ref1, ref1_stride, ref1_block_pitch, nullptr, d_ref2,
                          ref2_stride, ref2_block_pitch, width, height, d_out, nblocks, stream);
}
template <typename PixT>
static int residual_impl(const PixT* d_src, uint32_t src_stride, size_t src_block_pitch, const PixT* d_pred, uint32_t pred_stride,
                         size_t pred_block_pitch, int16_t* d_res, uint32_t res_stride, size_t res_block_pitch, uint32_t width,
                         uint32_t height, size_t nblocks, void* stream) {
    if (int rc = require_init()) return rc;
    if (nblocks == 0) return SVT_HIP_OK;
    ResidualPlan p;
    if (int rc = residual_plan(p, sizeof(PixT), d_src, d_pred, d_res, width, height, nblocks)) return rc;
#define RESL(CS, P2) hipLaunchKernelGGL((residual_kernel<CS, P2, PixT>), dim3(p.grid), dim3(256), 0, (hipStream_t)stream, d_src, src_stride, \
                       src_block_pitch, d_pred, pred_stride, pred_block_pitch, d_res, res_stride, res_block_pitch,   \
                       width, height, (uint32_t)nblocks)
#define RESC(CS) if (p.pow2) RESL(CS, true); else RESL(CS, false)
    switch (p.rcs) {
    case 16: if constexpr (sizeof(PixT) == 1) { RESC(16); } break;
    case 8: RESC(8); break;
    case 4: RESC(4); break;
    default: RESC(1); break;
    }
#undef RESC
#undef RESL
    return launch_status("residual");
}
extern "C" int svt_hip_residual_batch(const uint8_t* d_src, uint32_t src_stride, size_t src_block_pitch,
                                      const uint8_t* d_pred, uint32_t pred_stride, size_t pred_block_pitch,
                                      int16_t* d_res, uint32_t res_stride, size_t res_block_pitch, uint32_t width,
                                      uint32_t height, size_t nblocks, void* stream) {
    return residual_impl<uint8_t>(d_src, src_stride, src_block_pitch, d_pred, pred_stride, pred_block_pitch, d_res, res_stride,
                                  res_block_pitch, width, height, nblocks, stream);
}
extern "C" int svt_hip_residual16_batch(const uint16_t* d_src, uint32_t src_stride, size_t src_block_pitch,
                                        const uint16_t* d_pred, uint32_t pred_stride, size_t pred_block_pitch,
                                        int16_t* d_res, uint32_t res_stride, size_t res_block_pitch, uint32_t width,
                                        uint32_t height, size_t nblocks, void* stream) {
    return residual_impl<uint16_t>(d_src, src_stride, src_block_pitch, d_pred, pred_stride, pred_block_pitch, d_res, res_stride,
                                   res_block_pitch, width, height, nblocks, stream);
}

static int sad_search_impl(bool need_offs, const uint8_t* d_src, uint32_t src_stride, size_t src_block_pitch, const uint32_t* d_src_offs, const uint8_t* d_ref,
                           uint32_t ref_stride, uint32_t ref_stride_raw, size_t ref_block_pitch, const uint32_t* d_ref_offs, uint32_t width, uint32_t height,
                           int16_t search_area_width, int16_t search_area_height, uint64_t* d_best_sad, int16_t* d_x, int16_t* d_y, size_t nblocks, void* stream) {
    if (int rc = require_init()) return rc;
    if (nblocks == 0) return SVT_HIP_OK;
    if (int rc = sad_search_args_check(need_offs, d_src_offs, d_ref_offs, d_src, d_ref, d_best_sad, d_x, d_y)) return rc;
    // the kernel, its variant, the launch shape and the LDS layout: search_plan.h
    const SadSearchKnobs knobs = {g_tune_no_qsad, g_tune_no_q2, g_tune_no_q2p, g_tune_no_q16, g_tune_q2_su4};
    SadSearchPlan p;
    if (int rc = sad_search_plan(width, height, search_area_width, search_area_height, ref_stride == ref_stride_raw, nblocks, knobs, g_num_cu, p)) return rc;
    const int sw = search_area_width, sh = search_area_height;
    unsigned long long* best = (unsigned long long*)d_best_sad;
    const uint32_t n = (uint32_t)nblocks;
#define SSL(KERNEL, ...) hipLaunchKernelGGL((KERNEL), dim3(p.grid), dim3(p.threads), p.lds, (hipStream_t)stream, __VA_ARGS__, d_src_offs, d_ref_offs, n)
#define SSQ(CW, CH) SSL((sad_search_q_kernel<CW, CH>), d_src, src_stride, src_block_pitch, d_ref, ref_stride, ref_stride_raw, ref_block_pitch, width, height, sw, sh, \
                        best, d_x, d_y, p.src_bytes, p.ref_bytes, p.lpb)
#define SSQ16(CW) SSL(sad_search_q16_kernel<CW>, d_src, src_stride, src_block_pitch, d_ref, ref_stride, ref_block_pitch, height, sw, sh, best, d_x, d_y, p.wpitch, \
                      p.ref_bytes, p.lpb, p.tsh, p.cpr_magic)
#define SSQ2(CW, CH, SU) SSL((sad_search_q2_kernel<CW, CH, SU>), d_src, src_stride, src_block_pitch, d_ref, ref_stride, ref_block_pitch, sw, sh, best, d_x, d_y, \
                             p.ref_bytes, p.lpb, p.cpr_magic)
#define SSQ2P(CW, CH) SSL((sad_search_q2p_kernel<CW, CH>), d_src, src_stride, src_block_pitch, d_ref, ref_stride, ref_block_pitch, sw, sh, best, d_x, d_y, p.wstride, \
                          p.wpitch, p.lpb, p.cpr_magic)
    switch (p.kernel) {
    case SAD_K_Q2P:
        if (p.cw == 16) SSQ2P(16, 16); else SSQ2P(8, 8);
        return launch_status("sad_search_q2p");
    case SAD_K_Q2:
        if (p.cw == 16) { if (p.su == 8) SSQ2(16, 16, 8); else SSQ2(16, 16, 4); }
        else { if (p.su == 8) SSQ2(8, 8, 8); else SSQ2(8, 8, 4); }
        return launch_status("sad_search_q2");
    case SAD_K_Q16:
        if (p.cw == 16) SSQ16(16); else if (p.cw == 32) SSQ16(32); else SSQ16(64);
        return launch_status("sad_search_q16");
    case SAD_K_Q:
        if (p.cw == 16) SSQ(16, 16); else if (p.cw == 8) SSQ(8, 8); else if (p.cw == 32) SSQ(32, 32); else if (p.cw == 64) SSQ(64, 64); else SSQ(0, 0);
        return launch_status("sad_search_q");
    default:
        SSL(sad_search_kernel, d_src, src_stride, src_block_pitch, d_ref, ref_stride, ref_stride_raw, ref_block_pitch, width, height, sw, sh, best, d_x, d_y,
            p.src_bytes, p.ref_bytes);
        return launch_status("sad_search");
    }
#undef SSQ2P
#undef SSQ2
#undef SSQ16
#undef SSQ
#undef SSL
}

extern "C" int svt_hip_sad_search_batch(const uint8_t* d_src, uint32_t src_stride, size_t src_block_pitch,
                                        const uint8_t* d_ref, uint32_t ref_stride, uint32_t ref_stride_raw,
                                        size_t ref_block_pitch, uint32_t width, uint32_t height,
                                        int16_t search_area_width, int16_t search_area_height,
                                        uint64_t* d_best_sad, int16_t* d_x, int16_t* d_y, size_t nblocks,
                                        void* stream) {
    return sad_search_impl(false, d_src, src_stride, src_block_pitch, nullptr, d_ref, ref_stride, ref_stride_raw, ref_block_pitch,
                           nullptr, width, height, search_area_width, search_area_height, d_best_sad, d_x, d_y, nblocks, stream);
}
extern "C" int svt_hip_sad_search_planes_batch(const uint8_t* d_src_plane, uint32_t src_stride, const uint32_t* d_src_offsets,
                                               const uint8_t* d_ref_plane, uint32_t ref_stride, uint32_t ref_stride_raw,
                                               const uint32_t* d_ref_offsets, uint32_t width, uint32_t height,
                                               int16_t search_area_width, int16_t search_area_height,
                                               uint64_t* d_best_sad, int16_t* d_x, int16_t* d_y, size_t nblocks,
                                               void* stream) {
    return sad_search_impl(true, d_src_plane, src_stride, 0, d_src_offsets, d_ref_plane, ref_stride, ref_stride_raw, 0, d_ref_offsets,
                           width, height, search_area_width, search_area_height, d_best_sad, d_x, d_y, nblocks, stream);
}

// A full-pel search the plan routed (me_plan.h): one workgroup per block
static int launch_me_fullpel(const MeFullpelRoute& r, const uint8_t* d_src, uint32_t src_stride, size_t src_block_pitch, const uint32_t* d_src_offs,
                             const uint8_t* d_ref, uint32_t ref_stride, size_t ref_block_pitch, const uint32_t* d_ref_offs, int search_w, int search_h,
                             const int16_t* d_origins, int x_origin, int y_origin, int flavour, int nsq, uint32_t* d_best_sad, uint32_t* d_best_mv, void* stream) {
    const dim3 grid(r.grid), threads(ME_THREADS);
    const hipStream_t s = (hipStream_t)stream;
    switch (r.kernel) {
    case ME_K_SQ16: {
        auto* kernel = !r.masked ? me_sb_search16_kernel<false> : me_sb_search16_kernel<true>;
        hipLaunchKernelGGL(kernel, grid, threads, r.lds, s, d_src, src_stride, src_block_pitch, d_ref, ref_stride, ref_block_pitch, search_w, search_h, d_origins,
                           x_origin, y_origin, d_best_sad, d_best_mv, r.window.wpitch, d_src_offs, d_ref_offs, r.grid, r.w8q, r.ref_layout, r.pu_pitch);
        return launch_status(r.ref_layout ? "me_sb_search16 (reference layout)" : "me_sb_search16");
    }
    case ME_K_NSQ4:
        hipLaunchKernelGGL(me_nsq4_kernel, grid, threads, r.lds, s, d_src, src_stride, src_block_pitch, d_ref, ref_stride, ref_block_pitch, search_w, search_h,
                           d_origins, x_origin, y_origin, d_best_sad, d_best_mv, r.window.wpitch, d_src_offs, d_ref_offs, r.grid, r.pu_pitch);
        return launch_status("me_nsq4");
    default:
        hipLaunchKernelGGL(me_fullpel_exact_kernel, grid, threads, 0, s, d_src, src_stride, src_block_pitch, d_src_offs, d_ref, ref_stride, ref_block_pitch,
                           d_ref_offs, search_w, search_h, d_origins, x_origin, y_origin, flavour, nsq ? 1 : 0, d_best_sad, d_best_mv, r.pu_pitch, r.grid);
        return launch_status("me_fullpel_exact");
    }
}

static int me_sb_search_impl(bool need_offs, const uint8_t* d_src, uint32_t src_stride, size_t src_block_pitch, const uint32_t* d_src_offs,
                             const uint8_t* d_ref, uint32_t ref_stride, size_t ref_block_pitch, const uint32_t* d_ref_offs,
                             int search_w, int search_h, const int16_t* d_origins, int x_origin,
                             int y_origin, uint32_t* d_best_sad, uint32_t* d_best_mv, size_t nblocks,
                             void* stream) {
    if (int rc = require_init()) return rc;
    if (nblocks == 0) return SVT_HIP_OK;
    MeFullpelRoute r;
    if (int rc = me_sb_search_plan(r, need_offs, d_src_offs, d_ref_offs, d_src, d_ref, d_best_sad, d_best_mv, search_w, search_h, nblocks)) return rc;
    return launch_me_fullpel(r, d_src, src_stride, src_block_pitch, d_src_offs, d_ref, ref_stride, ref_block_pitch, d_ref_offs, search_w, search_h, d_origins,
                             x_origin, y_origin, SVT_HIP_FLAVOUR_C, 0, d_best_sad, d_best_mv, stream);
}

extern "C" int svt_hip_me_sb_search_batch(const uint8_t* d_src, uint32_t src_stride, size_t src_block_pitch,
                                          const uint8_t* d_ref, uint32_t ref_stride, size_t ref_block_pitch,
                                          int search_w, int search_h, const int16_t* d_origins, int x_origin,
                                          int y_origin, uint32_t* d_best_sad, uint32_t* d_best_mv, size_t nblocks,
                                          void* stream) {
    return me_sb_search_impl(false, d_src, src_stride, src_block_pitch, nullptr, d_ref, ref_stride, ref_block_pitch, nullptr, search_w,
                             search_h, d_origins, x_origin, y_origin, d_best_sad, d_best_mv, nblocks, stream);
}
extern "C" int svt_hip_me_sb_search_planes_batch(const uint8_t* d_src_plane, uint32_t src_stride, const uint32_t* d_src_offsets,
                                                 const uint8_t* d_ref_plane, uint32_t ref_stride, const uint32_t* d_ref_offsets,
                                                 int search_w, int search_h, const int16_t* d_origins, int x_origin,
                                                 int y_origin, uint32_t* d_best_sad, uint32_t* d_best_mv, size_t nblocks,
                                                 void* stream) {
    return me_sb_search_impl(true, d_src_plane, src_stride, 0, d_src_offsets, d_ref_plane, ref_stride, 0, d_ref_offsets, search_w,
                             search_h, d_origins, x_origin, y_origin, d_best_sad, d_best_mv, nblocks, stream);
}

// one HME level for many SBs, search-area clipping on the device; 1 .. 4 search regions per launch (include/svt_hip_dsp.h)
extern "C" int svt_hip_hme_level_regions_batch(const uint8_t* d_src_pic, uint32_t src_stride, const uint8_t* d_ref_pic, uint32_t ref_stride,
                                               const int16_t* d_sb_origin, const uint16_t* d_sb_size, const int16_t* d_centers,
                                               int center_shift, const svt_hip_hme_params* params, int nregions, uint64_t* d_best_sad,
                                               int16_t* d_mv, size_t ntasks, void* stream) {
    if (int rc = require_init()) return rc;
    if (ntasks == 0) return SVT_HIP_OK;
    HmeLevelPlan p;
    if (int rc = hme_level_plan(p, d_src_pic, d_ref_pic, d_sb_origin, d_sb_size, center_shift, params, nregions, d_best_sad, d_mv, ntasks)) return rc;
    HmeParamSets hp;
    static_assert(sizeof(HmeParams) == sizeof(svt_hip_hme_params), "layout");
    memset(&hp, 0, sizeof(hp));
    memcpy(hp.p, params, (size_t)nregions * sizeof(HmeParams));
    hipLaunchKernelGGL(hme_level_kernel, dim3(p.grid_x, p.grid_y), dim3(ME_THREADS), p.win.lds, (hipStream_t)stream, d_src_pic, src_stride,
                       d_ref_pic, ref_stride, d_sb_origin, d_sb_size, d_centers, center_shift, hp, (unsigned long long*)d_best_sad, d_mv, p.win.wpitch,
                       p.grid_x);
    return launch_status("hme_level");
}
extern "C" int svt_hip_hme_level_batch(const uint8_t* d_src_pic, uint32_t src_stride, const uint8_t* d_ref_pic, uint32_t ref_stride,
                                       const int16_t* d_sb_origin, const uint16_t* d_sb_size, const int16_t* d_centers,
                                       int center_shift, const svt_hip_hme_params* params, uint64_t* d_best_sad, int16_t* d_mv,
                                       size_t ntasks, void* stream) {
    return svt_hip_hme_level_regions_batch(d_src_pic, src_stride, d_ref_pic, ref_stride, d_sb_origin, d_sb_size, d_centers, center_shift, params, 1,
                                           d_best_sad, d_mv, ntasks, stream);
}

// K6 in the reference's result layout, both result flavours, square or all 209 PUs (include/svt_hip_dsp.h); the kernel: me_fullpel_route
extern "C" int svt_hip_me_fullpel_search_batch(const uint8_t* d_src, uint32_t src_stride, size_t src_block_pitch,
                                               const uint32_t* d_src_offsets, const uint8_t* d_ref, uint32_t ref_stride,
                                               size_t ref_block_pitch, const uint32_t* d_ref_offsets, int search_w,
                                               int search_h, const int16_t* d_origins, int x_origin, int y_origin,
                                               int flavour, int nsq, uint32_t* d_best_sad, uint32_t* d_best_mv,
                                               uint32_t pu_pitch, size_t nblocks, void* stream) {
    if (int rc = require_init()) return rc;
    if (nblocks == 0) return SVT_HIP_OK;
    MeFullpelRoute r;
    if (int rc = me_fullpel_search_plan(r, d_src, d_ref, d_best_sad, d_best_mv, search_w, search_h, flavour, nsq, pu_pitch, nblocks, g_tune_me_exact)) return rc;
    return launch_me_fullpel(r, d_src, src_stride, src_block_pitch, d_src_offsets, d_ref, ref_stride, ref_block_pitch, d_ref_offsets, search_w, search_h,
                             d_origins, x_origin, y_origin, flavour, nsq, d_best_sad, d_best_mv, stream);
}

// ---- MotionEstimateLcu's glue: set-up, per-SB areas, bi-prediction + result rows (include/svt_hip_dsp.h) --------------------
extern "C" int svt_hip_me_setup_batch(const uint8_t* d_src_pic, uint32_t src_stride, const uint8_t* d_ref_pic, uint32_t ref_stride,
                                      const int16_t* d_sb_origin, const uint16_t* d_sb_size, const uint64_t* d_hme_sad, const int16_t* d_hme_mv,
                                      const svt_hip_me_setup_params* params, int16_t* d_center, int16_t* d_area, size_t ntasks, void* stream) {
    if (int rc = require_init()) return rc;
    if (ntasks == 0) return SVT_HIP_OK;
    uint32_t grid;
    if (int rc = me_setup_plan(grid, d_src_pic, d_ref_pic, d_sb_origin, d_sb_size, d_hme_sad, d_hme_mv, params, d_area, ntasks)) return rc;
    static_assert(sizeof(MeSetupParams) == sizeof(svt_hip_me_setup_params), "layout");
    MeSetupParams mp;
    memcpy(&mp, params, sizeof(mp));
    hipLaunchKernelGGL(me_setup_kernel, dim3(grid), dim3(256), 0, (hipStream_t)stream, d_src_pic, src_stride, d_ref_pic,
                       ref_stride, d_sb_origin, d_sb_size, (const unsigned long long*)d_hme_sad, d_hme_mv, mp, d_center, d_area, (uint32_t)ntasks);
    return launch_status("me_setup");
}

extern "C" int svt_hip_me_fullpel_search_areas_batch(const uint8_t* d_src, uint32_t src_stride, const uint32_t* d_src_offsets, const uint8_t* d_ref,
                                                     uint32_t ref_stride, const uint32_t* d_ref_offsets, const int16_t* d_areas, int max_search_w,
                                                     int max_search_h, int flavour, int nsq, uint32_t* d_best_sad, uint32_t* d_best_mv,
                                                     uint32_t pu_pitch, size_t nblocks, void* stream) {
    if (int rc = require_init()) return rc;
    if (nblocks == 0) return SVT_HIP_OK;
    MeAreasPlan p;
    if (int rc = me_fullpel_areas_plan(p, d_src, d_ref, d_src_offsets, d_ref_offsets, d_areas, d_best_sad, d_best_mv, max_search_w, max_search_h, flavour, nsq,
                                       pu_pitch, nblocks))
        return rc;
    auto* kernel = p.nsq ? me_fullpel_areas_kernel<true> : me_fullpel_areas_kernel<false>;
    hipLaunchKernelGGL(kernel, dim3(p.grid), dim3(ME_THREADS), p.window.lds, (hipStream_t)stream, d_src, src_stride, d_src_offsets, d_ref, ref_stride,
                       d_ref_offsets, d_areas, max_search_w, max_search_h, flavour, d_best_sad, d_best_mv, pu_pitch, p.window.wpitch, p.window.pair_off, p.grid);
    return launch_status("me_fullpel_areas");
}

// raster PU order (partitionWidth / partitionHeight / puSearchIndexMap, EbMotionEstimation.h:178-315): 14 shape groups, each a
// raster walk of its grid; the storage index is the PU of the result rows with the same rectangle (me_pu_rect)
const MePuMap& svthost::me_pu_map() {
    static const MePuMap m = [] {
        MePuMap t;
        memset(&t, 0, sizeof(t));
        static const int gw[14] = {8, 4, 2, 1, 8, 4, 2, 4, 2, 1, 4, 1, 8, 2}, gh[14] = {8, 4, 2, 1, 4, 2, 1, 8, 4, 2, 1, 4, 2, 8};
        int p = 0, rows = 0;
        for (int g = 0; g < 14; g++) {
            const int cols = 8 / gw[g], n = cols * (8 / gh[g]);
            for (int i = 0; i < n; i++, p++) {
                const int x = (i % cols) * gw[g], y = (i / cols) * gh[g];
                t.x8[p] = (uint8_t)x; t.y8[p] = (uint8_t)y; t.w8[p] = (uint8_t)gw[g]; t.h8[p] = (uint8_t)gh[g];
                t.row0[p] = (uint16_t)rows;
                rows += 4 * gh[g];
                int found = 255;
                for (int q = 0; q < ME_PUS_ALL; q++) {
                    int qx, qy, qw, qh;
                    me_pu_rect(q, qx, qy, qw, qh);
                    if (qx == x && qy == y && qw == gw[g] && qh == gh[g]) { found = q; break; }
                }
                t.storage[p] = (uint8_t)found;
            }
        }
        t.row0[ME_PUS_ALL] = (uint16_t)rows;
        return t;
    }();
    return m;
}
extern "C" int svt_hip_me_pu_storage_index(int pu_index) {
    if (pu_index < 0 || pu_index >= ME_PUS_ALL) return -1;
    return me_pu_map().storage[pu_index];
}

extern "C" int svt_hip_me_bipred_batch(const uint8_t* d_src_pic, uint32_t src_stride, const uint8_t* d_ref0_pic, uint32_t ref0_stride,
                                       const uint8_t* d_ref1_pic, uint32_t ref1_stride, const int16_t* d_sb_origin, const uint32_t* d_best_sad0,
                                       const uint32_t* d_best_mv0, const uint32_t* d_best_sad1, const uint32_t* d_best_mv1, uint32_t pu_pitch, int npus,
                                       int bipred_all_pus, int sub_sad, uint32_t* d_bipred_sad, svt_hip_me_result* d_results, size_t nsb, void* stream) {
    if (int rc = require_init()) return rc;
    if (nsb == 0) return SVT_HIP_OK;
    MeBipredPlan p;
    if (int rc = me_bipred_plan(p, d_src_pic, d_ref0_pic, d_ref1_pic, d_sb_origin, d_best_sad0, d_best_mv0, d_best_sad1, d_best_mv1, pu_pitch, npus, bipred_all_pus,
                                sub_sad, d_results, nsb))
        return rc;
    static_assert(sizeof(MeResult) == sizeof(svt_hip_me_result), "layout");
    hipLaunchKernelGGL(me_bipred_kernel, dim3(p.grid), dim3(ME_THREADS), 0, (hipStream_t)stream, d_src_pic, src_stride, d_ref0_pic, ref0_stride,
                       d_ref1_pic, ref1_stride, d_sb_origin, d_best_sad0, d_best_mv0, d_best_sad1, d_best_mv1, pu_pitch, npus, p.all_pus, p.sub_sad, me_pu_map(),
                       d_bipred_sad, reinterpret_cast<MeResult*>(d_results), p.grid);
    return launch_status("me_bipred");
}

static int full_distortion32_impl(const int32_t* d_coeff, uint32_t coeff_stride, size_t coeff_block_pitch, const int32_t* d_recon,
                                  uint32_t recon_stride, size_t recon_block_pitch, uint32_t width, uint32_t height,
                                  int cbf_zero, const uint32_t* d_nz, int flavour, uint64_t* d_out, size_t nblocks, void* stream) {
    if (int rc = require_init()) return rc;
    if (nblocks == 0) return SVT_HIP_OK;
    Dist32Plan p;
    if (int rc = full_distortion32_plan(p, d_coeff, d_recon, d_out, width, height, cbf_zero, flavour, nblocks)) return rc;
    auto* kernel = p.avx2 ? full_distortion32_kernel<true> : full_distortion32_kernel<false>;
    hipLaunchKernelGGL(kernel, dim3(p.grid), dim3(256), 0, (hipStream_t)stream, d_coeff, coeff_stride, coeff_block_pitch, d_recon, recon_stride,
                       recon_block_pitch, width, height, cbf_zero, d_nz, (unsigned long long*)d_out, (uint32_t)nblocks);
    return launch_status("full_distortion32");
}
extern "C" int svt_hip_full_distortion32_batch(const int32_t* d_coeff, uint32_t coeff_stride, size_t coeff_block_pitch,
                                               const int32_t* d_recon, uint32_t recon_stride, size_t recon_block_pitch,
                                               uint32_t width, uint32_t height, int cbf_zero, uint64_t* d_out,
                                               size_t nblocks, void* stream) {
    return full_distortion32_impl(d_coeff, coeff_stride, coeff_block_pitch, d_recon, recon_stride, recon_block_pitch, width, height,
                                  cbf_zero, nullptr, SVT_HIP_FLAVOUR_C, d_out, nblocks, stream);
}
extern "C" int svt_hip_picture_full_distortion32_batch(const int32_t* d_coeff, size_t coeff_block_pitch, const int32_t* d_recon,
                                                       size_t recon_block_pitch, uint32_t bwidth, uint32_t bheight,
                                                       const uint32_t* d_count_non_zero_coeffs, int flavour, uint64_t* d_out,
                                                       size_t nblocks, void* stream) {
    // picture_full_distortion32_bits (EbPictureOperators.c:349-457): the row stride of both buffers is the (clamped) width,
    // count_non_zero_coeffs == 0 selects the cbf_zero kernel per block.  (cbf_zero 0: a NULL d_recon is refused like any NULL buffer)
    const uint32_t w = dist32_picture_side(bwidth), h = dist32_picture_side(bheight);
    return full_distortion32_impl(d_coeff, w, coeff_block_pitch, d_recon, w, recon_block_pitch, w, h, 0, d_count_non_zero_coeffs, flavour,
                                  d_out, nblocks, stream);
}

// copies a w x h u8 block with `stride` into dense device memory
static void h2d_block(void* d, const uint8_t* h, uint32_t stride, uint32_t w, uint32_t ht, const char* fn) {
    HIP_DIE(hipMemcpy2DAsync(d, w, h, stride, w, ht, hipMemcpyHostToDevice, t_ctx.stream), fn);
}

extern "C" uint32_t svt_hip_nxm_sad_kernel(const uint8_t* src, uint32_t src_stride, const uint8_t* ref,
                                           uint32_t ref_stride, uint32_t height, uint32_t width) {
    const char* fn = "svt_hip_nxm_sad_kernel";
    const size_t bb = align256((size_t)width * height);
    DROPIN_TRY(t_ctx.ensure(2 * bb + 256), fn);
    uint8_t* d_a = (uint8_t*)t_ctx.dbuf;
    uint8_t* d_b = d_a + bb;
    uint32_t* d_o = (uint32_t*)(d_a + 2 * bb);
    h2d_block(d_a, src, src_stride, width, height, fn);
    h2d_block(d_b, ref, ref_stride, width, height, fn);
    DROPIN_TRY(svt_hip_sad_batch(d_a, width, 0, d_b, width, 0, width, height, d_o, 1, t_ctx.stream), fn);
    uint32_t out = 0;
    HIP_DIE(hipMemcpyAsync(&out, d_o, 4, hipMemcpyDeviceToHost, t_ctx.stream), fn);
    HIP_DIE(hipStreamSynchronize(t_ctx.stream), fn);
    return out;
}
extern "C" uint64_t svt_hip_spatial_full_distortion_kernel(uint8_t* input, uint32_t input_stride, uint8_t* recon,
                                                           uint32_t recon_stride, uint32_t area_width,
                                                           uint32_t area_height) {
    const char* fn = "svt_hip_spatial_full_distortion_kernel";
    const size_t bb = align256((size_t)area_width * area_height);
    DROPIN_TRY(t_ctx.ensure(2 * bb + 256), fn);
    uint8_t* d_a = (uint8_t*)t_ctx.dbuf;
    uint8_t* d_b = d_a + bb;
    uint64_t* d_o = (uint64_t*)(d_a + 2 * bb);
    h2d_block(d_a, input, input_stride, area_width, area_height, fn);
    h2d_block(d_b, recon, recon_stride, area_width, area_height, fn);
    DROPIN_TRY(svt_hip_sse_batch(d_a, area_width, 0, d_b, area_width, 0, area_width, area_height, d_o, 1, t_ctx.stream), fn);
    uint64_t out = 0;
    HIP_DIE(hipMemcpyAsync(&out, d_o, 8, hipMemcpyDeviceToHost, t_ctx.stream), fn);
    HIP_DIE(hipStreamSynchronize(t_ctx.stream), fn);
    return out;
}
extern "C" void svt_hip_residual_kernel(uint8_t* input, uint32_t input_stride, uint8_t* pred, uint32_t pred_stride,
                                        int16_t* residual, uint32_t residual_stride, uint32_t area_width,
                                        uint32_t area_height) {
    const char* fn = "svt_hip_residual_kernel";
    const size_t bb = align256((size_t)area_width * area_height);
    DROPIN_TRY(t_ctx.ensure(4 * bb), fn);
    uint8_t* d_a = (uint8_t*)t_ctx.dbuf;
    uint8_t* d_b = d_a + bb;
    int16_t* d_r = (int16_t*)(d_a + 2 * bb);
    h2d_block(d_a, input, input_stride, area_width, area_height, fn);
    h2d_block(d_b, pred, pred_stride, area_width, area_height, fn);
    DROPIN_TRY(svt_hip_residual_batch(d_a, area_width, 0, d_b, area_width, 0, d_r, area_width, 0, area_width, area_height, 1, t_ctx.stream), fn);
    HIP_DIE(hipMemcpy2DAsync(residual, (size_t)residual_stride * 2, d_r, (size_t)area_width * 2, (size_t)area_width * 2,
                             area_height, hipMemcpyDeviceToHost, t_ctx.stream), fn);
    HIP_DIE(hipStreamSynchronize(t_ctx.stream), fn);
}
extern "C" void svt_hip_sad_loop_kernel(uint8_t* src, uint32_t src_stride, uint8_t* ref, uint32_t ref_stride,
                                        uint32_t height, uint32_t width, uint64_t* best_sad, int16_t* x_search_center,
                                        int16_t* y_search_center, uint32_t src_stride_raw, int16_t search_area_width,
                                        int16_t search_area_height) {
    const char* fn = "svt_hip_sad_loop_kernel";
    // stage the touched source rows and the touched reference span as-is (strides kept)
    const size_t src_span = (size_t)(height - 1) * src_stride + width;
    const size_t ref_span = (size_t)(search_area_height - 1) * src_stride_raw + (size_t)(height - 1) * ref_stride +
                            width + search_area_width - 1;
    const size_t sb = align256(src_span), rb = align256(ref_span);
    DROPIN_TRY(t_ctx.ensure(sb + rb + 256), fn);
    uint8_t* d_s = (uint8_t*)t_ctx.dbuf;
    uint8_t* d_r = d_s + sb;
    uint64_t* d_best = (uint64_t*)(d_r + rb);
    int16_t* d_xy = (int16_t*)(d_best + 1);
    int16_t xy[2] = {*x_search_center, *y_search_center};
    HIP_DIE(hipMemcpyAsync(d_s, src, src_span, hipMemcpyHostToDevice, t_ctx.stream), fn);
    HIP_DIE(hipMemcpyAsync(d_r, ref, ref_span, hipMemcpyHostToDevice, t_ctx.stream), fn);
    HIP_DIE(hipMemcpyAsync(d_xy, xy, 4, hipMemcpyHostToDevice, t_ctx.stream), fn);
    DROPIN_TRY(svt_hip_sad_search_batch(d_s, src_stride, 0, d_r, ref_stride, src_stride_raw, 0, width, height,
                                        search_area_width, search_area_height, d_best, d_xy, d_xy + 1, 1, t_ctx.stream), fn);
    HIP_DIE(hipMemcpyAsync(best_sad, d_best, 8, hipMemcpyDeviceToHost, t_ctx.stream), fn);
    HIP_DIE(hipMemcpyAsync(xy, d_xy, 4, hipMemcpyDeviceToHost, t_ctx.stream), fn);
    HIP_DIE(hipStreamSynchronize(t_ctx.stream), fn);
    *x_search_center = xy[0];
    *y_search_center = xy[1];
}

static void dropin_dist32(int cbf_zero, int32_t* coeff, uint32_t cs, int32_t* recon, uint32_t rs, uint64_t out[2],
                          uint32_t w, uint32_t h, const char* fn) {
    const size_t bb = align256((size_t)w * h * 4);
    DROPIN_TRY(t_ctx.ensure(2 * bb + 256), fn);
    int32_t* d_c = (int32_t*)t_ctx.dbuf;
    int32_t* d_r = (int32_t*)(t_ctx.dbuf + bb);
    uint64_t* d_o = (uint64_t*)(t_ctx.dbuf + 2 * bb);
    HIP_DIE(hipMemcpy2DAsync(d_c, (size_t)w * 4, coeff, (size_t)cs * 4, (size_t)w * 4, h, hipMemcpyHostToDevice, t_ctx.stream), fn);
    if (!cbf_zero)
        HIP_DIE(hipMemcpy2DAsync(d_r, (size_t)w * 4, recon, (size_t)rs * 4, (size_t)w * 4, h, hipMemcpyHostToDevice, t_ctx.stream), fn);
    DROPIN_TRY(svt_hip_full_distortion32_batch(d_c, w, 0, d_r, w, 0, w, h, cbf_zero, d_o, 1, t_ctx.stream), fn);
    HIP_DIE(hipMemcpyAsync(out, d_o, 16, hipMemcpyDeviceToHost, t_ctx.stream), fn);
    HIP_DIE(hipStreamSynchronize(t_ctx.stream), fn);
}
extern "C" void svt_hip_full_distortion_kernel32_bits(int32_t* coeff, uint32_t coeff_stride, int32_t* recon_coeff,
                                                      uint32_t recon_coeff_stride, uint64_t distortion_result[2],
                                                      uint32_t area_width, uint32_t area_height) {
    dropin_dist32(0, coeff, coeff_stride, recon_coeff, recon_coeff_stride, distortion_result, area_width, area_height,
                  "svt_hip_full_distortion_kernel32_bits");
}
extern "C" void svt_hip_full_distortion_kernel_cbf_zero32_bits(int32_t* coeff, uint32_t coeff_stride, int32_t* recon_coeff,
                                                               uint32_t recon_coeff_stride, uint64_t distortion_result[2],
                                                               uint32_t area_width, uint32_t area_height) {
    dropin_dist32(1, coeff, coeff_stride, recon_coeff, recon_coeff_stride, distortion_result, area_width, area_height,
                  "svt_hip_full_distortion_kernel_cbf_zero32_bits");
}


// combined_averaging_sad (EB_SADAVGKERNELNxM_TYPE, EbComputeSAD.h:49-57; NxMSadAveragingKernel_funcPtrArray)
extern "C" uint32_t svt_hip_combined_averaging_sad(uint8_t* src, uint32_t src_stride, uint8_t* ref1, uint32_t ref1_stride,
                                                   uint8_t* ref2, uint32_t ref2_stride, uint32_t height, uint32_t width) {
    const char* fn = "svt_hip_combined_averaging_sad";
    const size_t bb = align256((size_t)width * height);
    DROPIN_TRY(t_ctx.ensure(3 * bb + 256), fn);
    uint8_t* d_a = (uint8_t*)t_ctx.dbuf;
    uint8_t* d_b = d_a + bb;
    uint8_t* d_c = d_a + 2 * bb;
    uint32_t* d_o = (uint32_t*)(d_a + 3 * bb);
    h2d_block(d_a, src, src_stride, width, height, fn);
    h2d_block(d_b, ref1, ref1_stride, width, height, fn);
    h2d_block(d_c, ref2, ref2_stride, width, height, fn);
    DROPIN_TRY(svt_hip_sad_avg_batch(d_a, width, 0, d_b, width, 0, d_c, width, 0, width, height, d_o, 1, t_ctx.stream), fn);
    uint32_t out = 0;
    HIP_DIE(hipMemcpyAsync(&out, d_o, 4, hipMemcpyDeviceToHost, t_ctx.stream), fn);
    HIP_DIE(hipStreamSynchronize(t_ctx.stream), fn);
    return out;
}

// aom_sadMxN / aom_sadMxNx4d (aom_dsp_rtcd.h:1328-1500; C: C_DEFAULT/EbComputeSAD_C.c:140-233)
static void dropin_sad_x4d(int w, int h, const uint8_t* src, int src_stride, const uint8_t* const ref[4], int ref_stride,
                           uint32_t* sad_array, const char* fn) {
    const size_t bb = align256((size_t)w * h);
    DROPIN_TRY(t_ctx.ensure(5 * bb + 256), fn);
    uint8_t* d = (uint8_t*)t_ctx.dbuf;
    uint32_t* d_o = (uint32_t*)(d + 5 * bb);
    h2d_block(d, src, (uint32_t)src_stride, w, h, fn);
    for (int i = 0; i < 4; i++) h2d_block(d + (size_t)(1 + i) * bb, ref[i], (uint32_t)ref_stride, w, h, fn);
    // four dense reference blocks bb bytes apart against one source block (a_shift = 2 through the x4d entry point)
    const uint32_t offs[4] = {0, (uint32_t)bb, (uint32_t)(2 * bb), (uint32_t)(3 * bb)};
    uint32_t* d_offs = d_o + 4;
    HIP_DIE(hipMemcpyAsync(d_offs, offs, sizeof(offs), hipMemcpyHostToDevice, t_ctx.stream), fn);
    DROPIN_TRY(svt_hip_sad_x4d_batch(d, w, 0, nullptr, d + bb, w, d_offs, w, h, d_o, 1, t_ctx.stream), fn);
    HIP_DIE(hipMemcpyAsync(sad_array, d_o, 16, hipMemcpyDeviceToHost, t_ctx.stream), fn);
    HIP_DIE(hipStreamSynchronize(t_ctx.stream), fn);
}
#define DEF_SAD(W, H)                                                                                                          \
    extern "C" unsigned int svt_hip_aom_sad##W##x##H(const uint8_t* src_ptr, int src_stride, const uint8_t* ref_ptr, int ref_stride) { \
        return svt_hip_nxm_sad_kernel(src_ptr, (uint32_t)src_stride, ref_ptr, (uint32_t)ref_stride, H, W);                     \
    }                                                                                                                          \
    extern "C" void svt_hip_aom_sad##W##x##H##x4d(const uint8_t* src_ptr, int src_stride, const uint8_t* const ref_ptr[],     \
                                                  int ref_stride, uint32_t* sad_array) {                                      \
        dropin_sad_x4d(W, H, src_ptr, src_stride, ref_ptr, ref_stride, sad_array, "svt_hip_aom_sad" #W "x" #H "x4d");          \
    }
SVT_HIP_SAD_SIZES(DEF_SAD)
#undef DEF_SAD

// residual_kernel16bit (EbPictureOperators.c:134-164)
extern "C" void svt_hip_residual_kernel16bit(uint16_t* input, uint32_t input_stride, uint16_t* pred, uint32_t pred_stride,
                                             int16_t* residual, uint32_t residual_stride, uint32_t area_width,
                                             uint32_t area_height) {
    const char* fn = "svt_hip_residual_kernel16bit";
    const size_t bb = align256((size_t)area_width * area_height * 2);
    DROPIN_TRY(t_ctx.ensure(3 * bb), fn);
    uint16_t* d_a = (uint16_t*)t_ctx.dbuf;
    uint16_t* d_b = (uint16_t*)(t_ctx.dbuf + bb);
    int16_t* d_r = (int16_t*)(t_ctx.dbuf + 2 * bb);
    const size_t rowb = (size_t)area_width * 2;
    HIP_DIE(hipMemcpy2DAsync(d_a, rowb, input, (size_t)input_stride * 2, rowb, area_height, hipMemcpyHostToDevice, t_ctx.stream), fn);
    HIP_DIE(hipMemcpy2DAsync(d_b, rowb, pred, (size_t)pred_stride * 2, rowb, area_height, hipMemcpyHostToDevice, t_ctx.stream), fn);
    DROPIN_TRY(svt_hip_residual16_batch(d_a, area_width, 0, d_b, area_width, 0, d_r, area_width, 0, area_width, area_height, 1, t_ctx.stream), fn);
    HIP_DIE(hipMemcpy2DAsync(residual, (size_t)residual_stride * 2, d_r, rowb, rowb, area_height, hipMemcpyDeviceToHost, t_ctx.stream), fn);
    HIP_DIE(hipStreamSynchronize(t_ctx.stream), fn);
}

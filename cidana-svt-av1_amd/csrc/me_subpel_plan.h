// me_subpel_plan.h — what the sub-pel motion estimation calls (svt_hip_me_subpel_frame, svt_hip_motion_estimate_subpel_frame,
// svt_hip_me_subpel_planes) settle on the host before they enqueue: the checks, the padding the interpolation needs, the LDS sizes and
// the grid; and every check of both whole-picture calls put together (me_frame_check).  The clauses it shares with the full-pel calls, the
// padded-plane check and the geometry are me_plan.h's.  Host only (no HIP header): tests/c/me_subpel_plan_host.cpp compiles it with g++; the kernels (kernel_me_subpel.h) use the same
// constants.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "../../include/svt_hip_dsp.h"
#include "host_err.h"
#include "me_plan.h"

namespace svthost {

// ---- the padding ---------------------------------------------------------------------------------------------------------------------
// MotionEstimateLcu clips a search area's origin to BLOCK_SIZE_64 - 1 samples left of / above the picture and its last point to the
// picture's last sample (:7955-8040), so the top-left sample of a PU's block at its full-pel winner lies in [-63, side - 1] and the block
// ends at most 64 samples after that.  The refinement reads, around that block:
//   ME_FILTER_TAP >> 1 = 2 samples before it   plane B at the block's first column reads I[x - 2 .. x + 1], plane H / J likewise in y
//   3 samples after it                         the quarter pass starts at (mv + 2) >> 2, one sample further when the half-pel winner lies
//                                              right of / below the full-pel one; it reads plane B / J one more sample to the right there
//                                              (pos_b + 1, pos_j + stride); and the filter reaches one sample past the sample it centres on
// The reference reads from integer_buffer_ptr = the window's origin minus ME_FILTER_TAP >> 1 rows and columns (:8048-8052) with one more
// row / column of filter reach: the same 2 on the near side (its first plane column is the sample LEFT of search point 0, which no PU
// reads), and on the far side the whole ROUND_UP_MUL_8(width + 2) region its kernels want, which the refinement never reads.
constexpr int ME_SP_FILTER_TAP = 4;                                  // ME_FILTER_TAP
constexpr int ME_SP_AREA_PAD = 63;                                   // BLOCK_SIZE_64 - 1
constexpr int ME_SP_BEFORE = ME_SP_FILTER_TAP >> 1, ME_SP_AFTER = 3; // samples of window before / after a PU's block
constexpr int ME_SP_FIRST = -ME_SP_AREA_PAD - ME_SP_BEFORE;          // first sample read: -65
constexpr int ME_SP_LAST_PAST_SIDE = 64 - 2 + ME_SP_AFTER;           // last sample read: (side - 1) + (64 - 1) + 3 = side + 65
constexpr int ME_SP_MARGIN = ME_SP_LAST_PAST_SIDE + 1;               // samples of padding on every side: 66
static_assert(-ME_SP_FIRST <= ME_SP_MARGIN && ME_SP_MARGIN == 66 && ME_SP_MARGIN <= 68, "the encoder's 68-sample padding must pass");

// ---- LDS -----------------------------------------------------------------------------------------------------------------------------
// A wave refines one PU at a time from its own window: the integer samples of the block with ME_SP_BEFORE / ME_SP_AFTER samples round
// it, and plane B of those rows (planes H and J are taken from the two on the fly).  The bi-prediction keeps one list's compensated block
// next to the window while it stages the other list's.  No window of the search is too large: the LDS does not depend on the search area.
constexpr int ME_SP_THREADS = 256, ME_SP_WAVES = ME_SP_THREADS / 64;
constexpr int ME_SP_WIN = 64 + ME_SP_BEFORE + ME_SP_AFTER;           // 69 rows / columns of integer samples
constexpr int ME_SP_IW = 72, ME_SP_BW = 68;                          // row pitches of the integer window and of plane B (64 + 2 columns)
constexpr int ME_SP_WAVE_LDS = (ME_SP_WIN * ME_SP_IW + ME_SP_WIN * ME_SP_BW + 15) & ~15;
constexpr int ME_SP_REFINE_LDS = ME_SP_WAVES * ME_SP_WAVE_LDS;
constexpr int ME_SP_BIPRED_LDS = ME_SP_WAVES * (ME_SP_WAVE_LDS + 64 * 64);
constexpr int ME_SP_BIPRED_TABLES = 209 * 4 + 1472;                  // the kernel's own cells: per-PU sums and the PU map
static_assert(ME_SP_IW >= ME_SP_WIN && ME_SP_BW >= 64 + 2 && ME_SP_REFINE_LDS <= 64 * 1024 && ME_SP_BIPRED_LDS + ME_SP_BIPRED_TABLES <= 64 * 1024,
              "static LDS of a workgroup");

constexpr uint32_t ME_SP_MAX_PICS = ME_FRAME_MAX_PICS;

inline bool me_sp_flag(int32_t v) { return v == 0 || v == 1; }

inline int me_subpel_params_check(const svt_hip_me_subpel_params* s) {
    if (!s) return SVT_HIP_OK;                           // NULL: the reference's setting, everything on
    if (!me_sp_flag(s->fractional_search64x64) || !me_sp_flag(s->enable_half_pel32x32) || !me_sp_flag(s->enable_half_pel16x16) ||
        !me_sp_flag(s->enable_half_pel8x8) || !me_sp_flag(s->enable_quarter_pel))
        return set_err(SVT_HIP_ERR_INVALID, "sub-pel enables must be 0 or 1");
    return SVT_HIP_OK;
}

// what the stage reads of the frame parameters: the shared clauses (me_plan.h), then its own
inline int me_subpel_frame_check(const svt_hip_me_frame_params* P) {
    if (int rc = me_picture_check(P)) return rc;
    if (int rc = me_pus_check(P)) return rc;
    if (P->fractional_search_method < 0 || P->fractional_search_method > 2)
        return set_err(SVT_HIP_ERR_INVALID, "fractional_search_method %d (SUB_SAD 0, FULL_SAD 1, SSD 2)", P->fractional_search_method);
    if (P->cu8x8_mode < 0) return set_err(SVT_HIP_ERR_INVALID, "negative cu8x8_mode");
    return SVT_HIP_OK;
}

inline int me_subpel_pictures_check(const svt_hip_me_pyramid* src, const svt_hip_me_pyramid* ref0, const svt_hip_me_pyramid* ref1,
                                    const svt_hip_me_frame_params* P, uint32_t n_pictures) {
    if (n_pictures > ME_SP_MAX_PICS) return set_err(SVT_HIP_ERR_INVALID, "%u pictures (at most %u)", n_pictures, ME_SP_MAX_PICS);
    const uint32_t w = (uint32_t)P->picture_width, h = (uint32_t)P->picture_height;
    // the source is read inside its SBs only (a partial SB's block reaches 56 samples into the padding): the search's own 64 do
    if (int rc = me_plane_check(src, 0, w, h, 64, n_pictures, "source", ME_READ_BLOCKS)) return rc;
    if (int rc = me_plane_check(ref0, 0, w, h, ME_SP_MARGIN, n_pictures, "list 0", ME_READ_INTERPOLATION)) return rc;
    if (P->slice_type == SVT_HIP_SLICE_B) { if (int rc = me_plane_check(ref1, 0, w, h, ME_SP_MARGIN, n_pictures, "list 1", ME_READ_INTERPOLATION)) return rc; }
    else if (ref1) return set_err(SVT_HIP_ERR_INVALID, "a P picture takes no list-1 reference");
    return SVT_HIP_OK;
}

// grid of the refinement: (SB, list, picture); the bi-prediction's: (SB, 1, picture)
inline int me_subpel_grid(const svt_hip_me_frame_params* P, uint32_t n_pictures, uint32_t g[3]) {
    const MeGeom m = me_geom(*P);
    g[0] = m.nsb; g[1] = (uint32_t)m.nl; g[2] = n_pictures;
    return me_geom_check(m);
}

// the scalars the two kernels take: a NULL enable set is the reference's, everything on
struct MeSubpelScalars { int f64, h32, h16, h8, qp, no8; };
inline MeSubpelScalars me_subpel_scalars(const svt_hip_me_frame_params& P, const svt_hip_me_subpel_params* sp) {
    MeSubpelScalars s;
    s.f64 = sp ? sp->fractional_search64x64 : 1;
    s.h32 = sp ? sp->enable_half_pel32x32 : 1; s.h16 = sp ? sp->enable_half_pel16x16 : 1; s.h8 = sp ? sp->enable_half_pel8x8 : 1;
    s.qp = sp ? sp->enable_quarter_pel : 1;
    s.no8 = P.cu8x8_mode == 1 ? 1 : 0;                   // disable8x8CuInMeFlag = cu8x8_mode == CU_8x8_MODE_1 (:8205)
    return s;
}

// every check of svt_hip_me_subpel_frame
inline int me_subpel_check(const svt_hip_me_pyramid* src, const svt_hip_me_pyramid* ref0, const svt_hip_me_pyramid* ref1, const svt_hip_me_frame_params* P,
                           const svt_hip_me_subpel_params* sp, uint32_t n_pictures, const uint32_t* d_best_sad,
                           const uint32_t* d_best_mv, const uint32_t* d_best_ssd, const uint8_t* d_half_dir) {
    if (int rc = me_subpel_frame_check(P)) return rc;
    if (int rc = me_subpel_params_check(sp)) return rc;
    if (int rc = me_subpel_pictures_check(src, ref0, ref1, P, n_pictures)) return rc;
    (void)d_half_dir;                                    // bytes: any address
    if (!d_best_sad || !d_best_mv) return set_err(SVT_HIP_ERR_INVALID, "NULL d_best_sad / d_best_mv");
    if (((uintptr_t)d_best_sad & 3) || ((uintptr_t)d_best_mv & 3) || ((uintptr_t)d_best_ssd & 3))
        return set_err(SVT_HIP_ERR_INVALID, "misaligned rows");
    uint32_t g[3];
    return me_subpel_grid(P, n_pictures, g);
}

// every check of svt_hip_motion_estimate_frame (subpel off) and svt_hip_motion_estimate_subpel_frame, in the order a caller observes;
// then the plan holds the launches' scalars (me_plan.h).  An empty stack is validated like any other.
inline int me_frame_check(const svt_hip_me_pyramid* src, const svt_hip_me_pyramid* ref0, const svt_hip_me_pyramid* ref1, const svt_hip_me_frame_params* P, bool subpel,
                          const svt_hip_me_subpel_params* sp, uint32_t n_pictures, const uint32_t* d_best_sad, const uint32_t* d_best_mv,
                          const int16_t* d_area_origin, const uint32_t* d_bipred_sad, const svt_hip_me_result* d_results, const void* d_scratch, size_t scratch_bytes,
                          MeFramePlan& pl) {
    if (int rc = me_frame_plan(P, pl)) return rc;
    if (subpel) {
        if (int rc = me_subpel_frame_check(P)) return rc;
        if (int rc = me_subpel_params_check(sp)) return rc;
    }
    if (int rc = me_frame_pictures_check(src, ref0, ref1, P, pl, n_pictures)) return rc;
    if (subpel) { if (int rc = me_subpel_pictures_check(src, ref0, ref1, P, n_pictures)) return rc; }      // the interpolation's wider padding
    return me_frame_outputs_check(ref0, ref1, pl, n_pictures, d_best_sad, d_best_mv, d_area_origin, d_bipred_sad, d_results, d_scratch, scratch_bytes);
}

// svt_hip_me_subpel_planes: the window's samples and the filter's reach must lie inside the padded plane
inline int me_subpel_planes_check(const svt_hip_me_pyramid* ref, int32_t width, int32_t height, int32_t x0, int32_t y0, uint32_t w, uint32_t h,
                                  const uint8_t* d_planes) {
    if (width < 8 || height < 8 || width > 16384 || height > 16384) return set_err(SVT_HIP_ERR_INVALID, "picture %d x %d", width, height);
    if (int rc = me_plane_check(ref, 0, (uint32_t)width, (uint32_t)height, ME_SP_MARGIN, 1, "reference", ME_READ_INTERPOLATION)) return rc;
    if (!d_planes) return set_err(SVT_HIP_ERR_INVALID, "NULL d_planes");
    if (w < 1 || h < 1 || w > 4096 || h > 4096) return set_err(SVT_HIP_ERR_INVALID, "window %u x %u (1 .. 4096)", w, h);
    // plane J at (y, x) reads I[y - 2 .. y + 1][x - 2 .. x + 1]
    if (x0 - 2 < -ME_SP_MARGIN || y0 - 2 < -ME_SP_MARGIN || (int64_t)x0 + w + 1 > (int64_t)width + ME_SP_MARGIN || (int64_t)y0 + h + 1 > (int64_t)height + ME_SP_MARGIN)
        return set_err(SVT_HIP_ERR_INVALID, "window (%d, %d) %u x %u reaches outside the %d samples of padding", x0, y0, w, h, ME_SP_MARGIN);
    return SVT_HIP_OK;
}
inline uint32_t me_subpel_planes_grid(uint32_t w, uint32_t h) { return (w * h + 255) / 256; }      // one lane per sample of the window

}  // namespace svthost

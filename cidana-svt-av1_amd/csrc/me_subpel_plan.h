// me_subpel_plan.h — what the sub-pel motion estimation calls (svt_hip_me_subpel_frame, svt_hip_motion_estimate_subpel_frame,
// svt_hip_me_subpel_planes) settle on the host before they enqueue: the checks, the padding the interpolation needs, the LDS sizes and
// the grid.  Host only (no HIP header): tests/c/me_subpel_plan_host.cpp compiles it with g++; the kernels (kernel_me_subpel.h) use the same
// constants.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "../../include/svt_hip_dsp.h"
#include "host_err.h"

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

constexpr uint32_t ME_SP_MAX_PICS = 65535;

inline bool me_sp_flag(int32_t v) { return v == 0 || v == 1; }

inline int me_subpel_params_check(const svt_hip_me_subpel_params* s) {
    if (!s) return SVT_HIP_OK;                           // NULL: the reference's setting, everything on
    if (!me_sp_flag(s->fractional_search64x64) || !me_sp_flag(s->enable_half_pel32x32) || !me_sp_flag(s->enable_half_pel16x16) ||
        !me_sp_flag(s->enable_half_pel8x8) || !me_sp_flag(s->enable_quarter_pel))
        return set_err(SVT_HIP_ERR_INVALID, "sub-pel enables must be 0 or 1");
    return SVT_HIP_OK;
}

// what the stage reads of the frame parameters
inline int me_subpel_frame_check(const svt_hip_me_frame_params* P) {
    if (!P) return set_err(SVT_HIP_ERR_INVALID, "NULL parameters");
    if (P->picture_width < 8 || P->picture_height < 8 || (P->picture_width & 7) || (P->picture_height & 7) || P->picture_width > 16384 ||
        P->picture_height > 16384)
        return set_err(SVT_HIP_ERR_INVALID, "picture %d x %d: both sides must be multiples of 8, 8 .. 16384", P->picture_width, P->picture_height);
    if (P->slice_type != SVT_HIP_SLICE_B && P->slice_type != SVT_HIP_SLICE_P) return set_err(SVT_HIP_ERR_INVALID, "slice type %d (B 0 / P 1)", P->slice_type);
    if (P->max_number_of_pus_per_sb != SVT_HIP_ME_PUS && P->max_number_of_pus_per_sb != SVT_HIP_ME_PUS_ALL)
        return set_err(SVT_HIP_ERR_INVALID, "%d PUs per SB (85 or 209)", P->max_number_of_pus_per_sb);
    if (P->fractional_search_method < 0 || P->fractional_search_method > 2)
        return set_err(SVT_HIP_ERR_INVALID, "fractional_search_method %d (SUB_SAD 0, FULL_SAD 1, SSD 2)", P->fractional_search_method);
    if (P->cu8x8_mode < 0) return set_err(SVT_HIP_ERR_INVALID, "negative cu8x8_mode");
    return SVT_HIP_OK;
}

// level 0 of a pyramid: the margin above
inline int me_subpel_plane_check(const svt_hip_me_pyramid* p, const char* what, int32_t width, int32_t height, uint32_t n_pictures) {
    if (!p) return set_err(SVT_HIP_ERR_INVALID, "%s: NULL pyramid", what);
    if (!p->d_plane[0]) return set_err(SVT_HIP_ERR_INVALID, "%s: level 0 plane is NULL", what);
    const uint32_t m = (uint32_t)ME_SP_MARGIN;
    if (p->origin_x[0] < m || p->origin_y[0] < m || p->origin_x[0] > 32767 || p->origin_y[0] > 32767)
        return set_err(SVT_HIP_ERR_INVALID, "%s: origin (%u, %u) below the %u samples of padding the interpolation reads", what, p->origin_x[0], p->origin_y[0], m);
    if ((uint64_t)p->stride[0] < (uint64_t)p->origin_x[0] + (uint32_t)width + m || p->stride[0] > (1u << 20))
        return set_err(SVT_HIP_ERR_INVALID, "%s: stride %u below origin + width + %u", what, p->stride[0], m);
    if (n_pictures > 1 && p->pitch[0] < (uint64_t)p->stride[0] * ((uint64_t)p->origin_y[0] + (uint32_t)height + m))
        return set_err(SVT_HIP_ERR_INVALID, "%s: pitch below one padded picture", what);
    return SVT_HIP_OK;
}

inline int me_subpel_pictures_check(const svt_hip_me_pyramid* src, const svt_hip_me_pyramid* ref0, const svt_hip_me_pyramid* ref1,
                                    const svt_hip_me_frame_params* P, uint32_t n_pictures) {
    if (n_pictures > ME_SP_MAX_PICS) return set_err(SVT_HIP_ERR_INVALID, "%u pictures (at most %u)", n_pictures, ME_SP_MAX_PICS);
    // the source is read inside its SBs only (a partial SB's block reaches 56 samples into the padding): the search's own 64 do
    if (!src) return set_err(SVT_HIP_ERR_INVALID, "source: NULL pyramid");
    if (!src->d_plane[0]) return set_err(SVT_HIP_ERR_INVALID, "source: level 0 plane is NULL");
    if ((uint64_t)src->stride[0] < (uint64_t)src->origin_x[0] + (uint32_t)P->picture_width + 64u || src->stride[0] > (1u << 20) || src->origin_x[0] > 32767 ||
        src->origin_y[0] > 32767)
        return set_err(SVT_HIP_ERR_INVALID, "source: stride %u below origin + width + 64", src->stride[0]);
    if (n_pictures > 1 && src->pitch[0] < (uint64_t)src->stride[0] * ((uint64_t)src->origin_y[0] + (uint32_t)P->picture_height + 64u))
        return set_err(SVT_HIP_ERR_INVALID, "source: pitch below one padded picture");
    if (int rc = me_subpel_plane_check(ref0, "list 0", P->picture_width, P->picture_height, n_pictures)) return rc;
    if (P->slice_type == SVT_HIP_SLICE_B) { if (int rc = me_subpel_plane_check(ref1, "list 1", P->picture_width, P->picture_height, n_pictures)) return rc; }
    else if (ref1) return set_err(SVT_HIP_ERR_INVALID, "a P picture takes no list-1 reference");
    return SVT_HIP_OK;
}

// grid of the refinement: (SB, list, picture); the bi-prediction's: (SB, 1, picture)
inline int me_subpel_grid(const svt_hip_me_frame_params* P, uint32_t n_pictures, uint32_t g[3]) {
    const uint32_t nsbx = (uint32_t)(P->picture_width + 63) / 64, nsby = (uint32_t)(P->picture_height + 63) / 64;
    g[0] = nsbx * nsby; g[1] = P->slice_type == SVT_HIP_SLICE_P ? 1u : 2u; g[2] = n_pictures;
    if (g[0] > 0x7fffffffu / 2) return set_err(SVT_HIP_ERR_INVALID, "too many SBs");
    return SVT_HIP_OK;
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

// svt_hip_me_subpel_planes: the window's samples and the filter's reach must lie inside the padded plane
inline int me_subpel_planes_check(const svt_hip_me_pyramid* ref, int32_t width, int32_t height, int32_t x0, int32_t y0, uint32_t w, uint32_t h,
                                  const uint8_t* d_planes) {
    if (width < 8 || height < 8 || width > 16384 || height > 16384) return set_err(SVT_HIP_ERR_INVALID, "picture %d x %d", width, height);
    if (int rc = me_subpel_plane_check(ref, "reference", width, height, 1)) return rc;
    if (!d_planes) return set_err(SVT_HIP_ERR_INVALID, "NULL d_planes");
    if (w < 1 || h < 1 || w > 4096 || h > 4096) return set_err(SVT_HIP_ERR_INVALID, "window %u x %u (1 .. 4096)", w, h);
    // plane J at (y, x) reads I[y - 2 .. y + 1][x - 2 .. x + 1]
    if (x0 - 2 < -ME_SP_MARGIN || y0 - 2 < -ME_SP_MARGIN || (int64_t)x0 + w + 1 > (int64_t)width + ME_SP_MARGIN || (int64_t)y0 + h + 1 > (int64_t)height + ME_SP_MARGIN)
        return set_err(SVT_HIP_ERR_INVALID, "window (%d, %d) %u x %u reaches outside the %d samples of padding", x0, y0, w, h, ME_SP_MARGIN);
    return SVT_HIP_OK;
}

}  // namespace svthost

// me_plan.h — what the motion-estimation calls settle on the host before they enqueue: the stage calls of svt_hip_pixel.hip
// (svt_hip_hme_level_*, svt_hip_me_setup_batch, svt_hip_me_sb_search_*, svt_hip_me_fullpel_search_*, svt_hip_me_bipred_batch) and the
// whole-picture calls of svt_hip_me_frame.hip / svt_hip_me_subpel.hip.  Every refusal, in the order a caller observes it; the kernel a
// full-pel search is routed to; the grids; the scalars the host derives for the frame kernels (which list takes an HME centre, the
// second-best rule, the clip of the HME levels, the bi-prediction switches).  Each clause that several calls share has one statement here.
// Host only (no HIP header): tests/c/me_plan_host.cpp compiles it with g++.  The windows in LDS are search_plan.h's; the sub-pel stage's
// own checks are me_subpel_plan.h's, which builds on this file.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include "../../include/svt_hip_dsp.h"
#include "host_err.h"
#include "search_plan.h"

namespace svthost {

// ---- clauses that several calls share ------------------------------------------------------------------------------------------------
inline int me_flavour_check(int flavour) {
    if (flavour != SVT_HIP_FLAVOUR_C && flavour != SVT_HIP_FLAVOUR_AVX2) return set_err(SVT_HIP_ERR_INVALID, "flavour %d", flavour);
    return SVT_HIP_OK;
}
// the result rows of a full-pel search: the flavour they follow and room for the 85 or 209 PUs of an SB
inline int me_rows_check(int flavour, int nsq, uint32_t pu_pitch) {
    if (int rc = me_flavour_check(flavour)) return rc;
    const uint32_t npus = nsq ? SVT_HIP_ME_PUS_ALL : SVT_HIP_ME_PUS;
    if (pu_pitch < npus) return set_err(SVT_HIP_ERR_INVALID, "pu_pitch %u < %u PUs", pu_pitch, npus);
    return SVT_HIP_OK;
}
// one workgroup (or one lane group) per item: the count is a 32-bit kernel argument
inline int me_count_check(size_t n, const char* items) {
    if (n > 0x7fffffffu) return set_err(SVT_HIP_ERR_INVALID, "too many %s", items);
    return SVT_HIP_OK;
}
// the region grid of the HME levels and the search area, as svt_hip_me_setup_batch and the frame plan bound them
inline bool me_regions_ok(int rw, int rh) { return rw >= 1 && rw <= 2 && rh >= 1 && rh <= 2; }
inline bool me_search_area_ok(int w, int h) { return w >= 1 && h >= 1 && w <= 4096 && h <= 4096; }

// what every whole-picture call reads first of the frame parameters: the picture and the slice type ...
inline int me_picture_check(const svt_hip_me_frame_params* P) {
    if (!P) return set_err(SVT_HIP_ERR_INVALID, "NULL parameters");
    if (P->picture_width < 8 || P->picture_height < 8 || (P->picture_width & 7) || (P->picture_height & 7) || P->picture_width > 16384 ||
        P->picture_height > 16384)
        return set_err(SVT_HIP_ERR_INVALID, "picture %d x %d: both sides must be multiples of 8, 8 .. 16384", P->picture_width, P->picture_height);
    if (P->slice_type != SVT_HIP_SLICE_B && P->slice_type != SVT_HIP_SLICE_P) return set_err(SVT_HIP_ERR_INVALID, "slice type %d (B 0 / P 1)", P->slice_type);
    return SVT_HIP_OK;
}
// ... and the PU count (the frame plan has clauses of its own between the two, and a caller sees the first that fails)
inline int me_pus_check(const svt_hip_me_frame_params* P) {
    if (P->max_number_of_pus_per_sb != SVT_HIP_ME_PUS && P->max_number_of_pus_per_sb != SVT_HIP_ME_PUS_ALL)
        return set_err(SVT_HIP_ERR_INVALID, "%d PUs per SB (85 or 209)", P->max_number_of_pus_per_sb);
    return SVT_HIP_OK;
}

// lists and SBs of a picture the checks above accepted.  (16384 x 16384 has 65 536 SBs: the bound cannot fail; it is the kernels' 2 * nsb)
struct MeGeom { int nl; uint32_t nsbx, nsby, nsb; };
inline MeGeom me_geom(const svt_hip_me_frame_params& P) {
    MeGeom g;
    g.nl = P.slice_type == SVT_HIP_SLICE_P ? 1 : 2;
    g.nsbx = (uint32_t)(P.picture_width + 63) / 64;
    g.nsby = (uint32_t)(P.picture_height + 63) / 64;
    g.nsb = g.nsbx * g.nsby;
    return g;
}
inline int me_geom_check(const MeGeom& g) {
    if (g.nsb > 0x7fffffffu / 2) return set_err(SVT_HIP_ERR_INVALID, "too many SBs");
    return SVT_HIP_OK;
}

// BiPredictionSearch: every PU when the 8x8 PUs are on or all 209 are searched (else PUs 0 .. 20, EbMotionEstimation.c:8305); its SAD on
// every other row, doubled, under SUB_SAD_SEARCH
struct MeBipredSwitches { int all_pus, sub_sad; };
inline MeBipredSwitches me_bipred_switches(const svt_hip_me_frame_params& P) {
    return MeBipredSwitches{(P.cu8x8_mode == 0 || P.max_number_of_pus_per_sb == SVT_HIP_ME_PUS_ALL) ? 1 : 0, P.fractional_search_method == 0 ? 1 : 0};
}

// ---- a padded plane of a pyramid -----------------------------------------------------------------------------------------------------
// Who reads the plane decides the words of a refusal and whether the padding is needed before the picture too.
struct MePlaneReader { const char* name; bool names_level, near_side; };
constexpr MePlaneReader ME_READ_SEARCH = {"search", true, true};                    // the HME levels and the full-pel search: 64 >> level samples
constexpr MePlaneReader ME_READ_INTERPOLATION = {"interpolation", false, true};     // the sub-pel stage's references (me_subpel_plan.h)
// the sub-pel stage's source: read inside its SBs only, so the padding counts after the picture alone; an origin past 32767 is reported
// with the stride's words
constexpr MePlaneReader ME_READ_BLOCKS = {"", false, false};

// level k of a pyramid holds a width x height picture with `pad` samples of padding round it (after it only: near_side off)
inline int me_plane_check(const svt_hip_me_pyramid* p, int k, uint32_t width, uint32_t height, uint32_t pad, uint32_t n_pictures, const char* what,
                          const MePlaneReader& reader) {
    if (!p) return set_err(SVT_HIP_ERR_INVALID, "%s: NULL pyramid", what);
    if (!p->d_plane[k]) return set_err(SVT_HIP_ERR_INVALID, "%s: level %d plane is NULL", what, k);
    char lv[16] = "";
    if (reader.names_level) snprintf(lv, sizeof(lv), "level %d ", k);
    const bool far_origin = p->origin_x[k] > 32767 || p->origin_y[k] > 32767;
    if (reader.near_side && (p->origin_x[k] < pad || p->origin_y[k] < pad || far_origin))
        return set_err(SVT_HIP_ERR_INVALID, "%s: %sorigin (%u, %u) below the %u samples of padding the %s reads", what, lv, p->origin_x[k], p->origin_y[k], pad,
                       reader.name);
    if ((uint64_t)p->stride[k] < (uint64_t)p->origin_x[k] + width + pad || p->stride[k] > (1u << 20) || far_origin)
        return set_err(SVT_HIP_ERR_INVALID, "%s: %sstride %u below origin + width + %u", what, lv, p->stride[k], pad);
    if (n_pictures > 1 && p->pitch[k] < (uint64_t)p->stride[k] * ((uint64_t)p->origin_y[k] + height + pad))
        return set_err(SVT_HIP_ERR_INVALID, "%s: %spitch below one padded picture", what, lv);
    return SVT_HIP_OK;
}

// sample (0, 0) of level k and the bytes from one picture of a stack to the next (0: a single picture)
struct MePlaneAt { const uint8_t* p; uint32_t stride; uint64_t pitch; };
inline MePlaneAt me_plane_at(const svt_hip_me_pyramid* p, int k, uint32_t n_pictures) {
    return MePlaneAt{p->d_plane[k] + (size_t)p->origin_y[k] * p->stride[k] + p->origin_x[k], p->stride[k], n_pictures > 1 ? p->pitch[k] : 0};
}

// ---- the whole-picture call: svt_hip_motion_estimate_frame / _subpel_frame -----------------------------------------------------------
// HME_LEVEL_0_SEARCH_AREA_MULTIPLIER_X / _Y [hierarchical_levels][temporal_layer_index] (EbDefinitions.h:3019-3035; both tables
// hold the same numbers): percent by which level 0 widens its area in the lower temporal layers
inline uint32_t hme_level0_multiplier(int hierarchical_levels, int temporal_layer) {
    constexpr uint16_t top3[3][4] = {{200, 140, 100, 70}, {350, 200, 100, 100}, {525, 350, 200, 100}};
    if (hierarchical_levels < 3 || temporal_layer > 3) return 100;
    return top3[hierarchical_levels - 3][temporal_layer];
}

constexpr uint32_t ME_FRAME_MAX_PICS = 65535;            // grid.z

struct MeFramePlan {
    int nl, nreg, last_level, nsq;
    int level_on[3];
    uint32_t nsbx, nsby, nsb;
    int max_w, max_h;
    MeWindow search;
    HmeWindow hme_win;
    // [HME level][region r = rh * regions_w + rw]; pad_width / pad_height of levels 0 and 1 are the reference's, set by
    // me_frame_outputs_check once the pictures are known (the scratch size does not depend on them)
    svt_hip_hme_params hme[3][4];
    // what the launches pass that follows from the parameters alone
    int hme_list[2];                 // this list takes an HME centre at all
    int second_best[2];              // ... the second entry of the region sort
    int zz_check;                    // CheckZeroZeroCenter runs
    uint32_t hme_wpitch;             // LDS pitch of the HME window rows (8 with no level on: the kernel divides by nothing, but stages by it)
    int bipred_all, sub_sad;         // me_bipred_switches
};

// the parameter checks that need no picture: everything svt_hip_motion_estimate_frame_scratch_bytes can know
inline int me_frame_plan(const svt_hip_me_frame_params* P, MeFramePlan& pl) {
    if (!P) return set_err(SVT_HIP_ERR_INVALID, "NULL parameters");
    memset(&pl, 0, sizeof(pl));
    if (int rc = me_picture_check(P)) return rc;
    if (P->hierarchical_levels < 0 || P->hierarchical_levels > 5 || P->temporal_layer_index < 0 || P->temporal_layer_index > P->hierarchical_levels)
        return set_err(SVT_HIP_ERR_INVALID, "temporal layer %d of %d hierarchical levels (0 .. 5)", P->temporal_layer_index, P->hierarchical_levels);
    if (int rc = me_flavour_check(P->flavour)) return rc;
    if (int rc = me_pus_check(P)) return rc;
    if (P->nsq_search_level < 0 || P->cu8x8_mode < 0 || P->fractional_search_method < 0)
        return set_err(SVT_HIP_ERR_INVALID, "negative nsq_search_level / cu8x8_mode / fractional_search_method");
    const int rw = P->number_hme_search_region_in_width, rh = P->number_hme_search_region_in_height;
    if (!me_regions_ok(rw, rh)) return set_err(SVT_HIP_ERR_INVALID, "%d x %d HME search regions (1 .. 2 each)", rw, rh);
    if (P->hme_level0_total_search_area_width < 0 || P->hme_level0_total_search_area_height < 0)
        return set_err(SVT_HIP_ERR_INVALID, "negative HME level-0 total search area");
    const MeGeom g = me_geom(*P);
    pl.nl = g.nl; pl.nsbx = g.nsbx; pl.nsby = g.nsby; pl.nsb = g.nsb;
    pl.nsq = P->max_number_of_pus_per_sb == SVT_HIP_ME_PUS_ALL;
    pl.nreg = rw * rh;
    pl.last_level = -1;
    const int on[3] = {P->enable_hme_level0_flag, P->enable_hme_level1_flag, P->enable_hme_level2_flag};
    for (int lv = 0; lv < 3; lv++) {
        pl.level_on[lv] = P->enable_hme_flag && on[lv];
        if (pl.level_on[lv]) pl.last_level = lv;
    }
    // MotionEstimateLcu reads an uninitialised centre there (xHmeSearchCenter, :7946): refused rather than guessed
    if (P->enable_hme_flag && pl.last_level < 0) return set_err(SVT_HIP_ERR_INVALID, "enable_hme_flag with no HME level on");
    if (pl.level_on[0] && P->flavour == SVT_HIP_FLAVOUR_AVX2 && (P->picture_width & 63))
        return set_err(SVT_HIP_ERR_INVALID, "the AVX2 flavour of HME level 0 is undefined on a picture width (%d) that is not a multiple of 64", P->picture_width);
    // list 1 of a picture above the base layer whose references are one picture takes the second entry of the reference's region
    // sort, which walks a square grid only (svt_hip_me_setup_batch)
    const bool same_poc = P->ref_pic_poc[0] == P->ref_pic_poc[1];
    if (pl.nl == 2 && pl.last_level == 2 && same_poc && P->temporal_layer_index > 0 && rw != rh)
        return set_err(SVT_HIP_ERR_INVALID, "same-POC references need number_hme_search_region_in_width == _in_height");
    if (!me_search_area_ok(P->search_area_width, P->search_area_height))
        return set_err(SVT_HIP_ERR_INVALID, "search area %d x %d", P->search_area_width, P->search_area_height);
    pl.max_w = (P->search_area_width + 7) & ~7;
    pl.max_h = P->search_area_height;
    // as svt_hip_me_fullpel_search_areas_batch sizes its window (search_plan.h)
    if (int rc = me_window_check(pl.max_w, pl.max_h, pl.nsq, ME_NSQ_LDS_MAX, pl.search)) return rc;
    const uint32_t mult = hme_level0_multiplier(P->hierarchical_levels, P->temporal_layer_index);
    svt_hip_hme_params all[3 * 4];
    int nall = 0;
    for (int lv = 0; lv < 3; lv++) {
        if (!pl.level_on[lv]) continue;
        const int k = 2 - lv;                             // pyramid level of HME level lv
        for (int i = 0; i < rw; i++)
            if (P->hme_search_area_in_width_array[lv][i] == 0) return set_err(SVT_HIP_ERR_INVALID, "HME level %d: a zero search-area width", lv);
        for (int i = 0; i < rh; i++)
            if (P->hme_search_area_in_height_array[lv][i] == 0) return set_err(SVT_HIP_ERR_INVALID, "HME level %d: a zero search-area height", lv);
        for (int r = 0; r < pl.nreg; r++) {
            // region r = rh * regions_w + rw: the reference's visiting order.  The padding enters as the picture's origin: 1 here, the
            // reference's once the pictures are known
            svt_hip_hme_params& hp = pl.hme[lv][r];
            if (svt_hip_hme_level_params(lv, P->hme_search_area_in_width_array[lv], P->hme_search_area_in_height_array[lv], (uint32_t)(r % rw),
                                         (uint32_t)(r / rw), (uint32_t)P->hme_level0_total_search_area_width,
                                         (uint32_t)P->hme_level0_total_search_area_height, mult, mult, 1, 1, (uint32_t)(P->picture_width >> k),
                                         (uint32_t)(P->picture_height >> k), &hp) != SVT_HIP_OK)
                return set_err(SVT_HIP_ERR_INVALID, "HME level %d parameters", lv);
            if (hp.search_area_width < 1 || hp.search_area_height < 1)
                return set_err(SVT_HIP_ERR_INVALID, "HME level %d region %d: search area %d x %d", lv, r, hp.search_area_width, hp.search_area_height);
            all[nall++] = hp;
        }
    }
    // as svt_hip_hme_level_regions_batch sizes its window, over every level's regions
    if (int rc = hme_window(all, nall, pl.hme_win)) return rc;
    pl.hme_wpitch = pl.hme_win.wpitch ? pl.hme_win.wpitch : 8;
    for (int l = 0; l < 2; l++) {
        // BASE_LAYER_REF (:7656): list 1 of a base-layer picture whose two references are one picture searches round (0, 0)
        pl.hme_list[l] = (P->temporal_layer_index > 0 || l == 0 || !same_poc) ? 1 : 0;
        pl.second_best[l] = (pl.last_level == 2 && same_poc && l == 1) ? 1 : 0;
    }
    pl.zz_check = P->is_used_as_reference_flag ? 1 : 0;
    const MeBipredSwitches b = me_bipred_switches(*P);
    pl.bipred_all = b.all_pus; pl.sub_sad = b.sub_sad;
    return SVT_HIP_OK;
}

// [picture][SB][list][4] search areas
inline size_t me_frame_scratch(const MeFramePlan& pl, uint32_t n_pictures) {
    return ((size_t)n_pictures * pl.nsbx * pl.nsby * pl.nl * 4 * sizeof(int16_t) + 255) & ~(size_t)255;
}

// the stack and the three pyramids: the decimated pictures are read by their HME level only
inline int me_frame_pictures_check(const svt_hip_me_pyramid* src, const svt_hip_me_pyramid* ref0, const svt_hip_me_pyramid* ref1, const svt_hip_me_frame_params* P,
                                   const MeFramePlan& pl, uint32_t n_pictures) {
    if (n_pictures > ME_FRAME_MAX_PICS) return set_err(SVT_HIP_ERR_INVALID, "%u pictures (at most 65535)", n_pictures);
    const svt_hip_me_pyramid* pyr[3] = {src, ref0, ref1};
    static const char* const what[3] = {"source", "list 0", "list 1"};
    for (int i = 0; i < 3; i++) {
        if (i == 2 && pl.nl != 2) {
            if (ref1) return set_err(SVT_HIP_ERR_INVALID, "a P picture takes no list-1 reference");
            break;
        }
        for (int k = 0; k < 3; k++) {
            if (k > 0 && !pl.level_on[2 - k]) continue;
            if (int rc = me_plane_check(pyr[i], k, (uint32_t)P->picture_width >> k, (uint32_t)P->picture_height >> k, 64u >> k, n_pictures, what[i], ME_READ_SEARCH))
                return rc;
        }
    }
    return SVT_HIP_OK;
}

// the rest of the call's clauses; then the clip of HME levels 0 and 1 enters the plan: the reference's padding, origin - 1 (HmeLevel0
// :5729, HmeLevel1 :5905; level 2 clips against BLOCK_SIZE_64 - 1, already set).  One parameter row serves both lists, so their origins
// must agree.
inline int me_frame_outputs_check(const svt_hip_me_pyramid* ref0, const svt_hip_me_pyramid* ref1, MeFramePlan& pl, uint32_t n_pictures, const uint32_t* d_best_sad,
                                  const uint32_t* d_best_mv, const int16_t* d_area_origin, const uint32_t* d_bipred_sad, const svt_hip_me_result* d_results,
                                  const void* d_scratch, size_t scratch_bytes) {
    if (pl.nl == 2)
        for (int lv = 0; lv < 2; lv++)
            if (pl.level_on[lv] && (ref1->origin_x[2 - lv] != ref0->origin_x[2 - lv] || ref1->origin_y[2 - lv] != ref0->origin_y[2 - lv]))
                return set_err(SVT_HIP_ERR_INVALID, "the two references' decimated pictures must have the same origin (it is the HME levels' clip)");
    if (!d_best_sad || !d_best_mv || !d_area_origin || !d_bipred_sad || !d_results) return set_err(SVT_HIP_ERR_INVALID, "NULL output");
    if (((uintptr_t)d_best_sad & 3) || ((uintptr_t)d_best_mv & 3) || ((uintptr_t)d_bipred_sad & 3) || ((uintptr_t)d_results & 3) || ((uintptr_t)d_area_origin & 1))
        return set_err(SVT_HIP_ERR_INVALID, "misaligned output");
    if (!d_scratch || ((uintptr_t)d_scratch & 15) || scratch_bytes < me_frame_scratch(pl, n_pictures ? n_pictures : 1))
        return set_err(SVT_HIP_ERR_INVALID, "scratch NULL, not 16-byte aligned or below svt_hip_motion_estimate_frame_scratch_bytes()");
    if (n_pictures == 0) return SVT_HIP_OK;               // the caller returns here: nothing below can refuse an empty stack
    if (pl.nsb > 0x7fffffffu / 2) return set_err(SVT_HIP_ERR_INVALID, "too many SBs");
    for (int lv = 0; lv < 2; lv++)
        for (int r = 0; r < pl.nreg && pl.level_on[lv]; r++) {
            pl.hme[lv][r].pad_width = (int32_t)ref0->origin_x[2 - lv] - 1;
            pl.hme[lv][r].pad_height = (int32_t)ref0->origin_y[2 - lv] - 1;
        }
    return SVT_HIP_OK;
}

// ---- the stage calls (svt_hip_pixel.hip): every clause after the empty-batch return, in the order a caller observes ------------------
// svt_hip_hme_level_regions_batch: 1 .. 4 search regions of one level, grid (task, region)
struct HmeLevelPlan { HmeWindow win; uint32_t grid_x, grid_y; };
inline int hme_level_plan(HmeLevelPlan& p, const void* d_src_pic, const void* d_ref_pic, const void* d_sb_origin, const void* d_sb_size, int center_shift,
                          const svt_hip_hme_params* params, int nregions, const void* d_best_sad, const void* d_mv, size_t ntasks) {
    p = HmeLevelPlan{};
    if (!d_src_pic || !d_ref_pic || !d_sb_origin || !d_sb_size || !params || !d_best_sad || !d_mv) return set_err(SVT_HIP_ERR_INVALID, "NULL argument");
    if (nregions < 1 || nregions > 4) return set_err(SVT_HIP_ERR_INVALID, "%d search regions (1..4)", nregions);
    if (center_shift < 0 || center_shift > 2) return set_err(SVT_HIP_ERR_INVALID, "centre shift %d", center_shift);
    if (int rc = me_count_check(ntasks, "tasks")) return rc;
    for (int r = 0; r < nregions; r++) {
        const svt_hip_hme_params& P = params[r];
        if (P.search_area_width < 1 || P.search_area_height < 1 || (P.round_down != 8 && P.round_down != 16) || P.mv_shift < 0 || P.mv_shift > 2 ||
            P.ref_width < 1 || P.ref_height < 1)
            return set_err(SVT_HIP_ERR_INVALID, "HME parameters: area %dx%d, round_down %d, mv_shift %d", P.search_area_width, P.search_area_height,
                           P.round_down, P.mv_shift);
    }
    if (int rc = hme_window(params, nregions, p.win)) return rc;
    p.grid_x = (uint32_t)ntasks; p.grid_y = (uint32_t)nregions;
    return SVT_HIP_OK;
}

// svt_hip_me_setup_batch: four tasks (waves) per workgroup
inline int me_setup_plan(uint32_t& grid, const void* d_src_pic, const void* d_ref_pic, const void* d_sb_origin, const void* d_sb_size, const void* d_hme_sad,
                         const void* d_hme_mv, const svt_hip_me_setup_params* params, const void* d_area, size_t ntasks) {
    grid = 0;
    if (!d_src_pic || !d_ref_pic || !d_sb_origin || !d_sb_size || !params || !d_area) return set_err(SVT_HIP_ERR_INVALID, "NULL argument");
    if ((d_hme_sad == nullptr) != (d_hme_mv == nullptr)) return set_err(SVT_HIP_ERR_INVALID, "d_hme_sad and d_hme_mv go together");
    const svt_hip_me_setup_params& P = *params;
    // the frame plan's region grid, or none at all (no HME)
    if (!(me_regions_ok(P.regions_w, P.regions_h) || (P.regions_w == 0 && P.regions_h == 0)))
        return set_err(SVT_HIP_ERR_INVALID, "%d x %d search regions (0 x 0, or 1 .. 2 each)", P.regions_w, P.regions_h);
    // the reference's sort walks its [width][height] arrays through [q / regions_w][q % regions_w]: outside a square grid that reads
    // entries no level has written (stack garbage in the reference) - refused rather than guessed
    if (P.second_best && P.regions_w != P.regions_h) return set_err(SVT_HIP_ERR_INVALID, "second_best needs regions_w == regions_h");
    if (!me_search_area_ok(P.search_area_width, P.search_area_height) || P.picture_width < 1 || P.picture_height < 1 || P.ref_width < 1 || P.ref_height < 1)
        return set_err(SVT_HIP_ERR_INVALID, "search area %d x %d, picture %d x %d", P.search_area_width, P.search_area_height, P.picture_width, P.picture_height);
    if (int rc = me_count_check(ntasks, "tasks")) return rc;
    grid = (uint32_t)((ntasks + 3) / 4);
    return SVT_HIP_OK;
}

// The kernel of a full-pel search over one search_w x search_h area for every block, one workgroup per block:
//   SQ16   me_sb_search16_kernel<masked>: the 85 square PUs, 16 points per lane, any width (a width that is no multiple of 16 masks the tail of
//          each row); the AVX2 flavour only re-labels the 32x32 keys (w8q)
//   NSQ4   me_nsq4_kernel: all 209 PUs, widths where every point takes the reference's eight-point form, 4 points per lane
//   EXACT  me_fullpel_exact_kernel: every other width of the 209-PU search (single-point quirks), any window too large for the LDS of the
//          other two, and everything under the knob (svt_hip_tune me_exact); no window in LDS
// ref_layout: the rows are the reference's (EbMeTierZeroPu order, pu_pitch apart), not svt_hip_me_sb_search_batch's own.
enum MeFullpelKernel { ME_K_SQ16, ME_K_NSQ4, ME_K_EXACT };
struct MeFullpelRoute {
    int kernel, masked, w8q, ref_layout;
    uint32_t grid, pu_pitch;
    MeWindow window;
    size_t lds;                      // dynamic LDS of the launch: the window's, 0 for EXACT
};
inline int me_fullpel_route(int search_w, int search_h, int flavour, int nsq, int me_exact, MeFullpelRoute& r) {
    r = MeFullpelRoute{};
    if (int rc = me_window(search_w, search_h, 0, r.window)) return rc;
    r.ref_layout = 1;
    if (!nsq && !me_exact && r.window.lds <= ME_LDS_MAX) {
        r.kernel = ME_K_SQ16;
        r.masked = (search_w & 15) != 0;
        r.w8q = flavour == SVT_HIP_FLAVOUR_AVX2 ? (search_w & ~7) : 0;
        r.lds = r.window.lds;
    } else if (nsq && !me_exact && (search_w & 7) == 0 && r.window.lds <= ME_NSQ_LDS_MAX) {
        r.kernel = ME_K_NSQ4;
        r.lds = r.window.lds;
    } else {
        r.kernel = ME_K_EXACT;
    }
    return SVT_HIP_OK;
}

// svt_hip_me_sb_search_batch / _planes_batch: SQ16 with the call's own row layout.  (No bound on the block count: it is the grid, and a
// count past 2^32 wraps in the cast as it always has)
inline int me_sb_search_plan(MeFullpelRoute& r, bool need_offs, const void* d_src_offs, const void* d_ref_offs, const void* d_src, const void* d_ref,
                             const void* d_best_sad, const void* d_best_mv, int search_w, int search_h, size_t nblocks) {
    r = MeFullpelRoute{};
    if (int rc = search_offsets_check(need_offs, d_src_offs, d_ref_offs)) return rc;
    if (!d_src || !d_ref || !d_best_sad || !d_best_mv) return set_err(SVT_HIP_ERR_INVALID, "NULL buffer");
    if (int rc = me_window_check(search_w, search_h, 0, ME_LDS_MAX, r.window)) return rc;
    r.kernel = ME_K_SQ16;
    r.masked = (search_w & 15) != 0;
    r.lds = r.window.lds;
    r.grid = (uint32_t)nblocks; r.pu_pitch = SVT_HIP_ME_PUS;
    return SVT_HIP_OK;
}

// svt_hip_me_fullpel_search_batch
inline int me_fullpel_search_plan(MeFullpelRoute& r, const void* d_src, const void* d_ref, const void* d_best_sad, const void* d_best_mv, int search_w,
                                  int search_h, int flavour, int nsq, uint32_t pu_pitch, size_t nblocks, int me_exact) {
    r = MeFullpelRoute{};
    if (!d_src || !d_ref || !d_best_sad || !d_best_mv) return set_err(SVT_HIP_ERR_INVALID, "NULL buffer");
    if (int rc = me_rows_check(flavour, nsq, pu_pitch)) return rc;
    if (int rc = me_fullpel_route(search_w, search_h, flavour, nsq, me_exact, r)) return rc;
    r.grid = (uint32_t)nblocks; r.pu_pitch = pu_pitch;
    return SVT_HIP_OK;
}

// svt_hip_me_fullpel_search_areas_batch: me_fullpel_areas_kernel<nsq>, the window sized by the bound of the areas; nsq: with the
// single-point areas' pairs
struct MeAreasPlan { int nsq; uint32_t grid; MeWindow window; };
inline int me_fullpel_areas_plan(MeAreasPlan& p, const void* d_src, const void* d_ref, const void* d_src_offs, const void* d_ref_offs, const void* d_areas,
                                 const void* d_best_sad, const void* d_best_mv, int max_search_w, int max_search_h, int flavour, int nsq, uint32_t pu_pitch,
                                 size_t nblocks) {
    p = MeAreasPlan{};
    if (!d_src || !d_ref || !d_src_offs || !d_ref_offs || !d_areas || !d_best_sad || !d_best_mv) return set_err(SVT_HIP_ERR_INVALID, "NULL argument");
    if (int rc = me_rows_check(flavour, nsq, pu_pitch)) return rc;
    if (int rc = me_count_check(nblocks, "blocks")) return rc;
    if (int rc = me_window_check(max_search_w, max_search_h, nsq, ME_NSQ_LDS_MAX, p.window)) return rc;
    p.nsq = nsq ? 1 : 0;
    p.grid = (uint32_t)nblocks;
    return SVT_HIP_OK;
}

// svt_hip_me_bipred_batch: one workgroup per SB
struct MeBipredPlan { uint32_t grid; int all_pus, sub_sad; };
inline int me_bipred_plan(MeBipredPlan& p, const void* d_src_pic, const void* d_ref0_pic, const void* d_ref1_pic, const void* d_sb_origin, const void* d_best_sad0,
                          const void* d_best_mv0, const void* d_best_sad1, const void* d_best_mv1, uint32_t pu_pitch, int npus, int bipred_all_pus, int sub_sad,
                          const void* d_results, size_t nsb) {
    p = MeBipredPlan{};
    if (!d_src_pic || !d_sb_origin || !d_best_sad0 || !d_best_mv0 || !d_results) return set_err(SVT_HIP_ERR_INVALID, "NULL argument");
    if ((d_best_sad1 == nullptr) != (d_best_mv1 == nullptr)) return set_err(SVT_HIP_ERR_INVALID, "d_best_sad1 and d_best_mv1 go together");
    if (d_best_sad1 && (!d_ref0_pic || !d_ref1_pic)) return set_err(SVT_HIP_ERR_INVALID, "two lists need both reference planes");
    if (npus != SVT_HIP_ME_PUS && npus != SVT_HIP_ME_PUS_ALL) return set_err(SVT_HIP_ERR_INVALID, "npus %d (85 or 209)", npus);
    if (pu_pitch < (uint32_t)npus) return set_err(SVT_HIP_ERR_INVALID, "pu_pitch %u < %d PUs", pu_pitch, npus);
    if (int rc = me_count_check(nsb, "SBs")) return rc;
    p.grid = (uint32_t)nsb;
    p.all_pus = bipred_all_pus ? 1 : 0; p.sub_sad = sub_sad ? 1 : 0;
    return SVT_HIP_OK;
}

}  // namespace svthost

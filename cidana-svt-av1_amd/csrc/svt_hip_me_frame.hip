// svt_hip_me_frame.hip — svt_hip_motion_estimate_frame: MotionEstimateLcu for every SB of a picture (or of a stack of pictures
// under one parameter set) in three launches (kernel_me_frame.h): prologue (HME levels, best region, CheckZeroZeroCenter, search
// area), full-pel search, bi-prediction + me_results rows.  svt_hip_motion_estimate_subpel_frame: the same with use_subpel_flag = 1 -
// prologue, search, then the two sub-pel launches of svt_hip_me_subpel.hip (refinement, bi-prediction on fractional vectors).
#include "host_common.h"
#include "kernel_me_frame.h"
#include "me_subpel_plan.h"
#include "search_plan.h"

using namespace svtdev;
using namespace svthost;

static_assert(sizeof(svt_hip_me_frame_params) == 116, "svt_hip_me_frame_params layout");
static_assert(sizeof(svt_hip_me_pyramid) == 88, "svt_hip_me_pyramid layout");

// HME_LEVEL_0_SEARCH_AREA_MULTIPLIER_X / _Y [hierarchical_levels][temporal_layer_index] (EbDefinitions.h:3019-3035; both tables
// hold the same numbers): percent by which level 0 widens its area in the lower temporal layers
static uint32_t hme_level0_multiplier(int hierarchical_levels, int temporal_layer) {
    static const uint16_t top3[3][4] = {{200, 140, 100, 70}, {350, 200, 100, 100}, {525, 350, 200, 100}};
    if (hierarchical_levels < 3 || temporal_layer > 3) return 100;
    return top3[hierarchical_levels - 3][temporal_layer];
}

namespace {
struct MeFramePlan {
    int nl, nreg, last_level, nsq;
    int level_on[3];
    uint32_t nsbx, nsby;
    int max_w, max_h;
    MeWindow search;
    HmeWindow hme_win;
    svt_hip_hme_params hme[3][4];
};
}  // namespace

// the parameter checks that need no picture: everything svt_hip_motion_estimate_frame_scratch_bytes can know
static int me_frame_plan(const svt_hip_me_frame_params* P, MeFramePlan& pl) {
    if (!P) return set_err(SVT_HIP_ERR_INVALID, "NULL parameters");
    memset(&pl, 0, sizeof(pl));
    if (P->picture_width < 8 || P->picture_height < 8 || (P->picture_width & 7) || (P->picture_height & 7) || P->picture_width > 16384 ||
        P->picture_height > 16384)
        return set_err(SVT_HIP_ERR_INVALID, "picture %d x %d: both sides must be multiples of 8, 8 .. 16384", P->picture_width, P->picture_height);
    if (P->slice_type != SVT_HIP_SLICE_B && P->slice_type != SVT_HIP_SLICE_P) return set_err(SVT_HIP_ERR_INVALID, "slice type %d (B 0 / P 1)", P->slice_type);
    if (P->hierarchical_levels < 0 || P->hierarchical_levels > 5 || P->temporal_layer_index < 0 || P->temporal_layer_index > P->hierarchical_levels)
        return set_err(SVT_HIP_ERR_INVALID, "temporal layer %d of %d hierarchical levels (0 .. 5)", P->temporal_layer_index, P->hierarchical_levels);
    if (P->flavour != SVT_HIP_FLAVOUR_C && P->flavour != SVT_HIP_FLAVOUR_AVX2) return set_err(SVT_HIP_ERR_INVALID, "flavour %d", P->flavour);
    if (P->max_number_of_pus_per_sb != SVT_HIP_ME_PUS && P->max_number_of_pus_per_sb != SVT_HIP_ME_PUS_ALL)
        return set_err(SVT_HIP_ERR_INVALID, "%d PUs per SB (85 or 209)", P->max_number_of_pus_per_sb);
    if (P->nsq_search_level < 0 || P->cu8x8_mode < 0 || P->fractional_search_method < 0)
        return set_err(SVT_HIP_ERR_INVALID, "negative nsq_search_level / cu8x8_mode / fractional_search_method");
    const int rw = P->number_hme_search_region_in_width, rh = P->number_hme_search_region_in_height;
    if (rw < 1 || rw > 2 || rh < 1 || rh > 2) return set_err(SVT_HIP_ERR_INVALID, "%d x %d HME search regions (1 .. 2 each)", rw, rh);
    if (P->hme_level0_total_search_area_width < 0 || P->hme_level0_total_search_area_height < 0)
        return set_err(SVT_HIP_ERR_INVALID, "negative HME level-0 total search area");
    pl.nl = P->slice_type == SVT_HIP_SLICE_P ? 1 : 2;
    pl.nsq = P->max_number_of_pus_per_sb == SVT_HIP_ME_PUS_ALL;
    pl.nreg = rw * rh;
    pl.nsbx = (uint32_t)(P->picture_width + 63) / 64;
    pl.nsby = (uint32_t)(P->picture_height + 63) / 64;
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
    if (pl.nl == 2 && pl.last_level == 2 && P->ref_pic_poc[0] == P->ref_pic_poc[1] && P->temporal_layer_index > 0 && rw != rh)
        return set_err(SVT_HIP_ERR_INVALID, "same-POC references need number_hme_search_region_in_width == _in_height");
    if (P->search_area_width < 1 || P->search_area_height < 1 || P->search_area_width > 4096 || P->search_area_height > 4096)
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
            // region r = rh * regions_w + rw: the reference's visiting order.  The padding enters as the picture's origin; it is
            // filled in per call (me_frame_hme_pads) since the scratch size does not depend on it
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
    return hme_window(all, nall, pl.hme_win);             // as svt_hip_hme_level_regions_batch sizes its window, over every level's regions
}

static size_t me_frame_scratch(const MeFramePlan& pl, uint32_t n_pictures) {
    return align256((size_t)n_pictures * pl.nsbx * pl.nsby * pl.nl * 4 * sizeof(int16_t));
}

extern "C" size_t svt_hip_motion_estimate_frame_scratch_bytes(const svt_hip_me_frame_params* params, uint32_t n_pictures) {
    MeFramePlan pl;
    if (me_frame_plan(params, pl) != SVT_HIP_OK) return 0;
    return me_frame_scratch(pl, n_pictures ? n_pictures : 1);
}

static int me_pyramid_check(const svt_hip_me_pyramid* p, const char* what, const svt_hip_me_frame_params* P, const MeFramePlan& pl, uint32_t n_pictures) {
    if (!p) return set_err(SVT_HIP_ERR_INVALID, "%s: NULL pyramid", what);
    for (int k = 0; k < 3; k++) {
        const int lv = 2 - k;
        if (k > 0 && !pl.level_on[lv]) continue;          // the decimated pictures are read by their HME level only
        const uint32_t w = (uint32_t)P->picture_width >> k, h = (uint32_t)P->picture_height >> k, pad = 64u >> k;
        if (!p->d_plane[k]) return set_err(SVT_HIP_ERR_INVALID, "%s: level %d plane is NULL", what, k);
        if (p->origin_x[k] < pad || p->origin_y[k] < pad || p->origin_x[k] > 32767 || p->origin_y[k] > 32767)
            return set_err(SVT_HIP_ERR_INVALID, "%s: level %d origin (%u, %u) below the %u samples of padding the search reads", what, k, p->origin_x[k],
                           p->origin_y[k], pad);
        if ((uint64_t)p->stride[k] < (uint64_t)p->origin_x[k] + w + pad || p->stride[k] > (1u << 20))
            return set_err(SVT_HIP_ERR_INVALID, "%s: level %d stride %u below origin + width + %u", what, k, p->stride[k], pad);
        if (n_pictures > 1 && p->pitch[k] < (uint64_t)p->stride[k] * ((uint64_t)p->origin_y[k] + h + pad))
            return set_err(SVT_HIP_ERR_INVALID, "%s: level %d pitch below one padded picture", what, k);
    }
    return SVT_HIP_OK;
}

// Both whole-picture calls: the checks, then the launches.  subpel: use_subpel_flag = 1 - after the search the result rows are refined to
// quarter-pel and the bi-prediction runs on the fractional vectors (svt_hip_me_subpel.hip); sp = its enables (NULL: all on).
static int me_frame_enqueue(const svt_hip_me_pyramid* src, const svt_hip_me_pyramid* ref0, const svt_hip_me_pyramid* ref1, const svt_hip_me_frame_params* params,
                            bool subpel, const svt_hip_me_subpel_params* sp, uint32_t n_pictures, uint32_t* d_best_sad, uint32_t* d_best_mv,
                            int16_t* d_area_origin, uint32_t* d_bipred_sad, svt_hip_me_result* d_results, void* d_scratch, size_t scratch_bytes, void* stream) {
    if (int rc = require_init()) return rc;
    MeFramePlan pl;
    if (int rc = me_frame_plan(params, pl)) return rc;
    const svt_hip_me_frame_params& P = *params;
    if (subpel) {
        if (int rc = me_subpel_frame_check(params)) return rc;
        if (int rc = me_subpel_params_check(sp)) return rc;
    }
    if (n_pictures > 65535) return set_err(SVT_HIP_ERR_INVALID, "%u pictures (at most 65535)", n_pictures);
    if (int rc = me_pyramid_check(src, "source", params, pl, n_pictures)) return rc;
    if (int rc = me_pyramid_check(ref0, "list 0", params, pl, n_pictures)) return rc;
    if (pl.nl == 2) { if (int rc = me_pyramid_check(ref1, "list 1", params, pl, n_pictures)) return rc; }
    else if (ref1) return set_err(SVT_HIP_ERR_INVALID, "a P picture takes no list-1 reference");
    if (subpel) { if (int rc = me_subpel_pictures_check(src, ref0, ref1, params, n_pictures)) return rc; }      // the interpolation's wider padding
    // levels 0 and 1 clip against the reference's padding; one parameter row serves both lists, so their origins must agree
    if (pl.nl == 2)
        for (int lv = 0; lv < 2; lv++)
            if (pl.level_on[lv] && (ref1->origin_x[2 - lv] != ref0->origin_x[2 - lv] || ref1->origin_y[2 - lv] != ref0->origin_y[2 - lv]))
                return set_err(SVT_HIP_ERR_INVALID, "the two references' decimated pictures must have the same origin (it is the HME levels' clip)");
    if (!d_best_sad || !d_best_mv || !d_area_origin || !d_bipred_sad || !d_results) return set_err(SVT_HIP_ERR_INVALID, "NULL output");
    if (((uintptr_t)d_best_sad & 3) || ((uintptr_t)d_best_mv & 3) || ((uintptr_t)d_bipred_sad & 3) || ((uintptr_t)d_results & 3) || ((uintptr_t)d_area_origin & 1))
        return set_err(SVT_HIP_ERR_INVALID, "misaligned output");
    if (!d_scratch || ((uintptr_t)d_scratch & 15) || scratch_bytes < me_frame_scratch(pl, n_pictures ? n_pictures : 1))
        return set_err(SVT_HIP_ERR_INVALID, "scratch NULL, not 16-byte aligned or below svt_hip_motion_estimate_frame_scratch_bytes()");
    if (n_pictures == 0) return SVT_HIP_OK;
    const uint32_t nsb = pl.nsbx * pl.nsby;
    if (nsb > 0x7fffffffu / 2) return set_err(SVT_HIP_ERR_INVALID, "too many SBs");

    MeFrameDev d;
    memset(&d, 0, sizeof(d));
    const svt_hip_me_pyramid* refs[2] = {ref0, pl.nl == 2 ? ref1 : nullptr};
    for (int k = 0; k < 3; k++) {
        if (k > 0 && !pl.level_on[2 - k]) continue;
        d.src[k] = src->d_plane[k] + (size_t)src->origin_y[k] * src->stride[k] + src->origin_x[k];
        d.src_stride[k] = src->stride[k];
        d.src_pitch[k] = n_pictures > 1 ? src->pitch[k] : 0;
        for (int l = 0; l < pl.nl; l++) {
            d.ref[l][k] = refs[l]->d_plane[k] + (size_t)refs[l]->origin_y[k] * refs[l]->stride[k] + refs[l]->origin_x[k];
            d.ref_stride[l][k] = refs[l]->stride[k];
            d.ref_pitch[l][k] = n_pictures > 1 ? refs[l]->pitch[k] : 0;
        }
    }
    static_assert(sizeof(HmeParams) == sizeof(svt_hip_hme_params), "layout");
    for (int lv = 0; lv < 3; lv++)
        for (int r = 0; r < pl.nreg && pl.level_on[lv]; r++) {
            memcpy(&d.hme[lv][r], &pl.hme[lv][r], sizeof(HmeParams));
            // levels 0 and 1 clip against the reference's padding, origin - 1 (HmeLevel0 :5729, HmeLevel1 :5905); level 2 against
            // BLOCK_SIZE_64 - 1, already set.  (Both lists' origins agree: checked above)
            if (lv < 2) { d.hme[lv][r].pad_width = (int32_t)ref0->origin_x[2 - lv] - 1; d.hme[lv][r].pad_height = (int32_t)ref0->origin_y[2 - lv] - 1; }
        }
    d.setup.picture_width = P.picture_width; d.setup.picture_height = P.picture_height;
    d.setup.ref_width = P.picture_width; d.setup.ref_height = P.picture_height;
    d.setup.search_area_width = P.search_area_width; d.setup.search_area_height = P.search_area_height;
    d.setup.regions_w = P.number_hme_search_region_in_width; d.setup.regions_h = P.number_hme_search_region_in_height;
    d.setup.second_best = 0;
    d.setup.zz_check = P.is_used_as_reference_flag ? 1 : 0;
    const bool same_poc = P.ref_pic_poc[0] == P.ref_pic_poc[1];
    for (int l = 0; l < 2; l++) {
        // BASE_LAYER_REF (:7656): list 1 of a base-layer picture whose two references are one picture searches round (0, 0)
        d.hme_list[l] = (P.temporal_layer_index > 0 || l == 0 || !same_poc) ? 1 : 0;
        d.second_best[l] = (pl.last_level == 2 && same_poc && l == 1) ? 1 : 0;
        d.level_on[l] = pl.level_on[l];
    }
    d.level_on[2] = pl.level_on[2];
    d.nreg = pl.nreg; d.last_level = pl.last_level;
    d.nlists = pl.nl; d.npus = P.max_number_of_pus_per_sb;
    d.nsbx = pl.nsbx; d.nsb = nsb;
    d.hme_wpitch = pl.hme_win.wpitch ? pl.hme_win.wpitch : 8;
    d.area = (int16_t*)d_scratch;
    d.area_origin = d_area_origin;
    d.best_sad = d_best_sad; d.best_mv = d_best_mv;

    const hipStream_t s = (hipStream_t)stream;
    const dim3 grid(nsb, (uint32_t)pl.nl, n_pictures);
    hipLaunchKernelGGL(me_frame_prologue_kernel, grid, dim3(ME_THREADS), pl.hme_win.lds, s, d);
    if (int rc = launch_status("me_frame_prologue")) return rc;
    auto* search = pl.nsq ? me_frame_search_kernel<true> : me_frame_search_kernel<false>;
    hipLaunchKernelGGL(search, grid, dim3(ME_THREADS), pl.search.lds, s, d, pl.max_w, pl.max_h, P.flavour, pl.search.wpitch, pl.search.pair_off);
    if (int rc = launch_status("me_frame_search")) return rc;
    if (subpel) {
        if (int rc = me_subpel_enqueue_refine(src, ref0, ref1, params, sp, n_pictures, d_best_sad, d_best_mv, nullptr, nullptr, s)) return rc;
        return me_subpel_enqueue_bipred(src, ref0, ref1, params, n_pictures, d_best_sad, d_best_mv, d_bipred_sad, d_results, s);
    }
    static_assert(sizeof(MeResult) == sizeof(svt_hip_me_result), "layout");
    hipLaunchKernelGGL(me_frame_bipred_kernel, dim3(nsb, 1, n_pictures), dim3(ME_THREADS), 0, s, d, (P.cu8x8_mode == 0 || pl.nsq) ? 1 : 0,
                       P.fractional_search_method == 0 ? 1 : 0, me_pu_map(), d_bipred_sad, reinterpret_cast<MeResult*>(d_results));
    return launch_status("me_frame_bipred");
}

extern "C" int svt_hip_motion_estimate_frame(const svt_hip_me_pyramid* src, const svt_hip_me_pyramid* ref0, const svt_hip_me_pyramid* ref1,
                                             const svt_hip_me_frame_params* params, uint32_t n_pictures, uint32_t* d_best_sad, uint32_t* d_best_mv,
                                             int16_t* d_area_origin, uint32_t* d_bipred_sad, svt_hip_me_result* d_results, void* d_scratch,
                                             size_t scratch_bytes, void* stream) {
    return me_frame_enqueue(src, ref0, ref1, params, false, nullptr, n_pictures, d_best_sad, d_best_mv, d_area_origin, d_bipred_sad, d_results, d_scratch,
                            scratch_bytes, stream);
}

extern "C" size_t svt_hip_motion_estimate_subpel_frame_scratch_bytes(const svt_hip_me_frame_params* params, uint32_t n_pictures) {
    if (me_subpel_frame_check(params) != SVT_HIP_OK) return 0;
    return svt_hip_motion_estimate_frame_scratch_bytes(params, n_pictures);
}

extern "C" int svt_hip_motion_estimate_subpel_frame(const svt_hip_me_pyramid* src, const svt_hip_me_pyramid* ref0, const svt_hip_me_pyramid* ref1,
                                                    const svt_hip_me_frame_params* params, const svt_hip_me_subpel_params* subpel, uint32_t n_pictures,
                                                    uint32_t* d_best_sad, uint32_t* d_best_mv, int16_t* d_area_origin, uint32_t* d_bipred_sad,
                                                    svt_hip_me_result* d_results, void* d_scratch, size_t scratch_bytes, void* stream) {
    return me_frame_enqueue(src, ref0, ref1, params, true, subpel, n_pictures, d_best_sad, d_best_mv, d_area_origin, d_bipred_sad, d_results, d_scratch,
                            scratch_bytes, stream);
}

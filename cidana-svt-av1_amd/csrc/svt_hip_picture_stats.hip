// svt_hip_picture_stats.hip — svt_hip_picture_stats_frame: GatheringPictureStatistics for every SB and every histogram region of a
// picture (or of a stack of pictures under one parameter set) in two launches (kernel_picture_stats.h): SB statistics + histograms,
// then the per-picture sums.
#include "host_common.h"
#include "kernel_picture_stats.h"

using namespace svtdev;
using namespace svthost;

static_assert(sizeof(svt_hip_pic_stats_planes) == 112, "svt_hip_pic_stats_planes layout");
static_assert(sizeof(svt_hip_pic_stats_params) == 20, "svt_hip_pic_stats_params layout");
static_assert(sizeof(svt_hip_pic_stats_out) == 64, "svt_hip_pic_stats_out layout");

extern "C" int svt_hip_picture_stats_frame(const svt_hip_pic_stats_planes* planes, const svt_hip_pic_stats_params* params, uint32_t n_pictures,
                                           const svt_hip_pic_stats_out* out, void* stream) {
    if (int rc = require_init()) return rc;
    if (!planes || !params || !out) return set_err(SVT_HIP_ERR_INVALID, "NULL planes, parameters or outputs");
    const svt_hip_pic_stats_params& P = *params;
    if (P.picture_width < 8 || P.picture_height < 8 || (P.picture_width & 7) || (P.picture_height & 7) || P.picture_width > 16384 ||
        P.picture_height > 16384)
        return set_err(SVT_HIP_ERR_INVALID, "picture %d x %d: both sides must be multiples of 8, 8 .. 16384", P.picture_width, P.picture_height);
    if (P.block_mean_calc_prec != SVT_HIP_BLOCK_MEAN_PREC_FULL && P.block_mean_calc_prec != SVT_HIP_BLOCK_MEAN_PREC_SUB)
        return set_err(SVT_HIP_ERR_INVALID, "block_mean_calc_prec %d (FULL 0 / SUB 1)", P.block_mean_calc_prec);
    const uint32_t w = (uint32_t)P.picture_width, h = (uint32_t)P.picture_height;
    const int rw = P.regions_per_width, rh = P.regions_per_height;
    if (rw < 1 || rw > 4 || rh < 1 || rh > 4) return set_err(SVT_HIP_ERR_INVALID, "%d x %d regions (1 .. 4 each)", rw, rh);
    // a region of the 1/16 picture with no sample: the reference divides by its area (:4191)
    if ((w >> 2) < (uint32_t)rw || (h >> 2) < (uint32_t)rh)
        return set_err(SVT_HIP_ERR_INVALID, "%d x %d regions on a 1/16 picture of %u x %u: a region would be empty", rw, rh, w >> 2, h >> 2);
    if (n_pictures > 65535) return set_err(SVT_HIP_ERR_INVALID, "%u pictures (at most 65535)", n_pictures);

    const svt_hip_pic_stats_planes& L = *planes;
    static const char* const kName[4] = {"luma", "Cb", "Cr", "1/16 luma"};
    for (int k = 0; k < 4; k++) {
        if (!L.d_plane[k]) return set_err(SVT_HIP_ERR_INVALID, "%s plane is NULL", kName[k]);
        if (L.origin_x[k] > 32767 || L.origin_y[k] > 32767 || L.stride[k] > (1u << 20)) return set_err(SVT_HIP_ERR_INVALID, "%s: origin or stride out of range", kName[k]);
    }
    const uint32_t ox = L.origin_x[0], oy = L.origin_y[0];
    // partial SBs read their full 64x64 from the padding (ComputeBlockMeanComputeVariance has no picture bound)
    if (ox < 64 || oy < 64 || (uint64_t)L.stride[0] < (uint64_t)ox + w + 64)
        return set_err(SVT_HIP_ERR_INVALID, "luma: origin (%u, %u) / stride %u leave less than 64 samples of padding", ox, oy, L.stride[0]);
    for (int k = 1; k < 3; k++) {
        if (L.origin_x[k] != ox >> 1 || L.origin_y[k] != oy >> 1)
            return set_err(SVT_HIP_ERR_INVALID, "%s: origin (%u, %u) is not the luma origin >> 1", kName[k], L.origin_x[k], L.origin_y[k]);
        if ((uint64_t)L.stride[k] < (uint64_t)(ox >> 1) + (w >> 1)) return set_err(SVT_HIP_ERR_INVALID, "%s: stride %u below origin + width", kName[k], L.stride[k]);
    }
    if ((uint64_t)L.stride[3] < (uint64_t)L.origin_x[3] + (w >> 2)) return set_err(SVT_HIP_ERR_INVALID, "1/16 luma: stride %u below origin + width", L.stride[3]);
    if (n_pictures > 1) {
        const uint64_t rows[4] = {(uint64_t)oy + h + 64, (uint64_t)(oy >> 1) + (h >> 1), (uint64_t)(oy >> 1) + (h >> 1), (uint64_t)L.origin_y[3] + (h >> 2)};
        for (int k = 0; k < 4; k++)
            if (L.pitch[k] < (uint64_t)L.stride[k] * rows[k]) return set_err(SVT_HIP_ERR_INVALID, "%s: pitch below one picture", kName[k]);
    }
    const svt_hip_pic_stats_out& O = *out;
    if (!O.d_y_mean || !O.d_variance || !O.d_cb_mean || !O.d_cr_mean || !O.d_pic_avg_variance || !O.d_histogram || !O.d_avg_intensity_region ||
        !O.d_avg_intensity)
        return set_err(SVT_HIP_ERR_INVALID, "NULL output");
    if (((uintptr_t)O.d_variance & 1) || ((uintptr_t)O.d_pic_avg_variance & 1) || ((uintptr_t)O.d_histogram & 3)) return set_err(SVT_HIP_ERR_INVALID, "misaligned output");
    if (n_pictures == 0) return SVT_HIP_OK;

    PicStatsDev d;
    memset(&d, 0, sizeof(d));
    for (int k = 0; k < 4; k++) {
        d.plane[k] = L.d_plane[k];
        d.stride[k] = L.stride[k];
        d.pitch[k] = n_pictures > 1 ? L.pitch[k] : 0;
    }
    d.ox = ox; d.oy = oy; d.ox16 = L.origin_x[3]; d.oy16 = L.origin_y[3];
    d.width = w; d.height = h;
    d.nsbx = (w + 63) / 64; d.nsb = d.nsbx * ((h + 63) / 64);
    d.rw = (uint32_t)rw; d.rh = (uint32_t)rh; d.nhist = (uint32_t)(rw * rh * 3);
    d.sub = P.block_mean_calc_prec == SVT_HIP_BLOCK_MEAN_PREC_SUB;
    d.y_mean = O.d_y_mean; d.variance = O.d_variance; d.cb_mean = O.d_cb_mean; d.cr_mean = O.d_cr_mean;
    d.pic_avg_variance = O.d_pic_avg_variance; d.histogram = O.d_histogram; d.avg_region = O.d_avg_intensity_region; d.avg = O.d_avg_intensity;

    const hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(picture_stats_kernel, dim3(d.nhist + (d.nsb + PST_SBS - 1) / PST_SBS, n_pictures), dim3(PST_THREADS), 0, s, d);
    if (int rc = launch_status("picture_stats")) return rc;
    hipLaunchKernelGGL(picture_stats_sum_kernel, dim3(n_pictures), dim3(PST_THREADS), 0, s, d);
    return launch_status("picture_stats_sum");
}

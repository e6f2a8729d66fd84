/* ref_warp.c - harness round the reference's warped motion, for tests/golden/make_golden_warp.py.  Own glue only: it is compiled next to
 * the reference's Codec/EbWarpedMotion.c (where that file lies) into oracle/_ref/libsvtref_warp.so; select_samples and the block-size
 * tables resolve against oracle/_ref/libsvtref.so.
 *
 *   ref_warp_table  warped_filter[193][8]
 *   ref_warp_fit    warped_motion_parameters (EbAdaptiveMotionVectorPrediction.c:1876-1937) from the point where the samples exist:
 *                   select_samples when there is more than one, then find_projection, on a zeroed EbWarpedMotionParams
 *   ref_warp_pred   one plane of warped_motion_prediction (EbInterPrediction.c:2584): av1_warp_plane at 8 bit, av1_warp_plane_hbd
 *                   above, with get_conv_params_no_round(0, 0, 0, NULL, 128, 0, bd) */
#include <string.h>

#include "EbWarpedMotion.h"
#include "EbAdaptiveMotionVectorPrediction.h"

int select_samples(MV *mv, int *pts, int *pts_inref, int len, block_size bsize);

void ref_warp_table(int16_t *out) { memcpy(out, warped_filter, sizeof(int16_t) * (WARPEDPIXEL_PREC_SHIFTS * 3 + 1) * 8); }

/* out[0] = the sample count find_projection saw (*num_samples), out[1] = find_projection's return value (-1: not called, no samples),
 * out[2..7] = wmmat[0..5], out[8..11] = alpha, beta, gamma, delta.  pts / pts_inref are left as select_samples left them. */
void ref_warp_fit(int nsamples, int *pts, int *pts_inref, int bsize, int mv_x, int mv_y, int mi_row, int mi_col, int32_t *out) {
    EbWarpedMotionParams wm;
    memset(&wm, 0, sizeof(wm));
    memset(out, 0, 12 * sizeof(int32_t));
    out[1] = -1;
    if (nsamples == 0) return;
    MV mv;
    mv.col = (int16_t)mv_x;
    mv.row = (int16_t)mv_y;
    if (nsamples > 1) nsamples = select_samples(&mv, pts, pts_inref, nsamples, (block_size)bsize);
    out[0] = nsamples;
    out[1] = find_projection(nsamples, pts, pts_inref, (block_size)bsize, mv.row, mv.col, &wm, mi_row, mi_col);
    for (int i = 0; i < 6; i++) out[2 + i] = wm.wmmat[i];
    out[8] = wm.alpha; out[9] = wm.beta; out[10] = wm.gamma; out[11] = wm.delta;
}

/* get_shear_params on wmmat = mat[0..5]: returns its return value (1: allowed), shear = alpha, beta, gamma, delta */
int ref_warp_shear(const int32_t *mat, int16_t *shear) {
    EbWarpedMotionParams wm;
    memset(&wm, 0, sizeof(wm));
    wm.wmtype = AFFINE;
    for (int i = 0; i < 6; i++) wm.wmmat[i] = mat[i];
    const int ok = get_shear_params(&wm);
    shear[0] = wm.alpha; shear[1] = wm.beta; shear[2] = wm.gamma; shear[3] = wm.delta;
    return ok;
}

void ref_warp_pred(int bd, const void *ref, int width, int height, int stride, void *pred, int p_col, int p_row, int p_width, int p_height,
                   int p_stride, int ss, const int32_t *mat, const int16_t *shear) {
    EbWarpedMotionParams wm;
    memset(&wm, 0, sizeof(wm));
    wm.wmtype = AFFINE;
    for (int i = 0; i < 6; i++) wm.wmmat[i] = mat[i];
    wm.alpha = shear[0]; wm.beta = shear[1]; wm.gamma = shear[2]; wm.delta = shear[3];
    ConvolveParams cp = get_conv_params_no_round(0, 0, 0, NULL, 128, 0, bd);
    if (bd == 8)
        av1_warp_plane(&wm, 0, bd, (const uint8_t *)ref, width, height, stride, (uint8_t *)pred, p_col, p_row, p_width, p_height, p_stride, ss, ss, &cp);
    else
        av1_warp_plane_hbd(&wm, bd, (const uint16_t *)ref, width, height, stride, (uint16_t *)pred, p_col, p_row, p_width, p_height, p_stride, ss,
                           ss, &cp);
}

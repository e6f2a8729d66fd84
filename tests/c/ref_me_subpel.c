/*
 * tests/c/ref_me_subpel.c — the project's harness around the reference's own sub-pel motion estimation (EbMotionEstimation.c):
 * InterpolateSearchRegionAVC (:3409), HalfPelSearch_LCU (:3829), QuarterPelSearch_LCU (:4746) and MotionEstimateLcu (:7527) with
 * use_subpel_flag = 1.  TEST INFRASTRUCTURE ONLY: tests/golden/make_golden_me_subpel.py compiles it, next to the reference's
 * EbAvcStyleMcp sources, into oracle/_ref/libsvtref_me_subpel.so.
 *
 * The drivers are `static` in the reference, so this translation unit compiles the reference source where it lies (#include of the
 * .c file, as oracle/ref_me.c does) and calls them as they are.  Nothing of the reference is re-implemented: the contexts are the
 * reference's own structs, zero-allocated, with the fields the functions read filled as MotionEstimateLcu (:8040-8236) and the ME
 * context constructor (EbMotionEstimationContext.c:48-117) fill them - real pos_b / pos_h / pos_j planes, avctemp_buffer, the two
 * one_d_intermediate_results buffers and interpolated_stride = MAX_SEARCH_AREA_WIDTH.
 */
#include "EbMotionEstimation.c"
#include "EbSequenceControlSet.h"
#include "EbReferenceObject.h"

#define SP_ROWS 160                                  /* rows of a sub-pel plane: search areas up to 64 high (64 + 63 + ME_FILTER_TAP + 1) */

static int sp_alloc_planes(MeContext_t *c, int nlists) {
    const uint32_t istride = MAX_SEARCH_AREA_WIDTH;
    c->interpolated_stride = istride;
    for (int l = 0; l < nlists; l++) {
        c->pos_b_buffer[l][0] = (uint8_t *)calloc((size_t)istride * SP_ROWS, 1);
        c->pos_h_buffer[l][0] = (uint8_t *)calloc((size_t)istride * SP_ROWS, 1);
        c->pos_j_buffer[l][0] = (uint8_t *)calloc((size_t)istride * SP_ROWS, 1);
        if (!c->pos_b_buffer[l][0] || !c->pos_h_buffer[l][0] || !c->pos_j_buffer[l][0]) return -1;
    }
    c->avctemp_buffer = (uint8_t *)calloc((size_t)istride * SP_ROWS, 1);
    if (posix_memalign((void **)&c->one_d_intermediate_results_buf0, 64, 64 * 64) || posix_memalign((void **)&c->one_d_intermediate_results_buf1, 64, 64 * 64) ||
        !c->avctemp_buffer)
        return -1;
    memset(c->one_d_intermediate_results_buf0, 0, 64 * 64);
    memset(c->one_d_intermediate_results_buf1, 0, 64 * 64);
    return 0;
}
static void sp_free_planes(MeContext_t *c, int nlists) {
    for (int l = 0; l < nlists; l++) { free(c->pos_b_buffer[l][0]); free(c->pos_h_buffer[l][0]); free(c->pos_j_buffer[l][0]); }
    free(c->avctemp_buffer); free(c->one_d_intermediate_results_buf0); free(c->one_d_intermediate_results_buf1);
}

/* the result pointers of one list as MotionEstimateLcu sets them (:8065-8143) */
static void sp_point_rows(MeContext_t *c, uint32_t li) {
    uint32_t *S = c->p_sb_best_sad[li][0], *M = c->p_sb_best_mv[li][0], *D = c->p_sb_best_ssd[li][0];
    c->p_best_sad64x64 = &S[ME_TIER_ZERO_PU_64x64];   c->p_best_mv64x64 = &M[ME_TIER_ZERO_PU_64x64];   c->p_best_ssd64x64 = &D[ME_TIER_ZERO_PU_64x64];
    c->p_best_sad32x32 = &S[ME_TIER_ZERO_PU_32x32_0]; c->p_best_mv32x32 = &M[ME_TIER_ZERO_PU_32x32_0]; c->p_best_ssd32x32 = &D[ME_TIER_ZERO_PU_32x32_0];
    c->p_best_sad16x16 = &S[ME_TIER_ZERO_PU_16x16_0]; c->p_best_mv16x16 = &M[ME_TIER_ZERO_PU_16x16_0]; c->p_best_ssd16x16 = &D[ME_TIER_ZERO_PU_16x16_0];
    c->p_best_sad8x8 = &S[ME_TIER_ZERO_PU_8x8_0];     c->p_best_mv8x8 = &M[ME_TIER_ZERO_PU_8x8_0];     c->p_best_ssd8x8 = &D[ME_TIER_ZERO_PU_8x8_0];
    c->p_best_sad64x32 = &S[ME_TIER_ZERO_PU_64x32_0]; c->p_best_mv64x32 = &M[ME_TIER_ZERO_PU_64x32_0]; c->p_best_ssd64x32 = &D[ME_TIER_ZERO_PU_64x32_0];
    c->p_best_sad32x16 = &S[ME_TIER_ZERO_PU_32x16_0]; c->p_best_mv32x16 = &M[ME_TIER_ZERO_PU_32x16_0]; c->p_best_ssd32x16 = &D[ME_TIER_ZERO_PU_32x16_0];
    c->p_best_sad16x8 = &S[ME_TIER_ZERO_PU_16x8_0];   c->p_best_mv16x8 = &M[ME_TIER_ZERO_PU_16x8_0];   c->p_best_ssd16x8 = &D[ME_TIER_ZERO_PU_16x8_0];
    c->p_best_sad32x64 = &S[ME_TIER_ZERO_PU_32x64_0]; c->p_best_mv32x64 = &M[ME_TIER_ZERO_PU_32x64_0]; c->p_best_ssd32x64 = &D[ME_TIER_ZERO_PU_32x64_0];
    c->p_best_sad16x32 = &S[ME_TIER_ZERO_PU_16x32_0]; c->p_best_mv16x32 = &M[ME_TIER_ZERO_PU_16x32_0]; c->p_best_ssd16x32 = &D[ME_TIER_ZERO_PU_16x32_0];
    c->p_best_sad8x16 = &S[ME_TIER_ZERO_PU_8x16_0];   c->p_best_mv8x16 = &M[ME_TIER_ZERO_PU_8x16_0];   c->p_best_ssd8x16 = &D[ME_TIER_ZERO_PU_8x16_0];
    c->p_best_sad32x8 = &S[ME_TIER_ZERO_PU_32x8_0];   c->p_best_mv32x8 = &M[ME_TIER_ZERO_PU_32x8_0];   c->p_best_ssd32x8 = &D[ME_TIER_ZERO_PU_32x8_0];
    c->p_best_sad8x32 = &S[ME_TIER_ZERO_PU_8x32_0];   c->p_best_mv8x32 = &M[ME_TIER_ZERO_PU_8x32_0];   c->p_best_ssd8x32 = &D[ME_TIER_ZERO_PU_8x32_0];
    c->p_best_sad64x16 = &S[ME_TIER_ZERO_PU_64x16_0]; c->p_best_mv64x16 = &M[ME_TIER_ZERO_PU_64x16_0]; c->p_best_ssd64x16 = &D[ME_TIER_ZERO_PU_64x16_0];
    c->p_best_sad16x64 = &S[ME_TIER_ZERO_PU_16x64_0]; c->p_best_mv16x64 = &M[ME_TIER_ZERO_PU_16x64_0]; c->p_best_ssd16x64 = &D[ME_TIER_ZERO_PU_16x64_0];
}

/* the half-pel directions in the order of the result rows (EbMeTierZeroPu) */
static void sp_directions(const MeContext_t *c, uint8_t *dir) {
    memset(dir, 0, MAX_ME_PU_COUNT);
    dir[ME_TIER_ZERO_PU_64x64] = c->psub_pel_direction64x64;
    memcpy(dir + ME_TIER_ZERO_PU_32x32_0, c->psub_pel_direction32x32, 4);
    memcpy(dir + ME_TIER_ZERO_PU_16x16_0, c->psub_pel_direction16x16, 16);
    memcpy(dir + ME_TIER_ZERO_PU_8x8_0, c->psub_pel_direction8x8, 64);
    memcpy(dir + ME_TIER_ZERO_PU_64x32_0, c->psub_pel_direction64x32, 2);
    memcpy(dir + ME_TIER_ZERO_PU_32x16_0, c->psub_pel_direction32x16, 8);
    memcpy(dir + ME_TIER_ZERO_PU_16x8_0, c->psub_pel_direction16x8, 32);
    memcpy(dir + ME_TIER_ZERO_PU_32x64_0, c->psub_pel_direction32x64, 2);
    memcpy(dir + ME_TIER_ZERO_PU_16x32_0, c->psub_pel_direction16x32, 8);
    memcpy(dir + ME_TIER_ZERO_PU_8x16_0, c->psub_pel_direction8x16, 32);
    memcpy(dir + ME_TIER_ZERO_PU_32x8_0, c->psub_pel_direction32x8, 16);
    memcpy(dir + ME_TIER_ZERO_PU_8x32_0, c->psub_pel_direction8x32, 16);
    memcpy(dir + ME_TIER_ZERO_PU_64x16_0, c->psub_pel_direction64x16, 4);
    memcpy(dir + ME_TIER_ZERO_PU_16x64_0, c->psub_pel_direction16x64, 4);
}

/* ---- the refinement of one SB against one reference, stage by stage ------------------------------------------------------------
 * src: the SB's top-left source sample inside its (padded) picture; ref0: the co-located sample of the (padded) reference.
 * flg[]: 0 fractionalSearchMethod 1 fractional_search64x64 2 / 3 / 4 enableHalfPel32x32 / 16x16 / 8x8 5 enableQuarterPel
 *        6 disable8x8CuInMeFlag 7 209 PUs (pic_depth_mode <= PIC_ALL_C_DEPTH_MODE) 8 asm_type
 * best_sad / best_mv: [209] in, the full-pel search's rows.  Outputs: half_* after HalfPelSearch_LCU alone, quarter_* after
 * QuarterPelSearch_LCU (each [209]; dir uint8).  planes (may be NULL): [3][plane_h][plane_w] = pos_b / pos_h / pos_j as the call site
 * hands them on (:8194-8201: pos_b + 2 * stride, pos_h + 1, pos_j), entry [r][c] belonging to search point (c, r). */
int ref_me_subpel_stage(const uint8_t *src, uint32_t src_stride, const uint8_t *ref0, uint32_t ref_stride, int xo, int yo, int saw, int sah,
                        const int32_t *flg, const uint32_t *best_sad, const uint32_t *best_mv, uint32_t *half_sad, uint32_t *half_mv,
                        uint32_t *half_ssd, uint8_t *half_dir, uint32_t *quarter_sad, uint32_t *quarter_mv, uint32_t *quarter_ssd,
                        uint8_t *planes, int plane_w, int plane_h) {
    MeContext_t *c = (MeContext_t *)calloc(1, sizeof(MeContext_t));
    PictureParentControlSet_t *pcs = (PictureParentControlSet_t *)calloc(1, sizeof(PictureParentControlSet_t));
    SequenceControlSet *scs = (SequenceControlSet *)calloc(1, sizeof(SequenceControlSet));
    EncodeContext_t *ectx = (EncodeContext_t *)calloc(1, sizeof(EncodeContext_t));
    uint8_t *sb = NULL;
    if (!c || !pcs || !scs || !ectx || sp_alloc_planes(c, 1) || posix_memalign((void **)&sb, 64, 64 * 64)) return -1;
    if (sah + 63 + ME_FILTER_TAP + 1 > SP_ROWS) return -3;
    const uint32_t li = 0;
    const EbAsm asm_type = (EbAsm)flg[8];
    scs->encode_context_ptr = ectx;
    pcs->pic_depth_mode = flg[7] ? 0 : 2;
    c->fractionalSearchMethod = (uint8_t)flg[0];
    c->fractional_search64x64 = (EbBool)flg[1];
    for (int r = 0; r < 64; r++) memcpy(sb + 64 * r, src + (size_t)r * src_stride, 64);
    c->sb_buffer = sb; c->sb_buffer_stride = 64;
    c->sb_src_ptr = (uint8_t *)src; c->sb_src_stride = src_stride;
    const uint8_t *area = ref0 + (ptrdiff_t)yo * (ptrdiff_t)ref_stride + xo;
    c->integer_buffer_ptr[li][0] = (uint8_t *)area - (ME_FILTER_TAP >> 1) - (ME_FILTER_TAP >> 1) * (ptrdiff_t)ref_stride;
    c->interpolated_full_stride[li][0] = ref_stride;
    memcpy(c->p_sb_best_sad[li][0], best_sad, sizeof(uint32_t) * MAX_ME_PU_COUNT);
    memcpy(c->p_sb_best_mv[li][0], best_mv, sizeof(uint32_t) * MAX_ME_PU_COUNT);
    sp_point_rows(c, li);
    uint8_t *full = c->integer_buffer_ptr[li][0] + (ME_FILTER_TAP >> 1) + ((ME_FILTER_TAP >> 1) * c->interpolated_full_stride[li][0]);
    uint8_t *pb = &(c->pos_b_buffer[li][0][(ME_FILTER_TAP >> 1) * c->interpolated_stride]);
    uint8_t *ph = &(c->pos_h_buffer[li][0][1]);
    uint8_t *pj = &(c->pos_j_buffer[li][0][0]);
    InterpolateSearchRegionAVC(c, li, full, c->interpolated_full_stride[li][0], (uint32_t)saw + (BLOCK_SIZE_64 - 1), (uint32_t)sah + (BLOCK_SIZE_64 - 1), 8, asm_type);
    if (planes)
        for (int r = 0; r < plane_h; r++) {
            memcpy(planes + ((size_t)0 * plane_h + r) * plane_w, pb + (size_t)r * c->interpolated_stride, plane_w);
            memcpy(planes + ((size_t)1 * plane_h + r) * plane_w, ph + (size_t)r * c->interpolated_stride, plane_w);
            memcpy(planes + ((size_t)2 * plane_h + r) * plane_w, pj + (size_t)r * c->interpolated_stride, plane_w);
        }
    HalfPelSearch_LCU(scs, pcs, c, full, c->interpolated_full_stride[li][0], pb, ph, pj, (int16_t)xo, (int16_t)yo, asm_type, (EbBool)flg[6],
                      (EbBool)flg[2], (EbBool)flg[3], (EbBool)flg[4]);
    memcpy(half_sad, c->p_sb_best_sad[li][0], sizeof(uint32_t) * MAX_ME_PU_COUNT);
    memcpy(half_mv, c->p_sb_best_mv[li][0], sizeof(uint32_t) * MAX_ME_PU_COUNT);
    memcpy(half_ssd, c->p_sb_best_ssd[li][0], sizeof(uint32_t) * MAX_ME_PU_COUNT);
    sp_directions(c, half_dir);
    QuarterPelSearch_LCU(c, full, c->interpolated_full_stride[li][0], pb, ph, pj, (int16_t)xo, (int16_t)yo, asm_type, (EbBool)flg[6], (EbBool)flg[5],
                         (EbBool)(flg[7] != 0));
    memcpy(quarter_sad, c->p_sb_best_sad[li][0], sizeof(uint32_t) * MAX_ME_PU_COUNT);
    memcpy(quarter_mv, c->p_sb_best_mv[li][0], sizeof(uint32_t) * MAX_ME_PU_COUNT);
    memcpy(quarter_ssd, c->p_sb_best_ssd[li][0], sizeof(uint32_t) * MAX_ME_PU_COUNT);
    sp_free_planes(c, 1);
    free(sb); free(ectx); free(scs); free(pcs); free(c);
    return 0;
}

/* ---- MotionEstimateLcu whole with use_subpel_flag = 1: the parameter block, the buffers and the outputs of oracle/ref_me.c's
 * ref_motion_estimate_lcu (which documents the slots), plus best_ssd [2][209] --------------------------------------------------------- */
int ref_me_subpel_lcu(const int32_t *prm, uint8_t *const *bufs, uint32_t *best_sad, uint32_t *best_mv, int16_t *area_origin, uint32_t *bipred_sad,
                      int32_t *results, uint32_t *best_ssd) {
    PictureParentControlSet_t *pcs = (PictureParentControlSet_t *)calloc(1, sizeof(PictureParentControlSet_t));
    SequenceControlSet *scs = (SequenceControlSet *)calloc(1, sizeof(SequenceControlSet));
    EncodeContext_t *ectx = (EncodeContext_t *)calloc(1, sizeof(EncodeContext_t));
    MeContext_t *c = (MeContext_t *)calloc(1, sizeof(MeContext_t));
    EbObjectWrapper *w = (EbObjectWrapper *)calloc(3, sizeof(EbObjectWrapper));
    EbPaReferenceObject *ro = (EbPaReferenceObject *)calloc(2, sizeof(EbPaReferenceObject));
    EbPictureBufferDesc_t *pic = (EbPictureBufferDesc_t *)calloc(9, sizeof(EbPictureBufferDesc_t));
    MeCuResults_t *mer = (MeCuResults_t *)calloc(MAX_ME_PU_COUNT, sizeof(MeCuResults_t));
    MeCuResults_t *mer_rows[1] = {mer};
    uint16_t *eight = NULL;
    uint8_t *sb = NULL;
    if (!pcs || !scs || !ectx || !c || !w || !ro || !pic || !mer || posix_memalign((void **)&eight, 64, sizeof(uint16_t) * 8 * 16) ||
        posix_memalign((void **)&sb, 64, 64 * 64 + 32 * 32 + 16 * 16) || sp_alloc_planes(c, 2))
        return -1;
    if (prm[14] + 63 + ME_FILTER_TAP + 1 > SP_ROWS) return -3;
    for (int k = 0; k < 9; k++) {                       /* k = 3 * picture (src, ref0, ref1) + level (full, 1/4, 1/16) */
        const int32_t *g = prm + 27 + 5 * (k % 3);
        pic[k].buffer_y = bufs[k];
        pic[k].stride_y = (uint16_t)g[0]; pic[k].origin_x = (uint16_t)g[1]; pic[k].origin_y = (uint16_t)g[2];
        pic[k].width = (uint16_t)g[3]; pic[k].height = (uint16_t)g[4];
    }
    for (int l = 0; l < 2; l++) {
        ro[l].input_padded_picture_ptr = &pic[3 * (l + 1)];
        ro[l].quarter_decimated_picture_ptr = &pic[3 * (l + 1) + 1];
        ro[l].sixteenth_decimated_picture_ptr = &pic[3 * (l + 1) + 2];
        w[l].object_ptr = &ro[l];
        pcs->ref_pa_pic_ptr_array[l] = &w[l];
        pcs->ref_pic_poc_array[l] = (uint64_t)prm[19 + l];
    }
    scs->luma_width = (uint16_t)prm[0]; scs->luma_height = (uint16_t)prm[1];
    scs->input_resolution = (uint8_t)prm[22];
    scs->encode_context_ptr = ectx;
    ectx->asm_type = (EbAsm)prm[21];
    w[2].object_ptr = scs;
    pcs->sequence_control_set_wrapper_ptr = &w[2];
    pcs->slice_type = (EB_SLICE)prm[4];
    pcs->pic_depth_mode = (uint8_t)prm[5];
    pcs->temporal_layer_index = (uint8_t)prm[6];
    pcs->hierarchical_levels = (uint8_t)prm[7];
    pcs->enable_hme_flag = (EbBool)prm[8];
    pcs->enable_hme_level0_flag = (EbBool)prm[9]; pcs->enable_hme_level1_flag = (EbBool)prm[10]; pcs->enable_hme_level2_flag = (EbBool)prm[11];
    pcs->is_used_as_reference_flag = (EbBool)prm[12];
    pcs->use_subpel_flag = 1;
    pcs->cu8x8_mode = (uint8_t)prm[23];
    pcs->max_number_of_pus_per_sb = (uint16_t)prm[25];
    pcs->nsq_search_level = (uint8_t)prm[26];
    pcs->me_results = mer_rows;
    c->search_area_width = (uint16_t)prm[13]; c->search_area_height = (uint16_t)prm[14];
    c->number_hme_search_region_in_width = (uint16_t)prm[15]; c->number_hme_search_region_in_height = (uint16_t)prm[16];
    c->hme_level0_total_search_area_width = (uint16_t)prm[17]; c->hme_level0_total_search_area_height = (uint16_t)prm[18];
    for (int i = 0; i < 2; i++) {
        c->hme_level0_search_area_in_width_array[i] = (uint16_t)prm[42 + i]; c->hme_level0_search_area_in_height_array[i] = (uint16_t)prm[44 + i];
        c->hme_level1_search_area_in_width_array[i] = (uint16_t)prm[46 + i]; c->hme_level1_search_area_in_height_array[i] = (uint16_t)prm[48 + i];
        c->hme_level2_search_area_in_width_array[i] = (uint16_t)prm[50 + i]; c->hme_level2_search_area_in_height_array[i] = (uint16_t)prm[52 + i];
    }
    c->update_hme_search_center_flag = 0;
    c->fractionalSearchMethod = (uint8_t)prm[24];
    c->p_eight_pos_sad16x16 = eight;
    /* the SB buffers as MotionEstimationKernel loads them (EbMotionEstimationProcess.c:504-556) */
    const uint32_t ox = (uint32_t)prm[2], oy = (uint32_t)prm[3];
    const uint32_t sbw = (uint32_t)prm[0] - ox < 64 ? (uint32_t)prm[0] - ox : 64, sbh = (uint32_t)prm[1] - oy < 64 ? (uint32_t)prm[1] - oy : 64;
    c->sb_buffer = sb; c->sb_buffer_stride = 64;
    c->quarter_sb_buffer = sb + 64 * 64; c->quarter_sb_buffer_stride = 32;
    c->sixteenth_sb_buffer = sb + 64 * 64 + 32 * 32; c->sixteenth_sb_buffer_stride = 16;
    size_t bi = (size_t)(pic[0].origin_y + oy) * pic[0].stride_y + pic[0].origin_x + ox;
    for (int r = 0; r < 64; r++) memcpy(c->sb_buffer + 64 * r, pic[0].buffer_y + bi + (size_t)r * pic[0].stride_y, 64);
    c->sb_src_ptr = pic[0].buffer_y + bi;
    c->sb_src_stride = pic[0].stride_y;
    if (pcs->enable_hme_level1_flag) {
        bi = (size_t)(pic[1].origin_y + (oy >> 1)) * pic[1].stride_y + pic[1].origin_x + (ox >> 1);
        for (uint32_t r = 0; r < (sbh >> 1); r++) memcpy(c->quarter_sb_buffer + 32 * r, pic[1].buffer_y + bi + (size_t)r * pic[1].stride_y, sbw >> 1);
    }
    if (pcs->enable_hme_level0_flag) {
        bi = (size_t)(pic[2].origin_y + (oy >> 2)) * pic[2].stride_y + pic[2].origin_x + (ox >> 2);
        uint8_t *l = c->sixteenth_sb_buffer;
        const uint8_t *f = pic[2].buffer_y + bi;
        for (uint32_t r = 0; r < (sbh >> 2); r += 2) { memcpy(l, f, sbw >> 2); l += 16; f += (size_t)pic[2].stride_y << 1; }
    }
    EbPictureBufferDesc_t input = pic[0];                /* input_ptr: width / height are read for the SB size */
    input.width = (uint16_t)prm[0]; input.height = (uint16_t)prm[1];
    const EbErrorType rc = MotionEstimateLcu(pcs, 0, ox, oy, c, &input);
    for (int l = 0; l < 2; l++) {
        memcpy(best_sad + l * MAX_ME_PU_COUNT, c->p_sb_best_sad[l][0], sizeof(uint32_t) * MAX_ME_PU_COUNT);
        memcpy(best_mv + l * MAX_ME_PU_COUNT, c->p_sb_best_mv[l][0], sizeof(uint32_t) * MAX_ME_PU_COUNT);
        memcpy(best_ssd + l * MAX_ME_PU_COUNT, c->p_sb_best_ssd[l][0], sizeof(uint32_t) * MAX_ME_PU_COUNT);
        area_origin[2 * l] = c->x_search_area_origin[l][0]; area_origin[2 * l + 1] = c->y_search_area_origin[l][0];
    }
    memcpy(bipred_sad, c->p_sb_bipred_sad, sizeof(uint32_t) * MAX_ME_PU_COUNT);
    for (int p = 0; p < MAX_ME_PU_COUNT; p++) {
        int32_t *o = results + 11 * p;
        o[0] = mer[p].xMvL0; o[1] = mer[p].yMvL0; o[2] = mer[p].xMvL1; o[3] = mer[p].yMvL1;
        for (int k = 0; k < 3; k++) { o[4 + 2 * k] = (int32_t)mer[p].distortionDirection[k].distortion; o[5 + 2 * k] = (int32_t)mer[p].distortionDirection[k].direction; }
        o[10] = mer[p].totalMeCandidateIndex;
    }
    sp_free_planes(c, 2);
    free(eight); free(sb); free(mer); free(pic); free(ro); free(w); free(c); free(ectx); free(scs); free(pcs);
    return rc == EB_ErrorNone ? 0 : -2;
}

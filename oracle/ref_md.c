/*
 * oracle/ref_md.c — OUR harness around the end of the reference's intra fast loop of mode decision; compiled into
 * oracle/_ref/libsvtref.so (oracle/Makefile).  TEST INFRASTRUCTURE ONLY.  Nothing of the reference is re-implemented and no stand-in
 * is written for any of its functions (one forwarding excepted, below): every entry allocates zeroed reference structures, fills the fields the called function reads
 * (listed beside each entry with the reference lines that read them) and calls the reference's own function.
 *
 *  ref_md_intra_fast_cost   av1_intra_fast_cost (EbRateDistortionCost.c:531-729) for the candidates of one block
 *  ref_md_model_rd_from_sse model_rd_from_sse (EbInterPrediction.c:3402-3438)
 *  ref_md_sort              sort_fast_loop_candidates (EbModeDecision.c:436-489) on caller-given buffer costs
 *  ref_md_fast_search       inject_intra_candidates -> perform_fast_loop -> sort_fast_loop_candidates for one block, with the counts
 *                           md_encode_block derives in front of them (EbProductCodingLoop.c:3038-3140)
 *  ref_md_inject_intra      inject_intra_candidates (EbModeDecision.c:2364-2536): the list of one block geometry
 *  ref_md_mean8x8           compute_sub_mean8x8_sse2_intrin / compute_mean_of_squared_values8x8_sse2_intrin
 *                           (ASM_SSE2/EbComputeMean_Intrinsic_SSE2.c:52-76, 80-118)
 *
 * The geometry of a block is the reference's own: build_blk_geom(0) fills blk_geom_mds[] (EbUtility.c:1092), ref_md_geom() only
 * searches that table for the first entry of the wanted width, height and origin inside the 64x64 superblock (PART_N entries first).
 *
 * THE ONE EXCEPTION to "no stand-in": Log2f (EbDefinitions.h:1849 names it Log2f_SSE2) exists in the reference only as a NASM routine
 * of one instruction (ASM_SSE2/EbPictureOperators_SSE2.asm:629-632, `bsr rax, r0`), which this C-only subset cannot assemble, and
 * build_blk_geom (EbUtility.c:836-837) and perform_fast_loop's SSD branch (EbProductCodingLoop.c:1249, 1272) call it.  It is
 * forwarded below to the reference's own C function of the same meaning, Log2f64 (EbUtility.c:434-450); nothing is computed here.
 */
#include <stdint.h>
#include <stdlib.h>
#include <string.h>
#include "EbDefinitions.h"
#include "EbUtility.h"
#include "EbPictureControlSet.h"
#include "EbSequenceControlSet.h"
#include "EbModeDecisionProcess.h"
#include "EbModeDecision.h"
#include "EbRateDistortionCost.h"
#include "EbMdRateEstimation.h"
#include "EbNeighborArrays.h"
#include "EbIntraPrediction.h"

void ref_ois_setup(void);
/* reference functions that no header declares (types only; the definitions are the reference's) */
void build_blk_geom(int32_t);
extern uint32_t max_num_active_blocks;
void init_intra_predictors_internal(void);
void init_intra_dc_predictors_c_internal(void);
void model_rd_from_sse(block_size, int16_t, uint64_t, uint32_t *, uint64_t *);
void inject_intra_candidates(PictureControlSet_t *, ModeDecisionContext_t *, const SequenceControlSet *, LargestCodingUnit_t *, uint32_t *);
void perform_fast_loop(PictureControlSet_t *, ModeDecisionContext_t *, ModeDecisionCandidateBuffer_t **, ModeDecisionCandidate_t *, int32_t,
                       int32_t, EbPictureBufferDesc_t *, uint32_t, uint32_t, uint32_t, CodingUnit_t *, uint32_t, uint32_t, uint32_t, uint32_t,
                       EbBool, EbBool, EbAsm);
uint64_t compute_sub_mean8x8_sse2_intrin(uint8_t *, uint16_t);
uint64_t compute_mean_of_squared_values8x8_sse2_intrin(uint8_t *, uint32_t, uint32_t, uint32_t);

uint32_t Log2f_SSE2(uint32_t x) { return (uint32_t)Log2f64(x); }

enum { REF_MD_MAX_CAND = 64, REF_MD_NEIGH = 4096, REF_MD_PRED_STRIDE = SB_STRIDE_Y, REF_MD_PRED_ROWS = 64 + 64 };

/* the structures of one mode-decision block, allocated once and zeroed again by every entry */
typedef struct {
    PictureControlSet_t *pcs;
    PictureParentControlSet_t *ppcs;
    SequenceControlSet *scs;
    Av1Common *cm;
    ModeDecisionContext_t *ctx;
    CodingUnit_t *cu;
    LargestCodingUnit_t *sb;
    MdRateEstimationContext_t *rates;
    ModeDecisionCandidate_t *cand;
    ModeDecisionCandidateBuffer_t *buf[MAX_NFL + 2];
    EbPictureBufferDesc_t *pred[MAX_NFL + 2];
    uint8_t *pred_mem[MAX_NFL + 2];
    uint64_t fast_cost[MAX_NFL + 2];
    NeighborArrayUnit_t mode_type, luma_mode, chroma_mode, luma_recon;
    uint8_t *na_mem;
    EbPictureBufferDesc_t input;
    BlockGeom geom;
} RefMdWorld;
static RefMdWorld *g_w;
static int g_geom_ready;

static void ref_md_geom_table(void) {
    if (!g_geom_ready) {
        build_blk_geom(0);
        g_geom_ready = 1;
    }
}

static RefMdWorld *ref_md_world(void) {
    ref_md_geom_table();
    if (!g_w) {
        RefMdWorld *w = calloc(1, sizeof(*w));
        w->pcs = malloc(sizeof(*w->pcs)); w->ppcs = malloc(sizeof(*w->ppcs)); w->scs = malloc(sizeof(*w->scs));
        w->cm = malloc(sizeof(*w->cm)); w->ctx = malloc(sizeof(*w->ctx)); w->cu = malloc(sizeof(*w->cu));
        w->sb = malloc(sizeof(*w->sb)); w->rates = malloc(sizeof(*w->rates));
        w->cand = malloc(REF_MD_MAX_CAND * sizeof(*w->cand));
        for (int i = 0; i < MAX_NFL + 2; i++) {
            w->buf[i] = malloc(sizeof(*w->buf[i]));
            w->pred[i] = malloc(sizeof(*w->pred[i]));
            w->pred_mem[i] = malloc((size_t)REF_MD_PRED_STRIDE * REF_MD_PRED_ROWS);
        }
        w->na_mem = malloc((size_t)8 * REF_MD_NEIGH + 2 * MAX_PICTURE_HEIGHT_SIZE);
        g_w = w;
    }
    RefMdWorld *w = g_w;
    memset(w->pcs, 0, sizeof(*w->pcs)); memset(w->ppcs, 0, sizeof(*w->ppcs)); memset(w->scs, 0, sizeof(*w->scs));
    memset(w->cm, 0, sizeof(*w->cm)); memset(w->ctx, 0, sizeof(*w->ctx)); memset(w->cu, 0, sizeof(*w->cu));
    memset(w->sb, 0, sizeof(*w->sb)); memset(w->rates, 0, sizeof(*w->rates));
    memset(w->cand, 0, REF_MD_MAX_CAND * sizeof(*w->cand));
    /* the links every entry needs: pcs -> parent -> av1_cm -> back pointer (av1_allow_intrabc, EbEntropyCoding.c:4822-4825) */
    w->pcs->parent_pcs_ptr = w->ppcs;
    w->ppcs->av1_cm = w->cm;
    w->ppcs->sequence_control_set_ptr = w->scs;
    w->cm->p_pcs_ptr = w->ppcs;
    w->cm->pcs_ptr = w->pcs;
    w->ctx->cu_ptr = w->cu;
    w->ctx->sb_ptr = w->sb;
    w->ctx->md_rate_estimation_ptr = w->rates;
    w->ctx->fast_candidate_array = w->cand;
    w->ctx->candidate_buffer_ptr_array = w->buf;
    w->ctx->fast_cost_array = w->fast_cost;
    for (int i = 0; i < REF_MD_MAX_CAND; i++)
        w->cand[i].md_rate_estimation_ptr = w->rates;            /* EbModeDecisionProcess.c:47, 403 */
    for (int i = 0; i < MAX_NFL + 2; i++) {
        memset(w->buf[i], 0, sizeof(*w->buf[i]));
        memset(w->pred[i], 0, sizeof(*w->pred[i]));
        w->buf[i]->prediction_ptr = w->pred[i];
        w->buf[i]->fast_cost_ptr = &w->fast_cost[i];             /* EbModeDecisionProcess.c: fast_cost_ptr = &fast_cost_array[i] */
        w->buf[i]->candidate_ptr = &w->cand[0];
        w->fast_cost[i] = MAX_CU_COST;                           /* ProductCodingLoopInitFastLoop, EbProductCodingLoop.c:1069-1071 */
    }
    return w;
}

/* the reference's geometry of a bwidth x bheight block at (org_x, org_y) inside its superblock; has_uv < 0 keeps the table's value.
 * Returns 0 when the table has no such block. */
static int ref_md_geom(RefMdWorld *w, int bwidth, int bheight, int org_x, int org_y, int has_uv) {
    const BlockGeom *hit = NULL;
    for (int pass = 0; pass < 2 && !hit; pass++)
        for (uint32_t i = 0; i < max_num_active_blocks && !hit; i++) {
            const BlockGeom *g = get_blk_geom_mds(i);
            if (g->bwidth == bwidth && g->bheight == bheight && (org_x < 0 || (g->origin_x == org_x && g->origin_y == org_y)) &&
                (pass == 1 || g->shape == PART_N))
                hit = g;
        }
    if (!hit)
        return 0;
    w->geom = *hit;
    if (has_uv >= 0)
        w->geom.has_uv = has_uv;
    w->ctx->blk_geom = &w->geom;
    return 1;
}

/* the six rate tables in the order and shapes of MdRateEstimationContext_s (EbMdRateEstimation.h:59, 93-103), packed int32 */
static void ref_md_rates(RefMdWorld *w, const int32_t *packed, int32_t intrabc_bits0) {
    MdRateEstimationContext_t *r = w->rates;
    size_t at = 0;
#define TAKE(field) do { memcpy(r->field, packed + at, sizeof(r->field)); at += sizeof(r->field) / sizeof(int32_t); } while (0)
    TAKE(yModeFacBits); TAKE(mbModeFacBits); TAKE(intraUVmodeFacBits); TAKE(angleDeltaFacBits); TAKE(skipModeFacBits); TAKE(intraInterFacBits);
#undef TAKE
    r->intrabcFacBits[0] = intrabc_bits0;
}

/* picture-level fields of the fast cost: slice_type (EbRateDistortionCost.c:627-631, 677); the parent's slice_type,
 * allow_screen_content_tools and allow_intrabc (av1_allow_intrabc, :556, :679: the PARENT's slice type, so a picture that allows
 * intrabc gets an I-slice parent whatever slice_type the cost reads); base_qindex and deq.y_dequant_Q3[q][1] (:689-692) */
static void ref_md_picture(RefMdWorld *w, int slice_is_intra, int allow_intrabc, int base_qindex, int ac_dequant_q3) {
    w->pcs->slice_type = slice_is_intra ? I_SLICE : P_SLICE;
    w->ppcs->slice_type = (slice_is_intra || allow_intrabc) ? I_SLICE : P_SLICE;
    w->ppcs->allow_screen_content_tools = w->ppcs->allow_intrabc = allow_intrabc ? 1 : 0;
    w->ppcs->base_qindex = (uint16_t)base_qindex;
    w->ppcs->deq.y_dequant_Q3[base_qindex][1] = (int16_t)ac_dequant_q3;
}

/* (a) av1_intra_fast_cost, called directly, for ncand candidates of one block.
 *   blk[9]   top_mode, left_mode (the two last arguments, :625-626), skip_flag_context (:615), is_inter_ctx (:677), mi_row, mi_col
 *            (:667), bwidth, bheight of the geometry (:601, 627, 666-667, 695, 705), has_uv (-1: the table's)
 *   pic[6]   slice_is_intra, allow_intrabc (the picture allows intrabc: intrabcFacBits[0] is added, :679-680; use_intrabc stays 0),
 *            intrabc_bits0, base_qindex, ac_dequant_q3, use_ssd
 *   cand     [ncand][7]: pred_mode (:616), angle_delta[Y] (:636), intra_chroma_mode (:606), angle_delta[UV] (:672),
 *            is_directional_mode_flag (:633), is_directional_chroma_mode_flag (:671), use_angle_delta (:633, 671)
 *   out      cost[ncand]; rate[ncand][2] = fast_luma_rate, fast_chroma_rate (:685-686) */
int ref_md_intra_fast_cost(const int32_t *blk, const int32_t *pic, uint64_t lambda, const int32_t *rates, int ncand, const int32_t *cand,
                           const uint64_t *luma, const uint64_t *chroma, uint64_t *cost, uint32_t *rate) {
    RefMdWorld *w = ref_md_world();
    if (ncand < 0 || ncand > REF_MD_MAX_CAND || !ref_md_geom(w, blk[6], blk[7], -1, -1, blk[8]))
        return -1;
    ref_md_picture(w, pic[0], pic[1], pic[3], pic[4]);
    ref_md_rates(w, rates, pic[2]);
    w->cu->skip_flag_context = (unsigned)blk[2];
    w->cu->is_inter_ctx = (uint32_t)blk[3];
    for (int c = 0; c < ncand; c++) {
        ModeDecisionCandidate_t *k = &w->cand[c];
        const int32_t *v = cand + 7 * c;
        k->type = INTRA_MODE;
        k->pred_mode = (PredictionMode)v[0];
        k->intra_luma_mode = (uint32_t)v[0];
        k->angle_delta[PLANE_TYPE_Y] = v[1];
        k->intra_chroma_mode = (uint32_t)v[2];
        k->angle_delta[PLANE_TYPE_UV] = v[3];
        k->is_directional_mode_flag = (uint8_t)v[4];
        k->is_directional_chroma_mode_flag = (uint8_t)v[5];
        k->use_angle_delta = (uint8_t)v[6];
        k->use_intrabc = 0;
        cost[c] = av1_intra_fast_cost(w->cu, k, 0, luma[c], chroma[c], lambda, (EbBool)pic[5], w->pcs, NULL, w->ctx->blk_geom,
                                      (uint32_t)blk[4], (uint32_t)blk[5], (uint32_t)blk[1], (uint32_t)blk[0]);
        rate[2 * c] = (uint32_t)k->fast_luma_rate;
        rate[2 * c + 1] = (uint32_t)k->fast_chroma_rate;
    }
    return 0;
}

/* (b) model_rd_from_sse, called directly: reads nothing but its arguments and num_pels_log2_lookup[bsize] */
void ref_md_model_rd_from_sse(int bsize, int quantizer, uint64_t sse, uint32_t *rate, uint64_t *dist) {
    *rate = 0;
    *dist = 0;
    model_rd_from_sse((block_size)bsize, (int16_t)quantizer, sse, rate, dist);
}

/* (c) sort_fast_loop_candidates, called directly.  Fills: the buffers' fast_cost_ptr targets (:450, 473, 482) = costs[nbuf], their
 * candidate_ptr->type = INTRA_MODE (:462-463), context full_recon_search_count (:444).  best[MAX_NFL + 2], sorted[MAX_NFL] are zeroed
 * first (the function copies MAX_NFL entries of best into sorted, :477-479); *ref_fast_cost starts at MAX_MODE_COST (the caller's
 * initial value, EbProductCodingLoop.c:3133). */
int ref_md_sort(int nbuf, const uint64_t *costs, int full_recon_search_count, uint8_t *best, uint8_t *sorted, uint64_t *ref_fast_cost) {
    RefMdWorld *w = ref_md_world();
    if (nbuf < 1 || nbuf > MAX_NFL + 1 || full_recon_search_count < 1 || full_recon_search_count > nbuf)
        return -1;
    for (int i = 0; i < nbuf; i++)
        w->fast_cost[i] = costs[i];
    w->cand[0].type = INTRA_MODE;
    w->ctx->full_recon_search_count = (uint32_t)full_recon_search_count;
    memset(w->ctx->best_candidate_index_array, 0, sizeof(w->ctx->best_candidate_index_array));
    memset(w->ctx->sorted_candidate_index_array, 0, sizeof(w->ctx->sorted_candidate_index_array));
    *ref_fast_cost = MAX_MODE_COST;
    sort_fast_loop_candidates(w->ctx, (uint32_t)nbuf, w->buf, w->ctx->best_candidate_index_array, w->ctx->sorted_candidate_index_array,
                              ref_fast_cost);
    memcpy(best, w->ctx->best_candidate_index_array, MAX_NFL + 2);
    memcpy(sorted, w->ctx->sorted_candidate_index_array, MAX_NFL);
    return 0;
}

/* what inject_intra_candidates reads: blk_geom (bsize, sq_size, bwidth, bheight, has_uv, txsize_uv[0]; :2385-2391, 2404-2413, 2428,
 * 2466-2474), static_config.encoder_bit_depth (:2379), parent intra_pred_mode (:2397-2407) and reduced_tx_set_used (:2475),
 * context chroma_level (:2448) and fast_candidate_array (:2387) */
static uint32_t ref_md_inject(RefMdWorld *w, int intra_pred_mode, int is_16bit, int chroma_level) {
    uint32_t n = 0;
    w->scs->static_config.encoder_bit_depth = is_16bit ? EB_10BIT : EB_8BIT;
    w->ppcs->intra_pred_mode = (uint8_t)intra_pred_mode;
    w->ppcs->reduced_tx_set_used = 0;
    w->ctx->chroma_level = (uint8_t)chroma_level;
    inject_intra_candidates(w->pcs, w->ctx, w->scs, w->sb, &n);
    return n;
}

static void ref_md_list_out(const RefMdWorld *w, uint32_t n, int32_t *list) {
    for (uint32_t c = 0; c < n; c++) {
        const ModeDecisionCandidate_t *k = &w->cand[c];
        int32_t *v = list + 7 * c;
        v[0] = (int32_t)k->pred_mode; v[1] = k->angle_delta[PLANE_TYPE_Y]; v[2] = (int32_t)k->intra_chroma_mode;
        v[3] = k->angle_delta[PLANE_TYPE_UV]; v[4] = k->is_directional_mode_flag; v[5] = k->is_directional_chroma_mode_flag;
        v[6] = k->use_angle_delta;
    }
}

/* the reference's geometry table, entry by entry: info[8] = bwidth, bheight, sq_size, bsize, has_uv, shape, origin_x, origin_y of
 * blk_geom_mds[idx]; returns 0, or -1 past the table's end */
int ref_md_geom_info(int idx, int32_t *info) {
    ref_md_geom_table();
    if (idx < 0 || (uint32_t)idx >= max_num_active_blocks)
        return -1;
    const BlockGeom *g = get_blk_geom_mds((uint32_t)idx);
    info[0] = g->bwidth; info[1] = g->bheight; info[2] = g->sq_size; info[3] = (int32_t)g->bsize; info[4] = g->has_uv;
    info[5] = (int32_t)g->shape; info[6] = g->origin_x; info[7] = g->origin_y;
    return 0;
}

/* (e) inject_intra_candidates' list of blk_geom_mds[idx]: list [n][7] in the layout of (a)'s cand.  Returns n, or -1 past the table. */
int ref_md_inject_intra(int idx, int intra_pred_mode, int is_16bit, int chroma_level, int32_t *list) {
    RefMdWorld *w = ref_md_world();
    if (idx < 0 || (uint32_t)idx >= max_num_active_blocks)
        return -1;
    w->geom = *get_blk_geom_mds((uint32_t)idx);
    w->ctx->blk_geom = &w->geom;
    const uint32_t n = ref_md_inject(w, intra_pred_mode, is_16bit, chroma_level);
    ref_md_list_out(w, n, list);
    return (int)n;
}

static void ref_md_neighbor_unit(NeighborArrayUnit_t *u, uint8_t *mem, int granularity_log2) {
    memset(u, 0, sizeof(*u));
    u->leftArray = mem; u->topArray = mem + REF_MD_NEIGH;
    u->leftArraySize = u->topArraySize = REF_MD_NEIGH;
    u->unit_size = 1;
    u->granularity_normal = (uint8_t)(1 << granularity_log2); u->granularityNormalLog2 = (uint8_t)granularity_log2;
    u->granularity_top_left = (uint8_t)(1 << granularity_log2); u->granularityTopLeftLog2 = (uint8_t)granularity_log2;
}

/* (d) one block through inject_intra_candidates -> perform_fast_loop -> sort_fast_loop_candidates, as md_encode_block runs them.
 *   p[20]: 0 pic_width, 1 pic_height (luma, multiples of 8), 2 src_stride, 3 x, 4 y (picture origin of the block), 5 bwidth, 6 bheight,
 *          7 top_mode, 8 left_mode (neighbour blocks' luma modes: the intra_luma_mode neighbour arrays, EbIntraPrediction.c:4609-4615,
 *          and the mode-info grid get_filt_type reads), 9 skip_flag_context, 10 is_inter_ctx, 11 path (0: the non-decoupled call,
 *          EbProductCodingLoop.c:3103-3131; 1: the decoupled intra call, :3040-3078), 12 ssd_search (decoupled_fast_loop_search_method
 *          == SSD_SEARCH), 13 slice_is_intra, 14 full_recon_search_count (set_nfl's value), 15 intra_pred_mode, 16 base_qindex,
 *          17 ac_dequant_q3, 18 asm_type, 19 chroma_level (1 or 2: chroma blind at MD, luma only)
 *   src: the luma plane; top [1 + 2 * bwidth], left [1 + 2 * bheight]: the recon neighbours, element 0 the corner (copied into
 *   luma_recon_neighbor_array where AV1IntraPredictionCL reads them, EbIntraPrediction.c:4636-4641)
 *   Structures filled beyond those of (a), (c), (e): context cu_origin_x / y (:4589-4641, EbProductCodingLoop.c:1206-1207),
 *   round_origin_x / y, fast_lambda / full_lambda (:1319), mode_type / intra_luma_mode / intra_chroma_mode / luma_recon neighbour
 *   arrays, sb_ptr->tile_info; cm mi_rows / mi_cols / mi_stride (EbIntraPrediction.c:4131-4138, 4179), pcs mi_grid_base (:4181-4198),
 *   scs sb_size (has_top_right / has_bottom_left), parent interpolation_search_level (EbProductCodingLoop.c:1138) and
 *   enhanced_picture_ptr (the caller's argument); each buffer's prediction_ptr (a SB_STRIDE_Y plane, origin 0).
 *   out_i[8]: 0 ncand, 1 nbuf (buffer_total_count), 2 n (full_recon_search_count on return), 3 bsize, 4 has_uv, 5 scratch present,
 *          6 shape, 7 sq_size
 *   list [ncand][7] as (e); buf_cand [nbuf]: the list index of the candidate each buffer holds on return; buf_cost [nbuf]
 *   (fast_cost_array); best [MAX_NFL + 2], sorted [MAX_NFL]; ref_fast_cost; cand_rate [ncand][2], cand_dist [ncand]
 *   (luma_fast_distortion), cand_cost [ncand] = av1_intra_fast_cost called once more on each candidate's stored distortion (the loop
 *   keeps only the surviving buffers' costs); buf_pred [nbuf][bheight][bwidth]: the buffers' predictions. */
int ref_md_fast_search(const int32_t *p, const uint8_t *src, const uint8_t *top, const uint8_t *left, uint64_t fast_lambda,
                       uint64_t full_lambda, const int32_t *rates, int32_t *out_i, int32_t *list, int32_t *buf_cand, uint64_t *buf_cost,
                       uint8_t *best, uint8_t *sorted, uint64_t *ref_fast_cost, uint32_t *cand_rate, uint64_t *cand_dist,
                       uint64_t *cand_cost, uint8_t *buf_pred) {
    ref_ois_setup();
    static int predictors_ready;
    if (!predictors_ready) {
        init_intra_dc_predictors_c_internal();
        init_intra_predictors_internal();
        predictors_ready = 1;
    }
    RefMdWorld *w = ref_md_world();
    const int pw = p[0], ph = p[1], x = p[3], y = p[4], bw = p[5], bh = p[6];
    if (pw <= 0 || ph <= 0 || pw > REF_MD_NEIGH / 2 || ph > MAX_PICTURE_HEIGHT_SIZE / 2 || (pw & 7) || (ph & 7) || x < 0 || y < 0 ||
        x + bw > pw || y + bh > ph || p[14] < 1 || p[14] > MAX_NFL || p[19] == CHROMA_MODE_0)
        return -1;
    if (!ref_md_geom(w, bw, bh, x & 63, y & 63, -1))
        return -2;
    ModeDecisionContext_t *ctx = w->ctx;
    ref_md_picture(w, p[13], 0, p[16], p[17]);
    ref_md_rates(w, rates, 0);
    w->cu->skip_flag_context = (unsigned)p[9];
    w->cu->is_inter_ctx = (uint32_t)p[10];
    ctx->cu_origin_x = (uint16_t)x; ctx->cu_origin_y = (uint16_t)y;
    ctx->round_origin_x = (uint32_t)((x >> 3) << 3); ctx->round_origin_y = (uint32_t)((y >> 3) << 3);
    ctx->fast_lambda = (uint32_t)fast_lambda; ctx->full_lambda = (uint32_t)full_lambda;
    ctx->full_recon_search_count = (uint32_t)p[14];
    ctx->decouple_intra_inter_fast_loop = (uint8_t)p[11];
    ctx->decoupled_fast_loop_search_method = p[12] ? SSD_SEARCH : 0;
    w->ppcs->interpolation_search_level = 0;
    w->scs->sb_size = BLOCK_64X64;
    /* neighbour arrays: every neighbour an intra block of the caller's mode */
    memset(w->na_mem, 0, (size_t)8 * REF_MD_NEIGH + 2 * MAX_PICTURE_HEIGHT_SIZE);
    ref_md_neighbor_unit(&w->mode_type, w->na_mem, 2);
    ref_md_neighbor_unit(&w->luma_mode, w->na_mem + 2 * REF_MD_NEIGH, 2);
    ref_md_neighbor_unit(&w->chroma_mode, w->na_mem + 4 * REF_MD_NEIGH, 2);
    ref_md_neighbor_unit(&w->luma_recon, w->na_mem + 6 * REF_MD_NEIGH, 0);
    w->luma_recon.topLeftArray = w->na_mem + 8 * REF_MD_NEIGH;
    memset(w->mode_type.leftArray, INTRA_MODE, REF_MD_NEIGH); memset(w->mode_type.topArray, INTRA_MODE, REF_MD_NEIGH);
    memset(w->luma_mode.leftArray, p[8], REF_MD_NEIGH); memset(w->luma_mode.topArray, p[7], REF_MD_NEIGH);
    memcpy(w->luma_recon.topArray + x, top + 1, (size_t)2 * bw);
    memcpy(w->luma_recon.leftArray + y, left + 1, (size_t)2 * bh);
    w->luma_recon.topLeftArray[MAX_PICTURE_HEIGHT_SIZE + x - y] = top[0];
    ctx->mode_type_neighbor_array = &w->mode_type; ctx->intra_luma_mode_neighbor_array = &w->luma_mode;
    ctx->intra_chroma_mode_neighbor_array = &w->chroma_mode; ctx->luma_recon_neighbor_array = &w->luma_recon;
    /* the mode-info grid: the blocks above and to the left carry the caller's modes */
    const int mi_rows = ph >> 2, mi_cols = pw >> 2, nmi = mi_rows * mi_cols;
    w->cm->mi_rows = mi_rows; w->cm->mi_cols = mi_cols; w->cm->mi_stride = mi_cols;
    ModeInfo *mip = calloc((size_t)nmi, sizeof(ModeInfo));
    ModeInfo **grid = calloc((size_t)nmi, sizeof(ModeInfo *));
    for (int i = 0; i < nmi; i++) {
        mip[i].mbmi.ref_frame[0] = INTRA_FRAME;
        grid[i] = &mip[i];
    }
    if (y > 0) mip[((y >> 2) - 1) * mi_cols + (x >> 2)].mbmi.mode = (PredictionMode)p[7];
    if (x > 0) mip[(y >> 2) * mi_cols + (x >> 2) - 1].mbmi.mode = (PredictionMode)p[8];
    w->pcs->mi_grid_base = grid;
    w->sb->tile_info.mi_row_start = 0; w->sb->tile_info.mi_row_end = mi_rows;
    w->sb->tile_info.mi_col_start = 0; w->sb->tile_info.mi_col_end = mi_cols;
    /* pictures */
    memset(&w->input, 0, sizeof(w->input));
    w->input.buffer_y = w->input.bufferCb = w->input.bufferCr = (EbByte)src;
    w->input.stride_y = w->input.strideCb = w->input.strideCr = (uint16_t)p[2];
    w->input.width = (uint16_t)pw; w->input.height = (uint16_t)ph;
    w->ppcs->enhanced_picture_ptr = &w->input;
    for (int i = 0; i < MAX_NFL + 2; i++) {
        memset(w->pred_mem[i], 0, (size_t)REF_MD_PRED_STRIDE * REF_MD_PRED_ROWS);
        w->pred[i]->buffer_y = w->pred_mem[i];
        w->pred[i]->stride_y = REF_MD_PRED_STRIDE;
    }

    /* ---- md_encode_block, EbProductCodingLoop.c:2962-2967 and :3026-3140, in its own order ---- */
    EbPictureBufferDesc_t *input = w->ppcs->enhanced_picture_ptr;
    const uint32_t input_origin = (uint32_t)((y + input->origin_y) * input->stride_y + (x + input->origin_x));
    const uint32_t input_cb_origin = (uint32_t)(((ctx->round_origin_y >> 1) + (input->origin_y >> 1)) * input->strideCb +
                                                ((ctx->round_origin_x >> 1) + (input->origin_x >> 1)));
    const uint32_t cu_origin = (uint32_t)(w->geom.origin_x + w->geom.origin_y * SB_STRIDE_Y);
    const uint32_t cu_chroma_origin = (uint32_t)(ROUND_UV(w->geom.origin_x) / 2 + ROUND_UV(w->geom.origin_y) / 2 * SB_STRIDE_UV);
    const uint32_t total = ref_md_inject(w, p[15], 0, p[19]);          /* ProductGenerateMdCandidatesCu: the intra list only */
    ctx->fast_candidate_intra_count = total;
    const EbAsm asm_type = (EbAsm)p[18];
    const int decoupled = ctx->decouple_intra_inter_fast_loop && (w->geom.sq_size > 4 && w->geom.shape == PART_N && ctx->full_recon_search_count > 1);
    uint32_t nbuf, scratch;
    if (decoupled) {
        ctx->fast_candidate_inter_count = total - ctx->fast_candidate_intra_count;
        ctx->full_recon_search_count = MIN(total, ctx->full_recon_search_count);
        const uint32_t n_intra = (w->pcs->slice_type == I_SLICE) ? ctx->full_recon_search_count : 1;
        const uint32_t n_inter = MIN(ctx->full_recon_search_count - n_intra, ctx->fast_candidate_inter_count);
        ctx->full_recon_search_count = n_intra + n_inter;
        const uint32_t intra_buffers = ctx->fast_candidate_intra_count > n_intra ? n_intra + 1 : n_intra;
        const uint32_t inter_buffers = ctx->fast_candidate_inter_count > n_inter ? n_inter + 1 : n_inter;
        nbuf = intra_buffers + inter_buffers;
        scratch = intra_buffers > n_intra;
        perform_fast_loop(w->pcs, ctx, w->buf, w->cand, 0, (int32_t)ctx->fast_candidate_intra_count - 1, input, input_origin,
                          input_cb_origin, input_cb_origin, w->cu, cu_origin, cu_chroma_origin, 0, intra_buffers, (EbBool)scratch,
                          ctx->decoupled_fast_loop_search_method == SSD_SEARCH, asm_type);
    } else {
        ctx->full_recon_search_count = MIN(total, ctx->full_recon_search_count);
        nbuf = total > ctx->full_recon_search_count ? ctx->full_recon_search_count + 1 : ctx->full_recon_search_count;
        scratch = total > ctx->full_recon_search_count;
        perform_fast_loop(w->pcs, ctx, w->buf, w->cand, 0, (int32_t)total - 1, input, input_origin, input_cb_origin, input_cb_origin,
                          w->cu, cu_origin, cu_chroma_origin, 0, nbuf, (EbBool)scratch, 0, asm_type);
    }
    *ref_fast_cost = MAX_MODE_COST;
    memset(ctx->best_candidate_index_array, 0, sizeof(ctx->best_candidate_index_array));
    memset(ctx->sorted_candidate_index_array, 0, sizeof(ctx->sorted_candidate_index_array));
    sort_fast_loop_candidates(ctx, nbuf, w->buf, ctx->best_candidate_index_array, ctx->sorted_candidate_index_array, ref_fast_cost);

    /* ---- outputs ---- */
    out_i[0] = (int32_t)total; out_i[1] = (int32_t)nbuf; out_i[2] = (int32_t)ctx->full_recon_search_count;
    out_i[3] = (int32_t)w->geom.bsize; out_i[4] = w->geom.has_uv; out_i[5] = (int32_t)scratch;
    out_i[6] = (int32_t)w->geom.shape; out_i[7] = w->geom.sq_size;
    ref_md_list_out(w, total, list);
    for (uint32_t b = 0; b < nbuf; b++) {
        buf_cand[b] = (int32_t)(w->buf[b]->candidate_ptr - w->cand);
        buf_cost[b] = w->fast_cost[b];
        const uint8_t *from = w->pred_mem[b] + cu_origin;
        for (int r = 0; r < bh; r++)
            memcpy(buf_pred + ((size_t)b * bh + r) * bw, from + (size_t)r * REF_MD_PRED_STRIDE, (size_t)bw);
    }
    memcpy(best, ctx->best_candidate_index_array, MAX_NFL + 2);
    memcpy(sorted, ctx->sorted_candidate_index_array, MAX_NFL);
    const int use_ssd = decoupled && ctx->decoupled_fast_loop_search_method == SSD_SEARCH;
    for (uint32_t c = 0; c < total; c++) {
        ModeDecisionCandidate_t *k = &w->cand[c];
        cand_rate[2 * c] = (uint32_t)k->fast_luma_rate; cand_rate[2 * c + 1] = (uint32_t)k->fast_chroma_rate;
        cand_dist[c] = k->luma_fast_distortion;
        cand_cost[c] = av1_intra_fast_cost(w->cu, k, w->cu->qp, k->luma_fast_distortion, 0, use_ssd ? ctx->full_lambda : ctx->fast_lambda,
                                           (EbBool)use_ssd, w->pcs, NULL, ctx->blk_geom, (uint32_t)(y >> MI_SIZE_LOG2),
                                           (uint32_t)(x >> MI_SIZE_LOG2), ctx->intra_luma_left_mode, ctx->intra_luma_top_mode);
    }
    w->pcs->mi_grid_base = NULL;
    free(grid); free(mip);
    return 0;
}

/* (f) the two SSE2 mean leaves of picture analysis, called directly: which = 0 compute_sub_mean8x8_sse2_intrin, 1
 * compute_mean_of_squared_values8x8_sse2_intrin (8 x 8, the area ComputeBlockMeanComputeVariance gives it) */
uint64_t ref_md_mean8x8(const uint8_t *samples, int stride, int which) {
    return which ? compute_mean_of_squared_values8x8_sse2_intrin((uint8_t *)samples, (uint32_t)stride, 8, 8)
                 : compute_sub_mean8x8_sse2_intrin((uint8_t *)samples, (uint16_t)stride);
}

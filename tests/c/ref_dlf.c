/* ref_dlf.c - harness round the reference's deblocking filter, for tests/golden/make_golden_dlf.py.  It is compiled against the
 * reference's headers and linked with the reference's EbDeblockingFilter.c / EbDeblockingFilter_Intrinsic_SSE2.c objects into
 * oracle/_ref/libsvtref_dlf.so.  It allocates zeroed control sets, picture descriptors and a ModeInfo grid, fills only what
 * av1_loop_filter_init, av1_loop_filter_frame, PictureSseCalculations and av1_pick_filter_level read, and calls them.
 *
 * A picture is handed over as three planes of width x height samples (uint8 or uint16) with their strides; the harness copies them
 * into descriptors with 64 samples of padding all round (the SSE2 filters load whole vectors) and copies the result back.  The grid is
 * handed over as 4-byte records {bsize, tx_size, ref_frame0 | skip << 7, mode} of [height / 4][mi_stride]. */
#include <stdint.h>
#include <stdlib.h>
#include <string.h>
#include "EbDefinitions.h"
#include "EbUtility.h"
#include "EbPictureControlSet.h"
#include "EbSequenceControlSet.h"
#include "EbDeblockingFilter.h"
#include "EbDlfProcess.h"

#define PADDING 64

/* EbDeblockingFilter.c defines it without a header declaration */
uint64_t PictureSseCalculations(PictureControlSet_t *picture_control_set_ptr, EbPictureBufferDesc_t *recon_ptr, int32_t plane);

typedef struct ref_dlf_params {
    int32_t width, height, bit_depth;
    int32_t filter_level[2], filter_level_u, filter_level_v, sharpness_level;
    int32_t mode_ref_delta_enabled;
    int8_t ref_deltas[8], mode_deltas[2];
    int8_t pad[2];
    int32_t loop_filter_mode, tx_mode_only_4x4, is_key_frame, base_qindex;      /* the pick only */
} ref_dlf_params;

typedef struct Ctx {
    PictureControlSet_t pcs;
    PictureParentControlSet_t ppcs;
    SequenceControlSet scs;
    EbObjectWrapper scs_wrapper;
    EbPictureBufferDesc_t recon, source, temp;
    DlfContext_t dlf;
    ModeInfo *mi;
    ModeInfo **grid;
    int is16;
} Ctx;

static void desc_alloc(EbPictureBufferDesc_t *d, int w, int h, int is16) {
    memset(d, 0, sizeof(*d));
    d->origin_x = PADDING; d->origin_y = PADDING;
    d->width = (uint16_t)w; d->height = (uint16_t)h; d->maxWidth = (uint16_t)w; d->maxHeight = (uint16_t)h;
    d->bit_depth = is16 ? EB_10BIT : EB_8BIT;
    d->stride_y = (uint16_t)(w + 2 * PADDING); d->strideCb = d->strideCr = (uint16_t)(w / 2 + PADDING);
    d->lumaSize = (uint32_t)d->stride_y * (uint32_t)(h + 2 * PADDING);
    d->chromaSize = (uint32_t)d->strideCb * (uint32_t)(h / 2 + PADDING);
    d->buffer_y = (EbByte)calloc((size_t)d->lumaSize << is16, 1);
    d->bufferCb = (EbByte)calloc((size_t)d->chromaSize << is16, 1);
    d->bufferCr = (EbByte)calloc((size_t)d->chromaSize << is16, 1);
}
static void desc_free(EbPictureBufferDesc_t *d) { free(d->buffer_y); free(d->bufferCb); free(d->bufferCr); }

static uint8_t *plane_origin(EbPictureBufferDesc_t *d, int plane, int is16, int *stride) {
    if (plane == 0) { *stride = d->stride_y; return d->buffer_y + (((size_t)d->origin_x + (size_t)d->origin_y * d->stride_y) << is16); }
    *stride = d->strideCb;
    return (plane == 1 ? d->bufferCb : d->bufferCr) + (((size_t)d->origin_x / 2 + (size_t)d->origin_y / 2 * d->strideCb) << is16);
}
static void plane_in(EbPictureBufferDesc_t *d, int plane, int is16, const void *src, int stride, int w, int h) {
    int ds;
    uint8_t *o = plane_origin(d, plane, is16, &ds);
    for (int y = 0; y < h; y++) memcpy(o + (((size_t)y * ds) << is16), (const uint8_t *)src + (((size_t)y * stride) << is16), (size_t)w << is16);
}
static void plane_out(EbPictureBufferDesc_t *d, int plane, int is16, void *dst, int stride, int w, int h) {
    int ds;
    uint8_t *o = plane_origin(d, plane, is16, &ds);
    for (int y = 0; y < h; y++) memcpy((uint8_t *)dst + (((size_t)y * stride) << is16), o + (((size_t)y * ds) << is16), (size_t)w << is16);
}

static Ctx *ctx_new(const ref_dlf_params *p, const uint8_t *mi_rec, int mi_stride_in) {
    Ctx *c = (Ctx *)calloc(1, sizeof(Ctx));
    const int w = p->width, h = p->height;
    c->is16 = p->bit_depth > 8;
    c->pcs.parent_pcs_ptr = &c->ppcs;
    c->ppcs.sequence_control_set_ptr = &c->scs;
    c->ppcs.sequence_control_set_wrapper_ptr = &c->scs_wrapper;
    c->scs_wrapper.object_ptr = &c->scs;
    c->scs.static_config.encoder_bit_depth = (uint32_t)p->bit_depth;
    c->scs.sb_size = BLOCK_64X64; c->scs.sb_size_pix = 64;
    c->scs.luma_width = (uint16_t)w; c->scs.luma_height = (uint16_t)h;
    c->scs.chroma_width = (uint16_t)(w / 2); c->scs.chroma_height = (uint16_t)(h / 2);
    c->scs.picture_width_in_sb = (uint8_t)((w + 63) / 64);
    c->scs.picture_height_in_sb = (uint8_t)((h + 63) / 64);
    c->scs.pad_right = 0; c->scs.pad_bottom = 0;
    desc_alloc(&c->recon, w, h, c->is16);
    desc_alloc(&c->source, w, h, c->is16);
    desc_alloc(&c->temp, w, h, c->is16);
    c->pcs.recon_picture_ptr = &c->recon; c->pcs.recon_picture16bit_ptr = &c->recon;
    c->ppcs.enhanced_picture_ptr = &c->source; c->pcs.input_frame16bit = &c->source;
    c->dlf.temp_lf_recon_picture_ptr = &c->temp; c->dlf.temp_lf_recon_picture16bit_ptr = &c->temp;
    c->ppcs.is_used_as_reference_flag = EB_FALSE;
    c->ppcs.loop_filter_mode = (uint8_t)p->loop_filter_mode;
    c->ppcs.tx_mode = p->tx_mode_only_4x4 ? ONLY_4X4 : TX_MODE_LARGEST;
    c->ppcs.av1FrameType = p->is_key_frame ? KEY_FRAME : INTER_FRAME;
    c->ppcs.base_qindex = (uint16_t)p->base_qindex;
    struct loopfilter *lf = &c->ppcs.lf;
    lf->filter_level[0] = p->filter_level[0]; lf->filter_level[1] = p->filter_level[1];
    lf->filter_level_u = p->filter_level_u; lf->filter_level_v = p->filter_level_v;
    lf->sharpness_level = p->sharpness_level;
    lf->mode_ref_delta_enabled = (uint8_t)p->mode_ref_delta_enabled;
    for (int i = 0; i < 8; i++) lf->ref_deltas[i] = p->ref_deltas[i];
    for (int i = 0; i < 2; i++) lf->mode_deltas[i] = p->mode_deltas[i];
    /* the grid: picture_width_in_sb * 16 units a row, whole superblock rows; units outside the picture point at unit 0 */
    const int gs = c->scs.picture_width_in_sb * 16, gr = c->scs.picture_height_in_sb * 16;
    c->mi = (ModeInfo *)calloc((size_t)gs * gr + 1, sizeof(ModeInfo));
    c->grid = (ModeInfo **)calloc((size_t)gs * gr, sizeof(ModeInfo *));
    for (int r = 0; r < gr; r++)
        for (int col = 0; col < gs; col++) {
            ModeInfo *m = &c->mi[(size_t)r * gs + col];
            c->grid[(size_t)r * gs + col] = m;
            if (mi_rec && r < h / 4 && col < w / 4) {
                const uint8_t *e = mi_rec + ((size_t)r * mi_stride_in + col) * 4;
                m->mbmi.sb_type = (block_size)e[0];
                m->mbmi.tx_size = (TxSize)e[1];
                m->mbmi.ref_frame[0] = (MvReferenceFrame)(e[2] & 7);
                m->mbmi.skip = (int8_t)(e[2] >> 7);
                m->mbmi.mode = (PredictionMode)e[3];
            }
        }
    c->pcs.mi_grid_base = c->grid;
    av1_loop_filter_init(&c->pcs);
    return c;
}
static void ctx_free(Ctx *c) {
    desc_free(&c->recon); desc_free(&c->source); desc_free(&c->temp);
    free(c->mi); free(c->grid); free(c);
}

/* av1_loop_filter_frame(recon, pcs, plane_start, plane_end) on the three planes, in place */
int ref_dlf_frame(const ref_dlf_params *p, void *y, int sy, void *cb, int scb, void *cr, int scr, const uint8_t *mi, int mi_stride,
                  int plane_start, int plane_end) {
    Ctx *c = ctx_new(p, mi, mi_stride);
    plane_in(&c->recon, 0, c->is16, y, sy, p->width, p->height);
    plane_in(&c->recon, 1, c->is16, cb, scb, p->width / 2, p->height / 2);
    plane_in(&c->recon, 2, c->is16, cr, scr, p->width / 2, p->height / 2);
    av1_loop_filter_frame(&c->recon, &c->pcs, plane_start, plane_end);
    plane_out(&c->recon, 0, c->is16, y, sy, p->width, p->height);
    plane_out(&c->recon, 1, c->is16, cb, scb, p->width / 2, p->height / 2);
    plane_out(&c->recon, 2, c->is16, cr, scr, p->width / 2, p->height / 2);
    ctx_free(c);
    return 0;
}

/* ss_err[level] of every plane: per level the plane is filtered as try_filter_frame does (luma with the level in both directions),
 * PictureSseCalculations against the source, and the unfiltered plane is put back.  sse: [3][64] */
int ref_dlf_table(const ref_dlf_params *p, const void *y, int sy, const void *cb, int scb, const void *cr, int scr, const void *src_y, int ssy,
                  const void *src_cb, int sscb, const void *src_cr, int sscr, const uint8_t *mi, int mi_stride, uint64_t *sse) {
    Ctx *c = ctx_new(p, mi, mi_stride);
    const void *rp[3] = {y, cb, cr}, *sp[3] = {src_y, src_cb, src_cr};
    const int rs[3] = {sy, scb, scr}, ss[3] = {ssy, sscb, sscr};
    for (int pl = 0; pl < 3; pl++) plane_in(&c->source, pl, c->is16, sp[pl], ss[pl], pl ? p->width / 2 : p->width, pl ? p->height / 2 : p->height);
    for (int pl = 0; pl < 3; pl++)
        for (int level = 0; level < 64; level++) {
            struct loopfilter *lf = &c->ppcs.lf;
            plane_in(&c->recon, pl, c->is16, rp[pl], rs[pl], pl ? p->width / 2 : p->width, pl ? p->height / 2 : p->height);
            if (pl == 0) lf->filter_level[0] = lf->filter_level[1] = level;
            else if (pl == 1) lf->filter_level_u = level;
            else lf->filter_level_v = level;
            av1_loop_filter_frame(&c->recon, &c->pcs, pl, pl + 1);
            sse[pl * 64 + level] = PictureSseCalculations(&c->pcs, &c->recon, pl);
        }
    ctx_free(c);
    return 0;
}

/* av1_pick_filter_level whole: method 0 = LPF_PICK_FROM_FULL_IMAGE (the descriptor's four levels are the previous picture's),
 * 1 = LPF_PICK_FROM_Q.  levels: {filter_level[0], filter_level[1], filter_level_u, filter_level_v}; sharpness: what the pick stored */
int ref_dlf_pick(const ref_dlf_params *p, int method, const void *y, int sy, const void *cb, int scb, const void *cr, int scr, const void *src_y,
                 int ssy, const void *src_cb, int sscb, const void *src_cr, int sscr, const uint8_t *mi, int mi_stride, int32_t *levels,
                 int32_t *sharpness) {
    Ctx *c = ctx_new(p, mi, mi_stride);
    if (y) {
        const void *rp[3] = {y, cb, cr}, *sp[3] = {src_y, src_cb, src_cr};
        const int rs[3] = {sy, scb, scr}, ss[3] = {ssy, sscb, sscr};
        for (int pl = 0; pl < 3; pl++) {
            plane_in(&c->recon, pl, c->is16, rp[pl], rs[pl], pl ? p->width / 2 : p->width, pl ? p->height / 2 : p->height);
            plane_in(&c->source, pl, c->is16, sp[pl], ss[pl], pl ? p->width / 2 : p->width, pl ? p->height / 2 : p->height);
        }
    }
    av1_pick_filter_level(&c->dlf, &c->source, &c->pcs, method ? LPF_PICK_FROM_Q : LPF_PICK_FROM_FULL_IMAGE);
    levels[0] = c->ppcs.lf.filter_level[0]; levels[1] = c->ppcs.lf.filter_level[1];
    levels[2] = c->ppcs.lf.filter_level_u; levels[3] = c->ppcs.lf.filter_level_v;
    if (sharpness) *sharpness = c->ppcs.lf.sharpness_level;
    ctx_free(c);
    return 0;
}

/* one of the sixteen filters on a four-sample edge unit: s points at q0 of the unit's first line.  flavour 0: the entry the
 * reference's macro selects (_sse2); 1: the _c version, -1 returned where the reference has none */
int ref_dlf_filter(int flavour, int dir, int len, int bd, void *s, int pitch, int mblim, int lim, int hev) {
    uint8_t b[16], l[16], t[16];
    memset(b, mblim, 16); memset(l, lim, 16); memset(t, hev, 16);
    if (bd == 8) {
        uint8_t *q = (uint8_t *)s;
        if (flavour == 0) {
            if (dir == 0) { if (len == 4) aom_lpf_vertical_4(q, pitch, b, l, t); else if (len == 6) aom_lpf_vertical_6(q, pitch, b, l, t);
                            else if (len == 8) aom_lpf_vertical_8(q, pitch, b, l, t); else aom_lpf_vertical_14(q, pitch, b, l, t); }
            else { if (len == 4) aom_lpf_horizontal_4(q, pitch, b, l, t); else if (len == 6) aom_lpf_horizontal_6(q, pitch, b, l, t);
                   else if (len == 8) aom_lpf_horizontal_8(q, pitch, b, l, t); else aom_lpf_horizontal_14(q, pitch, b, l, t); }
            return 0;
        }
        if (dir == 0 && len == 4) { aom_lpf_vertical_4_c(q, pitch, b, l, t); return 0; }
        if (dir == 0 && len == 8) { aom_lpf_vertical_8_c(q, pitch, b, l, t); return 0; }
        if (dir == 1 && len == 4) { aom_lpf_horizontal_4_c(q, pitch, b, l, t); return 0; }
        if (dir == 1 && len == 6) { aom_lpf_horizontal_6_c(q, pitch, b, l, t); return 0; }
        if (dir == 1 && len == 8) { aom_lpf_horizontal_8_c(q, pitch, b, l, t); return 0; }
        return -1;
    }
    uint16_t *q = (uint16_t *)s;
    if (flavour == 0) {
        if (dir == 0) { if (len == 4) aom_highbd_lpf_vertical_4(q, pitch, b, l, t, bd); else if (len == 6) aom_highbd_lpf_vertical_6(q, pitch, b, l, t, bd);
                        else if (len == 8) aom_highbd_lpf_vertical_8(q, pitch, b, l, t, bd); else aom_highbd_lpf_vertical_14(q, pitch, b, l, t, bd); }
        else { if (len == 4) aom_highbd_lpf_horizontal_4(q, pitch, b, l, t, bd); else if (len == 6) aom_highbd_lpf_horizontal_6(q, pitch, b, l, t, bd);
               else if (len == 8) aom_highbd_lpf_horizontal_8(q, pitch, b, l, t, bd); else aom_highbd_lpf_horizontal_14(q, pitch, b, l, t, bd); }
        return 0;
    }
    if (dir == 0 && len == 4) { aom_highbd_lpf_vertical_4_c(q, pitch, b, l, t, bd); return 0; }
    if (dir == 0 && len == 8) { aom_highbd_lpf_vertical_8_c(q, pitch, b, l, t, bd); return 0; }
    if (dir == 1 && len == 4) { aom_highbd_lpf_horizontal_4_c(q, pitch, b, l, t, bd); return 0; }
    if (dir == 1 && len == 8) { aom_highbd_lpf_horizontal_8_c(q, pitch, b, l, t, bd); return 0; }
    return -1;
}

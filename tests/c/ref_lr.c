/* ref_lr.c - harness round the reference's loop restoration, for tests/golden/make_golden_lr.py.  It compiles the reference's
 * EbRestorationPick.c in place (#include) to reach its static try_restoration_unit_seg, and is linked with the reference's
 * EbRestoration.c, convolve.c, EbPsnr.c and the AVX2 restoration objects into oracle/_ref/libsvtref_lr.so.
 *
 * A picture is handed over as three tightly packed planes (uint8 or uint16) of the deblocked picture, the CDEF output and the source.
 * The harness copies them into Yv12BufferConfig frames with 64 samples of padding all round, allocates the stripe boundary buffers the
 * way av1_alloc_restoration_buffers sizes them (that function itself allocates through the encoder's memory map, which a harness
 * does not have), and calls av1_loop_restoration_save_boundary_lines on the deblocked frame (after_cdef 0) and on the CDEF frame
 * (after_cdef 1), as EbCdefProcess.c / EbDlfProcess.c do.  A whole picture is then filtered by the body of
 * av1_loop_restoration_filter_frame: extend_frame, av1_foreach_rest_unit_in_frame with a visitor that hands every unit to
 * av1_loop_restoration_filter_unit exactly as filter_frame_on_unit does; the function itself is not called because it allocates
 * cm->rst_frame through the same memory map.  flavour 0 sets the reference's dispatch pointers to the _c functions, 1 to _avx2. */
/* every trial of the reference's search goes through av1_loop_restoration_filter_unit: the include below sees it under another name, a
 * hook defined further down that notes the trial's taps and hands over to the real function */
#define av1_loop_restoration_filter_unit ref_lr_hooked_filter_unit
#include "EbRestorationPick.c"
#undef av1_loop_restoration_filter_unit
void av1_loop_restoration_filter_unit(uint8_t need_bounadaries, const RestorationTileLimits *limits, const RestorationUnitInfo *rui,
                                      const RestorationStripeBoundaries *rsb, RestorationLineBuffers *rlbs, const AV1PixelRect *tile_rect, int32_t tile_stripe0,
                                      int32_t ss_x, int32_t ss_y, int32_t highbd, int32_t bit_depth, uint8_t *data8, int32_t stride, uint8_t *dst8, int32_t dst_stride,
                                      int32_t *tmpbuf, int32_t optimized_lr);

#define PADDING 64
#define MAX_LOG 256
static int g_log_n = -1;                /* -1: not logging */
static int16_t g_log[MAX_LOG][6];       /* vfilter[0 .. 2], hfilter[0 .. 2] of every trial */

void ref_lr_hooked_filter_unit(uint8_t need_bounadaries, const RestorationTileLimits *limits, const RestorationUnitInfo *rui,
                               const RestorationStripeBoundaries *rsb, RestorationLineBuffers *rlbs, const AV1PixelRect *tile_rect, int32_t tile_stripe0,
                               int32_t ss_x, int32_t ss_y, int32_t highbd, int32_t bit_depth, uint8_t *data8, int32_t stride, uint8_t *dst8, int32_t dst_stride,
                               int32_t *tmpbuf, int32_t optimized_lr) {
    if (g_log_n >= 0 && g_log_n < MAX_LOG && rui->restoration_type == RESTORE_WIENER) {
        for (int i = 0; i < 3; i++) { g_log[g_log_n][i] = rui->wiener_info.vfilter[i]; g_log[g_log_n][3 + i] = rui->wiener_info.hfilter[i]; }
        g_log_n++;
    }
    av1_loop_restoration_filter_unit(need_bounadaries, limits, rui, rsb, rlbs, tile_rect, tile_stripe0, ss_x, ss_y, highbd, bit_depth, data8, stride, dst8,
                                     dst_stride, tmpbuf, optimized_lr);
}

/* two one-line assembly routines of the reference the search calls: the MMX state reset, and the 16x16 squared error of 16-bit samples
 * (ASM_SSE2/highbd_variance_impl_sse2.asm behind aom_highbd_8_mse16x16_sse2), restated in C */
void RunEmms(void) { __asm__ volatile("emms"); }
static void hbd_mse16x16(const uint8_t *a8, int32_t a_stride, const uint8_t *b8, int32_t b_stride, uint32_t *sse) {
    const uint16_t *a = CONVERT_TO_SHORTPTR(a8), *b = CONVERT_TO_SHORTPTR(b8);
    uint32_t s = 0;
    for (int y = 0; y < 16; y++)
        for (int x = 0; x < 16; x++) { const int32_t d = (int32_t)a[y * a_stride + x] - (int32_t)b[y * b_stride + x]; s += (uint32_t)(d * d); }
    *sse = s;
}

typedef struct ref_lr_rec { int32_t type, vfilter[3], hfilter[3], ep, xqd[2]; } ref_lr_rec;

typedef struct Frame { Yv12BufferConfig y; uint8_t *alloc[3]; } Frame;

typedef struct Ctx {
    Av1Common cm;
    Frame dblk, cdef, src, dst;
    int w, h, bd, hbd;
    int32_t *tmpbuf;
} Ctx;

static void frame_alloc(Frame *f, int w, int h, int hbd) {
    memset(f, 0, sizeof(*f));
    for (int p = 0; p < 3; p++) {
        const int pw = p ? w / 2 : w, ph = p ? h / 2 : h, stride = pw + 2 * PADDING;
        f->alloc[p] = (uint8_t *)calloc((size_t)stride * (ph + 2 * PADDING) << hbd, 1);
        uint8_t *o = f->alloc[p] + (((size_t)PADDING * stride + PADDING) << hbd);
        f->y.buffers[p] = hbd ? CONVERT_TO_BYTEPTR(o) : o;
        f->y.strides[p > 0] = stride;
        f->y.widths[p > 0] = pw; f->y.heights[p > 0] = ph;
        f->y.crop_widths[p > 0] = pw; f->y.crop_heights[p > 0] = ph;
    }
    f->y.border = PADDING; f->y.subsampling_x = 1; f->y.subsampling_y = 1;
    f->y.flags = hbd ? YV12_FLAG_HIGHBITDEPTH : 0;
}
static uint8_t *frame_origin(Frame *f, int p, int hbd) {
    const int stride = f->y.strides[p > 0];
    return f->alloc[p] + (((size_t)PADDING * stride + PADDING) << hbd);
}
static void frame_in(Frame *f, int hbd, const void *const planes[3]) {
    for (int p = 0; p < 3; p++) {
        const int pw = f->y.crop_widths[p > 0], ph = f->y.crop_heights[p > 0], stride = f->y.strides[p > 0];
        uint8_t *o = frame_origin(f, p, hbd);
        for (int y = 0; y < ph; y++) memcpy(o + (((size_t)y * stride) << hbd), (const uint8_t *)planes[p] + (((size_t)y * pw) << hbd), (size_t)pw << hbd);
    }
}
static void frame_out(Frame *f, int hbd, void *const planes[3]) {
    for (int p = 0; p < 3; p++) {
        const int pw = f->y.crop_widths[p > 0], ph = f->y.crop_heights[p > 0], stride = f->y.strides[p > 0];
        uint8_t *o = frame_origin(f, p, hbd);
        for (int y = 0; y < ph; y++) memcpy((uint8_t *)planes[p] + (((size_t)y * pw) << hbd), o + (((size_t)y * stride) << hbd), (size_t)pw << hbd);
    }
}
static void frame_free(Frame *f) { for (int p = 0; p < 3; p++) free(f->alloc[p]); }

static void set_flavour(int avx2) {
    apply_selfguided_restoration = avx2 ? apply_selfguided_restoration_avx2 : apply_selfguided_restoration_c;
    av1_selfguided_restoration = avx2 ? av1_selfguided_restoration_avx2 : av1_selfguided_restoration_c;
    av1_wiener_convolve_add_src = avx2 ? av1_wiener_convolve_add_src_avx2 : av1_wiener_convolve_add_src_c;
    av1_highbd_wiener_convolve_add_src = avx2 ? av1_highbd_wiener_convolve_add_src_avx2 : av1_highbd_wiener_convolve_add_src_c;
    av1_compute_stats = avx2 ? av1_compute_stats_avx2 : av1_compute_stats_c;
    av1_compute_stats_highbd = avx2 ? av1_compute_stats_highbd_avx2 : av1_compute_stats_highbd_c;
    av1_lowbd_pixel_proj_error = avx2 ? av1_lowbd_pixel_proj_error_avx2 : av1_lowbd_pixel_proj_error_c;
    av1_highbd_pixel_proj_error = avx2 ? av1_highbd_pixel_proj_error_avx2 : av1_highbd_pixel_proj_error_c;
    aom_mse16x16 = aom_mse16x16_c;      /* what get_sse (EbPsnr.c:98) sums over whole 16x16 blocks */
    aom_highbd_8_mse16x16 = hbd_mse16x16;
}

void ref_lr_free(Ctx *c) {
    if (!c) return;
    for (int p = 0; p < 3; p++) {
        free(c->cm.rst_info[p].unit_info);
        free(c->cm.rst_info[p].boundaries.stripe_boundary_above);
        free(c->cm.rst_info[p].boundaries.stripe_boundary_below);
    }
    frame_free(&c->dblk); frame_free(&c->cdef); frame_free(&c->src); frame_free(&c->dst);
    free(c->tmpbuf);
    free(c);
}

Ctx *ref_lr_new(int w, int h, int bd, const int32_t unit_size[3], const void *const dblk[3], const void *const cdef[3], const void *const src[3]) {
    Ctx *c = (Ctx *)calloc(1, sizeof(Ctx));
    c->w = w; c->h = h; c->bd = bd; c->hbd = bd > 8;
    Av1Common *cm = &c->cm;
    cm->width = w; cm->height = h; cm->superres_upscaled_width = w; cm->superres_upscaled_height = h;
    cm->subsampling_x = 1; cm->subsampling_y = 1; cm->bit_depth = bd; cm->use_highbitdepth = c->hbd;
    cm->mi_rows = h / 4; cm->mi_cols = w / 4;
    frame_alloc(&c->dblk, w, h, c->hbd); frame_alloc(&c->cdef, w, h, c->hbd); frame_alloc(&c->src, w, h, c->hbd); frame_alloc(&c->dst, w, h, c->hbd);
    frame_in(&c->dblk, c->hbd, dblk); frame_in(&c->cdef, c->hbd, cdef); frame_in(&c->src, c->hbd, src);
    cm->frame_to_show = &c->cdef.y;
    c->tmpbuf = (int32_t *)calloc(RESTORATION_TMPBUF_SIZE, 1);
    cm->rst_tmpbuf = c->tmpbuf;
    /* av1_alloc_restoration_struct (EbRestoration.c:198-235) and av1_alloc_restoration_buffers (:1746-1808), with calloc */
    const int num_stripes = (RESTORATION_UNIT_OFFSET + (cm->mi_rows << MI_SIZE_LOG2) + 63) / 64;
    cm->rst_end_stripe[0] = num_stripes;
    for (int p = 0; p < 3; p++) {
        RestorationInfo *rsi = &cm->rst_info[p];
        rsi->restoration_unit_size = unit_size[p];
        const int pw = p ? w / 2 : w, ph = p ? h / 2 : h;
        rsi->horz_units_per_tile = AOMMAX((pw + (unit_size[p] >> 1)) / unit_size[p], 1);
        rsi->vert_units_per_tile = AOMMAX((ph + (unit_size[p] >> 1)) / unit_size[p], 1);
        rsi->units_per_tile = rsi->horz_units_per_tile * rsi->vert_units_per_tile;
        rsi->unit_info = (RestorationUnitInfo *)calloc((size_t)rsi->units_per_tile, sizeof(RestorationUnitInfo));
        const int stride = ALIGN_POWER_OF_TWO(pw + 2 * RESTORATION_EXTRA_HORZ, 5);
        const int size = num_stripes * stride * RESTORATION_CTX_VERT << c->hbd;
        rsi->boundaries.stripe_boundary_above = (uint8_t *)calloc((size_t)size, 1);
        rsi->boundaries.stripe_boundary_below = (uint8_t *)calloc((size_t)size, 1);
        rsi->boundaries.stripe_boundary_size = size;
        rsi->boundaries.stripe_boundary_stride = stride;
    }
    av1_loop_restoration_save_boundary_lines(&c->dblk.y, cm, 0);
    av1_loop_restoration_save_boundary_lines(&c->cdef.y, cm, 1);
    /* what av1_loop_restoration_filter_frame and restoration_seg_search do before any unit is filtered */
    for (int p = 0; p < 3; p++)
        extend_frame(c->cdef.y.buffers[p], c->cdef.y.crop_widths[p > 0], c->cdef.y.crop_heights[p > 0], c->cdef.y.strides[p > 0], RESTORATION_BORDER,
                     RESTORATION_BORDER, c->hbd);
    return c;
}

/* the reference's own numbers: out = {horz_units_per_tile, vert_units_per_tile, units_per_tile} as av1_alloc_restoration_struct's
 * formula gives them, and the limits the visitor hands out */
typedef struct Limits { int want, found; RestorationTileLimits l; int count; } Limits;
static void limits_visitor(const RestorationTileLimits *limits, const AV1PixelRect *tile_rect, int32_t rest_unit_idx, void *priv) {
    Limits *L = (Limits *)priv;
    (void)tile_rect;
    L->count++;
    if (rest_unit_idx == L->want) { L->l = *limits; L->found = 1; }
}
int ref_lr_grid(Ctx *c, int plane, int32_t out[4]) {
    Limits L; memset(&L, 0, sizeof(L)); L.want = -1;
    av1_foreach_rest_unit_in_frame(&c->cm, plane, NULL, limits_visitor, &L);
    out[0] = c->cm.rst_info[plane].horz_units_per_tile; out[1] = c->cm.rst_info[plane].vert_units_per_tile;
    out[2] = c->cm.rst_info[plane].units_per_tile; out[3] = L.count;
    return 0;
}
int ref_lr_limits(Ctx *c, int plane, int unit, int32_t out[4]) {
    Limits L; memset(&L, 0, sizeof(L)); L.want = unit;
    av1_foreach_rest_unit_in_frame(&c->cm, plane, NULL, limits_visitor, &L);
    if (!L.found) return -1;
    out[0] = L.l.h_start; out[1] = L.l.h_end; out[2] = L.l.v_start; out[3] = L.l.v_end;
    return 0;
}

static void fill_rui(RestorationUnitInfo *rui, const ref_lr_rec *r) {
    memset(rui, 0, sizeof(*rui));
    rui->restoration_type = (RestorationType)r->type;
    for (int i = 0; i < 3; i++) {
        rui->wiener_info.vfilter[i] = rui->wiener_info.vfilter[6 - i] = (int16_t)r->vfilter[i];
        rui->wiener_info.hfilter[i] = rui->wiener_info.hfilter[6 - i] = (int16_t)r->hfilter[i];
    }
    rui->wiener_info.vfilter[3] = (int16_t)(-2 * (r->vfilter[0] + r->vfilter[1] + r->vfilter[2]));
    rui->wiener_info.hfilter[3] = (int16_t)(-2 * (r->hfilter[0] + r->hfilter[1] + r->hfilter[2]));
    rui->sgrproj_info.ep = r->ep; rui->sgrproj_info.xqd[0] = r->xqd[0]; rui->sgrproj_info.xqd[1] = r->xqd[1];
}

typedef struct FrameCtxt { Ctx *c; int plane; RestorationLineBuffers rlbs; } FrameCtxt;
static void frame_visitor(const RestorationTileLimits *limits, const AV1PixelRect *tile_rect, int32_t rest_unit_idx, void *priv) {
    FrameCtxt *f = (FrameCtxt *)priv;
    Ctx *c = f->c;
    const int p = f->plane;
    const RestorationInfo *rsi = &c->cm.rst_info[p];
    av1_loop_restoration_filter_unit(1, limits, &rsi->unit_info[rest_unit_idx], &rsi->boundaries, &f->rlbs, tile_rect, 0, p > 0, p > 0, c->hbd, c->bd,
                                     c->cdef.y.buffers[p], c->cdef.y.strides[p > 0], c->dst.y.buffers[p], c->dst.y.strides[p > 0], c->cm.rst_tmpbuf, 0);
}

/* units[plane]: units_per_tile records; out: three tightly packed planes */
int ref_lr_frame(Ctx *c, int flavour, const int32_t frame_type[3], const ref_lr_rec *const units[3], void *const out[3]) {
    set_flavour(flavour);
    for (int p = 0; p < 3; p++) {
        RestorationInfo *rsi = &c->cm.rst_info[p];
        rsi->frame_restoration_type = (RestorationType)frame_type[p];
        const int pw = c->cdef.y.crop_widths[p > 0], ph = c->cdef.y.crop_heights[p > 0];
        if (frame_type[p] == RESTORE_NONE) {       /* the plane is left as it is */
            uint8_t *s = frame_origin(&c->cdef, p, c->hbd), *d = frame_origin(&c->dst, p, c->hbd);
            for (int y = 0; y < ph; y++)
                memcpy(d + (((size_t)y * c->dst.y.strides[p > 0]) << c->hbd), s + (((size_t)y * c->cdef.y.strides[p > 0]) << c->hbd), (size_t)pw << c->hbd);
            continue;
        }
        for (int u = 0; u < rsi->units_per_tile; u++) fill_rui(&rsi->unit_info[u], &units[p][u]);
        FrameCtxt f; f.c = c; f.plane = p;
        av1_foreach_rest_unit_in_frame(&c->cm, p, NULL, frame_visitor, &f);
    }
    frame_out(&c->dst, c->hbd, out);
    return 0;
}

/* the plain squared error of 16-bit samples over a unit: what sse_restoration_unit gives at high bit depth, where the reference's
 * aom_highbd_8_mse16x16 exists only as an assembly routine (ASM_SSE2/highbd_variance_impl_sse2.asm) */
static int64_t sse16(Ctx *c, Frame *a, Frame *b, int plane, const RestorationTileLimits *l) {
    const uint16_t *pa = (const uint16_t *)frame_origin(a, plane, 1), *pb = (const uint16_t *)frame_origin(b, plane, 1);
    const int sa = a->y.strides[plane > 0], sb = b->y.strides[plane > 0];
    int64_t sum = 0;
    (void)c;
    for (int y = l->v_start; y < l->v_end; y++)
        for (int x = l->h_start; x < l->h_end; x++) {
            const int64_t d = (int64_t)pa[(size_t)y * sa + x] - (int64_t)pb[(size_t)y * sb + x];
            sum += d * d;
        }
    return sum;
}

/* try_restoration_unit_seg for one unit and record; a record of type none gives the unfiltered unit's error (search_norestore_seg).
 * At high bit depth the unit is filtered by the same av1_loop_restoration_filter_unit call try_restoration_unit_seg makes and the error
 * is summed here (sse16). */
int64_t ref_lr_try(Ctx *c, int flavour, int plane, int unit, const ref_lr_rec *rec) {
    set_flavour(flavour);
    Limits L; memset(&L, 0, sizeof(L)); L.want = unit;
    av1_foreach_rest_unit_in_frame(&c->cm, plane, NULL, limits_visitor, &L);
    if (!L.found) return -1;
    RestSearchCtxt rsc; memset(&rsc, 0, sizeof(rsc));
    rsc.src = &c->src.y; rsc.dst = &c->dst.y; rsc.cm = &c->cm; rsc.plane = plane; rsc.org_frame_to_show = &c->cdef.y; rsc.tmpbuf = c->tmpbuf;
    rsc.tile_stripe0 = 0;
    const int is_uv = plane > 0;
    AV1PixelRect tile; tile.left = 0; tile.top = 0; tile.right = c->w >> is_uv; tile.bottom = c->h >> is_uv;
    if (rec->type == RESTORE_NONE) return c->hbd ? sse16(c, &c->src, &c->cdef, plane, &L.l) : sse_restoration_unit(&L.l, rsc.src, rsc.org_frame_to_show, plane, 0);
    RestorationUnitInfo rui;
    fill_rui(&rui, rec);
    if (!c->hbd) return try_restoration_unit_seg(&rsc, &L.l, &tile, &rui);
    RestorationLineBuffers rlbs;
    av1_loop_restoration_filter_unit(1, &L.l, &rui, &c->cm.rst_info[plane].boundaries, &rlbs, &tile, 0, is_uv, is_uv, 1, c->bd, c->cdef.y.buffers[plane],
                                     c->cdef.y.strides[is_uv], c->dst.y.buffers[plane], c->dst.y.strides[is_uv], c->tmpbuf, 0);
    return sse16(c, &c->src, &c->dst, plane, &L.l);
}

/* av1_compute_stats[_highbd]_{c,avx2} over one unit; M [win2], H [win2 * win2] */
int ref_lr_stats(Ctx *c, int flavour, int plane, int unit, int win, int64_t *M, int64_t *H) {
    Limits L; memset(&L, 0, sizeof(L)); L.want = unit;
    av1_foreach_rest_unit_in_frame(&c->cm, plane, NULL, limits_visitor, &L);
    if (!L.found) return -1;
    const int is_uv = plane > 0;
    const uint8_t *dgd = c->cdef.y.buffers[plane], *src = c->src.y.buffers[plane];
    const int ds = c->cdef.y.strides[is_uv], ss = c->src.y.strides[is_uv];
    if (c->hbd) (flavour ? av1_compute_stats_highbd_avx2 : av1_compute_stats_highbd_c)(win, dgd, src, L.l.h_start, L.l.h_end, L.l.v_start, L.l.v_end, ds, ss, M, H,
                                                                                        (aom_bit_depth_t)c->bd);
    else (flavour ? av1_compute_stats_avx2 : av1_compute_stats_c)(win, dgd, src, L.l.h_start, L.l.h_end, L.l.v_start, L.l.v_end, ds, ss, M, H);
    return 0;
}

/* search_wiener_seg whole for one unit: statistics, derivation, score, refinement walk.  out_taps: the final vfilter[0 .. 2],
 * hfilter[0 .. 2]; *out_sse: rusi->sse[RESTORE_WIENER] (INT64_MAX when the score rejects); trials [max_trials][6]: the taps of every
 * trial in order (the first is the derivation's filter); returns the number of trials, or -1 */
int ref_lr_search_wiener(Ctx *c, int flavour, int plane, int unit, int wn_filter_mode, int16_t out_taps[6], int64_t *out_sse, int16_t *trials, int max_trials) {
    set_flavour(flavour);
    Limits L; memset(&L, 0, sizeof(L)); L.want = unit;
    av1_foreach_rest_unit_in_frame(&c->cm, plane, NULL, limits_visitor, &L);
    if (!L.found) return -1;
    const int n = c->cm.rst_info[plane].units_per_tile;
    RestUnitSearchInfo *rusi = (RestUnitSearchInfo *)calloc((size_t)n, sizeof(RestUnitSearchInfo));
    RestSearchCtxt rsc; memset(&rsc, 0, sizeof(rsc));
    c->cm.wn_filter_mode = (int8_t)wn_filter_mode;
    init_rsc_seg(&c->cdef.y, &c->src.y, &c->cm, NULL, plane, rusi, &c->dst.y, &rsc);
    rsc.tmpbuf = c->tmpbuf;
    rsc.tile_stripe0 = 0;
    const int is_uv = plane > 0;
    AV1PixelRect tile; tile.left = 0; tile.top = 0; tile.right = c->w >> is_uv; tile.bottom = c->h >> is_uv;
    g_log_n = 0;
    search_wiener_seg(&L.l, &tile, unit, &rsc);
    const int ntrials = g_log_n;
    g_log_n = -1;
    for (int i = 0; i < 3; i++) { out_taps[i] = rusi[unit].wiener.vfilter[i]; out_taps[3 + i] = rusi[unit].wiener.hfilter[i]; }
    *out_sse = rusi[unit].sse[RESTORE_WIENER];
    for (int t = 0; t < ntrials && t < max_trials; t++) memcpy(trials + 6 * t, g_log[t], sizeof(g_log[t]));
    free(rusi);
    return ntrials <= max_trials ? ntrials : -1;
}

/* rest_finish_search whole (all three planes).  in[plane]: units_per_tile records of what the searches left per unit; costs: rdmult,
 * wiener_restore_cost[2], sgrproj_restore_cost[2], switchable_restore_cost[3]; out_type[3]: frame_restoration_type per plane;
 * out[plane]: the unit records copy_unit_info filled (type; the Wiener taps of a Wiener unit, ep / xqd otherwise) */
typedef struct ref_lr_result { int64_t sse[3]; int32_t vfilter[3], hfilter[3], ep, xqd[2]; int32_t pad; } ref_lr_result;
int ref_lr_finish(Ctx *c, int wn_filter_mode, const int32_t costs[8], const ref_lr_result *const in[3], int32_t out_type[3], ref_lr_rec *const out[3]) {
    Macroblock *x = (Macroblock *)calloc(1, sizeof(Macroblock));
    PictureParentControlSet_t *ppcs = (PictureParentControlSet_t *)calloc(1, sizeof(PictureParentControlSet_t));
    x->rdmult = costs[0];
    x->wiener_restore_cost[0] = costs[1]; x->wiener_restore_cost[1] = costs[2];
    x->sgrproj_restore_cost[0] = costs[3]; x->sgrproj_restore_cost[1] = costs[4];
    for (int i = 0; i < 3; i++) x->switchable_restore_cost[i] = costs[5 + i];
    c->cm.wn_filter_mode = (int8_t)wn_filter_mode;
    c->cm.p_pcs_ptr = ppcs;
    for (int p = 0; p < 3; p++) {
        const int n = c->cm.rst_info[p].units_per_tile;
        RestUnitSearchInfo *r = (RestUnitSearchInfo *)calloc((size_t)n, sizeof(RestUnitSearchInfo));
        for (int u = 0; u < n; u++) {
            for (int k = 0; k < 3; k++) r[u].sse[k] = in[p][u].sse[k];
            ref_lr_rec rec; memset(&rec, 0, sizeof(rec));
            for (int k = 0; k < 3; k++) { rec.vfilter[k] = in[p][u].vfilter[k]; rec.hfilter[k] = in[p][u].hfilter[k]; }
            RestorationUnitInfo rui;
            fill_rui(&rui, &rec);
            r[u].wiener = rui.wiener_info;
            r[u].sgrproj.ep = in[p][u].ep; r[u].sgrproj.xqd[0] = in[p][u].xqd[0]; r[u].sgrproj.xqd[1] = in[p][u].xqd[1];
        }
        ppcs->rusi_picture[p] = r;
        memset(c->cm.rst_info[p].unit_info, 0, (size_t)n * sizeof(RestorationUnitInfo));
    }
    rest_finish_search(x, &c->cm);
    for (int p = 0; p < 3; p++) {
        const int n = c->cm.rst_info[p].units_per_tile;
        out_type[p] = (int32_t)c->cm.rst_info[p].frame_restoration_type;
        for (int u = 0; u < n; u++) {
            const RestorationUnitInfo *ui = &c->cm.rst_info[p].unit_info[u];
            memset(&out[p][u], 0, sizeof(ref_lr_rec));
            if (out_type[p] == RESTORE_NONE) continue;
            out[p][u].type = (int32_t)ui->restoration_type;
            if (ui->restoration_type == RESTORE_WIENER) {
                for (int k = 0; k < 3; k++) { out[p][u].vfilter[k] = ui->wiener_info.vfilter[k]; out[p][u].hfilter[k] = ui->wiener_info.hfilter[k]; }
            } else {
                out[p][u].ep = ui->sgrproj_info.ep; out[p][u].xqd[0] = ui->sgrproj_info.xqd[0]; out[p][u].xqd[1] = ui->sgrproj_info.xqd[1];
            }
        }
        free(ppcs->rusi_picture[p]);
    }
    c->cm.p_pcs_ptr = NULL;
    free(ppcs); free(x);
    return 0;
}

/* ref_lr_sgr.c - harness round the reference's self-guided parameter search, for tests/golden/make_golden_lr_sgr.py.  It takes
 * tests/c/ref_lr.c whole (#include: its context, its frames and, through it, the statics of EbRestorationPick.c) and is linked as
 * that file is, into oracle/_ref/libsvtref_lr_sgr.so.
 *
 * Every evaluation of the reference's walk goes through the dispatch pointers av1_lowbd_pixel_proj_error /
 * av1_highbd_pixel_proj_error: the harness puts a logging wrapper there that notes xq and the result and hands over to the flavour's
 * function. */
#include "ref_lr.c"

#define SGR_MAX_LOG 512
static int g_sgr_log_n = -1;                      /* -1: not logging */
static int64_t g_sgr_log[SGR_MAX_LOG][3];         /* xq[0], xq[1], the error */
static int64_t (*g_real_lowbd)(const uint8_t *, int32_t, int32_t, int32_t, const uint8_t *, int32_t, int32_t *, int32_t, int32_t *, int32_t, int32_t[2],
                               const sgr_params_type *);
static int64_t (*g_real_highbd)(const uint8_t *, int32_t, int32_t, int32_t, const uint8_t *, int32_t, int32_t *, int32_t, int32_t *, int32_t, int32_t[2],
                                const sgr_params_type *);

static void sgr_note(const int32_t xq[2], int64_t err) {
    if (g_sgr_log_n >= 0 && g_sgr_log_n < SGR_MAX_LOG) {
        g_sgr_log[g_sgr_log_n][0] = xq[0]; g_sgr_log[g_sgr_log_n][1] = xq[1]; g_sgr_log[g_sgr_log_n][2] = err;
    }
    if (g_sgr_log_n >= 0) g_sgr_log_n++;
}
static int64_t logged_lowbd(const uint8_t *src8, int32_t width, int32_t height, int32_t src_stride, const uint8_t *dat8, int32_t dat_stride, int32_t *flt0,
                            int32_t flt0_stride, int32_t *flt1, int32_t flt1_stride, int32_t xq[2], const sgr_params_type *params) {
    const int64_t e = g_real_lowbd(src8, width, height, src_stride, dat8, dat_stride, flt0, flt0_stride, flt1, flt1_stride, xq, params);
    sgr_note(xq, e);
    return e;
}
static int64_t logged_highbd(const uint8_t *src8, int32_t width, int32_t height, int32_t src_stride, const uint8_t *dat8, int32_t dat_stride, int32_t *flt0,
                             int32_t flt0_stride, int32_t *flt1, int32_t flt1_stride, int32_t xq[2], const sgr_params_type *params) {
    const int64_t e = g_real_highbd(src8, width, height, src_stride, dat8, dat_stride, flt0, flt0_stride, flt1, flt1_stride, xq, params);
    sgr_note(xq, e);
    return e;
}
static void set_sgr_flavour(int avx2) {
    set_flavour(avx2);
    get_proj_subspace = avx2 ? get_proj_subspace_avx2 : get_proj_subspace_c;
    g_real_lowbd = av1_lowbd_pixel_proj_error; g_real_highbd = av1_highbd_pixel_proj_error;
    av1_lowbd_pixel_proj_error = logged_lowbd; av1_highbd_pixel_proj_error = logged_highbd;
}

typedef struct SgrUnit { RestorationTileLimits l; const uint8_t *dgd, *src; int w, h, dgd_stride, src_stride, pu_w, pu_h; } SgrUnit;
/* the operands search_sgrproj_seg (:1681-1712) hands to search_selfguided_restoration */
static int sgr_unit(Ctx *c, int plane, int unit, SgrUnit *u) {
    Limits L; memset(&L, 0, sizeof(L)); L.want = unit;
    av1_foreach_rest_unit_in_frame(&c->cm, plane, NULL, limits_visitor, &L);
    if (!L.found) return -1;
    const int is_uv = plane > 0;
    u->l = L.l;
    u->dgd_stride = c->cdef.y.strides[is_uv]; u->src_stride = c->src.y.strides[is_uv];
    u->dgd = c->cdef.y.buffers[plane] + L.l.v_start * u->dgd_stride + L.l.h_start;
    u->src = c->src.y.buffers[plane] + L.l.v_start * u->src_stride + L.l.h_start;
    u->w = L.l.h_end - L.l.h_start; u->h = L.l.v_end - L.l.v_start;
    u->pu_w = RESTORATION_PROC_UNIT_SIZE >> is_uv; u->pu_h = RESTORATION_PROC_UNIT_SIZE >> is_uv;
    return 0;
}

/* search_sgrproj_seg for one unit: search_selfguided_restoration as it is called there, then try_restoration_unit_seg on its result
 * (ref_lr_try: at high bit depth the error is summed by the harness, as for every try of the fixture).  out = {ep, xqd[0], xqd[1]};
 * ep_cnt [16]: cm->sg_frame_ep_cnt, which the call increments */
int64_t ref_lr_sgr_search(Ctx *c, int flavour, int plane, int unit, const int8_t ref_ep[2], int sg_filter_mode, int32_t out[3], int32_t *ep_cnt) {
    set_sgr_flavour(flavour);
    SgrUnit u;
    if (sgr_unit(c, plane, unit, &u)) return -1;
    c->cm.sg_filter_mode = (int8_t)sg_filter_mode;
    c->cm.sg_ref_frame_ep[0] = ref_ep[0]; c->cm.sg_ref_frame_ep[1] = ref_ep[1];
    memcpy(c->cm.sg_frame_ep_cnt, ep_cnt, sizeof(c->cm.sg_frame_ep_cnt));
    const SgrprojInfo s = search_selfguided_restoration(u.dgd, u.w, u.h, u.dgd_stride, u.src, u.src_stride, c->hbd, c->bd, u.pu_w, u.pu_h, c->tmpbuf,
                                                        c->cm.sg_ref_frame_ep, c->cm.sg_frame_ep_cnt, get_sg_step(c->cm.sg_filter_mode));
    memcpy(ep_cnt, c->cm.sg_frame_ep_cnt, sizeof(c->cm.sg_frame_ep_cnt));
    out[0] = s.ep; out[1] = s.xqd[0]; out[2] = s.xqd[1];
    ref_lr_rec rec; memset(&rec, 0, sizeof(rec));
    rec.type = RESTORE_SGRPROJ; rec.ep = s.ep; rec.xqd[0] = s.xqd[0]; rec.xqd[1] = s.xqd[1];
    return ref_lr_try(c, flavour, plane, unit, &rec);
}

/* one round of search_selfguided_restoration's loop (:634-646) for one (unit, ep): apply_sgr, the dispatched get_proj_subspace,
 * encode_xq, finer_search_pixel_proj_error.  out = {exq[0], exq[1], start xqd[0], [1], final xqd[0], [1]}; *err: the walk's result;
 * trials [max_trials][3]: xq[0], xq[1] and the error of every evaluation in order; flt0 / flt1 (may be NULL): the filtered planes,
 * tightly packed w x h.  Returns the evaluations made, or -1 */
int ref_lr_sgr_ep(Ctx *c, int flavour, int plane, int unit, int ep, int32_t out[6], int64_t *err, int64_t *trials, int max_trials, int32_t *flt0_out,
                  int32_t *flt1_out) {
    set_sgr_flavour(flavour);
    SgrUnit u;
    if (sgr_unit(c, plane, unit, &u)) return -1;
    int32_t *flt0 = c->tmpbuf, *flt1 = flt0 + RESTORATION_UNITPELS_MAX;
    const int32_t flt_stride = ALIGN_POWER_OF_TWO(u.w, 3) + 8;      /* a multiple of 8 with room past the width, as the search's own */
    int32_t exq[2], exqd[2];
    apply_sgr(ep, u.dgd, u.w, u.h, u.dgd_stride, c->hbd, c->bd, u.pu_w, u.pu_h, flt0, flt1, flt_stride);
    aom_clear_system_state();
    const sgr_params_type *const params = &sgr_params[ep];
    get_proj_subspace(u.src, u.w, u.h, u.src_stride, u.dgd, u.dgd_stride, c->hbd, flt0, flt_stride, flt1, flt_stride, exq, params);
    aom_clear_system_state();
    encode_xq(exq, exqd, params);
    out[0] = exq[0]; out[1] = exq[1]; out[2] = exqd[0]; out[3] = exqd[1];
    g_sgr_log_n = 0;
    *err = finer_search_pixel_proj_error(u.src, u.w, u.h, u.src_stride, u.dgd, u.dgd_stride, c->hbd, flt0, flt_stride, flt1, flt_stride, 2, exqd, params);
    const int n = g_sgr_log_n;
    g_sgr_log_n = -1;
    out[4] = exqd[0]; out[5] = exqd[1];
    for (int t = 0; t < n && t < max_trials && t < SGR_MAX_LOG; t++) memcpy(trials + 3 * t, g_sgr_log[t], sizeof(g_sgr_log[t]));
    for (int y = 0; y < u.h; y++) {
        if (flt0_out && params->r[0] > 0) memcpy(flt0_out + (size_t)y * u.w, flt0 + (size_t)y * flt_stride, (size_t)u.w * sizeof(int32_t));
        if (flt1_out && params->r[1] > 0) memcpy(flt1_out + (size_t)y * u.w, flt1 + (size_t)y * flt_stride, (size_t)u.w * sizeof(int32_t));
    }
    return n <= max_trials && n <= SGR_MAX_LOG ? n : -1;
}

/* get_sg_step (:681-700) and the mid_ep / start_ep / end_ep lines of search_selfguided_restoration (:625-631) cannot be called on
 * their own, so the function is run whole on unit 0 of the luma plane with a wrapper in the av1_selfguided_restoration dispatch
 * pointer that notes the parameter set of every filter call: out = {lowest ep seen, highest ep seen + 1}, or {-1, -1} when the range
 * was empty.  Returns the number of different ep seen (the range has no holes when it equals out[1] - out[0]). */
static uint8_t g_ep_seen[SGRPROJ_PARAMS];
static void (*g_real_sgr)(const uint8_t *, int32_t, int32_t, int32_t, int32_t *, int32_t *, int32_t, int32_t, int32_t, int32_t);
static void noting_sgr(const uint8_t *dgd8, int32_t width, int32_t height, int32_t stride, int32_t *flt0, int32_t *flt1, int32_t flt_stride, int32_t sgr_params_idx,
                       int32_t bit_depth, int32_t highbd) {
    if (sgr_params_idx >= 0 && sgr_params_idx < SGRPROJ_PARAMS) g_ep_seen[sgr_params_idx] = 1;
    g_real_sgr(dgd8, width, height, stride, flt0, flt1, flt_stride, sgr_params_idx, bit_depth, highbd);
}
int ref_lr_sgr_ep_seen(Ctx *c, const int8_t ref_ep[2], int sg_filter_mode, int32_t out[2]) {
    int32_t cnt[SGRPROJ_PARAMS];
    memset(cnt, 0, sizeof(cnt));
    memset(g_ep_seen, 0, sizeof(g_ep_seen));
    set_sgr_flavour(0);
    g_real_sgr = av1_selfguided_restoration;
    av1_selfguided_restoration = noting_sgr;
    SgrUnit u;
    if (sgr_unit(c, 0, 0, &u)) return -1;
    c->cm.sg_filter_mode = (int8_t)sg_filter_mode;
    c->cm.sg_ref_frame_ep[0] = ref_ep[0]; c->cm.sg_ref_frame_ep[1] = ref_ep[1];
    const SgrprojInfo s = search_selfguided_restoration(u.dgd, u.w, u.h, u.dgd_stride, u.src, u.src_stride, c->hbd, c->bd, u.pu_w, u.pu_h, c->tmpbuf,
                                                        c->cm.sg_ref_frame_ep, cnt, get_sg_step(c->cm.sg_filter_mode));
    av1_selfguided_restoration = g_real_sgr;
    (void)s;
    int n = 0;
    out[0] = out[1] = -1;
    for (int ep = 0; ep < SGRPROJ_PARAMS; ep++)
        if (g_ep_seen[ep]) { if (out[0] < 0) out[0] = ep; out[1] = ep + 1; n++; }
    return n;
}

// lr_plan.h — what the loop-restoration calls (svt_hip_lr_apply_frame, svt_hip_lr_try_frame, svt_hip_lr_wiener_stats_frame) settle on
// the host before they enqueue: the unit grid (foreach_rest_unit_in_tile, EbRestoration.c:1331-1377; av1_alloc_restoration_struct,
// :198-235), the stripe grid (av1_loop_restoration_filter_unit, :1168-1236), the halo rule that stands in for the reference's
// boundary buffers, the checks, the launch shapes and the scratch size.
// Host only (no HIP header): tests/c/lr_plan_host.cpp compiles it with g++; the kernels (kernel_lr.h) call the same constexpr
// functions.
//
// The halo rule.  save_tile_row_boundary_lines (:1666) keeps, per stripe [y0, y1), the deblocked rows y0 - 2, y0 - 1 ("above", when
// the stripe is not the picture's first) and y1, y1 + 1 ("below", when y1 is not the picture's bottom); get_stripe_boundary_info
// (:342) says copy_above = not the first stripe, copy_below = not the last; setup_processing_stripe_boundary (:374, opt == 0) then
// writes buffer rows 0, 0, 1 above and 0, 1, 1 below.  Where nothing is copied the frame itself is read, which extend_frame (:276)
// has extended by three copies of its edge row.  So a halo row is one row of one of two pictures: lr_halo_row.  Both sides being
// multiples of 8 (4 in chroma), y1 < height implies y1 + 1 < height: the reference's one-line case (lines_to_save == 1, :1608)
// cannot occur, and other sides are refused.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "../../include/svt_hip_dsp.h"
#include "host_err.h"

namespace svthost {

constexpr int LR_THREADS = 256;
constexpr int LR_BORDER = 3;                                 // RESTORATION_BORDER: halo rows and columns of a stripe
constexpr int LR_PROC = 64, LR_OFFSET = 8;                   // RESTORATION_PROC_UNIT_SIZE, RESTORATION_UNIT_OFFSET (luma; >> ss_y)
constexpr uint32_t LR_MAX_SIDE = 65535, LR_MAX_PICS = 65535;
constexpr int LR_WIN = 7, LR_WIN2 = 49;
constexpr int LR_STATS_TILE = 64;                            // the statistics walk a unit in 64 x 64 tiles

constexpr int lr_clamp(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }
constexpr int lr_min(int a, int b) { return a < b ? a : b; }
constexpr int lr_max(int a, int b) { return a > b ? a : b; }

// the ranges of a record (EbRestoration.h:137-163, :107-110)
constexpr int kLrTapMin[3] = {-5, -23, -17}, kLrTapMax[3] = {10, 8, 46};
constexpr int kLrXqdMin[2] = {-96, -32}, kLrXqdMax[2] = {31, 95};

// ---- unit grid ------------------------------------------------------------------------------------------------------------------
// count_units_in_tile (:194): round to nearest, at least one
constexpr int lr_units(int unit_size, int size) { return lr_max((size + (unit_size >> 1)) / unit_size, 1); }
// the limits of unit i of n along one axis; off = 0 horizontally, RESTORATION_UNIT_OFFSET >> ss_y vertically
constexpr int lr_unit_start(int i, int unit_size, int off) { return i == 0 ? 0 : i * unit_size - off; }
constexpr int lr_unit_end(int i, int n, int unit_size, int off, int size) { return i == n - 1 ? size : (i + 1) * unit_size - off; }
// the unit a sample lies in
constexpr int lr_unit_of(int coord, int n, int unit_size, int off) { return lr_min((coord + off) / unit_size, n - 1); }

// ---- stripe grid ----------------------------------------------------------------------------------------------------------------
constexpr int lr_stripe_h(int ss) { return LR_PROC >> ss; }
constexpr int lr_stripe_off(int ss) { return LR_OFFSET >> ss; }
constexpr int lr_stripes(int height, int ss) { return (height + lr_stripe_off(ss) + lr_stripe_h(ss) - 1) / lr_stripe_h(ss); }
constexpr int lr_stripe_of(int y, int ss) { return (y + lr_stripe_off(ss)) / lr_stripe_h(ss); }
constexpr int lr_stripe_start(int s, int ss) { return lr_max(0, s * lr_stripe_h(ss) - lr_stripe_off(ss)); }
constexpr int lr_stripe_end(int s, int ss, int height) { return lr_min(height, (s + 1) * lr_stripe_h(ss) - lr_stripe_off(ss)); }

// the halo rule: row r (y0 - 3 .. y1 + 2) of the stripe [y0, y1) of a plane `height` rows high -> the row to read, and whether it is
// read from the deblocked picture (else from the CDEF output)
struct LrRow { int row; bool dblk; };
constexpr LrRow lr_halo_row(int r, int y0, int y1, int height) {
    if (r < y0) return y0 == 0 ? LrRow{0, false} : LrRow{lr_max(r, y0 - 2), true};
    if (r >= y1) return y1 == height ? LrRow{height - 1, false} : LrRow{lr_min(r, y1 + 1), true};
    return LrRow{r, false};
}
static_assert(lr_halo_row(53, 56, 120, 200).row == 54 && lr_halo_row(53, 56, 120, 200).dblk && lr_halo_row(55, 56, 120, 200).row == 55, "above");
static_assert(lr_halo_row(122, 56, 120, 200).row == 121 && lr_halo_row(120, 56, 120, 200).dblk && lr_halo_row(-2, 0, 56, 200).row == 0, "below");
static_assert(!lr_halo_row(-1, 0, 56, 200).dblk && lr_halo_row(201, 184, 200, 200).row == 199 && !lr_halo_row(200, 184, 200, 200).dblk, "edges");

// ---- one plane's geometry, as the kernels take it -------------------------------------------------------------------------------
struct LrPlane {
    int w, h, ss;                // the plane's sides; 1 for chroma
    int us, nh, nv;              // unit size and counts
    int tw;                      // tile width of the filter kernels: 64, or 32 for a unit size of 32 (a tile lies in one unit)
    int ntx, nstripes;
    uint32_t unit0;              // where the plane's records start inside a picture's block
};
inline bool lr_unit_size_ok(const uint32_t us[3]) {
    return (us[0] == 64 || us[0] == 128 || us[0] == 256) && (us[1] == us[0] || us[1] == us[0] / 2) && us[2] == us[1];
}
inline bool lr_geometry_ok(uint32_t width, uint32_t height, const uint32_t us[3], uint32_t npics) {
    if (width == 0 || height == 0 || (width & 7) || (height & 7) || width > LR_MAX_SIDE || height > LR_MAX_SIDE) return false;
    return us && lr_unit_size_ok(us) && npics >= 1 && npics <= LR_MAX_PICS;
}
inline LrPlane lr_plane(uint32_t width, uint32_t height, const uint32_t us[3], int plane) {
    LrPlane p{};
    p.ss = plane > 0;
    p.w = (int)(width >> p.ss); p.h = (int)(height >> p.ss);
    p.us = (int)us[plane];
    p.nh = lr_units(p.us, p.w); p.nv = lr_units(p.us, p.h);
    p.tw = p.us >= 64 ? 64 : 32;
    p.ntx = (p.w + p.tw - 1) / p.tw;
    p.nstripes = lr_stripes(p.h, p.ss);
    p.unit0 = 0;
    for (int i = 0; i < plane; i++) p.unit0 += (uint32_t)(lr_units((int)us[i], (int)(width >> (i > 0))) * lr_units((int)us[i], (int)(height >> (i > 0))));
    return p;
}
inline uint32_t lr_units_per_pic(uint32_t width, uint32_t height, const uint32_t us[3]) {
    const LrPlane p = lr_plane(width, height, us, 2);
    return p.unit0 + (uint32_t)(p.nh * p.nv);
}
// tiles a unit of this plane has at the most (the grids of try and statistics): the last unit of a row is below unit_size * 3 / 2
// wide, the last of a column below unit_size * 3 / 2 plus the offset high and starts on a stripe boundary
inline uint32_t lr_try_tiles(const LrPlane& p) {
    const int wmax = lr_min(p.w, p.us * 3 / 2), hmax = lr_min(p.h, p.us * 3 / 2 + lr_stripe_off(p.ss));
    return (uint32_t)((wmax + p.tw - 1) / p.tw) * (uint32_t)((hmax + lr_stripe_h(p.ss) - 1) / lr_stripe_h(p.ss) + 1);
}
inline uint32_t lr_stats_tiles(const LrPlane& p) {
    const int wmax = lr_min(p.w, p.us * 3 / 2), hmax = lr_min(p.h, p.us * 3 / 2 + lr_stripe_off(p.ss));
    return (uint32_t)((wmax + LR_STATS_TILE - 1) / LR_STATS_TILE) * (uint32_t)((hmax + LR_STATS_TILE - 1) / LR_STATS_TILE);
}
// per unit its average (uint32)
inline size_t lr_stats_scratch_bytes(uint32_t width, uint32_t height, const uint32_t us[3], uint32_t npics) {
    if (!lr_geometry_ok(width, height, us, npics)) return 0;
    return ((size_t)lr_units_per_pic(width, height, us) * npics * sizeof(uint32_t) + 7) & ~(size_t)7;
}

// bytes a stack of planes spans, for the overlap check
inline uint64_t lr_span(uint32_t rows, uint32_t stride, uint32_t width, uint32_t npics, uint64_t pitch, int bytes) {
    return ((uint64_t)(npics - 1) * pitch + (uint64_t)(rows - 1) * stride + width) * (uint64_t)bytes;
}

inline int lr_record_check(const svt_hip_lr_unit& u, int frame_type) {
    if (u.type < 0 || u.type > 2) return set_err(SVT_HIP_ERR_INVALID, "unit type %d (0 .. 2)", u.type);
    if (u.type != 0 && frame_type >= 0 && frame_type != 3 && frame_type != u.type)
        return set_err(SVT_HIP_ERR_INVALID, "unit type %d under frame type %d", u.type, frame_type);
    for (int i = 0; i < 3; i++)
        if (u.vfilter[i] < kLrTapMin[i] || u.vfilter[i] > kLrTapMax[i] || u.hfilter[i] < kLrTapMin[i] || u.hfilter[i] > kLrTapMax[i])
            return set_err(SVT_HIP_ERR_INVALID, "Wiener tap %d: %d / %d (%d .. %d)", i, u.vfilter[i], u.hfilter[i], kLrTapMin[i], kLrTapMax[i]);
    if (u.ep < 0 || u.ep > 15) return set_err(SVT_HIP_ERR_INVALID, "ep %d (0 .. 15)", u.ep);
    for (int i = 0; i < 2; i++)
        if (u.xqd[i] < kLrXqdMin[i] || u.xqd[i] > kLrXqdMax[i]) return set_err(SVT_HIP_ERR_INVALID, "xqd[%d] = %d (%d .. %d)", i, u.xqd[i], kLrXqdMin[i], kLrXqdMax[i]);
    return SVT_HIP_OK;
}

enum { LR_APPLY = 0, LR_TRY = 1, LR_STATS = 2 };
inline int lr_check(const svt_hip_lr_pic* p, int what, const int32_t* frame_type, const svt_hip_lr_unit* h_units, uint32_t nunits) {
    if (!p) return set_err(SVT_HIP_ERR_INVALID, "NULL picture descriptor");
    if (what < LR_APPLY || what > LR_STATS) return set_err(SVT_HIP_ERR_INVALID, "what %d (0 apply, 1 try, 2 statistics)", what);
    if (p->bit_depth != 8 && p->bit_depth != 10) return set_err(SVT_HIP_ERR_INVALID, "bit depth %d (8 or 10)", p->bit_depth);
    if (p->npics < 1 || p->npics > LR_MAX_PICS) return set_err(SVT_HIP_ERR_INVALID, "npics %u (1 .. %u)", p->npics, LR_MAX_PICS);
    if (!lr_geometry_ok(p->width, p->height, p->unit_size, p->npics))
        return set_err(SVT_HIP_ERR_INVALID, "picture %u x %u (non-zero multiples of 8, at most %u) or unit_size %u / %u / %u (luma 64, 128, 256; chroma equal or half)",
                       p->width, p->height, LR_MAX_SIDE, p->unit_size[0], p->unit_size[1], p->unit_size[2]);
    const int bytes = p->bit_depth == 8 ? 1 : 2;
    for (int i = 0; i < 3; i++) {
        const uint32_t w = i ? p->width / 2 : p->width;
        if (!p->d_cdef[i] || p->cdef_stride[i] < w || ((uintptr_t)p->d_cdef[i] & (bytes - 1)))
            return set_err(SVT_HIP_ERR_INVALID, "plane %d: CDEF picture NULL, misaligned or stride below the width", i);
        if (what != LR_STATS && (!p->d_dblk[i] || p->dblk_stride[i] < w || ((uintptr_t)p->d_dblk[i] & (bytes - 1))))
            return set_err(SVT_HIP_ERR_INVALID, "plane %d: deblocked picture NULL, misaligned or stride below the width", i);
        if (what != LR_APPLY && (!p->d_src[i] || p->src_stride[i] < w || ((uintptr_t)p->d_src[i] & (bytes - 1))))
            return set_err(SVT_HIP_ERR_INVALID, "plane %d: source NULL, misaligned or stride below the width", i);
        if (what == LR_APPLY && (!p->d_dst[i] || p->dst_stride[i] < w || ((uintptr_t)p->d_dst[i] & (bytes - 1))))
            return set_err(SVT_HIP_ERR_INVALID, "plane %d: output NULL, misaligned or stride below the width", i);
    }
    if (what == LR_APPLY) {
        if (!frame_type) return set_err(SVT_HIP_ERR_INVALID, "NULL frame_type");
        // the pictures of a stack may not share output samples: workgroups of different pictures would race on them
        for (int i = 0; i < 3 && p->npics > 1; i++) {
            const uint32_t w = i ? p->width / 2 : p->width, h = i ? p->height / 2 : p->height;
            if (p->dst_pitch[i] < (uint64_t)(h - 1) * p->dst_stride[i] + w)
                return set_err(SVT_HIP_ERR_INVALID, "plane %d: dst_pitch %llu below one picture (%llu samples)", i, (unsigned long long)p->dst_pitch[i],
                               (unsigned long long)((uint64_t)(h - 1) * p->dst_stride[i] + w));
        }
        for (int i = 0; i < 3; i++)
            if (frame_type[i] < 0 || frame_type[i] > 3) return set_err(SVT_HIP_ERR_INVALID, "frame_type[%d] = %d (0 .. 3)", i, frame_type[i]);
        for (int i = 0; i < 3; i++)
            for (int j = 0; j < 6; j++) {
                const uint32_t wi = i ? p->width / 2 : p->width, hi = i ? p->height / 2 : p->height;
                const int jp = j % 3;
                const uint32_t wj = jp ? p->width / 2 : p->width, hj = jp ? p->height / 2 : p->height;
                const uintptr_t d0 = (uintptr_t)p->d_dst[i], d1 = d0 + lr_span(hi, p->dst_stride[i], wi, p->npics, p->dst_pitch[i], bytes);
                const uintptr_t r0 = (uintptr_t)(j < 3 ? p->d_cdef[jp] : p->d_dblk[jp]);
                const uintptr_t r1 = r0 + (j < 3 ? lr_span(hj, p->cdef_stride[jp], wj, p->npics, p->cdef_pitch[jp], bytes)
                                                 : lr_span(hj, p->dblk_stride[jp], wj, p->npics, p->dblk_pitch[jp], bytes));
                if (d0 < r1 && r0 < d1) return set_err(SVT_HIP_ERR_INVALID, "d_dst[%d] overlaps %s[%d]", i, j < 3 ? "d_cdef" : "d_dblk", jp);
            }
    }
    if (h_units) {
        if (nunits != lr_units_per_pic(p->width, p->height, p->unit_size))
            return set_err(SVT_HIP_ERR_INVALID, "%u records of %u", nunits, lr_units_per_pic(p->width, p->height, p->unit_size));
        for (int pl = 0; pl < 3; pl++) {
            const LrPlane g = lr_plane(p->width, p->height, p->unit_size, pl);
            for (int k = 0; k < g.nh * g.nv; k++)
                if (int rc = lr_record_check(h_units[g.unit0 + k], what == LR_APPLY ? frame_type[pl] : -1)) return rc;
        }
    }
    return SVT_HIP_OK;
}

inline int lr_try_check(const svt_hip_lr_pic* p, const void* d_cand, uint32_t ncand, const void* d_sse) {
    if (int rc = lr_check(p, LR_TRY, nullptr, nullptr, 0)) return rc;
    if (ncand == 0 || ncand > 0x7fffffu) return set_err(SVT_HIP_ERR_INVALID, "ncand %u (1 .. %u)", ncand, 0x7fffffu);
    if (!d_cand || ((uintptr_t)d_cand & 3)) return set_err(SVT_HIP_ERR_INVALID, "NULL or misaligned d_cand");
    if (!d_sse || ((uintptr_t)d_sse & 7)) return set_err(SVT_HIP_ERR_INVALID, "NULL or misaligned d_sse (8 bytes)");
    return SVT_HIP_OK;
}

inline int lr_stats_check(const svt_hip_lr_pic* p, const int32_t* win, const void* d_M, const void* d_H, const void* d_scratch, size_t scratch_bytes) {
    if (int rc = lr_check(p, LR_STATS, nullptr, nullptr, 0)) return rc;
    if (!win) return set_err(SVT_HIP_ERR_INVALID, "NULL wiener_win");
    for (int i = 0; i < 3; i++)
        if (win[i] != 7 && win[i] != 5 && win[i] != 3) return set_err(SVT_HIP_ERR_INVALID, "wiener_win[%d] = %d (7, 5 or 3)", i, win[i]);
    if (!d_M || ((uintptr_t)d_M & 7) || !d_H || ((uintptr_t)d_H & 7)) return set_err(SVT_HIP_ERR_INVALID, "NULL or misaligned d_M / d_H (8 bytes)");
    const size_t need = lr_stats_scratch_bytes(p->width, p->height, p->unit_size, p->npics);
    if (!d_scratch || ((uintptr_t)d_scratch & 7) || scratch_bytes < need)
        return set_err(SVT_HIP_ERR_INVALID, "scratch: NULL, misaligned or %zu bytes of %zu", scratch_bytes, need);
    if ((uint64_t)lr_units_per_pic(p->width, p->height, p->unit_size) * p->npics > 0x7fffffu) return set_err(SVT_HIP_ERR_INVALID, "too many units");
    return SVT_HIP_OK;
}

}  // namespace svthost

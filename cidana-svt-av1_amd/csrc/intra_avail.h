// intra_avail.h — the neighbour availability of av1_predict_intra_block (EbIntraPrediction.c:4078-4333 / :4336-4566 with has_top_right
// :1567 and has_bottom_left :1755), stated once for the host entry points (svt_hip_intra_has_top_right, svt_hip_intra_has_bottom_left,
// svt_hip_intra_neighbor_px, host_tables.cpp) and for the device walk of svt_hip_intra_encode_frame (kernel_intra_encode.h).
// Plain C++17 without tables in memory: the block sizes' sides ride in two packed constants, a transform block comes as its sides in
// samples, so the same functions compile for the host and for the device.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define SVT_AVAIL_HD __host__ __device__ inline
#else
#define SVT_AVAIL_HD inline
#endif

namespace svtavail {

// block_size order of the AV1 enum: 4X4 4X8 8X4 8X8 8X16 16X8 16X16 16X32 32X16 32X32 32X64 64X32 64X64 64X128 128X64 128X128 4X16 16X4
// 8X32 32X8 16X64 64X16; log2 of the sides in 4-sample units, a nibble per block size
constexpr uint64_t kWlLo = 0x5544433322211100ull, kWlHi = 0x423120ull;      // {0,0,1,1,1,2,2,2,3,3,3,4,4,4,5,5} {0,2,1,3,2,4}
constexpr uint64_t kHlLo = 0x5454343232121010ull, kHlHi = 0x241302ull;      // {0,1,0,1,2,1,2,3,2,3,4,3,4,5,4,5} {2,0,3,1,4,2}
SVT_AVAIL_HD int blk_wl(int bsize) { return (int)(((bsize < 16 ? kWlLo >> (4 * bsize) : kWlHi >> (4 * (bsize - 16)))) & 15u); }
SVT_AVAIL_HD int blk_hl(int bsize) { return (int)(((bsize < 16 ? kHlLo >> (4 * bsize) : kHlHi >> (4 * (bsize - 16)))) & 15u); }
enum { kPartVertA = 6, kPartVertB = 7 };

// Coding-order key of the 4x4 unit (x, y) of a 128x128 superblock when it is coded in blocks of 2^bwl x 2^bhl units: the
// Morton (Z) code of the enclosing square of side max(bw, bh) - with `vert` the last split is visited TL, BL, TR, BR, as
// PARTITION_VERT_A / VERT_B do - followed by the index of the rectangular block inside that square (left to right for tall
// blocks, top to bottom for wide ones).  A neighbour is already coded exactly when its key is smaller.
SVT_AVAIL_HD uint32_t order_key(int x, int y, int bwl, int bhl, bool vert) {
    const int sql = bwl > bhl ? bwl : bhl;
    const uint32_t sx = (uint32_t)x >> sql, sy = (uint32_t)y >> sql;
    uint32_t key = 0;
    for (int b = 5; b >= 1; b--) key = (key << 2) | (((sy >> b) & 1u) << 1) | ((sx >> b) & 1u);
    key = (key << 2) | (vert ? (((sx & 1u) << 1) | (sy & 1u)) : (((sy & 1u) << 1) | (sx & 1u)));
    const uint32_t part = bwl < bhl ? (((uint32_t)x >> bwl) & ((1u << (sql - bwl)) - 1u)) : (((uint32_t)y >> bhl) & ((1u << (sql - bhl)) - 1u));
    return (key << 2) | part;
}
SVT_AVAIL_HD bool args_ok(int sb_mi, int bsize, int partition) {
    if ((sb_mi != 16 && sb_mi != 32) || bsize < 0 || bsize >= 22 || partition < 0 || partition > 9) return false;
    // the VERT_A / VERT_B order exists for squares >= 8x8 and tall rectangles only (has_tr_vert_tables, :1536-1550)
    if ((partition == kPartVertA || partition == kPartVertB) && (bsize == 0 || bsize >= 16 || blk_wl(bsize) > blk_hl(bsize))) return false;
    return true;
}

// txw: the transform block's width in samples
SVT_AVAIL_HD int has_top_right(int sb_mi, int bsize, int mi_row, int mi_col, int top_available, int right_available, int partition, int txw,
                               int row_off, int col_off, int ss_x, int ss_y) {
    if (!top_available || !right_available) return 0;
    const int bwl = blk_wl(bsize), bhl = blk_hl(bsize);
    const int plane_bw_unit = ((1 << bwl) >> ss_x) > 1 ? ((1 << bwl) >> ss_x) : 1;
    const int tr_units = txw >> 2;
    if (row_off > 0) {                                   // only the columns to the right inside the block matter
        if (bwl > 4) {                                   // 128-wide blocks are coded as 64-wide halves
            if (row_off == (16 >> ss_y) && col_off + tr_units == (16 >> ss_x)) return 1;
            const int u64 = 16 >> ss_x;
            return col_off % u64 + tr_units < u64;
        }
        return col_off + tr_units < plane_bw_unit;
    }
    if (col_off + tr_units < plane_bw_unit) return 1;    // still inside the block above
    const int brow = (mi_row & (sb_mi - 1)) >> bhl, bcol = (mi_col & (sb_mi - 1)) >> bwl;
    if (brow == 0) return 1;                             // above superblock row: coded
    if (((bcol + 1) << bwl) >= sb_mi) return 0;          // right superblock: not coded yet
    const bool vert = (partition == kPartVertA || partition == kPartVertB) && bwl == bhl;
    const int x = bcol << bwl, y = brow << bhl;
    return order_key(x + (1 << bwl), y - 1, bwl, bhl, vert) < order_key(x, y, bwl, bhl, vert);
}

// txh: the transform block's height in samples
SVT_AVAIL_HD int has_bottom_left(int sb_mi, int bsize, int mi_row, int mi_col, int bottom_available, int left_available, int partition, int txh,
                                 int row_off, int col_off, int ss_x, int ss_y) {
    if (!bottom_available || !left_available) return 0;
    const int bwl = blk_wl(bsize), bhl = blk_hl(bsize);
    const int th_units = txh >> 2;
    if (bwl > 4 && col_off > 0) {
        const int u64 = 16 >> ss_x;
        if (col_off % u64 == 0) {                        // left edge of the right 64-wide half: the left half is coded
            const int h64 = 16 >> ss_y, bh_units = (1 << bhl) >> ss_y;
            return row_off % h64 + th_units < (bh_units < h64 ? bh_units : h64);
        }
    }
    if (col_off > 0) return 0;                           // below-left is inside this block: not coded yet
    const int plane_bh_unit = ((1 << bhl) >> ss_y) > 1 ? ((1 << bhl) >> ss_y) : 1;
    if (row_off + th_units < plane_bh_unit) return 1;    // still beside the block on the left
    const int brow = (mi_row & (sb_mi - 1)) >> bhl, bcol = (mi_col & (sb_mi - 1)) >> bwl;
    if (bcol == 0)                                       // left superblock: coded down to its bottom edge only
        return ((brow << bhl) >> ss_y) + row_off + th_units < (sb_mi >> ss_y);
    if (((brow + 1) << bhl) >= sb_mi) return 0;          // bottom superblock row: not coded yet
    const bool vert = (partition == kPartVertA || partition == kPartVertB) && bwl == bhl;
    const int x = bcol << bwl, y = brow << bhl;
    return order_key(x - 1, y + (1 << bhl), bwl, bhl, vert) < order_key(x, y, bwl, bhl, vert);
}

// what av1_predict_intra_block hands build_intra_predictors for one transform block (txw x txh samples at (col_off, row_off) units inside
// the wpx x hpx plane block of the block at (bl_org_x_pict, bl_org_y_pict), 4:2:0): the four sample counts, and whether the above / left
// mode-info neighbours exist (what get_filt_type may consult).  tile: {mi_row_start, mi_row_end, mi_col_start, mi_col_end}.
struct Pos {
    int sb_mi, bsize, partition, plane, is_16bit, mi_rows, mi_cols, bl_org_x_pict, bl_org_y_pict, col_off, row_off, wpx, hpx, txw, txh;
    int tile_mi_row_start, tile_mi_row_end, tile_mi_col_start, tile_mi_col_end;
};
struct Px { int n_top, n_topright, n_left, n_bottomleft, up, left; };
SVT_AVAIL_HD bool neighbor_px(const Pos& p, Px& o) {
    const int mirow = p.bl_org_y_pict >> 2, micol = p.bl_org_x_pict >> 2;
    const int ss = p.plane ? 1 : 0;                       // 4:2:0
    // the 8-bit function predicts inside a one-tile picture; the 16-bit one inside the given tile
    const int r0 = p.is_16bit ? p.tile_mi_row_start : 0, r1 = p.is_16bit ? p.tile_mi_row_end : p.mi_rows;
    const int c0 = p.is_16bit ? p.tile_mi_col_start : 0, c1 = p.is_16bit ? p.tile_mi_col_end : p.mi_cols;
    const int bw = 1 << blk_wl(p.bsize), bh = 1 << blk_hl(p.bsize);
    int up = mirow > r0, left = micol > c0;
    if (ss && bw < 2) left = (micol - 1) > p.tile_mi_col_start;      // sub-8x8 chroma: the luma block one further out (:4176-4179)
    if (ss && bh < 2) up = (mirow - 1) > p.tile_mi_row_start;
    const int txw = p.txw, txh = p.txh;
    const int have_top = p.row_off || up, have_left = p.col_off || left;
    // distance from the transform block's right / bottom edge to the picture's
    const int xr = (((p.mi_cols - bw - micol) * 32) >> (3 + ss)) + (p.wpx - (p.col_off << 2) - txw);
    const int yd = (((p.mi_rows - bh - mirow) * 32) >> (3 + ss)) + (p.hpx - (p.row_off << 2) - txh);
    const int right_av = micol + ((p.col_off + (txw >> 2)) << ss) < c1;
    const int bottom_av = yd > 0 && (mirow + ((p.row_off + (txh >> 2)) << ss) < r1);
    int bs = p.bsize;                                     // scale_chroma_bsize (:3619): chroma of sub-8x8 luma blocks is predicted as 8x8 / 8x16 / 16x8
    if (ss) bs = (bs <= 2) ? 3 : (bs == 16 ? 4 : (bs == 17 ? 5 : bs));
    const int tr = has_top_right(p.sb_mi, bs, mirow, micol, have_top, right_av, p.partition, txw, p.row_off, p.col_off, ss, ss);
    const int bl = has_bottom_left(p.sb_mi, bs, mirow, micol, bottom_av, have_left, p.partition, txh, p.row_off, p.col_off, ss, ss);
    o.n_top = have_top ? (txw < xr + txw ? txw : xr + txw) : 0; o.n_topright = tr > 0 ? (txw < xr ? txw : xr) : 0;
    o.n_left = have_left ? (txh < yd + txh ? txh : yd + txh) : 0; o.n_bottomleft = bl > 0 ? (txh < yd ? txh : yd) : 0;
    o.up = up; o.left = left;
    return o.n_top >= 0 && o.n_left >= 0 && o.n_topright >= 0 && o.n_bottomleft >= 0;      // else: outside the picture (:3713 asserts)
}

}  // namespace svtavail

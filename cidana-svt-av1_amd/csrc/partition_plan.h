// partition_plan.h — what svt_hip_partition_decide_frame settles on the host before it enqueues: the checks, the launch shape, and the
// block geometry of a 64x64 superblock in md-scan order, built at compile time from the scan rule (EbUtility.c:782-917): a square of
// size S at (x, y) lists the blocks of its shapes (nine for 64 / 32 / 16, three for 8, one for 4), each block a rectangle in quarters of S,
// then its four quadrants in Z order, the fourth being the last quadrant.  Host only (no HIP header): tests/c/partition_plan_host.cpp
// compiles it with g++; the kernel's device table (kernel_partition.h) is initialised from the same constexpr builder.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "../../include/svt_hip_dsp.h"
#include "av1_geom.h"
#include "host_err.h"

namespace svthost {

constexpr int PART_BLOCKS = SVT_HIP_SB_BLOCKS, PART_SQUARES = SVT_HIP_SB_SQUARES, PART_MAX_FINAL = SVT_HIP_SB_MAX_FINAL;
constexpr int PART_THREADS = 256, PART_WAVES = PART_THREADS / 64;      // one wave per superblock
constexpr uint32_t PART_MAX_NSB = 0x80000000u / PART_SQUARES;          // nsb * 341 stays below 2^31
constexpr int PART_SHAPES = 9;
constexpr int PART_NO_PARENT = 0xFFFF;

// a shape's blocks as rectangles in quarters of the square: x | y << 4 | w << 8 | h << 12; 0: no such block
constexpr uint16_t part_rect(int x, int y, int w, int h) { return (uint16_t)(x | y << 4 | w << 8 | h << 12); }
constexpr uint16_t kPartRects[PART_SHAPES][4] = {
    {part_rect(0, 0, 4, 4), 0, 0, 0},                                                                   // N
    {part_rect(0, 0, 4, 2), part_rect(0, 2, 4, 2), 0, 0},                                               // H: top, bottom
    {part_rect(0, 0, 2, 4), part_rect(2, 0, 2, 4), 0, 0},                                               // V: left, right
    {part_rect(0, 0, 2, 2), part_rect(2, 0, 2, 2), part_rect(0, 2, 4, 2), 0},                           // HA: the top half split
    {part_rect(0, 0, 4, 2), part_rect(0, 2, 2, 2), part_rect(2, 2, 2, 2), 0},                           // HB: the bottom half split
    {part_rect(0, 0, 2, 2), part_rect(0, 2, 2, 2), part_rect(2, 0, 2, 4), 0},                           // VA: the left half split
    {part_rect(0, 0, 2, 4), part_rect(2, 0, 2, 2), part_rect(2, 2, 2, 2), 0},                           // VB: the right half split
    {part_rect(0, 0, 4, 1), part_rect(0, 1, 4, 1), part_rect(0, 2, 4, 1), part_rect(0, 3, 4, 1)},       // H4
    {part_rect(0, 0, 1, 4), part_rect(1, 0, 1, 4), part_rect(2, 0, 1, 4), part_rect(3, 0, 1, 4)},       // V4
};
constexpr int part_shapes_of(int sq_size) { return sq_size >= 16 ? 9 : (sq_size == 8 ? 3 : 1); }
constexpr int part_totns(int shape) { return shape < 1 ? 1 : (shape < 3 ? 2 : (shape < 7 ? 3 : 4)); }

struct PartSquare { uint16_t mds, parent; uint8_t depth, x, y, last_quadrant; };      // parent: square index, PART_NO_PARENT at the root
struct PartGeomTab {
    svt_hip_blk_geom blk[PART_BLOCKS];
    uint16_t sq_of[PART_BLOCKS];           // the square index (0 .. 340, mds order) of a block's square
    PartSquare sq[PART_SQUARES];
    int nblk, nsq;
};

constexpr void part_scan(PartGeomTab& T, int sq_size, int x, int y, int depth, int last_quadrant, int parent) {
    const int sqi = T.nblk, s = T.nsq++, q = sq_size / 4;
    T.sq[s] = PartSquare{(uint16_t)sqi, (uint16_t)parent, (uint8_t)depth, (uint8_t)x, (uint8_t)y, (uint8_t)last_quadrant};
    int d1i = 0;
    for (int shape = 0; shape < part_shapes_of(sq_size); shape++) {
        for (int nsi = 0; nsi < part_totns(shape); nsi++) {
            const int r = kPartRects[shape][nsi];
            svt_hip_blk_geom g{};
            g.sqi_mds = (uint16_t)sqi; g.shape = (uint8_t)shape; g.depth = (uint8_t)depth; g.nsi = (uint8_t)nsi; g.totns = (uint8_t)part_totns(shape);
            g.d1i = (uint8_t)d1i++; g.sq_size = (uint8_t)sq_size; g.is_last_quadrant = (uint8_t)last_quadrant;
            g.origin_x = (uint8_t)(x + q * (r & 15)); g.origin_y = (uint8_t)(y + q * (r >> 4 & 15));
            g.bwidth = (uint8_t)(q * (r >> 8 & 15)); g.bheight = (uint8_t)(q * (r >> 12 & 15));
            g.bsize = (uint8_t)bsize_of(g.bwidth, g.bheight);
            // chroma: a 4x4 carries it in the last quadrant only; a block with a side of 4 shares its chroma block with its neighbours,
            // and the last of each group of 2 (one side 4) or 4 (both) carries it
            g.has_uv = 1;
            if (g.bwidth == 4 && g.bheight == 4) g.has_uv = (uint8_t)last_quadrant;
            else if (g.bwidth == 4 || g.bheight == 4) {
                const int same = (g.bwidth == 4 ? 2 : 1) * (g.bheight == 4 ? 2 : 1);
                g.has_uv = nsi == same - 1 || nsi == 2 * same - 1;
            }
            T.sq_of[T.nblk] = (uint16_t)s;
            T.blk[T.nblk++] = g;
        }
    }
    if (sq_size > 4) {
        const int h = sq_size / 2;
        part_scan(T, h, x, y, depth + 1, 0, s);
        part_scan(T, h, x + h, y, depth + 1, 0, s);
        part_scan(T, h, x, y + h, depth + 1, 0, s);
        part_scan(T, h, x + h, y + h, depth + 1, 1, s);
    }
}
constexpr PartGeomTab part_geom_tab() {
    PartGeomTab T{};
    part_scan(T, 64, 0, 0, 0, 0, PART_NO_PARENT);
    return T;
}

// workgroups of a call: PART_WAVES superblocks each, the last one partial
inline uint32_t partition_grid(uint32_t nsb) { return (nsb + PART_WAVES - 1) / PART_WAVES; }

inline int partition_check(const svt_hip_partition_args* a) {
    if (!a) return set_err(SVT_HIP_ERR_INVALID, "NULL arguments");
    if (a->nsb == 0 || a->nsb > PART_MAX_NSB) return set_err(SVT_HIP_ERR_INVALID, "nsb %u (1 .. %u)", a->nsb, PART_MAX_NSB);
    if (a->pic_width == 0 || a->pic_height == 0) return set_err(SVT_HIP_ERR_INVALID, "picture %u x %u", a->pic_width, a->pic_height);
    if (!a->d_sb || !a->d_partition_bits || !a->d_sq || !a->d_final_count || !a->d_final) return set_err(SVT_HIP_ERR_INVALID, "NULL member");
    if (a->nleaves > 0 && (!a->d_leaf || a->nsrc == 0)) return set_err(SVT_HIP_ERR_INVALID, "NULL d_leaf or nsrc 0 with nleaves %u", a->nleaves);
    if ((a->d_decision != nullptr) == (a->d_cost != nullptr)) return set_err(SVT_HIP_ERR_INVALID, "exactly one of d_decision / d_cost");
    if (a->d_final_decision && !a->d_decision) return set_err(SVT_HIP_ERR_INVALID, "d_final_decision without d_decision");
    const uintptr_t a8 = (uintptr_t)a->d_decision | (uintptr_t)a->d_cost | (uintptr_t)a->d_sq | (uintptr_t)a->d_final_decision;
    const uintptr_t a4 = (uintptr_t)a->d_sb | (uintptr_t)a->d_leaf | (uintptr_t)a->d_partition_bits | (uintptr_t)a->d_final_count | (uintptr_t)a->d_final;
    if ((a8 & 7) || (a4 & 3))
        return set_err(SVT_HIP_ERR_INVALID, "misaligned buffer (d_decision / d_cost / d_sq / d_final_decision 8 bytes, the others 4)");
    return SVT_HIP_OK;
}

}  // namespace svthost

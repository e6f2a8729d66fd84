// kernel_partition.h — partition_kernel: the d1 / d2 partition decision of mode_decision_sb (EbProductCodingLoop.c:3375-3502) around
// md_encode_block, and the block list of the encode pass (EbCodingLoop.c:2571-2589, :3618-3621), one wave per 64x64 superblock.
//
// One wave owns one superblock; tiles are per wave, no barrier between waves.  A wave keeps in LDS the superblock's 1 101 costs, each
// block's entry number (0: not listed), per-square bytes and the src of the final blocks: 15.2 KB, 60.6 KB per workgroup of four.
//   load    lanes stride the leaf list: cost through src into cost[mds], the entry number; a PART_N entry also its square's flags and
//           contexts.  d1_blocks_accumlated of entry i is i minus the index of the last PART_N entry at or before it, plus 1 (i + 1
//           when there is none): a ballot per 64 entries and a wave-uniform carry.  The entry whose count equals its tot_d1_blocks
//           marks its square as the one d2 is called on.
//   d1      lane per square, shapes in ascending order: d1_non_square_block_decision (EbFullLoop.c:1876-1898).
//   d2      level by level, the 8x8 parents first, the root last, lanes over the parents of the level.  The sequential loop compares a
//           parent when a climb (d2_inter_depth_block_decision, :2037-2103) reaches its fourth child: either the climb begins there (d2
//           called on the child with split_flag 0) or it passed through it (the child was compared itself: the climb goes on whatever a
//           comparison gives).  Everything a comparison at a parent reads was final before it: the parent's own d1 (its entries come
//           before its children's), the first three children's subtrees (all their entries come before the fourth child's) and the
//           fourth child's, whose last comparison is the one the climb came from.  A comparison writes its parent only.  So the parents
//           of one level are independent and a level needs only the levels below: the level order gives the loop's result.  One bit
//           per square carries "this climb began at a 4x4" (compute_depth_costs tests the LAST LEAF's block size before it adds the
//           children's PARTITION_NONE rates); the I-slice root keeps current_depth_cost of the climb's previous level.
//   emit    a square is coded when its own part is not PARTITION_SPLIT and every ancestor's is; a wave prefix sum over the squares in
//           mds order (their coding order) gives each its slot.  Then the decision records, nine 8-byte words per final block.
// Every index from device data is clamped (mds to 1 100, src to nsrc - 1, the leaf range to nleaves and 1 101 entries).
#pragma once
#include "dev_common.h"
#include "kernel_final_list.h"
#include "partition_plan.h"

namespace svtdev {

constexpr int PT_THREADS = svthost::PART_THREADS, PT_WAVES = svthost::PART_WAVES;
constexpr int PT_BLOCKS = svthost::PART_BLOCKS, PT_SQUARES = svthost::PART_SQUARES, PT_MAX_FINAL = svthost::PART_MAX_FINAL;
constexpr int PT_COST_WORDS = 1104;        // 1 101 costs; word 1101 carries the fourth 32x32's current_depth_cost to the root
constexpr int PT_SQ_BYTES = 344;
constexpr int PT_DEC_WORDS = 9;            // svt_hip_md_decision as 8-byte words
constexpr unsigned long long PT_MAX_MODE_COST = 13616969489728ull * 8;
constexpr uint32_t PT_PARTITION_SPLIT = 3, PT_BITS_ROW = 11;
// per-square bytes: what the PART_N entry gave, and what d2 left
constexpr uint32_t PT_TESTED = 1, PT_MDC_SPLIT = 2;
constexpr uint32_t PT_COMPARED = 1, PT_BEGAN_4X4 = 2;

struct PartBlkDev { uint16_t sq; uint8_t shape, nsi, x, y, bsize, totns; };
struct PartSqDev { uint16_t mds, parent; uint8_t depth, x, y, pad; };
struct PartDevTab { PartBlkDev blk[PT_BLOCKS]; PartSqDev sq[PT_SQUARES]; };
static_assert(sizeof(PartBlkDev) == 8 && sizeof(PartSqDev) == 8, "one 8-byte load per entry");
constexpr PartDevTab part_dev_tab() {
    const svthost::PartGeomTab G = svthost::part_geom_tab();
    PartDevTab T{};
    for (int i = 0; i < PT_BLOCKS; i++)
        T.blk[i] = PartBlkDev{G.sq_of[i], G.blk[i].shape, G.blk[i].nsi, G.blk[i].origin_x, G.blk[i].origin_y, G.blk[i].bsize, G.blk[i].totns};
    for (int s = 0; s < PT_SQUARES; s++) T.sq[s] = PartSqDev{G.sq[s].mds, G.sq[s].parent, G.sq[s].depth, G.sq[s].x, G.sq[s].y, 0};
    return T;
}
static __device__ const PartDevTab kPartTab = part_dev_tab();

struct PartitionDesc {
    const uint32_t* sb;                    // svt_hip_part_sb as three words
    const uint32_t* leaf;                  // svt_hip_part_leaf as three words
    const unsigned long long* decision;    // svt_hip_md_decision as nine words, or NULL
    const unsigned long long* cost;
    const int32_t* bits;                   // partitionFacBits [20][11]
    unsigned long long* sq;                // svt_hip_part_sq as two words
    uint32_t* final_count;
    uint32_t* final_blk;                   // svt_hip_part_final as three words
    unsigned long long* final_decision;
    uint32_t nsb, nleaves, nsrc, lambda, pic_width, pic_height;
    uint32_t slice_is_intra;
};

// the first block of a shape inside its square (ns_blk_offset by shape) and the blocks of a shape, 5 and 3 bits per shape
__device__ __forceinline__ uint32_t pt_shape_off(uint32_t shape) { return (uint32_t)(0x158B96828C20ull >> (5 * shape)) & 31u; }
__device__ __forceinline__ uint32_t pt_shape_n(uint32_t shape) { return (uint32_t)(0x48DB691u >> (3 * shape)) & 7u; }
static_assert(((0x158B96828C20ull >> 0) & 31) == 0 && ((0x158B96828C20ull >> 5) & 31) == 1 && ((0x158B96828C20ull >> 10) & 31) == 3 &&
              ((0x158B96828C20ull >> 15) & 31) == 5 && ((0x158B96828C20ull >> 20) & 31) == 8 && ((0x158B96828C20ull >> 25) & 31) == 11 &&
              ((0x158B96828C20ull >> 30) & 31) == 14 && ((0x158B96828C20ull >> 35) & 31) == 17 && ((0x158B96828C20ull >> 40) & 31) == 21, "shape offsets");
static_assert(((0x48DB691u >> 0) & 7) == 1 && ((0x48DB691u >> 3) & 7) == 2 && ((0x48DB691u >> 6) & 7) == 2 && ((0x48DB691u >> 9) & 7) == 3 &&
              ((0x48DB691u >> 12) & 7) == 3 && ((0x48DB691u >> 15) & 7) == 3 && ((0x48DB691u >> 18) & 7) == 3 && ((0x48DB691u >> 21) & 7) == 4 &&
              ((0x48DB691u >> 24) & 7) == 4, "blocks per shape");
__device__ __forceinline__ uint32_t pt_part_of_shape(uint32_t shape) { return shape < 3 ? shape : shape + 1; }      // from_shape_to_part
__device__ __forceinline__ uint32_t pt_shape_of_part(uint32_t part) { return part < 3 ? part : part - 1; }          // (part != 3)
// squares in the subtree of a child of a square at `depth`: 85, 21, 5, 1
__device__ __forceinline__ uint32_t pt_child_squares(uint32_t depth) { return (0x01051555u >> (8 * depth)) & 255u; }

// av1_split_flag_rate (EbRateDistortionCost.c:2268-2342) for the square of `depth` at (px, py) in the picture
__device__ __forceinline__ unsigned long long pt_rate(const PartitionDesc& F, uint32_t depth, uint32_t px, uint32_t py, int left, int above, bool split) {
    const uint32_t size = 64u >> depth, type = split ? PT_PARTITION_SPLIT : 0u;
    long long r;
    if (size < 8) {
        r = F.bits[type];
    } else {
        const uint32_t hbs = size >> 1, bsl = 3 - depth;
        const bool has_rows = py + hbs < F.pic_height, has_cols = px + hbs < F.pic_width;
        if (has_rows && has_cols) {
            r = F.bits[(size == 8 ? 4u : 10u) * PT_BITS_ROW + type];       // the row is partition_cdf_length(bsize)
        } else if (split) {
            r = 0;                                                          // AOM_ICDF(CDF_PROB_TOP)
        } else {
            if (left == -1) left = 0;                                       // INVALID_NEIGHBOR_DATA
            if (above == -1) above = 0;
            const uint32_t ctx = (uint32_t)((left >> bsl) & 1) * 2 + (uint32_t)((above >> bsl) & 1) + bsl * 4;      // 0 .. 15
            const int32_t* in = F.bits + ctx * PT_BITS_ROW;
            // partition_gather_vert_alike (bottom half outside only) / _horz_alike on the row of bits: the sum of
            // cdf_element_prob over VERT, SPLIT, HORZ_A, VERT_A, VERT_B, VERT_4 / HORZ, SPLIT, HORZ_A, HORZ_B, VERT_A, HORZ_4
            const uint32_t set = (!has_rows && has_cols) ? 0x2DCu : 0x17Au;
            uint32_t sum = 0;
#pragma unroll
            for (uint32_t e = 1; e < 10; e++)
                if (set >> e & 1u) sum += (uint32_t)in[e - 1] - (uint32_t)in[e];
            r = (int32_t)sum;
        }
    }
    return ((unsigned long long)r * (unsigned long long)F.lambda + 256ull) >> 9;
}

__global__ __launch_bounds__(PT_THREADS) void partition_kernel(const PartitionDesc F) {
    __shared__ unsigned long long cost_all[PT_WAVES * PT_COST_WORDS];
    __shared__ uint32_t fsrc_all[PT_WAVES * PT_MAX_FINAL];
    __shared__ uint16_t entry_all[PT_WAVES * PT_COST_WORDS];
    __shared__ uint16_t best_all[PT_WAVES * PT_SQ_BYTES];
    __shared__ uint8_t sqb_all[PT_WAVES * 7 * PT_SQ_BYTES];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const uint32_t sb = blockIdx.x * PT_WAVES + wave;                      // (host-checked: below 2^31 / 341 + 4)
    if (sb >= F.nsb) return;                                                // wave-uniform; no workgroup barrier below
    unsigned long long* cost = cost_all + wave * PT_COST_WORDS;
    uint32_t* fsrc = fsrc_all + wave * PT_MAX_FINAL;
    uint16_t* entry = entry_all + wave * PT_COST_WORDS;
    uint16_t* best = best_all + wave * PT_SQ_BYTES;
    uint8_t* part = sqb_all + wave * 7 * PT_SQ_BYTES;
    uint8_t* split = part + PT_SQ_BYTES;
    uint8_t* given = split + PT_SQ_BYTES;                                   // PT_TESTED | PT_MDC_SPLIT
    uint8_t* called = given + PT_SQ_BYTES;                                  // d2 is called on this square
    uint8_t* climb = called + PT_SQ_BYTES;                                  // PT_COMPARED | PT_BEGAN_4X4
    int8_t* left = (int8_t*)(climb + PT_SQ_BYTES);
    int8_t* above = left + PT_SQ_BYTES;

    // ---- start: Initialize_cu_data_structure, and zero where the reference reads stale memory ----
    for (int i = lane; i < PT_COST_WORDS; i += 64) { cost[i] = 0; entry[i] = 0; }
    for (int s = lane; s < PT_SQ_BYTES; s += 64) {
        part[s] = (uint8_t)PT_PARTITION_SPLIT; split[s] = 1; given[s] = 0; called[s] = 0; climb[s] = 0; left[s] = 0; above[s] = 0; best[s] = 0;
    }
    wave_lds_fence();

    // ---- load: the leaf list ----
    const uint32_t lf = min(F.sb[3 * (size_t)sb], F.nleaves);
    const uint32_t sbw1 = F.sb[3 * (size_t)sb + 1], sbw2 = F.sb[3 * (size_t)sb + 2];
    const uint32_t cnt = min(min(sbw1 & 0xffffu, F.nleaves - lf), (uint32_t)PT_BLOCKS);
    const uint32_t ox = sbw1 >> 16, oy = sbw2 & 0xffffu;
    int last_n = -1;                                                        // the last PART_N entry so far
#pragma unroll 1
    for (uint32_t base = 0; base < cnt; base += 64) {
        const uint32_t i = base + (uint32_t)lane;
        const bool valid = i < cnt;
        uint32_t w0 = 0, w1 = 0, w2 = 0;
        if (valid) { const uint32_t* L = F.leaf + 3 * (size_t)(lf + i); w0 = L[0]; w1 = L[1]; w2 = L[2]; }
        const uint32_t mds = min(w0 & 0xffffu, (uint32_t)PT_BLOCKS - 1);
        const PartBlkDev g = kPartTab.blk[mds];
        const bool is_n = valid && g.shape == 0;
        const unsigned long long ns = __ballot(is_n);
        const unsigned long long upto = ns & (~0ull >> (63 - lane));
        const int my_n = upto ? (int)base + 63 - __clzll((long long)upto) : last_n;
        const uint32_t acc = my_n < 0 ? i + 1 : i - (uint32_t)my_n + 1;
        if (valid) {
            const uint32_t src = min(w2, F.nsrc - 1);
            cost[mds] = F.cost ? F.cost[src] : F.decision[PT_DEC_WORDS * (size_t)src];
            entry[mds] = (uint16_t)(i + 1);
            const uint32_t flag = (w0 >> 16) & 1u;                          // (a one-bit member takes bit 0)
            if (is_n) {
                given[g.sq] = (uint8_t)(PT_TESTED | (flag ? PT_MDC_SPLIT : 0u));
                split[g.sq] = (uint8_t)flag;
                left[g.sq] = (int8_t)(w1 & 0xffu); above[g.sq] = (int8_t)(w1 >> 8 & 0xffu);
            }
            if (acc == (w0 >> 24)) called[g.sq] = 1;
        }
        if (ns) last_n = (int)base + 63 - __clzll((long long)ns);
    }
    wave_lds_fence();

    // ---- d1: lane per square, shapes ascending ----
#pragma unroll 1
    for (int s = lane; s < PT_SQUARES; s += 64) {
        const PartSqDev q = kPartTab.sq[s];
        const uint32_t nshapes = q.depth <= 2 ? 9u : (q.depth == 3 ? 3u : 1u);
        unsigned long long c = cost[q.mds];
        uint32_t p = part[s], b = best[s];
#pragma unroll 1
        for (uint32_t shape = 0; shape < nshapes; shape++) {
            const uint32_t first = q.mds + pt_shape_off(shape), n = pt_shape_n(shape);
            if (entry[first + n - 1] == 0) continue;                        // d1 runs at the shape's last block
            unsigned long long tot = 0;
            for (uint32_t k = 0; k < n; k++) tot += cost[first + k];
            if (shape == 0 || tot < c) { c = tot; p = pt_part_of_shape(shape); b = first; }
        }
        cost[q.mds] = c; part[s] = (uint8_t)p; best[s] = (uint16_t)b;
    }
    wave_lds_fence();

    // ---- d2: level by level from the 8x8 parents to the root ----
#pragma unroll 1
    for (int d = 3; d >= 0; d--) {
        if (lane < (1 << (2 * d))) {
            uint32_t s = 0;                                                 // the lane's parent: Z-order digits of the lane, top down
            for (int k = 0; k < d; k++) s += 1 + (((uint32_t)lane >> (2 * (d - 1 - k))) & 3u) * pt_child_squares(k);
            const uint32_t nq = pt_child_squares(d), c0 = s + 1, c3 = c0 + 3 * nq;
            const bool began = called[c3] && (given[c3] & PT_TESTED) && !(given[c3] & PT_MDC_SPLIT);
            const bool passed = (climb[c3] & PT_COMPARED) != 0;
            if (began || passed) {
                const bool began4 = began ? d == 3 : (climb[c3] & PT_BEGAN_4X4) != 0;
                const PartSqDev P = kPartTab.sq[s];
                unsigned long long parent_cost, current;
                if (F.slice_is_intra && d == 0) {
                    parent_cost = PT_MAX_MODE_COST;
                    current = passed ? cost[PT_BLOCKS] : 0;
                } else {
                    const int l = left[c0], a = above[c0];
                    left[s] = (int8_t)l; above[s] = (int8_t)a;
                    parent_cost = (given[s] & PT_TESTED) ? cost[P.mds] + pt_rate(F, d, ox + P.x, oy + P.y, l, a, false) : PT_MAX_MODE_COST;
                    current = pt_rate(F, d, ox + P.x, oy + P.y, l, a, true);
#pragma unroll 1
                    for (uint32_t k = 0; k < 4; k++) {
                        const uint32_t cs = c0 + k * nq;
                        const PartSqDev C = kPartTab.sq[cs];
                        current += cost[C.mds];
                        if (!began4 && !(given[cs] & PT_MDC_SPLIT)) current += pt_rate(F, d + 1, ox + C.x, oy + C.y, left[cs], above[cs], false);
                    }
                }
                if (parent_cost <= current) { split[s] = 0; cost[P.mds] = parent_cost; }
                else { cost[P.mds] = current; part[s] = (uint8_t)PT_PARTITION_SPLIT; }
                climb[s] = (uint8_t)(PT_COMPARED | (began4 ? PT_BEGAN_4X4 : 0u));
                if (d == 1 && lane == 3) cost[PT_BLOCKS] = current;
            }
        }
        wave_lds_fence();
    }

    // ---- the squares, and the final blocks in coding order ----
    uint32_t total = 0;
#pragma unroll 1
    for (int base = 0; base < PT_SQUARES; base += 64) {
        const int s = base + lane;
        uint32_t n = 0, p = PT_PARTITION_SPLIT;
        PartSqDev q{};
        if (s < PT_SQUARES) {
            q = kPartTab.sq[s];
            p = part[s];
            unsigned long long* out = F.sq + 2 * ((size_t)sb * PT_SQUARES + (size_t)s);
            out[0] = cost[q.mds];
            out[1] = (unsigned long long)best[s] | (unsigned long long)p << 16 | (unsigned long long)split[s] << 24 |
                     (unsigned long long)(given[s] & PT_TESTED) << 32;
            bool reached = true;
            for (uint32_t a = q.parent; a != svthost::PART_NO_PARENT; a = kPartTab.sq[a].parent) reached = reached && part[a] == PT_PARTITION_SPLIT;
            if (reached && p != PT_PARTITION_SPLIT) n = pt_shape_n(pt_shape_of_part(min(p, 9u)));
        }
        const uint32_t incl = wave_scan_incl(n, lane);
        const uint32_t slot0 = total + incl - n;
        total += wave_scan_total(incl);
        for (uint32_t k = 0; k < n; k++) {
            const uint32_t slot = slot0 + k;
            if (slot >= (uint32_t)PT_MAX_FINAL) break;                      // (disjoint blocks of at least 4x4: cannot happen)
            const uint32_t mds = q.mds + pt_shape_off(pt_shape_of_part(min(p, 9u))) + k;
            const PartBlkDev g = kPartTab.blk[mds];
            const uint32_t e = entry[mds];
            const uint32_t src = e ? min(F.leaf[3 * (size_t)(lf + e - 1) + 2], F.nsrc - 1) : SVT_HIP_PART_NO_SRC;
            FinalEntry fe;
            fe.mds = mds; fe.x = ox + g.x; fe.y = oy + g.y; fe.bsize_byte = g.bsize; fe.part = p; fe.src = src;
            final_entry_store(F.final_blk, sb, slot, fe);
            fsrc[slot] = src;
        }
    }
    total = min(total, (uint32_t)PT_MAX_FINAL);
    if (lane == 0) F.final_count[sb] = total;
    if (F.final_decision) {
        wave_lds_fence();
        unsigned long long* out = F.final_decision + PT_DEC_WORDS * (size_t)sb * PT_MAX_FINAL;
#pragma unroll 1
        for (uint32_t w = (uint32_t)lane; w < total * PT_DEC_WORDS; w += 64) {
            const uint32_t k = w / PT_DEC_WORDS, j = w - k * PT_DEC_WORDS, src = fsrc[k];
            out[w] = src != SVT_HIP_PART_NO_SRC ? F.decision[PT_DEC_WORDS * (size_t)src + j] : 0ull;
        }
    }
}

}  // namespace svtdev

// kernel_coeff_rate.h — coeff_rate_kernel: the coefficient rate of quantised transform blocks, av1_cost_coeffs_txb
// (EbRateDistortionCost.c:412-519) without its Av1TransformTypeRateEstimation term, and av1_cost_skip_txb (:401-410) for eob 0, for
// every (block, transform type) of many groups in one launch.  It reads what full_loop_kernel writes (qcoeff, eob) and the scan
// tables' inverse; the cost tables are the caller's data (one LV_MAP_COEFF_COST and one LV_MAP_EOB_COST per group).
//
// The reference walks the scan backwards from eob - 1.  Nothing in a coefficient's cost depends on that walk: the cost is a
// function of the coefficient, of its scan index (iscan[pos]: costed iff < eob, the last one iff == eob - 1, the DC iff == 0) and of
// a fixed neighbourhood of LEVELS to the right of and below it.  So lanes own positions and one sum ends the block.
//
//   levels   av1_txb_init_levels_c: min(|q|, 127) in a map of stride KW + TX_PAD_HOR with zero padding, KW x KH = the packed
//            min(W, 32) x min(H, 32) block.  The map lives in LDS, (KH + 4) rows (no row above the block is ever read, the farthest
//            read is four rows below or four columns right of a coefficient), and never goes to HBM.
//   lane     owns a QUAD: four consecutive positions of one row (KW is a multiple of 4).  One 16-byte load of qcoeff, one 8-byte load
//            of iscan, one 4-byte LDS store of the four levels; then seven 4-byte LDS loads give every neighbour of the four positions
//            in any class (rows r and r+1: columns c..c+7; rows r+2, r+3, r+4: c..c+3), and the bytes are picked in registers.
//   context  av1_get_nz_map_contexts (the AV1 specification's get_nz_map_ctx; the reference's only implementation is
//            av1_get_nz_map_contexts_sse2): last coefficient 0 / 1 / 2 / 3 by scan index 0, <= KW*KH/8, <= KW*KH/4, else; others
//            min((sum of min(level, 3) over the class's five neighbours + 1) >> 1, 4) + av1_nz_map_ctx_offset[tx_size][min(row, 4)]
//            [min(col, 4)] (2-D; position 0 is context 0), + 26 + {0, 5, 10}[min(col | row, 2)] (horizontal by column, vertical by row).
//   range    get_br_ctx (:366-399), lps_cost, get_golomb_cost (:98-105) on the unclamped |q|.
//   eob      get_eob_cost (:229-245) once per block.
// Packing: a (block, type) PAIR is KW * KH / 4 quads.  A pair of 64 quads or more takes a whole wave (1, 2 or 4 quads per lane); smaller
// pairs share a wave, 64 / quads pairs each on its own aligned lane group (16 pairs of 4x4).  32-bit sums, reduced inside the lane
// group with DPP and, across rows of 16 lanes, ds_bpermute (group_sum_rt, as the CDEF kernel).  One 8-byte store per pair.
// A workgroup (4 waves) belongs to one group, stages that group's two cost tables in LDS once and then runs 1 .. CR_ITERS wave-units
// per wave (the host's choice: one while the group has too few units to fill the machine, four when it has plenty).  Everything about
// the size is wave-uniform runtime data (shifts): one kernel for the 19 sizes.
// Contexts are clamped (txb_skip_ctx to 0..12, dc_sign_ctx to 0..2), the eob to KW * KH: a bad value gives an unspecified cost and
// no out-of-range read.
#pragma once
#include "dev_common.h"
#include "group_table.h"

namespace svtdev {

constexpr int CR_MAX_GROUPS = 32;          // per launch: what fits the kernel arguments
constexpr int CR_MAX_TYPES = 16;
constexpr int CR_THREADS = 256, CR_WAVES = CR_THREADS / 64;
constexpr int CR_ITERS = 4;                // most wave-units per wave: the staged tables then serve CR_WAVES * CR_ITERS units
constexpr int CR_COEFF_COST_WORDS = 529;   // LV_MAP_COEFF_COST (EbMdRateEstimation.h:34-41)
constexpr int CR_EOB_COST_WORDS = 22;      // LV_MAP_EOB_COST
// word offsets of LV_MAP_COEFF_COST's members
constexpr int CR_TXB_SKIP = 0;             // txb_skip_cost[13][2]
constexpr int CR_BASE_EOB = 26;            // base_eob_cost[4][3]
constexpr int CR_BASE = 38;                // base_cost[42][4]
constexpr int CR_EOB_EXTRA = 206;          // eob_extra_cost[22][2]
constexpr int CR_DC_SIGN = 250;            // dc_sign_cost[3][2]
constexpr int CR_LPS = 256;                // lps_cost[21][13]
constexpr int CR_LEVELS_WAVE = (32 + 4) * (32 + 4) + 16;      // the largest padded map (32x32), 16-byte multiple
constexpr int CR_TABLE_WORDS = CR_COEFF_COST_WORDS + CR_EOB_COST_WORDS + 1;

struct CoeffRateGroupDev {
    const int32_t* qcoeff;                                 // [nblocks][ntypes][KW * KH]
    const uint16_t* eob;                                   // [nblocks][ntypes]
    const int16_t* iscan;                                  // ntypes x KW * KH
    const uint8_t* skip_ctx; const uint8_t* dc_ctx;        // [nblocks]
    const int32_t* type_bits;                              // optional [nblocks][ntypes]
    const int32_t* coeff_cost; const int32_t* eob_cost;
    unsigned long long* bits;                              // [nblocks][ntypes]
    uint32_t nblocks, wg_end;
    int32_t ntypes;
    uint8_t bwl, bhl;                                      // log2 of the packed sides, min(W, 32) and min(H, 32)
    uint8_t shape;                                         // of the REAL sides: 0 square, 1 wide, 2 tall (64x16 is wide though packed 32x16)
    uint8_t iters;                                         // wave-units per wave, 1 .. CR_ITERS (host: coeff_rate_iters)
    uint8_t types[CR_MAX_TYPES];
};
struct CoeffRateDesc {
    int32_t ngroups;
    CoeffRateGroupDev g[CR_MAX_GROUPS];
};
static_assert(sizeof(CoeffRateDesc) <= 4000, "kernel arguments");

// av1_nz_map_ctx_offset (EbRateDistortionCost.c:249-364) holds five patterns; rows and columns are clamped to 4.
//   square:  {0,1,6,6,21} {1,6,6,21,21} {6,6,21,21,21} {6,21,21,21,21} {21,...}        = by min(row + col, 4): 0 1 6 6 21 .. but [0][0] = 0
//   wide  (W > H):  columns 0, 1 are 16 (but [0][0] = 0), then row 0: 6 6 21, row 1: 6 21 21, rows 2+: 21
//   tall  (W < H):  rows 0, 1 are 11 (but [0][0] = 0), then rows 2: 6 6 21 21 21, 3: 6 21 21 21 21, 4: 21
// (the 4-wide and 4-high sizes' zero entries are never indexed: that row or column does not exist)
__device__ __forceinline__ int cr_nz_offset_2d(int shape, int row, int col) {          // shape: 0 square, 1 wide, 2 tall; selects only
    const int s = row + col;
    const int square = s < 2 ? 1 : (s < 4 ? 6 : 21);
    const int wide = col < 2 ? 16 : ((((row == 0) & (col < 4)) | ((row == 1) & (col == 2))) ? 6 : 21);
    const int tall = row < 2 ? 11 : ((((row == 2) & (col < 2)) | ((row == 3) & (col == 0))) ? 6 : 21);
    const int r = shape == 0 ? square : (shape == 1 ? wide : tall);
    return (row | col) == 0 ? 0 : r;
}

__device__ __forceinline__ uint32_t cr_byte(uint32_t w, int i) { return (w >> (8 * i)) & 0xffu; }
__device__ __forceinline__ uint32_t cr_min3(uint32_t v) { return min(v, 3u); }

__global__ __launch_bounds__(CR_THREADS) void coeff_rate_kernel(const CoeffRateDesc fd) {
    __shared__ __attribute__((aligned(16))) int32_t tab[CR_TABLE_WORDS];
    __shared__ __attribute__((aligned(16))) uint8_t levels_all[CR_WAVES * CR_LEVELS_WAVE];
    uint32_t bid;
    const int gi = group_of(fd, bid);
    if (gi >= fd.ngroups) return;
    const CoeffRateGroupDev& F = fd.g[gi];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;

    // ---- the group's cost tables, once per workgroup; this wave's level map zeroed (the padding stays zero: only the block is rewritten) ----
    for (int i = threadIdx.x; i < CR_COEFF_COST_WORDS; i += CR_THREADS) tab[i] = F.coeff_cost[i];
    if (threadIdx.x < CR_EOB_COST_WORDS) tab[CR_COEFF_COST_WORDS + threadIdx.x] = F.eob_cost[threadIdx.x];
    uint8_t* lv = levels_all + wave * CR_LEVELS_WAVE;
    for (int i = lane; i < CR_LEVELS_WAVE / 4; i += 64) reinterpret_cast<uint32_t*>(lv)[i] = 0;
    __syncthreads();
    const int32_t* eobc = tab + CR_COEFF_COST_WORDS;

    // ---- geometry: all powers of two, wave-uniform ----
    const int bwl = F.bwl, bhl = F.bhl, shape = F.shape;
    const int kw = 1 << bwl, nc = 1 << (bwl + bhl), stride = kw + 4;
    const int qpl = bwl + bhl - 2;                          // log2 quads per pair
    const int gl = qpl < 6 ? qpl : 6;                       // log2 lanes per pair
    const int ppw = 64 >> gl;                               // pairs per wave-unit
    const int qiter = 1 << (qpl - gl);                      // quads per lane
    const int sub = lane >> gl, l = lane & ((1 << gl) - 1);
    uint8_t* mylv = lv + sub * (stride << bhl) + sub * (stride << 2);           // (KH + 4) * stride per pair
    const int ntypes = F.ntypes, iters = F.iters;
    const uint32_t npairs = F.nblocks * (uint32_t)ntypes;                      // host-checked: below 2^31

#pragma unroll 1
    for (int it = 0; it < iters; it++) {
        const uint32_t first = ((bid * iters + it) * CR_WAVES + wave) * ppw;  // (below npairs + 2^8: no wrap)
        if (first >= npairs) break;                         // wave-uniform
        const uint32_t pair = first + sub;
        const bool valid = pair < npairs;
        const uint32_t pc = valid ? pair : npairs - 1;      // spare lane groups redo the last pair and store nothing
        const uint32_t blk = pc / (uint32_t)ntypes;
        const int t = (int)(pc - blk * (uint32_t)ntypes);
        const int dcs = min((int)F.dc_ctx[blk], 2);
        const int cls = (0x5400u >> F.types[t]) & 1 ? 2 : ((0xa800u >> F.types[t]) & 1 ? 1 : 0);   // tx_type_to_class: V_* vertical, H_* horizontal
        const int eob = min((int)F.eob[pc], nc);
        const int32_t* q = F.qcoeff + (size_t)pc * nc;
        const int16_t* is = F.iscan + t * nc;

        // ---- levels: the lane's quads into the map ----
        int4 qv[4];
        uint2 iv[4];
#pragma unroll
        for (int k = 0; k < 4; k++) {
            if (k < qiter) {
                const int p0 = (l + (k << 6)) << 2;
                qv[k] = eob ? *reinterpret_cast<const int4*>(q + p0) : make_int4(0, 0, 0, 0);
                iv[k] = *reinterpret_cast<const uint2*>(is + p0);
                const uint32_t a0 = min((uint32_t)abs(qv[k].x), 127u), a1 = min((uint32_t)abs(qv[k].y), 127u);
                const uint32_t a2 = min((uint32_t)abs(qv[k].z), 127u), a3 = min((uint32_t)abs(qv[k].w), 127u);
                const int row = p0 >> bwl, col = p0 & (kw - 1);
                *reinterpret_cast<uint32_t*>(mylv + row * stride + col) = a0 | (a1 << 8) | (a2 << 16) | (a3 << 24);
            }
        }
        wave_lds_fence();

        uint32_t cost = 0;
#pragma unroll
        for (int k = 0; k < 4; k++) {
            if (k < qiter) {
                const int p0 = (l + (k << 6)) << 2;
                const int row = p0 >> bwl, col = p0 & (kw - 1);
                const uint8_t* at = mylv + row * stride + col;
                const uint32_t r0a = *reinterpret_cast<const uint32_t*>(at), r0b = *reinterpret_cast<const uint32_t*>(at + 4);
                const uint32_t r1a = *reinterpret_cast<const uint32_t*>(at + stride), r1b = *reinterpret_cast<const uint32_t*>(at + stride + 4);
                const uint32_t r2a = *reinterpret_cast<const uint32_t*>(at + 2 * stride), r3a = *reinterpret_cast<const uint32_t*>(at + 3 * stride);
                const uint32_t r4a = *reinterpret_cast<const uint32_t*>(at + 4 * stride);
                const unsigned long long r0 = r0a | ((unsigned long long)r0b << 32), r1 = r1a | ((unsigned long long)r1b << 32);
                const int vq[4] = {qv[k].x, qv[k].y, qv[k].z, qv[k].w};
                const int sc4[4] = {(int)(iv[k].x & 0xffffu), (int)(iv[k].x >> 16), (int)(iv[k].y & 0xffffu), (int)(iv[k].y >> 16)};
                // branch-free per position: every table read is issued (at an index that is always inside the tables) and the terms are
                // selected afterwards, so that the LDS reads of a quad overlap instead of waiting one conditional block after the other
#pragma unroll
                for (int j = 0; j < 4; j++) {
                    const int v = vq[j], sc = sc4[j], c = col + j;
                    const uint32_t level = (uint32_t)abs(v), l3 = cr_min3(level);
                    // neighbours of (row, c): right 1 .. 4 in row r, below 1 .. 4 in column c, and the diagonal
                    const uint32_t e1 = (uint32_t)(r0 >> (8 * (j + 1))) & 0xffu, e2 = (uint32_t)(r0 >> (8 * (j + 2))) & 0xffu;
                    const uint32_t e3 = (uint32_t)(r0 >> (8 * (j + 3))) & 0xffu, e4 = (uint32_t)(r0 >> (8 * (j + 4))) & 0xffu;
                    const uint32_t s1 = cr_byte(r1a, j), s2 = cr_byte(r2a, j), s3 = cr_byte(r3a, j), s4 = cr_byte(r4a, j);
                    const uint32_t dg = (uint32_t)(r1 >> (8 * (j + 1))) & 0xffu;
                    const bool dc = (row | c) == 0;
                    // base level: base_eob_cost by the scan index for the last coefficient, base_cost by the neighbourhood for the others
                    const uint32_t far3 = cls == 0 ? cr_min3(dg) + cr_min3(e2) + cr_min3(s2)
                                                   : (cls == 1 ? cr_min3(e2) + cr_min3(e3) + cr_min3(e4) : cr_min3(s2) + cr_min3(s3) + cr_min3(s4));
                    const uint32_t mag = cr_min3(e1) + cr_min3(s1) + far3;
                    const int off = cls == 0 ? cr_nz_offset_2d(shape, min(row, 4), min(c, 4)) : 26 + 5 * min(cls == 1 ? c : row, 2);
                    const int ctx = ((cls == 0) & dc) ? 0 : (int)min((mag + 1) >> 1, 4u) + off;
                    const int ctx_last = sc == 0 ? 0 : (sc <= (nc >> 3) ? 1 : (sc <= (nc >> 2) ? 2 : 3));
                    const uint32_t base = tab[sc == eob - 1 ? CR_BASE_EOB + ctx_last * 3 + (int)max(l3, 1u) - 1 : CR_BASE + ctx * 4 + (int)l3];
                    // sign: dc_sign_cost for scan index 0, a literal bit elsewhere
                    const uint32_t dc_sign = (uint32_t)tab[CR_DC_SIGN + 2 * dcs + (v < 0)];
                    // range: get_br_ctx, lps_cost, Golomb from level 15 up
                    const uint32_t bmag = min((e1 + s1 + (cls == 0 ? dg : (cls == 1 ? e2 : s2)) + 1) >> 1, 6u);
                    const bool near = cls == 0 ? ((row < 2) & (c < 2)) : (cls == 1 ? c == 0 : row == 0);
                    const int bctx = (int)bmag + (dc ? 0 : (near ? 7 : 14));
                    const uint32_t lps = (uint32_t)tab[CR_LPS + bctx * 13 + (int)min(max(level, 3u) - 3, 12u)];
                    const uint32_t golomb = level >= 15 ? (uint32_t)(2 * (32 - __clz((int)(max(level, 15u) - 14))) - 1) << 9 : 0u;      // get_golomb_cost
                    const uint32_t nz = (sc == 0 ? dc_sign : 512u) + (level > 2 ? lps + golomb : 0u);
                    cost += sc < eob ? base + (v != 0 ? nz : 0u) : 0u;
                }
            }
        }
        wave_lds_fence();                                   // the next unit rewrites the map
        cost = group_sum_rt(cost, 1u << gl);

        if (valid && l == 0) {
            const int sk = min((int)F.skip_ctx[blk], 12);
            unsigned long long bits;
            if (eob == 0) {
                bits = (unsigned long long)(long long)tab[CR_TXB_SKIP + 2 * sk + 1];
            } else {
                // get_eob_cost: the eob's position token, then its extra bits
                const int eob_pt = eob < 3 ? eob : 33 - __clz(eob - 1);      // 1 2 3 3 4 4 4 4 5 ..: eob_to_pos_small / _large
                int c32 = tab[CR_TXB_SKIP + 2 * sk] + eobc[(cls ? 11 : 0) + eob_pt - 1];
                const int offset_bits = eob_pt - 2;                          // k_eob_offset_bits (<= 0: none)
                if (offset_bits > 0) {
                    const int extra = eob - ((1 << offset_bits) + 1);        // eob - k_eob_group_start[eob_pt]
                    c32 += tab[CR_EOB_EXTRA + 2 * eob_pt + ((extra >> (offset_bits - 1)) & 1)];
                    if (offset_bits > 1) c32 += (offset_bits - 1) << 9;
                }
                if (F.type_bits) c32 += F.type_bits[pair];
                bits = (unsigned long long)(long long)(int)((uint32_t)c32 + cost);     // the reference's int32 cost, returned as uint64_t
            }
            F.bits[pair] = bits;
        }
    }
}

}  // namespace svtdev

// intra_plan.h — the intra and chroma-from-luma family planned on the host: the argument checks, the lane and grid arithmetic and the
// LDS sizes of every device-pointer entry point of svt_hip_intra.hip, derived before the launch.  svt_hip_intra.hip checks, then
// launches from here.  Plain C++17, no HIP header: a CPU program can include it (tests/c/intra_plan_host.cpp).  The geometry in
// namespace svtdev is the one statement of each rule: the kernels (kernel_intra.h, kernel_cfl.h, kernel_bip.h) call the same functions.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "../../include/svt_hip_dsp.h"
#include "av1_geom.h"
#include "group_table.h"
#include "host_err.h"

#ifdef __HIPCC__
#define SVT_INTRA_HD __host__ __device__ __forceinline__
#define SVT_INTRA_HDC __host__ __device__ constexpr
#else
#define SVT_INTRA_HD inline
#define SVT_INTRA_HDC constexpr
#endif

namespace svtdev {

// Neighbour layout per block: `nb_pitch` samples; position p of the reference's above_row / left_col lives at index NB_ORIGIN + p (p >= -2).
constexpr int NB_ORIGIN = 16;

// ---- the prediction kernels' lanes ----
// A block is covered by per_block = lanes_per_row * bh consecutive lanes (a power of two, 4 .. 512); a lane writes ppl samples of one
// row: 16 bytes of it where the block is that wide (ppl_wide samples), else the whole row.
struct IntraLanes { int ppl, lanes_per_row; uint32_t per_block; };
// (a kernel knows both at compile time: intra_pred_kernel<.., WIDE, ..> with PPL_WIDE = 16 bytes of its samples; the directional
// kernels have ppl as NPX and pass it with WIDE = true)
template <bool WIDE, int PPL_WIDE>
SVT_INTRA_HD IntraLanes intra_lanes_of(int bw, int bh) {
    IntraLanes L;
    L.ppl = WIDE ? PPL_WIDE : bw;
    L.lanes_per_row = WIDE ? bw >> __builtin_ctz((uint32_t)PPL_WIDE) : 1;
    L.per_block = (uint32_t)(L.lanes_per_row * bh);
    return L;
}
SVT_INTRA_HD IntraLanes intra_lanes(int bw, int bh, int sample_bytes) {
    if (sample_bytes == 1) return bw >= 16 ? intra_lanes_of<true, 16>(bw, bh) : intra_lanes_of<false, 16>(bw, bh);
    return bw >= 8 ? intra_lanes_of<true, 8>(bw, bh) : intra_lanes_of<false, 8>(bw, bh);
}
// blocks per lane of the wide plain kernels: 4 for the modes with per-pixel arithmetic (SMOOTH*, PAETH: + 9 % on 2^21 32x32 blocks, A/B),
// 2 for the copy-like ones (DC*, V, H: 2 - 4 % SLOWER at 4); the narrow form takes 1
SVT_INTRA_HDC int intra_wide_iu(int mode) {
    return mode == SVT_INTRA_SMOOTH || mode == SVT_INTRA_SMOOTH_V || mode == SVT_INTRA_SMOOTH_H || mode == SVT_INTRA_PAETH ? 4 : 2;
}
// samples the DC modes average; dc_magic = floor(2^32 / cnt) + 1 makes umulhi(s + cnt / 2, dc_magic) the exact quotient (cnt <= 128, s < 2^20)
SVT_INTRA_HDC int intra_dc_count(int mode, int bw, int bh) { return mode == SVT_INTRA_DC ? bw + bh : (mode == SVT_INTRA_DC_TOP ? bw : bh); }
SVT_INTRA_HDC uint32_t intra_dc_magic(int cnt) { return (uint32_t)(0x100000000ull / (uint64_t)cnt) + 1u; }

// ---- the directional kernels' staged edges (intra_dir_body, kernel_intra.h) ----
// A workgroup's 256 lanes work on `slots` blocks, lpb lanes on each.  Per block the two edges are staged in LDS as pair dwords, array
// positions [NB_ORIGIN - 2, n_pad), estride dwords per edge (+ 3: the last group of four may pass n_pad; a multiple of 8).
SVT_INTRA_HD uint32_t dir_lpb(uint32_t per_block) { return per_block >= 256 ? 256u : per_block; }
SVT_INTRA_HD int dir_estride(int n_pad) { return (n_pad + 10) & ~7; }
// LDS pair dwords between the staged edges of consecutive blocks of a workgroup.  Lanes of `lpb` rows read a window of about lpb
// consecutive dwords of their block's edge, and a half wave (32 lanes, one LDS pass) holds 32 / lpb blocks: a stride that is
// lpb modulo 32 puts those windows on disjoint banks (2 * estride alone is 0 or 16 modulo 32: the open-loop search's 8x8 pass,
// 8 lanes per block, measured 50 % of its LDS cycles in bank conflicts).  Even, so that the 8-byte staging stores stay aligned.
SVT_INTRA_HD int dir_slot_stride(int estride, uint32_t lpb) {
    const int base = 2 * estride;
    return lpb < 32u ? base + (int)(((uint32_t)lpb - (uint32_t)base) & 31u) : base;
}
// dword offset of zone 2's column table (2 x 64 dwords) behind the workgroup's slots
SVT_INTRA_HD size_t dir_tab_offset(int estride, uint32_t lpb) { return (size_t)(256u >> __builtin_ctz(lpb)) * dir_slot_stride(estride, lpb); }
constexpr int DIR_TAB_DWORDS = 2 * 64;

struct DirLds {
    int lim_a, lim_l;        // last edge sample the reference may read: index NB_ORIGIN + max_base, max_base = (bw + bh - 1) << upsample
    int n_pad;               // the LDS copy continues with copies of it for one lane-row (+ 2) so that the pixel loop needs no bounds test
    int estride;
    uint32_t lpb, slots;
    int slot_stride;
    size_t tab_dword, bytes;
};
SVT_INTRA_HD DirLds dir_lds(int bw, int bh, int sample_bytes, int up_above, int up_left) {
    DirLds D;
    D.lim_a = NB_ORIGIN + ((bw + bh - 1) << up_above);
    D.lim_l = NB_ORIGIN + ((bw + bh - 1) << up_left);
    const int up = up_above > up_left ? up_above : up_left;
    D.n_pad = (D.lim_a > D.lim_l ? D.lim_a : D.lim_l) + ((16 / sample_bytes) << up) + 3;
    D.estride = dir_estride(D.n_pad);
    D.lpb = dir_lpb(intra_lanes(bw, bh, sample_bytes).per_block);
    D.slots = 256u >> __builtin_ctz(D.lpb);
    D.slot_stride = dir_slot_stride(D.estride, D.lpb);
    D.tab_dword = dir_tab_offset(D.estride, D.lpb);
    D.bytes = (D.tab_dword + DIR_TAB_DWORDS) * 4;
    return D;
}

// zone 2's per-angle tables of the left-edge terms, see DirMulti (kernel_intra.h)
template <typename Multi>
inline void dir_z2_tables(Multi& d) {
    d.z2_tab = 1;
    for (int a = 0; a < d.n; a++)
        for (int k = 0; k < 16; k++) {
            const int ys = -(int)d.dy[a] * (k + 1);
            const uint32_t sh = ((uint32_t)ys & 63u) >> 1;
            d.z2_w2[a][k] = (32u - sh) | (sh << 16);
            d.z2_ol[a][k] = 4 * (ys >> 6);
        }
}

// ---- chroma from luma: a lane takes a chunk of 4 (4-wide blocks) or 8 samples of a row; at most 64 lanes per block, slots blocks per workgroup ----
struct CflLanes { uint32_t nchunks, lpb, slots; };
SVT_INTRA_HD CflLanes cfl_lanes(uint32_t w, uint32_t h) {
    const uint32_t nchunks = (w / (w < 8 ? 4 : 8)) * h, lpb = nchunks < 64 ? nchunks : 64;
    return {nchunks, lpb, 256 / lpb};
}

// ---- The level map of a w x h coefficient block: (w + TX_PAD_HOR) * (h + TX_PAD_VER) + TX_PAD_END bytes = ndw dwords, written by lpb lanes
// per block (a dword each, or 16 bytes when pitch and pointer allow: wide), slots blocks per workgroup; row_magic divides by a row's dwords
struct LevelsGeom { uint32_t bytes, ndw, lpb, slots, row_magic; bool wide; };
SVT_INTRA_HD LevelsGeom levels_geom(uint32_t w, uint32_t h, size_t pitch, const void* ptr) {
    const uint32_t bytes = (w + 4) * (h + 6) + 16, ndw = bytes >> 2;
    const bool wide = (pitch & 15) == 0 && ((uintptr_t)ptr & 15) == 0;
    const uint32_t items = wide ? (ndw + 3) / 4 : ndw;
    uint32_t lpb = 1;
    while (lpb < items && lpb < 256) lpb <<= 1;
    return {bytes, ndw, lpb, 256 / lpb, (uint32_t)(0x100000000ull / ((w + 4) >> 2)) + 1u, wide};
}
// get_txb_wide / get_txb_high: a side of the packed coefficient block (a 64-sample side keeps its 32 low-frequency columns / rows)
SVT_INTRA_HDC uint32_t txb_side(int v) { return v > 32 ? 32u : (uint32_t)v; }

// ---- build_intra_predictors (kernel_bip.h): BIP_WAVES waves per workgroup, 64 / bip_lanes_per_block blocks per wave ----
constexpr int BIP_WAVES = 4;
// lanes per block: w + h + 1 edge samples in at most three rounds (the smoothing stage keeps three values per lane)
SVT_INTRA_HDC int bip_lanes_per_block(int w, int h) {
    const int need = (w + h + 1 + 2) / 3;
    int l = 4;
    while (l < need) l <<= 1;
    return l > 64 ? 64 : l;
}
// the ordering pass (bip_order_tile_kernel, svt_hip_intra.hip): tiles of BIP_ORDER_TILE consecutive blocks, a workgroup each
constexpr int BIP_ORDER_ITEMS = 4;
constexpr int BIP_ORDER_THREADS = 1024;
constexpr int BIP_ORDER_TILE = BIP_ORDER_THREADS * BIP_ORDER_ITEMS;
static_assert(BIP_ORDER_TILE == SVT_HIP_INTRA_ORDER_TILE, "header constant");

// ---- the group tables of svt_hip_encode_recon_frame_ex's two launches (group_table.h; kernel_cfl.h) ----
constexpr int LEVELS_MAX_GROUPS = 48;
struct LevelsGroupDev {
    const int32_t* coeff; uint8_t* levels;
    uint32_t levels_pitch, w, h, lpb, ndw, row_magic, nblocks, wg_end;
    uint32_t wide;                   // 16-byte stores (buffer and pitch 16-byte aligned)
};
struct LevelsFrameDesc { int32_t ngroups; LevelsGroupDev g[LEVELS_MAX_GROUPS]; };
static_assert(sizeof(LevelsFrameDesc) <= 4000, "kernel arguments");

constexpr int CFL_MAX_GROUPS = 16;      // the chroma transform sizes 4 .. 32 in both dimensions
struct CflGroupDev {
    const void* luma; void* cb; void* cr;
    const uint32_t* xy; const int32_t* alpha_cb; const int32_t* alpha_cr;
    uint32_t luma_stride, cb_stride, cr_stride, nblocks, w, h, lpb, wg_end;
    int32_t round_offset, num_pel_log2;
};
struct CflFrameDesc { int32_t ngroups; CflGroupDev g[CFL_MAX_GROUPS]; };
static_assert(sizeof(CflFrameDesc) <= 4000, "kernel arguments");

}  // namespace svtdev

namespace svthost {

// svt_hip_tune's dir_no_split and dir_split_target, and the device's CU count
struct IntraKnobs { int dir_no_split, dir_split_target, num_cu; };

constexpr size_t kIntraMaxBlocks = 0x7fffffffu;       // blocks of one batch call: the kernels count them in 32 bits

inline bool tx_side_ok(uint32_t v) { return v == 4 || v == 8 || v == 16 || v == 32 || v == 64; }
inline bool cfl_dim_ok(uint32_t v) { return v != 64 && tx_side_ok(v); }
inline bool intra_size_ok(int bw, int bh) {
    if (!tx_side_ok((uint32_t)bw) || !tx_side_ok((uint32_t)bh)) return false;
    const int m = bw > bh ? bw : bh, mn = bw < bh ? bw : bh;
    return m <= 4 * mn;     // the 19 TX sizes
}
// sample depths of the pixel entry points: 8 for uint8 samples; 8, 10 or 12 for uint16
inline bool sample_depth_ok(int is_16bit, int bd) { return bd == 8 || (is_16bit && (bd == 10 || bd == 12)); }
inline int intra_too_many() { return set_err(SVT_HIP_ERR_INVALID, "too many blocks for one launch"); }
// workgroups of `per_wg` items each over n items (n <= kIntraMaxBlocks * 512: no overflow in 64 bits)
inline uint64_t intra_wgs(uint64_t n, uint64_t per_wg) { return (n + per_wg - 1) / per_wg; }

// angles per workgroup (chunk) and the parts over grid.y: all n angles in one part when the batch alone gives `want` workgroups, else
// split (each part re-stages the edges).  No angles: no part.
inline void dir_angle_split(int n, size_t grid, size_t want, bool no_split, int& chunk, uint32_t& grid_y) {
    size_t parts = (no_split || grid >= want) ? 1 : (want + grid - 1) / grid;
    if (parts > (size_t)n) parts = (size_t)n;
    chunk = n ? (int)((n + parts - 1) / parts) : 1;
    grid_y = n ? (uint32_t)((n + chunk - 1) / chunk) : 0;
}

// ---- cfl_ac_kernel: svt_hip_cfl_luma_subsampling_420_batch (in_mode 0 / 1: 8- / 16-bit luma), svt_hip_subtract_average_batch (in_mode 2) ----
// the chroma block under a width x height luma block with its rounding terms (sides the plan below refuses give 0 for num_pel_log2)
struct Cfl420Shape { uint32_t w, h; int round_offset, num_pel_log2; };
inline Cfl420Shape cfl_420_shape(uint32_t width, uint32_t height) {
    Cfl420Shape S = {width >> 1, height >> 1, 0, 0};
    if (!cfl_dim_ok(S.w) || !cfl_dim_ok(S.h)) return S;
    S.round_offset = (int)(S.w * S.h / 2);
    S.num_pel_log2 = __builtin_ctz(S.w) + __builtin_ctz(S.h);
    return S;
}
struct CflAcPlan { int in_mode; uint32_t grid, lpb, nblocks; };
inline int cfl_ac_plan(CflAcPlan& P, int in_mode, const void* d_luma, const void* d_q3, uint32_t q3_line, size_t q3_block_pitch, uint32_t w, uint32_t h,
                       int num_pel_log2, size_t nblocks) {
    if (!d_q3 || (in_mode != 2 && !d_luma)) return set_err(SVT_HIP_ERR_INVALID, "NULL buffer");
    if (!cfl_dim_ok(w) || !cfl_dim_ok(h)) return set_err(SVT_HIP_ERR_INVALID, "chroma block %ux%u", w, h);
    if (q3_line < w || q3_block_pitch < (size_t)q3_line * (h - 1) + w) return set_err(SVT_HIP_ERR_INVALID, "q3 layout: line %u, block pitch %zu", q3_line, q3_block_pitch);
    if (num_pel_log2 < 0 || num_pel_log2 > 31) return set_err(SVT_HIP_ERR_INVALID, "num_pel_log2 %d", num_pel_log2);
    if (nblocks > 0x7fffffffu / 64) return intra_too_many();          // (the kernel counts LANES in 32 bits)
    P.in_mode = in_mode;
    P.lpb = svtdev::cfl_lanes(w, h).lpb;
    P.grid = (uint32_t)intra_wgs((uint64_t)nblocks * P.lpb, 256);
    P.nblocks = (uint32_t)nblocks;
    return SVT_HIP_OK;
}

// ---- svt_hip_cfl_predict_batch ----
struct CflPredictPlan { uint32_t grid, sh, nblocks; int hi; };
inline int cfl_predict_plan(CflPredictPlan& P, const void* d_ac_q3, const void* d_pred, const void* d_dst, const void* d_alpha_q3, uint32_t q3_line,
                            uint32_t pred_stride, uint32_t dst_stride, int bit_depth, uint32_t width, uint32_t height, int is_16bit, size_t nblocks) {
    if (!d_ac_q3 || !d_pred || !d_dst || !d_alpha_q3) return set_err(SVT_HIP_ERR_INVALID, "NULL buffer");
    if (!cfl_dim_ok(width) || !cfl_dim_ok(height)) return set_err(SVT_HIP_ERR_INVALID, "chroma block %ux%u", width, height);
    if (!sample_depth_ok(is_16bit, bit_depth)) return set_err(SVT_HIP_ERR_INVALID, "bit depth %d", bit_depth);
    if (q3_line < width || pred_stride < width || dst_stride < width) return set_err(SVT_HIP_ERR_INVALID, "stride smaller than the block");
    if (nblocks > kIntraMaxBlocks) return intra_too_many();
    P.sh = (uint32_t)__builtin_ctz(svtdev::cfl_lanes(width, height).nchunks);       // a lane per chunk: a power of two, 4 .. 128
    P.grid = (uint32_t)intra_wgs((uint64_t)nblocks << P.sh, 256);                   // (at most 2^30: half a workgroup per block at 32x32)
    P.nblocks = (uint32_t)nblocks;
    P.hi = (1 << bit_depth) - 1;
    return SVT_HIP_OK;
}

// ---- svt_hip_txb_init_levels_batch ----
struct LevelsPlan { svtdev::LevelsGeom lg; uint32_t grid, nblocks; };
inline int txb_init_levels_plan(LevelsPlan& P, const void* d_coeff, size_t coeff_block_pitch, const void* d_levels_buf, size_t levels_block_pitch, uint32_t width,
                                uint32_t height, size_t nblocks) {
    if (!d_coeff || !d_levels_buf) return set_err(SVT_HIP_ERR_INVALID, "NULL buffer");
    if (!tx_side_ok(width) || !tx_side_ok(height)) return set_err(SVT_HIP_ERR_INVALID, "block %ux%u", width, height);
    P.lg = svtdev::levels_geom(width, height, levels_block_pitch, d_levels_buf);
    if (levels_block_pitch < P.lg.bytes || (levels_block_pitch & 3) || ((uintptr_t)d_levels_buf & 3))
        return set_err(SVT_HIP_ERR_INVALID, "levels buffer: %zu B per block (need >= %u, multiple of 4, 4-byte aligned)", levels_block_pitch, P.lg.bytes);
    if (coeff_block_pitch < (size_t)width * height) return set_err(SVT_HIP_ERR_INVALID, "coeff_block_pitch %zu", coeff_block_pitch);
    if (nblocks > kIntraMaxBlocks) return intra_too_many();
    P.grid = (uint32_t)intra_wgs(nblocks, P.lg.slots);
    P.nblocks = (uint32_t)nblocks;
    return SVT_HIP_OK;
}

// ---- svt_hip_intra_pred_batch, and the open-loop search's segments (multi_n angles on edges staged once; 0: the dx, dy of the call) ----
enum IntraFamily { INTRA_FAM_PLAIN, INTRA_FAM_DIR };      // intra_pred_kernel<T, MODE, WIDE, IU>, intra_dir_kernel<T, MODE, NPX, TAB>
struct IntraPredPlan {
    IntraFamily family;
    int is_16bit, mode;
    bool wide; int iu;               // plain: 16 bytes per lane and iu blocks per lane, or the narrow form (a row per lane, iu 1)
    int npx; bool tab;               // directional: samples per lane; zone 2 with the host's per-angle tables (dir_z2_tables)
    uint32_t grid_x, grid_y, nblocks;
    size_t lds_bytes;
    uint32_t dc_magic;               // plain
    svtdev::DirLds lds;              // directional
    int chunk;                       // directional: angles per workgroup (DirMulti::chunk)
};
inline int intra_pred_plan(IntraPredPlan& P, const void* d_dst, const void* d_above, const void* d_left, int32_t nb_pitch, int mode, int bw, int bh,
                           int upsample_above, int upsample_left, int dx, int dy, int is_16bit, int bd, size_t nblocks, int multi_n, const IntraKnobs& knobs) {
    using namespace svtdev;
    if (!d_dst || !d_above || !d_left) return set_err(SVT_HIP_ERR_INVALID, "NULL buffer");
    if (mode < 0 || mode >= SVT_INTRA_MODES) return set_err(SVT_HIP_ERR_INVALID, "intra mode %d", mode);
    if (!intra_size_ok(bw, bh)) return set_err(SVT_HIP_ERR_INVALID, "block %dx%d is not an AV1 transform size", bw, bh);
    if (!sample_depth_ok(is_16bit, bd)) return set_err(SVT_HIP_ERR_INVALID, "bit depth %d", bd);
    if ((upsample_above | upsample_left) & ~1) return set_err(SVT_HIP_ERR_INVALID, "upsample flags");
    const bool dir = mode >= SVT_INTRA_Z1;
    if (dir) {
        if (dx <= 0 || dy <= 0) return set_err(SVT_HIP_ERR_INVALID, "dx/dy must be positive");
        const int need = NB_ORIGIN + (((bw + bh) << 1) + 2);
        if (nb_pitch < need) return set_err(SVT_HIP_ERR_INVALID, "nb_pitch %d < %d", nb_pitch, need);
    } else if (nb_pitch < NB_ORIGIN + (bw > bh ? bw : bh)) {
        return set_err(SVT_HIP_ERR_INVALID, "nb_pitch %d too small", nb_pitch);
    }
    if (nblocks > kIntraMaxBlocks) return intra_too_many();
    const int es = is_16bit ? 2 : 1;
    const IntraLanes L = intra_lanes(bw, bh, es);
    uint64_t grid = intra_wgs((uint64_t)L.per_block * nblocks, 256);
    if (grid > kMaxLaunchWgs) return intra_too_many();
    P = IntraPredPlan{};
    P.family = dir ? INTRA_FAM_DIR : INTRA_FAM_PLAIN;
    P.is_16bit = is_16bit ? 1 : 0; P.mode = mode; P.nblocks = (uint32_t)nblocks;
    P.grid_y = 1; P.chunk = 1; P.iu = 1;
    if (!dir) {
        P.wide = L.ppl == 16 / es;
        if (P.wide) { P.iu = intra_wide_iu(mode); grid = intra_wgs(grid, (uint64_t)P.iu); }
        P.dc_magic = intra_dc_magic(intra_dc_count(mode, bw, bh));
    }
    // grid * 256 must be a multiple of per_block so that a lane keeps its (row, column) across iterations
    if (L.per_block > 256) grid = (grid + 1) & ~(uint64_t)1;
    P.grid_x = (uint32_t)grid;
    if (dir) {
        P.npx = L.ppl;
        P.lds = dir_lds(bw, bh, es, upsample_above, upsample_left);
        P.lds_bytes = P.lds.bytes;
        // see DirMulti: one lane per row, no up-sampling
        P.tab = multi_n > 0 && mode == SVT_INTRA_Z2 && L.lanes_per_row == 1 && (upsample_above | upsample_left) == 0;
        // angles per workgroup: all of them when the batch alone gives every CU a few workgroups, else split over grid.y (each part re-stages the edges)
        if (multi_n > 0) dir_angle_split(multi_n, (size_t)grid, (size_t)knobs.dir_split_target * (size_t)knobs.num_cu, knobs.dir_no_split != 0, P.chunk, P.grid_y);
    }
    return SVT_HIP_OK;
}

// ---- svt_hip_filter_intra_edge_batch, svt_hip_upsample_intra_edge_batch: an edge per workgroup ----
struct EdgePlan { uint32_t grid, threads, nblocks; int bd; };
inline int filter_edge_plan(EdgePlan& P, const void* d_edges, int32_t nb_pitch, int sz, int strength, size_t nblocks) {
    if (!d_edges) return set_err(SVT_HIP_ERR_INVALID, "NULL buffer");
    if (sz < 1 || sz > 129 || strength < 0 || strength > 3 || nb_pitch < svtdev::NB_ORIGIN + sz)
        return set_err(SVT_HIP_ERR_INVALID, "edge sz %d strength %d pitch %d", sz, strength, nb_pitch);
    if (nblocks > kIntraMaxBlocks) return intra_too_many();
    P = EdgePlan{(uint32_t)nblocks, 256, (uint32_t)nblocks, 0};
    return SVT_HIP_OK;
}
inline int upsample_edge_plan(EdgePlan& P, const void* d_edges, int32_t nb_pitch, int sz, int is_16bit, int bd, size_t nblocks) {
    if (!d_edges) return set_err(SVT_HIP_ERR_INVALID, "NULL buffer");
    if (sz < 1 || sz > 16 || nb_pitch < svtdev::NB_ORIGIN + 2 * sz) return set_err(SVT_HIP_ERR_INVALID, "upsample sz %d pitch %d", sz, nb_pitch);
    if (nblocks > kIntraMaxBlocks) return intra_too_many();
    P = EdgePlan{(uint32_t)nblocks, 64, (uint32_t)nblocks, is_16bit ? bd : 8};
    return SVT_HIP_OK;
}

// ---- svt_hip_build_intra_predictors_batch and _ordered_batch (the caller of the ordered form has refused a NULL order) ----
struct BipPlan { int w, h; uint32_t grid, threads, nblocks; };
inline int bip_plan(BipPlan& P, const void* d_dst, int32_t dst_stride, size_t dst_block_pitch, const void* d_dst_offsets, const void* d_top_neigh,
                    const void* d_left_neigh, int32_t neigh_pitch, const void* d_blocks, int tx_size, int is_16bit, int bd, size_t nblocks) {
    if (!d_dst || !d_top_neigh || !d_left_neigh || !d_blocks) return set_err(SVT_HIP_ERR_INVALID, "NULL buffer");
    if (tx_size < 0 || tx_size >= SVT_TX_SIZES_ALL) return set_err(SVT_HIP_ERR_INVALID, "tx_size %d", tx_size);
    if (!sample_depth_ok(is_16bit, bd)) return set_err(SVT_HIP_ERR_INVALID, "bit depth %d", bd);
    const int w = kTxW[tx_size], h = kTxH[tx_size];
    if (neigh_pitch < 1 + 2 * (w > h ? w : h)) return set_err(SVT_HIP_ERR_INVALID, "neigh_pitch %d < %d", neigh_pitch, 1 + 2 * (w > h ? w : h));
    if (dst_stride < w) return set_err(SVT_HIP_ERR_INVALID, "dst_stride %d < width %d", dst_stride, w);
    if (!d_dst_offsets && dst_block_pitch == 0) return set_err(SVT_HIP_ERR_INVALID, "dst_block_pitch 0 without offsets");
    if (nblocks > kIntraMaxBlocks) return intra_too_many();
    const uint64_t per_wg = (uint64_t)svtdev::BIP_WAVES * (uint64_t)(64 / svtdev::bip_lanes_per_block(w, h));       // blocks per workgroup
    P = BipPlan{w, h, (uint32_t)intra_wgs(nblocks, per_wg), 64u * svtdev::BIP_WAVES, (uint32_t)nblocks};
    return SVT_HIP_OK;
}

// ---- svt_hip_intra_order_blocks_batch ----
struct BipOrderPlan { int w, h; uint32_t grid, threads, nblocks; };
inline int bip_order_plan(BipOrderPlan& P, const void* d_blocks, const void* d_order, int tx_size, size_t nblocks) {
    if (!d_blocks || !d_order) return set_err(SVT_HIP_ERR_INVALID, "NULL buffer");
    if (tx_size < 0 || tx_size >= SVT_TX_SIZES_ALL) return set_err(SVT_HIP_ERR_INVALID, "tx_size %d", tx_size);
    if (nblocks > kIntraMaxBlocks) return set_err(SVT_HIP_ERR_INVALID, "too many blocks");
    P = BipOrderPlan{kTxW[tx_size], kTxH[tx_size], (uint32_t)intra_wgs(nblocks, svtdev::BIP_ORDER_TILE), svtdev::BIP_ORDER_THREADS, (uint32_t)nblocks};
    return SVT_HIP_OK;
}

// ---- svt_hip_encode_recon_frame_ex: the chroma-from-luma groups and the level maps beside the transform chain ----
// The call's own arguments, before its groups are looked at (svt_hip_intra.hip checks the transform groups, tx_plan.h, between the two).
inline int frame_ex_args_check(const svt_hip_frame_group* groups, int ngroups, int first_chroma_group, const svt_hip_frame_cfl_group* cfl, int ncfl, int is_16bit,
                               int bd) {
    if (ngroups < 0 || ncfl < 0 || (ngroups && !groups) || (ncfl && !cfl)) return set_err(SVT_HIP_ERR_INVALID, "group lists");
    if (ngroups > 256) return set_err(SVT_HIP_ERR_INVALID, "more than 256 groups in one call");
    if (ncfl > svtdev::CFL_MAX_GROUPS)
        return set_err(SVT_HIP_ERR_INVALID, "%d chroma-from-luma groups (at most %d: one per chroma transform size)", ncfl, svtdev::CFL_MAX_GROUPS);
    if (ncfl && (first_chroma_group < 0 || first_chroma_group > ngroups)) return set_err(SVT_HIP_ERR_INVALID, "first_chroma_group %d of %d", first_chroma_group, ngroups);
    if (!sample_depth_ok(is_16bit, bd)) return set_err(SVT_HIP_ERR_INVALID, "bit depth %d", bd);
    return SVT_HIP_OK;
}
inline uint32_t cfl_group_wgs(const svt_hip_frame_cfl_group& C) { return (C.nblocks - 1) / svtdev::cfl_lanes(C.width, C.height).slots + 1; }
inline uint32_t levels_group_wgs(uint32_t nblocks, const svtdev::LevelsGeom& lg) { return (uint32_t)intra_wgs(nblocks, lg.slots); }
inline svtdev::LevelsGeom levels_group_geom(const svt_hip_frame_group& G, const svt_hip_frame_levels& L) {
    return svtdev::levels_geom(svtdev::txb_side(kTxW[G.tx_size]), svtdev::txb_side(kTxH[G.tx_size]), L.levels_block_pitch, L.d_levels_buf);
}
// Every chroma-from-luma group and every level map (levels may be null: none) of groups frame_groups_check accepted.  Enqueues nothing;
// ncfl_live receives the number of non-empty chroma-from-luma groups (all of one launch: ncfl <= CFL_MAX_GROUPS).
inline int frame_ex_groups_check(const svt_hip_frame_group* groups, int ngroups, const svt_hip_frame_cfl_group* cfl, int ncfl, const svt_hip_frame_levels* levels,
                                 int& ncfl_live) {
    uint64_t cfl_wgs = 0;
    ncfl_live = 0;
    for (int g = 0; g < ncfl; g++) {
        const svt_hip_frame_cfl_group& C = cfl[g];
        if (C.nblocks == 0) continue;
        if (!C.d_luma_recon || !C.d_pred_cb || !C.d_pred_cr || !C.d_xy || !C.d_alpha_q3_cb || !C.d_alpha_q3_cr)
            return set_err(SVT_HIP_ERR_INVALID, "chroma-from-luma group %d: NULL member", g);
        if (!cfl_dim_ok(C.width) || !cfl_dim_ok(C.height)) return set_err(SVT_HIP_ERR_INVALID, "chroma-from-luma group %d: chroma block %ux%u", g, C.width, C.height);
        if (C.luma_stride < 2 * C.width || C.pred_stride_cb < C.width || C.pred_stride_cr < C.width)
            return set_err(SVT_HIP_ERR_INVALID, "chroma-from-luma group %d: stride smaller than the block", g);
        if ((cfl_wgs += cfl_group_wgs(C)) > kMaxLaunchWgs) return set_err(SVT_HIP_ERR_INVALID, "chroma-from-luma group %d: too many blocks for one launch", g);
        ncfl_live++;
    }
    if (levels)
        for (int g = 0; g < ngroups; g++) {
            const svt_hip_frame_levels& L = levels[g];
            if (!groups[g].nblocks || !L.d_levels_buf) continue;
            const size_t bytes = levels_group_geom(groups[g], L).bytes;
            if (L.levels_block_pitch < bytes || (L.levels_block_pitch & 3) || ((uintptr_t)L.d_levels_buf & 3) || L.levels_block_pitch > 0xffffffffu)
                return set_err(SVT_HIP_ERR_INVALID, "group %d: levels buffer %zu B per block (need >= %zu, multiple of 4, 4-byte aligned)", g, L.levels_block_pitch, bytes);
            if (groups[g].nblocks > kMaxLaunchWgs) return set_err(SVT_HIP_ERR_INVALID, "group %d: too many blocks for one launch", g);
        }
    return SVT_HIP_OK;
}
// The launches of a call that frame_ex_groups_check accepted: launch(desc, total_workgroups) -> int (0 = OK).  One launch for the
// chroma-from-luma groups; one per LEVELS_MAX_GROUPS level maps.
template <typename Launch>
inline int cfl_frame_enqueue(const svt_hip_frame_cfl_group* cfl, int ncfl, Launch&& launch) {
    GroupTable<svtdev::CflFrameDesc, svtdev::CFL_MAX_GROUPS> tab;
    for (int g = 0; g < ncfl; g++) {
        const svt_hip_frame_cfl_group& C = cfl[g];
        if (C.nblocks == 0) continue;
        svtdev::CflGroupDev* D = tab.add(cfl_group_wgs(C), launch);
        if (!D) return tab.rc;
        D->lpb = svtdev::cfl_lanes(C.width, C.height).lpb;
        D->luma = C.d_luma_recon; D->cb = C.d_pred_cb; D->cr = C.d_pred_cr; D->xy = C.d_xy; D->alpha_cb = C.d_alpha_q3_cb; D->alpha_cr = C.d_alpha_q3_cr;
        D->luma_stride = C.luma_stride; D->cb_stride = C.pred_stride_cb; D->cr_stride = C.pred_stride_cr; D->nblocks = C.nblocks; D->w = C.width; D->h = C.height;
        D->round_offset = (int32_t)(C.width * C.height / 2);
        D->num_pel_log2 = __builtin_ctz(C.width) + __builtin_ctz(C.height);
    }
    return tab.flush(launch);
}
template <typename Launch>
inline int levels_frame_enqueue(const svt_hip_frame_group* groups, const svt_hip_frame_levels* levels, int ngroups, Launch&& launch) {
    GroupTable<svtdev::LevelsFrameDesc, svtdev::LEVELS_MAX_GROUPS> tab;
    for (int g = 0; g < ngroups; g++) {
        const svt_hip_frame_group& G = groups[g];
        const svt_hip_frame_levels& L = levels[g];
        if (!G.nblocks || !L.d_levels_buf) continue;
        const svtdev::LevelsGeom lg = levels_group_geom(G, L);
        svtdev::LevelsGroupDev* D = tab.add(levels_group_wgs(G.nblocks, lg), launch);
        if (!D) return tab.rc;
        D->coeff = G.d_qcoeff; D->levels = L.d_levels_buf; D->levels_pitch = (uint32_t)L.levels_block_pitch;
        D->w = svtdev::txb_side(kTxW[G.tx_size]); D->h = svtdev::txb_side(kTxH[G.tx_size]); D->lpb = lg.lpb; D->ndw = lg.ndw;
        D->row_magic = lg.row_magic; D->nblocks = G.nblocks; D->wide = lg.wide;
    }
    return tab.flush(launch);
}

// ---- the open-loop intra search's three zones in one launch (ois_dir3_kernel: 8x8 / 16x16 8-bit blocks, a lane per row, SAD mode) ----
// n[z]: the angles of zone z's segment.  Angles per workgroup, per zone: as separate launches each zone wants dir_split_target (4)
// workgroups per CU before it stops spreading its angles over grid.y; with the three zones in one launch the sum counts - swept 1 .. 8
// on the 1080p search: 1 is best for 8x8 (0.0526 against 0.0567 ms at 4) and 16x16 (0.0443 against 0.0471)
struct OisDir3Plan {
    svtdev::DirLds lds;
    uint32_t grid_x, grid_y, nblocks;
    int chunk[3];
    uint32_t y_end[2];
};
inline void ois_dir3_plan(OisDir3Plan& P, uint32_t bsize, size_t nblocks, const int n[3], const IntraKnobs& knobs) {
    P.lds = svtdev::dir_lds((int)bsize, (int)bsize, 1, 0, 0);
    P.grid_x = (uint32_t)intra_wgs((uint64_t)P.lds.lpb * nblocks, 256);        // (nblocks <= 2^31 / 256: ois_job)
    P.nblocks = (uint32_t)nblocks;
    uint32_t gy[3];
    for (int z = 0; z < 3; z++) dir_angle_split(n[z], P.grid_x, (size_t)knobs.num_cu, knobs.dir_no_split != 0, P.chunk[z], gy[z]);
    P.y_end[0] = gy[0]; P.y_end[1] = gy[0] + gy[1];
    P.grid_y = gy[0] + gy[1] + gy[2];
}

}  // namespace svthost

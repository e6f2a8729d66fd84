// svt_hip_intra.hip — entry points of the intra family of libsvt_hip_dsp.so (include/svt_hip_dsp.h): intra prediction, edge
// filters, chroma-from-luma helpers, txb_init_levels, the open-loop intra search and their drop-ins.  A device-pointer entry point is
// require_init, the empty-batch return, its plan (intra_plan.h: every check, the grid, the LDS bytes) and one switch to the
// instantiation with the launch.
#include "host_common.h"
#include "kernel_cfl.h"
#include "kernel_intra.h"
#include "kernel_bip.h"
#include "kernel_ois.h"
#include "intra_plan.h"
#include "ois_plan.h"
#include "tx_plan.h"

using namespace svtdev;
using namespace svthost;

// the knobs the family's plans read (intra_plan.h): filled from the globals of host_common.h here and nowhere else
static IntraKnobs intra_knobs() { return IntraKnobs{g_tune_dir_no_split, g_tune_dir_split_target, g_num_cu}; }

// ---- K11 chroma-from-luma helpers + av1_txb_init_levels ----
// f(T{}) with the sample type, for the uint8_t / uint16_t launch pairs
template <typename F> static void by_sample(int is_16bit, F&& f) { if (is_16bit) f(uint16_t{}); else f(uint8_t{}); }

static int cfl_ac_launch(int in_mode, const void* d_luma, uint32_t luma_stride, size_t luma_block_pitch, const uint32_t* d_xy,
                         int16_t* d_q3, uint32_t q3_line, size_t q3_block_pitch, uint32_t w, uint32_t h, int subtract,
                         int round_offset, int num_pel_log2, size_t nblocks, void* stream, const char* what) {
    if (int rc = require_init()) return rc;
    if (nblocks == 0) return SVT_HIP_OK;
    CflAcPlan p;
    if (int rc = cfl_ac_plan(p, in_mode, d_luma, d_q3, q3_line, q3_block_pitch, w, h, num_pel_log2, nblocks)) return rc;
#define CFL_AC(IN)                                                                                                          \
    hipLaunchKernelGGL((cfl_ac_kernel<IN>), dim3(p.grid), dim3(256), 0, (hipStream_t)stream, d_luma, luma_stride,           \
                       luma_block_pitch, d_xy, d_q3, q3_line, q3_block_pitch, w, h, p.lpb, subtract, round_offset, num_pel_log2, \
                       p.nblocks)
    if (p.in_mode == 0) CFL_AC(0); else if (p.in_mode == 1) CFL_AC(1); else CFL_AC(2);
#undef CFL_AC
    return launch_status(what);
}

extern "C" int svt_hip_cfl_luma_subsampling_420_batch(const void* d_luma, uint32_t luma_stride, size_t luma_block_pitch,
                                                      const uint32_t* d_xy, int is_16bit, int16_t* d_q3, uint32_t q3_line,
                                                      size_t q3_block_pitch, uint32_t width, uint32_t height,
                                                      int subtract_average, size_t nblocks, void* stream) {
    if ((width & 1) || (height & 1)) return set_err(SVT_HIP_ERR_INVALID, "luma block %ux%u", width, height);
    const Cfl420Shape c = cfl_420_shape(width, height);
    return cfl_ac_launch(is_16bit ? 1 : 0, d_luma, luma_stride, luma_block_pitch, d_xy, d_q3, q3_line, q3_block_pitch, c.w, c.h,
                         subtract_average ? 1 : 0, c.round_offset, c.num_pel_log2, nblocks, stream, "cfl_luma_subsampling_420");
}

extern "C" int svt_hip_subtract_average_batch(int16_t* d_q3, uint32_t q3_line, size_t q3_block_pitch, uint32_t width,
                                              uint32_t height, int32_t round_offset, int32_t num_pel_log2, size_t nblocks,
                                              void* stream) {
    return cfl_ac_launch(2, nullptr, 0, 0, nullptr, d_q3, q3_line, q3_block_pitch, width, height, 1, round_offset,
                         num_pel_log2, nblocks, stream, "subtract_average");
}

extern "C" int svt_hip_cfl_predict_batch(const int16_t* d_ac_q3, uint32_t q3_line, size_t q3_block_pitch, const void* d_pred,
                                         uint32_t pred_stride, void* d_dst, uint32_t dst_stride, const uint32_t* d_xy,
                                         const int32_t* d_alpha_q3, int bit_depth, uint32_t width, uint32_t height,
                                         int is_16bit, size_t nblocks, void* stream) {
    if (int rc = require_init()) return rc;
    if (nblocks == 0) return SVT_HIP_OK;
    CflPredictPlan p;
    if (int rc = cfl_predict_plan(p, d_ac_q3, d_pred, d_dst, d_alpha_q3, q3_line, pred_stride, dst_stride, bit_depth, width, height, is_16bit, nblocks)) return rc;
    by_sample(is_16bit, [&](auto t) {
        using T = decltype(t);
        hipLaunchKernelGGL((cfl_predict_kernel<T>), dim3(p.grid), dim3(256), 0, (hipStream_t)stream, d_ac_q3, q3_line, q3_block_pitch, (const T*)d_pred,
                           pred_stride, (T*)d_dst, dst_stride, d_xy, d_alpha_q3, p.hi, width, height, p.sh, p.nblocks);
    });
    return launch_status("cfl_predict");
}

extern "C" int svt_hip_txb_init_levels_batch(const int32_t* d_coeff, size_t coeff_block_pitch, uint8_t* d_levels_buf,
                                             size_t levels_block_pitch, uint32_t width, uint32_t height, size_t nblocks,
                                             void* stream) {
    if (int rc = require_init()) return rc;
    if (nblocks == 0) return SVT_HIP_OK;
    LevelsPlan p;
    if (int rc = txb_init_levels_plan(p, d_coeff, coeff_block_pitch, d_levels_buf, levels_block_pitch, width, height, nblocks)) return rc;
    hipLaunchKernelGGL(p.lg.wide ? txb_init_levels_kernel<true> : txb_init_levels_kernel<false>, dim3(p.grid), dim3(256), 0, (hipStream_t)stream, d_coeff,
                       coeff_block_pitch, d_levels_buf, levels_block_pitch, width, height, p.lg.lpb, p.lg.ndw, p.lg.row_magic, p.nblocks);
    return launch_status("txb_init_levels");
}

// ---- the frame call with its chroma-from-luma step and level maps (header: svt_hip_encode_recon_frame_ex) ----
extern "C" int svt_hip_encode_recon_frame_ex(const svt_hip_frame_group* groups, int ngroups, int first_chroma_group,
                                             const svt_hip_frame_cfl_group* cfl, int ncfl, const svt_hip_frame_levels* levels,
                                             int is_16bit, int bd, const int16_t* zbin, const int16_t* round, const int16_t* quant,
                                             const int16_t* quant_shift, const int16_t* dequant, void* stream) {
    if (int rc = require_init()) return rc;
    // everything is validated before anything is enqueued
    if (int rc = frame_ex_args_check(groups, ngroups, first_chroma_group, cfl, ncfl, is_16bit, bd)) return rc;
    if (int rc = frame_groups_check(groups, ngroups, tx_knobs())) return rc;
    int ncfl_live = 0;
    if (int rc = frame_ex_groups_check(groups, ngroups, cfl, ncfl, levels, ncfl_live)) return rc;
    hipStream_t s = (hipStream_t)stream;
    // stream order carries the dependencies: luma reconstruction -> chroma-from-luma prediction -> chroma encode -> level maps
    const int n_first = ncfl_live ? first_chroma_group : ngroups;
    if (int rc = svt_hip_encode_recon_frame(groups, n_first, is_16bit, bd, zbin, round, quant, quant_shift, dequant, stream)) return rc;
    if (ncfl_live) {
        const int hi = (1 << bd) - 1;
        if (int rc = cfl_frame_enqueue(cfl, ncfl, [&](const CflFrameDesc& cd, uint32_t total) {
                by_sample(is_16bit, [&](auto t) { hipLaunchKernelGGL((cfl_frame_kernel<decltype(t)>), dim3(total), dim3(256), 0, s, cd, hi); });
                return launch_status("cfl_frame");
            })) return rc;
        if (int rc = svt_hip_encode_recon_frame(groups + n_first, ngroups - n_first, is_16bit, bd, zbin, round, quant, quant_shift, dequant, stream)) return rc;
    }
    if (!levels) return SVT_HIP_OK;
    return levels_frame_enqueue(groups, levels, ngroups, [&](const LevelsFrameDesc& fd, uint32_t total) -> int {
        hipLaunchKernelGGL(levels_frame_kernel, dim3(total), dim3(256), 0, s, fd);
        return launch_status("levels_frame");
    });
}

// multi (directional modes only): several (dx, dy) of the same zone in one launch on edges staged once, see DirMulti
static int intra_pred_impl(void* d_dst, int32_t dst_stride, size_t dst_block_pitch,
                           const uint32_t* d_dst_offsets, const void* d_above, const void* d_left,
                           int32_t nb_pitch, int mode, int bw, int bh, int upsample_above,
                           int upsample_left, int dx, int dy, int is_16bit, int bd, size_t nblocks,
                           void* stream, const DirMulti* multi) {
    if (int rc = require_init()) return rc;
    if (nblocks == 0) return SVT_HIP_OK;
    IntraPredPlan p;
    if (int rc = intra_pred_plan(p, d_dst, d_above, d_left, nb_pitch, mode, bw, bh, upsample_above, upsample_left, dx, dy, is_16bit, bd, nblocks, multi ? multi->n : 0,
                                 intra_knobs()))
        return rc;
    hipStream_t s = (hipStream_t)stream;
    if (p.family == INTRA_FAM_DIR) {
        DirMulti dm;
        if (multi) dm = *multi; else dm.n = 0;
        dm.z2_tab = 0;
        if (p.tab) dir_z2_tables(dm);
        dm.chunk = p.chunk;
#define IDL(T, M, P, TB)                                                                                                     \
    hipLaunchKernelGGL((intra_dir_kernel<T, M, P, TB>), dim3(p.grid_x, p.grid_y), dim3(256), p.lds_bytes, s, (T*)d_dst, dst_stride, \
                       dst_block_pitch, d_dst_offsets, (const T*)d_above, (const T*)d_left, nb_pitch, bw, bh,               \
                       upsample_above, upsample_left, dx, dy, p.lds.lim_a, p.lds.lim_l, p.lds.n_pad, bd, p.nblocks, dm)
#define IDM(T, P)                                                                                                             \
    switch (mode) {                                                                                                           \
    case SVT_INTRA_Z1: IDL(T, IM_Z1, P, false); break; default: IDL(T, IM_Z3, P, false); break;                                \
    case SVT_INTRA_Z2: if (p.tab) IDL(T, IM_Z2, P, true); else IDL(T, IM_Z2, P, false); break;                                  \
    }
        // samples per lane is a template parameter: 4 / 8 / 16 for bytes, 4 / 8 for 16-bit samples
        if (is_16bit) { if (p.npx == 8) { IDM(uint16_t, 8) } else { IDM(uint16_t, 4) } }
        else if (p.npx == 16) { IDM(uint8_t, 16) } else if (p.npx == 8) { IDM(uint8_t, 8) } else { IDM(uint8_t, 4) }
#undef IDM
#undef IDL
        return launch_status("intra_dir");
    }
#define IPL(T, M)                                                                                                     \
    if (p.wide)                                                                                                       \
        hipLaunchKernelGGL((intra_pred_kernel<T, M, true, intra_wide_iu(M)>), dim3(p.grid_x), dim3(256), 0, s, (T*)d_dst, dst_stride, \
                           dst_block_pitch, d_dst_offsets, (const T*)d_above, (const T*)d_left, nb_pitch, bw, bh, bd,    \
                           p.dc_magic, p.nblocks);                                                                    \
    else                                                                                                              \
        hipLaunchKernelGGL((intra_pred_kernel<T, M, false, 1>), dim3(p.grid_x), dim3(256), 0, s, (T*)d_dst, dst_stride, \
                           dst_block_pitch, d_dst_offsets, (const T*)d_above, (const T*)d_left, nb_pitch, bw, bh, bd,    \
                           p.dc_magic, p.nblocks)
#define IPM(T)                                                                                                        \
    switch (mode) {                                                                                                   \
    case SVT_INTRA_DC: IPL(T, IM_DC); break; case SVT_INTRA_V: IPL(T, IM_V); break; case SVT_INTRA_H: IPL(T, IM_H); break; \
    case SVT_INTRA_SMOOTH: IPL(T, IM_SMOOTH); break; case SVT_INTRA_SMOOTH_V: IPL(T, IM_SMOOTH_V); break;             \
    case SVT_INTRA_SMOOTH_H: IPL(T, IM_SMOOTH_H); break; case SVT_INTRA_PAETH: IPL(T, IM_PAETH); break;               \
    case SVT_INTRA_DC_TOP: IPL(T, IM_DC_TOP); break; case SVT_INTRA_DC_LEFT: IPL(T, IM_DC_LEFT); break;               \
    default: IPL(T, IM_DC_128); break;                                                                                \
    }
    if (is_16bit) { IPM(uint16_t) } else { IPM(uint8_t) }
#undef IPM
#undef IPL
    return launch_status("intra_pred");
}
// (intra_wide_iu takes an SVT_INTRA_* mode: the kernels' IM_* numbers of the non-directional modes are the same)
static_assert((int)IM_DC == SVT_INTRA_DC && (int)IM_SMOOTH == SVT_INTRA_SMOOTH && (int)IM_SMOOTH_V == SVT_INTRA_SMOOTH_V && (int)IM_SMOOTH_H == SVT_INTRA_SMOOTH_H &&
              (int)IM_PAETH == SVT_INTRA_PAETH && (int)IM_DC_128 == SVT_INTRA_DC_128, "IM_* == SVT_INTRA_*");

extern "C" int svt_hip_intra_pred_batch(void* d_dst, int32_t dst_stride, size_t dst_block_pitch,
                                        const uint32_t* d_dst_offsets, const void* d_above, const void* d_left,
                                        int32_t nb_pitch, int mode, int bw, int bh, int upsample_above,
                                        int upsample_left, int dx, int dy, int is_16bit, int bd, size_t nblocks,
                                        void* stream) {
    return intra_pred_impl(d_dst, dst_stride, dst_block_pitch, d_dst_offsets, d_above, d_left, nb_pitch, mode, bw, bh,
                           upsample_above, upsample_left, dx, dy, is_16bit, bd, nblocks, stream, nullptr);
}

extern "C" int svt_hip_filter_intra_edge_batch(void* d_edges, int32_t nb_pitch, int sz, int strength, int is_16bit,
                                               size_t nblocks, void* stream) {
    if (int rc = require_init()) return rc;
    if (nblocks == 0 || strength == 0) return SVT_HIP_OK;
    EdgePlan p;
    if (int rc = filter_edge_plan(p, d_edges, nb_pitch, sz, strength, nblocks)) return rc;
    by_sample(is_16bit, [&](auto t) {
        hipLaunchKernelGGL((filter_edge_kernel<decltype(t)>), dim3(p.grid), dim3(p.threads), 0, (hipStream_t)stream, (decltype(t)*)d_edges, nb_pitch, NB_ORIGIN, sz, strength, p.nblocks);
    });
    return launch_status("filter_intra_edge");
}
extern "C" int svt_hip_upsample_intra_edge_batch(void* d_edges, int32_t nb_pitch, int sz, int is_16bit, int bd,
                                                 size_t nblocks, void* stream) {
    if (int rc = require_init()) return rc;
    if (nblocks == 0) return SVT_HIP_OK;
    EdgePlan p;
    if (int rc = upsample_edge_plan(p, d_edges, nb_pitch, sz, is_16bit, bd, nblocks)) return rc;
    by_sample(is_16bit, [&](auto t) {
        hipLaunchKernelGGL((upsample_edge_kernel<decltype(t)>), dim3(p.grid), dim3(p.threads), 0, (hipStream_t)stream, (decltype(t)*)d_edges, nb_pitch, NB_ORIGIN, sz, p.bd, p.nblocks);
    });
    return launch_status("upsample_intra_edge");
}

// ---- build_intra_predictors{,_high} for a batch (EbIntraPrediction.c:3667-4076), see kernel_bip.h ----
namespace svtdev {
// ---- ordering pass: block indices grouped by kind inside TILES of BIP_ORDER_TILE consecutive blocks (a counting sort over the
// IM_MODES = 13 bins in LDS; the order inside a bin is whatever the atomics give - the prediction of a block does not depend on its
// place in the order).  One kernel, no global counters: the first version sorted the whole batch (count kernel + scatter kernel, 17 +
// 20 us per 2^20 blocks, each a single residency round of 256 workgroups waiting on 13 contended global atomics); a wave only needs
// ITS four blocks to share a kind, and a tile of 4 096 blocks holds ~ 315 of each, so the waves of a tile are uniform except at its
// (at most 12) kind boundaries - 1.2 % of the waves; a mixed wave runs every kind it holds, several times a uniform wave's cost
// (tiles of 1 024 blocks measured no faster than the global sort for that reason).  1 024 threads per workgroup: 256 workgroups of
// 16 waves keep enough loads in flight.  (The tile constants: intra_plan.h.)
__global__ __launch_bounds__(BIP_ORDER_THREADS) void bip_order_tile_kernel(const BipBlk* __restrict__ blks, int w, int h, uint32_t* __restrict__ order, uint32_t nblocks) {
    __shared__ uint32_t s_cnt[16], s_base[16];
    if (threadIdx.x < 16) s_cnt[threadIdx.x] = 0;
    __syncthreads();
    const uint32_t base = blockIdx.x * (uint32_t)BIP_ORDER_TILE;
    BipBlk d[BIP_ORDER_ITEMS];
#pragma unroll
    for (int k = 0; k < BIP_ORDER_ITEMS; k++) {                 // the tile's descriptors, coalesced, all loads in flight together
        const uint32_t i = base + k * (uint32_t)BIP_ORDER_THREADS + threadIdx.x;
        d[k] = blks[i < nblocks ? i : 0u];
    }
    uint32_t kind[BIP_ORDER_ITEMS], local[BIP_ORDER_ITEMS];
#pragma unroll
    for (int k = 0; k < BIP_ORDER_ITEMS; k++) {
        const uint32_t i = base + k * (uint32_t)BIP_ORDER_THREADS + threadIdx.x;
        int pa;
        kind[k] = (uint32_t)bip_kind_of(d[k], w, h, pa);
        local[k] = i < nblocks ? atomicAdd(&s_cnt[kind[k]], 1u) : 0u;
    }
    __syncthreads();
    if (threadIdx.x < 16) {
        uint32_t start = 0;                                     // bin start = the counts of the bins before it
        for (int k = 0; k < (int)threadIdx.x; k++) start += s_cnt[k];
        s_base[threadIdx.x] = start;
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < BIP_ORDER_ITEMS; k++) {
        const uint32_t i = base + k * (uint32_t)BIP_ORDER_THREADS + threadIdx.x;
        if (i < nblocks) order[base + s_base[kind[k]] + local[k]] = i;
    }
}
}  // namespace svtdev

static_assert(sizeof(svt_hip_intra_blk) == sizeof(BipBlk), "svt_hip_intra_blk layout");
template <int W, int H>
static int bip_launch(void* d_dst, int32_t dst_stride, size_t dst_block_pitch, const uint32_t* d_dst_offsets, const void* d_top_neigh,
                      const void* d_left_neigh, int32_t neigh_pitch, const svt_hip_intra_blk* d_blocks, const uint32_t* d_order, int is_16bit,
                      int bd, const BipPlan& p, hipStream_t s) {
    by_sample(is_16bit, [&](auto t) {
        using T = decltype(t);
        hipLaunchKernelGGL((bip_kernel<T, W, H>), dim3(p.grid), dim3(p.threads), 0, s, (T*)d_dst, dst_stride, dst_block_pitch, d_dst_offsets,
                           (const T*)d_top_neigh, (const T*)d_left_neigh, neigh_pitch, (const BipBlk*)d_blocks, d_order, bd, p.nblocks);
    });
    return launch_status("build_intra_predictors");
}
static int bip_impl(void* d_dst, int32_t dst_stride, size_t dst_block_pitch, const uint32_t* d_dst_offsets, const void* d_top_neigh,
                    const void* d_left_neigh, int32_t neigh_pitch, const svt_hip_intra_blk* d_blocks, const uint32_t* d_order, int tx_size,
                    int is_16bit, int bd, size_t nblocks, void* stream) {
    if (int rc = require_init()) return rc;
    if (nblocks == 0) return SVT_HIP_OK;
    BipPlan p;
    if (int rc = bip_plan(p, d_dst, dst_stride, dst_block_pitch, d_dst_offsets, d_top_neigh, d_left_neigh, neigh_pitch, d_blocks, tx_size, is_16bit, bd, nblocks)) return rc;
#define BIP_LAUNCH(W, H) bip_launch<W, H>(d_dst, dst_stride, dst_block_pitch, d_dst_offsets, d_top_neigh, d_left_neigh, neigh_pitch, d_blocks, d_order, is_16bit, bd, \
                                          p, (hipStream_t)stream)
    TX_SWITCH(tx_size, BIP_LAUNCH)
#undef BIP_LAUNCH
}
extern "C" int svt_hip_build_intra_predictors_batch(void* d_dst, int32_t dst_stride, size_t dst_block_pitch,
                                                    const uint32_t* d_dst_offsets, const void* d_top_neigh,
                                                    const void* d_left_neigh, int32_t neigh_pitch,
                                                    const svt_hip_intra_blk* d_blocks, int tx_size, int is_16bit, int bd,
                                                    size_t nblocks, void* stream) {
    return bip_impl(d_dst, dst_stride, dst_block_pitch, d_dst_offsets, d_top_neigh, d_left_neigh, neigh_pitch, d_blocks, nullptr, tx_size, is_16bit, bd,
                    nblocks, stream);
}
extern "C" int svt_hip_build_intra_predictors_ordered_batch(void* d_dst, int32_t dst_stride, size_t dst_block_pitch,
                                                            const uint32_t* d_dst_offsets, const void* d_top_neigh,
                                                            const void* d_left_neigh, int32_t neigh_pitch,
                                                            const svt_hip_intra_blk* d_blocks, const uint32_t* d_order, int tx_size,
                                                            int is_16bit, int bd, size_t nblocks, void* stream) {
    if (nblocks && !d_order) { if (int rc = require_init()) return rc; return set_err(SVT_HIP_ERR_INVALID, "NULL order"); }
    return bip_impl(d_dst, dst_stride, dst_block_pitch, d_dst_offsets, d_top_neigh, d_left_neigh, neigh_pitch, d_blocks, d_order, tx_size, is_16bit, bd,
                    nblocks, stream);
}
extern "C" int svt_hip_intra_order_blocks_batch(const svt_hip_intra_blk* d_blocks, int tx_size, size_t nblocks, uint32_t* d_order,
                                                uint32_t* d_work, void* stream) {
    if (int rc = require_init()) return rc;
    if (nblocks == 0) return SVT_HIP_OK;
    (void)d_work;                                             // (the first version's global counters; unused)
    BipOrderPlan p;
    if (int rc = bip_order_plan(p, d_blocks, d_order, tx_size, nblocks)) return rc;
    hipLaunchKernelGGL(bip_order_tile_kernel, dim3(p.grid), dim3(p.threads), 0, (hipStream_t)stream, (const BipBlk*)d_blocks, p.w, p.h, d_order, p.nblocks);
    return launch_status("intra_order_blocks");
}

// ---- open-loop intra search: check, plan (ois_plan.h), enqueue ----
static_assert(sizeof(DirMulti::dx) == kDirMaxAngles * sizeof(int16_t) && sizeof(DirMultiLite::dx) == sizeof(DirMulti::dx) && OIS_NB_ORIGIN == NB_ORIGIN, "ois_plan.h");
extern "C" size_t svt_hip_ois_work_bytes(uint32_t bsize, int ncand, size_t nblocks) { return ois_work_layout(bsize, ncand, nblocks).total; }

struct OisPic { const uint8_t* pic; uint32_t stride, width, height; hipStream_t s; };
struct OisJob {            // one group, checked: its plan, its arrays, its work buffer carved (ois_work_layout)
    OisPlan plan;
    const uint32_t* xy; uint32_t* dist; int8_t* best; uint8_t *above, *left, *dc, *pred; size_t cand_pitch, nblocks;
};

static int ois_job(OisJob& J, const OisPic& P, const svt_hip_ois_group& G) {
    if (!P.pic || !G.d_xy || !G.d_distortion || !G.d_best_index || !G.d_work || !G.modes || !G.angle_deltas) return set_err(SVT_HIP_ERR_INVALID, "NULL buffer");
    if (int rc = ois_plan(J.plan, G.bsize, G.modes, G.angle_deltas, G.ncand, {g_tune_ois_no_fold != 0, g_tune_ois_no_nd != 0, g_tune_ois_no_dir3 != 0}))
        return set_err(rc, "%s", J.plan.err);
    if (P.width == 0 || P.height == 0 || P.width > 0xffffu || P.height > 0xffffu || P.stride < P.width)
        return set_err(SVT_HIP_ERR_INVALID, "picture %ux%u stride %u", P.width, P.height, P.stride);
    const OisWorkLayout L = ois_work_layout(G.bsize, G.ncand, G.nblocks);
    if (G.work_bytes < L.total) return set_err(SVT_HIP_ERR_INVALID, "work buffer: %zu B, need %zu", G.work_bytes, L.total);
    if (G.nblocks > 0x7fffffffu / 256) return set_err(SVT_HIP_ERR_INVALID, "too many blocks for one launch");
    uint8_t* w = (uint8_t*)G.d_work;
    J.xy = G.d_xy; J.dist = G.d_distortion; J.best = G.d_best_index; J.nblocks = G.nblocks;
    J.above = w + L.above; J.left = w + L.left; J.dc = w + L.dc; J.pred = w + L.pred; J.cand_pitch = L.cand_pitch;
    return SVT_HIP_OK;
}

static int ois_gather_enqueue(const OisPic& P, const OisJob& J) {
    hipLaunchKernelGGL(ois_gather_kernel, dim3(ois_wgs(J.nblocks, ois_gather_slots(J.plan.bsize))), dim3(256), 0, P.s, P.pic, P.stride, P.width, P.height,
                       J.xy, J.plan.bsize, J.above, J.left, (uint32_t)ois_nb_pitch(J.plan.bsize), J.dc, (uint32_t)J.nblocks);
    return launch_status("ois_gather");
}

// the angles of a directional launch (S null: none); dense: each prediction to its candidate's batch in J.pred (summed as well when the
// plan folds), else sums only
template <typename Z>
static void ois_dir_multi(Z& z, const OisPic& P, const OisJob& J, const OisDirSeg* S, bool dense) {
    z.n = 0; z.batch_pitch = dense ? J.cand_pitch : 0;
    z.sad_pic = P.pic; z.sad_stride = P.stride; z.sad_xy = J.xy; z.sad_dist = dense && !J.plan.fold ? nullptr : J.dist; z.sad_ncand = (uint32_t)J.plan.ncand;
    if (!S) return;
    z.n = S->n; memcpy(z.dx, S->dx, sizeof(S->dx)); memcpy(z.dy, S->dy, sizeof(S->dy)); memcpy(z.slot, S->slot, sizeof(S->slot));
}
static int ois_seg_enqueue(const OisPic& P, const OisJob& J, const OisDirSeg& S, bool dense) {
    const int b = (int)J.plan.bsize;
    DirMulti z;
    ois_dir_multi(z, P, J, &S, dense);
    return intra_pred_impl(dense ? (void*)J.pred : (void*)J.dist /* unused in SAD mode */, b, (size_t)b * b, nullptr, J.above, J.left, (int32_t)ois_nb_pitch(b),
                           SVT_INTRA_Z1 + S.zone, b, b, 0, 0, 1, 1, 0, 8, J.nblocks, P.s, &z);
}

// the directional candidates of the three zones in ONE launch (ois_dir3_kernel): 8x8 / 16x16 SAD mode
static int ois_dir3_enqueue(const OisPic& P, const OisJob& J) {
    const uint32_t bsize = J.plan.bsize;
    const OisDirSeg* of[3] = {};                                 // at most one segment per zone (OisPlan::dir3)
    for (int i = 0; i < J.plan.nseg; i++) of[J.plan.seg[i].zone] = &J.plan.seg[i];
    DirOis3 m;
    memset(&m, 0, sizeof(m));
    ois_dir_multi(m.z1, P, J, of[0], false); ois_dir_multi(m.z2, P, J, of[1], false); ois_dir_multi(m.z3, P, J, of[2], false);
    dir_z2_tables(m.z2);
    const int n[3] = {m.z1.n, m.z2.n, m.z3.n};
    OisDir3Plan p;                                               // the grid, the LDS and each zone's angle chunk (intra_plan.h)
    ois_dir3_plan(p, bsize, J.nblocks, n, intra_knobs());
    m.z1.chunk = p.chunk[0]; m.z2.chunk = p.chunk[1]; m.z3.chunk = p.chunk[2];
    m.y_end[0] = p.y_end[0]; m.y_end[1] = p.y_end[1];
    hipLaunchKernelGGL(bsize == 8 ? ois_dir3_kernel<8> : ois_dir3_kernel<16>, dim3(p.grid_x, p.grid_y), dim3(256), p.lds.bytes, P.s, J.above, J.left,
                       (int32_t)ois_nb_pitch(bsize), (int)bsize, p.lds.lim_a, p.lds.n_pad, p.nblocks, m);
    return launch_status("ois_dir3");
}

// OIS_PATH_FUSED after the gather: the directional candidates sum their SADs into dist, the three zones in one launch or segment by segment
// (no clearing of the neighbour arrays: the directional kernels stage positions [-2, 2 * bsize) only, all written by the gather)
static int ois_chain_enqueue(const OisPic& P, const OisJob& J) {
    if (J.plan.dir3) return ois_dir3_enqueue(P, J);
    for (int i = 0; i < J.plan.nseg; i++)
        if (int rc = ois_seg_enqueue(P, J, J.plan.seg[i], false)) return rc;
    return SVT_HIP_OK;
}

// OIS_PATH_GENERAL: every candidate's prediction into its own dense batch, then ONE SAD launch over (block, candidate).  The directional
// candidates of a segment share one launch (DirMulti): 9 prediction launches for the reference's 45-candidate list instead of 44.  With plan.fold
// (8x8 / 16x16: a block's lanes share a wave) they are compared with the source block there: no scratch round trip for 38 of the 45 candidates.
static int ois_general_enqueue(const OisPic& P, const OisJob& J) {
    const OisPlan& plan = J.plan;
    const int b = (int)plan.bsize;
    if (hipMemsetAsync(J.above, 0, (size_t)(J.dc - J.above), P.s) != hipSuccess) return set_err(SVT_HIP_ERR_RUNTIME, "hipMemsetAsync");
    if (int rc = ois_gather_enqueue(P, J)) return rc;
    int si = 0;
    for (int c = 0; c <= plan.ncand; c++) {                // (c = ncand: the segments still open at the end of the list)
        for (; si < plan.nseg && plan.seg[si].before == c; si++)
            if (int rc = ois_seg_enqueue(P, J, plan.seg[si], true)) return rc;
        const int mode = c < plan.ncand ? ois_dense_mode(plan.kinds.k[c]) : -1;
        if (mode < 0) continue;
        if (int rc = svt_hip_intra_pred_batch(J.pred + (size_t)c * J.cand_pitch, b, (size_t)b * b, nullptr, J.above, J.left, (int32_t)ois_nb_pitch(b), mode,
                                              b, b, 0, 0, 1, 1, 0, 8, J.nblocks, P.s))
            return rc;
    }
    const OisLanes g = ois_lanes(plan.bsize, plan.ncand);
    hipLaunchKernelGGL(ois_sad_kernel, dim3(ois_wgs(J.nblocks, g.slots)), dim3(256), g.shmem, P.s, P.pic, P.stride, J.xy,
                       plan.bsize, J.pred, J.cand_pitch, J.dc, (unsigned long long)plan.const_mask, (unsigned long long)plan.fold_mask, J.dist, J.best,
                       (uint32_t)plan.ncand, (uint32_t)J.nblocks);
    return launch_status("ois_sad");
}

// A whole group on its own.  The last launch of the fused paths: everything but the directional candidates - DC, V, H, SMOOTH*, PAETH -
// predicted and summed straight from the picture, the folded sums picked up, each block's best index taken; no prediction goes to memory
static int ois_enqueue(const OisPic& P, const OisJob& J) {
    if (J.plan.path == OIS_PATH_GENERAL) return ois_general_enqueue(P, J);
    if (J.plan.path == OIS_PATH_FUSED) {
        if (int rc = ois_gather_enqueue(P, J)) return rc;
        if (int rc = ois_chain_enqueue(P, J)) return rc;
    }
    const OisLanes g = ois_lanes(J.plan.bsize, J.plan.ncand, 4);
    hipLaunchKernelGGL(g.cs == 8 ? ois_nd_kernel<8> : ois_nd_kernel<16>, dim3(ois_wgs(J.nblocks, g.slots)), dim3(256), g.shmem, P.s, P.pic, P.stride, P.width, P.height,
                       J.xy, J.plan.bsize, J.plan.kinds, J.dist, J.best, (uint32_t)J.plan.ncand, (uint32_t)J.nblocks);
    return launch_status("ois_nd");
}

extern "C" int svt_hip_ois_search_batch(const uint8_t* d_pic, uint32_t stride, uint32_t width, uint32_t height,
                                        const uint32_t* d_xy, uint32_t bsize, const uint8_t* modes, const int8_t* angle_deltas,
                                        int ncand, uint32_t* d_distortion, int8_t* d_best_index, void* d_work,
                                        size_t work_bytes, size_t nblocks, void* stream) {
    if (int rc = require_init()) return rc;
    if (nblocks == 0) return SVT_HIP_OK;
    const OisPic P = {d_pic, stride, width, height, (hipStream_t)stream};
    const svt_hip_ois_group G = {d_xy, bsize, modes, angle_deltas, ncand, d_distortion, d_best_index, d_work, work_bytes, nblocks};
    OisJob J;
    if (int rc = ois_job(J, P, G)) return rc;
    return ois_enqueue(P, J);
}

extern "C" int svt_hip_ois_search_frame(const uint8_t* d_pic, uint32_t stride, uint32_t width, uint32_t height,
                                        const svt_hip_ois_group* groups, int ngroups, void* stream) {
    if (int rc = require_init()) return rc;
    if (ngroups == 0) return SVT_HIP_OK;
    if (!groups || ngroups < 0 || ngroups > 64) return set_err(SVT_HIP_ERR_INVALID, "group list");
    // every group is checked and planned before anything is enqueued
    const OisPic P = {d_pic, stride, width, height, (hipStream_t)stream};
    OisJob jobs[64];
    int njobs = 0;
    for (int g = 0; g < ngroups; g++) {
        if (groups[g].nblocks == 0) continue;
        if (int rc = ois_job(jobs[njobs++], P, groups[g])) return rc;
    }
    // Every group's chain (neighbour gather, the directional launches) goes out on the caller's stream, one after the other - each fills
    // the GPU - and the non-directional launch of EVERY group, which also takes each block's best index, follows as ONE launch
    // (ois_nd_multi_kernel; a side stream for the single-launch groups did not hide them behind the chains).
    // svt_hip_tune("ois_no_nd_multi", 1): every group as svt_hip_ois_search_batch runs it.
    if (g_tune_ois_no_nd_multi) {
        for (int j = 0; j < njobs; j++)
            if (int rc = ois_enqueue(P, jobs[j])) return rc;
        return SVT_HIP_OK;
    }
    // the neighbour gathers of the groups that have directional candidates: one launch, first
    GroupTable<OisGatherMulti, OIS_GATHER_MAX_GROUPS> gather;
    auto gather_launch = [&](const OisGatherMulti& gm, uint32_t total) -> int {
        hipLaunchKernelGGL(ois_gather_multi_kernel, dim3(total), dim3(256), 0, P.s, d_pic, stride, width, height, gm);
        return launch_status("ois_gather_multi");
    };
    for (int j = 0; j < njobs; j++) {
        const OisJob& J = jobs[j];
        if (J.plan.path != OIS_PATH_FUSED) continue;
        OisGatherGroup* D = gather.add(ois_wgs(J.nblocks, ois_gather_slots(J.plan.bsize)), gather_launch);
        if (!D) return gather.rc;
        D->xy = J.xy; D->above = J.above; D->left = J.left; D->dc = J.dc; D->bsize = J.plan.bsize;
        D->nb_pitch = (uint32_t)ois_nb_pitch(J.plan.bsize); D->nblocks = (uint32_t)J.nblocks;
    }
    if (int rc = gather.flush(gather_launch)) return rc;
    // largest blocks first: their workgroups are the longest latency chains (64x64: one block per workgroup, two barriers)
    GroupTable<OisNdMulti, OIS_ND_MAX_GROUPS, true> nd;
    size_t shmem = 0;                           // of the launch: the largest of its groups
    auto nd_launch = [&](const OisNdMulti& m, uint32_t total) -> int {
        hipLaunchKernelGGL(ois_nd_multi_kernel, dim3(total), dim3(256), shmem, P.s, d_pic, stride, width, height, m);
        shmem = 0;
        return launch_status("ois_nd_multi");
    };
    for (int j = 0; j < njobs; j++) {
        const OisJob& J = jobs[j];
        if (J.plan.path == OIS_PATH_GENERAL) { if (int rc = ois_general_enqueue(P, J)) return rc; continue; }
        if (J.plan.path == OIS_PATH_FUSED) if (int rc = ois_chain_enqueue(P, J)) return rc;
        const OisLanes g = ois_lanes(J.plan.bsize, J.plan.ncand, 4);
        OisNdGroup* D = nd.add(ois_wgs(J.nblocks, g.slots), nd_launch, J.plan.bsize);
        if (!D) return nd.rc;
        D->xy = J.xy; D->dist = J.dist; D->best_index = J.best; D->bsize = J.plan.bsize; D->ncand = (uint32_t)J.plan.ncand;
        D->nblocks = (uint32_t)J.nblocks; D->kinds = J.plan.kinds;
        shmem = g.shmem > shmem ? g.shmem : shmem;
    }
    return nd.flush(nd_launch);
}

// ===========================================================================
// (A) drop-in entry points: host pointers, one block, synchronous
// one intra block: stage [lo, hi) of above / left around the origin, predict, copy the block back
static void dropin_intra(int mode, int bw, int bh, void* dst, ptrdiff_t stride, const void* above, const void* left,
                         int a_lo, int a_hi, int l_lo, int l_hi, int ua, int ul, int dx, int dy, int is16, int bd,
                         const char* fn) {
    const size_t es = is16 ? 2 : 1;
    const int pitch = NB_ORIGIN + 2 * (bw + bh) + 16;
    const size_t nb_b = align256((size_t)pitch * es), px_b = (size_t)bw * bh * es;
    DROPIN_TRY(t_ctx.ensure(2 * nb_b + px_b), fn);
    char* d_a = t_ctx.dbuf;
    char* d_l = t_ctx.dbuf + nb_b;
    char* d_px = t_ctx.dbuf + 2 * nb_b;
    HIP_DIE(hipMemsetAsync(d_a, 0, 2 * nb_b, t_ctx.stream), fn);
    if (a_hi > a_lo)
        HIP_DIE(hipMemcpyAsync(d_a + (size_t)(NB_ORIGIN + a_lo) * es, (const char*)above + (ptrdiff_t)a_lo * (ptrdiff_t)es,
                               (size_t)(a_hi - a_lo) * es, hipMemcpyHostToDevice, t_ctx.stream), fn);
    if (l_hi > l_lo)
        HIP_DIE(hipMemcpyAsync(d_l + (size_t)(NB_ORIGIN + l_lo) * es, (const char*)left + (ptrdiff_t)l_lo * (ptrdiff_t)es,
                               (size_t)(l_hi - l_lo) * es, hipMemcpyHostToDevice, t_ctx.stream), fn);
    DROPIN_TRY(svt_hip_intra_pred_batch(d_px, bw, (size_t)bw * bh, nullptr, d_a, d_l, pitch, mode, bw, bh, ua, ul, dx, dy,
                                        is16, bd, 1, t_ctx.stream), fn);
    HIP_DIE(hipMemcpy2DAsync(dst, (size_t)stride * es, d_px, (size_t)bw * es, (size_t)bw * es, bh, hipMemcpyDeviceToHost, t_ctx.stream), fn);
    HIP_DIE(hipStreamSynchronize(t_ctx.stream), fn);
}
extern "C" void svt_hip_intra_predictor(int mode, int bw, int bh, uint8_t* dst, ptrdiff_t stride, const uint8_t* above,
                                        const uint8_t* left) {
    dropin_intra(mode, bw, bh, dst, stride, above, left, -1, bw, 0, bh, 0, 0, 1, 1, 0, 8, "svt_hip_intra_predictor");
}
extern "C" void svt_hip_highbd_intra_predictor(int mode, int bw, int bh, uint16_t* dst, ptrdiff_t stride,
                                               const uint16_t* above, const uint16_t* left, int32_t bd) {
    dropin_intra(mode, bw, bh, dst, stride, above, left, -1, bw, 0, bh, 0, 0, 1, 1, 1, bd, "svt_hip_highbd_intra_predictor");
}
#define DR_RANGES_Z1 0, (((bw + bh - 1) << upsample_above) + 2), 0, 0
#define DR_RANGES_Z3 0, 0, 0, (((bw + bh - 1) << upsample_left) + 2)
#define DR_RANGES_Z2 -(1 << upsample_above), (((bw - 1) << upsample_above) + 2), -(1 << upsample_left), (((bh - 1) << upsample_left) + 2)
extern "C" void svt_hip_av1_dr_prediction_z1(uint8_t* dst, ptrdiff_t stride, int32_t bw, int32_t bh, const uint8_t* above,
                                             const uint8_t* left, int32_t upsample_above, int32_t dx, int32_t dy) {
    dropin_intra(SVT_INTRA_Z1, bw, bh, dst, stride, above, left, DR_RANGES_Z1, upsample_above, 0, dx, dy, 0, 8, "svt_hip_av1_dr_prediction_z1");
}
extern "C" void svt_hip_av1_dr_prediction_z2(uint8_t* dst, ptrdiff_t stride, int32_t bw, int32_t bh, const uint8_t* above,
                                             const uint8_t* left, int32_t upsample_above, int32_t upsample_left,
                                             int32_t dx, int32_t dy) {
    dropin_intra(SVT_INTRA_Z2, bw, bh, dst, stride, above, left, DR_RANGES_Z2, upsample_above, upsample_left, dx, dy, 0, 8, "svt_hip_av1_dr_prediction_z2");
}
extern "C" void svt_hip_av1_dr_prediction_z3(uint8_t* dst, ptrdiff_t stride, int32_t bw, int32_t bh, const uint8_t* above,
                                             const uint8_t* left, int32_t upsample_left, int32_t dx, int32_t dy) {
    dropin_intra(SVT_INTRA_Z3, bw, bh, dst, stride, above, left, DR_RANGES_Z3, 0, upsample_left, dx, dy, 0, 8, "svt_hip_av1_dr_prediction_z3");
}
extern "C" void svt_hip_av1_highbd_dr_prediction_z1(uint16_t* dst, ptrdiff_t stride, int32_t bw, int32_t bh,
                                                    const uint16_t* above, const uint16_t* left, int32_t upsample_above,
                                                    int32_t dx, int32_t dy, int32_t bd) {
    dropin_intra(SVT_INTRA_Z1, bw, bh, dst, stride, above, left, DR_RANGES_Z1, upsample_above, 0, dx, dy, 1, bd, "svt_hip_av1_highbd_dr_prediction_z1");
}
extern "C" void svt_hip_av1_highbd_dr_prediction_z2(uint16_t* dst, ptrdiff_t stride, int32_t bw, int32_t bh,
                                                    const uint16_t* above, const uint16_t* left, int32_t upsample_above,
                                                    int32_t upsample_left, int32_t dx, int32_t dy, int32_t bd) {
    dropin_intra(SVT_INTRA_Z2, bw, bh, dst, stride, above, left, DR_RANGES_Z2, upsample_above, upsample_left, dx, dy, 1, bd, "svt_hip_av1_highbd_dr_prediction_z2");
}
extern "C" void svt_hip_av1_highbd_dr_prediction_z3(uint16_t* dst, ptrdiff_t stride, int32_t bw, int32_t bh,
                                                    const uint16_t* above, const uint16_t* left, int32_t upsample_left,
                                                    int32_t dx, int32_t dy, int32_t bd) {
    dropin_intra(SVT_INTRA_Z3, bw, bh, dst, stride, above, left, DR_RANGES_Z3, 0, upsample_left, dx, dy, 1, bd, "svt_hip_av1_highbd_dr_prediction_z3");
}


// ---- per-size RTCD slot entry points (intra_pred_fn / intra_high_pred_fn, EbIntraPrediction.h:36-41): what
// init_intra_predictors_internal stores in pred[][] / dc_pred[][][] (EbIntraPrediction.c:2842-3350) ----
#define DEF_PRED(mode, MODE, W, H)                                                                                          \
    extern "C" void svt_hip_aom_##mode##_predictor_##W##x##H(uint8_t* dst, ptrdiff_t stride, const uint8_t* above,        \
                                                             const uint8_t* left) {                                       \
        dropin_intra(MODE, W, H, dst, stride, above, left, -1, W, 0, H, 0, 0, 1, 1, 0, 8, "svt_hip_aom_" #mode "_predictor_" #W "x" #H); \
    }                                                                                                                     \
    extern "C" void svt_hip_aom_highbd_##mode##_predictor_##W##x##H(uint16_t* dst, ptrdiff_t stride, const uint16_t* above, \
                                                                    const uint16_t* left, int bd) {                       \
        dropin_intra(MODE, W, H, dst, stride, above, left, -1, W, 0, H, 0, 0, 1, 1, 1, bd, "svt_hip_aom_highbd_" #mode "_predictor_" #W "x" #H); \
    }
SVT_HIP_INTRA_MODES(SVT_HIP_BLOCK_SIZES_2, DEF_PRED)
#undef DEF_PRED
extern "C" void svt_hip_eb_smooth_v_predictor(uint8_t* dst, ptrdiff_t stride, int32_t bw, int32_t bh, const uint8_t* above,
                                              const uint8_t* left) {
    dropin_intra(SVT_INTRA_SMOOTH_V, bw, bh, dst, stride, above, left, -1, bw, 0, bh, 0, 0, 1, 1, 0, 8, "svt_hip_eb_smooth_v_predictor");
}
extern "C" void svt_hip_eb_smooth_h_predictor(uint8_t* dst, ptrdiff_t stride, int32_t bw, int32_t bh, const uint8_t* above,
                                              const uint8_t* left) {
    dropin_intra(SVT_INTRA_SMOOTH_H, bw, bh, dst, stride, above, left, -1, bw, 0, bh, 0, 0, 1, 1, 0, 8, "svt_hip_eb_smooth_h_predictor");
}

// ---- av1_filter_intra_edge{,_high}, av1_upsample_intra_edge{,_high} (aom_dsp_rtcd.h:152-156, 431-437) ----
static void dropin_edge(int upsample, void* p, int sz, int strength_or_bd, int is16, const char* fn) {
    const size_t es = is16 ? 2 : 1;
    const int pitch = NB_ORIGIN + 2 * sz + 16;
    DROPIN_TRY(t_ctx.ensure((size_t)pitch * es), fn);
    char* d = t_ctx.dbuf;
    // filter: p[0 .. sz-1] in and out; upsample: p[-1 .. sz-1] in, p[-2 .. 2*sz-2] out (EbIntraPrediction.c:3597-3660)
    const int in_lo = upsample ? -1 : 0, in_n = upsample ? sz + 1 : sz, out_lo = upsample ? -2 : 0, out_n = upsample ? 2 * sz + 1 : sz;
    HIP_DIE(hipMemcpyAsync(d + (size_t)(NB_ORIGIN + in_lo) * es, (const char*)p + (ptrdiff_t)in_lo * (ptrdiff_t)es, (size_t)in_n * es,
                           hipMemcpyHostToDevice, t_ctx.stream), fn);
    if (upsample) DROPIN_TRY(svt_hip_upsample_intra_edge_batch(d, pitch, sz, is16, strength_or_bd, 1, t_ctx.stream), fn);
    else DROPIN_TRY(svt_hip_filter_intra_edge_batch(d, pitch, sz, strength_or_bd, is16, 1, t_ctx.stream), fn);
    HIP_DIE(hipMemcpyAsync((char*)p + (ptrdiff_t)out_lo * (ptrdiff_t)es, d + (size_t)(NB_ORIGIN + out_lo) * es, (size_t)out_n * es,
                           hipMemcpyDeviceToHost, t_ctx.stream), fn);
    HIP_DIE(hipStreamSynchronize(t_ctx.stream), fn);
}
extern "C" void svt_hip_av1_filter_intra_edge(uint8_t* p, int32_t sz, int32_t strength) {
    if (strength) dropin_edge(0, p, sz, strength, 0, "svt_hip_av1_filter_intra_edge");
}
extern "C" void svt_hip_av1_filter_intra_edge_high(uint16_t* p, int32_t sz, int32_t strength) {
    if (strength) dropin_edge(0, p, sz, strength, 1, "svt_hip_av1_filter_intra_edge_high");
}
extern "C" void svt_hip_av1_upsample_intra_edge(uint8_t* p, int32_t sz) { dropin_edge(1, p, sz, 8, 0, "svt_hip_av1_upsample_intra_edge"); }
extern "C" void svt_hip_av1_upsample_intra_edge_high(uint16_t* p, int32_t sz, int32_t bd) {
    dropin_edge(1, p, sz, bd, 1, "svt_hip_av1_upsample_intra_edge_high");
}

// ---- subtract_average, cfl_predict_lbd / _hbd, av1_txb_init_levels (aom_dsp_rtcd.h:140-148, 2376) ----
extern "C" void svt_hip_subtract_average(int16_t* pred_buf_q3, int32_t width, int32_t height, int32_t round_offset,
                                         int32_t num_pel_log2) {
    const char* fn = "svt_hip_subtract_average";
    const size_t bytes = (size_t)32 * height * 2;                     // CFL_BUF_LINE = 32 int16 per row
    DROPIN_TRY(t_ctx.ensure(bytes), fn);
    HIP_DIE(hipMemcpyAsync(t_ctx.dbuf, pred_buf_q3, bytes, hipMemcpyHostToDevice, t_ctx.stream), fn);
    DROPIN_TRY(svt_hip_subtract_average_batch((int16_t*)t_ctx.dbuf, 32, (size_t)32 * height, (uint32_t)width, (uint32_t)height, round_offset, num_pel_log2, 1,
                                              t_ctx.stream), fn);
    HIP_DIE(hipMemcpyAsync(pred_buf_q3, t_ctx.dbuf, bytes, hipMemcpyDeviceToHost, t_ctx.stream), fn);
    HIP_DIE(hipStreamSynchronize(t_ctx.stream), fn);
}
static void dropin_cfl_predict(const int16_t* q3, const void* pred, int32_t pred_stride, void* dst, int32_t dst_stride,
                               int32_t alpha_q3, int32_t bit_depth, int32_t width, int32_t height, int is16, const char* fn) {
    const size_t es = is16 ? 2 : 1;
    const size_t qb = align256((size_t)32 * height * 2), pb = align256((size_t)width * height * es);
    DROPIN_TRY(t_ctx.ensure(qb + 2 * pb + 256), fn);
    char* d_q = t_ctx.dbuf;
    char* d_p = d_q + qb;
    char* d_d = d_p + pb;
    int32_t* d_alpha = (int32_t*)(d_d + pb);
    HIP_DIE(hipMemcpyAsync(d_q, q3, (size_t)32 * height * 2, hipMemcpyHostToDevice, t_ctx.stream), fn);
    HIP_DIE(hipMemcpy2DAsync(d_p, (size_t)width * es, pred, (size_t)pred_stride * es, (size_t)width * es, height, hipMemcpyHostToDevice, t_ctx.stream), fn);
    HIP_DIE(hipMemcpyAsync(d_alpha, &alpha_q3, 4, hipMemcpyHostToDevice, t_ctx.stream), fn);
    DROPIN_TRY(svt_hip_cfl_predict_batch((const int16_t*)d_q, 32, (size_t)32 * height, d_p, (uint32_t)width, d_d, (uint32_t)width, nullptr, d_alpha, bit_depth,
                                         (uint32_t)width, (uint32_t)height, is16, 1, t_ctx.stream), fn);
    HIP_DIE(hipMemcpy2DAsync(dst, (size_t)dst_stride * es, d_d, (size_t)width * es, (size_t)width * es, height, hipMemcpyDeviceToHost, t_ctx.stream), fn);
    HIP_DIE(hipStreamSynchronize(t_ctx.stream), fn);
}
extern "C" void svt_hip_cfl_predict_lbd(const int16_t* pred_buf_q3, uint8_t* pred, int32_t pred_stride, uint8_t* dst,
                                        int32_t dst_stride, int32_t alpha_q3, int32_t bit_depth, int32_t width, int32_t height) {
    dropin_cfl_predict(pred_buf_q3, pred, pred_stride, dst, dst_stride, alpha_q3, bit_depth, width, height, 0, "svt_hip_cfl_predict_lbd");
}
extern "C" void svt_hip_cfl_predict_hbd(const int16_t* pred_buf_q3, uint16_t* pred, int32_t pred_stride, uint16_t* dst,
                                        int32_t dst_stride, int32_t alpha_q3, int32_t bit_depth, int32_t width, int32_t height) {
    dropin_cfl_predict(pred_buf_q3, pred, pred_stride, dst, dst_stride, alpha_q3, bit_depth, width, height, 1, "svt_hip_cfl_predict_hbd");
}
extern "C" void svt_hip_av1_txb_init_levels(const svt_tran_low_t* const coeff, const int32_t width, const int32_t height,
                                            uint8_t* const levels) {
    const char* fn = "svt_hip_av1_txb_init_levels";
    // `levels` points TX_PAD_TOP rows into the padded buffer (EbRateDistortionCost.c:125-150): whole buffer = (w+4)*(h+6)+16
    const int stride = width + 4;
    const size_t cb = align256((size_t)width * height * 4), lb = (size_t)stride * (height + 6) + 16;
    const size_t lpitch = (lb + 3) & ~(size_t)3;
    DROPIN_TRY(t_ctx.ensure(cb + lpitch), fn);
    HIP_DIE(hipMemcpyAsync(t_ctx.dbuf, coeff, (size_t)width * height * 4, hipMemcpyHostToDevice, t_ctx.stream), fn);
    DROPIN_TRY(svt_hip_txb_init_levels_batch((const int32_t*)t_ctx.dbuf, (size_t)width * height, (uint8_t*)t_ctx.dbuf + cb, lpitch, (uint32_t)width, (uint32_t)height, 1,
                                             t_ctx.stream), fn);
    HIP_DIE(hipMemcpyAsync(levels - 2 * stride, t_ctx.dbuf + cb, lb, hipMemcpyDeviceToHost, t_ctx.stream), fn);
    HIP_DIE(hipStreamSynchronize(t_ctx.stream), fn);
}

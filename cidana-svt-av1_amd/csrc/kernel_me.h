// kernel_me.h — the motion-search stage kernels (svt_hip_pixel.hip launches them): K6 full-pel search in its forms
// (me_sb_search16_kernel, me_nsq4_kernel, me_fullpel_exact_kernel, me_fullpel_areas_kernel), MotionEstimateLcu's glue
// (me_setup_kernel, me_bipred_kernel) and the HME levels (hme_level_kernel).  Each is a wrapper that finds its block's rows and
// calls the steps of kernel_me_steps.h, where the algorithms, the reference's line numbers and the LDS layouts are described.
#pragma once
#include "kernel_me_steps.h"

namespace svtdev {

template <bool MASKED>
__global__ __launch_bounds__(ME_THREADS) __attribute__((amdgpu_waves_per_eu(2, 2))) void me_sb_search16_kernel(
    const uint8_t* __restrict__ src, uint32_t src_stride, size_t src_block_pitch,
    const uint8_t* __restrict__ ref, uint32_t ref_stride, size_t ref_block_pitch, int search_w, int search_h,
    const int16_t* __restrict__ origins /* [n][2] x,y or NULL */, int x_origin, int y_origin,
    uint32_t* __restrict__ best_sad, uint32_t* __restrict__ best_mv, uint32_t wpitch,
    const uint32_t* __restrict__ src_offs, const uint32_t* __restrict__ ref_offs, uint32_t nblocks,
    int w8q = 0, int ref_layout = 0, uint32_t pu_pitch = ME_PUS) {
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
    const uint32_t blk = blockIdx.x;
    if (blk >= nblocks) return;
    const uint8_t* gs = src + (src_offs ? (size_t)src_offs[blk] : (size_t)blk * src_block_pitch);
    const uint8_t* gr = ref + (ref_offs ? (size_t)ref_offs[blk] : (size_t)blk * ref_block_pitch);
    const int ox = origins ? origins[2 * blk] : x_origin, oy = origins ? origins[2 * blk + 1] : y_origin;
    me_sb_search16_body<MASKED>(smem, gs, src_stride, gr, ref_stride, search_w, search_h, ox, oy, best_sad + (size_t)blk * pu_pitch,
                                best_mv + (size_t)blk * pu_pitch, wpitch, w8q, ref_layout);
}

__global__ __launch_bounds__(ME_THREADS) __attribute__((amdgpu_waves_per_eu(2, 2))) void me_nsq4_kernel(
    const uint8_t* __restrict__ src, uint32_t src_stride, size_t src_block_pitch,
    const uint8_t* __restrict__ ref, uint32_t ref_stride, size_t ref_block_pitch, int search_w, int search_h,
    const int16_t* __restrict__ origins /* [n][2] x,y or NULL */, int x_origin, int y_origin,
    uint32_t* __restrict__ best_sad, uint32_t* __restrict__ best_mv, uint32_t wpitch,
    const uint32_t* __restrict__ src_offs, const uint32_t* __restrict__ ref_offs, uint32_t nblocks, uint32_t pu_pitch) {
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
    const uint32_t blk = blockIdx.x;
    if (blk >= nblocks) return;
    const uint8_t* gs = src + (src_offs ? (size_t)src_offs[blk] : (size_t)blk * src_block_pitch);
    const uint8_t* gr = ref + (ref_offs ? (size_t)ref_offs[blk] : (size_t)blk * ref_block_pitch);
    const int ox = origins ? origins[2 * blk] : x_origin, oy = origins ? origins[2 * blk + 1] : y_origin;
    me_nsq4_body(smem, gs, src_stride, gr, ref_stride, search_w, search_h, ox, oy, best_sad + (size_t)blk * pu_pitch,
                 best_mv + (size_t)blk * pu_pitch, wpitch, nullptr);
}

__global__ __launch_bounds__(ME_THREADS) void me_fullpel_exact_kernel(
    const uint8_t* __restrict__ src, uint32_t src_stride, size_t src_block_pitch, const uint32_t* __restrict__ src_offs,
    const uint8_t* __restrict__ ref, uint32_t ref_stride, size_t ref_block_pitch, const uint32_t* __restrict__ ref_offs,
    int search_w, int search_h, const int16_t* __restrict__ origins, int x_origin, int y_origin, int flavour, int nsq,
    uint32_t* __restrict__ best_sad, uint32_t* __restrict__ best_mv, uint32_t pu_pitch, uint32_t nblocks) {
    __shared__ __attribute__((aligned(16))) uint32_t s_src[32 * 16];      // even source rows
    __shared__ uint32_t s_s8[8][64];                                       // [point of the step][8x8 block, raster]
    const uint32_t blk = blockIdx.x;
    if (blk >= nblocks) return;
    const uint8_t* gs = src + (src_offs ? (size_t)src_offs[blk] : (size_t)blk * src_block_pitch);
    const uint8_t* gr = ref + (ref_offs ? (size_t)ref_offs[blk] : (size_t)blk * ref_block_pitch);
    const int ox = origins ? origins[2 * blk] : x_origin, oy = origins ? origins[2 * blk + 1] : y_origin;
    me_exact_body(s_src, s_s8, gs, src_stride, gr, ref_stride, search_w, search_h, ox, oy, flavour, nsq, best_sad + (size_t)blk * pu_pitch,
                  best_mv + (size_t)blk * pu_pitch);
}

template <bool NSQ>
__global__ __launch_bounds__(ME_THREADS) __attribute__((amdgpu_waves_per_eu(2, 2))) void me_fullpel_areas_kernel(
    const uint8_t* __restrict__ src, uint32_t src_stride, const uint32_t* __restrict__ src_offs, const uint8_t* __restrict__ ref,
    uint32_t ref_stride, const uint32_t* __restrict__ ref_offs, const int16_t* __restrict__ areas /* [n][4] */, int max_w, int max_h,
    int flavour, uint32_t* __restrict__ best_sad, uint32_t* __restrict__ best_mv, uint32_t pu_pitch, uint32_t wpitch, uint32_t pair_off,
    uint32_t nblocks) {
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
    const uint32_t blk = blockIdx.x;
    if (blk >= nblocks) return;
    me_fullpel_area_body<NSQ>(smem, src + (size_t)src_offs[blk], src_stride, ref + (size_t)ref_offs[blk], ref_stride, areas + 4 * (size_t)blk, max_w,
                              max_h, flavour, best_sad + (size_t)blk * pu_pitch, best_mv + (size_t)blk * pu_pitch, wpitch, pair_off);
}

__global__ __launch_bounds__(256) void me_setup_kernel(
    const uint8_t* __restrict__ src_pic, uint32_t src_stride, const uint8_t* __restrict__ ref_pic, uint32_t ref_stride,
    const int16_t* __restrict__ sb_origin /* [n][2] */, const uint16_t* __restrict__ sb_size /* [n][2] */,
    const unsigned long long* __restrict__ hme_sad /* [regions][n] or NULL */, const int16_t* __restrict__ hme_mv /* [regions][n][2] */,
    const MeSetupParams p, int16_t* __restrict__ center /* [n][2] or NULL */, int16_t* __restrict__ area /* [n][4] */, uint32_t ntasks) {
    const uint32_t task = blockIdx.x * 4 + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (task >= ntasks) return;                             // wave-uniform; nothing below synchronises across waves
    const int ox = sb_origin[2 * task], oy = sb_origin[2 * task + 1];
    const int sbw = sb_size[2 * task], sbh = sb_size[2 * task + 1];
    const int nreg = p.regions_w * p.regions_h;
    int xc = 0, yc = 0;
    if (hme_sad && nreg > 0 && sbh == 64) {
        // region r = rh * regions_w + rw: r = 0, 1, 2, 3 is the reference's visiting order [w][h] = [0][0], [1][0], [0][1], [1][1]
        unsigned long long s[4];
        int cx[4], cy[4];
#pragma unroll
        for (int r = 0; r < 4; r++) {
            const bool on = r < nreg;
            s[r] = on ? hme_sad[(size_t)r * ntasks + task] : ~0ull;
            cx[r] = on ? hme_mv[((size_t)r * ntasks + task) * 2] : 0;
            cy[r] = on ? hme_mv[((size_t)r * ntasks + task) * 2 + 1] : 0;
        }
        me_pick_centre(s, cx, cy, nreg, p.regions_w, p.second_best, xc, yc);
    }
    int a4[4];
    me_zz_check_and_area(src_pic, src_stride, ref_pic, ref_stride, ox, oy, sbw, sbh, p, lane, xc, yc, a4);
    if (lane == 0) {
        if (center) { center[2 * task] = (int16_t)xc; center[2 * task + 1] = (int16_t)yc; }
        area[4 * task] = (int16_t)a4[0]; area[4 * task + 1] = (int16_t)a4[1]; area[4 * task + 2] = (int16_t)a4[2]; area[4 * task + 3] = (int16_t)a4[3];
    }
}

__global__ __launch_bounds__(ME_THREADS) void me_bipred_kernel(
    const uint8_t* __restrict__ src_pic, uint32_t src_stride, const uint8_t* __restrict__ ref0_pic, uint32_t ref0_stride,
    const uint8_t* __restrict__ ref1_pic, uint32_t ref1_stride, const int16_t* __restrict__ sb_origin,
    const uint32_t* __restrict__ best_sad0, const uint32_t* __restrict__ best_mv0, const uint32_t* __restrict__ best_sad1,
    const uint32_t* __restrict__ best_mv1, uint32_t pu_pitch, int npus, int bipred_all_pus, int sub_sad, const MePuMap map,
    uint32_t* __restrict__ bipred_sad /* [n][pu_pitch] storage order, or NULL */, MeResult* __restrict__ results /* [n][npus] raster order */,
    uint32_t nsb) {
    const uint32_t sb = blockIdx.x;
    if (sb >= nsb) return;
    const size_t row = (size_t)sb * pu_pitch;
    // every entry of the SB's bipred_sad row is defined after the call: 0 for PUs without a bi-prediction SAD and past the PU count
    // (the body's own stores come after its barriers, as in me_frame_bipred_kernel)
    if (bipred_sad)
        for (uint32_t i = threadIdx.x; i < pu_pitch; i += ME_THREADS) bipred_sad[row + i] = 0u;
    me_bipred_body(src_pic, src_stride, ref0_pic, ref0_stride, ref1_pic, ref1_stride, sb_origin[2 * sb], sb_origin[2 * sb + 1], best_sad0 + row,
                   best_mv0 + row, best_sad1 ? best_sad1 + row : nullptr, best_mv1 ? best_mv1 + row : nullptr, npus, bipred_all_pus, sub_sad, map,
                   bipred_sad ? bipred_sad + row : nullptr, results + (size_t)sb * npus);
}

__global__ __launch_bounds__(ME_THREADS) void hme_level_kernel(
    const uint8_t* __restrict__ src_pic, uint32_t src_stride, const uint8_t* __restrict__ ref_pic, uint32_t ref_stride,
    const int16_t* __restrict__ sb_origin /* [n][2] */, const uint16_t* __restrict__ sb_size /* [n][2] */,
    const int16_t* __restrict__ centers /* [regions][n][2] or NULL */, int center_shift, const HmeParamSets ps,
    unsigned long long* __restrict__ best_sad /* [regions][n] */, int16_t* __restrict__ mv /* [regions][n][2] */, uint32_t wpitch, uint32_t ntasks) {
    const HmeParams& p = ps.p[blockIdx.y];
    if (centers) centers += (size_t)blockIdx.y * ntasks * 2;
    best_sad += (size_t)blockIdx.y * ntasks;
    mv += (size_t)blockIdx.y * ntasks * 2;
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
    uint32_t* s_src = reinterpret_cast<uint32_t*>(smem);            // [32 rows][16 dwords]: the block's even rows, zero-padded
    uint8_t* s_ref = smem + svthost::ME_SRC_LDS;
    __shared__ unsigned long long s_red[4];
    const uint32_t task = blockIdx.x;
    if (task >= ntasks) return;
    const int tid = threadIdx.x;
    const int ox = sb_origin[2 * task], oy = sb_origin[2 * task + 1];
    const int sbw = sb_size[2 * task], sbh = sb_size[2 * task + 1];
    // The size table lives in device memory, the host cannot check it; s_src holds 32 rows of 64 bytes and the window is sized for
    // blocks of at most 64x64 (include/svt_hip_dsp.h).  An entry outside 1..64 x 2..64 is answered, not searched.
    if (sbw < 1 || sbh < 2 || sbw > 64 || sbh > 64) {
        if (tid == 0) { best_sad[task] = ~0ull; mv[2 * task] = 0; mv[2 * task + 1] = 0; }
        return;
    }
    const int xc = centers ? (centers[2 * task] >> center_shift) : 0, yc = centers ? (centers[2 * task + 1] >> center_shift) : 0;
    const HmeArea a = hme_place_area(p, ox, oy, xc, yc);
    const int xo = a.xo, yo = a.yo, saw = a.saw, sah = a.sah;
    const int hh = sbh >> 1;                                          // rows compared
    const int win_w = sbw + saw - 1, win_h = sah + 2 * hh - 2;
    const uint8_t* gs = src_pic + (ptrdiff_t)oy * (ptrdiff_t)src_stride + ox;
    const uint8_t* gr = ref_pic + (ptrdiff_t)(oy + yo) * (ptrdiff_t)ref_stride + (ox + xo);
    hme_stage_block(s_src, gs, src_stride, sbw, hh);
    hme_stage_window(s_ref, gr, ref_stride, win_w, win_h, wpitch);
    __syncthreads();
    const unsigned long long best = hme_search_wave(s_src, s_ref, wpitch, sbw, hh, saw, sah);
    if ((tid & 63) == 0) s_red[tid >> 6] = best;
    __syncthreads();
    if (tid == 0) {
        const unsigned long long b = hme_min4(s_red);
        const int cand = (int)(unsigned)b;
        const int ys = cand / saw, xs = cand - ys * saw;
        best_sad[task] = (b >> 32) * 2ull;
        mv[2 * task] = (int16_t)((xs + xo) << p.mv_shift);
        mv[2 * task + 1] = (int16_t)((ys + yo) << p.mv_shift);
    }
}

}  // namespace svtdev

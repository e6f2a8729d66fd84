// kernel_me_frame.h — MotionEstimateLcu (EbMotionEstimation.c:7527) for every SB of a picture, or of a stack of pictures that
// share one parameter set, in three launches (svt_hip_motion_estimate_frame, svt_hip_me_frame.hip):
//   me_frame_prologue_kernel  one workgroup per (SB, reference list, picture): the enabled HME levels 0 / 1 / 2 over all search
//                             regions, the best region (with the same-POC second-best rule of list 1), CheckZeroZeroCenter and
//                             the search area's round-up / clip / round-down - the chain that the stage calls spread over
//                             svt_hip_hme_level_regions_batch x 3 and svt_hip_me_setup_batch per list, each handing a few bytes
//                             per SB to the next through HBM.  Here a level's per-region centres and SADs stay in LDS, only the
//                             final area reaches memory.  It also initialises the SB's result rows (MAX_SAD_VALUE / 0).
//   me_frame_search_kernel    the full-pel search over each SB's own area, both lists and all pictures in one launch
//                             (me_fullpel_area_body, the body of me_fullpel_areas_kernel)
//   me_frame_bipred_kernel    BiPredictionSearch and the me_results rows (me_bipred_body, the body of me_bipred_kernel)
// The search steps are those of hme_level_kernel / me_setup_kernel (kernel_me.h), which live in kernel_me_steps.h as device functions: the numbers
// are the stage calls' numbers by construction.  SB origins and plane offsets come from the block index; no tables.
#pragma once
#include "kernel_me_steps.h"

namespace svtdev {

struct MeFrameDev {
    const uint8_t* src[3];              // sample (0, 0) of the source's full / quarter / sixteenth luma picture
    const uint8_t* ref[2][3];           // the same of list 0 / list 1
    uint32_t src_stride[3], ref_stride[2][3];
    unsigned long long src_pitch[3], ref_pitch[2][3];      // bytes between the pictures of a stack
    HmeParams hme[3][4];                // [HME level][region r = rh * regions_w + rw]
    MeSetupParams setup;                // regions_w / _h as configured; second_best is taken from second_best[list]
    int32_t level_on[3];                // HME level 0 / 1 / 2 runs (enable_hme_flag folded in)
    int32_t hme_list[2];                // this list takes an HME centre at all (BASE_LAYER_REF rule, :7656)
    int32_t second_best[2];
    int32_t nreg, last_level;           // regions_w * regions_h; the last enabled level (-1: none)
    int32_t nlists, npus;
    uint32_t nsbx, nsb;                 // SBs per row / per picture
    uint32_t hme_wpitch;                // LDS pitch of the HME window rows
    int16_t* area;                      // [picture][SB][list][4]
    int16_t* area_origin;               // [picture][SB][list][2]
    uint32_t* best_sad;                 // [picture][SB][list][ME_PUS_ALL]
    uint32_t* best_mv;
};

constexpr unsigned ME_MAX_SAD_VALUE = 128 * 128 * 255;          // EbMotionEstimation.h:79

__global__ __launch_bounds__(ME_THREADS) void me_frame_prologue_kernel(const MeFrameDev d) {
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
    uint32_t* s_src = reinterpret_cast<uint32_t*>(smem);            // [32 rows][16 dwords]: the level's SB block, even rows
    uint8_t* s_ref = smem + svthost::ME_SRC_LDS;                              // the region's clipped window
    __shared__ unsigned long long s_red[4];
    __shared__ unsigned long long s_sad[4];                         // the level's result per region: what the stage calls keep in HBM
    __shared__ int s_cx[4], s_cy[4];
    const uint32_t sb = blockIdx.x, list = blockIdx.y, pic = blockIdx.z;
    const int tid = threadIdx.x;
    const int ox = (int)(sb % d.nsbx) * 64, oy = (int)(sb / d.nsbx) * 64;
    const int sbw = min(64, d.setup.picture_width - ox), sbh = min(64, d.setup.picture_height - oy);
    const size_t row = ((size_t)pic * d.nsb + sb) * d.nlists + list;
    // the result rows start from MAX_SAD_VALUE as the reference's do (InitializeBuffer_32bits, :8131); entries past the PU
    // count are never touched by the reference's zero-allocated context
    for (int i = tid; i < ME_PUS_ALL; i += ME_THREADS) {
        d.best_sad[row * ME_PUS_ALL + i] = i < d.npus ? ME_MAX_SAD_VALUE : 0u;
        d.best_mv[row * ME_PUS_ALL + i] = 0u;
    }
    if (tid < 4) { s_sad[tid] = ~0ull; s_cx[tid] = 0; s_cy[tid] = 0; }
    // "no HME in boundaries" (:7681): SBs that are not 64 rows high keep the (0, 0) centre
    const bool hme = d.hme_list[list] && d.last_level >= 0 && sbh == 64;
    if (hme) {
#pragma unroll 1
        for (int lv = 0; lv <= d.last_level; lv++) {
            __syncthreads();                                          // the level before is done with s_src, s_sad, s_cx / s_cy
            if (!d.level_on[lv]) {                                    // a switched-off level hands the initial centre (0, 0) to the next
                if (tid < 4) { s_cx[tid] = 0; s_cy[tid] = 0; }
                continue;
            }
            const int sh = 2 - lv, k = 2 - lv;                        // level 0 works on the sixteenth picture
            const int lox = ox >> sh, loy = oy >> sh, lw = sbw >> sh, lh = sbh >> sh, hh = lh >> 1;
            const uint8_t* src_pic = d.src[k] + (size_t)pic * d.src_pitch[k];
            const uint8_t* ref_pic = d.ref[list][k] + (size_t)pic * d.ref_pitch[list][k];
            // lw >= 2: the host admits picture sides that are multiples of 8 only, so the narrowest partial SB is 8 wide
            hme_stage_block(s_src, src_pic + (ptrdiff_t)loy * (ptrdiff_t)d.src_stride[k] + lox, d.src_stride[k], lw, hh);
#pragma unroll 1
            for (int r = 0; r < d.nreg; r++) {
                const HmeParams& p = d.hme[lv][r];
                // level 1 starts from the level-0 vector >> 1, level 2 from the level-1 vector (the reference's call sites)
                const int xc = s_cx[r] >> (lv == 1 ? 1 : 0), yc = s_cy[r] >> (lv == 1 ? 1 : 0);
                const HmeArea a = hme_place_area(p, lox, loy, xc, yc);
                __syncthreads();                                      // the region before is done with s_ref and s_red
                hme_stage_window(s_ref, ref_pic + (ptrdiff_t)(loy + a.yo) * (ptrdiff_t)d.ref_stride[list][k] + (lox + a.xo), d.ref_stride[list][k],
                                 lw + a.saw - 1, a.sah + 2 * hh - 2, d.hme_wpitch);
                __syncthreads();
                const unsigned long long wk = hme_search_wave(s_src, s_ref, d.hme_wpitch, lw, hh, a.saw, a.sah);
                if ((tid & 63) == 0) s_red[tid >> 6] = wk;
                __syncthreads();
                if (tid == 0) {
                    const unsigned long long b = hme_min4(s_red);
                    const int cand = (int)(unsigned)b;
                    const int ys = cand / a.saw, xs = cand - ys * a.saw;
                    s_sad[r] = (b >> 32) * 2ull;
                    s_cx[r] = (int16_t)((xs + a.xo) << p.mv_shift);
                    s_cy[r] = (int16_t)((ys + a.yo) << p.mv_shift);
                }
            }
        }
    }
    __syncthreads();
    if (tid >= 64) return;                                            // the set-up is one wave's work (me_setup_kernel: a wave per task)
    unsigned long long s[4];
    int cx[4], cy[4];
#pragma unroll
    for (int r = 0; r < 4; r++) { s[r] = s_sad[r]; cx[r] = s_cx[r]; cy[r] = s_cy[r]; }
    int xc = 0, yc = 0;
    if (hme) me_pick_centre(s, cx, cy, d.nreg, d.setup.regions_w, d.second_best[list], xc, yc);
    int area[4];
    me_zz_check_and_area(d.src[0] + (size_t)pic * d.src_pitch[0], d.src_stride[0], d.ref[list][0] + (size_t)pic * d.ref_pitch[list][0],
                         d.ref_stride[list][0], ox, oy, sbw, sbh, d.setup, tid, xc, yc, area);
    if (tid == 0) {
#pragma unroll
        for (int i = 0; i < 4; i++) d.area[4 * row + i] = (int16_t)area[i];
        d.area_origin[2 * row] = (int16_t)area[0];
        d.area_origin[2 * row + 1] = (int16_t)area[1];
    }
}

// the search proper: me_fullpel_areas_kernel's body, its block = (SB, list, picture) instead of a row of two offset tables
template <bool NSQ>
__global__ __launch_bounds__(ME_THREADS) __attribute__((amdgpu_waves_per_eu(2, 2))) void me_frame_search_kernel(
    const MeFrameDev d, int max_w, int max_h, int flavour, uint32_t wpitch, uint32_t pair_off) {
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
    const uint32_t sb = blockIdx.x, list = blockIdx.y, pic = blockIdx.z;
    const int ox = (int)(sb % d.nsbx) * 64, oy = (int)(sb / d.nsbx) * 64;
    const size_t row = ((size_t)pic * d.nsb + sb) * d.nlists + list;
    const uint8_t* gs = d.src[0] + (size_t)pic * d.src_pitch[0] + (ptrdiff_t)oy * (ptrdiff_t)d.src_stride[0] + ox;
    const uint8_t* gr = d.ref[list][0] + (size_t)pic * d.ref_pitch[list][0] + (ptrdiff_t)oy * (ptrdiff_t)d.ref_stride[list][0] + ox;
    me_fullpel_area_body<NSQ>(smem, gs, d.src_stride[0], gr, d.ref_stride[list][0], d.area + 4 * row, max_w, max_h, flavour,
                              d.best_sad + row * ME_PUS_ALL, d.best_mv + row * ME_PUS_ALL, wpitch, pair_off);
}

__global__ __launch_bounds__(ME_THREADS) void me_frame_bipred_kernel(const MeFrameDev d, int bipred_all_pus, int sub_sad, const MePuMap map,
                                                                     uint32_t* __restrict__ bipred_sad /* [picture][SB][ME_PUS_ALL] */,
                                                                     MeResult* __restrict__ results /* [picture][SB][ME_PUS_ALL] */) {
    const uint32_t sb = blockIdx.x, pic = blockIdx.z;
    const int tid = threadIdx.x;
    const int ox = (int)(sb % d.nsbx) * 64, oy = (int)(sb / d.nsbx) * 64;
    const size_t sbi = (size_t)pic * d.nsb + sb, row = sbi * d.nlists;
    const bool two = d.nlists == 2;
    // every entry of the two outputs is defined after the call: PUs without a bi-prediction SAD and rows past the PU count are zero
    for (int i = tid; i < ME_PUS_ALL; i += ME_THREADS) {
        bipred_sad[sbi * ME_PUS_ALL + i] = 0u;
        if (i >= d.npus) {
            MeResult z;
            __builtin_memset(&z, 0, sizeof(z));
            results[sbi * ME_PUS_ALL + i] = z;
        }
    }
    const uint32_t* bs0 = d.best_sad + row * ME_PUS_ALL;
    const uint32_t* bm0 = d.best_mv + row * ME_PUS_ALL;
    me_bipred_body(d.src[0] + (size_t)pic * d.src_pitch[0], d.src_stride[0], d.ref[0][0] + (size_t)pic * d.ref_pitch[0][0], d.ref_stride[0][0],
                   two ? d.ref[1][0] + (size_t)pic * d.ref_pitch[1][0] : nullptr, d.ref_stride[1][0], ox, oy, bs0, bm0, two ? bs0 + ME_PUS_ALL : nullptr,
                   two ? bm0 + ME_PUS_ALL : nullptr, d.npus, bipred_all_pus, sub_sad, map, bipred_sad + sbi * ME_PUS_ALL, results + sbi * ME_PUS_ALL);
}

}  // namespace svtdev

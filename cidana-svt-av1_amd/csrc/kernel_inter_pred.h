// kernel_inter_pred.h — AV1 translational inter prediction for many (plane, block size) groups in one launch: what av1_inter_prediction /
// av1_inter_prediction_hbd (EbInterPrediction.c:1024, :2093) write for a block, list 0, list 1 or their plain average, with the
// distortion against the source summed while the prediction is still in registers.
//
// One body for the sixteen convolve entries (convolve[sub x][sub y][compound], :843-873).  With round_0 = 3 and round_1 = 11 (single
// reference) or 7 (compound) from get_conv_params_no_round (convolve.h:115), every entry is the 2-D entry run with the full-pel kernel
// {0, 0, 0, 128, 0, 0, 0, 0} in the direction it does not filter, and the offsets the reference carries through its unsigned
// intermediate cancel.  With p the samples, fx / fy the two kernels (each sums to 128):
//     hr = (sum fx[k] * p[x - 3 + k] + 4) >> 3                   first pass, signed: im_block of :158 minus 1 << (bd + 3)
//     V  = sum fy[k] * hr[y - 3 + k]                             second pass: `sum` of :172 minus (1 << (bd + 11)) + (1 << (bd + 10))
//     single reference:  pred = clip((V + 1024) >> 11)
//     compound:          c = (V + 64) >> 7 per list (the CONV_BUF_TYPE value minus round_offset), pred = clip((((c0 + c1) >> 1) + 8) >> 4)
// x-only (V = 128 * hr), y-only (hr = 16 * p) and copy (V = 2048 * p) give :243, :210 and :262 exactly, and likewise the jnt_ entries;
// tests/golden/make_golden_inter_pred.py asserts it against the sixteen compiled entries.  A wave whose blocks are all full-pel skips
// the filter and the LDS and reads V = 2048 * p straight from the plane.
//
// Work split (inter_plan.h, InterGeom): a lane owns 4 samples of a row of a tile of at most 16 x 16; small blocks share a wave.  Per list
// a slot's lanes stage its (tw + 7) x (th + 7) window into LDS as uint16 (every load of a batch of 8 issued before the first LDS write),
// run the first pass over its th + 7 rows into int16 rows in LDS, and the second pass into registers.  List 0's result stays in four
// registers while list 1 goes through the same LDS: the compound intermediate never reaches memory.  The tap tables, the clamp, the
// lane geometry, a round's block, the window and the first pass are kernel_inter_steps.h's, shared with interp_sse_kernel.
#pragma once
#include "group_table.h"
#include "kernel_inter_steps.h"

namespace svtdev {

template <typename PIX>
__global__ __launch_bounds__(IP_THREADS) void inter_pred_kernel(const InterPredDesc fd) {
    __shared__ __attribute__((aligned(16))) uint16_t s_win[IP_WAVES][IP_LDS_WIN];
    __shared__ __attribute__((aligned(16))) int16_t s_hr[IP_WAVES][IP_LDS_HR];
    __shared__ uint32_t s_part[IP_WAVES];

    uint32_t bid;
    const int gi = group_of(fd, bid);
    if (gi >= fd.ngroups) return;
    const InterPredGroupDev& D = fd.g[gi];
    const InterGeom ge = inter_geom(D.lw, D.lh);
    const IpLane T = ip_lane(ge, D.ss, D.lw, D.lh);
    const int w = T.w, h = T.h, tw = T.tw, lane = T.lane, wave = T.wave, row = T.row, col4 = T.col4;
    uint16_t* const win = &s_win[wave][T.slot * T.PW * (T.th + 7)];
    int16_t* const hrb = &s_hr[wave][T.slot * tw * (T.th + 7)];
    const int maxv = (1 << fd.bd) - 1;
    const bool want_dist = D.dist != nullptr;

    uint32_t dist = 0;
    uint32_t blk_of_lane = 0;
    bool active = false;
#pragma unroll 1
    for (int r = 0; r < ge.rounds; r++) {
        const IpBlock B = ip_block(ge, T, r, bid, D.blk, D.nblocks, fd.pic_w, fd.pic_h);
        active = B.active;
        blk_of_lane = B.b;
        const int tabx = ip_table((B.w3 >> 8) & 0xff, w <= 4), taby = ip_table((B.w3 >> 16) & 0xff, h <= 4);      // filter_x, filter_y
        const int dir = B.dir, px = B.px, py = B.py, tx = B.tx, ty = B.ty;
        const bool frac = (B.use0 && ((B.qx0 | B.qy0) & 15)) || (B.use1 && ((B.qx1 | B.qy1) & 15));
        const bool filter_wave = __any(frac);

        // one list into V (named registers: the two calls below are the unrolled loop over the lists)
        auto one_list = [&](int (&Vl)[4], const bool use_l, const int qxl, const int qyl, const void* plane) {
            if (!__any(use_l)) return;
            // sample (0, 0) of this lane's tile in the list's plane
            const long long org = (long long)(py + ty + (qyl >> 4)) * (long long)D.ref_stride + (px + tx + (qxl >> 4));
            const PIX* const ref = reinterpret_cast<const PIX*>(plane) + (use_l ? org : 0);
            if (!filter_wave) {
                if (use_l) {
                    const PIX* p = ref + (long long)row * D.ref_stride + col4;
#pragma unroll
                    for (int j = 0; j < 4; j++) Vl[j] = (int)p[j] << 11;
                }
                return;
            }
            // ---- the window, then the first pass over it (kernel_inter_steps.h) ----
            ip_stage_window(T, win, ref - 3ll * D.ref_stride - 3, D.ref_stride, use_l);
            ip_first_pass(T, win, hrb, ip_load_taps(tabx, qxl & 15));
            wave_lds_fence();
            // ---- second pass: this lane's four samples ----
            {
                const IpTaps fy = ip_load_taps(taby, qyl & 15);
#pragma unroll
                for (int k = 0; k < 8; k++) {
                    const uint2 q = *reinterpret_cast<const uint2*>(&hrb[(row + k) * tw + col4]);
                    Vl[0] += fy.f[k] * (int)(int16_t)(q.x & 0xffff);
                    Vl[1] += fy.f[k] * ((int)q.x >> 16);
                    Vl[2] += fy.f[k] * (int)(int16_t)(q.y & 0xffff);
                    Vl[3] += fy.f[k] * ((int)q.y >> 16);
                }
            }
            wave_lds_fence();                       // list 1 stages over list 0's window
        };
        int V0[4] = {0, 0, 0, 0}, V1[4] = {0, 0, 0, 0};
        one_list(V0, B.use0, B.qx0, B.qy0, D.ref[0]);
        one_list(V1, B.use1, B.qx1, B.qy1, D.ref[1]);

        // ---- rounding (:175-178, :313-328), store, distortion ----
        int o[4];
#pragma unroll
        for (int j = 0; j < 4; j++) {
            int v;
            if (dir == 2) v = (((((V0[j] + 64) >> 7) + ((V1[j] + 64) >> 7)) >> 1) + 8) >> 4;
            else v = ((dir == 0 ? V0[j] : V1[j]) + 1024) >> 11;
            o[j] = min(max(v, 0), maxv);
        }
        if (active && D.pred) {
            PIX* dst = reinterpret_cast<PIX*>(D.pred);
            if (D.pred_stride == 0) dst += (size_t)B.b * (size_t)(w * h) + (size_t)((ty + row) * w + tx + col4);
            else dst += (size_t)(py + ty + row) * D.pred_stride + (size_t)(px + tx + col4);
            if constexpr (sizeof(PIX) == 1) {
                *reinterpret_cast<ip_u1*>(dst) = (uint32_t)o[0] | ((uint32_t)o[1] << 8) | ((uint32_t)o[2] << 16) | ((uint32_t)o[3] << 24);
            } else {
                ip_v2u pk;
                pk.x = (uint32_t)o[0] | ((uint32_t)o[1] << 16);
                pk.y = (uint32_t)o[2] | ((uint32_t)o[3] << 16);
                *reinterpret_cast<ip_v2u*>(dst) = pk;
            }
        }
        if (want_dist && active) {
            const PIX* sp = reinterpret_cast<const PIX*>(D.src) + (size_t)(py + ty + row) * D.src_stride + (size_t)(px + tx + col4);
#pragma unroll
            for (int j = 0; j < 4; j++) {
                const int d = o[j] - (int)sp[j];
                dist += fd.metric == SVT_HIP_FAST_SSD ? (uint32_t)(d * d) : (uint32_t)(d < 0 ? -d : d);
            }
        }
    }

    if (want_dist) {          // group-uniform: every wave of the workgroup takes the barrier
        // at most 1024 samples of a block per wave: the 32-bit sum holds 1024 * 1023^2
        const uint32_t wsum = group_sum_rt(dist, (uint32_t)ge.dist_lanes);
        if (ge.waves_per_block > 1) {
            if (lane == 0) s_part[wave] = wsum;
            __syncthreads();
            if (lane == 0 && (wave & (ge.waves_per_block - 1)) == 0 && active) {
                unsigned long long sum = 0;
                for (int k = 0; k < ge.waves_per_block; k++) sum += s_part[wave + k];
                D.dist[blk_of_lane] = sum;
            }
        } else if (active && (lane & (ge.dist_lanes - 1)) == 0) {
            D.dist[blk_of_lane] = wsum;
        }
    }
}

}  // namespace svtdev

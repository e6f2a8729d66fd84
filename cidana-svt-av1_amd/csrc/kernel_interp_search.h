// kernel_interp_search.h — the interpolation filter search of mode decision (interpolation_filter_search, EbInterPrediction.c:3578-3917).
//
// interp_sse_kernel: for a block record and a plane, the SSE against the source of the nine predictions inter_pred_kernel
// (kernel_inter_pred.h) would write with filter pair i = 3 * filter_y + filter_x, filter_sets[i] of :3573.  The tiling, the clamp, the
// addressing, the tap tables, the window and the first pass are the text that kernel runs (kernel_inter_steps.h), the second pass and
// the two rounding lines the arithmetic stated there (hr, V); what differs is how often each step runs.  Per list
// a slot's lanes stage the (tw + 7) x (th + 7) window into LDS ONCE, run the THREE horizontal passes into three sets of int16 rows, and
// each lane runs the NINE vertical passes over its four samples: the eight rows of a horizontal set are read once and feed the three
// vertical filters.  A full-pel direction takes phase 0, {0, 0, 0, 128, 0, 0, 0, 0} in every table, which is the copy exactly, so the wave
// always filters.  BI_PRED: list 0's nine compound intermediates (V + 64) >> 7 stay in registers as packed int16 pairs (|V| < 2^22)
// while list 1 goes through the same LDS.  The squared differences accumulate in nine registers per lane over the workgroup's rounds
// and are summed as inter_pred_kernel sums its distortion: in the wave over the lanes of a block, across waves through LDS.  No atomics,
// nothing zeroed by the caller; no prediction is written.
//
// interp_decide_kernel: the walk over that table, a thread a block, as svt_hip_dsp.h states it line by line.  model_rd_from_sse is
// fp_model_rd (model_rd.h, shared with fast_pick_kernel), included, not restated.
#pragma once
#include "group_table.h"
#include "interp_plan.h"
#include "kernel_inter_steps.h"
#include "model_rd.h"

namespace svtdev {

__global__ __launch_bounds__(IP_THREADS) void interp_sse_kernel(const InterpSseDesc fd) {
    __shared__ __attribute__((aligned(16))) uint16_t s_win[IP_WAVES][IP_LDS_WIN];
    __shared__ __attribute__((aligned(16))) int16_t s_hr[IP_WAVES][IS_LDS_HR];
    __shared__ uint32_t s_part[IP_WAVES][IS_NPAIR];

    uint32_t bid;
    const int gi = group_of(fd, bid);
    if (gi >= fd.ngroups) return;
    const InterpSseGroupDev& D = fd.g[gi];
    const InterGeom ge = inter_geom(D.lw, D.lh);
    const IpLane T = ip_lane(ge, D.ss, D.lw, D.lh);
    const int w = T.w, h = T.h, tw = T.tw, lane = T.lane, wave = T.wave, row = T.row, col4 = T.col4;
    uint16_t* const win = &s_win[wave][T.slot * T.PW * (T.th + 7)];
    int16_t* const hrb = &s_hr[wave][T.slot * tw * (T.th + 7)];   // filter f's rows: hrb + f * IP_LDS_HR

    uint32_t sse[IS_NPAIR];
#pragma unroll
    for (int i = 0; i < IS_NPAIR; i++) sse[i] = 0;
    uint32_t blk_of_lane = 0;
    bool active = false;
#pragma unroll 1
    for (int r = 0; r < ge.rounds; r++) {
        const IpBlock B = ip_block(ge, T, r, bid, D.blk, D.nblocks, fd.pic_w, fd.pic_h);
        active = B.active;
        blk_of_lane = B.b;
        const int dir = B.dir, px = B.px, py = B.py, tx = B.tx, ty = B.ty;

        // the lane's four source samples
        int sp[4] = {0, 0, 0, 0};
        if (active) {
            const uint32_t s4 = *reinterpret_cast<const ip_u1*>(D.src + (size_t)(py + ty + row) * D.src_stride + (size_t)(px + tx + col4));
            sp[0] = s4 & 0xff; sp[1] = (s4 >> 8) & 0xff; sp[2] = (s4 >> 16) & 0xff; sp[3] = s4 >> 24;
        }

        uint32_t keep[IS_NPAIR][2];                 // list 0's compound intermediates of a BI_PRED block, two int16 a word
#pragma unroll
        for (int i = 0; i < IS_NPAIR; i++) keep[i][0] = keep[i][1] = 0;

        // one list (the two calls below are the unrolled loop over the lists)
        auto one_list = [&](const int list, const bool use_l, const int qxl, const int qyl, const uint8_t* plane) {
            if (!__any(use_l)) return;
            const long long org = (long long)(py + ty + (qyl >> 4)) * (long long)D.ref_stride + (px + tx + (qxl >> 4));
            const uint8_t* const wbase = plane + (use_l ? org - 3ll * D.ref_stride - 3 : 0);
            // ---- the window once, then the three first passes over it, one per horizontal filter (kernel_inter_steps.h) ----
            ip_stage_window(T, win, wbase, D.ref_stride, use_l);
#pragma unroll 1
            for (int f = 0; f < 3; f++) ip_first_pass(T, win, hrb + f * IP_LDS_HR, ip_load_taps(ip_table(f, w <= 4), qxl & 15));
            wave_lds_fence();
            // ---- nine second passes: a horizontal set's eight rows feed the three vertical filters ----
            IpTaps fy[3];
#pragma unroll
            for (int g = 0; g < 3; g++) fy[g] = ip_load_taps(ip_table(g, h <= 4), qyl & 15);
#pragma unroll
            for (int f = 0; f < 3; f++) {
                const int16_t* const hf = hrb + f * IP_LDS_HR;
                int V[3][4] = {{0, 0, 0, 0}, {0, 0, 0, 0}, {0, 0, 0, 0}};
#pragma unroll
                for (int k = 0; k < 8; k++) {
                    const uint2 q = *reinterpret_cast<const uint2*>(&hf[(row + k) * tw + col4]);
                    const int hv[4] = {(int)(int16_t)(q.x & 0xffff), (int)q.x >> 16, (int)(int16_t)(q.y & 0xffff), (int)q.y >> 16};
#pragma unroll
                    for (int g = 0; g < 3; g++)
#pragma unroll
                        for (int j = 0; j < 4; j++) V[g][j] += fy[g].f[k] * hv[j];
                }
#pragma unroll
                for (int g = 0; g < 3; g++) {
                    const int i = 3 * g + f;                     // filter_sets[i] = {vertical g, horizontal f}
                    // rounding (:175-178, :313-328) as inter_pred_kernel
                    const int c0[4] = {(int)(int16_t)(keep[i][0] & 0xffff), (int)keep[i][0] >> 16, (int)(int16_t)(keep[i][1] & 0xffff), (int)keep[i][1] >> 16};
                    uint32_t acc = 0;
                    int cc[4];
#pragma unroll
                    for (int j = 0; j < 4; j++) {
                        cc[j] = (V[g][j] + 64) >> 7;
                        int v = dir == 2 ? (((c0[j] + cc[j]) >> 1) + 8) >> 4 : (V[g][j] + 1024) >> 11;
                        v = min(max(v, 0), 255);
                        const int d = v - sp[j];
                        acc += (uint32_t)(d * d);
                    }
                    if (list == 0) {
                        keep[i][0] = (uint32_t)(cc[0] & 0xffff) | ((uint32_t)cc[1] << 16);
                        keep[i][1] = (uint32_t)(cc[2] & 0xffff) | ((uint32_t)cc[3] << 16);
                    }
                    // the list that completes the block's prediction: its own for a single reference, list 1 for BI_PRED
                    if (use_l && (dir == 2 ? list == 1 : true)) sse[i] += acc;
                }
            }
            wave_lds_fence();                       // the next list, or the next round, stages over these rows
        };
        one_list(0, B.use0, B.qx0, B.qy0, D.ref[0]);
        one_list(1, B.use1, B.qx1, B.qy1, D.ref[1]);
    }

    // ---- the nine sums: at most 1024 samples of a block per wave, 1024 * 255^2 < 2^32; a 64 x 64 block: 4096 * 255^2 < 2^32 ----
    uint32_t wsum[IS_NPAIR];
#pragma unroll
    for (int i = 0; i < IS_NPAIR; i++) wsum[i] = group_sum_rt(sse[i], (uint32_t)ge.dist_lanes);
    if (ge.waves_per_block > 1) {                   // group-uniform: every wave of the workgroup takes the barrier
        if (lane == 0) {
#pragma unroll
            for (int i = 0; i < IS_NPAIR; i++) s_part[wave][i] = wsum[i];
        }
        __syncthreads();
        if (lane < IS_NPAIR && (wave & (ge.waves_per_block - 1)) == 0 && active) {
            uint32_t sum = 0;
            for (int k = 0; k < ge.waves_per_block; k++) sum += s_part[wave + k][lane];
            D.sse[(size_t)blk_of_lane * D.sse_stride + lane] = sum;
        }
    } else if (active && (lane & (ge.dist_lanes - 1)) == 0) {
        uint32_t* const out = D.sse + (size_t)blk_of_lane * D.sse_stride;
#pragma unroll
        for (int i = 0; i < IS_NPAIR; i++) out[i] = wsum[i];
    }
}

// model_rd_for_sb (:3440-3529) of one pair: the plane sums, then RDCOST (:3305) with the switchable rate
struct InterpRd { long long rd; long long skip_sse; int rs; int skip; };
__device__ __forceinline__ InterpRd interp_rd_of(const uint32_t* sse, int i, int planes, uint32_t nlog2_y, uint32_t qstep, uint32_t lambda, int rs) {
    unsigned long long rate_sum = 0, dist_sum = 0, total_sse = 0;
    for (int p = 0; p < planes; p++) {
        const uint32_t s = sse[p * IS_NPAIR + i];
        uint32_t rate;
        unsigned long long dist;
        fp_model_rd(s, p ? nlog2_y - 2 : nlog2_y, qstep, rate, dist);
        total_sse += s; rate_sum += rate; dist_sum += dist;
    }
    InterpRd R;
    R.rs = rs;
    R.skip = total_sse == 0;
    R.skip_sse = (long long)(total_sse << 4);
    const int tmp_rate = (int)rate_sum;
    R.rd = (long long)((((unsigned long long)(long long)(rs + tmp_rate) * lambda + 256ull) >> 9) + dist_sum * 128ull);
    return R;
}

__global__ __launch_bounds__(ID_THREADS) void interp_decide_kernel(const InterpDecideDesc fd) {
    uint32_t bid;
    const int gi = group_of(fd, bid);
    if (gi >= fd.ngroups) return;
    const InterpDecideGroupDev& D = fd.g[gi];
    const uint32_t b = bid * ID_THREADS + threadIdx.x;
    if (b >= D.nblocks) return;
    const int planes = fd.use_uv ? 3 : 1;
    const uint32_t* const sse = D.sse + (size_t)b * (size_t)(planes * IS_NPAIR);
    const int ctx0 = min((int)D.ctx[2 * (size_t)b], 15), ctx1 = min((int)D.ctx[2 * (size_t)b + 1], 15);
    const bool searchable = D.searchable[b] != 0;
    auto cost = [&](int i) {                        // av1_get_switchable_rate (:3184): dir 0 is the vertical filter
        const int rs = fd.rates[ctx0 * 3 + i / 3] + fd.rates[ctx1 * 3 + i % 3];
        return interp_rd_of(sse, i, planes, D.nlog2_y, fd.qstep, fd.lambda, rs);
    };
    InterpRd best = cost(0);                        // :3621-3661
    int best_i = 0;
    auto consider = [&](int i) {                    // :3737, :3811, :3886: strictly below, and everything follows the winner
        const InterpRd c = cost(i);
        if (c.rd < best.rd) { best = c; best_i = i; }
    };
    if (searchable) {
        if (fd.mode == SVT_HIP_INTERP_DUAL_FAST) {
            for (int i = 1; i < 3; i++) consider(i);                       // :3683
            const int best_dual_mode = best_i;
            for (int i = best_dual_mode + 3; i < IS_NPAIR; i += 3) consider(i);      // :3755
        } else {
            for (int i = 1; i < IS_NPAIR; i++) {                           // :3828
                if (fd.mode == SVT_HIP_INTERP_SINGLE && i / 3 != i % 3) continue;
                consider(i);
            }
        }
    }
    const uint32_t fy = (uint32_t)(best_i / 3), fx = (uint32_t)(best_i % 3);
    unsigned long long* const out = D.decision + 4 * (size_t)b;
    out[0] = (unsigned long long)(fy | fx << 16) | (unsigned long long)(uint32_t)best.rs << 32;
    out[1] = (unsigned long long)best.rd;
    out[2] = (unsigned long long)best.skip_sse;
    out[3] = (unsigned long long)(uint32_t)best.skip;
    if (D.blk_out) {
        ip_v4a4 raw = *reinterpret_cast<const ip_v4a4*>(D.blk + b);
        raw.w = (raw.w & 0xff0000ffu) | fx << 8 | fy << 16;
        *reinterpret_cast<ip_v4a4*>(D.blk_out + b) = raw;
    }
}

}  // namespace svtdev

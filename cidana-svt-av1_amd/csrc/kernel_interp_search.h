// kernel_interp_search.h — the interpolation filter search of mode decision (interpolation_filter_search, EbInterPrediction.c:3578-3917).
//
// interp_sse_kernel: for a block record and a plane, the SSE against the source of the nine predictions inter_pred_kernel
// (kernel_inter_pred.h) would write with filter pair i = 3 * filter_y + filter_x, filter_sets[i] of :3573.  Same tiling (InterGeom), same
// clamp, addressing, tap tables and arithmetic (hr, V and the two rounding lines stated there); what differs is what is shared.  Per list
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
#include "interp_plan.h"
#include "kernel_inter_pred.h"
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
    const int ss = D.ss, w = 1 << D.lw, h = 1 << D.lh, tw = 1 << ge.ltw, th = 1 << ge.lth;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int L = 1 << ge.llanes, slot = lane >> ge.llanes, li = lane & (L - 1);
    const int row = li >> (ge.ltw - 2), col4 = (li & ((tw >> 2) - 1)) << 2;
    const int PW = tw + 8, wd = tw + 7, ws = wd * (th + 7);
    const uint32_t recip = 65536u / (uint32_t)wd + 1;          // e / wd == (e * recip) >> 16 for e < ws <= 529
    uint16_t* const win = &s_win[wave][slot * PW * (th + 7)];
    int16_t* const hrb = &s_hr[wave][slot * tw * (th + 7)];   // filter f's rows: hrb + f * IP_LDS_HR

    uint32_t sse[IS_NPAIR];
#pragma unroll
    for (int i = 0; i < IS_NPAIR; i++) sse[i] = 0;
    uint32_t blk_of_lane = 0;
    bool active = false;
#pragma unroll 1
    for (int r = 0; r < ge.rounds; r++) {
        const uint32_t t = (uint32_t)(r * IP_WAVES + wave) * ge.slots + slot;           // tile of the workgroup
        const uint32_t b = bid * ge.blocks_per_wg + (ge.rounds > 1 ? 0 : t >> ge.ltpb);
        const int ti = t & ((1 << ge.ltpb) - 1);
        const int tx = (ti & ((w >> ge.ltw) - 1)) << ge.ltw, ty = (ti >> (D.lw - ge.ltw)) << ge.lth;
        active = b < D.nblocks;
        blk_of_lane = b;

        // ---- the block: clamp and addressing, as inter_pred_kernel ----
        ip_v4a4 raw = {0, 0, 0, 0};
        if (active) raw = *reinterpret_cast<const ip_v4a4*>(D.blk + b);
        int bx = raw.x & 0xffff, by = raw.x >> 16;
        bx = min(bx, (int)fd.pic_w - (w << ss));
        by = min(by, (int)fd.pic_h - (h << ss));
        const int dir = min((int)(raw.w & 0xff), 2);
        const int px = ss ? ((bx >> 3) << 3) >> 1 : bx, py = ss ? ((by >> 3) << 3) >> 1 : by;
        const bool use0 = active && dir != 1, use1 = active && dir != 0;
        const int qx0 = ip_clamp_mv((int16_t)(raw.y & 0xffff), bx, w << ss, w, fd.pic_w, ss);
        const int qy0 = ip_clamp_mv((int)raw.y >> 16, by, h << ss, h, fd.pic_h, ss);
        const int qx1 = ip_clamp_mv((int16_t)(raw.z & 0xffff), bx, w << ss, w, fd.pic_w, ss);
        const int qy1 = ip_clamp_mv((int)raw.z >> 16, by, h << ss, h, fd.pic_h, ss);

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
            // ---- stage the window once: rows -3 .. th + 3, columns -3 .. tw + 3 ----
#pragma unroll 1
            for (int e0 = li; e0 < ws; e0 += 8 * L) {
                uint8_t v[8];
#pragma unroll
                for (int k = 0; k < 8; k++) {
                    const int e = e0 + k * L;
                    const int rr = (int)(((uint32_t)e * recip) >> 16), cc = e - rr * wd;
                    v[k] = use_l && e < ws ? wbase[(long long)rr * D.ref_stride + cc] : (uint8_t)0;
                }
#pragma unroll
                for (int k = 0; k < 8; k++) {
                    const int e = e0 + k * L;
                    const int rr = (int)(((uint32_t)e * recip) >> 16), cc = e - rr * wd;
                    if (e < ws) win[rr * PW + cc] = v[k];
                }
            }
            wave_lds_fence();
            // ---- three first passes: th + 7 rows of tw per horizontal filter ----
#pragma unroll 1
            for (int f = 0; f < 3; f++) {
                const IpTaps fx = ip_load_taps(ip_table(f, w <= 4), qxl & 15);
                int16_t* const hf = hrb + f * IP_LDS_HR;
#pragma unroll 1
                for (int hrow = row; hrow < th + 7; hrow += th) {
                    const uint2* p = reinterpret_cast<const uint2*>(&win[hrow * PW + col4]);
                    const uint2 a = p[0], bq = p[1], c = p[2];
                    const int s[12] = {(int)(a.x & 0xffff), (int)(a.x >> 16), (int)(a.y & 0xffff), (int)(a.y >> 16),
                                       (int)(bq.x & 0xffff), (int)(bq.x >> 16), (int)(bq.y & 0xffff), (int)(bq.y >> 16),
                                       (int)(c.x & 0xffff), (int)(c.x >> 16), (int)(c.y & 0xffff), (int)(c.y >> 16)};
                    int o[4];
#pragma unroll
                    for (int j = 0; j < 4; j++) {
                        int acc = 4;
#pragma unroll
                        for (int k = 0; k < 8; k++) acc += fx.f[k] * s[j + k];
                        o[j] = acc >> 3;
                    }
                    uint2 pk;
                    pk.x = (uint32_t)(o[0] & 0xffff) | ((uint32_t)o[1] << 16);
                    pk.y = (uint32_t)(o[2] & 0xffff) | ((uint32_t)o[3] << 16);
                    *reinterpret_cast<uint2*>(&hf[hrow * tw + col4]) = pk;
                }
            }
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
        one_list(0, use0, qx0, qy0, D.ref[0]);
        one_list(1, use1, qx1, qy1, D.ref[1]);
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

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
// registers while list 1 goes through the same LDS: the compound intermediate never reaches memory.
#pragma once
#include "dev_common.h"
#include "group_table.h"
#include "inter_plan.h"

namespace svtdev {

// The sub-pel kernels, this project's statement of AV1's interpolation filters (AV1 spec 7.11.3.4; the reference's copies are
// sub_pel_filters_8 / _8smooth / _8sharp, bilinear_filters, sub_pel_filters_4 / _4smooth, EbInterPrediction.c:106-127, :878-922).
// Rows: InterpFilter 0 .. 3 (REGULAR, SMOOTH, SHARP, BILINEAR), then the two 4-tap tables a dimension <= 4 takes instead (REGULAR and
// SHARP -> 4, SMOOTH -> 5).  tests/test_inter_pred_cpu.py reads the rows between the two marker lines and compares them with the
// tables recorded from the compiled reference (tests/golden/inter_pred.npz).
// INTER-TAPS-BEGIN
static __device__ const int16_t kInterTaps[6][16][8] __attribute__((aligned(16))) = {
    {{0, 0, 0, 128, 0, 0, 0, 0}, {0, 2, -6, 126, 8, -2, 0, 0}, {0, 2, -10, 122, 18, -4, 0, 0}, {0, 2, -12, 116, 28, -8, 2, 0},
     {0, 2, -14, 110, 38, -10, 2, 0}, {0, 2, -14, 102, 48, -12, 2, 0}, {0, 2, -16, 94, 58, -12, 2, 0}, {0, 2, -14, 84, 66, -12, 2, 0},
     {0, 2, -14, 76, 76, -14, 2, 0}, {0, 2, -12, 66, 84, -14, 2, 0}, {0, 2, -12, 58, 94, -16, 2, 0}, {0, 2, -12, 48, 102, -14, 2, 0},
     {0, 2, -10, 38, 110, -14, 2, 0}, {0, 2, -8, 28, 116, -12, 2, 0}, {0, 0, -4, 18, 122, -10, 2, 0}, {0, 0, -2, 8, 126, -6, 2, 0}},
    {{0, 0, 0, 128, 0, 0, 0, 0}, {0, 2, 28, 62, 34, 2, 0, 0}, {0, 0, 26, 62, 36, 4, 0, 0}, {0, 0, 22, 62, 40, 4, 0, 0},
     {0, 0, 20, 60, 42, 6, 0, 0}, {0, 0, 18, 58, 44, 8, 0, 0}, {0, 0, 16, 56, 46, 10, 0, 0}, {0, -2, 16, 54, 48, 12, 0, 0},
     {0, -2, 14, 52, 52, 14, -2, 0}, {0, 0, 12, 48, 54, 16, -2, 0}, {0, 0, 10, 46, 56, 16, 0, 0}, {0, 0, 8, 44, 58, 18, 0, 0},
     {0, 0, 6, 42, 60, 20, 0, 0}, {0, 0, 4, 40, 62, 22, 0, 0}, {0, 0, 4, 36, 62, 26, 0, 0}, {0, 0, 2, 34, 62, 28, 2, 0}},
    {{0, 0, 0, 128, 0, 0, 0, 0}, {-2, 2, -6, 126, 8, -2, 2, 0}, {-2, 6, -12, 124, 16, -6, 4, -2}, {-2, 8, -18, 120, 26, -10, 6, -2},
     {-4, 10, -22, 116, 38, -14, 6, -2}, {-4, 10, -22, 108, 48, -18, 8, -2}, {-4, 10, -24, 100, 60, -20, 8, -2}, {-4, 10, -24, 90, 70, -22, 10, -2},
     {-4, 12, -24, 80, 80, -24, 12, -4}, {-2, 10, -22, 70, 90, -24, 10, -4}, {-2, 8, -20, 60, 100, -24, 10, -4}, {-2, 8, -18, 48, 108, -22, 10, -4},
     {-2, 6, -14, 38, 116, -22, 10, -4}, {-2, 6, -10, 26, 120, -18, 8, -2}, {-2, 4, -6, 16, 124, -12, 6, -2}, {0, 2, -2, 8, 126, -6, 2, -2}},
    {{0, 0, 0, 128, 0, 0, 0, 0}, {0, 0, 0, 120, 8, 0, 0, 0}, {0, 0, 0, 112, 16, 0, 0, 0}, {0, 0, 0, 104, 24, 0, 0, 0},
     {0, 0, 0, 96, 32, 0, 0, 0}, {0, 0, 0, 88, 40, 0, 0, 0}, {0, 0, 0, 80, 48, 0, 0, 0}, {0, 0, 0, 72, 56, 0, 0, 0},
     {0, 0, 0, 64, 64, 0, 0, 0}, {0, 0, 0, 56, 72, 0, 0, 0}, {0, 0, 0, 48, 80, 0, 0, 0}, {0, 0, 0, 40, 88, 0, 0, 0},
     {0, 0, 0, 32, 96, 0, 0, 0}, {0, 0, 0, 24, 104, 0, 0, 0}, {0, 0, 0, 16, 112, 0, 0, 0}, {0, 0, 0, 8, 120, 0, 0, 0}},
    {{0, 0, 0, 128, 0, 0, 0, 0}, {0, 0, -4, 126, 8, -2, 0, 0}, {0, 0, -8, 122, 18, -4, 0, 0}, {0, 0, -10, 116, 28, -6, 0, 0},
     {0, 0, -12, 110, 38, -8, 0, 0}, {0, 0, -12, 102, 48, -10, 0, 0}, {0, 0, -14, 94, 58, -10, 0, 0}, {0, 0, -12, 84, 66, -10, 0, 0},
     {0, 0, -12, 76, 76, -12, 0, 0}, {0, 0, -10, 66, 84, -12, 0, 0}, {0, 0, -10, 58, 94, -14, 0, 0}, {0, 0, -10, 48, 102, -12, 0, 0},
     {0, 0, -8, 38, 110, -12, 0, 0}, {0, 0, -6, 28, 116, -10, 0, 0}, {0, 0, -4, 18, 122, -8, 0, 0}, {0, 0, -2, 8, 126, -4, 0, 0}},
    {{0, 0, 0, 128, 0, 0, 0, 0}, {0, 0, 30, 62, 34, 2, 0, 0}, {0, 0, 26, 62, 36, 4, 0, 0}, {0, 0, 22, 62, 40, 4, 0, 0},
     {0, 0, 20, 60, 42, 6, 0, 0}, {0, 0, 18, 58, 44, 8, 0, 0}, {0, 0, 16, 56, 46, 10, 0, 0}, {0, 0, 14, 54, 48, 12, 0, 0},
     {0, 0, 12, 52, 52, 12, 0, 0}, {0, 0, 12, 48, 54, 14, 0, 0}, {0, 0, 10, 46, 56, 16, 0, 0}, {0, 0, 8, 44, 58, 18, 0, 0},
     {0, 0, 6, 42, 60, 20, 0, 0}, {0, 0, 4, 40, 62, 22, 0, 0}, {0, 0, 4, 36, 62, 26, 0, 0}, {0, 0, 2, 34, 62, 30, 0, 0}},
};
// INTER-TAPS-END

typedef unsigned ip_u1 __attribute__((aligned(1)));
typedef unsigned ip_v2u __attribute__((ext_vector_type(2), aligned(1)));
typedef unsigned ip_v4a4 __attribute__((ext_vector_type(4), aligned(4)));       // a block record: d_blk is 4-byte aligned

// av1_get_interp_filter_params_with_block_size (:940-949): the table of InterpFilter f (clamped to 0 .. 3) for a plane dimension
__device__ __forceinline__ int ip_table(int f, bool small) {
    f = f > 3 ? 3 : f;
    return !small || f == 3 ? f : (f == 1 ? 5 : 4);
}

// One list's vector for one direction, as clamp_mv_to_umv_border_sb (:80-102) leaves it: 1/16 plane sample.  org = the block's LUMA
// origin, lsize = its LUMA side, psize = the plane's, pic = the picture's luma side.
__device__ __forceinline__ int ip_clamp_mv(int mv, int org, int lsize, int psize, int pic, int ss) {
    const int mi = org >> 2;
    const int to_lo = -(mi * 32), to_hi = ((pic >> 2) - (lsize >> 2) - mi) * 32;       // mb_to_left / _right_edge, EbAdaptiveMotionVectorPrediction.c:1169-1172
    const int sc = 1 << (1 - ss);
    const int spel_lo = (4 + psize) << 4, spel_hi = spel_lo - 16;                       // AOM_INTERP_EXTEND = 4, SUBPEL_BITS = 4
    const int v = (int16_t)(mv * sc);
    const int lo = to_lo * sc - spel_lo, hi = to_hi * sc + spel_hi;
    return (int16_t)(v < lo ? lo : (v > hi ? hi : v));
}

struct IpTaps { int f[8]; };
__device__ __forceinline__ IpTaps ip_load_taps(int table, int phase) {
    const uint4 r = *reinterpret_cast<const uint4*>(&kInterTaps[table][phase][0]);
    IpTaps t;
    t.f[0] = (int16_t)(r.x & 0xffff); t.f[1] = (int)r.x >> 16; t.f[2] = (int16_t)(r.y & 0xffff); t.f[3] = (int)r.y >> 16;
    t.f[4] = (int16_t)(r.z & 0xffff); t.f[5] = (int)r.z >> 16; t.f[6] = (int16_t)(r.w & 0xffff); t.f[7] = (int)r.w >> 16;
    return t;
}

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
    const int ss = D.ss, w = 1 << D.lw, h = 1 << D.lh, tw = 1 << ge.ltw, th = 1 << ge.lth;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int L = 1 << ge.llanes, slot = lane >> ge.llanes, li = lane & (L - 1);
    const int row = li >> (ge.ltw - 2), col4 = (li & ((tw >> 2) - 1)) << 2;
    const int PW = tw + 8, wd = tw + 7, ws = wd * (th + 7);
    const uint32_t recip = 65536u / (uint32_t)wd + 1;          // e / wd == (e * recip) >> 16 for e < ws <= 529
    uint16_t* const win = &s_win[wave][slot * PW * (th + 7)];
    int16_t* const hrb = &s_hr[wave][slot * tw * (th + 7)];
    const int maxv = (1 << fd.bd) - 1;
    const bool want_dist = D.dist != nullptr;

    uint32_t dist = 0;
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

        // ---- the block: clamp, addressing, filters (device bytes clamped: an out-of-range one changes the prediction, never the window) ----
        ip_v4a4 raw = {0, 0, 0, 0};
        if (active) raw = *reinterpret_cast<const ip_v4a4*>(D.blk + b);
        int bx = raw.x & 0xffff, by = raw.x >> 16;
        bx = min(bx, (int)fd.pic_w - (w << ss));
        by = min(by, (int)fd.pic_h - (h << ss));
        const int dir = min((int)(raw.w & 0xff), 2);
        const int fxi = (raw.w >> 8) & 0xff, fyi = (raw.w >> 16) & 0xff;
        const int tabx = ip_table(fxi, w <= 4), taby = ip_table(fyi, h <= 4);
        const int px = ss ? ((bx >> 3) << 3) >> 1 : bx, py = ss ? ((by >> 3) << 3) >> 1 : by;      // :1282, :1310
        const bool use0 = active && dir != 1, use1 = active && dir != 0;
        const int qx0 = ip_clamp_mv((int16_t)(raw.y & 0xffff), bx, w << ss, w, fd.pic_w, ss);
        const int qy0 = ip_clamp_mv((int)raw.y >> 16, by, h << ss, h, fd.pic_h, ss);
        const int qx1 = ip_clamp_mv((int16_t)(raw.z & 0xffff), bx, w << ss, w, fd.pic_w, ss);
        const int qy1 = ip_clamp_mv((int)raw.z >> 16, by, h << ss, h, fd.pic_h, ss);
        const bool frac = (use0 && ((qx0 | qy0) & 15)) || (use1 && ((qx1 | qy1) & 15));
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
            // ---- stage the window: rows -3 .. th + 3, columns -3 .. tw + 3 ----
            const PIX* const wbase = ref - 3ll * D.ref_stride - 3;
#pragma unroll 1
            for (int e0 = li; e0 < ws; e0 += 8 * L) {
                PIX v[8];
#pragma unroll
                for (int k = 0; k < 8; k++) {
                    const int e = e0 + k * L;
                    const int rr = (int)(((uint32_t)e * recip) >> 16), cc = e - rr * wd;
                    v[k] = use_l && e < ws ? wbase[(long long)rr * D.ref_stride + cc] : (PIX)0;
                }
#pragma unroll
                for (int k = 0; k < 8; k++) {
                    const int e = e0 + k * L;
                    const int rr = (int)(((uint32_t)e * recip) >> 16), cc = e - rr * wd;
                    if (e < ws) win[rr * PW + cc] = v[k];
                }
            }
            wave_lds_fence();
            // ---- first pass: th + 7 rows of tw, four outputs of a row per lane and step ----
            {
                const IpTaps fx = ip_load_taps(tabx, qxl & 15);
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
                    *reinterpret_cast<uint2*>(&hrb[hrow * tw + col4]) = pk;
                }
            }
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
        one_list(V0, use0, qx0, qy0, D.ref[0]);
        one_list(V1, use1, qx1, qy1, D.ref[1]);

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
            if (D.pred_stride == 0) dst += (size_t)b * (size_t)(w * h) + (size_t)((ty + row) * w + tx + col4);
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

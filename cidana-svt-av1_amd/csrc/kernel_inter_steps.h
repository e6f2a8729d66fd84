// kernel_inter_steps.h — what the kernels that run AV1's sub-pel convolve share: inter_pred_kernel (kernel_inter_pred.h), which states the
// arithmetic (hr, V, the rounding), and interp_sse_kernel (kernel_interp_search.h).  The tap tables and the vector clamp, then the four
// steps of a wave over the tiling of inter_plan.h's InterGeom, each stated once: the lane geometry (ip_lane), the tile and block record
// of a round (ip_block), one list's window into LDS (ip_stage_window) and one horizontal first pass over it (ip_first_pass).  Values in,
// values out: the LDS arrays, the second passes, the rounding and the sums are each kernel's own.
#pragma once
#include "dev_common.h"
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

// ---- the lane geometry of a wave: filled once per kernel ----
struct IpLane {
    int ss, lw, w, h, tw, th;        // the plane block and its tile
    int wave, lane, L, slot, li;     // L lanes hold a slot (a tile of the wave); li: the lane within its slot
    int row, col4;                   // the lane's four samples: row and first column of the tile
    int PW, wd, ws;                  // the staged window: LDS row pitch, width tw + 7, samples wd * (th + 7)
    uint32_t recip;                  // e / wd == (e * recip) >> 16 for e < ws <= 529
};
__device__ __forceinline__ IpLane ip_lane(const InterGeom& ge, int ss, int lw, int lh) {
    IpLane T;
    T.ss = ss; T.lw = lw; T.w = 1 << lw; T.h = 1 << lh; T.tw = 1 << ge.ltw; T.th = 1 << ge.lth;
    T.wave = threadIdx.x >> 6; T.lane = threadIdx.x & 63;
    T.L = 1 << ge.llanes; T.slot = T.lane >> ge.llanes; T.li = T.lane & (T.L - 1);
    T.row = T.li >> (ge.ltw - 2); T.col4 = (T.li & ((T.tw >> 2) - 1)) << 2;
    T.PW = T.tw + 8; T.wd = T.tw + 7; T.ws = T.wd * (T.th + 7);
    T.recip = 65536u / (uint32_t)T.wd + 1;
    return T;
}

// ---- the tile and block of round r: clamp and addressing (device bytes clamped: an out-of-range one changes the prediction, never the
// window).  w3 is the record's fourth word: direction, filter_x, filter_y ----
struct IpBlock {
    uint32_t b, w3;                  // the block of the group; inactive past nblocks
    int tx, ty;                      // the tile's origin in the block
    int dir, px, py;                 // 0 list 0, 1 list 1, 2 BI_PRED; the block's origin in the plane
    int qx0, qy0, qx1, qy1;          // the lists' clamped vectors, 1/16 plane sample
    bool active, use0, use1;
};
__device__ __forceinline__ IpBlock ip_block(const InterGeom& ge, const IpLane& T, int r, uint32_t bid, const svt_hip_inter_blk* blk, uint32_t nblocks,
                                            uint32_t pic_w, uint32_t pic_h) {
    IpBlock B;
    const int ss = T.ss, w = T.w, h = T.h;
    const uint32_t t = (uint32_t)(r * IP_WAVES + T.wave) * ge.slots + T.slot;         // tile of the workgroup
    B.b = bid * ge.blocks_per_wg + (ge.rounds > 1 ? 0 : t >> ge.ltpb);
    const int ti = t & ((1 << ge.ltpb) - 1);
    B.tx = (ti & ((w >> ge.ltw) - 1)) << ge.ltw; B.ty = (ti >> (T.lw - ge.ltw)) << ge.lth;
    B.active = B.b < nblocks;
    ip_v4a4 raw = {0, 0, 0, 0};
    if (B.active) raw = *reinterpret_cast<const ip_v4a4*>(blk + B.b);
    int bx = raw.x & 0xffff, by = raw.x >> 16;
    bx = min(bx, (int)pic_w - (w << ss));
    by = min(by, (int)pic_h - (h << ss));
    B.w3 = raw.w;
    B.dir = min((int)(raw.w & 0xff), 2);
    B.px = ss ? ((bx >> 3) << 3) >> 1 : bx; B.py = ss ? ((by >> 3) << 3) >> 1 : by;      // :1282, :1310
    B.use0 = B.active && B.dir != 1; B.use1 = B.active && B.dir != 0;
    B.qx0 = ip_clamp_mv((int16_t)(raw.y & 0xffff), bx, w << ss, w, pic_w, ss);
    B.qy0 = ip_clamp_mv((int)raw.y >> 16, by, h << ss, h, pic_h, ss);
    B.qx1 = ip_clamp_mv((int16_t)(raw.z & 0xffff), bx, w << ss, w, pic_w, ss);
    B.qy1 = ip_clamp_mv((int)raw.z >> 16, by, h << ss, h, pic_h, ss);
    return B;
}

// ---- one list's window into LDS as uint16: rows -3 .. th + 3, columns -3 .. tw + 3 of the tile whose sample (-3, -3) is wbase[0]; every
// load of a batch of 8 is issued before the first LDS write.  A lane without the list (use_l false) loads nothing and writes zeros ----
template <typename PIX>
__device__ __forceinline__ void ip_stage_window(const IpLane& T, uint16_t* win, const PIX* wbase, uint32_t ref_stride, bool use_l) {
#pragma unroll 1
    for (int e0 = T.li; e0 < T.ws; e0 += 8 * T.L) {
        PIX v[8];
#pragma unroll
        for (int k = 0; k < 8; k++) {
            const int e = e0 + k * T.L;
            const int rr = (int)(((uint32_t)e * T.recip) >> 16), cc = e - rr * T.wd;
            v[k] = use_l && e < T.ws ? wbase[(long long)rr * ref_stride + cc] : (PIX)0;
        }
#pragma unroll
        for (int k = 0; k < 8; k++) {
            const int e = e0 + k * T.L;
            const int rr = (int)(((uint32_t)e * T.recip) >> 16), cc = e - rr * T.wd;
            if (e < T.ws) win[rr * T.PW + cc] = v[k];
        }
    }
    wave_lds_fence();
}

// ---- one first pass with the taps fx: the window's th + 7 rows of tw into packed int16 rows at hr, four outputs of a row per lane and
// step: hr = (sum fx[k] * p[x - 3 + k] + 4) >> 3.  The caller fences before it reads the rows ----
__device__ __forceinline__ void ip_first_pass(const IpLane& T, const uint16_t* win, int16_t* hr, const IpTaps& fx) {
#pragma unroll 1
    for (int hrow = T.row; hrow < T.th + 7; hrow += T.th) {
        const uint2* p = reinterpret_cast<const uint2*>(&win[hrow * T.PW + T.col4]);
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
        *reinterpret_cast<uint2*>(&hr[hrow * T.tw + T.col4]) = pk;
    }
}

}  // namespace svtdev

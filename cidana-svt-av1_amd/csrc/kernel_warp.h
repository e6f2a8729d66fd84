// kernel_warp.h — AV1 warped motion for many groups in one launch: the local warp model of a (block, candidate) (warp_fit_kernel:
// warped_motion_parameters from the point where the samples exist, EbAdaptiveMotionVectorPrediction.c:1876-1937, find_affine_int and
// get_shear_params, EbWarpedMotion.c:1066, :344) and the warp filter (warp_pred_kernel: av1_warp_affine_c / av1_highbd_warp_affine_c,
// :672, :389, as warped_motion_prediction calls them) with the distortion against the source summed while the prediction is in
// registers.
//
// The filter, per 8 x 8 tile at (j, i) of the plane block, with round_0 = 3 and a single reference (get_conv_params_no_round):
//     centre   (j + 4) << ss, (i + 4) << ss through mat in wrapping int32; x4 = dst_x >> ss; ix4 = x4 >> 16;
//              sx4 = ((x4 & 0xffff) - 4 * (alpha + beta)) & ~63, and likewise iy4, sy4 with gamma, delta
//     first    hr[k][l] = ((1 << (bd + 6)) + sum_m f(sx4 + beta * (k - 3) + alpha * l)[m] * p[iy4 - 7 + k][ix4 - 7 + l + m] + 4) >> 3,
//              k 0 .. 14, l 0 .. 7: unsigned, 13 bits at bd 8 and 15 at bd 10, kept as uint16
//     second   pred[k][l] = clip((((1 << (bd + 11)) + sum_m f(sy4 + delta * k + gamma * l)[m] * hr[k + m][l] + 1024) >> 11)
//                                - (1 << (bd - 1)) - (1 << bd)),   k, l 0 .. 7
//     f(s)     row ((s + 512) >> 10) + 64 of the filter (warp_tables.h), the row clamped to 0 .. 192
// and both coordinates of p clamped to the plane.
//
// Work split (warp_plan.h, WarpGeom): a wave per tile, four tiles per workgroup.  The wave stages its 15 x 15 window into LDS already
// clamped, runs the first pass over 120 outputs in two steps into LDS, and the second pass with one output per lane into a register;
// the distortion is one wave sum per slot and wave.  The filter sits in LDS as 8 bytes per row.
#pragma once
#include "dev_common.h"
#include "group_table.h"
#include "warp_plan.h"
#include "warp_tables.h"

namespace svtdev {

static __device__ const svtwarp::WarpFilter kWarpTaps __attribute__((aligned(16))) = svtwarp::kWarpFilter;
static __device__ const svtwarp::DivLut kWarpDivLut = svtwarp::kDivLut;
constexpr int WP_TAB_WORDS = svtwarp::kWarpRows * 2;

static_assert(sizeof(svt_hip_warp_model) == 36 && alignof(svt_hip_warp_model) == 4, "the kernels move the record as nine words");
static_assert(sizeof(svt_hip_warp_samples) == 132, "svt_hip_warp_samples layout");

struct WpTaps { int f[8]; };
__device__ __forceinline__ WpTaps wp_taps(const uint32_t* tab, int s) {
    int offs = ((s + 512) >> 10) + 64;
    offs = offs < 0 ? 0 : (offs > 192 ? 192 : offs);
    const uint2 r = *reinterpret_cast<const uint2*>(&tab[offs * 2]);
    WpTaps t;
#pragma unroll
    for (int m = 0; m < 4; m++) {
        t.f[m] = (int)(int8_t)(r.x >> (8 * m));
        t.f[4 + m] = (int)(int8_t)(r.y >> (8 * m));
    }
    return t;
}

template <typename PIX>
__global__ __launch_bounds__(WP_THREADS) void warp_pred_kernel(const WarpPredDesc fd) {
    __shared__ __attribute__((aligned(16))) uint32_t s_tab[WP_TAB_WORDS];
    __shared__ __attribute__((aligned(16))) uint16_t s_win[WP_WAVES][15 * 16];
    __shared__ __attribute__((aligned(16))) uint16_t s_hr[WP_WAVES][15 * 8];
    __shared__ uint32_t s_part[WP_WAVES];

    for (int i = threadIdx.x; i < WP_TAB_WORDS; i += WP_THREADS) s_tab[i] = reinterpret_cast<const uint32_t*>(&kWarpTaps.t[0][0])[i];
    __syncthreads();

    uint32_t bid;
    const int gi = group_of(fd, bid);
    if (gi >= fd.ngroups) return;
    const WarpPredGroupDev& D = fd.g[gi];
    const WarpShape S = warp_shape_unpack(D.shape);
    const WarpGeom ge = warp_geom(S.lw, S.lh);
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)), lane = threadIdx.x & 63;
    const int ss = S.ss, w = 1 << S.lw, h = 1 << S.lh;
    const int PW = (int)(fd.pic_w >> ss), PH = (int)(fd.pic_h >> ss);
    const int bd = fd.bd, maxv = (1 << bd) - 1;
    uint16_t* const win = s_win[wave];
    uint16_t* const hrb = s_hr[wave];

    // ---- the slot of this wave, its record and its model: wave-uniform ----
    const uint32_t slot = bid * (uint32_t)ge.slots_per_wg + (uint32_t)(ge.ltpb <= 2 ? wave >> ge.ltpb : 0);
    bool live = slot < D.nslots;
    uint32_t rec = slot;
    if (live && D.sel) {
        const int c = (int)D.sel[slot] - S.sel_first;
        live = c >= 0 && c < S.ncand;
        rec = slot / (uint32_t)S.n * (uint32_t)S.ncand + (uint32_t)(live ? c : 0);
    }
    int mat[6] = {0, 0, 0, 0, 0, 0}, alpha = 0, beta = 0, gamma = 0, delta = 0, px = 0, py = 0;
    if (live) {
        const uint32_t* mw = reinterpret_cast<const uint32_t*>(&D.model[rec]);
        live = (mw[8] & 0xff) != 0;                                   // valid
        if (live) {
#pragma unroll
            for (int i = 0; i < 6; i++) mat[i] = (int)mw[i];
            alpha = (int16_t)(mw[6] & 0xffff); beta = (int)mw[6] >> 16; gamma = (int16_t)(mw[7] & 0xffff); delta = (int)mw[7] >> 16;
            const uint32_t xy = *reinterpret_cast<const uint32_t*>(&D.blk[rec]);
            const int x = min((int)(xy & 0xffff), (int)fd.pic_w - (w << ss)), y = min((int)(xy >> 16), (int)fd.pic_h - (h << ss));
            px = x >> ss; py = y >> ss;
        }
    }

    uint32_t dist = 0;
#pragma unroll 1
    for (int r = 0; r < ge.rounds; r++) {
        const int t = ge.ltpb <= 2 ? (wave & ((1 << ge.ltpb) - 1)) : r * WP_WAVES + wave;       // the tile of the block
        const int tx = (t & ((1 << ge.ltx) - 1)) << 3, ty = (t >> ge.ltx) << 3;
        if (!live) continue;
        const uint32_t cx = (uint32_t)((px + tx + 4) << ss), cy = (uint32_t)((py + ty + 4) << ss);
        const int dst_x = (int)((uint32_t)mat[2] * cx + (uint32_t)mat[3] * cy + (uint32_t)mat[0]);
        const int dst_y = (int)((uint32_t)mat[4] * cx + (uint32_t)mat[5] * cy + (uint32_t)mat[1]);
        const int x4 = dst_x >> ss, y4 = dst_y >> ss;
        const int ix4 = x4 >> 16, iy4 = y4 >> 16;
        const int sx4 = ((x4 & 0xffff) - 4 * (alpha + beta)) & ~63, sy4 = ((y4 & 0xffff) - 4 * (gamma + delta)) & ~63;

        // ---- the 15 x 15 window, clamped to the plane, rows of 16 in LDS ----
        const PIX* const ref = reinterpret_cast<const PIX*>(D.ref);
#pragma unroll
        for (int e = lane; e < 15 * 16; e += 64) {
            const int wr = e >> 4, wc = e & 15;
            const int row = min(max(iy4 - 7 + wr, 0), PH - 1), col = min(max(ix4 - 7 + wc, 0), PW - 1);
            win[e] = (uint16_t)ref[(size_t)row * D.ref_stride + (size_t)col];
        }
        wave_lds_fence();
        // ---- first pass: 15 rows of 8 ----
#pragma unroll
        for (int e = lane; e < 15 * 8; e += 64) {
            const int k = e >> 3, l = e & 7;
            const WpTaps f = wp_taps(s_tab, sx4 + beta * (k - 3) + alpha * l);
            int sum = (1 << (bd + 6)) + 4;
#pragma unroll
            for (int m = 0; m < 8; m++) sum += f.f[m] * (int)win[k * 16 + l + m];
            hrb[e] = (uint16_t)(sum >> 3);
        }
        wave_lds_fence();
        // ---- second pass: this lane's sample ----
        const int k = lane >> 3, l = lane & 7;
        const WpTaps f = wp_taps(s_tab, sy4 + delta * k + gamma * l);
        int sum = (1 << (bd + 11)) + 1024;
#pragma unroll
        for (int m = 0; m < 8; m++) sum += f.f[m] * (int)hrb[(k + m) * 8 + l];
        const int o = min(max((sum >> 11) - (1 << (bd - 1)) - (1 << bd), 0), maxv);
        wave_lds_fence();                           // the next round stages over this one's window and rows

        if (D.pred) {
            PIX* dst = reinterpret_cast<PIX*>(D.pred);
            if (D.pred_stride == 0) dst += (size_t)slot * (size_t)(w * h) + (size_t)((ty + k) * w + tx + l);
            else dst += (size_t)(py + ty + k) * D.pred_stride + (size_t)(px + tx + l);
            *dst = (PIX)o;
        }
        if (D.dist) {
            const PIX* sp = reinterpret_cast<const PIX*>(D.src) + (size_t)(py + ty + k) * D.src_stride + (size_t)(px + tx + l);
            const int d = o - (int)*sp;
            dist += fd.metric == SVT_HIP_FAST_SSD ? (uint32_t)(d * d) : (uint32_t)(d < 0 ? -d : d);
        }
    }

    if (D.dist) {             // group-uniform: every wave of the workgroup takes the barrier
        // at most 16 tiles of a slot per wave: the 32-bit sum holds 1024 * 1023^2
        const uint32_t wsum = group_sum_rt(dist, 64);
        if (lane == 0) s_part[wave] = wsum;
        __syncthreads();
        if (lane == 0 && live && (wave & (ge.waves_per_slot - 1)) == 0) {
            unsigned long long sum = 0;
            for (int i = 0; i < ge.waves_per_slot; i++) sum += s_part[wave + i];
            D.dist[slot] = sum;
        }
    }
}

// ---- the model fit: a wave per block, a lane per candidate ----
__device__ __forceinline__ long long wp_round_signed64(long long v, int n) {
    const long long half = (1ll << n) >> 1;
    return v < 0 ? -((-v + half) >> n) : (v + half) >> n;
}
__device__ __forceinline__ long long wp_clamp64(long long v, long long lo, long long hi) { return v < lo ? lo : (v > hi ? hi : v); }
__device__ __forceinline__ int wp_clamp16(int v) { return v < -32768 ? -32768 : (v > 32767 ? 32767 : v); }
// resolve_divisor_32 / _64: 1 / d = y / 2^shift for d > 0
__device__ __forceinline__ int wp_resolve_divisor(unsigned long long d, int& shift) {
    shift = 63 - __clzll((long long)d);
    const long long e = (long long)(d - (1ull << shift));
    const long long f = shift > 8 ? (e + ((1ll << (shift - 8)) >> 1)) >> (shift - 8) : e << (8 - shift);
    shift += 14;
    return kWarpDivLut.v[f > 256 ? 256 : f];
}
// ROUND_POWER_OF_TWO_SIGNED(v, WARP_PARAM_REDUCE_BITS) * (1 << WARP_PARAM_REDUCE_BITS), stored into an int16
__device__ __forceinline__ int wp_reduce(int v) { return (int16_t)((v < 0 ? -((-v + 32) >> 6) : (v + 32) >> 6) * 64); }

__global__ __launch_bounds__(WP_THREADS) void warp_fit_kernel(const WarpFitDesc fd) {
    uint32_t bid;
    const int gi = group_of(fd, bid);
    if (gi >= fd.ngroups) return;
    const WarpFitGroupDev& D = fd.g[gi];
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)), lane = threadIdx.x & 63;
    const uint32_t b = bid * WP_WAVES + (uint32_t)wave;
    if (b >= D.nblocks) return;
    const bool act = lane < (int)D.ncand;
    const int bw = D.bw, bh = D.bh;
    const int* const S = reinterpret_cast<const int*>(&D.samples[b]);
    const int ns = min(max(S[0], 0), 8);
    const int* const pts = S + 1;
    const int* const ptr = S + 17;

    int mat[6] = {0, 0, 0, 0, 0, 0}, alpha = 0, beta = 0, gamma = 0, delta = 0, n = 0;
    bool valid = false;
    if (act && ns > 0) {
        const uint32_t* bw32 = reinterpret_cast<const uint32_t*>(&D.blk[(size_t)b * D.ncand + (size_t)lane]);
        const uint32_t xy = bw32[0], mv = bw32[1];
        const int x = (int)(xy & 0xffff), y = (int)(xy >> 16), mvx = (int16_t)(mv & 0xffff), mvy = (int)mv >> 16;
        // select_samples: the kept samples as a mask (the reference's walk only permutes them; every sum below is order-free)
        uint32_t keep = 1;
        n = ns;
        if (ns > 1) {
            const int m = max(bw, bh), thresh = m < 16 ? 16 : (m > 112 ? 112 : m);
            keep = 0;
            for (int i = 0; i < ns; i++) {
                const int dx = ptr[2 * i] - pts[2 * i] - mvx, dy = ptr[2 * i + 1] - pts[2 * i + 1] - mvy;
                if ((dx < 0 ? -dx : dx) + (dy < 0 ? -dy : dy) <= thresh) keep |= 1u << i;
            }
            n = __popc(keep);
            if (!n) { keep = 1; n = 1; }                  // keep at least 1: the arrays as they are, one sample
        }
        // find_affine_int
        const int rsuy = bh / 2 - 1, rsux = bw / 2 - 1;
        const int suy = rsuy * 8, sux = rsux * 8, duy = suy + mvy, dux = sux + mvx;
        const int isuy = (y >> 2) * 4 + rsuy, isux = (x >> 2) * 4 + rsux;
        int a00 = 0, a01 = 0, a11 = 0, bx0 = 0, bx1 = 0, by0 = 0, by1 = 0;
        for (int i = 0; i < ns; i++) {
            if (!(keep >> i & 1)) continue;
            const int dx = ptr[2 * i] - dux, dy = ptr[2 * i + 1] - duy, sx = pts[2 * i] - sux, sy = pts[2 * i + 1] - suy;
            const int ex = sx - dx, ey = sy - dy;
            if ((ex < 0 ? -ex : ex) < 256 && (ey < 0 ? -ey : ey) < 256) {              // LS_MV_MAX
                a00 += (sx * sx * 4 + sx * 32 + 128) >> 4;                           // LS_SQUARE
                a01 += (sx * sy * 4 + (sx + sy) * 16 + 64) >> 4;                     // LS_PRODUCT1
                a11 += (sy * sy * 4 + sy * 32 + 128) >> 4;
                bx0 += (sx * dx * 4 + (sx + dx) * 16 + 128) >> 4;                    // LS_PRODUCT2
                bx1 += (sy * dx * 4 + (sy + dx) * 16 + 64) >> 4;
                by0 += (sx * dy * 4 + (sx + dy) * 16 + 64) >> 4;
                by1 += (sy * dy * 4 + (sy + dy) * 16 + 128) >> 4;
            }
        }
        const long long det = (long long)a00 * a11 - (long long)a01 * a01;
        if (det != 0) {
            int shift;
            int idet = wp_resolve_divisor((unsigned long long)(det < 0 ? -det : det), shift) * (det < 0 ? -1 : 1);
            shift -= 16;
            if (shift < 0) { idet = (int16_t)(idet * (1 << -shift)); shift = 0; }      // int16_t iDet <<= -shift
            const long long px0 = (long long)a11 * bx0 - (long long)a01 * bx1, px1 = -(long long)a01 * bx0 + (long long)a00 * bx1;
            const long long py0 = (long long)a11 * by0 - (long long)a01 * by1, py1 = -(long long)a01 * by0 + (long long)a00 * by1;
            const long long nd = 1 << 13;                                            // WARPEDMODEL_NONDIAGAFFINE_CLAMP
            mat[2] = (int)wp_clamp64(wp_round_signed64(px0 * idet, shift), 65536 - nd + 1, 65536 + nd - 1);
            mat[3] = (int)wp_clamp64(wp_round_signed64(px1 * idet, shift), -nd + 1, nd - 1);
            mat[4] = (int)wp_clamp64(wp_round_signed64(py0 * idet, shift), -nd + 1, nd - 1);
            mat[5] = (int)wp_clamp64(wp_round_signed64(py1 * idet, shift), 65536 - nd + 1, 65536 + nd - 1);
            const int vx = mvx * 8192 - (isux * (mat[2] - 65536) + isuy * mat[3]);
            const int vy = mvy * 8192 - (isux * mat[4] + isuy * (mat[5] - 65536));
            const int tc = 128 << 16;                                                // WARPEDMODEL_TRANS_CLAMP
            mat[0] = vx < -tc ? -tc : (vx > tc - 1 ? tc - 1 : vx);
            mat[1] = vy < -tc ? -tc : (vy > tc - 1 ? tc - 1 : vy);
            // get_shear_params
            if (mat[2] > 0) {
                int sh;
                const long long yv = wp_resolve_divisor((unsigned long long)mat[2], sh);
                alpha = wp_clamp16(mat[2] - 65536);
                beta = wp_clamp16(mat[3]);
                gamma = wp_clamp16((int)wp_round_signed64((long long)mat[4] * 65536 * yv, sh));
                delta = wp_clamp16(mat[5] - (int)wp_round_signed64((long long)mat[3] * mat[4] * yv, sh) - 65536);
                alpha = wp_reduce(alpha); beta = wp_reduce(beta); gamma = wp_reduce(gamma); delta = wp_reduce(delta);
                const int aa = alpha < 0 ? -alpha : alpha, ab = beta < 0 ? -beta : beta, ag = gamma < 0 ? -gamma : gamma, ad = delta < 0 ? -delta : delta;
                valid = 4 * aa + 7 * ab < 65536 && 4 * ag + 4 * ad < 65536;          // is_affine_shear_allowed
            }
        }
    }
    if (act) {
        uint32_t* mw = reinterpret_cast<uint32_t*>(&D.model[(size_t)b * D.ncand + (size_t)lane]);
#pragma unroll
        for (int i = 0; i < 6; i++) mw[i] = (uint32_t)mat[i];
        mw[6] = ((uint32_t)alpha & 0xffff) | ((uint32_t)beta << 16);
        mw[7] = ((uint32_t)gamma & 0xffff) | ((uint32_t)delta << 16);
        mw[8] = (valid ? 1u : 0u) | ((uint32_t)n << 8);
    }
    if (D.nvalid) {
        const unsigned long long bal = __ballot(act && valid);
        if (lane == 0) D.nvalid[b] = (uint32_t)__popcll(bal);
    }
}

}  // namespace svtdev

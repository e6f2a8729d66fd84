// kernel_picture_stats.h — GatheringPictureStatistics (EbPictureAnalysisProcess.c:4759-4812) for whole pictures: the 85 luma block
// means / variances and the 21 Cb / Cr block means of every 64x64 SB (ComputeBlockMeanComputeVariance :2066, ComputeChromaBlockMean
// :1770, ZeroOutChromaBlockMean :1706), the per-region histograms of the 1/16 luma and the chroma planes (:4146-4284, CalculateHistogram
// :201) with their average intensities, and the per-picture sums (pic_avg_variance :4689, average_intensity :4746-4748).
//
// Two launches.  picture_stats_kernel: blockIdx.x < nhist is one (region, plane) histogram in LDS, the blocks after them four SBs each
// (the histogram blocks walk the most samples per block, so they are dispatched first); blockIdx.y = picture.  picture_stats_sum_kernel:
// one block per picture adds up what the first launch wrote: the SBs' 64x64 variances, and the region sums, which it takes back out
// of the histograms (bin v holds (1 + count) << 4, so a plane's sum is the sum of v * count): no scratch, no atomics in global
// memory, nothing to zero.  All integer: the result does not depend on the order of the LDS adds.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "dev_common.h"

namespace svtdev {

constexpr int PST_THREADS = 256;
constexpr int PST_PUS = 85, PST_CHROMA_PUS = 21;      // ME_TIER_ZERO_PU_*: 0 = 64x64, 1-4 = 32x32, 5-20 = 16x16, 21-84 = 8x8
constexpr int PST_SBS = 4;                            // SBs per workgroup
constexpr int PST_SB_WORDS = 2 * PST_PUS + 2 * PST_CHROMA_PUS;       // an SB's trees in LDS: mean, mean of squares, Cb, Cr

struct PicStatsDev {
    const uint8_t* plane[4];       // buffer starts: luma, Cb, Cr, 1/16 luma
    uint32_t stride[4];
    uint64_t pitch[4];             // between the pictures of a stack
    uint32_t ox, oy;               // luma origin (the chroma addresses derive from it as the reference's do, (origin + offset) >> 1)
    uint32_t ox16, oy16;           // origin of the 1/16 picture
    uint32_t width, height;        // luma
    uint32_t nsbx, nsb;
    uint32_t rw, rh, nhist;        // regions per width / height, rw * rh * 3
    uint32_t sub;                  // BLOCK_MEAN_PREC_SUB: rows 0, 2, 4, 6 of an 8x8 block
    uint8_t* y_mean; uint16_t* variance; uint8_t* cb_mean; uint8_t* cr_mean;
    uint16_t* pic_avg_variance; uint32_t* histogram; uint8_t* avg_region; uint8_t* avg;
};

// sum and sum of squares of the 8 bytes (a, b)
__device__ __forceinline__ void pst_sums8(uint32_t a, uint32_t b, uint32_t& s, uint32_t& q) {
    s = __builtin_amdgcn_sad_u8(a, 0u, __builtin_amdgcn_sad_u8(b, 0u, 0u));
    q = __builtin_amdgcn_udot4(a, a, __builtin_amdgcn_udot4(b, b, 0u, false), false);
}

// (a + b + c + d) >> 2 of the four children of node (r, c) in a raster grid `n` nodes wide
__device__ __forceinline__ uint32_t pst_quad(const uint32_t* v, int r, int c, int n) {
    const uint32_t* p = v + 2 * r * n + 2 * c;
    return (uint32_t)(((uint64_t)p[0] + p[1] + p[n] + p[n + 1]) >> 2);
}

// PST_SBS consecutive SBs (raster order) per workgroup: every lane has that many 16-byte luma loads in flight (a workgroup with one
// SB per lane-load ran at the latency of that one load).  Luma: lane t loads 16 bytes of row t / 4 (two 8x8 blocks' worth), the eight
// rows of a block sit in lanes 4 apart.  Chroma (complete SBs only): wave 0 is Cb, wave 1 is Cr, lane l loads 16 bytes of row l / 2, a
// block's rows sit in lanes 2 apart; the lanes of an incomplete SB keep zeros, which is what ZeroOutChromaBlockMean stores.  SUB: the
// odd rows are not read at all; their lanes add zeros.
__device__ __forceinline__ void pst_sbs(const PicStatsDev& d, uint32_t sb0, uint32_t pic, uint32_t* lds) {
    const int t = (int)threadIdx.x;
    const bool odd_row_off = d.sub != 0;
    const int lrow = t >> 2, lseg = t & 3;                                  // luma: row, 16-byte segment
    const int cpl = (t >> 6) & 1, crow = (t & 63) >> 1, cseg = t & 1;       // chroma (lanes 0 .. 127): plane, row, segment
    const int ms = d.sub ? 3 : 2, qs = d.sub ? 11 : 10;

    uint32_t v[PST_SBS][4], cv[PST_SBS][4];
#pragma unroll
    for (int k = 0; k < PST_SBS; k++) {
#pragma unroll
        for (int q = 0; q < 4; q++) v[k][q] = cv[k][q] = 0;
        const uint32_t sb = sb0 + k;
        if (sb >= d.nsb) continue;
        const uint32_t sbx = sb % d.nsbx, sby = sb / d.nsbx;
        const bool complete = sbx * 64 + 64 <= d.width && sby * 64 + 64 <= d.height;       // is_complete_sb
        if (!(odd_row_off && (lrow & 1)))
            cfl_ld<16>(v[k], d.plane[0] + pic * d.pitch[0] + (size_t)(d.oy + sby * 64 + lrow) * d.stride[0] + d.ox + sbx * 64 + lseg * 16);
        if (complete && t < 128 && !(odd_row_off && (crow & 1)))
            cfl_ld<16>(cv[k], d.plane[1 + cpl] + pic * d.pitch[1 + cpl] + (size_t)(((d.oy + sby * 64) >> 1) + crow) * d.stride[1 + cpl] +
                                  ((d.ox + sbx * 64) >> 1) + cseg * 16);
    }
#pragma unroll
    for (int k = 0; k < PST_SBS; k++) {
        uint32_t* M = lds + k * PST_SB_WORDS;          // [85] mean, ME_TIER_ZERO_PU order
        uint32_t* Q = M + PST_PUS;                     // [85] mean of squares
        uint32_t* C = M + 2 * PST_PUS;                 // [2][21] chroma mean
        uint32_t s0, q0, s1, q1;
        pst_sums8(v[k][0], v[k][1], s0, q0);
        pst_sums8(v[k][2], v[k][3], s1, q1);
#pragma unroll
        for (int m = 4; m <= 16; m <<= 1) {
            s0 += __shfl_xor(s0, m, 64); q0 += __shfl_xor(q0, m, 64);
            s1 += __shfl_xor(s1, m, 64); q1 += __shfl_xor(q1, m, 64);
        }
        if ((lrow & 7) == 0) {
            const int b = (lrow >> 3) * 8 + lseg * 2;
            M[21 + b] = s0 << ms; Q[21 + b] = q0 << qs;
            M[22 + b] = s1 << ms; Q[22 + b] = q1 << qs;
        }
        if (t < 128) {
            uint32_t c0, c1, unused0, unused1;
            pst_sums8(cv[k][0], cv[k][1], c0, unused0);
            pst_sums8(cv[k][2], cv[k][3], c1, unused1);
#pragma unroll
            for (int m = 2; m <= 8; m <<= 1) { c0 += __shfl_xor(c0, m, 64); c1 += __shfl_xor(c1, m, 64); }
            if ((crow & 7) == 0) {
                const int b = (crow >> 3) * 4 + cseg * 2;
                C[cpl * PST_CHROMA_PUS + 5 + b] = c0 << ms;
                C[cpl * PST_CHROMA_PUS + 6 + b] = c1 << ms;
            }
        }
    }
    __syncthreads();
    if (t < 16 * PST_SBS) {                                                               // 16x16 (:2843-2881)
        uint32_t* M = lds + (t >> 4) * PST_SB_WORDS;
        const int i = t & 15;
        M[5 + i] = pst_quad(M + 21, i >> 2, i & 3, 8); M[PST_PUS + 5 + i] = pst_quad(M + PST_PUS + 21, i >> 2, i & 3, 8);
    } else if (t >= 64 && t < 64 + 8 * PST_SBS) {                                         // chroma 32x32 (:1992-2003)
        const int u = t - 64, j = u & 3;
        uint32_t* C = lds + (u >> 3) * PST_SB_WORDS + 2 * PST_PUS + ((u >> 2) & 1) * PST_CHROMA_PUS;
        C[1 + j] = pst_quad(C + 5, j >> 1, j & 1, 4);
    }
    __syncthreads();
    if (t < 4 * PST_SBS) {                                                                // 32x32 (:2884-2893)
        uint32_t* M = lds + (t >> 2) * PST_SB_WORDS;
        const int i = t & 3;
        M[1 + i] = pst_quad(M + 5, i >> 1, i & 1, 4); M[PST_PUS + 1 + i] = pst_quad(M + PST_PUS + 5, i >> 1, i & 1, 4);
    } else if (t >= 64 && t < 64 + 2 * PST_SBS) {
        // chroma 64x64, the reference's line as written (:2006-2007): entry 2 is never added, entry 3 twice
        const int u = t - 64;
        uint32_t* C = lds + (u >> 1) * PST_SB_WORDS + 2 * PST_PUS + (u & 1) * PST_CHROMA_PUS;
        C[0] = (C[1] + C[2] + C[4] + C[4]) >> 2;
    }
    __syncthreads();
    if (t < PST_SBS) {                                                                    // 64x64 (:2895-2896)
        uint32_t* M = lds + t * PST_SB_WORDS;
        M[0] = pst_quad(M + 1, 0, 0, 2); M[PST_PUS] = pst_quad(M + PST_PUS + 1, 0, 0, 2);
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < PST_SBS; k++) {
        if (sb0 + k >= d.nsb) continue;
        const uint32_t* M = lds + k * PST_SB_WORDS;
        const size_t s = (size_t)pic * d.nsb + sb0 + k;
        if (t < PST_PUS) {
            const uint64_t m = M[t], q = M[PST_PUS + t];
            d.y_mean[s * PST_PUS + t] = (uint8_t)(m >> 8);                                 // MEAN_PRECISION (:2899-2989)
            d.variance[s * PST_PUS + t] = (uint16_t)((q - m * m) >> 16);                   // VARIANCE_PRECISION (:2992-3082)
        } else if (t >= 128 && t < 128 + 2 * PST_CHROMA_PUS) {
            const int pl = (t - 128) / PST_CHROMA_PUS, e = (t - 128) % PST_CHROMA_PUS;
            (pl ? d.cr_mean : d.cb_mean)[s * PST_CHROMA_PUS + e] = (uint8_t)(M[2 * PST_PUS + pl * PST_CHROMA_PUS + e] >> 8);
        }
    }
}

// sum over the block of a per-thread value; valid in thread 0.  `red`: PST_THREADS / 64 words of LDS of its own
__device__ __forceinline__ uint64_t pst_block_sum(uint64_t v, uint64_t* red) {
    v = group_sum64<64>(v);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    uint64_t tot = 0;
    if (threadIdx.x == 0)
        for (int i = 0; i < PST_THREADS / 64; i++) tot += red[i];
    return tot;
}

// One (region, plane) histogram.  Luma: every sample of the region of the 1/16 picture, 16 bytes per lane and step (a row's last
// step is the 16 bytes that END at the region's right edge, the bytes already counted skipped; regions narrower than 16 go byte
// by byte).  Chroma: every 4th sample of every 4th row, four loads in flight per lane.
__device__ __forceinline__ void pst_hist(const PicStatsDev& d, uint32_t h, uint32_t pic, uint32_t* lds) {
    uint32_t* hist = lds;                                             // [256]
    uint64_t* red = reinterpret_cast<uint64_t*>(lds + 256);           // [4]
    const uint32_t t = threadIdx.x;
    const uint32_t region = h / 3, pl = h % 3;
    const uint32_t ri = region / d.rh, rj = region % d.rh;            // picture_histogram[region in width][region in height]
    hist[t] = 0;
    __syncthreads();
    uint32_t sum = 0;
    uint32_t area;                                                    // the divisor's area, as the reference forms it
    if (pl == 0) {
        const uint32_t pw = d.width >> 2, ph = d.height >> 2;
        const uint32_t rw0 = pw / d.rw, rh0 = ph / d.rh;
        const uint32_t W = rw0 + (ri == d.rw - 1 ? pw - d.rw * rw0 : 0), H = rh0 + (rj == d.rh - 1 ? ph - d.rh * rh0 : 0);
        area = W * H;
        const uint8_t* base = d.plane[3] + pic * d.pitch[3] + (size_t)(d.oy16 + rj * rh0) * d.stride[3] + d.ox16 + ri * rw0;
        if (W >= 16) {
            const uint32_t nch = (W + 15) >> 4, n = nch * H;
            for (uint32_t i = t; i < n; i += PST_THREADS) {
                const uint32_t y = i / nch, c = i - y * nch;
                uint32_t x0 = c * 16, skip = 0;
                if (x0 + 16 > W) { skip = x0 + 16 - W; x0 = W - 16; }
                uint32_t v[4];
                cfl_ld<16>(v, base + (size_t)y * d.stride[3] + x0);
#pragma unroll
                for (uint32_t k = 0; k < 16; k++) {
                    const uint32_t b = (v[k >> 2] >> (8 * (k & 3))) & 0xffu;
                    if (k >= skip) { atomicAdd(&hist[b], 1u); sum += b; }
                }
            }
        } else {
            const uint32_t n = W * H;
            for (uint32_t i = t; i < n; i += PST_THREADS) {
                const uint32_t y = i / W, x = i - y * W;
                const uint32_t b = base[(size_t)y * d.stride[3] + x];
                atomicAdd(&hist[b], 1u); sum += b;
            }
        }
    } else {
        const uint32_t rw0 = d.width / d.rw, rh0 = d.height / d.rh;
        const uint32_t LW = rw0 + (ri == d.rw - 1 ? d.width - d.rw * rw0 : 0), LH = rh0 + (rj == d.rh - 1 ? d.height - d.rh * rh0 : 0);
        area = LW * LH;
        const uint32_t nx = ((LW >> 1) + 3) >> 2, ny = ((LH >> 1) + 3) >> 2, n = nx * ny;
        const uint8_t* base = d.plane[pl] + pic * d.pitch[pl] + (size_t)((d.oy + rj * rh0) >> 1) * d.stride[pl] + ((d.ox + ri * rw0) >> 1);
        for (uint32_t i0 = t; i0 < n; i0 += 4 * PST_THREADS) {
            uint32_t b[4];
#pragma unroll
            for (uint32_t k = 0; k < 4; k++) {
                const uint32_t i = i0 + k * PST_THREADS;
                const uint32_t y = i / nx, x = i - y * nx;
                b[k] = i < n ? base[(size_t)(4 * y) * d.stride[pl] + 4 * x] : 0x100u;
            }
#pragma unroll
            for (uint32_t k = 0; k < 4; k++)
                if (b[k] < 0x100u) { atomicAdd(&hist[b[k]], 1u); sum += b[k]; }
        }
    }
    const uint64_t tot = pst_block_sum(sum, red);          // (its barrier also ends the histogram's adds)
    const size_t hr = (size_t)pic * (d.nhist / 3) + region;
    d.histogram[(hr * 3 + pl) * 256 + t] = (1u + hist[t]) << 4;
    if (t == 0) {
        uint64_t avg;
        if (pl == 0) avg = (tot + (area >> 1)) / area;
        else avg = ((tot << 4) + (area >> 3)) / (area >> 2);
        d.avg_region[hr * 3 + pl] = (uint8_t)avg;
    }
}

__global__ __launch_bounds__(PST_THREADS) void picture_stats_kernel(const PicStatsDev d) {
    __shared__ __attribute__((aligned(16))) uint32_t lds[PST_SBS * PST_SB_WORDS];
    static_assert(256 + 8 <= PST_SBS * PST_SB_WORDS, "the histogram and its reduction fit the SBs' LDS");
    if (blockIdx.x < d.nhist) pst_hist(d, blockIdx.x, blockIdx.y, lds);
    else pst_sbs(d, (blockIdx.x - d.nhist) * PST_SBS, blockIdx.y, lds);
}

// per picture: pic_avg_variance and average_intensity[3] from what picture_stats_kernel wrote
__global__ __launch_bounds__(PST_THREADS) void picture_stats_sum_kernel(const PicStatsDev d) {
    __shared__ uint64_t red[4][PST_THREADS / 64];
    const uint32_t t = threadIdx.x, pic = blockIdx.x, nreg = d.nhist / 3;
    uint64_t var = 0, sum[3] = {0, 0, 0};
    for (uint32_t s = t; s < d.nsb; s += PST_THREADS) var += d.variance[((size_t)pic * d.nsb + s) * PST_PUS];
    for (uint32_t r = 0; r < nreg; r++)
#pragma unroll
        for (uint32_t p = 0; p < 3; p++) sum[p] += (uint64_t)t * ((d.histogram[(((size_t)pic * nreg + r) * 3 + p) * 256 + t] >> 4) - 1u);
    const uint64_t tv = pst_block_sum(var, red[0]);
    const uint64_t ty = pst_block_sum(sum[0], red[1]), tb = pst_block_sum(sum[1], red[2]), tr = pst_block_sum(sum[2], red[3]);
    if (t == 0) {
        const uint64_t wh = (uint64_t)d.width * d.height;
        d.pic_avg_variance[pic] = (uint16_t)(tv / d.nsb);
        d.avg[pic * 3 + 0] = (uint8_t)(((ty << 4) + (wh >> 1)) / wh);
        d.avg[pic * 3 + 1] = (uint8_t)(((tb << 4) + (wh >> 3)) / (wh >> 2));
        d.avg[pic * 3 + 2] = (uint8_t)(((tr << 4) + (wh >> 3)) / (wh >> 2));
    }
}

}  // namespace svtdev

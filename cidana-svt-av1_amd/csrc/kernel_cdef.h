// kernel_cdef.h — the CDEF strength search (cdef_seg_search, EbCdefProcess.c:89-258; 16-bit :260) and the CDEF apply
// (av1_cdef_frame, EbCdef.c:471; 16-bit :801) for whole 4:2:0 pictures.
//
// One workgroup of four waves per (64x64 filter block, luma | both chroma planes, chunk of the strength window).  The workgroup
// builds the filter block's list of non-skipped 8x8 blocks (sb_compute_cdef_list), stages the luma tile with a 2-sample border in
// LDS as 16-bit samples (CDEF_VERY_LARGE outside the picture; the filter reads at most +-2 rows / columns), finds direction and
// variance of every 8x8 block (cdef_find_dir_c, EbCdef.c:129: each wave two of the eight directions, a lane per block), and the
// chroma workgroup then replaces the luma tile by the Cb and Cr tiles.  In the main loop a wave takes one listed 8x8 luma block
// (a lane per sample, so direction, variance and the adjusted strength are wave-uniform) or four 4x4 chroma blocks (16 lanes
// each).  A lane keeps its centre sample, its source sample and the differences to its twelve tap neighbours in registers; the taps
// are re-read from LDS only when the direction in force changes (dir -> 0 when the primary strength is 0), so the loop over the
// strengths is register-only: twelve `constrain`, the rounding, the clamp to the neighbourhood's min / max
// (cdef_filter_block_c, EbCdef.c:204-255), then the distortion sums reduced over the wave.  Lane k of the wave keeps the sums
// of the chunk's k-th strength; after the loop all lanes evaluate dist_8x8_16bit_c's binary64 expression (EbCdef.c:1305-1331) at
// once, one strength each.  Filtered samples never leave the registers in the search; the apply stores them.
#pragma once
#include "dev_common.h"

namespace svtdev {

constexpr int CDEF_LARGE = 30000;                 // CDEF_VERY_LARGE
constexpr int CDEF_TS_Y = 72, CDEF_TS_C = 40;     // LDS row pitch of the luma tile (68 used) and of a chroma tile (36 used)
constexpr int CDEF_TILE_C = 36 * CDEF_TS_C;       // samples of one chroma tile
constexpr int CDEF_THREADS = 256;

struct CdefDev {
    const void* rec[3];                 // filter input (deblocked reconstruction)
    const void* src[3];                 // source picture (search)
    void* dst[3];                       // filtered picture (apply)
    unsigned long long rec_pitch[3], src_pitch[3], dst_pitch[3];        // samples between the pictures of a stack
    uint32_t rec_stride[3], src_stride[3], dst_stride[3];               // samples
    const uint8_t* skip;                // one byte per 8x8 luma block
    unsigned long long skip_pitch;
    uint32_t skip_stride;
    uint32_t width, height, nhfb, nvfb;
    int cs;                             // coeff_shift = bit depth - 8
    int damping;                        // 3 + (base_qindex >> 6), before cdef_filter_fb's own adjustments
    int start_gi, end_gi, gpc;          // strength window, strengths per chunk (blockIdx.z)
    unsigned long long* mse;            // [npics][2][nfb][64]
    int* count;                         // [npics][nfb]
    const int8_t* ystr;                 // [npics][nfb] apply: luma / chroma strength, -1 = leave alone
    const int8_t* uvstr;
};

// cdef_directions (EbCdef.c:111) as (dy, dx) of the two taps
__constant__ int8_t kCdefDirs[8][2][2] = {{{-1, 1}, {-2, 2}}, {{0, 1}, {-1, 2}}, {{0, 1}, {0, 2}}, {{0, 1}, {1, 2}},
                                          {{1, 1}, {2, 2}},   {{1, 0}, {2, 1}},  {{1, 0}, {2, 0}}, {{1, 0}, {2, -1}}};

// the line of direction D that sample (i, j) of an 8x8 block lies on (cdef_find_dir_c's partial[D][..] index)
template <int D>
__device__ __forceinline__ constexpr int cdef_line(int i, int j) {
    return D == 0 ? i + j : D == 1 ? i + j / 2 : D == 2 ? i : D == 3 ? 3 + i - j / 2 : D == 4 ? 7 + i - j : D == 5 ? 3 - i / 2 + j : D == 6 ? j : i / 2 + j;
}

// cost[D] of cdef_find_dir_c for the 8x8 block at blk (LDS, row pitch CDEF_TS_Y)
template <int D>
__device__ __forceinline__ int cdef_dir_cost(const uint16_t* blk, int cs) {
    int p[15];
#pragma unroll
    for (int k = 0; k < 15; k++) p[k] = 0;
#pragma unroll
    for (int i = 0; i < 8; i++)
#pragma unroll
        for (int j = 0; j < 8; j++) p[cdef_line<D>(i, j)] += (int)(blk[i * CDEF_TS_Y + j] >> cs) - 128;
    // div_table[n] = 840 / n
    int cost = 0;
    if (D == 2 || D == 6) {
#pragma unroll
        for (int i = 0; i < 8; i++) cost += p[i] * p[i];
        cost *= 105;
    } else if (D == 0 || D == 4) {
#pragma unroll
        for (int i = 0; i < 7; i++) cost += (p[i] * p[i] + p[14 - i] * p[14 - i]) * (840 / (i + 1));
        cost += p[7] * p[7] * 105;
    } else {
#pragma unroll
        for (int j = 0; j < 5; j++) cost += p[3 + j] * p[3 + j];
        cost *= 105;
#pragma unroll
        for (int j = 0; j < 3; j++) cost += (p[j] * p[j] + p[10 - j] * p[10 - j]) * (840 / (2 * j + 2));
    }
    return cost;
}

__device__ __forceinline__ int cdef_msb(int v) { return 31 - __clz(v); }

// adjust_strength (EbCdef.c:267)
__device__ __forceinline__ int cdef_adjust_strength(int strength, int var) {
    const int i = (var >> 6) ? min(cdef_msb(var >> 6), 12) : 0;
    return var ? (strength * (4 + i) + 8) >> 4 : 0;
}

// constrain (EbCdef.c:101) as a clamp of the difference to +-max(0, threshold - (|diff| >> shift)); threshold 0 gives 0
__device__ __forceinline__ int cdef_constrain(int diff, int threshold, int shift) {
    const int m = max(0, threshold - (abs(diff) >> shift));
    return min(max(diff, -m), m);
}

// One lane's sample: centre, differences to the twelve taps, min / max of the neighbourhood (CDEF_VERY_LARGE left out of the max).
struct CdefTaps {
    int x, mn, mx;
    int d[12];          // 0..3 primary (tap 0 +, tap 0 -, tap 1 +, tap 1 -), 4..7 secondary tap 0, 8..11 secondary tap 1
};

__device__ __forceinline__ void cdef_load_taps(CdefTaps& t, const uint16_t* c, int ts, int dir) {
    const int x = t.x;
    int mn = x, mx = x;
#pragma unroll
    for (int k = 0; k < 2; k++) {
        const int d1 = (dir + 2) & 7, d2 = (dir + 6) & 7;
        const int o0 = kCdefDirs[dir][k][0] * ts + kCdefDirs[dir][k][1];
        const int o1 = kCdefDirs[d1][k][0] * ts + kCdefDirs[d1][k][1];
        const int o2 = kCdefDirs[d2][k][0] * ts + kCdefDirs[d2][k][1];
        const int v[6] = {c[o0], c[-o0], c[o1], c[-o1], c[o2], c[-o2]};
#pragma unroll
        for (int q = 0; q < 6; q++) {
            mn = min(mn, v[q]);
            mx = v[q] != CDEF_LARGE ? max(mx, v[q]) : mx;
        }
        t.d[2 * k] = v[0] - x;
        t.d[2 * k + 1] = v[1] - x;
#pragma unroll
        for (int q = 0; q < 4; q++) t.d[4 + 4 * k + q] = v[2 + q] - x;
    }
    t.mn = mn;
    t.mx = mx;
}

// cdef_filter_block_c for one sample; pri / sec are the strengths handed to it (luma primary already adjusted)
__device__ __forceinline__ int cdef_filter_px(const CdefTaps& t, int pri, int sec, int damping, int cs) {
    const int psh = pri ? max(0, damping - cdef_msb(pri)) : 0;
    const int ssh = sec ? max(0, damping - cdef_msb(sec)) : 0;
    const int odd = (pri >> cs) & 1;
    const int pt0 = odd ? 3 : 4, pt1 = odd ? 3 : 2;
    int sum = pt0 * (cdef_constrain(t.d[0], pri, psh) + cdef_constrain(t.d[1], pri, psh)) +
              pt1 * (cdef_constrain(t.d[2], pri, psh) + cdef_constrain(t.d[3], pri, psh));
    int s0 = 0, s1 = 0;
#pragma unroll
    for (int q = 0; q < 4; q++) {
        s0 += cdef_constrain(t.d[4 + q], sec, ssh);
        s1 += cdef_constrain(t.d[8 + q], sec, ssh);
    }
    sum += 2 * s0 + s1;
    const int y = t.x + ((8 + sum - (sum < 0)) >> 4);
    return min(max(y, t.mn), t.mx);
}

// dist_8x8_16bit_c's closing expression (EbCdef.c:1324-1330): every operation its own correctly rounded binary64 instruction, in
// the reference's order, none contracted.
__device__ __forceinline__ unsigned long long cdef_dist_8x8(unsigned long long sum_s, unsigned long long sum_d, unsigned long long sum_s2,
                                                            unsigned long long sum_d2, unsigned long long sum_sd, int cs) {
    const unsigned long long svar = sum_s2 - ((sum_s * sum_s + 32) >> 6);
    const unsigned long long dvar = sum_d2 - ((sum_d * sum_d + 32) >> 6);
    const double a = __dmul_rn((double)(sum_d2 + sum_s2 - 2 * sum_sd), .5);
    const double b = (double)(svar + dvar + (unsigned long long)(400 << 2 * cs));
    const double den = __dsqrt_rn(__dadd_rn((double)(20000 << 4 * cs), __dmul_rn((double)svar, (double)dvar)));
    return (unsigned long long)floor(__dadd_rn(.5, __ddiv_rn(__dmul_rn(a, b), den)));
}

// sum over the wave, valid in every lane
__device__ __forceinline__ uint32_t cdef_wave_sum(uint32_t v) { return group_sum_rt(v, 64); }

template <typename PixT, bool APPLY>
__global__ __launch_bounds__(CDEF_THREADS) void cdef_kernel(const CdefDev P) {
    __shared__ uint16_t tile[68 * CDEF_TS_Y];
    __shared__ int s_cost[8][64];
    __shared__ int s_var[64];
    __shared__ unsigned long long s_acc[2][64];
    __shared__ uint8_t s_dir[64], s_list[64], s_listed[64];
    __shared__ int s_count;

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const uint32_t nfb = P.nhfb * P.nvfb;
    const uint32_t pic = blockIdx.x / nfb, fb = blockIdx.x - pic * nfb;
    const int fbr = (int)(fb / P.nhfb), fbc = (int)(fb - (uint32_t)fbr * P.nhfb);
    const bool chroma = blockIdx.y != 0;
    const int cs = P.cs;
    const int W8 = (int)P.width >> 3, H8 = (int)P.height >> 3;
    const int nhb = min(8, W8 - fbc * 8), nvb = min(8, H8 - fbr * 8);
    const int g0 = P.start_gi + (int)blockIdx.z * P.gpc, g1 = min(P.end_gi, g0 + P.gpc);

    // sb_compute_cdef_list: the non-skipped 8x8 blocks in raster order
    if (wave == 0) {
        const int by = lane >> 3, bx = lane & 7;
        bool listed = false;
        if (by < nvb && bx < nhb)
            listed = P.skip[pic * P.skip_pitch + (size_t)(fbr * 8 + by) * P.skip_stride + (size_t)(fbc * 8 + bx)] == 0;
        const unsigned long long m = __ballot(listed);
        if (listed) s_list[__popcll(m & ((1ull << lane) - 1))] = (uint8_t)lane;
        s_listed[lane] = listed;
        if (lane == 0) s_count = __popcll(m);
        s_acc[0][lane] = 0;
        s_acc[1][lane] = 0;
    }
    __syncthreads();
    const int count = s_count;
    unsigned long long* mse = APPLY ? nullptr : P.mse + ((size_t)pic * 2 + (chroma ? 1 : 0)) * nfb * 64 + (size_t)fb * 64;
    if (!APPLY) {
        if (blockIdx.z == 0 && tid < 64) {
            if (tid < P.start_gi || tid >= P.end_gi || count == 0) mse[tid] = 0;
            if (tid == 0 && !chroma) P.count[(size_t)pic * nfb + fb] = count;
        }
        if (count == 0) return;
    }

    // the luma tile: rows / columns -2 .. 65 of the filter block
    {
        const PixT* rec = (const PixT*)P.rec[0] + pic * P.rec_pitch[0];
        const int y0 = fbr * 64 - 2, x0 = fbc * 64 - 2;
        for (int i = tid; i < 68 * 68; i += CDEF_THREADS) {
            const int r = i / 68, c = i - r * 68, y = y0 + r, x = x0 + c;
            int v = CDEF_LARGE;
            if (y >= 0 && y < (int)P.height && x >= 0 && x < (int)P.width) v = rec[(size_t)y * P.rec_stride[0] + x];
            tile[r * CDEF_TS_Y + c] = (uint16_t)v;
        }
    }
    __syncthreads();
    // cdef_find_dir: wave w the costs of directions 2w and 2w + 1, a lane per 8x8 block
    {
        const uint16_t* blk = tile + ((lane >> 3) * 8 + 2) * CDEF_TS_Y + (lane & 7) * 8 + 2;
        switch (wave) {
        case 0: s_cost[0][lane] = cdef_dir_cost<0>(blk, cs); s_cost[1][lane] = cdef_dir_cost<1>(blk, cs); break;
        case 1: s_cost[2][lane] = cdef_dir_cost<2>(blk, cs); s_cost[3][lane] = cdef_dir_cost<3>(blk, cs); break;
        case 2: s_cost[4][lane] = cdef_dir_cost<4>(blk, cs); s_cost[5][lane] = cdef_dir_cost<5>(blk, cs); break;
        default: s_cost[6][lane] = cdef_dir_cost<6>(blk, cs); s_cost[7][lane] = cdef_dir_cost<7>(blk, cs); break;
        }
    }
    __syncthreads();
    if (tid < 64) {
        int best = 0, bd = 0;
#pragma unroll
        for (int d = 0; d < 8; d++) {
            const int c = s_cost[d][tid];
            if (c > best) { best = c; bd = d; }
        }
        s_dir[tid] = (uint8_t)bd;
        s_var[tid] = (best - s_cost[(bd + 4) & 7][tid]) >> 10;
    }
    if (chroma) {
        // every wave has read the luma tile (barrier above): the Cb and Cr tiles, rows / columns -2 .. 33, take its place
        const int y0 = fbr * 32 - 2, x0 = fbc * 32 - 2, hc = (int)P.height >> 1, wc = (int)P.width >> 1;
        for (int i = tid; i < 2 * 36 * 36; i += CDEF_THREADS) {
            const int pl = i >= 36 * 36, k = i - pl * 36 * 36;
            const int r = k / 36, c = k - r * 36, y = y0 + r, x = x0 + c;
            int v = CDEF_LARGE;
            if (y >= 0 && y < hc && x >= 0 && x < wc) v = ((const PixT*)P.rec[1 + pl] + pic * P.rec_pitch[1 + pl])[(size_t)y * P.rec_stride[1 + pl] + x];
            tile[pl * CDEF_TILE_C + r * CDEF_TS_C + c] = (uint16_t)v;
        }
    }
    __syncthreads();

    const int damping = P.damping + cs - (chroma ? 1 : 0);
    const int ts = chroma ? CDEF_TS_C : CDEF_TS_Y;

    if (APPLY) {
        const int ys = P.ystr[(size_t)pic * nfb + fb], us = P.uvstr[(size_t)pic * nfb + fb];
        const bool filt = ys >= 0 && us >= 0 && (ys | us) != 0 && count > 0;           // EbCdef.c:600-604
        const int st = (chroma ? us : ys) & 63;
        int sec = st & 3;
        sec += sec == 3;
        const int t = (st >> 2) << cs;
        sec <<= cs;
        const int nblk = nvb * nhb;
        const int nitems = chroma ? (2 * nblk + 3) >> 2 : nblk;
        for (int item = wave; item < nitems; item += CDEF_THREADS / 64) {
            int q = chroma ? item * 4 + (lane >> 4) : item;
            const bool active = !chroma || q < 2 * nblk;
            q = active ? q : 0;
            const int pl = chroma && q >= nblk, b = q - pl * nblk;
            const int by = b / nhb, bx = b - by * nhb, blk = by * 8 + bx;
            const int py = chroma ? by * 4 + ((lane >> 2) & 3) : by * 8 + (lane >> 3);
            const int px = chroma ? bx * 4 + (lane & 3) : bx * 8 + (lane & 7);
            const uint16_t* c = tile + pl * CDEF_TILE_C + (py + 2) * ts + px + 2;
            CdefTaps tp;
            tp.x = c[0];
            int y = tp.x;
            if (filt && s_listed[blk]) {
                cdef_load_taps(tp, c, ts, t ? s_dir[blk] : 0);
                y = cdef_filter_px(tp, chroma ? t : cdef_adjust_strength(t, s_var[blk]), sec, damping, cs);
            }
            if (active) {
                const int plane = chroma ? 1 + pl : 0, sh = chroma ? 5 : 6;
                PixT* dst = (PixT*)P.dst[plane] + pic * P.dst_pitch[plane];
                dst[(size_t)((fbr << sh) + py) * P.dst_stride[plane] + (size_t)((fbc << sh) + px)] = (PixT)y;
            }
        }
        return;
    }

    const int ngi = g1 - g0;
    const int nitems = chroma ? (2 * count + 3) >> 2 : count;
    unsigned long long acc0 = 0, acc1 = 0;          // lane k: the chunk's k-th strength (luma: the block distortions; chroma: Cb, Cr)
    for (int item = wave; item < nitems; item += CDEF_THREADS / 64) {
        int q = chroma ? item * 4 + (lane >> 4) : item;
        const bool active = !chroma || q < 2 * count;
        q = active ? q : 0;
        const int pl = chroma && q >= count;
        const int blk = s_list[q - pl * count], by = blk >> 3, bx = blk & 7;
        const int py = chroma ? by * 4 + ((lane >> 2) & 3) : by * 8 + (lane >> 3);
        const int px = chroma ? bx * 4 + (lane & 3) : bx * 8 + (lane & 7);
        const uint16_t* c = tile + pl * CDEF_TILE_C + (py + 2) * ts + px + 2;
        const int plane = chroma ? 1 + pl : 0, sh = chroma ? 5 : 6;
        const int s = ((const PixT*)P.src[plane] + pic * P.src_pitch[plane])[(size_t)((fbr << sh) + py) * P.src_stride[plane] + (size_t)((fbc << sh) + px)];
        const int dir = s_dir[blk], var = s_var[blk];
        CdefTaps tp;
        tp.x = c[0];
        uint32_t sum_s = 0, sum_s2 = 0;
        if (!chroma) {
            sum_s = cdef_wave_sum((uint32_t)s);
            sum_s2 = cdef_wave_sum((uint32_t)(s * s));
        }
        uint32_t k0 = 0, k1 = 0, k2 = 0;            // what lane (gi - g0) keeps of its strength
        int zero_pri = -1;
        for (int gi = g0; gi < g1; gi++) {
            const int t = (gi >> 2) << cs;
            int sec = gi & 3;
            sec += sec == 3;
            sec <<= cs;
            if ((t == 0) != zero_pri) {
                zero_pri = t == 0;
                cdef_load_taps(tp, c, ts, t ? dir : 0);
            }
            const int y = cdef_filter_px(tp, chroma ? t : cdef_adjust_strength(t, var), sec, damping, cs);
            const bool mine = lane == gi - g0;
            if (!chroma) {
                const uint32_t sd = cdef_wave_sum((uint32_t)y), sd2 = cdef_wave_sum((uint32_t)(y * y)), ssd = cdef_wave_sum((uint32_t)(y * s));
                k0 = mine ? sd : k0;
                k1 = mine ? sd2 : k1;
                k2 = mine ? ssd : k2;
            } else {
                const int e = y - s;
                const uint32_t e2 = active ? (uint32_t)(e * e) : 0u;
                const uint32_t cb = cdef_wave_sum(pl ? 0u : e2), cr = cdef_wave_sum(pl ? e2 : 0u);
                k0 = mine ? cb : k0;
                k1 = mine ? cr : k1;
            }
        }
        if (!chroma) {
            if (lane < ngi) acc0 += cdef_dist_8x8(sum_s, k0, sum_s2, k1, k2, cs);
        } else {
            acc0 += k0;
            acc1 += k1;
        }
    }
    if (lane < ngi) {
        atomicAdd(&s_acc[0][lane], acc0);
        if (chroma) atomicAdd(&s_acc[1][lane], acc1);
    }
    __syncthreads();
    if (tid < ngi) mse[g0 + tid] = (s_acc[0][tid] >> 2 * cs) + (s_acc[1][tid] >> 2 * cs);
}

}  // namespace svtdev

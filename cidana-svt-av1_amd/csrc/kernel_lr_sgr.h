// kernel_lr_sgr.h — the self-guided parameter search of loop restoration (search_selfguided_restoration, EbRestorationPick.c:605-661):
// the kernels of svt_hip_lr_sgr_stats_frame, svt_hip_lr_sgr_walk_frame and svt_hip_lr_sgr_search_frame, on kernel_lr.h's staging and
// self-guided passes.  The scratch layout and the checks are lr_sgr_plan.h's, the projection and the walk lr_sgr_solve.h's.
//
// Filter once, score many times.  The statistics kernel walks the picture in the tiles of apply (one stripe by 64 columns, so a tile lies
// in one unit and the fast pass's row parity is the tile's own: stripe, unit and processing-unit starts are all even).  It stages a tile
// once under the search's halo rule - every row a row of the CDEF picture, clamped; apply_sgr runs on the extended CDEF frame and knows
// no stripes - and per ep filters it, adds f1 f1, f2 f2, f1 f2, f1 s, f2 s into 64-bit sums (exact in any order: integers, totals below
// 2^53) and leaves f1, f2 as an int16 pair per sample, src - dat as int16 once, in the unit-contiguous scratch.  The walk kernel then
// needs no picture: one workgroup per (picture, unit, ep) streams the unit's pairs once per evaluation and all its threads follow the
// same walk, because each evaluation's total is broadcast through LDS.  No workgroup waits for another.
#pragma once
#include "kernel_lr.h"
#include "lr_sgr_plan.h"

namespace svtdev {

constexpr int LR_SGR_NT = svthost::LR_SGR_WALK_THREADS;

struct LrSgrDev {
    int ep_lo, ep_hi;
    unsigned long long S;                     // samples of a picture
    short* sd; uint32_t* f;                   // the scratch's two sample arrays
    long long* stats;                         // [pic][unit][16][5]
    const short* start;                       // [pic][unit][16][2], or NULL: solved here from stats
    svthost::LrSgrWalkRec* walk;              // [pic][unit][16]
    svthost::LrSgrBestRec* best;              // [pic][unit]
    uint32_t* cand; const long long* sse;     // the search's own try: svt_hip_lr_cand as nine words, and its errors
};

__device__ __forceinline__ size_t lr_sgr_unit_base(const LrDev& F, int plane, int hs, int vs, int ve) {
    return (size_t)svthost::lr_sgr_plane_offset((uint32_t)F.pl[0].w, (uint32_t)F.pl[0].h, plane) + (size_t)svthost::lr_sgr_unit_offset(F.pl[plane].w, hs, vs, ve);
}

// the statistics' entries of the range: blockIdx.x * LR_NT + threadIdx.x = (pic * units_per_pic + unit) * n * 5 + (ep - ep_lo) * 5 + j
__global__ __launch_bounds__(LR_NT) void lr_sgr_zero_kernel(LrDev F, LrSgrDev G) {
    const size_t i = (size_t)blockIdx.x * LR_NT + threadIdx.x, per = (size_t)(G.ep_hi - G.ep_lo) * svthost::LR_SGR_STATS;
    if (i >= (size_t)F.npics * F.units_per_pic * per) return;
    G.stats[(i / per) * (svthost::LR_SGR_PARAMS * svthost::LR_SGR_STATS) + (size_t)G.ep_lo * svthost::LR_SGR_STATS + i % per] = 0;
}

// blockIdx.x = tile (tile column + stripe * ntx), .y = plane, .z = picture, as lr_apply_kernel
template <typename T>
__global__ __launch_bounds__(LR_NT) void lr_sgr_stats_kernel(LrDev F, LrSgrDev G) {
    __shared__ LrLds<T> L;
    __shared__ unsigned long long red[LR_NT / 64][svthost::LR_SGR_STATS];
    const int plane = blockIdx.y;
    const LrPlane& P = F.pl[plane];
    const uint32_t pic = blockIdx.z;
    const int tx = (int)(blockIdx.x % (uint32_t)P.ntx), s = (int)(blockIdx.x / (uint32_t)P.ntx);
    if (s >= P.nstripes) return;
    const int off = svthost::lr_stripe_off(P.ss);
    const int x0 = tx * P.tw, y0 = svthost::lr_stripe_start(s, P.ss), y1 = svthost::lr_stripe_end(s, P.ss, P.h), rows = y1 - y0;
    const int uj = svthost::lr_unit_of(x0, P.nh, P.us, 0), ui = svthost::lr_unit_of(y0, P.nv, P.us, off);
    const int hs = svthost::lr_unit_start(uj, P.us, 0), he = svthost::lr_unit_end(uj, P.nh, P.us, 0, P.w);
    const int vs = svthost::lr_unit_start(ui, P.us, off), ve = svthost::lr_unit_end(ui, P.nv, P.us, off, P.h);
    lr_stage<T, true>(F, L, plane, pic, x0, P.tw, y0, y1);
    __syncthreads();
    const int col = threadIdx.x % P.tw, row0 = threadIdx.x / P.tw, rstep = LR_NT / P.tw, uw = he - hs, nep = G.ep_hi - G.ep_lo;
    const bool in_x = x0 + col < he;
    // this thread's first sample inside the picture's unit-contiguous block; one row further down is uw further on
    const size_t first = lr_sgr_unit_base(F, plane, hs, vs, ve) + (size_t)(y0 - vs + row0) * uw + (size_t)(x0 - hs + col);
    const T* src = (const T*)F.src[plane] + pic * F.src_pitch[plane];
    int sd[LR_PER_THREAD];
#pragma unroll
    for (int k = 0; k < LR_PER_THREAD; k++) {
        const int row = row0 + k * rstep;
        sd[k] = 0;
        if (row < rows && in_x) {
            sd[k] = (int)src[(size_t)(y0 + row) * F.src_stride[plane] + x0 + col] - (int)L.in[(row + LR_B) * LR_IN_P + col + LR_B];
            G.sd[(size_t)pic * G.S + first + (size_t)k * rstep * uw] = (short)sd[k];
        }
    }
    for (int ep = G.ep_lo; ep < G.ep_hi; ep++) {
        const int r0 = kSgrR[ep][0], r1 = kSgrR[ep][1];
        int flt0[LR_PER_THREAD];
        if (r0 > 0) lr_sgr_pass0<T>(L, ep, F.bd, P.tw, rows, flt0);
        if (r1 > 0) lr_sgr_pass1_ab<T>(L, ep, F.bd, P.tw, rows);
        long long acc[svthost::LR_SGR_STATS] = {0, 0, 0, 0, 0};
        uint32_t* fout = G.f + ((size_t)pic * nep + (size_t)(ep - G.ep_lo)) * G.S + first;
#pragma unroll
        for (int k = 0; k < LR_PER_THREAD; k++) {
            const int row = row0 + k * rstep;
            if (row < rows && in_x) {
                const int px = (int)L.in[(row + LR_B) * LR_IN_P + col + LR_B], u = px << 4, sv = sd[k] * 16;
                const int f1 = r0 > 0 ? flt0[k] - u : 0, f2 = r1 > 0 ? lr_sgr_flt1<T>(L, row, col, px) - u : 0;
                acc[0] += (long long)(f1 * f1); acc[1] += (long long)(f2 * f2); acc[2] += (long long)(f1 * f2);
                acc[3] += (long long)(f1 * sv); acc[4] += (long long)(f2 * sv);
                fout[(size_t)k * rstep * uw] = ((uint32_t)f1 & 0xffffu) | ((uint32_t)f2 << 16);
            }
        }
#pragma unroll
        for (int j = 0; j < svthost::LR_SGR_STATS; j++) {
            const unsigned long long v = group_sum64<64>((unsigned long long)acc[j]);
            if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6][j] = v;
        }
        __syncthreads();                                                // red; and the planes are rewritten by the next ep
        if (threadIdx.x < svthost::LR_SGR_STATS) {
            unsigned long long tot = 0;
            for (int i = 0; i < LR_NT / 64; i++) tot += red[i][threadIdx.x];
            const size_t pu = (size_t)pic * F.units_per_pic + P.unit0 + (uint32_t)(ui * P.nh + uj);
            atomicAdd((unsigned long long*)G.stats + (pu * svthost::LR_SGR_PARAMS + (size_t)ep) * svthost::LR_SGR_STATS + threadIdx.x, tot);
        }
        // the next ep writes red only after a barrier of its passes (one radius is always above 0)
    }
}

// finer_search_pixel_proj_error per (picture, unit, ep): blockIdx.x = (pic * units_per_pic + unit) * n + (ep - ep_lo)
__global__ __launch_bounds__(LR_SGR_NT) void lr_sgr_walk_kernel(LrDev F, LrSgrDev G) {
    __shared__ unsigned long long red[LR_SGR_NT / 64];
    const uint32_t nep = (uint32_t)(G.ep_hi - G.ep_lo), pu = blockIdx.x / nep, e = blockIdx.x % nep;
    const uint32_t pic = pu / F.units_per_pic, u = pu % F.units_per_pic;
    const int ep = G.ep_lo + (int)e;
    const LrUnitRect r = lr_unit_rect(F, u);
    const uint32_t npix = (uint32_t)((r.he - r.hs) * (r.ve - r.vs));
    const size_t base = lr_sgr_unit_base(F, r.plane, r.hs, r.vs, r.ve);
    const uint2* sd = (const uint2*)(G.sd + (size_t)pic * G.S + base);                     // four samples each: a unit starts on a
    const uint4* f = (const uint4*)(G.f + ((size_t)pic * nep + e) * G.S + base);          // multiple of four and holds one
    const size_t slot = (size_t)pu * svthost::LR_SGR_PARAMS + (size_t)ep;
    int xqd[2];
    if (G.start) {
        xqd[0] = svthost::lr_sgr_r0(ep) ? svthost::lr_sgr_clamp(G.start[slot * 2], svthost::lr_sgr_xqd_min(0), svthost::lr_sgr_xqd_max(0)) : 0;
        xqd[1] = svthost::lr_sgr_clamp(G.start[slot * 2 + 1], svthost::lr_sgr_xqd_min(1), svthost::lr_sgr_xqd_max(1));
    } else {
        int64_t st[svthost::LR_SGR_STATS];
        for (int j = 0; j < svthost::LR_SGR_STATS; j++) st[j] = (int64_t)G.stats[slot * svthost::LR_SGR_STATS + j];
        svthost::lr_sgr_solve(st, npix, ep, xqd);
    }
    const auto eval = [&](int xq0, int xq1) -> int64_t {
        unsigned long long acc = 0;
        for (uint32_t i = threadIdx.x; i < npix / 4; i += LR_SGR_NT) {
            const uint4 fv = f[i];
            const uint2 sv = sd[i];
            const uint32_t fw[4] = {fv.x, fv.y, fv.z, fv.w};
            const int sw[4] = {(int)(short)(sv.x & 0xffffu), (int)(short)(sv.x >> 16), (int)(short)(sv.y & 0xffffu), (int)(short)(sv.y >> 16)};
            uint32_t part = 0;                                          // four terms below 2^30 each: e stays below 2^15 (DESIGN)
#pragma unroll
            for (int k = 0; k < 4; k++) part += svthost::lr_sgr_sample_err(xq0, xq1, (int)(short)(fw[k] & 0xffffu), (int)(short)(fw[k] >> 16), sw[k]);
            acc += part;
        }
        acc = group_sum64<64>(acc);
        if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = acc;
        __syncthreads();
        unsigned long long tot = 0;
#pragma unroll
        for (int i = 0; i < LR_SGR_NT / 64; i++) tot += red[i];
        __syncthreads();                                                // red is rewritten by the next evaluation
        return (int64_t)tot;
    };
    const int start[2] = {xqd[0], xqd[1]};
    int evals = 0;
    const int64_t err = svthost::lr_sgr_walk(ep, xqd, eval, svthost::LR_SGR_MAX_EVALS, &evals);
    if (threadIdx.x == 0) {
        svthost::LrSgrWalkRec w;
        w.err = err; w.xqd[0] = (int16_t)xqd[0]; w.xqd[1] = (int16_t)xqd[1]; w.evals = evals; w.pad = 0;
        w.start[0] = (int16_t)start[0]; w.start[1] = (int16_t)start[1];
        G.walk[slot] = w;
    }
}

// the first lowest error of the range wins (besterr == -1 || err < besterr); an empty range leaves ep 0, xqd 0, 0.  One thread per
// (picture, unit): the winner into d_best, and the candidate the try kernel measures next
__global__ __launch_bounds__(LR_NT) void lr_sgr_pick_kernel(LrDev F, LrSgrDev G) {
    const size_t pu = (size_t)blockIdx.x * LR_NT + threadIdx.x;
    if (pu >= (size_t)F.npics * F.units_per_pic) return;
    const uint32_t pic = (uint32_t)(pu / F.units_per_pic), u = (uint32_t)(pu % F.units_per_pic);
    const int plane = u >= F.pl[2].unit0 ? 2 : (u >= F.pl[1].unit0 ? 1 : 0);
    svthost::LrSgrBestRec b;
    b.sse = 0; b.proj_err = -1; b.ep = 0; b.xqd[0] = 0; b.xqd[1] = 0;
    for (int ep = G.ep_lo; ep < G.ep_hi; ep++) {
        const svthost::LrSgrWalkRec w = G.walk[pu * svthost::LR_SGR_PARAMS + (size_t)ep];
        if (b.proj_err == -1 || w.err < b.proj_err) { b.proj_err = w.err; b.ep = ep; b.xqd[0] = w.xqd[0]; b.xqd[1] = w.xqd[1]; }
    }
    G.best[pu] = b;
    uint32_t* c = G.cand + pu * 9;
    c[0] = pic; c[1] = (uint32_t)plane; c[2] = u - F.pl[plane].unit0;
    c[3] = 2; c[4] = 0; c[5] = 0; c[6] = 0;                            // svt_hip_lr_unit: self-guided, no taps
    c[7] = ((uint32_t)b.xqd[0] & 0xffffu) | ((uint32_t)b.xqd[1] << 16);
    c[8] = (uint32_t)b.ep;
}

__global__ __launch_bounds__(LR_NT) void lr_sgr_sse_kernel(LrDev F, LrSgrDev G) {
    const size_t pu = (size_t)blockIdx.x * LR_NT + threadIdx.x;
    if (pu < (size_t)F.npics * F.units_per_pic) G.best[pu].sse = G.sse[pu];
}

}  // namespace svtdev

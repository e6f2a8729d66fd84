// lr_sgr_solve.h — the arithmetic of the self-guided parameter search that host and device must do alike, stated once: the tail of
// get_proj_subspace with encode_xq (EbRestorationPick.c:522-577), decode_xq (EbRestoration.c:727-740), one sample of
// av1_{lowbd,highbd}_pixel_proj_error (:226-375) and the walk finer_search_pixel_proj_error (:398-459), templated on "the error of xq".
// No HIP header: g++ compiles it for the host (lr_search.cpp, tests/c/lr_sgr_plan_host.cpp), hipcc for the kernels
// (kernel_lr_sgr.h), where LR_HD is __host__ __device__.
//
// Binary64, contraction off.  The reference forms the five sums in double, every term an integer and every total below 2^53, so an
// int64 total converted to double is the reference's sum.  From there on each operation is one IEEE operation of the reference's
// expression, in its order; H00 * H11 - H01 * H10 fused into one rounding would be another number, so no expression here may be
// contracted.  rint(x * 128) outside int32 gives INT32_MIN, what the reference's compiled conversion (cvttsd2si) leaves; the sums
// after it wrap as the compiled reference's 32-bit additions do.
#pragma once
#include <math.h>
#include <stdint.h>

#if defined(__HIP__)
#define LR_HD __host__ __device__ inline __attribute__((always_inline))
#else
#define LR_HD inline
#endif
#if defined(__GNUC__) && !defined(__clang__)
#define LR_NO_CONTRACT __attribute__((optimize("fp-contract=off")))
#else
#define LR_NO_CONTRACT
#endif

namespace svthost {

constexpr int LR_SGR_PARAMS = 16;                             // SGRPROJ_PARAMS
constexpr int LR_SGR_PRJ = 128;                               // 1 << SGRPROJ_PRJ_BITS
constexpr int LR_SGR_START_STEP = 2;
// The walk's evaluations at the most: the start, then per component at step 2 the moves that fit in its range (both ranges hold 128
// values: 64 moves of 2) with the one that fails in each direction, then at step 1 one trial in each direction.
constexpr int LR_SGR_MAX_EVALS = 1 + 2 * (64 + 2) + 2 * 2;

LR_HD int lr_sgr_r0(int ep) { return ep < 10 || ep >= 14 ? 2 : 0; }      // sgr_params[ep].r[0], r[1] (EbRestoration.c:163-172)
LR_HD int lr_sgr_r1(int ep) { return ep < 14 ? 1 : 0; }
LR_HD int lr_sgr_clamp(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }
LR_HD int lr_sgr_xqd_min(int p) { return p ? -32 : -96; }                // SGRPROJ_PRJ_MIN0 / MIN1, MAX0 / MAX1
LR_HD int lr_sgr_xqd_max(int p) { return p ? 95 : 31; }

// (int32_t)rint(x * 128) as the reference's compiled code yields it
LR_HD LR_NO_CONTRACT int32_t lr_sgr_quantise(double x) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    const double v = rint(x * (double)LR_SGR_PRJ);
    if (!(v >= -2147483648.0 && v <= 2147483647.0)) return INT32_MIN;      // NaN included
    return (int32_t)v;
}

// the tail of get_proj_subspace: stats = {H00, H11, H01, C0, C1} as exact totals -> exq
LR_HD LR_NO_CONTRACT void lr_sgr_project(const int64_t stats[5], uint32_t npix, int ep, int32_t exq[2]) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    const double size = (double)(int32_t)npix;
    const double H00 = (double)stats[0] / size, H11 = (double)stats[1] / size, H01 = (double)stats[2] / size, H10 = H01;
    const double C0 = (double)stats[3] / size, C1 = (double)stats[4] / size;
    exq[0] = 0; exq[1] = 0;
    if (lr_sgr_r0(ep) == 0) {
        const double Det = H11;
        if (Det < 1e-8) return;
        exq[1] = lr_sgr_quantise(C1 / Det);
    } else if (lr_sgr_r1(ep) == 0) {
        const double Det = H00;
        if (Det < 1e-8) return;
        exq[0] = lr_sgr_quantise(C0 / Det);
    } else {
        const double a = H00 * H11, b = H01 * H10, Det = a - b;
        if (Det < 1e-8) return;
        const double n0a = H11 * C0, n0b = H01 * C1, n1a = H00 * C1, n1b = H10 * C0;
        const double x0 = (n0a - n0b) / Det, x1 = (n1a - n1b) / Det;
        exq[0] = lr_sgr_quantise(x0);
        exq[1] = lr_sgr_quantise(x1);
    }
}

// encode_xq (:561-577); the sums wrap as 32-bit additions
LR_HD void lr_sgr_encode_xq(const int32_t xq[2], int ep, int xqd[2]) {
    const auto sub = [](int32_t a, int32_t b) { return (int32_t)((uint32_t)a - (uint32_t)b); };
    if (lr_sgr_r0(ep) == 0) {
        xqd[0] = 0;
        xqd[1] = lr_sgr_clamp(sub(LR_SGR_PRJ, xq[1]), lr_sgr_xqd_min(1), lr_sgr_xqd_max(1));
    } else if (lr_sgr_r1(ep) == 0) {
        xqd[0] = lr_sgr_clamp(xq[0], lr_sgr_xqd_min(0), lr_sgr_xqd_max(0));
        xqd[1] = lr_sgr_clamp(LR_SGR_PRJ - xqd[0], lr_sgr_xqd_min(1), lr_sgr_xqd_max(1));
    } else {
        xqd[0] = lr_sgr_clamp(xq[0], lr_sgr_xqd_min(0), lr_sgr_xqd_max(0));
        xqd[1] = lr_sgr_clamp(sub(LR_SGR_PRJ - xqd[0], xq[1]), lr_sgr_xqd_min(1), lr_sgr_xqd_max(1));
    }
}

LR_HD void lr_sgr_solve(const int64_t stats[5], uint32_t npix, int ep, int xqd[2]) {
    int32_t exq[2];
    lr_sgr_project(stats, npix, ep, exq);
    lr_sgr_encode_xq(exq, ep, xqd);
}

// decode_xq
LR_HD void lr_sgr_decode_xq(const int xqd[2], int ep, int xq[2]) {
    if (lr_sgr_r0(ep) == 0) { xq[0] = 0; xq[1] = LR_SGR_PRJ - xqd[1]; }
    else if (lr_sgr_r1(ep) == 0) { xq[0] = xqd[0]; xq[1] = 0; }
    else { xq[0] = xqd[0]; xq[1] = LR_SGR_PRJ - xq[0] - xqd[1]; }
}

// one sample of the projection error: f1 = flt0 - u, f2 = flt1 - u (0 for a radius of 0), sd = src - dat.  No clip, no 16-bit cast.
LR_HD uint32_t lr_sgr_sample_err(int xq0, int xq1, int f1, int f2, int sd) {
    const int e = ((xq0 * f1 + xq1 * f2 + (1 << 10)) >> 11) - sd;
    return (uint32_t)(e * e);
}

// finer_search_pixel_proj_error with start_step 2.  eval(xq0, xq1) -> the error (int64) of the decoded pair; every caller of one walk
// must see the same values, so that all take the same path.  xqd: the start in, the result out.  Returns the result's error; *evals
// counts the evaluations, which never exceed max_evals (the walk stops where the next one would).
template <class Eval>
LR_HD int64_t lr_sgr_walk(int ep, int xqd[2], Eval&& eval, int max_evals, int* evals) {
    int n = 0, xq[2];
    lr_sgr_decode_xq(xqd, ep, xq);
    int64_t err = eval(xq[0], xq[1]);
    n++;
    bool out = false;
    for (int s = LR_SGR_START_STEP; s >= 1 && !out; s >>= 1) {
        for (int p = 0; p < 2 && !out; ++p) {
            if ((lr_sgr_r0(ep) == 0 && p == 0) || (lr_sgr_r1(ep) == 0 && p == 1)) continue;
            bool skip = false;
            for (int dir = 0; dir < 2 && !out; dir++) {        // 0: down, 1: up
                if (dir == 1 && skip) break;
                for (;;) {
                    const int next = dir ? xqd[p] + s : xqd[p] - s;
                    if (dir ? next > lr_sgr_xqd_max(p) : next < lr_sgr_xqd_min(p)) break;
                    if (n >= max_evals) { out = true; break; }
                    const int keep = xqd[p];
                    xqd[p] = next;
                    lr_sgr_decode_xq(xqd, ep, xq);
                    const int64_t err2 = eval(xq[0], xq[1]);
                    n++;
                    if (err2 > err) { xqd[p] = keep; break; }      // a tie is accepted
                    err = err2;
                    if (dir == 0) skip = true;
                    if (s != LR_SGR_START_STEP) break;             // at the highest step keep moving in the same direction
                }
            }
            if (skip) break;                                       // `if (skip) break;` leaves the p loop
        }
    }
    *evals = n;
    return err;
}

// get_sg_step (:681-700) and the mid_ep / start_ep / end_ep lines of search_selfguided_restoration (:625-631)
LR_HD void lr_sgr_ep_range(int ref0, int ref1, int sg_filter_mode, int32_t out[2]) {
    const int step = sg_filter_mode == 1 ? 0 : (sg_filter_mode == 2 ? 1 : (sg_filter_mode == 3 ? 4 : 16));
    if (ref0 < 0 && ref1 < 0) { out[0] = 0; out[1] = LR_SGR_PARAMS; return; }
    const int mid = ref1 < 0 ? ref0 : (ref0 < 0 ? ref1 : (ref0 + ref1) / 2);
    out[0] = mid - step > 0 ? mid - step : 0;
    out[1] = mid + step < LR_SGR_PARAMS ? mid + step : LR_SGR_PARAMS;
}

}  // namespace svthost

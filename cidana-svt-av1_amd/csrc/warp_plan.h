// warp_plan.h — svt_hip_warp_fit_frame and svt_hip_warp_pred_frame planned on the host: the argument checks, the split of a group over
// the waves of a workgroup, and the launch lists, all derived before the first launch.  svt_hip_warp.hip checks, then enqueues from
// here.  Plain C++17, no HIP header: a CPU program can include it (tests/c/warp_plan_host.cpp).  WarpGeom is the one statement of the
// prediction's tiling: warp_pred_kernel (kernel_warp.h) derives the same numbers from the same two logarithms.
#pragma once
#include <stdint.h>

#include <vector>

#include "../../include/svt_hip_dsp.h"
#include "av1_geom.h"
#include "group_table.h"
#include "host_err.h"
#include "inter_plan.h"

#ifdef __HIPCC__
#define SVT_WARP_HD __host__ __device__ __forceinline__
#else
#define SVT_WARP_HD inline
#endif

namespace svtdev {
constexpr int WP_WAVES = 4, WP_THREADS = 64 * WP_WAVES;    // waves of a workgroup, both kernels
constexpr int WP_MAX_GROUPS = 48;                          // groups of one launch (the descriptors ride in the kernel arguments)

// The warp filter works on 8 x 8 tiles, a wave each.  A plane block of (1 << lw) x (1 << lh) samples (lw, lh 3 .. 6) is 1 << ltpb tiles;
// a slot is one (block, candidate) output.  Blocks of up to four tiles share a workgroup (4 >> ltpb slots of it); a larger block takes
// a workgroup of its own and its tiles go round by round, tile t of a round to wave t.  A slot never straddles two workgroups, so its
// distortion is summed inside one.
struct WarpGeom {
    int ltx;                 // log2 tiles of a block row
    int ltpb;                // log2 tiles of a block
    int slots_per_wg;
    int rounds;              // passes of the four waves over a slot's tiles
    int waves_per_slot;      // waves a slot's distortion is summed over
};
SVT_WARP_HD WarpGeom warp_geom(int lw, int lh) {
    WarpGeom G;
    G.ltx = lw - 3;
    G.ltpb = (lw - 3) + (lh - 3);
    G.slots_per_wg = G.ltpb <= 2 ? WP_WAVES >> G.ltpb : 1;
    G.rounds = G.ltpb <= 2 ? 1 : 1 << (G.ltpb - 2);
    G.waves_per_slot = G.ltpb <= 2 ? 1 << G.ltpb : WP_WAVES;
    return G;
}

// the launches' group tables (group_table.h)
struct WarpFitGroupDev {
    const svt_hip_warp_samples* samples;
    const svt_hip_inter_blk* blk;
    svt_hip_warp_model* model;
    uint32_t* nvalid;
    uint32_t nblocks, wg_end;
    uint8_t ncand, bw, bh, pad;
};
struct WarpFitDesc {
    int32_t ngroups;
    WarpFitGroupDev g[WP_MAX_GROUPS];
};
struct WarpPredGroupDev {
    const void* ref;
    const svt_hip_inter_blk* blk;
    const svt_hip_warp_model* model;
    const uint8_t* sel;
    void* pred;
    const void* src;
    unsigned long long* dist;
    uint32_t ref_stride, pred_stride, src_stride;
    uint32_t nslots;                  // nblocks * (sel ? n : ncand)
    uint32_t wg_end;
    uint32_t shape;                   // warp_shape_pack: ss, lw / lh (log2 of the PLANE block), ncand, n, sel_first
};
struct WarpPredDesc {
    int32_t ngroups;
    uint32_t pic_w, pic_h;
    int32_t bd, metric;
    WarpPredGroupDev g[WP_MAX_GROUPS];
};
static_assert(sizeof(WarpFitDesc) <= 4000 && sizeof(WarpPredDesc) <= 4000, "kernel arguments");

struct WarpShape { int ss, lw, lh, ncand, n, sel_first; };
SVT_WARP_HD uint32_t warp_shape_pack(const WarpShape& s) {
    return (uint32_t)s.ss | (uint32_t)s.lw << 1 | (uint32_t)s.lh << 4 | (uint32_t)s.ncand << 8 | (uint32_t)s.n << 16 | (uint32_t)s.sel_first << 24;
}
SVT_WARP_HD WarpShape warp_shape_unpack(uint32_t v) {
    WarpShape s;
    s.ss = v & 1; s.lw = (v >> 1) & 7; s.lh = (v >> 4) & 7; s.ncand = (v >> 8) & 0x7f; s.n = (v >> 16) & 0x7f; s.sel_first = v >> 24;
    return s;
}
}  // namespace svtdev

namespace svthost {

constexpr int kWarpMaxCand = 64;
inline int warp_log2_side(int v) { return v == 8 ? 3 : v == 16 ? 4 : v == 32 ? 5 : v == 64 ? 6 : -1; }

// ---- svt_hip_warp_fit_frame ----
// Every group of the call before the first launch.  SVT_HIP_OK, or SVT_HIP_ERR_INVALID with the reason in svt_hip_last_error().
inline int warp_fit_check(const svt_hip_warp_fit_group* groups, int ngroups) {
    if (ngroups < 0 || (ngroups > 0 && !groups)) return set_err(SVT_HIP_ERR_INVALID, "NULL group list");
    for (int g = 0; g < ngroups; g++) {
        const svt_hip_warp_fit_group& G = groups[g];
        if (G.bsize < 0 || G.bsize >= 22) return set_err(SVT_HIP_ERR_INVALID, "group %d: bsize %d (0 .. 21)", g, G.bsize);
        const int bw = kBsizeW[G.bsize], bh = kBsizeH[G.bsize];
        if (bw < 8 || bh < 8 || bw > 64 || bh > 64) return set_err(SVT_HIP_ERR_INVALID, "group %d: bsize %d is %d x %d (both sides 8 .. 64)", g, G.bsize, bw, bh);
        if (G.ncand < 1 || G.ncand > kWarpMaxCand) return set_err(SVT_HIP_ERR_INVALID, "group %d: ncand %d (1 .. %d)", g, G.ncand, kWarpMaxCand);
        if (!G.d_samples || !G.d_blk || !G.d_model) return set_err(SVT_HIP_ERR_INVALID, "group %d: NULL d_samples, d_blk or d_model", g);
        if (((uintptr_t)G.d_samples & 3) || ((uintptr_t)G.d_blk & 3) || ((uintptr_t)G.d_model & 3) || ((uintptr_t)G.d_nvalid & 3))
            return set_err(SVT_HIP_ERR_INVALID, "group %d: misaligned buffer (4 bytes)", g);
        if (inter_wgs(G.nblocks, svtdev::WP_WAVES) > kMaxLaunchWgs) return set_err(SVT_HIP_ERR_INVALID, "group %d: nblocks %u too large", g, G.nblocks);
    }
    return SVT_HIP_OK;
}

// The launches of a call that warp_fit_check accepted: a wave per block, the non-empty groups in list order, launch(desc,
// total_workgroups) -> int (0 = OK) once per WP_MAX_GROUPS of them.
template <typename Launch>
inline int warp_fit_enqueue(const svt_hip_warp_fit_group* groups, int ngroups, Launch&& launch) {
    GroupTable<svtdev::WarpFitDesc, svtdev::WP_MAX_GROUPS> tab;
    for (int g = 0; g < ngroups; g++) {
        const svt_hip_warp_fit_group& G = groups[g];
        if (G.nblocks == 0) continue;
        svtdev::WarpFitGroupDev* D = tab.add((uint32_t)inter_wgs(G.nblocks, svtdev::WP_WAVES), launch);
        if (!D) return tab.rc;
        D->samples = G.d_samples; D->blk = G.d_blk; D->model = G.d_model; D->nvalid = G.d_nvalid; D->nblocks = G.nblocks;
        D->ncand = (uint8_t)G.ncand; D->bw = kBsizeW[G.bsize]; D->bh = kBsizeH[G.bsize];
    }
    return tab.flush(launch);
}

// ---- svt_hip_warp_pred_frame ----
inline uint64_t warp_pred_slots(const svt_hip_warp_pred_group& G) { return (uint64_t)G.nblocks * (uint64_t)(G.d_sel ? G.n : G.ncand); }

inline int warp_pred_check(const svt_hip_warp_pred_group* groups, int ngroups, uint32_t pic_width, uint32_t pic_height, int bd, int metric) {
    if (ngroups < 0 || (ngroups > 0 && !groups)) return set_err(SVT_HIP_ERR_INVALID, "NULL group list");
    if (bd != 8 && bd != 10) return set_err(SVT_HIP_ERR_INVALID, "bd %d (8 or 10)", bd);
    if (metric != SVT_HIP_FAST_SAD && metric != SVT_HIP_FAST_SSD) return set_err(SVT_HIP_ERR_INVALID, "metric %d", metric);
    if (int rc = inter_picture_check(pic_width, pic_height)) return rc;
    for (int g = 0; g < ngroups; g++) {
        const svt_hip_warp_pred_group& G = groups[g];
        if (G.ss != 0 && G.ss != 1) return set_err(SVT_HIP_ERR_INVALID, "group %d: ss %d (0 luma, 1 chroma of 4:2:0)", g, G.ss);
        const int lw = warp_log2_side(G.bwidth), lh = warp_log2_side(G.bheight);
        if (lw < 0 || lh < 0) return set_err(SVT_HIP_ERR_INVALID, "group %d: block %d x %d (sides 8, 16, 32, 64)", g, G.bwidth, G.bheight);
        if (G.ss && (G.bwidth < 16 || G.bheight < 16))
            return set_err(SVT_HIP_ERR_INVALID, "group %d: chroma of a %d x %d block (both sides >= 16; smaller blocks' chroma is translational)", g, G.bwidth, G.bheight);
        if ((uint32_t)G.bwidth > pic_width || (uint32_t)G.bheight > pic_height)
            return set_err(SVT_HIP_ERR_INVALID, "group %d: block %d x %d in a picture of %u x %u", g, G.bwidth, G.bheight, pic_width, pic_height);
        if (G.ncand < 1 || G.ncand > kWarpMaxCand) return set_err(SVT_HIP_ERR_INVALID, "group %d: ncand %d (1 .. %d)", g, G.ncand, kWarpMaxCand);
        if (!G.d_ref || !G.d_blk || !G.d_model) return set_err(SVT_HIP_ERR_INVALID, "group %d: NULL d_ref, d_blk or d_model", g);
        if (G.d_sel ? (G.n < 1 || G.n > kWarpMaxCand || G.sel_first < 0 || G.sel_first > 255) : (G.n != 0 || G.sel_first != 0))
            return set_err(SVT_HIP_ERR_INVALID, "group %d: d_sel with n 1 .. %d and sel_first 0 .. 255; without it n and sel_first are 0 (n %d, sel_first %d)", g,
                           kWarpMaxCand, G.n, G.sel_first);
        if (!G.d_pred && !G.d_src && !G.d_dist) return set_err(SVT_HIP_ERR_INVALID, "group %d: no output (d_pred, d_src and d_dist all NULL)", g);
        if (!G.d_src != !G.d_dist) return set_err(SVT_HIP_ERR_INVALID, "group %d: d_src and d_dist come together", g);
        const uint32_t pw = (uint32_t)G.bwidth >> G.ss;
        if (((uintptr_t)G.d_dist & 7) || ((uintptr_t)G.d_blk & 3) || ((uintptr_t)G.d_model & 3) || (G.d_pred && G.pred_stride == 0 && ((uintptr_t)G.d_pred & 15)))
            return set_err(SVT_HIP_ERR_INVALID, "group %d: misaligned buffer (d_dist 8 bytes, d_blk and d_model 4 bytes, a dense d_pred 16 bytes)", g);
        if (G.d_pred && G.pred_stride != 0 && G.pred_stride < pw) return set_err(SVT_HIP_ERR_INVALID, "group %d: pred_stride %u below the block width %u", g, G.pred_stride, pw);
        const svtdev::WarpGeom ge = svtdev::warp_geom(lw - G.ss, lh - G.ss);
        const uint64_t slots = warp_pred_slots(G);
        if (slots > kMaxLaunchWgs || (slots + (uint64_t)ge.slots_per_wg - 1) / (uint64_t)ge.slots_per_wg > kMaxLaunchWgs)
            return set_err(SVT_HIP_ERR_INVALID, "group %d: nblocks %u x %d slots too large", g, G.nblocks, G.d_sel ? G.n : G.ncand);
    }
    return SVT_HIP_OK;
}

struct WarpGroupPlan {
    int src;                 // index into the caller's list
    int lw, lh;              // log2 of the PLANE block
    uint32_t nslots, wgs;
    svtdev::WarpGeom geom;
};

// The non-empty groups in list order, each with its tiling and its workgroup count.  plans has room for ngroups entries; returns their
// number.  Groups that warp_pred_check accepted.
inline int warp_pred_plan(const svt_hip_warp_pred_group* groups, int ngroups, WarpGroupPlan* plans) {
    int n = 0;
    for (int g = 0; g < ngroups; g++) {
        const svt_hip_warp_pred_group& G = groups[g];
        if (G.nblocks == 0) continue;
        WarpGroupPlan& P = plans[n++];
        P.src = g;
        P.lw = warp_log2_side(G.bwidth) - G.ss;
        P.lh = warp_log2_side(G.bheight) - G.ss;
        P.geom = svtdev::warp_geom(P.lw, P.lh);
        P.nslots = (uint32_t)warp_pred_slots(G);
        P.wgs = (P.nslots + (uint32_t)P.geom.slots_per_wg - 1) / (uint32_t)P.geom.slots_per_wg;
    }
    return n;
}

template <typename Launch>
inline int warp_pred_enqueue(const svt_hip_warp_pred_group* groups, int ngroups, uint32_t pic_width, uint32_t pic_height, int bd, int metric,
                             Launch&& launch) {
    std::vector<WarpGroupPlan> plans((size_t)(ngroups > 0 ? ngroups : 0));
    const int n = warp_pred_plan(groups, ngroups, plans.data());
    GroupTable<svtdev::WarpPredDesc, svtdev::WP_MAX_GROUPS> tab;
    tab.desc.pic_w = pic_width; tab.desc.pic_h = pic_height; tab.desc.bd = bd; tab.desc.metric = metric;
    for (int i = 0; i < n; i++) {
        const WarpGroupPlan& P = plans[(size_t)i];
        const svt_hip_warp_pred_group& G = groups[P.src];
        svtdev::WarpPredGroupDev* D = tab.add(P.wgs, launch);
        if (!D) return tab.rc;
        D->ref = G.d_ref; D->blk = G.d_blk; D->model = G.d_model; D->sel = G.d_sel; D->pred = G.d_pred; D->src = G.d_src;
        D->dist = (unsigned long long*)G.d_dist;
        D->ref_stride = G.ref_stride; D->pred_stride = G.pred_stride; D->src_stride = G.src_stride; D->nslots = P.nslots;
        D->shape = svtdev::warp_shape_pack({G.ss, P.lw, P.lh, G.ncand, G.d_sel ? G.n : 0, G.d_sel ? G.sel_first : 0});
    }
    return tab.flush(launch);
}

}  // namespace svthost

// inter_plan.h — svt_hip_inter_pred_frame planned on the host: the argument checks, the tiling of a (plane, block size) group over the
// waves of a workgroup, and the launch list, all derived before the first launch.  svt_hip_inter_pred.hip checks, plans, then enqueues
// from the plan.  Plain C++17, no HIP header: a CPU program can include it (tests/c/inter_plan_host.cpp).  InterGeom is the one
// statement of the tiling: the kernels' ip_lane and ip_block (kernel_inter_steps.h) derive the same numbers from the same two logarithms.
#pragma once
#include <stdint.h>

#include <vector>

#include "../../include/svt_hip_dsp.h"
#include "group_table.h"
#include "host_err.h"

#ifdef __HIPCC__
#define SVT_INTER_HD __host__ __device__ __forceinline__
#else
#define SVT_INTER_HD inline
#endif

namespace svtdev {
constexpr int IP_WAVES = 4, IP_THREADS = 64 * IP_WAVES;     // waves of a workgroup
constexpr int IP_MAX_GROUPS = 48;                           // groups of one launch (InterPredDesc rides in the kernel arguments)
constexpr int IP_LDS_WIN = 2112, IP_LDS_HR = 704;           // per wave: staged windows (uint16) and first-pass rows (int16); 4x4 tiles set both

// A plane block of (1 << lw) x (1 << lh) samples is cut into tiles of at most 16 x 16; a lane owns 4 samples of one tile row, so a tile
// takes tile_px / 4 lanes and a wave holds 64 / that many tiles ("slots").  A workgroup's 4 * slots tiles go round by round, tile t of a
// round to wave t / slots, slot t % slots; a block's tiles are consecutive, so a block never straddles two workgroups.
struct InterGeom {
    int ltw, lth;            // log2 of the tile
    int llanes;              // log2 lanes of a slot
    int slots;               // tiles of a wave
    int ltpb;                // log2 tiles of a block
    int blocks_per_wg;       // whole blocks of a workgroup
    int rounds;              // passes of a workgroup over its 4 * slots tiles (> 1: one block, more tiles than the workgroup holds)
    int dist_lanes;          // lanes of one wave that hold one block (the span of the in-wave distortion sum)
    int waves_per_block;     // waves a block's distortion is summed over (through LDS when > 1)
};
SVT_INTER_HD InterGeom inter_geom(int lw, int lh) {
    InterGeom G;
    G.ltw = lw < 4 ? lw : 4;
    G.lth = lh < 4 ? lh : 4;
    G.llanes = G.ltw + G.lth - 2;
    G.slots = 64 >> G.llanes;
    G.ltpb = (lw - G.ltw) + (lh - G.lth);
    const int ltiles = 2 + 6 - G.llanes;                     // log2 tiles of a workgroup's round
    G.blocks_per_wg = G.ltpb <= ltiles ? 1 << (ltiles - G.ltpb) : 1;
    G.rounds = G.ltpb <= ltiles ? 1 : 1 << (G.ltpb - ltiles);
    const int tpb = 1 << G.ltpb;
    G.dist_lanes = (tpb < G.slots ? tpb : G.slots) << G.llanes;
    G.waves_per_block = tpb <= G.slots ? 1 : (tpb / G.slots < IP_WAVES ? tpb / G.slots : IP_WAVES);
    return G;
}

// the launch's group table (group_table.h): it rides in the kernel arguments
struct InterPredGroupDev {
    const void* ref[2];
    const svt_hip_inter_blk* blk;
    void* pred;
    const void* src;
    unsigned long long* dist;
    uint32_t ref_stride, pred_stride, src_stride, nblocks;
    uint32_t wg_end;
    uint8_t ss, lw, lh, pad;          // lw / lh: log2 of the PLANE block
};
struct InterPredDesc {
    int32_t ngroups;
    uint32_t pic_w, pic_h;
    int32_t bd, metric;
    InterPredGroupDev g[IP_MAX_GROUPS];
};
static_assert(sizeof(InterPredDesc) <= 4000, "kernel arguments");
}  // namespace svtdev

namespace svthost {

constexpr uint32_t kInterMaxSide = 16384;                   // picture sides (the clamp's 1/16-sample arithmetic stays far inside 32 bits)

inline int inter_log2_side(int v) { return v == 4 ? 2 : v == 8 ? 3 : v == 16 ? 4 : v == 32 ? 5 : v == 64 ? 6 : -1; }
// the two clauses every call of the family states (interp_plan.h too): the picture's sides, and the workgroups that `per_wg` blocks a
// workgroup make of a group (64 bits: nblocks goes up to 2^32 - 1, the checks compare the count with kMaxLaunchWgs)
inline int inter_picture_check(uint32_t pic_width, uint32_t pic_height) {
    const bool bad = pic_width == 0 || pic_height == 0 || (pic_width & 7) || (pic_height & 7) || pic_width > kInterMaxSide || pic_height > kInterMaxSide;
    return bad ? set_err(SVT_HIP_ERR_INVALID, "picture %u x %u: both sides must be multiples of 8, 8 .. %u", pic_width, pic_height, kInterMaxSide) : SVT_HIP_OK;
}
inline uint64_t inter_wgs(uint32_t nblocks, int per_wg) { return ((uint64_t)nblocks + (uint64_t)per_wg - 1) / (uint64_t)per_wg; }

struct InterGroupPlan {
    int src;                 // index into the caller's list
    int lw, lh;              // log2 of the PLANE block
    uint32_t wgs;
    svtdev::InterGeom geom;
};

// Every group of the call before the first launch.  SVT_HIP_OK, or SVT_HIP_ERR_INVALID with the reason in svt_hip_last_error().
inline int inter_pred_check(const svt_hip_inter_pred_group* groups, int ngroups, uint32_t pic_width, uint32_t pic_height, int bd, int metric) {
    if (ngroups < 0 || (ngroups > 0 && !groups)) return set_err(SVT_HIP_ERR_INVALID, "NULL group list");
    if (bd != 8 && bd != 10) return set_err(SVT_HIP_ERR_INVALID, "bd %d (8 or 10)", bd);
    if (metric != SVT_HIP_FAST_SAD && metric != SVT_HIP_FAST_SSD) return set_err(SVT_HIP_ERR_INVALID, "metric %d", metric);
    if (int rc = inter_picture_check(pic_width, pic_height)) return rc;
    for (int g = 0; g < ngroups; g++) {
        const svt_hip_inter_pred_group& G = groups[g];
        if (G.ss != 0 && G.ss != 1) return set_err(SVT_HIP_ERR_INVALID, "group %d: ss %d (0 luma, 1 chroma of 4:2:0)", g, G.ss);
        const int lw = inter_log2_side(G.bwidth), lh = inter_log2_side(G.bheight);
        if (lw < 0 || lh < 0) return set_err(SVT_HIP_ERR_INVALID, "group %d: block %d x %d (sides 4, 8, 16, 32, 64)", g, G.bwidth, G.bheight);
        if (G.ss && (G.bwidth < 8 || G.bheight < 8)) return set_err(SVT_HIP_ERR_INVALID, "group %d: chroma of a %d x %d block (both sides >= 8)", g, G.bwidth, G.bheight);
        if ((uint32_t)G.bwidth > pic_width || (uint32_t)G.bheight > pic_height)
            return set_err(SVT_HIP_ERR_INVALID, "group %d: block %d x %d in a picture of %u x %u", g, G.bwidth, G.bheight, pic_width, pic_height);
        if (!G.d_blk || !G.d_ref[0]) return set_err(SVT_HIP_ERR_INVALID, "group %d: NULL d_blk or d_ref[0]", g);
        if (!G.d_pred && !G.d_src && !G.d_dist) return set_err(SVT_HIP_ERR_INVALID, "group %d: no output (d_pred, d_src and d_dist all NULL)", g);
        if (!G.d_src != !G.d_dist) return set_err(SVT_HIP_ERR_INVALID, "group %d: d_src and d_dist come together", g);
        const uint32_t pw = (uint32_t)G.bwidth >> G.ss;
        if (((uintptr_t)G.d_dist & 7) || ((uintptr_t)G.d_blk & 3) || (G.d_pred && G.pred_stride == 0 && ((uintptr_t)G.d_pred & 15)))
            return set_err(SVT_HIP_ERR_INVALID, "group %d: misaligned buffer (d_dist 8 bytes, d_blk 4 bytes, a dense d_pred 16 bytes)", g);
        if (G.d_pred && G.pred_stride != 0 && G.pred_stride < pw) return set_err(SVT_HIP_ERR_INVALID, "group %d: pred_stride %u below the block width %u", g, G.pred_stride, pw);
        const svtdev::InterGeom ge = svtdev::inter_geom(lw - G.ss, lh - G.ss);
        if (inter_wgs(G.nblocks, ge.blocks_per_wg) > kMaxLaunchWgs) return set_err(SVT_HIP_ERR_INVALID, "group %d: nblocks %u too large", g, G.nblocks);
    }
    return SVT_HIP_OK;
}

// The non-empty groups in list order, each with its tiling and its workgroup count.  plans has room for ngroups entries; returns their
// number.  Groups that inter_pred_check accepted.
inline int inter_pred_plan(const svt_hip_inter_pred_group* groups, int ngroups, InterGroupPlan* plans) {
    int n = 0;
    for (int g = 0; g < ngroups; g++) {
        const svt_hip_inter_pred_group& G = groups[g];
        if (G.nblocks == 0) continue;
        InterGroupPlan& P = plans[n++];
        P.src = g;
        P.lw = inter_log2_side(G.bwidth) - G.ss;
        P.lh = inter_log2_side(G.bheight) - G.ss;
        P.geom = svtdev::inter_geom(P.lw, P.lh);
        P.wgs = (uint32_t)inter_wgs(G.nblocks, P.geom.blocks_per_wg);
    }
    return n;
}

// The launches of a call that inter_pred_check accepted: the planned groups go into the group table in list order and
// launch(desc, total_workgroups) -> int (0 = OK) is called once per IP_MAX_GROUPS of them.
template <typename Launch>
inline int inter_pred_enqueue(const svt_hip_inter_pred_group* groups, int ngroups, uint32_t pic_width, uint32_t pic_height, int bd, int metric,
                              Launch&& launch) {
    std::vector<InterGroupPlan> plans((size_t)(ngroups > 0 ? ngroups : 0));
    const int n = inter_pred_plan(groups, ngroups, plans.data());
    GroupTable<svtdev::InterPredDesc, svtdev::IP_MAX_GROUPS> tab;
    tab.desc.pic_w = pic_width; tab.desc.pic_h = pic_height; tab.desc.bd = bd; tab.desc.metric = metric;
    for (int i = 0; i < n; i++) {
        const InterGroupPlan& P = plans[(size_t)i];
        const svt_hip_inter_pred_group& G = groups[P.src];
        svtdev::InterPredGroupDev* D = tab.add(P.wgs, launch);
        if (!D) return tab.rc;
        D->ref[0] = G.d_ref[0]; D->ref[1] = G.d_ref[1]; D->blk = G.d_blk; D->pred = G.d_pred; D->src = G.d_src;
        D->dist = (unsigned long long*)G.d_dist;
        D->ref_stride = G.ref_stride; D->pred_stride = G.pred_stride; D->src_stride = G.src_stride; D->nblocks = G.nblocks;
        D->ss = (uint8_t)G.ss; D->lw = (uint8_t)P.lw; D->lh = (uint8_t)P.lh;
    }
    return tab.flush(launch);
}

}  // namespace svthost

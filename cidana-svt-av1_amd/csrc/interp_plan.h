// interp_plan.h — the interpolation filter search planned on the host: the argument checks of svt_hip_interp_sse_frame /
// _decide_frame / _search_frame, the scratch layout of the one-call search and the launch lists, all derived before the first launch.
// svt_hip_interp_search.hip checks, plans, then enqueues from the plan.  Plain C++17, no HIP header: a CPU program can include it
// (tests/c/interp_plan_host.cpp).  The tiling is inter_plan.h's InterGeom: a (group, plane) pair is one entry of the SSE kernel's group
// table, tiled exactly as svt_hip_inter_pred_frame tiles that plane block.
#pragma once
#include <stdint.h>

#include <vector>

#include "inter_plan.h"
#include "md_plan.h"

namespace svtdev {
constexpr int IS_NPAIR = 9;                                  // filter_sets (EbInterPrediction.c:3573)
constexpr int IS_LDS_HR = 3 * IP_LDS_HR;                     // per wave: the first-pass rows of the three horizontal filters
constexpr int ID_THREADS = 256, ID_MAX_GROUPS = 32;          // the walk: a thread a block

struct InterpSseGroupDev {
    const uint8_t* ref[2];
    const uint8_t* src;
    const svt_hip_inter_blk* blk;
    uint32_t* sse;                    // the plane's first entry of block 0; a block's entries are sse_stride words apart
    uint32_t ref_stride, src_stride, nblocks, sse_stride;
    uint32_t wg_end;
    uint8_t ss, lw, lh, pad;          // lw / lh: log2 of the PLANE block
};
struct InterpSseDesc {
    int32_t ngroups;
    uint32_t pic_w, pic_h;
    InterpSseGroupDev g[IP_MAX_GROUPS];
};
static_assert(sizeof(InterpSseDesc) <= 4000, "kernel arguments");

struct InterpDecideGroupDev {
    const uint32_t* sse;
    const uint8_t* ctx;
    const uint8_t* searchable;
    unsigned long long* decision;
    const svt_hip_inter_blk* blk;
    svt_hip_inter_blk* blk_out;
    uint32_t nblocks;
    uint32_t wg_end;
    uint32_t nlog2_y;                 // num_pels_log2 of the luma block (chroma: 2 less)
    uint32_t pad;
};
struct InterpDecideDesc {
    int32_t ngroups;
    uint32_t lambda, qstep;           // full_lambda; ac_dequant_q3 >> 3
    int32_t use_uv, mode;
    const int32_t* rates;
    InterpDecideGroupDev g[ID_MAX_GROUPS];
};
static_assert(sizeof(InterpDecideDesc) <= 4000, "kernel arguments");
}  // namespace svtdev

namespace svthost {

inline int interp_side_ok(int v) { return v == 8 || v == 16 || v == 32 || v == 64; }
inline int interp_planes(int use_uv) { return use_uv ? 3 : 1; }
inline size_t interp_sse_bytes(uint32_t nblocks, int use_uv) {       // a group's table, rounded up to the scratch's 16-byte grain
    return align16((size_t)nblocks * (size_t)interp_planes(use_uv) * svtdev::IS_NPAIR * sizeof(uint32_t));
}

// Every group of an SSE call before the first launch.  allow_null_sse: the one-call search carves the table from its scratch.
inline int interp_sse_check(const svt_hip_interp_sse_group* groups, int ngroups, uint32_t pic_width, uint32_t pic_height, int bd, int use_uv,
                            bool allow_null_sse = false) {
    if (int rc = group_list_check(groups, ngroups)) return rc;
    if (bd != 8) return set_err(SVT_HIP_ERR_INVALID, "bd %d (the filter search is pinned for 8-bit only)", bd);
    if (use_uv != 0 && use_uv != 1) return set_err(SVT_HIP_ERR_INVALID, "use_uv %d", use_uv);
    if (int rc = inter_picture_check(pic_width, pic_height)) return rc;
    for (int g = 0; g < ngroups; g++) {
        const svt_hip_interp_sse_group& G = groups[g];
        if (!interp_side_ok(G.bwidth) || !interp_side_ok(G.bheight))
            return set_err(SVT_HIP_ERR_INVALID, "group %d: block %d x %d (sides 8, 16, 32, 64)", g, G.bwidth, G.bheight);
        if ((uint32_t)G.bwidth > pic_width || (uint32_t)G.bheight > pic_height)
            return set_err(SVT_HIP_ERR_INVALID, "group %d: block %d x %d in a picture of %u x %u", g, G.bwidth, G.bheight, pic_width, pic_height);
        if (!G.d_blk || ((uintptr_t)G.d_blk & 3)) return set_err(SVT_HIP_ERR_INVALID, "group %d: d_blk NULL or not 4-byte aligned", g);
        if ((!G.d_sse && !allow_null_sse) || ((uintptr_t)G.d_sse & 3)) return set_err(SVT_HIP_ERR_INVALID, "group %d: d_sse NULL or not 4-byte aligned", g);
        for (int p = 0; p < interp_planes(use_uv); p++)
            if (!G.d_ref[0][p] || !G.d_src[p]) return set_err(SVT_HIP_ERR_INVALID, "group %d: NULL d_ref[0][%d] or d_src[%d]", g, p, p);
        const svtdev::InterGeom ge = svtdev::inter_geom(inter_log2_side(G.bwidth), inter_log2_side(G.bheight));
        if (inter_wgs(G.nblocks, ge.blocks_per_wg) > kMaxLaunchWgs) return set_err(SVT_HIP_ERR_INVALID, "group %d: nblocks %u too large", g, G.nblocks);
    }
    return SVT_HIP_OK;
}

// from_search: an empty group of the one-call search has no table to point at.
inline int interp_decide_check(const svt_hip_interp_decide_group* groups, int ngroups, const svt_hip_interp_params* params, bool from_search = false) {
    if (int rc = group_list_check(groups, ngroups)) return rc;
    if (!params || !params->d_rates || ((uintptr_t)params->d_rates & 3)) return set_err(SVT_HIP_ERR_INVALID, "NULL params or d_rates (4-byte aligned)");
    if (params->mode < SVT_HIP_INTERP_DUAL_FAST || params->mode > SVT_HIP_INTERP_SINGLE) return set_err(SVT_HIP_ERR_INVALID, "mode %d", params->mode);
    if (params->use_uv != 0 && params->use_uv != 1) return set_err(SVT_HIP_ERR_INVALID, "use_uv %d", params->use_uv);
    if (params->ac_dequant_q3 < 0 || params->ac_dequant_q3 > 32767) return set_err(SVT_HIP_ERR_INVALID, "ac_dequant_q3 %d (an int16 quantiser step)", params->ac_dequant_q3);
    for (int g = 0; g < ngroups; g++) {
        const svt_hip_interp_decide_group& G = groups[g];
        if (!interp_side_ok(G.bwidth) || !interp_side_ok(G.bheight))
            return set_err(SVT_HIP_ERR_INVALID, "group %d: block %d x %d (sides 8, 16, 32, 64)", g, G.bwidth, G.bheight);
        if ((!G.d_sse && !(from_search && G.nblocks == 0)) || ((uintptr_t)G.d_sse & 3))
            return set_err(SVT_HIP_ERR_INVALID, "group %d: d_sse NULL or not 4-byte aligned", g);
        if (!G.d_ctx || !G.d_searchable) return set_err(SVT_HIP_ERR_INVALID, "group %d: NULL d_ctx or d_searchable", g);
        if (!G.d_decision || ((uintptr_t)G.d_decision & 7)) return set_err(SVT_HIP_ERR_INVALID, "group %d: d_decision NULL or not 8-byte aligned", g);
        if (G.d_blk_out && !G.d_blk) return set_err(SVT_HIP_ERR_INVALID, "group %d: d_blk_out without d_blk", g);
        if (((uintptr_t)G.d_blk & 3) || ((uintptr_t)G.d_blk_out & 3)) return set_err(SVT_HIP_ERR_INVALID, "group %d: d_blk / d_blk_out not 4-byte aligned", g);
    }
    return SVT_HIP_OK;
}

// The launches of an SSE call that interp_sse_check accepted: per non-empty group an entry per plane, in list order;
// launch(desc, total_workgroups) -> int (0 = OK) once per IP_MAX_GROUPS entries.
template <typename Launch>
inline int interp_sse_enqueue(const svt_hip_interp_sse_group* groups, int ngroups, uint32_t pic_width, uint32_t pic_height, int use_uv, Launch&& launch) {
    GroupTable<svtdev::InterpSseDesc, svtdev::IP_MAX_GROUPS> tab;
    tab.desc.pic_w = pic_width; tab.desc.pic_h = pic_height;
    const int planes = interp_planes(use_uv);
    for (int g = 0; g < ngroups; g++) {
        const svt_hip_interp_sse_group& G = groups[g];
        if (G.nblocks == 0) continue;
        for (int p = 0; p < planes; p++) {
            const int ss = p ? 1 : 0, lw = inter_log2_side(G.bwidth) - ss, lh = inter_log2_side(G.bheight) - ss;
            const svtdev::InterGeom ge = svtdev::inter_geom(lw, lh);
            svtdev::InterpSseGroupDev* D = tab.add((uint32_t)inter_wgs(G.nblocks, ge.blocks_per_wg), launch);
            if (!D) return tab.rc;
            D->ref[0] = G.d_ref[0][p]; D->ref[1] = G.d_ref[1][p]; D->src = G.d_src[p]; D->blk = G.d_blk;
            D->sse = G.d_sse + p * svtdev::IS_NPAIR;
            D->ref_stride = G.ref_stride[p]; D->src_stride = G.src_stride[p]; D->nblocks = G.nblocks;
            D->sse_stride = (uint32_t)(planes * svtdev::IS_NPAIR);
            D->ss = (uint8_t)ss; D->lw = (uint8_t)lw; D->lh = (uint8_t)lh;
        }
    }
    return tab.flush(launch);
}

// The launches of a decide call that interp_decide_check accepted: a thread a block, one launch per ID_MAX_GROUPS non-empty groups.
template <typename Launch>
inline int interp_decide_enqueue(const svt_hip_interp_decide_group* groups, int ngroups, const svt_hip_interp_params& prm, Launch&& launch) {
    GroupTable<svtdev::InterpDecideDesc, svtdev::ID_MAX_GROUPS> tab;
    tab.desc.lambda = prm.full_lambda; tab.desc.qstep = (uint32_t)(prm.ac_dequant_q3 >> 3); tab.desc.use_uv = prm.use_uv;
    tab.desc.mode = prm.mode; tab.desc.rates = prm.d_rates;
    for (int g = 0; g < ngroups; g++) {
        const svt_hip_interp_decide_group& G = groups[g];
        if (G.nblocks == 0) continue;
        svtdev::InterpDecideGroupDev* D = tab.add((uint32_t)inter_wgs(G.nblocks, svtdev::ID_THREADS), launch);
        if (!D) return tab.rc;
        D->sse = G.d_sse; D->ctx = G.d_ctx; D->searchable = G.d_searchable; D->decision = (unsigned long long*)G.d_decision;
        D->blk = G.d_blk; D->blk_out = G.d_blk_out; D->nblocks = G.nblocks;
        D->nlog2_y = (uint32_t)(inter_log2_side(G.bwidth) + inter_log2_side(G.bheight));
    }
    return tab.flush(launch);
}

// ---- the one-call search: scratch and the two stages' groups ----
struct InterpStages { std::vector<svt_hip_interp_sse_group> sg; std::vector<svt_hip_interp_decide_group> dg; };      // an entry per group, empty ones included
// The walk (md_plan.h's Carver): per non-empty group without a table of its own, in group order, its table of interp_sse_bytes; with
// `st` both stages' groups.  The stages' own checks run on the result.
inline int interp_search_walk(int use_uv, const svt_hip_interp_search_group* groups, int ngroups, Carver& sc, InterpStages* st) {
    if (int rc = group_list_check(groups, ngroups)) return rc;
    if (use_uv != 0 && use_uv != 1) return set_err(SVT_HIP_ERR_INVALID, "use_uv %d", use_uv);
    if (st) { st->sg.resize((size_t)ngroups); st->dg.resize((size_t)ngroups); }
    for (int g = 0; g < ngroups; g++) {
        const svt_hip_interp_search_group& G = groups[g];
        svt_hip_interp_sse_group S = G.sse;
        if (S.nblocks && !S.d_sse) sc.piece(S.d_sse, interp_sse_bytes(S.nblocks, use_uv));
        if (!st) continue;
        svt_hip_interp_decide_group D{};
        D.bwidth = S.bwidth; D.bheight = S.bheight; D.nblocks = S.nblocks; D.d_sse = S.d_sse; D.d_ctx = G.d_ctx; D.d_searchable = G.d_searchable;
        D.d_decision = G.d_decision; D.d_blk = S.d_blk; D.d_blk_out = G.d_blk_out;
        st->sg[(size_t)g] = S; st->dg[(size_t)g] = D;
    }
    return SVT_HIP_OK;
}
inline size_t interp_search_scratch_bytes(const svt_hip_interp_search_group* groups, int ngroups, int use_uv) {      // 0: bad parameters or nothing to carve
    return scratch_bytes_of([=](auto* g, int n, Carver& sc, InterpStages* st) { return interp_search_walk(use_uv, g, n, sc, st); }, groups, ngroups);
}
// The group list, the parameters, then the scratch: sized, accepted or refused, carved (plan_stages).
inline int interp_search_plan(const svt_hip_interp_search_group* groups, int ngroups, const svt_hip_interp_params* params, void* d_scratch,
                              size_t scratch_bytes, InterpStages* st) {
    if (int rc = group_list_check(groups, ngroups)) return rc;
    if (!params) return set_err(SVT_HIP_ERR_INVALID, "NULL params");
    const auto walk = [params](auto* g, int n, Carver& sc, InterpStages* s) { return interp_search_walk(params->use_uv, g, n, sc, s); };
    return plan_stages(walk, groups, ngroups, d_scratch, scratch_bytes, st);
}

}  // namespace svthost

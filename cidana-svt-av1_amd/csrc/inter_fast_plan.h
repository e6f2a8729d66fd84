// inter_fast_plan.h — the inter fast search planned on the host: the argument check of svt_hip_inter_fast_pick_frame (its counts and
// blocks per wave are md_plan.h's fast_n, fast_nbuf, pick_bpw), and for svt_hip_inter_fast_search_frame ONE walk over its groups that
// sizes its scratch, carves it and derives the groups of its stages (distortion-only prediction, pick, the survivors' prediction, the
// intra gather).  svt_hip_inter_fast.hip checks and plans here, then enqueues.  Plain C++17, no HIP header: a CPU program can include
// it (tests/c/inter_fast_plan_host.cpp).
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <vector>

#include "inter_plan.h"
#include "md_plan.h"

namespace svthost {

// the shape of a combined list, as the pick and the search both require it (empty groups included)
inline int inter_fast_list_check(int g, int ninter, int nintra, int nfl) {
    if (ninter < 1 || ninter > 64 || nintra < 0 || nintra > 63 || ninter + nintra > SVT_HIP_FAST_LOOP_MAX_CANDIDATES)
        return set_err(SVT_HIP_ERR_INVALID, "group %d: ninter %d (1 .. 64), nintra %d (0 .. 63), together at most 64", g, ninter, nintra);
    if (nfl < 1 || nfl > SVT_HIP_MAX_NFL) return set_err(SVT_HIP_ERR_INVALID, "group %d: nfl %d (1 .. %d)", g, nfl, SVT_HIP_MAX_NFL);
    return SVT_HIP_OK;
}

// every group of a pick call before the first launch, empty groups' sizes and counts included
inline int inter_fast_pick_check(const svt_hip_inter_fast_pick_group* groups, int ngroups, int metric) {
    if (int rc = group_list_check(groups, ngroups)) return rc;
    if (int rc = metric_check(metric)) return rc;
    for (int g = 0; g < ngroups; g++) {
        const svt_hip_inter_fast_pick_group& G = groups[g];
        if (G.bsize < 0 || G.bsize > 21 || G.bsize_uv < 0 || G.bsize_uv > 21)
            return set_err(SVT_HIP_ERR_INVALID, "group %d: bsize %d / bsize_uv %d (0 .. 21)", g, G.bsize, G.bsize_uv);
        if (int rc = inter_fast_list_check(g, G.ninter, G.nintra, G.nfl)) return rc;
        if (G.ac_dequant_q3 < 0) return set_err(SVT_HIP_ERR_INVALID, "group %d: ac_dequant_q3 %d", g, G.ac_dequant_q3);
        if (G.nblocks == 0) continue;
        if (int rc = pairs_check(g, G.nblocks, (uint64_t)(G.ninter + G.nintra), "nblocks * ncand")) return rc;
        if (!G.d_blk || !G.d_cand_in || !G.d_ctx || !G.d_rates || !G.d_mv_cost || !G.d_dist || !G.d_cand || !G.d_sorted || !G.d_cost || !G.d_rate ||
            !G.d_ref_fast_cost || !G.d_blk_out)
            return set_err(SVT_HIP_ERR_INVALID, "group %d: NULL member", g);
        if (G.nintra > 0 && !G.d_intra_cost) return set_err(SVT_HIP_ERR_INVALID, "group %d: nintra %d without d_intra_cost", g, G.nintra);
        if (((uintptr_t)G.d_dist & 7) || ((uintptr_t)G.d_dist_cb & 7) || ((uintptr_t)G.d_dist_cr & 7) || ((uintptr_t)G.d_intra_cost & 7) ||
            ((uintptr_t)G.d_cost & 7) || ((uintptr_t)G.d_ref_fast_cost & 7) || ((uintptr_t)G.d_all_cost & 7) || ((uintptr_t)G.d_blk & 3) ||
            ((uintptr_t)G.d_blk_out & 3) || ((uintptr_t)G.d_cand_in & 3) || ((uintptr_t)G.d_cand_out & 3) || ((uintptr_t)G.d_ctx & 3) ||
            ((uintptr_t)G.d_rates & 3) || ((uintptr_t)G.d_mv_cost & 3) || ((uintptr_t)G.d_rate & 3) || ((uintptr_t)G.d_intra_rate & 3) ||
            ((uintptr_t)G.d_src_xy_out & 3))
            return set_err(SVT_HIP_ERR_INVALID, "group %d: misaligned buffer (the 8-byte arrays 8, the records, tables and 4-byte arrays 4)", g);
    }
    return SVT_HIP_OK;
}

// ---- svt_hip_inter_fast_search_frame: scratch and stage groups ---------------------------------------------------------------------------
struct InterFastGather {                                    // step 4 of one group: the intra survivors' luma predictions
    const uint8_t* d_cand; const void* d_intra_pred; void* d_pred_out;
    uint32_t nblocks, n, ninter, nintra, quads;             // quads: 16-byte pieces of a luma block
};
struct InterFastStages {
    std::vector<svt_hip_inter_pred_group> dist;             // step 1: Y, then Cb and Cr of the groups with chroma
    std::vector<svt_hip_inter_fast_pick_group> pick;        // step 2
    std::vector<svt_hip_inter_pred_group> pred;             // step 3
    std::vector<InterFastGather> gather;                    // step 4
};
// The walk (md_plan.h's Carver): checks what the carving needs of each group, carves, and with `st` derives the four stages' groups.
// bytes_per_sample (1: bd 8, 2: bd 10) sizes the intra gather only: the carved pieces are distortions, the same for either depth.
inline int inter_fast_search_walk(int bytes_per_sample, const svt_hip_inter_fast_search_group* groups, int ngroups, Carver& sc, InterFastStages* st) {
    if (int rc = group_list_check(groups, ngroups)) return rc;
    for (int g = 0; g < ngroups; g++) {
        const svt_hip_inter_fast_search_group& G = groups[g];
        svt_hip_inter_fast_pick_group P = G.pick;
        if (int rc = inter_fast_list_check(g, P.ninter, P.nintra, P.nfl)) return rc;
        if (int rc = pairs_check(g, P.nblocks, (uint64_t)(P.ninter + P.nintra), "nblocks * ncand")) return rc;
        if (P.bsize < 0 || P.bsize > 21 || kBsizeW[P.bsize] != G.bwidth || kBsizeH[P.bsize] != G.bheight)
            return set_err(SVT_HIP_ERR_INVALID, "group %d: bsize %d is not the %d x %d block", g, P.bsize, G.bwidth, G.bheight);
        const size_t pairs = (size_t)P.nblocks * (size_t)P.ninter;
        uint64_t *dy = (uint64_t*)P.d_dist, *dcb = (uint64_t*)P.d_dist_cb, *dcr = (uint64_t*)P.d_dist_cr;
        if (pairs) {
            if (!dy) sc.piece(dy, pairs * 8);
            if (G.use_chroma && !dcb) sc.piece(dcb, pairs * 8);
            if (G.use_chroma && !dcr) sc.piece(dcr, pairs * 8);
        }
        if (!st) continue;
        if (!G.use_chroma) dcb = dcr = nullptr;
        P.d_dist = dy; P.d_dist_cb = dcb; P.d_dist_cr = dcr;
        st->pick.push_back(P);
        if (P.nblocks == 0) continue;
        const int n = fast_n(P.nfl, P.ninter + P.nintra);
        if (!G.d_pred_out[0]) return set_err(SVT_HIP_ERR_INVALID, "group %d: NULL d_pred_out[0]", g);
        uint64_t* dists[3] = {dy, dcb, dcr};
        for (int p = 0; p < (G.use_chroma ? 3 : 1); p++) {
            svt_hip_inter_pred_group D{};
            D.d_ref[0] = G.d_ref[0][p]; D.d_ref[1] = G.d_ref[1][p]; D.ref_stride = G.ref_stride[p]; D.ss = p ? 1 : 0;
            D.bwidth = G.bwidth; D.bheight = G.bheight; D.nblocks = (uint32_t)pairs; D.d_blk = P.d_blk;
            D.d_src = G.d_src[p]; D.src_stride = G.src_stride[p]; D.d_dist = dists[p];
            if (!D.d_src) return set_err(SVT_HIP_ERR_INVALID, "group %d: NULL d_src[%d]", g, p);
            st->dist.push_back(D);
            if (!G.d_pred_out[p]) continue;
            svt_hip_inter_pred_group R = D;
            R.nblocks = P.nblocks * (uint32_t)n; R.d_blk = P.d_blk_out; R.d_pred = G.d_pred_out[p]; R.pred_stride = 0;
            R.d_src = nullptr; R.d_dist = nullptr;
            st->pred.push_back(R);
        }
        if (G.d_intra_pred && P.nintra > 0) {
            if (((uintptr_t)G.d_intra_pred & 15)) return set_err(SVT_HIP_ERR_INVALID, "group %d: d_intra_pred not 16-byte aligned", g);
            if (G.d_intra_pred == G.d_pred_out[0]) return set_err(SVT_HIP_ERR_INVALID, "group %d: d_intra_pred is d_pred_out[0]", g);
            InterFastGather T{P.d_cand, G.d_intra_pred, G.d_pred_out[0], P.nblocks, (uint32_t)n, (uint32_t)P.ninter, (uint32_t)P.nintra,
                              (uint32_t)(G.bwidth * G.bheight * bytes_per_sample / 16)};
            st->gather.push_back(T);
        }
    }
    return SVT_HIP_OK;
}
inline size_t inter_fast_search_scratch_bytes(const svt_hip_inter_fast_search_group* groups, int ngroups, int bytes_per_sample = 1) {
    return scratch_bytes_of([=](auto* g, int n, Carver& sc, InterFastStages* st) { return inter_fast_search_walk(bytes_per_sample, g, n, sc, st); }, groups, ngroups);
}

// Everything the call checks before its first launch: bd, the scratch, then every stage's own check on the derived groups.
inline int inter_fast_search_plan(const svt_hip_inter_fast_search_group* groups, int ngroups, uint32_t pic_width, uint32_t pic_height, int bd,
                                  int metric, void* d_scratch, size_t scratch_bytes, InterFastStages* st) {
    if (bd != 8 && bd != 10) return set_err(SVT_HIP_ERR_INVALID, "bd %d (8 or 10)", bd);
    const auto walk = [bd](auto* g, int n, Carver& sc, InterFastStages* s) { return inter_fast_search_walk(bd == 8 ? 1 : 2, g, n, sc, s); };
    if (int rc = plan_stages(walk, groups, ngroups, d_scratch, scratch_bytes, st)) return rc;
    if (int rc = inter_pred_check(st->dist.data(), (int)st->dist.size(), pic_width, pic_height, bd, metric)) return rc;
    if (int rc = inter_fast_pick_check(st->pick.data(), (int)st->pick.size(), metric)) return rc;
    return inter_pred_check(st->pred.data(), (int)st->pred.size(), pic_width, pic_height, bd, metric);
}

}  // namespace svthost

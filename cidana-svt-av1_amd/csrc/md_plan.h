// md_plan.h — what the mode-decision calls settle on the host before they touch a device: the size helpers, the argument check of each
// of the eight stages (full loop, coefficient rate, transform-type decide, fast loop, fast pick, CfL search, CfL decide, mode-decision
// decide) and, for each of the five calls composed of them, ONE walk over its groups that sizes its scratch, carves it and derives its stages' groups.
// The svt_hip_*.hip files check and plan here, then enqueue.  Plain C++17, no HIP header: a CPU program can include it
// (tests/c/md_plan_host.cpp).
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <string.h>
#include <vector>

#include "../../include/svt_hip_dsp.h"
#include "av1_geom.h"
#include "host_err.h"
#include "quant_params.h"

namespace svthost {
// ---- sizes ------------------------------------------------------------------------------------------------------------------------
// (kTxW / kTxH, kBsizeW / kBsizeH, kSizeGroup, kNumPelsLog2, tx_type_ok and tx_log_scale: av1_geom.h)
inline int log2_of(int v) { int l = 0; while ((1 << l) < v) l++; return l; }
inline size_t align16(size_t v) { return (v + 15) & ~(size_t)15; }
// a side as the coefficient arrays hold it (a 64-sample side packs to 32), and the coefficients of a block: min(W,32) * min(H,32)
inline int packed_side(int v) { return v < 32 ? v : 32; }
inline int coeffs_of(int tx_size) { return packed_side(kTxW[tx_size]) * packed_side(kTxH[tx_size]); }
constexpr int kCflCands = 2 * SVT_HIP_CFL_NALPHA;      // per block: two planes of SVT_HIP_CFL_NALPHA
// the end of the fast loop (fast pick, inter fast pick): the survivors of a list of ncand, the buffers the walk uses for them (one more
// as a scratch when the list is longer), and the blocks a wave takes: one until every wave slot of the device (32 per CU; 256 CUs when
// no device is known) has a block, then up to kPickMaxBpw, which spreads the staging of the rate tables over more blocks
constexpr int kPickMaxBpw = 4;                         // FW_MAX_BPW (kernel_fast_walk.h)
inline int fast_n(int nfl, int ncand) { return nfl < ncand ? nfl : ncand; }
inline int fast_nbuf(int n, int ncand) { return ncand > n ? n + 1 : n; }
inline int pick_bpw(uint32_t nblocks, int num_cu) {
    const uint32_t slots = (uint32_t)(num_cu > 0 ? num_cu : 256) * 32u, b = nblocks / slots;
    return b < 1 ? 1 : (b > (uint32_t)kPickMaxBpw ? kPickMaxBpw : (int)b);
}
inline svtdev::QParams make_qparams(const svt_hip_qrows& q, int log_scale) { return svtdev::make_qparams(q.zbin, q.round, q.quant, q.quant_shift, q.dequant, log_scale); }

// ---- the clauses the checks share ---------------------------------------------------------------------------------------------------
inline int group_list_check(const void* groups, int ngroups) { return ngroups < 0 || (ngroups > 0 && !groups) ? set_err(SVT_HIP_ERR_INVALID, "NULL group list") : SVT_HIP_OK; }
inline int tx_size_check(int g, int tx_size) { return tx_size < 0 || tx_size >= SVT_TX_SIZES_ALL ? set_err(SVT_HIP_ERR_INVALID, "group %d: tx_size %d", g, tx_size) : SVT_HIP_OK; }
// the entries of a per-block table (nblocks * `per` types, candidates or CfL entries) are counted in 31 bits on the device
inline int pairs_check(int g, uint64_t nblocks, uint64_t per, const char* what) { return nblocks * per > 0x7fffffffu ? set_err(SVT_HIP_ERR_INVALID, "group %d: %s too large", g, what) : SVT_HIP_OK; }
inline int flavour_check(int f) { return f != SVT_HIP_FLAVOUR_C && f != SVT_HIP_FLAVOUR_AVX2 ? set_err(SVT_HIP_ERR_INVALID, "flavour %d", f) : SVT_HIP_OK; }
inline int metric_check(int m) { return m != SVT_HIP_FAST_SAD && m != SVT_HIP_FAST_SSD ? set_err(SVT_HIP_ERR_INVALID, "metric %d", m) : SVT_HIP_OK; }
inline int ncand_check(int g, int n) { return n < 1 || n > SVT_HIP_FAST_LOOP_MAX_CANDIDATES ? set_err(SVT_HIP_ERR_INVALID, "group %d: ncand %d (1 .. 64)", g, n) : SVT_HIP_OK; }
// size, count and type list of a (transform size, type list) group, as the full-loop, rate and decide calls all require them (empty
// groups included): a size of the 19, 1 .. 16 types, each defined for the size, none listed twice
inline int group_types_check(int g, int tx_size, int ntypes, const uint8_t* types) {
    if (int rc = tx_size_check(g, tx_size)) return rc;
    if (ntypes < 1 || ntypes > 16) return set_err(SVT_HIP_ERR_INVALID, "group %d: ntypes %d (1 .. 16)", g, ntypes);
    unsigned seen = 0;
    for (int t = 0; t < ntypes; t++) {
        const int ty = types[t];
        if (!tx_type_ok(tx_size, ty)) return set_err(SVT_HIP_ERR_INVALID, "group %d: tx_type %d not defined for tx_size %d", g, ty, tx_size);
        if (seen & (1u << ty)) return set_err(SVT_HIP_ERR_INVALID, "group %d: tx_type %d listed twice", g, ty);
        seen |= 1u << ty;
    }
    return SVT_HIP_OK;
}
// what the fast loop and the fast pick require of a candidate list alike: 1 .. 64 candidates, modes 0 .. 12, angle deltas -3 .. 3
inline int cand_list_check(int g, int ncand, const uint8_t* modes, const int8_t* angle_deltas) {
    if (int rc = ncand_check(g, ncand)) return rc;
    for (int c = 0; c < ncand; c++) {
        if (modes[c] > 12) return set_err(SVT_HIP_ERR_INVALID, "group %d: candidate %d: mode %d", g, c, modes[c]);
        if (angle_deltas[c] < -3 || angle_deltas[c] > 3) return set_err(SVT_HIP_ERR_INVALID, "group %d: candidate %d: angle delta %d", g, c, angle_deltas[c]);
    }
    return SVT_HIP_OK;
}
// one set of quantiser rows (entries [0] and [1] are read) for the log scales 0 .. nscales - 1: the full loop's 3, a CfL plane's 1
inline int qrows_check(const svt_hip_qrows* q, const char* name, int nscales) {
    if (!q || !q->zbin || !q->round || !q->quant || !q->quant_shift || !q->dequant) return set_err(SVT_HIP_ERR_INVALID, "NULL quantiser table (%s)", name);
    for (int i = 0; i < 2; i++) {
        const int qs = q->quant_shift[i];
        if (qs <= 0 || (qs & (qs - 1))) return set_err(SVT_HIP_ERR_INVALID, "%s: quant_shift[%d] = %d is not a power of two", name, i, qs);
        if (q->dequant[i] < 0 || q->round[i] < 0) return set_err(SVT_HIP_ERR_INVALID, "%s: negative quantiser table entry", name);
    }
    for (int ls = 0; ls < nscales; ls++)
        if (!make_qparams(*q, ls).fast_ok)
            return set_err(SVT_HIP_ERR_INVALID, "%s: quantiser table outside the one-product quantiser's range (log_scale %d)", name, ls);
    return SVT_HIP_OK;
}
// size, type and candidate count of one CfL group, as every call of the family requires them (empty groups included)
inline int cfl_size_check(int g, int tx_size, int tx_type, uint32_t nblocks) {
    if (tx_size < 0 || tx_size >= SVT_TX_SIZES_ALL || kTxW[tx_size] > 16 || kTxH[tx_size] > 16)
        return set_err(SVT_HIP_ERR_INVALID, "group %d: tx_size %d is no CfL chroma size (both sides 4 .. 16)", g, tx_size);
    if (tx_type < 0 || !tx_type_ok(tx_size, tx_type)) return set_err(SVT_HIP_ERR_INVALID, "group %d: tx_type %d not defined for tx_size %d", g, tx_type, tx_size);
    return pairs_check(g, nblocks, kCflCands, "nblocks * 66");
}

// ---- the stages' argument checks: every group before the first launch, empty groups' sizes and lists included -----------------------------
inline int full_loop_check(const svt_hip_full_loop_group* groups, int ngroups, int flavour, const svt_hip_qrows& q) {
    if (int rc = group_list_check(groups, ngroups)) return rc;
    if (int rc = flavour_check(flavour)) return rc;
    if (int rc = qrows_check(&q, "quantiser", 3)) return rc;
    for (int g = 0; g < ngroups; g++) {
        const svt_hip_full_loop_group& G = groups[g];
        if (int rc = group_types_check(g, G.tx_size, G.ntypes, G.tx_types)) return rc;
        if (G.nblocks == 0) continue;
        if (int rc = pairs_check(g, G.nblocks, 1, "nblocks")) return rc;
        if (!G.d_src || !G.d_pred || !G.d_iscan || !G.d_dist || !G.d_eob) return set_err(SVT_HIP_ERR_INVALID, "group %d: NULL member", g);
        if (((uintptr_t)G.d_iscan & 7) || ((uintptr_t)G.d_dist & 15) || ((uintptr_t)G.d_qcoeff & 15) || ((uintptr_t)G.d_dqcoeff & 15))
            return set_err(SVT_HIP_ERR_INVALID, "group %d: misaligned buffer (d_iscan 8 bytes, d_dist / d_qcoeff / d_dqcoeff 16 bytes)", g);
        if ((G.d_src_xy && G.src_stride < (uint32_t)kTxW[G.tx_size]) || (G.d_pred_xy && G.pred_stride < (uint32_t)kTxW[G.tx_size]))
            return set_err(SVT_HIP_ERR_INVALID, "group %d: plane stride below the block width", g);
    }
    return SVT_HIP_OK;
}
inline int coeff_rate_check(const svt_hip_coeff_rate_group* groups, int ngroups) {
    if (int rc = group_list_check(groups, ngroups)) return rc;
    for (int g = 0; g < ngroups; g++) {
        const svt_hip_coeff_rate_group& G = groups[g];
        if (int rc = group_types_check(g, G.tx_size, G.ntypes, G.tx_types)) return rc;
        if (G.nblocks == 0) continue;
        if (int rc = pairs_check(g, G.nblocks, G.ntypes, "nblocks * ntypes")) return rc;
        if (!G.d_qcoeff || !G.d_eob || !G.d_iscan || !G.d_txb_skip_ctx || !G.d_dc_sign_ctx || !G.d_coeff_cost || !G.d_eob_cost || !G.d_bits)
            return set_err(SVT_HIP_ERR_INVALID, "group %d: NULL member", g);
        if (((uintptr_t)G.d_qcoeff & 15) || ((uintptr_t)G.d_iscan & 7) || ((uintptr_t)G.d_bits & 7) || ((uintptr_t)G.d_eob & 1) ||
            ((uintptr_t)G.d_type_bits & 3) || ((uintptr_t)G.d_coeff_cost & 3) || ((uintptr_t)G.d_eob_cost & 3))
            return set_err(SVT_HIP_ERR_INVALID, "group %d: misaligned buffer (d_qcoeff 16 bytes, d_iscan / d_bits 8, the int32 tables 4, d_eob 2)", g);
    }
    return SVT_HIP_OK;
}
inline int tx_decide_check(const svt_hip_tx_decide_group* groups, int ngroups) {
    if (int rc = group_list_check(groups, ngroups)) return rc;
    for (int g = 0; g < ngroups; g++) {
        const svt_hip_tx_decide_group& G = groups[g];
        if (int rc = group_types_check(g, G.tx_size, G.ntypes, G.tx_types)) return rc;
        if (G.nblocks == 0) continue;
        if (int rc = pairs_check(g, G.nblocks, G.ntypes, "nblocks * ntypes")) return rc;
        if (!G.d_dist || !G.d_eob || !G.d_bits || !G.d_decision) return set_err(SVT_HIP_ERR_INVALID, "group %d: NULL member", g);
        if ((G.d_best_qcoeff && !G.d_qcoeff) || (G.d_best_dqcoeff && !G.d_dqcoeff))
            return set_err(SVT_HIP_ERR_INVALID, "group %d: d_best_qcoeff / d_best_dqcoeff without its input", g);
        if ((G.d_best_qcoeff && G.d_best_qcoeff == G.d_qcoeff) || (G.d_best_dqcoeff && G.d_best_dqcoeff == G.d_dqcoeff))
            return set_err(SVT_HIP_ERR_INVALID, "group %d: d_best_qcoeff / d_best_dqcoeff is its own input", g);
        if (((uintptr_t)G.d_dist & 15) || ((uintptr_t)G.d_qcoeff & 15) || ((uintptr_t)G.d_dqcoeff & 15) || ((uintptr_t)G.d_best_qcoeff & 15) ||
            ((uintptr_t)G.d_best_dqcoeff & 15) || ((uintptr_t)G.d_bits & 7) || ((uintptr_t)G.d_decision & 7) || ((uintptr_t)G.d_eob & 1))
            return set_err(SVT_HIP_ERR_INVALID, "group %d: misaligned buffer (d_dist and the coefficient arrays 16 bytes, d_bits / d_decision 8, d_eob 2)", g);
    }
    return SVT_HIP_OK;
}
inline int fast_loop_check(const svt_hip_fast_loop_group* groups, int ngroups, int metric, int flavour) {
    if (int rc = group_list_check(groups, ngroups)) return rc;
    if (int rc = metric_check(metric)) return rc;
    if (int rc = flavour_check(flavour)) return rc;
    for (int g = 0; g < ngroups; g++) {
        const svt_hip_fast_loop_group& G = groups[g];
        if (int rc = tx_size_check(g, G.tx_size)) return rc;
        const int w = kTxW[G.tx_size], h = kTxH[G.tx_size];
        if (metric == SVT_HIP_FAST_SSD && flavour == SVT_HIP_FLAVOUR_AVX2 && w != h)
            return set_err(SVT_HIP_ERR_INVALID, "group %d: AVX2-flavour SSD is defined for square sizes only (%dx%d)", g, w, h);
        if (int rc = cand_list_check(g, G.ncand, G.modes, G.angle_deltas)) return rc;
        for (int c = 0; c < G.ncand; c++)                                           // (the fast pick does not ask this of its list)
            if (G.angle_deltas[c] != 0 && (G.modes[c] < 1 || G.modes[c] > 8))
                return set_err(SVT_HIP_ERR_INVALID, "group %d: candidate %d: angle delta on mode %d", g, c, G.modes[c]);
        if (G.nblocks == 0) continue;
        if (int rc = pairs_check(g, G.nblocks, 1, "nblocks")) return rc;
        if (!G.d_src || !G.d_top_neigh || !G.d_left_neigh || !G.d_blocks || !G.d_dist) return set_err(SVT_HIP_ERR_INVALID, "group %d: NULL member", g);
        if (((uintptr_t)G.d_dist & 7) || ((uintptr_t)G.d_pred & 15))
            return set_err(SVT_HIP_ERR_INVALID, "group %d: misaligned output (d_dist 8 bytes, d_pred 16 bytes)", g);
        if (G.neigh_pitch < 1 + 2 * (w > h ? w : h))
            return set_err(SVT_HIP_ERR_INVALID, "group %d: neigh_pitch %d < %d", g, G.neigh_pitch, 1 + 2 * (w > h ? w : h));
        if (G.d_src_xy && G.src_stride < (uint32_t)w) return set_err(SVT_HIP_ERR_INVALID, "group %d: src_stride below the block width", g);
    }
    return SVT_HIP_OK;
}
inline int fast_pick_check(const svt_hip_fast_pick_group* groups, int ngroups, int metric) {
    if (int rc = group_list_check(groups, ngroups)) return rc;
    if (int rc = metric_check(metric)) return rc;
    for (int g = 0; g < ngroups; g++) {
        const svt_hip_fast_pick_group& G = groups[g];
        if (int rc = tx_size_check(g, G.tx_size)) return rc;
        if (G.bsize < 0 || G.bsize > 21 || G.bsize_uv < 0 || G.bsize_uv > 21)
            return set_err(SVT_HIP_ERR_INVALID, "group %d: bsize %d / bsize_uv %d (0 .. 21)", g, G.bsize, G.bsize_uv);
        if (int rc = cand_list_check(g, G.ncand, G.modes, G.angle_deltas)) return rc;
        if (G.nfl < 1 || G.nfl > SVT_HIP_MAX_NFL) return set_err(SVT_HIP_ERR_INVALID, "group %d: nfl %d (1 .. %d)", g, G.nfl, SVT_HIP_MAX_NFL);
        if (G.ac_dequant_q3 < 0) return set_err(SVT_HIP_ERR_INVALID, "group %d: ac_dequant_q3 %d", g, G.ac_dequant_q3);
        for (int c = 0; c < G.ncand; c++) {
            if (G.uv_modes[c] > 13) return set_err(SVT_HIP_ERR_INVALID, "group %d: candidate %d: uv mode %d", g, c, G.uv_modes[c]);
            if (G.uv_angle_deltas[c] < -3 || G.uv_angle_deltas[c] > 3) return set_err(SVT_HIP_ERR_INVALID, "group %d: candidate %d: uv angle delta %d", g, c, G.uv_angle_deltas[c]);
        }
        if (G.nblocks == 0) continue;
        if (int rc = pairs_check(g, G.nblocks, G.ncand, "nblocks * ncand")) return rc;
        if (!G.d_dist || !G.d_blk || !G.d_rates || !G.d_cand || !G.d_sorted || !G.d_cost || !G.d_rate || !G.d_ref_fast_cost)
            return set_err(SVT_HIP_ERR_INVALID, "group %d: NULL member", g);
        if ((G.d_pred_out && !G.d_pred) || (G.d_src_xy_out && !G.d_src_xy))
            return set_err(SVT_HIP_ERR_INVALID, "group %d: d_pred_out / d_src_xy_out without its input", g);
        if (G.d_pred_out && G.d_pred_out == G.d_pred) return set_err(SVT_HIP_ERR_INVALID, "group %d: d_pred_out is its own input", g);
        if (((uintptr_t)G.d_pred & 15) || ((uintptr_t)G.d_pred_out & 15) || ((uintptr_t)G.d_dist & 7) || ((uintptr_t)G.d_dist_cb & 7) ||
            ((uintptr_t)G.d_dist_cr & 7) || ((uintptr_t)G.d_blk & 7) || ((uintptr_t)G.d_cost & 7) || ((uintptr_t)G.d_ref_fast_cost & 7) ||
            ((uintptr_t)G.d_all_cost & 7) || ((uintptr_t)G.d_rates & 3) || ((uintptr_t)G.d_rate & 3) || ((uintptr_t)G.d_src_xy & 3) ||
            ((uintptr_t)G.d_src_xy_out & 3))
            return set_err(SVT_HIP_ERR_INVALID, "group %d: misaligned buffer (d_pred / d_pred_out 16 bytes, the 8-byte arrays and d_blk 8, d_rates / d_rate / d_src_xy 4)", g);
    }
    return SVT_HIP_OK;
}
// the CfL search's own arguments; its rate stage is a coefficient-rate call over the groups cfl_search_walk derives
inline int cfl_search_check(const svt_hip_cfl_search_group* groups, int ngroups, int flavour, const svt_hip_qrows* q_cb, const svt_hip_qrows* q_cr) {
    if (int rc = group_list_check(groups, ngroups)) return rc;
    for (int g = 0; g < ngroups; g++)
        if (int rc = cfl_size_check(g, groups[g].tx_size, groups[g].tx_type, groups[g].nblocks)) return rc;
    if (int rc = flavour_check(flavour)) return rc;
    if (int rc = qrows_check(q_cb, "q_cb", 1)) return rc;
    if (int rc = qrows_check(q_cr, "q_cr", 1)) return rc;
    for (int g = 0; g < ngroups; g++) {
        const svt_hip_cfl_search_group& G = groups[g];
        if (G.nblocks == 0) continue;
        const uint32_t w = (uint32_t)kTxW[G.tx_size];
        if (!G.d_luma_recon || !G.d_src[0] || !G.d_src[1] || !G.d_pred[0] || !G.d_pred[1] || !G.d_xy || !G.d_iscan || !G.d_txb_skip_ctx[0] ||
            !G.d_txb_skip_ctx[1] || !G.d_dc_sign_ctx[0] || !G.d_dc_sign_ctx[1] || !G.d_coeff_cost || !G.d_eob_cost || !G.d_dist || !G.d_bits || !G.d_eob)
            return set_err(SVT_HIP_ERR_INVALID, "group %d: NULL member", g);
        if (((uintptr_t)G.d_iscan & 7) || ((uintptr_t)G.d_dist & 15) || ((uintptr_t)G.d_bits & 7) || ((uintptr_t)G.d_eob & 1) || ((uintptr_t)G.d_xy & 3))
            return set_err(SVT_HIP_ERR_INVALID, "group %d: misaligned buffer (d_dist 16 bytes, d_iscan / d_bits 8, d_xy 4, d_eob 2)", g);
        if (G.luma_stride < 2 * w || G.src_stride[0] < w || G.src_stride[1] < w || G.pred_stride[0] < w || G.pred_stride[1] < w)
            return set_err(SVT_HIP_ERR_INVALID, "group %d: plane stride below the block width", g);
    }
    return SVT_HIP_OK;
}
inline int cfl_decide_check(const svt_hip_cfl_decide_group* groups, int ngroups) {
    if (int rc = group_list_check(groups, ngroups)) return rc;
    for (int g = 0; g < ngroups; g++) {
        const svt_hip_cfl_decide_group& G = groups[g];
        if (G.nblocks == 0) continue;
        if (int rc = pairs_check(g, G.nblocks, kCflCands, "nblocks * 66")) return rc;
        if (!G.d_dist || !G.d_bits || !G.d_alpha_rate || !G.d_cfl_mode_bits || !G.d_dc_mode_bits || !G.d_decision)
            return set_err(SVT_HIP_ERR_INVALID, "group %d: NULL member", g);
        if (((uintptr_t)G.d_dist & 15) || ((uintptr_t)G.d_bits & 7) || ((uintptr_t)G.d_decision & 7) || ((uintptr_t)G.d_alpha_rate & 3) ||
            ((uintptr_t)G.d_cfl_mode_bits & 3) || ((uintptr_t)G.d_dc_mode_bits & 3) || ((uintptr_t)G.d_alpha_q3_cb & 3) || ((uintptr_t)G.d_alpha_q3_cr & 3))
            return set_err(SVT_HIP_ERR_INVALID, "group %d: misaligned buffer (d_dist 16 bytes, d_bits / d_decision 8, the int32 arrays 4)", g);
    }
    return SVT_HIP_OK;
}
// The decide of mode decision (svt_hip_md_decide_frame).  Its geometry comes from the block size alone: per plane (Y, Cb, Cr; 4:2:0, a
// chroma side at least 4) the samples of a prediction and the coefficients of the plane's one transform block.
struct MdGeom { int w[3], h[3], pred_bytes[3], ncoeff[3]; };
inline MdGeom md_geom(int bsize) {
    MdGeom m;
    for (int p = 0; p < 3; p++) {
        const int w = p ? (kBsizeW[bsize] / 2 < 4 ? 4 : kBsizeW[bsize] / 2) : kBsizeW[bsize], h = p ? (kBsizeH[bsize] / 2 < 4 ? 4 : kBsizeH[bsize] / 2) : kBsizeH[bsize];
        m.w[p] = w; m.h[p] = h; m.pred_bytes[p] = w * h; m.ncoeff[p] = packed_side(w) * packed_side(h);
    }
    return m;
}
inline bool md_bsize_ok(int bsize) { return bsize >= 0 && bsize <= 21 && (bsize < 13 || bsize > 15); }
// log2 blocks per wave-unit: the largest gather of the size (luma's prediction or coefficients) at most 2^9 quads, the unit's costs
// (rows of n + 1 words) inside the wave's tile of kMdTileWords, 64 blocks (one owning lane each) at most
constexpr int kMdTileWords = 64 * 17;                  // MD_COST_WORDS (kernel_md_decide.h)
inline int md_decide_bpul(int bsize, int n) {
    const MdGeom m = md_geom(bsize);
    const int py = log2_of(m.pred_bytes[0]) - 4, cy = log2_of(m.ncoeff[0]) - 2;
    int bpul = 9 - (py > cy ? py : cy);
    if (bpul > 6) bpul = 6;
    while ((n + 1) << bpul > kMdTileWords) bpul--;
    return bpul;
}
// the scalars of a group, as the decide and the composed search require them of every group, empty ones included
inline int md_scalars_check(int g, const svt_hip_md_decide_group& G) {
    if (!md_bsize_ok(G.bsize)) return set_err(SVT_HIP_ERR_INVALID, "group %d: bsize %d (0 .. 21 without the 128-wide 13 .. 15)", g, G.bsize);
    if (G.n < 1 || G.n > SVT_HIP_MAX_NFL) return set_err(SVT_HIP_ERR_INVALID, "group %d: n %d (1 .. %d)", g, G.n, SVT_HIP_MAX_NFL);
    if (G.ninter < 0 || G.nintra < 0 || G.ninter + G.nintra < 1 || G.ninter + G.nintra > SVT_HIP_FAST_LOOP_MAX_CANDIDATES)
        return set_err(SVT_HIP_ERR_INVALID, "group %d: ninter %d + nintra %d (1 .. 64 candidates)", g, G.ninter, G.nintra);
    for (int c = 0; c < G.nintra; c++)
        if (G.modes[c] > 12) return set_err(SVT_HIP_ERR_INVALID, "group %d: intra candidate %d: mode %d", g, c, G.modes[c]);
    if (G.full_loop_escape < 0 || G.full_loop_escape > 2) return set_err(SVT_HIP_ERR_INVALID, "group %d: full_loop_escape %d (0 .. 2)", g, G.full_loop_escape);
    return pairs_check(g, G.nblocks, (uint64_t)G.n, "nblocks * n");
}
inline int md_decide_check(const svt_hip_md_decide_group* groups, int ngroups) {
    if (int rc = group_list_check(groups, ngroups)) return rc;
    for (int g = 0; g < ngroups; g++) {
        const svt_hip_md_decide_group& G = groups[g];
        if (int rc = md_scalars_check(g, G)) return rc;
        if (G.nblocks == 0) continue;
        if (!G.d_luma || !G.d_rate || !G.d_cand || !G.d_blk || !G.d_rates || !G.d_decision) return set_err(SVT_HIP_ERR_INVALID, "group %d: NULL member", g);
        if (G.ninter > 0 && !G.d_cand_out) return set_err(SVT_HIP_ERR_INVALID, "group %d: d_cand_out is required with ninter > 0", g);
        const int nchroma = !!G.d_dist_cb + !!G.d_dist_cr + !!G.d_bits_cb + !!G.d_bits_cr + !!G.d_eob_cb + !!G.d_eob_cr;
        if (nchroma != 0 && nchroma != 6) return set_err(SVT_HIP_ERR_INVALID, "group %d: the six chroma arrays are given all or none (Cb without Cr)", g);
        uintptr_t a16 = (uintptr_t)G.d_inter_blk | (uintptr_t)G.d_best_inter_blk;
        if (G.d_best_inter_blk && (!G.d_inter_blk || G.d_best_inter_blk == G.d_inter_blk))
            return set_err(SVT_HIP_ERR_INVALID, "group %d: d_best_inter_blk without its input or equal to it", g);
        for (int p = 0; p < 3; p++) {
            const void* in[3] = {G.d_pred[p], G.d_qcoeff[p], G.d_dqcoeff[p]};
            const void* out[3] = {G.d_best_pred[p], G.d_best_qcoeff[p], G.d_best_dqcoeff[p]};
            for (int a = 0; a < 3; a++) {
                if (out[a] && (!in[a] || out[a] == in[a])) return set_err(SVT_HIP_ERR_INVALID, "group %d: plane %d: a gather without its input or equal to it", g, p);
                a16 |= (uintptr_t)in[a] | (uintptr_t)out[a];
            }
        }
        const uintptr_t a8 = (uintptr_t)G.d_luma | (uintptr_t)G.d_dist_cb | (uintptr_t)G.d_dist_cr | (uintptr_t)G.d_bits_cb | (uintptr_t)G.d_bits_cr |
                             (uintptr_t)G.d_cfl | (uintptr_t)G.d_decision | (uintptr_t)G.d_full_cost;
        const uintptr_t a4 = (uintptr_t)G.d_rate | (uintptr_t)G.d_rates | (uintptr_t)G.d_blk | (uintptr_t)G.d_cand_out;
        if ((a16 & 15) || (a8 & 7) || (a4 & 3) || (((uintptr_t)G.d_eob_cb | (uintptr_t)G.d_eob_cr) & 1))
            return set_err(SVT_HIP_ERR_INVALID, "group %d: misaligned buffer (prediction, coefficient and inter-record arrays 16 bytes, records and uint64 arrays 8, d_rate / d_rates / d_blk / d_cand_out 4, eobs 2)", g);
    }
    return SVT_HIP_OK;
}

// ---- the composed calls: scratch and stage groups ------------------------------------------------------------------------------------------
// Hands out the pieces of a scratch in the order they are asked for, each rounded up to 16 bytes.  Without a base it only adds them up
// and every piece is NULL, so the walk that sizes a call's scratch is the walk that carves it: a layout is stated once, as the
// piece() calls of its walk in the order include/svt_hip_dsp.h documents.
struct Carver {
    char* base;
    size_t used = 0;
    template <typename T> void piece(T*& p, size_t bytes) { p = base ? (T*)(base + used) : nullptr; used += align16(bytes); }
    // a piece that a later part of the same walk asks only "is it there?" of: while sizing it is not NULL either (the Carver's own address,
    // which nothing dereferences: a sizing walk derives no stage groups)
    template <typename T> void piece_present(T*& p, size_t bytes) { piece(p, bytes); if (!base) p = (T*)this; }
};
// A walk checks what the carving needs of each group (sizes and counts), carves, and with `st` appends the groups of the call's stages.
// plan_stages: the walk without a base sizes the scratch, the scratch is accepted or refused, and only then the walk runs over it.  The
// walk is any callable int(const G*, int, Carver&, St*): a function, or a lambda that binds what else the call's walk depends on.
template <typename Walk, typename G>
size_t scratch_bytes_of(Walk&& walk, const G* groups, int ngroups) {
    Carver size{nullptr};
    return walk(groups, ngroups, size, nullptr) == SVT_HIP_OK ? size.used : 0;
}
template <typename Walk, typename G, typename St>
int plan_stages(Walk&& walk, const G* groups, int ngroups, void* d_scratch, size_t scratch_bytes, St* st) {
    Carver size{nullptr};
    if (int rc = walk(groups, ngroups, size, (St*)nullptr)) return rc;
    if (size.used && (!d_scratch || ((uintptr_t)d_scratch & 15) || scratch_bytes < size.used))
        return set_err(SVT_HIP_ERR_INVALID, "scratch NULL, not 16-byte aligned or below the call's *_scratch_bytes()");
    Carver carve{(char*)d_scratch};
    return walk(groups, ngroups, carve, st);
}

// svt_hip_tx_search_frame: full loop -> coefficient rate -> decide.  Per non-empty group dist, eob, bits, qcoeff (each but bits only
// when not supplied) and dqcoeff (only when not supplied and d_best_dqcoeff asks for it).
struct TxSearchStages { std::vector<svt_hip_full_loop_group> fl; std::vector<svt_hip_coeff_rate_group> cr; std::vector<svt_hip_tx_decide_group> td; };
inline int tx_search_walk(const svt_hip_tx_search_group* groups, int ngroups, Carver& sc, TxSearchStages* st) {
    if (int rc = group_list_check(groups, ngroups)) return rc;
    for (int g = 0; g < ngroups; g++) {
        const svt_hip_tx_search_group& G = groups[g];
        svt_hip_full_loop_group F = G.fl;
        if (int rc = group_types_check(g, F.tx_size, F.ntypes, F.tx_types)) return rc;
        if (int rc = pairs_check(g, F.nblocks, F.ntypes, "nblocks * ntypes")) return rc;
        const size_t pairs = (size_t)F.nblocks * (size_t)F.ntypes, coeff_bytes = pairs * (size_t)coeffs_of(F.tx_size) * sizeof(int32_t);
        uint64_t* bits = nullptr;
        if (pairs) {
            if (!F.d_dist) sc.piece(F.d_dist, pairs * 16);
            if (!F.d_eob) sc.piece(F.d_eob, pairs * 2);
            sc.piece(bits, pairs * 8);
            if (!F.d_qcoeff) sc.piece(F.d_qcoeff, coeff_bytes);
            if (!F.d_dqcoeff && G.d_best_dqcoeff) sc.piece(F.d_dqcoeff, coeff_bytes);
        }
        if (!st) continue;
        svt_hip_coeff_rate_group C{};
        C.tx_size = F.tx_size; C.ntypes = F.ntypes; memcpy(C.tx_types, F.tx_types, sizeof(C.tx_types)); C.nblocks = F.nblocks;
        C.d_qcoeff = F.d_qcoeff; C.d_eob = F.d_eob; C.d_iscan = F.d_iscan; C.d_txb_skip_ctx = G.d_txb_skip_ctx; C.d_dc_sign_ctx = G.d_dc_sign_ctx;
        C.d_type_bits = G.d_type_bits; C.d_coeff_cost = G.d_coeff_cost; C.d_eob_cost = G.d_eob_cost; C.d_bits = bits;
        svt_hip_tx_decide_group D{};
        D.tx_size = F.tx_size; D.ntypes = F.ntypes; memcpy(D.tx_types, F.tx_types, sizeof(D.tx_types)); D.nblocks = F.nblocks;
        D.lambda = G.lambda; D.d_dist = F.d_dist; D.d_eob = F.d_eob; D.d_bits = bits; D.d_qcoeff = F.d_qcoeff; D.d_dqcoeff = F.d_dqcoeff;
        D.d_decision = G.d_decision; D.d_best_qcoeff = G.d_best_qcoeff; D.d_best_dqcoeff = G.d_best_dqcoeff;
        st->fl.push_back(F); st->cr.push_back(C); st->td.push_back(D);
    }
    return SVT_HIP_OK;
}

// svt_hip_intra_fast_search_frame: fast loop (luma; Cb, Cr) -> pick.  Per non-empty group luma's dist when NULL, Cb's and Cr's likewise
// when use_chroma, luma's predictions when NULL and the pick's d_pred_out asks for them.
struct FastSearchStages { std::vector<svt_hip_fast_loop_group> fl, flc; std::vector<svt_hip_fast_pick_group> fp; };      // flc: Cb, Cr of the groups with chroma
inline int fast_search_walk(const svt_hip_intra_fast_search_group* groups, int ngroups, Carver& sc, FastSearchStages* st) {
    if (int rc = group_list_check(groups, ngroups)) return rc;
    for (int g = 0; g < ngroups; g++) {
        const svt_hip_intra_fast_search_group& G = groups[g];
        svt_hip_fast_loop_group L = G.luma, CB = G.cb, CR = G.cr;
        if (int rc = tx_size_check(g, L.tx_size)) return rc;
        if (int rc = ncand_check(g, L.ncand)) return rc;
        if (G.use_chroma && (CB.nblocks != L.nblocks || CR.nblocks != L.nblocks || CB.ncand != L.ncand || CR.ncand != L.ncand))
            return set_err(SVT_HIP_ERR_INVALID, "group %d: the chroma groups' nblocks / ncand differ from luma's", g);
        if (int rc = pairs_check(g, L.nblocks, L.ncand, "nblocks * ncand")) return rc;
        const size_t pairs = (size_t)L.nblocks * (size_t)L.ncand;
        if (pairs) {
            if (!L.d_dist) sc.piece(L.d_dist, pairs * 8);
            if (G.use_chroma && !CB.d_dist) sc.piece(CB.d_dist, pairs * 8);
            if (G.use_chroma && !CR.d_dist) sc.piece(CR.d_dist, pairs * 8);
            if (!L.d_pred && G.pick.d_pred_out) sc.piece(L.d_pred, pairs * (size_t)(kTxW[L.tx_size] * kTxH[L.tx_size]));
        }
        if (!st) continue;
        svt_hip_fast_pick_group P = G.pick;
        P.tx_size = L.tx_size; P.nblocks = L.nblocks; P.ncand = L.ncand;
        memcpy(P.modes, L.modes, sizeof(P.modes)); memcpy(P.angle_deltas, L.angle_deltas, sizeof(P.angle_deltas));
        P.d_dist = L.d_dist; P.d_dist_cb = G.use_chroma ? CB.d_dist : nullptr; P.d_dist_cr = G.use_chroma ? CR.d_dist : nullptr;
        P.d_pred = L.d_pred;
        if (L.d_src_xy) P.d_src_xy = L.d_src_xy;
        st->fl.push_back(L); st->fp.push_back(P);
        if (G.use_chroma) { st->flc.push_back(CB); st->flc.push_back(CR); }
    }
    return SVT_HIP_OK;
}

// svt_hip_cfl_search_frame: the table -> coefficient rate, which reads (block, plane, a) as a block with one type.  Per non-empty group
// every candidate's qcoeff, then its txb_skip and dc_sign context bytes.  svt_hip_cfl_pick_frame: search -> decide; first, per
// non-empty group, dist, bits and eob (each only when not supplied), then the search's pieces.
struct CflStages { std::vector<svt_hip_cfl_search_group> sg; std::vector<svt_hip_coeff_rate_group> cr; std::vector<svt_hip_cfl_decide_group> dg; };
inline int cfl_search_walk(const svt_hip_cfl_search_group* groups, int ngroups, Carver& sc, CflStages* st) {
    if (int rc = group_list_check(groups, ngroups)) return rc;
    for (int g = 0; g < ngroups; g++) {
        const svt_hip_cfl_search_group& G = groups[g];
        if (int rc = cfl_size_check(g, G.tx_size, G.tx_type, G.nblocks)) return rc;
        svt_hip_coeff_rate_group C{};
        C.tx_size = G.tx_size; C.ntypes = 1; C.tx_types[0] = (uint8_t)G.tx_type;
        C.nblocks = G.nblocks * (uint32_t)kCflCands;
        if (G.nblocks) {
            sc.piece(C.d_qcoeff, (size_t)C.nblocks * (size_t)coeffs_of(G.tx_size) * sizeof(int32_t));
            sc.piece(C.d_txb_skip_ctx, C.nblocks);
            sc.piece(C.d_dc_sign_ctx, C.nblocks);
            C.d_eob = G.d_eob; C.d_iscan = G.d_iscan; C.d_coeff_cost = G.d_coeff_cost; C.d_eob_cost = G.d_eob_cost; C.d_bits = G.d_bits;
        }
        if (st) st->cr.push_back(C);
    }
    return SVT_HIP_OK;
}
inline int cfl_pick_walk(const svt_hip_cfl_pick_group* groups, int ngroups, Carver& sc, CflStages* st) {
    if (int rc = group_list_check(groups, ngroups)) return rc;
    std::vector<svt_hip_cfl_search_group> sg;
    for (int g = 0; g < ngroups; g++) {
        const svt_hip_cfl_pick_group& G = groups[g];
        svt_hip_cfl_search_group S = G.search;
        if (int rc = cfl_size_check(g, S.tx_size, S.tx_type, S.nblocks)) return rc;
        const size_t cands = (size_t)S.nblocks * (size_t)kCflCands;
        if (cands) {
            if (!S.d_dist) sc.piece(S.d_dist, cands * 16);
            if (!S.d_bits) sc.piece(S.d_bits, cands * 8);
            if (!S.d_eob) sc.piece(S.d_eob, cands * 2);
        }
        sg.push_back(S);
        if (!st) continue;
        svt_hip_cfl_decide_group D{};
        D.nblocks = S.nblocks; D.lambda = G.lambda; D.d_dist = S.d_dist; D.d_bits = S.d_bits; D.d_alpha_rate = G.d_alpha_rate;
        D.d_cfl_mode_bits = G.d_cfl_mode_bits; D.d_dc_mode_bits = G.d_dc_mode_bits; D.d_decision = G.d_decision;
        D.d_alpha_q3_cb = G.d_alpha_q3_cb; D.d_alpha_q3_cr = G.d_alpha_q3_cr;
        st->dg.push_back(D);
    }
    if (int rc = cfl_search_walk(sg.data(), ngroups, sc, st)) return rc;
    if (st) st->sg = std::move(sg);
    return SVT_HIP_OK;
}

// svt_hip_md_search_frame: luma transform-type search -> (Cb, Cr full loop -> coefficient rate) -> decide.  Per non-empty group the
// luma record, luma's best coefficients when a gather asks for them, then per chroma plane dist, eob, bits, qcoeff and (when its gather
// asks) dqcoeff, each only when not supplied; after all groups the luma search's own pieces (tx_search_walk).
struct MdSearchStages {
    TxSearchStages tx;
    std::vector<svt_hip_full_loop_group> flc; std::vector<svt_hip_coeff_rate_group> crc;        // Cb, Cr of the groups with chroma
    std::vector<svt_hip_md_decide_group> md;
};
inline int md_search_walk(const svt_hip_md_search_group* groups, int ngroups, Carver& sc, MdSearchStages* st) {
    if (int rc = group_list_check(groups, ngroups)) return rc;
    std::vector<svt_hip_tx_search_group> luma;
    for (int g = 0; g < ngroups; g++) {
        const svt_hip_md_search_group& G = groups[g];
        svt_hip_md_decide_group M = G.md;
        svt_hip_tx_search_group L = G.luma;
        if (int rc = md_scalars_check(g, M)) return rc;
        const uint32_t pairs = M.nblocks * (uint32_t)M.n;                           // (md_scalars_check: below 2^31)
        if (int rc = group_types_check(g, L.fl.tx_size, L.fl.ntypes, L.fl.tx_types)) return rc;
        bool dct = false;
        for (int t = 0; t < L.fl.ntypes; t++) dct |= L.fl.tx_types[t] == SVT_DCT_DCT;
        if (!dct) return set_err(SVT_HIP_ERR_INVALID, "group %d: the luma type list has no DCT_DCT", g);
        const MdGeom m = md_geom(M.bsize);
        if (kTxW[L.fl.tx_size] != m.w[0] || kTxH[L.fl.tx_size] != m.h[0]) return set_err(SVT_HIP_ERR_INVALID, "group %d: luma tx_size %d is not the block size's", g, L.fl.tx_size);
        if (L.fl.nblocks != pairs) return set_err(SVT_HIP_ERR_INVALID, "group %d: luma nblocks %u is not md.nblocks * md.n", g, L.fl.nblocks);
        svt_hip_full_loop_group C[2] = {G.cb, G.cr};
        uint64_t* cbits[2] = {G.d_bits_c[0], G.d_bits_c[1]};
        if (G.use_chroma)
            for (int p = 0; p < 2; p++) {
                if (int rc = group_types_check(g, C[p].tx_size, C[p].ntypes, C[p].tx_types)) return rc;
                if (C[p].ntypes != 1 || C[p].nblocks != pairs || kTxW[C[p].tx_size] != m.w[1 + p] || kTxH[C[p].tx_size] != m.h[1 + p])
                    return set_err(SVT_HIP_ERR_INVALID, "group %d: chroma plane %d: ntypes %d (1), nblocks %u (md.nblocks * md.n) or a tx_size %d that is not the block size's", g, p, C[p].ntypes, C[p].nblocks, C[p].tx_size);
            }
        if (pairs) {
            if (!L.d_decision) sc.piece(L.d_decision, (size_t)pairs * sizeof(svt_hip_tx_decision));
            if (!L.d_best_qcoeff && M.d_best_qcoeff[0]) sc.piece(L.d_best_qcoeff, (size_t)pairs * (size_t)m.ncoeff[0] * sizeof(int32_t));
            // (tx_search_walk below keeps the luma dqcoeff exactly when d_best_dqcoeff is there, while sizing too)
            if (!L.d_best_dqcoeff && M.d_best_dqcoeff[0]) sc.piece_present(L.d_best_dqcoeff, (size_t)pairs * (size_t)m.ncoeff[0] * sizeof(int32_t));
            if (G.use_chroma)
                for (int p = 0; p < 2; p++) {
                    const size_t coeff_bytes = (size_t)pairs * (size_t)m.ncoeff[1 + p] * sizeof(int32_t);
                    if (!C[p].d_dist) sc.piece(C[p].d_dist, (size_t)pairs * 16);
                    if (!C[p].d_eob) sc.piece(C[p].d_eob, (size_t)pairs * 2);
                    if (!cbits[p]) sc.piece(cbits[p], (size_t)pairs * 8);
                    if (!C[p].d_qcoeff) sc.piece(C[p].d_qcoeff, coeff_bytes);
                    if (!C[p].d_dqcoeff && M.d_best_dqcoeff[1 + p]) sc.piece(C[p].d_dqcoeff, coeff_bytes);
                }
        }
        luma.push_back(L);
        if (!st) continue;
        M.d_luma = L.d_decision; M.d_qcoeff[0] = L.d_best_qcoeff; M.d_dqcoeff[0] = L.d_best_dqcoeff;
        M.d_dist_cb = M.d_dist_cr = M.d_bits_cb = M.d_bits_cr = nullptr; M.d_eob_cb = M.d_eob_cr = nullptr;
        M.d_qcoeff[1] = M.d_qcoeff[2] = M.d_dqcoeff[1] = M.d_dqcoeff[2] = nullptr;
        if (G.use_chroma) {
            M.d_dist_cb = C[0].d_dist; M.d_dist_cr = C[1].d_dist; M.d_eob_cb = C[0].d_eob; M.d_eob_cr = C[1].d_eob;
            M.d_bits_cb = cbits[0]; M.d_bits_cr = cbits[1];
            for (int p = 0; p < 2; p++) {
                M.d_qcoeff[1 + p] = C[p].d_qcoeff; M.d_dqcoeff[1 + p] = C[p].d_dqcoeff;
                svt_hip_coeff_rate_group R{};
                R.tx_size = C[p].tx_size; R.ntypes = 1; R.tx_types[0] = C[p].tx_types[0]; R.nblocks = pairs;
                R.d_qcoeff = C[p].d_qcoeff; R.d_eob = C[p].d_eob; R.d_iscan = C[p].d_iscan; R.d_txb_skip_ctx = G.d_txb_skip_ctx_c[p];
                R.d_dc_sign_ctx = G.d_dc_sign_ctx_c[p]; R.d_coeff_cost = G.d_coeff_cost_uv; R.d_eob_cost = G.d_eob_cost_uv; R.d_bits = cbits[p];
                st->flc.push_back(C[p]); st->crc.push_back(R);
            }
        }
        st->md.push_back(M);
    }
    return tx_search_walk(luma.data(), ngroups, sc, st ? &st->tx : nullptr);
}
}  // namespace svthost

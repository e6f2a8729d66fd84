// svt_hip_md_decide.hip — svt_hip_md_decide_frame: the full cost of every (block, slot), the full loop's early exit, the best candidate
// of every block and the winner's prediction, coefficients and inter record (md_decide_kernel, kernel_md_decide.h), one launch per
// MD_MAX_GROUPS groups; svt_hip_md_search_frame, a picture's mode decision for a given partition as host composition: luma transform-type
// search -> chroma full loop -> chroma coefficient rate -> decide on one stream.  What is left here: the decide's launch geometry,
// group-table fill and launch and the entry points; the checks, the scratch layout and the stages' groups are md_plan.h's.
#include <stddef.h>

#include "host_common.h"
#include "kernel_md_decide.h"

using namespace svtdev;
using namespace svthost;

static_assert(sizeof(svt_hip_md_decision) == 8 * MD_DEC_WORDS && alignof(svt_hip_md_decision) == 8, "md_decide_kernel stores the record as nine words");
static_assert(offsetof(svt_hip_md_decision, full_distortion) == 40 && offsetof(svt_hip_md_decision, eob) == 44 && offsetof(svt_hip_md_decision, slot) == 50 &&
              offsetof(svt_hip_md_decision, y_has_coeff) == 56 && offsetof(svt_hip_md_decision, cfl_alpha_signs) == 64, "the words md_decide_kernel packs");
static_assert(sizeof(svt_hip_md_blk) == 4 && sizeof(svt_hip_tx_decision) == 40 && sizeof(svt_hip_cfl_decision) == 32 && sizeof(svt_hip_inter_cand) == 16 &&
              sizeof(svt_hip_inter_blk) == 16 && offsetof(svt_hip_cfl_decision, uv_mode) == 24 && offsetof(svt_hip_inter_cand, flags) == 15, "the records md_slot reads as words");
static_assert(offsetof(svt_hip_md_rates, intraUVmodeFacBits) == 4 * MD_RATE_UV && offsetof(svt_hip_md_rates, cflAlphaFacBits) == 4 * MD_RATE_CFL, "svt_hip_md_rates as words");
static_assert(kMdTileWords == MD_COST_WORDS && SVT_HIP_MAX_NFL == MD_MAX_SLOTS, "md_decide_bpul sizes the unit for the kernel's tile");

static int md_decide_enqueue(const svt_hip_md_decide_group* groups, int ngroups, hipStream_t s) {
    GroupTable<MdDecideDesc, MD_MAX_GROUPS> tab;
    auto launch = [&](const MdDecideDesc& fd, uint32_t total) -> int {
        hipLaunchKernelGGL(md_decide_kernel, dim3(total), dim3(MD_THREADS), 0, s, fd);
        return launch_status("md_decide");
    };
    for (int g = 0; g < ngroups; g++) {
        const svt_hip_md_decide_group& G = groups[g];
        if (G.nblocks == 0) continue;
        const int bpul = md_decide_bpul(G.bsize, G.n);
        const MdGeom m = md_geom(G.bsize);
        const uint32_t units = (uint32_t)(((uint64_t)G.nblocks + (1u << bpul) - 1) >> bpul);
        MdDecideGroupDev* D = tab.add((units + MD_WAVES - 1) / MD_WAVES, launch);
        if (!D) return tab.rc;
        D->luma = (const unsigned long long*)G.d_luma;
        D->cdist[0] = (const unsigned long long*)G.d_dist_cb; D->cdist[1] = (const unsigned long long*)G.d_dist_cr;
        D->cbits[0] = (const unsigned long long*)G.d_bits_cb; D->cbits[1] = (const unsigned long long*)G.d_bits_cr;
        D->ceob[0] = G.d_eob_cb; D->ceob[1] = G.d_eob_cr;
        D->rate = G.d_rate; D->cand = G.d_cand; D->cand_out = G.ninter > 0 ? (const uint32_t*)G.d_cand_out : nullptr;
        D->cfl = (const unsigned long long*)G.d_cfl; D->blk = (const uint32_t*)G.d_blk; D->rates = (const int32_t*)G.d_rates;
        D->decision = (unsigned long long*)G.d_decision; D->full_cost = (unsigned long long*)G.d_full_cost;
        for (int p = 0; p < 3; p++) {
            D->gin[p] = (const int32_t*)G.d_pred[p]; D->gout[p] = (int32_t*)G.d_best_pred[p]; D->nql[p] = (uint8_t)(log2_of(m.pred_bytes[p]) - 4);
            D->gin[3 + p] = G.d_qcoeff[p]; D->gout[3 + p] = G.d_best_qcoeff[p];
            D->gin[6 + p] = G.d_dqcoeff[p]; D->gout[6 + p] = G.d_best_dqcoeff[p];
            D->nql[3 + p] = D->nql[6 + p] = (uint8_t)(log2_of(m.ncoeff[p]) - 2);
        }
        D->gin[9] = (const int32_t*)G.d_inter_blk; D->gout[9] = (int32_t*)G.d_best_inter_blk; D->nql[9] = 0;
        for (int c = 0; c < G.nintra; c++) D->modes4[c >> 4] |= (unsigned long long)G.modes[c] << (4 * (c & 15));
        D->nblocks = G.nblocks; D->lambda = G.lambda; D->n = (uint8_t)G.n; D->ninter = (uint8_t)G.ninter;
        D->cfl_allowed = kBsizeW[G.bsize] <= 32 && kBsizeH[G.bsize] <= 32;
        D->slice_is_intra = G.slice_is_intra != 0; D->escape = (uint8_t)G.full_loop_escape; D->bpul = (uint8_t)bpul;
    }
    return tab.flush(launch);
}

extern "C" int svt_hip_md_decide_frame(const svt_hip_md_decide_group* groups, int ngroups, void* stream) {
    if (int rc = require_init()) return rc;
    if (int rc = md_decide_check(groups, ngroups)) return rc;
    return md_decide_enqueue(groups, ngroups, (hipStream_t)stream);
}

// ---- the whole decision: luma transform-type search -> chroma full loop and rate -> decide ----------------------------------------
extern "C" size_t svt_hip_md_search_scratch_bytes(const svt_hip_md_search_group* groups, int ngroups) {
    return scratch_bytes_of(md_search_walk, groups, ngroups);
}

extern "C" int svt_hip_md_search_frame(const svt_hip_md_search_group* groups, int ngroups, int flavour, const svt_hip_qrows* q_luma,
                                       const svt_hip_qrows* q_chroma, void* d_scratch, size_t scratch_bytes, void* stream) {
    hipStream_t s = (hipStream_t)stream;
    if (int rc = require_init()) return rc;
    if (!q_luma) return set_err(SVT_HIP_ERR_INVALID, "NULL q_luma");
    MdSearchStages st;
    if (int rc = plan_stages(md_search_walk, groups, ngroups, d_scratch, scratch_bytes, &st)) return rc;
    const int nchroma = (int)st.flc.size();
    if (nchroma && !q_chroma) return set_err(SVT_HIP_ERR_INVALID, "NULL q_chroma");
    // every stage's arguments before the first launch
    if (int rc = full_loop_check(st.tx.fl.data(), ngroups, flavour, *q_luma)) return rc;
    if (int rc = coeff_rate_check(st.tx.cr.data(), ngroups)) return rc;
    if (int rc = tx_decide_check(st.tx.td.data(), ngroups)) return rc;
    if (nchroma) {
        if (int rc = full_loop_check(st.flc.data(), nchroma, flavour, *q_chroma)) return rc;
        if (int rc = coeff_rate_check(st.crc.data(), nchroma)) return rc;
    }
    if (int rc = md_decide_check(st.md.data(), ngroups)) return rc;
    if (int rc = full_loop_enqueue(st.tx.fl.data(), ngroups, flavour, *q_luma, s)) return rc;
    if (int rc = coeff_rate_enqueue(st.tx.cr.data(), ngroups, s)) return rc;
    if (int rc = tx_decide_enqueue(st.tx.td.data(), ngroups, s)) return rc;
    if (nchroma) {
        if (int rc = full_loop_enqueue(st.flc.data(), nchroma, flavour, *q_chroma, s)) return rc;
        if (int rc = coeff_rate_enqueue(st.crc.data(), nchroma, s)) return rc;
    }
    return md_decide_enqueue(st.md.data(), ngroups, s);
}

// svt_hip_cfl_search.hip — the CfL alpha search of mode decision (kernel_cfl_search.h): svt_hip_cfl_search_frame, the table (one
// cfl_search_kernel launch per CFS_MAX_GROUPS groups, then svt_hip_coeff_rate_frame's launches over the candidates in the scratch);
// svt_hip_cfl_decide_frame, cfl_rd_pick_alpha's walk (one launch per CFD_MAX_GROUPS groups); svt_hip_cfl_pick_frame, both on one stream
// as host composition, the tables the caller does not keep in the scratch.
#include <vector>

#include "host_common.h"
#include "kernel_cfl_search.h"

using namespace svtdev;
using namespace svthost;

static_assert(sizeof(svt_hip_cfl_decision) == 32 && alignof(svt_hip_cfl_decision) == 8, "cfl_decide_kernel stores the record as four words");
static_assert(SVT_HIP_CFL_NALPHA == CFS_NALPHA, "svt_hip_dsp.h");

namespace {
constexpr uint64_t kCands = 2 * SVT_HIP_CFL_NALPHA;       // per block
inline size_t align16(size_t v) { return (v + 15) & ~(size_t)15; }
inline int coeffs_of(int tx_size) { return kTxW[tx_size] * kTxH[tx_size]; }
// what one group takes from the search's scratch, in carving order
struct SearchCarve { size_t qcoeff, ctx; size_t total() const { return qcoeff + 2 * ctx; } };
struct PickCarve { size_t dist, bits, eob; size_t total() const { return dist + bits + eob; } };

// size, type and candidate count of one group, as every call of the family requires them (empty groups included)
int cfl_size_check(int g, int tx_size, int tx_type, uint32_t nblocks) {
    if (tx_size < 0 || tx_size >= SVT_TX_SIZES_ALL || tx_class_of(tx_size) != 0)
        return set_err(SVT_HIP_ERR_INVALID, "group %d: tx_size %d is no CfL chroma size (both sides 4 .. 16)", g, tx_size);
    if (tx_type < 0 || !txfm_allowed(tx_size, tx_type)) return set_err(SVT_HIP_ERR_INVALID, "group %d: tx_type %d not defined for tx_size %d", g, tx_type, tx_size);
    if ((uint64_t)nblocks * kCands > 0x7fffffffu) return set_err(SVT_HIP_ERR_INVALID, "group %d: nblocks * 66 too large", g);
    return SVT_HIP_OK;
}

int search_plan(const svt_hip_cfl_search_group* groups, int ngroups, std::vector<SearchCarve>* carve, size_t* need) {
    if (ngroups < 0 || (ngroups > 0 && !groups)) return set_err(SVT_HIP_ERR_INVALID, "NULL group list");
    *need = 0;
    for (int g = 0; g < ngroups; g++) {
        const svt_hip_cfl_search_group& G = groups[g];
        if (int rc = cfl_size_check(g, G.tx_size, G.tx_type, G.nblocks)) return rc;
        SearchCarve c{};
        if (G.nblocks) {
            const size_t cands = (size_t)G.nblocks * (size_t)kCands;
            c.qcoeff = cands * (size_t)coeffs_of(G.tx_size) * sizeof(int32_t);
            c.ctx = align16(cands);
        }
        *need += c.total();
        if (carve) carve->push_back(c);
    }
    return SVT_HIP_OK;
}

int qrows_check(const svt_hip_qrows* q, const char* name) {
    if (!q || !q->zbin || !q->round || !q->quant || !q->quant_shift || !q->dequant) return set_err(SVT_HIP_ERR_INVALID, "NULL quantiser table (%s)", name);
    for (int i = 0; i < 2; i++) {
        const int qs = q->quant_shift[i];
        if (qs <= 0 || (qs & (qs - 1))) return set_err(SVT_HIP_ERR_INVALID, "%s: quant_shift[%d] = %d is not a power of two", name, i, qs);
        if (q->dequant[i] < 0 || q->round[i] < 0) return set_err(SVT_HIP_ERR_INVALID, "%s: negative quantiser table entry", name);
    }
    if (!quant_params(q->zbin, q->round, q->quant, q->quant_shift, q->dequant, 0).fast_ok)
        return set_err(SVT_HIP_ERR_INVALID, "%s: quantiser table outside the one-product quantiser's range", name);
    return SVT_HIP_OK;
}

// the rate stage's groups: (block, plane, a) as a block with one type, qcoeff and contexts in the scratch
void rate_groups(const svt_hip_cfl_search_group* groups, int ngroups, const std::vector<SearchCarve>& carve, void* d_scratch,
                 std::vector<svt_hip_coeff_rate_group>* cr) {
    cr->resize((size_t)ngroups);
    char* at = (char*)d_scratch;
    for (int g = 0; g < ngroups; g++) {
        const svt_hip_cfl_search_group& G = groups[g];
        const SearchCarve& c = carve[(size_t)g];
        svt_hip_coeff_rate_group& C = (*cr)[(size_t)g];
        memset(&C, 0, sizeof(C));
        C.tx_size = G.tx_size; C.ntypes = 1; C.tx_types[0] = (uint8_t)G.tx_type;
        C.nblocks = G.nblocks * (uint32_t)kCands;
        if (!G.nblocks) continue;
        C.d_qcoeff = (const int32_t*)at; at += c.qcoeff;
        C.d_txb_skip_ctx = (const uint8_t*)at; at += c.ctx;
        C.d_dc_sign_ctx = (const uint8_t*)at; at += c.ctx;
        C.d_eob = G.d_eob; C.d_iscan = G.d_iscan; C.d_coeff_cost = G.d_coeff_cost; C.d_eob_cost = G.d_eob_cost; C.d_bits = G.d_bits;
    }
}

int search_check(const svt_hip_cfl_search_group* groups, int ngroups, int flavour, const svt_hip_qrows* q_cb, const svt_hip_qrows* q_cr,
                 void* d_scratch, size_t scratch_bytes, std::vector<svt_hip_coeff_rate_group>* cr) {
    std::vector<SearchCarve> carve;
    size_t need = 0;
    if (int rc = search_plan(groups, ngroups, &carve, &need)) return rc;
    if (flavour != SVT_HIP_FLAVOUR_C && flavour != SVT_HIP_FLAVOUR_AVX2) return set_err(SVT_HIP_ERR_INVALID, "flavour %d", flavour);
    if (int rc = qrows_check(q_cb, "q_cb")) return rc;
    if (int rc = qrows_check(q_cr, "q_cr")) return rc;
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
    if (need && (!d_scratch || ((uintptr_t)d_scratch & 15) || scratch_bytes < need))
        return set_err(SVT_HIP_ERR_INVALID, "scratch NULL, not 16-byte aligned or below svt_hip_cfl_search_scratch_bytes()");
    rate_groups(groups, ngroups, carve, d_scratch, cr);
    return coeff_rate_check(cr->data(), ngroups);
}

int decide_check(const svt_hip_cfl_decide_group* groups, int ngroups) {
    if (ngroups < 0 || (ngroups > 0 && !groups)) return set_err(SVT_HIP_ERR_INVALID, "NULL group list");
    for (int g = 0; g < ngroups; g++) {
        const svt_hip_cfl_decide_group& G = groups[g];
        if (G.nblocks == 0) continue;
        if ((uint64_t)G.nblocks * kCands > 0x7fffffffu) return set_err(SVT_HIP_ERR_INVALID, "group %d: nblocks * 66 too large", g);
        if (!G.d_dist || !G.d_bits || !G.d_alpha_rate || !G.d_cfl_mode_bits || !G.d_dc_mode_bits || !G.d_decision)
            return set_err(SVT_HIP_ERR_INVALID, "group %d: NULL member", g);
        if (((uintptr_t)G.d_dist & 15) || ((uintptr_t)G.d_bits & 7) || ((uintptr_t)G.d_decision & 7) || ((uintptr_t)G.d_alpha_rate & 3) ||
            ((uintptr_t)G.d_cfl_mode_bits & 3) || ((uintptr_t)G.d_dc_mode_bits & 3) || ((uintptr_t)G.d_alpha_q3_cb & 3) || ((uintptr_t)G.d_alpha_q3_cr & 3))
            return set_err(SVT_HIP_ERR_INVALID, "group %d: misaligned buffer (d_dist 16 bytes, d_bits / d_decision 8, the int32 arrays 4)", g);
    }
    return SVT_HIP_OK;
}

int search_enqueue(const svt_hip_cfl_search_group* groups, int ngroups, int flavour, const svt_hip_qrows* q_cb, const svt_hip_qrows* q_cr,
                   const std::vector<svt_hip_coeff_rate_group>& cr, hipStream_t s) {
    GroupTable<CflSearchDesc, CFS_MAX_GROUPS> tab;
    tab.desc.avx2 = flavour == SVT_HIP_FLAVOUR_AVX2;
    tab.desc.qp[0] = quant_params(q_cb->zbin, q_cb->round, q_cb->quant, q_cb->quant_shift, q_cb->dequant, 0);
    tab.desc.qp[1] = quant_params(q_cr->zbin, q_cr->round, q_cr->quant, q_cr->quant_shift, q_cr->dequant, 0);
    auto launch = [&](const CflSearchDesc& fd, uint32_t total) -> int {
        hipLaunchKernelGGL(cfl_search_kernel, dim3(total), dim3(FullLoopClass<0>::THREADS), 0, s, fd);
        return launch_status("cfl_search");
    };
    for (int g = 0; g < ngroups; g++) {
        const svt_hip_cfl_search_group& G = groups[g];
        if (G.nblocks == 0) continue;
        // a workgroup's waves take (blocks, plane) units: half as many blocks as a staged body's workgroup
        const uint32_t per_wg = staged_blocks_per_wg(G.tx_size) / 2;
        CflSearchGroupDev* D = tab.add((G.nblocks + per_wg - 1) / per_wg, launch);
        if (!D) return tab.rc;
        const svt_hip_coeff_rate_group& C = cr[(size_t)g];
        D->luma = G.d_luma_recon; D->xy = G.d_xy; D->iscan = G.d_iscan;
        for (int p = 0; p < 2; p++) {
            D->src[p] = G.d_src[p]; D->pred[p] = G.d_pred[p]; D->skip_ctx[p] = G.d_txb_skip_ctx[p]; D->dc_ctx[p] = G.d_dc_sign_ctx[p];
            D->src_stride[p] = G.src_stride[p]; D->pred_stride[p] = G.pred_stride[p];
        }
        D->dist = (unsigned long long*)G.d_dist; D->eob = G.d_eob;
        D->qcoeff = (int32_t*)C.d_qcoeff; D->skip_out = (uint8_t*)C.d_txb_skip_ctx; D->dc_out = (uint8_t*)C.d_dc_sign_ctx;
        D->luma_stride = G.luma_stride; D->nblocks = G.nblocks; D->tx_size = G.tx_size; D->tx_type = G.tx_type;
    }
    if (int rc = tab.flush(launch)) return rc;
    return coeff_rate_enqueue(cr.data(), ngroups, s);
}

int decide_enqueue(const svt_hip_cfl_decide_group* groups, int ngroups, hipStream_t s) {
    GroupTable<CflDecideDesc, CFD_MAX_GROUPS> tab;
    auto launch = [&](const CflDecideDesc& fd, uint32_t total) -> int {
        hipLaunchKernelGGL(cfl_decide_kernel, dim3(total), dim3(CFD_THREADS), 0, s, fd);
        return launch_status("cfl_decide");
    };
    for (int g = 0; g < ngroups; g++) {
        const svt_hip_cfl_decide_group& G = groups[g];
        if (G.nblocks == 0) continue;
        CflDecideGroupDev* D = tab.add((G.nblocks + CFD_THREADS - 1) / CFD_THREADS, launch);
        if (!D) return tab.rc;
        D->dist = (const unsigned long long*)G.d_dist; D->bits = (const unsigned long long*)G.d_bits; D->alpha_rate = G.d_alpha_rate;
        D->cfl_mode_bits = G.d_cfl_mode_bits; D->dc_mode_bits = G.d_dc_mode_bits; D->decision = (unsigned long long*)G.d_decision;
        D->alpha_cb = G.d_alpha_q3_cb; D->alpha_cr = G.d_alpha_q3_cr; D->nblocks = G.nblocks; D->lambda = G.lambda;
    }
    return tab.flush(launch);
}

// the pick's own pieces of the scratch (the tables the caller does not supply), then the search's
int pick_plan(const svt_hip_cfl_pick_group* groups, int ngroups, std::vector<PickCarve>* carve, std::vector<svt_hip_cfl_search_group>* sg,
              size_t* tables, size_t* need) {
    if (ngroups < 0 || (ngroups > 0 && !groups)) return set_err(SVT_HIP_ERR_INVALID, "NULL group list");
    *tables = 0;
    sg->resize((size_t)ngroups);
    for (int g = 0; g < ngroups; g++) {
        const svt_hip_cfl_search_group& G = groups[g].search;
        (*sg)[(size_t)g] = G;
        if (int rc = cfl_size_check(g, G.tx_size, G.tx_type, G.nblocks)) return rc;
        PickCarve c{};
        if (G.nblocks) {
            const size_t cands = (size_t)G.nblocks * (size_t)kCands;
            c.dist = G.d_dist ? 0 : cands * 16;
            c.bits = G.d_bits ? 0 : align16(cands * 8);
            c.eob = G.d_eob ? 0 : align16(cands * 2);
        }
        *tables += c.total();
        if (carve) carve->push_back(c);
    }
    size_t search_need = 0;
    if (int rc = search_plan(sg->data(), ngroups, nullptr, &search_need)) return rc;
    *need = *tables + search_need;
    return SVT_HIP_OK;
}
}  // namespace

extern "C" size_t svt_hip_cfl_search_scratch_bytes(const svt_hip_cfl_search_group* groups, int ngroups) {
    size_t need = 0;
    if (search_plan(groups, ngroups, nullptr, &need) != SVT_HIP_OK) return 0;
    return need;
}

extern "C" int svt_hip_cfl_search_frame(const svt_hip_cfl_search_group* groups, int ngroups, int flavour, const svt_hip_qrows* q_cb,
                                        const svt_hip_qrows* q_cr, void* d_scratch, size_t scratch_bytes, void* stream) {
    if (int rc = require_init()) return rc;
    std::vector<svt_hip_coeff_rate_group> cr;
    if (int rc = search_check(groups, ngroups, flavour, q_cb, q_cr, d_scratch, scratch_bytes, &cr)) return rc;
    return search_enqueue(groups, ngroups, flavour, q_cb, q_cr, cr, (hipStream_t)stream);
}

extern "C" int svt_hip_cfl_decide_frame(const svt_hip_cfl_decide_group* groups, int ngroups, void* stream) {
    if (int rc = require_init()) return rc;
    if (int rc = decide_check(groups, ngroups)) return rc;
    return decide_enqueue(groups, ngroups, (hipStream_t)stream);
}

extern "C" size_t svt_hip_cfl_pick_scratch_bytes(const svt_hip_cfl_pick_group* groups, int ngroups) {
    std::vector<svt_hip_cfl_search_group> sg;
    size_t tables = 0, need = 0;
    if (pick_plan(groups, ngroups, nullptr, &sg, &tables, &need) != SVT_HIP_OK) return 0;
    return need;
}

extern "C" int svt_hip_cfl_pick_frame(const svt_hip_cfl_pick_group* groups, int ngroups, int flavour, const svt_hip_qrows* q_cb,
                                      const svt_hip_qrows* q_cr, void* d_scratch, size_t scratch_bytes, void* stream) {
    if (int rc = require_init()) return rc;
    std::vector<PickCarve> carve;
    std::vector<svt_hip_cfl_search_group> sg;
    size_t tables = 0, need = 0;
    if (int rc = pick_plan(groups, ngroups, &carve, &sg, &tables, &need)) return rc;
    if (need && (!d_scratch || ((uintptr_t)d_scratch & 15) || scratch_bytes < need))
        return set_err(SVT_HIP_ERR_INVALID, "scratch NULL, not 16-byte aligned or below svt_hip_cfl_pick_scratch_bytes()");
    std::vector<svt_hip_cfl_decide_group> dg((size_t)ngroups);
    char* at = (char*)d_scratch;
    auto take = [&](size_t bytes) { char* p = at; at += bytes; return (void*)p; };
    for (int g = 0; g < ngroups; g++) {
        const svt_hip_cfl_pick_group& G = groups[g];
        const PickCarve& c = carve[(size_t)g];
        svt_hip_cfl_search_group& S = sg[(size_t)g];
        if (c.dist) S.d_dist = (uint64_t*)take(c.dist);
        if (c.bits) S.d_bits = (uint64_t*)take(c.bits);
        if (c.eob) S.d_eob = (uint16_t*)take(c.eob);
        svt_hip_cfl_decide_group& D = dg[(size_t)g];
        memset(&D, 0, sizeof(D));
        D.nblocks = S.nblocks; D.lambda = G.lambda; D.d_dist = S.d_dist; D.d_bits = S.d_bits; D.d_alpha_rate = G.d_alpha_rate;
        D.d_cfl_mode_bits = G.d_cfl_mode_bits; D.d_dc_mode_bits = G.d_dc_mode_bits; D.d_decision = G.d_decision;
        D.d_alpha_q3_cb = G.d_alpha_q3_cb; D.d_alpha_q3_cr = G.d_alpha_q3_cr;
    }
    // both stages' arguments before the first launch
    std::vector<svt_hip_coeff_rate_group> cr;
    if (int rc = search_check(sg.data(), ngroups, flavour, q_cb, q_cr, need > tables ? (void*)at : nullptr, need - tables, &cr)) return rc;
    if (int rc = decide_check(dg.data(), ngroups)) return rc;
    if (int rc = search_enqueue(sg.data(), ngroups, flavour, q_cb, q_cr, cr, (hipStream_t)stream)) return rc;
    return decide_enqueue(dg.data(), ngroups, (hipStream_t)stream);
}

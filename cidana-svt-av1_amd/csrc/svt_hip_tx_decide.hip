// svt_hip_tx_decide.hip — svt_hip_tx_decide_frame: RD cost, best transform type and the winner's coefficients per block
// (tx_decide_kernel, kernel_tx_decide.h), one launch per TD_MAX_GROUPS groups; svt_hip_tx_search_frame, the whole transform-type search
// as host composition: full loop -> coefficient rate -> decide on one stream, the per-type arrays the caller does not keep in a scratch.
#include <vector>

#include "host_common.h"
#include "kernel_tx_decide.h"

using namespace svtdev;
using namespace svthost;

static_assert(sizeof(svt_hip_tx_decision) == 40 && alignof(svt_hip_tx_decision) == 8, "tx_decide_kernel stores the record as five words");

static int log2_of(int v) { int l = 0; while ((1 << l) < v) l++; return l; }
static int coeffs_of(int tx_size) { return (kTxW[tx_size] < 32 ? kTxW[tx_size] : 32) * (kTxH[tx_size] < 32 ? kTxH[tx_size] : 32); }
// log2 blocks per wave-unit: 2^TD_UNIT_QUADS_LOG2 quads of gather, 64 blocks (one owning lane each) at most
static int tx_decide_bpul(int nql) { return TD_UNIT_QUADS_LOG2 - nql < 6 ? TD_UNIT_QUADS_LOG2 - nql : 6; }

static int tx_decide_check(const svt_hip_tx_decide_group* groups, int ngroups) {
    if (ngroups < 0 || (ngroups > 0 && !groups)) return set_err(SVT_HIP_ERR_INVALID, "NULL group list");
    for (int g = 0; g < ngroups; g++) {
        const svt_hip_tx_decide_group& G = groups[g];
        if (int rc = group_types_check(g, G.tx_size, G.ntypes, G.tx_types)) return rc;
        if (G.nblocks == 0) continue;
        if ((uint64_t)G.nblocks * (uint64_t)G.ntypes > 0x7fffffffu) return set_err(SVT_HIP_ERR_INVALID, "group %d: nblocks * ntypes too large", g);
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

extern "C" int svt_hip_tx_decide_frame(const svt_hip_tx_decide_group* groups, int ngroups, void* stream) {
    if (int rc = require_init()) return rc;
    if (int rc = tx_decide_check(groups, ngroups)) return rc;
    hipStream_t s = (hipStream_t)stream;
    GroupTable<TxDecideDesc, TD_MAX_GROUPS> tab;
    auto launch = [&](const TxDecideDesc& fd, uint32_t total) -> int {
        hipLaunchKernelGGL(tx_decide_kernel, dim3(total), dim3(TD_THREADS), 0, s, fd);
        return launch_status("tx_decide");
    };
    for (int g = 0; g < ngroups; g++) {
        const svt_hip_tx_decide_group& G = groups[g];
        if (G.nblocks == 0) continue;
        const int nql = log2_of(coeffs_of(G.tx_size)) - 2, bpul = tx_decide_bpul(nql);
        const uint32_t units = (uint32_t)(((uint64_t)G.nblocks + (1u << bpul) - 1) >> bpul);
        TxDecideGroupDev* D = tab.add((units + TD_WAVES - 1) / TD_WAVES, launch);
        if (!D) return tab.rc;
        D->dist = (const unsigned long long*)G.d_dist; D->eob = G.d_eob; D->bits = (const unsigned long long*)G.d_bits;
        D->qcoeff = G.d_qcoeff; D->dqcoeff = G.d_dqcoeff; D->decision = (unsigned long long*)G.d_decision;
        D->best_qcoeff = G.d_best_qcoeff; D->best_dqcoeff = G.d_best_dqcoeff;
        D->nblocks = G.nblocks; D->lambda = G.lambda; D->ntypes = (uint8_t)G.ntypes;
        D->nql = (uint8_t)nql; D->bpul = (uint8_t)bpul;
        D->dct_index = -1;
        for (int t = 0; t < G.ntypes; t++) {
            D->types |= (unsigned long long)G.tx_types[t] << (4 * t);
            if (G.tx_types[t] == SVT_DCT_DCT) D->dct_index = (int8_t)t;
        }
    }
    return tab.flush(launch);
}

// ---- the whole search: full loop -> coefficient rate -> decide ------------------------------------------------------------------
namespace {
inline size_t align16(size_t v) { return (v + 15) & ~(size_t)15; }
// what one group takes from the scratch, in carving order; every piece a multiple of 16 bytes
struct TxSearchCarve { size_t dist, eob, bits, qcoeff, dqcoeff; size_t total() const { return dist + eob + bits + qcoeff + dqcoeff; } };
}  // namespace

// size / types / pair count of every group, and the scratch they need; 0 groups or only empty ones need none
static int tx_search_plan(const svt_hip_tx_search_group* groups, int ngroups, std::vector<TxSearchCarve>* carve, size_t* need) {
    if (ngroups < 0 || (ngroups > 0 && !groups)) return set_err(SVT_HIP_ERR_INVALID, "NULL group list");
    *need = 0;
    for (int g = 0; g < ngroups; g++) {
        const svt_hip_tx_search_group& G = groups[g];
        if (int rc = group_types_check(g, G.fl.tx_size, G.fl.ntypes, G.fl.tx_types)) return rc;
        TxSearchCarve c{};
        const uint64_t pairs = (uint64_t)G.fl.nblocks * (uint64_t)G.fl.ntypes;
        if (pairs > 0x7fffffffu) return set_err(SVT_HIP_ERR_INVALID, "group %d: nblocks * ntypes too large", g);
        if (pairs) {
            const size_t coeff_bytes = (size_t)pairs * (size_t)coeffs_of(G.fl.tx_size) * sizeof(int32_t);
            c.dist = G.fl.d_dist ? 0 : (size_t)pairs * 16;
            c.eob = G.fl.d_eob ? 0 : align16((size_t)pairs * 2);
            c.bits = align16((size_t)pairs * 8);
            c.qcoeff = G.fl.d_qcoeff ? 0 : coeff_bytes;
            c.dqcoeff = (G.fl.d_dqcoeff || !G.d_best_dqcoeff) ? 0 : coeff_bytes;
        }
        *need += c.total();
        if (carve) carve->push_back(c);
    }
    return SVT_HIP_OK;
}

extern "C" size_t svt_hip_tx_search_scratch_bytes(const svt_hip_tx_search_group* groups, int ngroups) {
    size_t need = 0;
    if (tx_search_plan(groups, ngroups, nullptr, &need) != SVT_HIP_OK) return 0;
    return need;
}

extern "C" int svt_hip_tx_search_frame(const svt_hip_tx_search_group* groups, int ngroups, int flavour, const int16_t* zbin,
                                       const int16_t* round, const int16_t* quant, const int16_t* quant_shift, const int16_t* dequant,
                                       void* d_scratch, size_t scratch_bytes, void* stream) {
    if (int rc = require_init()) return rc;
    std::vector<TxSearchCarve> carve;
    size_t need = 0;
    if (int rc = tx_search_plan(groups, ngroups, &carve, &need)) return rc;
    if (need && (!d_scratch || ((uintptr_t)d_scratch & 15) || scratch_bytes < need))
        return set_err(SVT_HIP_ERR_INVALID, "scratch NULL, not 16-byte aligned or below svt_hip_tx_search_scratch_bytes()");
    std::vector<svt_hip_full_loop_group> fl((size_t)ngroups);
    std::vector<svt_hip_coeff_rate_group> cr((size_t)ngroups);
    std::vector<svt_hip_tx_decide_group> td((size_t)ngroups);
    char* at = (char*)d_scratch;
    auto take = [&](size_t bytes) { char* p = at; at += bytes; return (void*)p; };
    for (int g = 0; g < ngroups; g++) {
        const svt_hip_tx_search_group& G = groups[g];
        const TxSearchCarve& c = carve[(size_t)g];
        svt_hip_full_loop_group& F = fl[(size_t)g];
        F = G.fl;
        uint64_t* bits = nullptr;
        if (G.fl.nblocks) {
            if (c.dist) F.d_dist = (uint64_t*)take(c.dist);
            if (c.eob) F.d_eob = (uint16_t*)take(c.eob);
            bits = (uint64_t*)take(c.bits);
            if (c.qcoeff) F.d_qcoeff = (int32_t*)take(c.qcoeff);
            if (c.dqcoeff) F.d_dqcoeff = (int32_t*)take(c.dqcoeff);
        }
        svt_hip_coeff_rate_group& C = cr[(size_t)g];
        memset(&C, 0, sizeof(C));
        C.tx_size = F.tx_size; C.ntypes = F.ntypes; memcpy(C.tx_types, F.tx_types, sizeof(C.tx_types)); C.nblocks = F.nblocks;
        C.d_qcoeff = F.d_qcoeff; C.d_eob = F.d_eob; C.d_iscan = F.d_iscan; C.d_txb_skip_ctx = G.d_txb_skip_ctx; C.d_dc_sign_ctx = G.d_dc_sign_ctx;
        C.d_type_bits = G.d_type_bits; C.d_coeff_cost = G.d_coeff_cost; C.d_eob_cost = G.d_eob_cost; C.d_bits = bits;
        svt_hip_tx_decide_group& D = td[(size_t)g];
        memset(&D, 0, sizeof(D));
        D.tx_size = F.tx_size; D.ntypes = F.ntypes; memcpy(D.tx_types, F.tx_types, sizeof(D.tx_types)); D.nblocks = F.nblocks;
        D.lambda = G.lambda; D.d_dist = F.d_dist; D.d_eob = F.d_eob; D.d_bits = bits; D.d_qcoeff = F.d_qcoeff; D.d_dqcoeff = F.d_dqcoeff;
        D.d_decision = G.d_decision; D.d_best_qcoeff = G.d_best_qcoeff; D.d_best_dqcoeff = G.d_best_dqcoeff;
    }
    // all three stages' arguments before the first launch
    if (int rc = full_loop_check(fl.data(), ngroups, flavour, zbin, round, quant, quant_shift, dequant)) return rc;
    if (int rc = coeff_rate_check(cr.data(), ngroups)) return rc;
    if (int rc = tx_decide_check(td.data(), ngroups)) return rc;
    if (int rc = svt_hip_full_loop_frame(fl.data(), ngroups, flavour, zbin, round, quant, quant_shift, dequant, stream)) return rc;
    if (int rc = svt_hip_coeff_rate_frame(cr.data(), ngroups, stream)) return rc;
    return svt_hip_tx_decide_frame(td.data(), ngroups, stream);
}

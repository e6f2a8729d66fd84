// svt_hip_tx_decide.hip — svt_hip_tx_decide_frame: RD cost, best transform type and the winner's coefficients per block
// (tx_decide_kernel, kernel_tx_decide.h), one launch per TD_MAX_GROUPS groups; svt_hip_tx_search_frame, the whole transform-type search
// as host composition: full loop -> coefficient rate -> decide on one stream, the per-type arrays the caller does not keep in a scratch.
// What is left here: the decide's launch geometry, group-table fill and launch (tx_decide_enqueue) and the entry points; the checks, the
// scratch layout and the three stages' groups are md_plan.h's.
#include "host_common.h"
#include "kernel_tx_decide.h"

using namespace svtdev;
using namespace svthost;

static_assert(sizeof(svt_hip_tx_decision) == 40 && alignof(svt_hip_tx_decision) == 8, "tx_decide_kernel stores the record as five words");

// log2 blocks per wave-unit: 2^TD_UNIT_QUADS_LOG2 quads of gather, 64 blocks (one owning lane each) at most
static int tx_decide_bpul(int nql) { return TD_UNIT_QUADS_LOG2 - nql < 6 ? TD_UNIT_QUADS_LOG2 - nql : 6; }

int svthost::tx_decide_enqueue(const svt_hip_tx_decide_group* groups, int ngroups, hipStream_t s) {
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

extern "C" int svt_hip_tx_decide_frame(const svt_hip_tx_decide_group* groups, int ngroups, void* stream) {
    if (int rc = require_init()) return rc;
    if (int rc = tx_decide_check(groups, ngroups)) return rc;
    return tx_decide_enqueue(groups, ngroups, (hipStream_t)stream);
}

// ---- the whole search: full loop -> coefficient rate -> decide ------------------------------------------------------------------
extern "C" size_t svt_hip_tx_search_scratch_bytes(const svt_hip_tx_search_group* groups, int ngroups) {
    return scratch_bytes_of(tx_search_walk, groups, ngroups);
}

extern "C" int svt_hip_tx_search_frame(const svt_hip_tx_search_group* groups, int ngroups, int flavour, const int16_t* zbin,
                                       const int16_t* round, const int16_t* quant, const int16_t* quant_shift, const int16_t* dequant,
                                       void* d_scratch, size_t scratch_bytes, void* stream) {
    const svt_hip_qrows q = {zbin, round, quant, quant_shift, dequant};
    hipStream_t s = (hipStream_t)stream;
    if (int rc = require_init()) return rc;
    TxSearchStages st;
    if (int rc = plan_stages(tx_search_walk, groups, ngroups, d_scratch, scratch_bytes, &st)) return rc;
    // all three stages' arguments before the first launch
    if (int rc = full_loop_check(st.fl.data(), ngroups, flavour, q)) return rc;
    if (int rc = coeff_rate_check(st.cr.data(), ngroups)) return rc;
    if (int rc = tx_decide_check(st.td.data(), ngroups)) return rc;
    if (int rc = full_loop_enqueue(st.fl.data(), ngroups, flavour, q, s)) return rc;
    if (int rc = coeff_rate_enqueue(st.cr.data(), ngroups, s)) return rc;
    return tx_decide_enqueue(st.td.data(), ngroups, s);
}

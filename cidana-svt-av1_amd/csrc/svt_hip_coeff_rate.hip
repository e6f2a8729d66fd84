// svt_hip_coeff_rate.hip — svt_hip_coeff_rate_frame: the coefficient rate of quantised blocks (coeff_rate_kernel, kernel_coeff_rate.h),
// one launch per CR_MAX_GROUPS groups; svt_hip_coeff_cost_index, the host helper that names a size's cost tables.  What is left here: the
// launch geometry, the group-table fill and the launch (coeff_rate_enqueue); the argument check is md_plan.h's.
#include "host_common.h"
#include "kernel_coeff_rate.h"

using namespace svtdev;
using namespace svthost;

static uint64_t pairs_of(const svt_hip_coeff_rate_group& G) { return (uint64_t)G.nblocks * (uint64_t)G.ntypes; }
// (block, type) pairs per wave-unit: 64 / min(quads, 64)
static uint32_t pairs_per_unit(int tx_size) {
    const int quads = coeffs_of(tx_size) / 4;
    return (uint32_t)(quads < 64 ? 64 / quads : 1);
}
// wave-units per wave: 1 until the group has 2048 workgroups of its own (8 per CU), then up to CR_ITERS, which spreads the staging of
// the cost tables over more work
static uint32_t coeff_rate_iters(uint64_t units) {
    const uint64_t it = units / (uint64_t)(CR_WAVES * 2048);
    return (uint32_t)(it < 1 ? 1 : (it > (uint64_t)CR_ITERS ? (uint64_t)CR_ITERS : it));
}

// txs_ctx = (txsize_sqr_map + txsize_sqr_up_map + 1) >> 1 (TX_4X4 = 0 .. TX_64X64 = 4) and txsize_log2_minus4, from the sides
extern "C" int svt_hip_coeff_cost_index(int tx_size, int* txs_ctx, int* eob_multi_size) {
    if (tx_size < 0 || tx_size >= SVT_TX_SIZES_ALL) return set_err(SVT_HIP_ERR_INVALID, "bad tx_size %d", tx_size);
    const int lw = log2_of(kTxW[tx_size]), lh = log2_of(kTxH[tx_size]);
    const int lo = (lw < lh ? lw : lh) - 2, hi = (lw > lh ? lw : lh) - 2;
    if (txs_ctx) *txs_ctx = (lo + hi + 1) >> 1;
    if (eob_multi_size) *eob_multi_size = log2_of(coeffs_of(tx_size)) - 4;
    return SVT_HIP_OK;
}

int svthost::coeff_rate_enqueue(const svt_hip_coeff_rate_group* groups, int ngroups, hipStream_t s) {
    GroupTable<CoeffRateDesc, CR_MAX_GROUPS> tab;
    auto launch = [&](const CoeffRateDesc& fd, uint32_t total) -> int {
        hipLaunchKernelGGL(coeff_rate_kernel, dim3(total), dim3(CR_THREADS), 0, s, fd);
        return launch_status("coeff_rate");
    };
    for (int g = 0; g < ngroups; g++) {
        const svt_hip_coeff_rate_group& G = groups[g];
        if (G.nblocks == 0) continue;
        const uint32_t ppu = pairs_per_unit(G.tx_size);
        const uint64_t units = (pairs_of(G) + ppu - 1) / ppu;
        const uint32_t iters = coeff_rate_iters(units), per_wg = (uint32_t)CR_WAVES * iters;
        CoeffRateGroupDev* D = tab.add((uint32_t)((units + per_wg - 1) / per_wg), launch);
        if (!D) return tab.rc;
        const int w = kTxW[G.tx_size], h = kTxH[G.tx_size];
        D->qcoeff = G.d_qcoeff; D->eob = G.d_eob; D->iscan = G.d_iscan; D->skip_ctx = G.d_txb_skip_ctx; D->dc_ctx = G.d_dc_sign_ctx;
        D->type_bits = G.d_type_bits; D->coeff_cost = G.d_coeff_cost; D->eob_cost = G.d_eob_cost; D->bits = (unsigned long long*)G.d_bits;
        D->nblocks = G.nblocks; D->ntypes = G.ntypes;
        D->bwl = (uint8_t)log2_of(packed_side(w)); D->bhl = (uint8_t)log2_of(packed_side(h));
        D->shape = w == h ? 0 : (w > h ? 1 : 2);
        D->iters = (uint8_t)iters;
        memcpy(D->types, G.tx_types, sizeof(D->types));
    }
    return tab.flush(launch);
}

extern "C" int svt_hip_coeff_rate_frame(const svt_hip_coeff_rate_group* groups, int ngroups, void* stream) {
    if (int rc = require_init()) return rc;
    if (int rc = coeff_rate_check(groups, ngroups)) return rc;
    return coeff_rate_enqueue(groups, ngroups, (hipStream_t)stream);
}

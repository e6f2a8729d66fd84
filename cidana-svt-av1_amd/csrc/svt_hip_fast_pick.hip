// svt_hip_fast_pick.hip — svt_hip_fast_pick_frame: fast cost, the N best and their order per block, the survivors' predictions gathered
// (fast_pick_kernel, kernel_fast_pick.h), one launch per non-empty group; svt_hip_intra_fast_search_frame, the whole intra fast search
// as host composition: fast loop (luma, Cb, Cr) -> pick on one stream, the arrays the caller does not keep in a scratch.
#include <vector>

#include "host_common.h"
#include "kernel_fast_pick.h"

using namespace svtdev;
using namespace svthost;

static_assert(sizeof(svt_hip_fast_pick_blk) == 8, "fast_pick_kernel loads the record as one word");
static_assert(sizeof(svt_hip_fast_rates) == FP_RATE_WORDS * sizeof(int32_t), "fast_pick_kernel stages the tables as words");
static_assert(offsetof(svt_hip_fast_rates, mbModeFacBits) == FP_MB * 4 && offsetof(svt_hip_fast_rates, intraUVmodeFacBits) == FP_UV * 4 &&
              offsetof(svt_hip_fast_rates, angleDeltaFacBits) == FP_ANG * 4 && offsetof(svt_hip_fast_rates, skipModeFacBits) == FP_SKIP * 4 &&
              offsetof(svt_hip_fast_rates, intraInterFacBits) == FP_II * 4, "svt_hip_fast_rates layout");
static_assert(sizeof(FastPickDev) <= 4000, "kernel arguments");

// size_group_lookup / num_pels_log2_lookup (EbDefinitions.h:1311, 1315)
static const uint8_t kSizeGroup[22] = {0, 0, 0, 1, 1, 1, 2, 2, 2, 3, 3, 3, 3, 3, 3, 3, 0, 0, 1, 1, 2, 2};
static const uint8_t kNumPelsLog2[22] = {4, 5, 5, 6, 7, 7, 8, 9, 9, 10, 11, 11, 12, 13, 13, 14, 6, 6, 8, 8, 10, 10};

static int log2_of(int v) { int l = 0; while ((1 << l) < v) l++; return l; }

// blocks per wave: one until every wave slot of the device (32 per CU) has a block, then up to FP_MAX_BPW, which spreads the staging of the
// rate tables over more blocks
static int fast_pick_bpw(uint32_t nblocks) {
    const uint32_t slots = (uint32_t)(g_num_cu > 0 ? g_num_cu : 256) * 32u, b = nblocks / slots;
    return b < 1 ? 1 : (b > (uint32_t)FP_MAX_BPW ? FP_MAX_BPW : (int)b);
}

static int fast_pick_check(const svt_hip_fast_pick_group* groups, int ngroups, int metric) {
    if (ngroups < 0 || (ngroups > 0 && !groups)) return set_err(SVT_HIP_ERR_INVALID, "NULL group list");
    if (metric != SVT_HIP_FAST_SAD && metric != SVT_HIP_FAST_SSD) return set_err(SVT_HIP_ERR_INVALID, "metric %d", metric);
    for (int g = 0; g < ngroups; g++) {
        const svt_hip_fast_pick_group& G = groups[g];
        if (G.tx_size < 0 || G.tx_size >= SVT_TX_SIZES_ALL) return set_err(SVT_HIP_ERR_INVALID, "group %d: tx_size %d", g, G.tx_size);
        if (G.bsize < 0 || G.bsize > 21 || G.bsize_uv < 0 || G.bsize_uv > 21)
            return set_err(SVT_HIP_ERR_INVALID, "group %d: bsize %d / bsize_uv %d (0 .. 21)", g, G.bsize, G.bsize_uv);
        if (G.ncand < 1 || G.ncand > SVT_HIP_FAST_LOOP_MAX_CANDIDATES) return set_err(SVT_HIP_ERR_INVALID, "group %d: ncand %d (1 .. 64)", g, G.ncand);
        if (G.nfl < 1 || G.nfl > SVT_HIP_MAX_NFL) return set_err(SVT_HIP_ERR_INVALID, "group %d: nfl %d (1 .. %d)", g, G.nfl, SVT_HIP_MAX_NFL);
        if (G.ac_dequant_q3 < 0) return set_err(SVT_HIP_ERR_INVALID, "group %d: ac_dequant_q3 %d", g, G.ac_dequant_q3);
        for (int c = 0; c < G.ncand; c++) {
            const int m = G.modes[c], a = G.angle_deltas[c], um = G.uv_modes[c], ua = G.uv_angle_deltas[c];
            if (m > 12) return set_err(SVT_HIP_ERR_INVALID, "group %d: candidate %d: mode %d", g, c, m);
            if (um > 13) return set_err(SVT_HIP_ERR_INVALID, "group %d: candidate %d: uv mode %d", g, c, um);
            if (a < -3 || a > 3 || ua < -3 || ua > 3) return set_err(SVT_HIP_ERR_INVALID, "group %d: candidate %d: angle delta %d / %d", g, c, a, ua);
        }
        if (G.nblocks == 0) continue;
        if ((uint64_t)G.nblocks * (uint64_t)G.ncand > 0x7fffffffu) return set_err(SVT_HIP_ERR_INVALID, "group %d: nblocks * ncand too large", g);
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

static int fast_pick_enqueue(const svt_hip_fast_pick_group* groups, int ngroups, int metric, hipStream_t s) {
    for (int g = 0; g < ngroups; g++) {
        const svt_hip_fast_pick_group& G = groups[g];
        if (G.nblocks == 0) continue;
        const int w = kTxW[G.tx_size], h = kTxH[G.tx_size];
        FastPickDev D;
        memset(&D, 0, sizeof(D));
        D.dist = (const unsigned long long*)G.d_dist; D.dist_cb = (const unsigned long long*)G.d_dist_cb; D.dist_cr = (const unsigned long long*)G.d_dist_cr;
        D.blk = (const unsigned long long*)G.d_blk; D.rates = (const int32_t*)G.d_rates; D.pred = G.d_pred; D.src_xy = G.d_src_xy;
        D.cand_out = G.d_cand; D.sorted = G.d_sorted; D.cost = (unsigned long long*)G.d_cost; D.rate = G.d_rate;
        D.ref_fast_cost = (unsigned long long*)G.d_ref_fast_cost; D.all_cost = (unsigned long long*)G.d_all_cost;
        D.pred_out = G.d_pred_out; D.src_xy_out = G.d_src_xy_out;
        D.nblocks = G.nblocks; D.lambda = G.lambda; D.intrabc_bits = G.intrabc_bits; D.qstep = (uint32_t)(G.ac_dequant_q3 >> 3);
        for (int c = 0; c < G.ncand; c++) {
            const int um = G.uv_modes[c] == 13 ? 0 : G.uv_modes[c];              // UV_CFL_PRED is costed as UV_DC_PRED
            D.cand[c] = (uint16_t)(G.modes[c] | ((G.angle_deltas[c] + 3) << 4) | (um << 8) | ((G.uv_angle_deltas[c] + 3) << 12));
        }
        const int n = G.nfl < G.ncand ? G.nfl : G.ncand;
        D.ncand = (uint8_t)G.ncand; D.n = (uint8_t)n; D.nbuf = (uint8_t)(G.ncand > n ? n + 1 : n);
        D.ssd = metric == SVT_HIP_FAST_SSD; D.slice_is_intra = G.slice_is_intra != 0; D.use_angle_delta = G.use_angle_delta != 0;
        D.cfl_allowed = w <= 32 && h <= 32; D.size_group = kSizeGroup[G.bsize];
        D.nlog2_y = kNumPelsLog2[G.bsize]; D.nlog2_uv = kNumPelsLog2[G.bsize_uv];
        D.ql = (uint8_t)(log2_of(w * h) - 4);
        D.bpw = (uint8_t)fast_pick_bpw(G.nblocks);
        const uint32_t per_wg = (uint32_t)(FP_WAVES * D.bpw), wgs = (G.nblocks + per_wg - 1) / per_wg;
        hipLaunchKernelGGL(fast_pick_kernel, dim3(wgs), dim3(FP_THREADS), 0, s, D);
        if (int rc = launch_status("fast_pick")) return rc;
    }
    return SVT_HIP_OK;
}

extern "C" int svt_hip_fast_pick_frame(const svt_hip_fast_pick_group* groups, int ngroups, int metric, void* stream) {
    if (int rc = require_init()) return rc;
    if (int rc = fast_pick_check(groups, ngroups, metric)) return rc;
    return fast_pick_enqueue(groups, ngroups, metric, (hipStream_t)stream);
}

// ---- the whole intra fast search: fast loop (luma, Cb, Cr) -> pick ---------------------------------------------------------------
namespace {
inline size_t align16(size_t v) { return (v + 15) & ~(size_t)15; }
// what one group takes from the scratch, in carving order; every piece a multiple of 16 bytes
struct FastSearchCarve { size_t dist, dist_cb, dist_cr, pred; size_t total() const { return dist + dist_cb + dist_cr + pred; } };
}  // namespace

// the sizes the carving needs, checked here because the scratch is sized before the stages' own checks run; everything else is theirs
static int fast_search_plan(const svt_hip_intra_fast_search_group* groups, int ngroups, std::vector<FastSearchCarve>* carve, size_t* need) {
    if (ngroups < 0 || (ngroups > 0 && !groups)) return set_err(SVT_HIP_ERR_INVALID, "NULL group list");
    *need = 0;
    for (int g = 0; g < ngroups; g++) {
        const svt_hip_intra_fast_search_group& G = groups[g];
        const svt_hip_fast_loop_group& L = G.luma;
        if (L.tx_size < 0 || L.tx_size >= SVT_TX_SIZES_ALL) return set_err(SVT_HIP_ERR_INVALID, "group %d: tx_size %d", g, L.tx_size);
        if (L.ncand < 1 || L.ncand > SVT_HIP_FAST_LOOP_MAX_CANDIDATES) return set_err(SVT_HIP_ERR_INVALID, "group %d: ncand %d (1 .. 64)", g, L.ncand);
        if (G.use_chroma && (G.cb.nblocks != L.nblocks || G.cr.nblocks != L.nblocks || G.cb.ncand != L.ncand || G.cr.ncand != L.ncand))
            return set_err(SVT_HIP_ERR_INVALID, "group %d: the chroma groups' nblocks / ncand differ from luma's", g);
        FastSearchCarve c{};
        const uint64_t pairs = (uint64_t)L.nblocks * (uint64_t)L.ncand;
        if (pairs > 0x7fffffffu) return set_err(SVT_HIP_ERR_INVALID, "group %d: nblocks * ncand too large", g);
        if (pairs) {
            c.dist = L.d_dist ? 0 : align16((size_t)pairs * 8);
            c.dist_cb = (!G.use_chroma || G.cb.d_dist) ? 0 : align16((size_t)pairs * 8);
            c.dist_cr = (!G.use_chroma || G.cr.d_dist) ? 0 : align16((size_t)pairs * 8);
            c.pred = (L.d_pred || !G.pick.d_pred_out) ? 0 : align16((size_t)pairs * (size_t)(kTxW[L.tx_size] * kTxH[L.tx_size]));
        }
        *need += c.total();
        if (carve) carve->push_back(c);
    }
    return SVT_HIP_OK;
}

extern "C" size_t svt_hip_intra_fast_search_scratch_bytes(const svt_hip_intra_fast_search_group* groups, int ngroups) {
    size_t need = 0;
    if (fast_search_plan(groups, ngroups, nullptr, &need) != SVT_HIP_OK) return 0;
    return need;
}

extern "C" int svt_hip_intra_fast_search_frame(const svt_hip_intra_fast_search_group* groups, int ngroups, int metric, int flavour,
                                               void* d_scratch, size_t scratch_bytes, void* stream) {
    if (int rc = require_init()) return rc;
    std::vector<FastSearchCarve> carve;
    size_t need = 0;
    if (int rc = fast_search_plan(groups, ngroups, &carve, &need)) return rc;
    if (need && (!d_scratch || ((uintptr_t)d_scratch & 15) || scratch_bytes < need))
        return set_err(SVT_HIP_ERR_INVALID, "scratch NULL, not 16-byte aligned or below svt_hip_intra_fast_search_scratch_bytes()");
    std::vector<svt_hip_fast_loop_group> fl, flc;              // luma groups; the chroma groups of those that have them
    std::vector<svt_hip_fast_pick_group> fp((size_t)ngroups);
    fl.reserve((size_t)ngroups);
    char* at = (char*)d_scratch;
    auto take = [&](size_t bytes) { char* p = at; at += bytes; return (void*)p; };
    for (int g = 0; g < ngroups; g++) {
        const svt_hip_intra_fast_search_group& G = groups[g];
        const FastSearchCarve& c = carve[(size_t)g];
        svt_hip_fast_loop_group L = G.luma, CB = G.cb, CR = G.cr;
        if (c.dist) L.d_dist = (uint64_t*)take(c.dist);
        if (c.dist_cb) CB.d_dist = (uint64_t*)take(c.dist_cb);
        if (c.dist_cr) CR.d_dist = (uint64_t*)take(c.dist_cr);
        if (c.pred) L.d_pred = (uint8_t*)take(c.pred);
        fl.push_back(L);
        if (G.use_chroma) { flc.push_back(CB); flc.push_back(CR); }
        svt_hip_fast_pick_group& P = fp[(size_t)g];
        P = G.pick;
        P.tx_size = L.tx_size; P.nblocks = L.nblocks; P.ncand = L.ncand;
        memcpy(P.modes, L.modes, sizeof(P.modes)); memcpy(P.angle_deltas, L.angle_deltas, sizeof(P.angle_deltas));
        P.d_dist = L.d_dist; P.d_dist_cb = G.use_chroma ? CB.d_dist : nullptr; P.d_dist_cr = G.use_chroma ? CR.d_dist : nullptr;
        P.d_pred = L.d_pred;
        if (L.d_src_xy) P.d_src_xy = L.d_src_xy;
    }
    // every stage's arguments before the first launch
    if (int rc = fast_loop_check(fl.data(), ngroups, metric, flavour)) return rc;
    if (int rc = fast_loop_check(flc.data(), (int)flc.size(), metric, flavour)) return rc;
    if (int rc = fast_pick_check(fp.data(), ngroups, metric)) return rc;
    if (int rc = svt_hip_intra_fast_loop_frame(fl.data(), ngroups, metric, flavour, stream)) return rc;
    if (!flc.empty())
        if (int rc = svt_hip_intra_fast_loop_frame(flc.data(), (int)flc.size(), metric, flavour, stream)) return rc;
    return fast_pick_enqueue(fp.data(), ngroups, metric, (hipStream_t)stream);
}

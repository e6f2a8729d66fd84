// csrc/warp_plan.h on the CPU: what svt_hip_warp_fit_frame and svt_hip_warp_pred_frame decide on the host before they touch a device.
// A valid group list is accepted and the same list with one field changed is refused, for every clause of warp_fit_check and
// warp_pred_check; the tiling (WarpGeom) of every plane block shape holds its invariants and a mixed list's workgroup counts and group
// tables equal hand-computed values; a list longer than one launch's table is cut where the table is full; the shape word round-trips;
// the filter and divisor tables (csrc/warp_tables.h) hold what the kernels assume of them.  "Device" pointers are addresses inside a
// host array that nothing dereferences.  Plain C++17 (g++), linked with csrc/host_err.cpp, also built under
// -fsanitize=address,undefined by tests/test_warp_plan_host.py.  Exit status 0 and "ok" when every case holds.
#include <stdio.h>
#include <stdlib.h>

#include <functional>
#include <vector>

#include "../../cidana-svt-av1_amd/csrc/warp_plan.h"
#include "../../cidana-svt-av1_amd/csrc/warp_tables.h"

using namespace svthost;
using namespace svtdev;

#define CHECK(c) do { if (!(c)) { fprintf(stderr, "%s:%d: %s (last error: %s)\n", __FILE__, __LINE__, #c, svt_hip_last_error()); return 1; } } while (0)
static const int INVALID = SVT_HIP_ERR_INVALID;

alignas(64) static char g_dev[1 << 18];
static size_t g_dev_next = 0;
static void* dev() {
    if (64 * (g_dev_next + 2) > sizeof(g_dev)) { fprintf(stderr, "g_dev too small\n"); exit(2); }
    return g_dev + 64 * ++g_dev_next;
}

static svt_hip_warp_fit_group fit_group(int bsize, uint32_t n, int ncand) {
    svt_hip_warp_fit_group G = {};
    G.bsize = bsize; G.nblocks = n; G.ncand = ncand;
    G.d_samples = (const svt_hip_warp_samples*)dev(); G.d_blk = (const svt_hip_inter_blk*)dev(); G.d_model = (svt_hip_warp_model*)dev();
    G.d_nvalid = (uint32_t*)dev();
    return G;
}
static svt_hip_warp_pred_group pred_group(int ss, int bw, int bh, uint32_t n, int ncand, int nsel = 0, int first = 0) {
    svt_hip_warp_pred_group G = {};
    G.d_ref = dev(); G.ref_stride = 512; G.ss = ss; G.bwidth = bw; G.bheight = bh; G.nblocks = n; G.ncand = ncand;
    G.d_blk = (const svt_hip_inter_blk*)dev(); G.d_model = (const svt_hip_warp_model*)dev();
    if (nsel) { G.d_sel = (const uint8_t*)dev(); G.n = nsel; G.sel_first = first; }
    G.d_pred = dev(); G.pred_stride = 0; G.d_src = dev(); G.src_stride = 512; G.d_dist = (uint64_t*)dev();
    return G;
}

static int fit_check(const std::vector<svt_hip_warp_fit_group>& v) { return warp_fit_check(v.data(), (int)v.size()); }
static int pred_check(const std::vector<svt_hip_warp_pred_group>& v, uint32_t w = 128, uint32_t h = 64, int bd = 8, int metric = SVT_HIP_FAST_SAD) {
    return warp_pred_check(v.data(), (int)v.size(), w, h, bd, metric);
}

static int fit_refusals() {
    const std::vector<svt_hip_warp_fit_group> good = {fit_group(3, 10, 1), fit_group(6, 7, 13), fit_group(12, 1, 64), fit_group(20, 0, 2)};
    CHECK(fit_check(good) == SVT_HIP_OK);
    CHECK(warp_fit_check(nullptr, 0) == SVT_HIP_OK && warp_fit_check(nullptr, 1) == INVALID && warp_fit_check(good.data(), -1) == INVALID);
    // every block size: accepted exactly when both sides are 8 .. 64
    for (int b = -1; b <= 22; b++) {
        std::vector<svt_hip_warp_fit_group> v = good;
        v[0].bsize = b;
        const bool ok = b >= 0 && b < 22 && kBsizeW[b] >= 8 && kBsizeH[b] >= 8 && kBsizeW[b] <= 64 && kBsizeH[b] <= 64;
        CHECK(fit_check(v) == (ok ? SVT_HIP_OK : INVALID));
    }
    using Edit = std::function<void(svt_hip_warp_fit_group&)>;
    const Edit edits[] = {
        [](auto& G) { G.bsize = 0; }, [](auto& G) { G.bsize = 2; }, [](auto& G) { G.bsize = 13; }, [](auto& G) { G.bsize = 16; },
        [](auto& G) { G.ncand = 0; }, [](auto& G) { G.ncand = -1; }, [](auto& G) { G.ncand = 65; },
        [](auto& G) { G.d_samples = nullptr; }, [](auto& G) { G.d_blk = nullptr; }, [](auto& G) { G.d_model = nullptr; },
        [](auto& G) { G.d_samples = (const svt_hip_warp_samples*)((const char*)G.d_samples + 2); },
        [](auto& G) { G.d_blk = (const svt_hip_inter_blk*)((const char*)G.d_blk + 2); },
        [](auto& G) { G.d_model = (svt_hip_warp_model*)((char*)G.d_model + 1); }, [](auto& G) { G.d_nvalid = (uint32_t*)((char*)G.d_nvalid + 2); },
    };
    for (size_t gi = 0; gi < good.size(); gi++) {
        int k = 0;
        for (const Edit& e : edits) {
            std::vector<svt_hip_warp_fit_group> v = good;
            e(v[gi]);
            if (fit_check(v) != INVALID) { fprintf(stderr, "fit edit %d of group %zu was accepted\n", k, gi); return 1; }
            k++;
        }
    }
    {
        std::vector<svt_hip_warp_fit_group> v = good;
        v[0].d_nvalid = nullptr;                                           // optional
        v[1].nblocks = 0xffffffffu;                                        // four blocks a workgroup: 2^30 workgroups
        CHECK(fit_check(v) == SVT_HIP_OK);
    }
    return 0;
}

static int pred_refusals() {
    const std::vector<svt_hip_warp_pred_group> good = {pred_group(0, 16, 16, 10, 1), pred_group(1, 32, 16, 7, 13), pred_group(0, 64, 64, 1, 3, 2, 5),
                                                       pred_group(0, 8, 8, 0, 1)};
    CHECK(pred_check(good) == SVT_HIP_OK);
    CHECK(pred_check(good, 128, 64, 10, SVT_HIP_FAST_SSD) == SVT_HIP_OK);
    CHECK(warp_pred_check(nullptr, 0, 128, 64, 8, 0) == SVT_HIP_OK && warp_pred_check(nullptr, 1, 128, 64, 8, 0) == INVALID);
    CHECK(warp_pred_check(good.data(), -1, 128, 64, 8, 0) == INVALID);
    for (int bd : {0, 7, 9, 12, 16}) CHECK(pred_check(good, 128, 64, bd) == INVALID);
    for (int m : {-1, 2, 100}) CHECK(pred_check(good, 128, 64, 8, m) == INVALID);
    for (uint32_t w : {0u, 4u, 100u, 132u, 16392u}) CHECK(pred_check(good, w, 64) == INVALID);
    for (uint32_t h : {0u, 4u, 68u, 16392u}) CHECK(pred_check(good, 128, h) == INVALID);
    CHECK(pred_check(good, 16384, 16384) == SVT_HIP_OK);
    CHECK(pred_check(good, 56, 64) == INVALID && pred_check(good, 128, 56) == INVALID);          // the 64x64 group does not fit the picture
    using Edit = std::function<void(svt_hip_warp_pred_group&)>;
    const Edit edits[] = {
        [](auto& G) { G.ss = 2; }, [](auto& G) { G.ss = -1; },
        [](auto& G) { G.bwidth = 0; }, [](auto& G) { G.bwidth = 4; }, [](auto& G) { G.bwidth = 12; }, [](auto& G) { G.bwidth = 128; }, [](auto& G) { G.bwidth = -8; },
        [](auto& G) { G.bheight = 4; }, [](auto& G) { G.bheight = 24; }, [](auto& G) { G.bheight = 128; },
        [](auto& G) { G.ss = 1; G.bwidth = 8; G.bheight = 16; }, [](auto& G) { G.ss = 1; G.bwidth = 16; G.bheight = 8; },
        [](auto& G) { G.ncand = 0; }, [](auto& G) { G.ncand = 65; },
        [](auto& G) { G.d_ref = nullptr; }, [](auto& G) { G.d_blk = nullptr; }, [](auto& G) { G.d_model = nullptr; },
        [](auto& G) { G.d_pred = nullptr; G.d_src = nullptr; G.d_dist = nullptr; },
        [](auto& G) { G.d_src = nullptr; }, [](auto& G) { G.d_dist = nullptr; },
        [](auto& G) { G.d_dist = (uint64_t*)((char*)G.d_dist + 4); }, [](auto& G) { G.d_blk = (const svt_hip_inter_blk*)((const char*)G.d_blk + 2); },
        [](auto& G) { G.d_model = (const svt_hip_warp_model*)((const char*)G.d_model + 2); }, [](auto& G) { G.d_pred = (char*)G.d_pred + 8; },
        [](auto& G) { G.pred_stride = (uint32_t)(G.bwidth >> G.ss) - 1; }, [](auto& G) { G.pred_stride = 1; },
        // d_sel comes with n and sel_first, and they with it
        [](auto& G) { if (G.d_sel) G.n = 0; else G.n = 2; }, [](auto& G) { if (G.d_sel) G.n = 65; else G.sel_first = 1; },
        [](auto& G) { if (G.d_sel) G.sel_first = -1; else G.n = -1; }, [](auto& G) { if (G.d_sel) G.sel_first = 256; else { G.n = 3; G.sel_first = 2; } },
    };
    for (size_t gi = 0; gi < good.size(); gi++) {
        int k = 0;
        for (const Edit& e : edits) {
            std::vector<svt_hip_warp_pred_group> v = good;
            e(v[gi]);
            if (pred_check(v) != INVALID) { fprintf(stderr, "pred edit %d of group %zu was accepted\n", k, gi); return 1; }
            k++;
        }
    }
    // what is allowed: the distortion alone, the prediction alone, a strided prediction at any alignment, a stride equal to the width
    {
        std::vector<svt_hip_warp_pred_group> v = good;
        v[1].d_pred = nullptr;
        v[2].d_src = nullptr; v[2].d_dist = nullptr;
        v[0].pred_stride = 16; v[0].d_pred = (char*)v[0].d_pred + 3;
        v[2].sel_first = 255; v[2].n = 64;
        CHECK(pred_check(v) == SVT_HIP_OK);
        v[1].d_pred = dev(); v[1].pred_stride = 16;                                    // chroma of 32 x 16: the plane block is 16 wide
        CHECK(pred_check(v) == SVT_HIP_OK);
        v[1].pred_stride = 15;
        CHECK(pred_check(v) == INVALID);
    }
    // nblocks * slots against one launch
    {
        std::vector<svt_hip_warp_pred_group> v = good;
        v[2].nblocks = 0x7fffffffu / 2;                                                // 64x64, two survivors: a workgroup per slot
        CHECK(pred_check(v) == SVT_HIP_OK);
        v[2].nblocks = 0x40000000u;
        CHECK(pred_check(v) == INVALID);
        v[2].nblocks = 1; v[3].nblocks = 0x7fffffffu;                                  // 8x8: four slots a workgroup
        CHECK(pred_check(v) == SVT_HIP_OK);
        v[3].nblocks = 0x80000000u;
        CHECK(pred_check(v) == INVALID);
        v[3].nblocks = 0x7fffffffu; v[3].ncand = 2;
        CHECK(pred_check(v) == INVALID);
    }
    return 0;
}

static int geometry() {
    for (int lw = 3; lw <= 6; lw++)
        for (int lh = 3; lh <= 6; lh++) {
            const WarpGeom G = warp_geom(lw, lh);
            const int tiles = 1 << G.ltpb;
            CHECK(tiles * 64 == (1 << lw) * (1 << lh) && (1 << G.ltx) * 8 == (1 << lw));
            CHECK(G.slots_per_wg * tiles == WP_WAVES * G.rounds);                        // the four waves are used exactly
            CHECK(G.rounds == 1 || G.slots_per_wg == 1);
            CHECK(G.waves_per_slot * G.slots_per_wg == WP_WAVES && G.waves_per_slot * G.rounds == tiles);
            CHECK(G.rounds * 64 <= 1024);                                                // a wave's 32-bit sum: at most 1024 samples of 1023^2
        }
    struct { int lw, lh; WarpGeom g; } want[] = {
        {3, 3, {0, 0, 4, 1, 1}}, {4, 3, {1, 1, 2, 1, 2}}, {3, 4, {0, 1, 2, 1, 2}}, {4, 4, {1, 2, 1, 1, 4}},
        {5, 4, {2, 3, 1, 2, 4}}, {6, 5, {3, 5, 1, 8, 4}}, {6, 6, {3, 6, 1, 16, 4}}, {3, 6, {0, 3, 1, 2, 4}},
    };
    for (const auto& w : want) {
        const WarpGeom G = warp_geom(w.lw, w.lh);
        CHECK(G.ltx == w.g.ltx && G.ltpb == w.g.ltpb && G.slots_per_wg == w.g.slots_per_wg && G.rounds == w.g.rounds && G.waves_per_slot == w.g.waves_per_slot);
    }
    for (int ss = 0; ss < 2; ss++)
        for (int lw = 3; lw <= 6; lw++)
            for (int n : {0, 1, 64})
                for (int first : {0, 7, 255}) {
                    const WarpShape s = warp_shape_unpack(warp_shape_pack({ss, lw, 9 - lw, 64 - n / 2, n, first}));
                    CHECK(s.ss == ss && s.lw == lw && s.lh == 9 - lw && s.ncand == 64 - n / 2 && s.n == n && s.sel_first == first);
                }
    return 0;
}

struct FitLaunch { WarpFitDesc desc; uint32_t total; };
struct PredLaunch { WarpPredDesc desc; uint32_t total; };

static int tables() {
    // fit: 10 blocks, 7 blocks, an empty group, 1 block -> 3, 2, 1 workgroups
    const std::vector<svt_hip_warp_fit_group> f = {fit_group(3, 10, 1), fit_group(9, 7, 13), fit_group(6, 0, 4), fit_group(21, 1, 64)};
    CHECK(fit_check(f) == SVT_HIP_OK);
    std::vector<FitLaunch> fgot;
    auto frec = [&](const WarpFitDesc& fd, uint32_t total) -> int { fgot.push_back({fd, total}); return 0; };
    CHECK(warp_fit_enqueue(f.data(), (int)f.size(), frec) == 0);
    CHECK(fgot.size() == 1 && fgot[0].total == 6 && fgot[0].desc.ngroups == 3);
    const int fsrc[3] = {0, 1, 3}, fbw[3] = {8, 32, 64}, fbh[3] = {8, 32, 16};
    const uint32_t fend[3] = {3, 5, 6};
    for (int i = 0; i < 3; i++) {
        const svt_hip_warp_fit_group& G = f[fsrc[i]];
        const WarpFitGroupDev& E = fgot[0].desc.g[i];
        CHECK(E.wg_end == fend[i] && E.bw == fbw[i] && E.bh == fbh[i] && E.ncand == G.ncand && E.nblocks == G.nblocks);
        CHECK(E.samples == G.d_samples && E.blk == G.d_blk && E.model == G.d_model && E.nvalid == G.d_nvalid);
    }
    // pred: luma 8x8 x 10 x 1, chroma of 32x16 x 7 x 13, luma 64x64 x 3 with 2 survivors of 3, an empty group, luma 16x8 x 5 x 2
    const std::vector<svt_hip_warp_pred_group> v = {pred_group(0, 8, 8, 10, 1), pred_group(1, 32, 16, 7, 13), pred_group(0, 64, 64, 3, 3, 2, 5),
                                                    pred_group(0, 16, 16, 0, 1), pred_group(0, 16, 8, 5, 2)};
    CHECK(pred_check(v, 128, 64, 10, SVT_HIP_FAST_SSD) == SVT_HIP_OK);
    std::vector<WarpGroupPlan> plans(v.size());
    CHECK(warp_pred_plan(v.data(), (int)v.size(), plans.data()) == 4);
    const int src[4] = {0, 1, 2, 4}, lw[4] = {3, 4, 6, 4}, lh[4] = {3, 3, 6, 3};
    const uint32_t slots[4] = {10, 91, 6, 10}, wgs[4] = {3, 46, 6, 5}, ends[4] = {3, 49, 55, 60};
    for (int i = 0; i < 4; i++) CHECK(plans[i].src == src[i] && plans[i].lw == lw[i] && plans[i].lh == lh[i] && plans[i].nslots == slots[i] && plans[i].wgs == wgs[i]);
    std::vector<PredLaunch> got;
    auto rec = [&](const WarpPredDesc& fd, uint32_t total) -> int { got.push_back({fd, total}); return 0; };
    CHECK(warp_pred_enqueue(v.data(), (int)v.size(), 128, 64, 10, SVT_HIP_FAST_SSD, rec) == 0);
    CHECK(got.size() == 1 && got[0].total == 60 && got[0].desc.ngroups == 4);
    const WarpPredDesc& D = got[0].desc;
    CHECK(D.pic_w == 128 && D.pic_h == 64 && D.bd == 10 && D.metric == SVT_HIP_FAST_SSD);
    for (int i = 0; i < 4; i++) {
        const svt_hip_warp_pred_group& G = v[src[i]];
        const WarpPredGroupDev& E = D.g[i];
        const WarpShape s = warp_shape_unpack(E.shape);
        CHECK(E.wg_end == ends[i] && E.nslots == slots[i] && s.lw == lw[i] && s.lh == lh[i] && s.ss == G.ss && s.ncand == G.ncand);
        CHECK(s.n == (G.d_sel ? G.n : 0) && s.sel_first == (G.d_sel ? G.sel_first : 0));
        CHECK(E.ref == G.d_ref && E.blk == G.d_blk && E.model == G.d_model && E.sel == G.d_sel && E.pred == G.d_pred && E.src == G.d_src && (void*)E.dist == (void*)G.d_dist);
        CHECK(E.ref_stride == G.ref_stride && E.pred_stride == G.pred_stride && E.src_stride == G.src_stride);
    }
    // more groups than a table holds: a launch per WP_MAX_GROUPS, in list order; a failing launch ends the call with its code
    std::vector<svt_hip_warp_pred_group> many;
    for (int i = 0; i < 2 * WP_MAX_GROUPS + 5; i++) many.push_back(pred_group(0, 16, 16, (uint32_t)(i + 1), 1));
    got.clear();
    CHECK(warp_pred_enqueue(many.data(), (int)many.size(), 128, 64, 8, SVT_HIP_FAST_SAD, rec) == 0);
    CHECK(got.size() == 3 && got[0].desc.ngroups == WP_MAX_GROUPS && got[1].desc.ngroups == WP_MAX_GROUPS && got[2].desc.ngroups == 5);
    uint32_t first = 1;
    for (const PredLaunch& L : got) {
        uint32_t end = 0;
        for (int i = 0; i < L.desc.ngroups; i++) { end += first++; CHECK(L.desc.g[i].wg_end == end && L.desc.g[i].nslots == first - 1); }
        CHECK(L.total == end);
    }
    int calls = 0;
    CHECK(warp_pred_enqueue(many.data(), (int)many.size(), 128, 64, 8, SVT_HIP_FAST_SAD, [&](const WarpPredDesc&, uint32_t) { return ++calls == 2 ? -4 : 0; }) == -4);
    CHECK(calls == 2);
    std::vector<svt_hip_warp_fit_group> fmany;
    for (int i = 0; i < WP_MAX_GROUPS + 1; i++) fmany.push_back(fit_group(6, 4, 1));
    fgot.clear();
    CHECK(warp_fit_enqueue(fmany.data(), (int)fmany.size(), frec) == 0 && fgot.size() == 2 && fgot[0].total == WP_MAX_GROUPS && fgot[1].total == 1);
    // no groups, or only empty ones: nothing is launched
    got.clear(); fgot.clear();
    const std::vector<svt_hip_warp_pred_group> none = {pred_group(0, 8, 8, 0, 1), pred_group(1, 16, 16, 0, 1)};
    CHECK(warp_pred_enqueue(none.data(), 2, 128, 64, 8, 0, rec) == 0 && warp_pred_enqueue(nullptr, 0, 128, 64, 8, 0, rec) == 0 && got.empty());
    const std::vector<svt_hip_warp_fit_group> fnone = {fit_group(6, 0, 1)};
    CHECK(warp_fit_enqueue(fnone.data(), 1, frec) == 0 && warp_fit_enqueue(nullptr, 0, frec) == 0 && fgot.empty());
    return 0;
}

static int filter_tables() {
    // what the kernels assume: rows sum to 128 (asserted at compile time too), taps in a signed byte, the closing row, Div_Lut monotone
    for (int r = 0; r < svtwarp::kWarpRows; r++) {
        int s = 0;
        for (int k = 0; k < 8; k++) s += svtwarp::kWarpFilter.t[r][k];
        CHECK(s == 128);
    }
    for (int k = 0; k < 8; k++) CHECK(svtwarp::kWarpFilter.t[192][k] == svtwarp::kWarpFilter.t[191][k]);
    CHECK(svtwarp::kWarpFilter.t[64][3] == 127 && svtwarp::kWarpFilter.t[64][4] == 1 && svtwarp::kWarpFilter.t[128][3] == 1 && svtwarp::kWarpFilter.t[128][4] == 127);
    for (int i = 1; i <= 256; i++) CHECK(svtwarp::kDivLut.v[i] < svtwarp::kDivLut.v[i - 1]);
    CHECK(svtwarp::kDivLut.v[1] == 16320 && svtwarp::kDivLut.v[128] == 10923 && svtwarp::kDivLut.v[255] == 8208);
    return 0;
}

int main() {
    if (fit_refusals() || pred_refusals() || geometry() || tables() || filter_tables()) return 1;
    printf("ok\n");
    return 0;
}

// csrc/interp_plan.h on the CPU: what svt_hip_interp_sse_frame / _decide_frame / _search_frame decide on the host before they touch a
// device.  A valid group list is accepted and the same list with one field changed is refused, for every clause of interp_sse_check and
// interp_decide_check; the (group, plane) entries, workgroup counts and group tables of a mixed list equal hand-computed values; a list
// longer than one launch's table is cut where the table is full; the one-call search's scratch size and carving.  "Device" pointers are
// addresses inside a host array that nothing dereferences.  Plain C++17 (g++), linked with csrc/host_err.cpp, also built under
// -fsanitize=address,undefined by tests/test_interp_plan_host.py.  Exit status 0 and "ok" when every case holds.
#include <stdio.h>
#include <stdlib.h>

#include <functional>
#include <vector>

#include "../../cidana-svt-av1_amd/csrc/interp_plan.h"

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

static svt_hip_interp_sse_group sgroup(int bw, int bh, uint32_t n) {
    svt_hip_interp_sse_group G = {};
    for (int p = 0; p < 3; p++) {
        G.d_ref[0][p] = (const uint8_t*)dev(); G.d_ref[1][p] = (const uint8_t*)dev(); G.d_src[p] = (const uint8_t*)dev();
        G.ref_stride[p] = 512u >> (p > 0); G.src_stride[p] = 256u >> (p > 0);
    }
    G.bwidth = bw; G.bheight = bh; G.nblocks = n; G.d_blk = (const svt_hip_inter_blk*)dev(); G.d_sse = (uint32_t*)dev();
    return G;
}

static svt_hip_interp_decide_group dgroup(int bw, int bh, uint32_t n) {
    svt_hip_interp_decide_group G = {};
    G.bwidth = bw; G.bheight = bh; G.nblocks = n; G.d_sse = (const uint32_t*)dev(); G.d_ctx = (const uint8_t*)dev();
    G.d_searchable = (const uint8_t*)dev(); G.d_decision = (svt_hip_interp_decision*)dev(); G.d_blk = (const svt_hip_inter_blk*)dev();
    G.d_blk_out = (svt_hip_inter_blk*)dev();
    return G;
}

static int32_t g_rates[48];
static svt_hip_interp_params params(int use_uv = 1, int mode = SVT_HIP_INTERP_FULL) {
    svt_hip_interp_params P = {};
    P.full_lambda = 3000; P.ac_dequant_q3 = 400; P.d_rates = g_rates; P.use_uv = use_uv; P.mode = mode;
    return P;
}

static int scheck(const std::vector<svt_hip_interp_sse_group>& v, uint32_t w = 128, uint32_t h = 64, int bd = 8, int use_uv = 1) {
    return interp_sse_check(v.data(), (int)v.size(), w, h, bd, use_uv);
}

static int sse_refusals() {
    const std::vector<svt_hip_interp_sse_group> good = {sgroup(16, 16, 10), sgroup(8, 32, 7), sgroup(64, 64, 1), sgroup(8, 8, 0)};
    CHECK(scheck(good) == SVT_HIP_OK && scheck(good, 128, 64, 8, 0) == SVT_HIP_OK);
    CHECK(interp_sse_check(nullptr, 0, 128, 64, 8, 1) == SVT_HIP_OK);
    CHECK(interp_sse_check(nullptr, 1, 128, 64, 8, 1) == INVALID && interp_sse_check(good.data(), -1, 128, 64, 8, 1) == INVALID);
    for (int bd : {0, 7, 9, 10, 12, 16}) CHECK(scheck(good, 128, 64, bd) == INVALID);          // 8-bit only
    for (int uv : {-1, 2, 3}) CHECK(scheck(good, 128, 64, 8, uv) == INVALID);
    for (uint32_t w : {0u, 4u, 100u, 132u, 16392u}) CHECK(scheck(good, w, 64) == INVALID);
    for (uint32_t h : {0u, 4u, 68u, 16392u}) CHECK(scheck(good, 128, h) == INVALID);
    CHECK(scheck(good, 16384, 16384) == SVT_HIP_OK);
    CHECK(scheck(good, 56, 64) == INVALID && scheck(good, 128, 56) == INVALID);                 // the 64x64 group does not fit
    using Edit = std::function<void(svt_hip_interp_sse_group&)>;
    const Edit edits[] = {
        [](auto& G) { G.bwidth = 0; }, [](auto& G) { G.bwidth = 4; }, [](auto& G) { G.bwidth = 12; }, [](auto& G) { G.bwidth = 128; }, [](auto& G) { G.bwidth = -8; },
        [](auto& G) { G.bheight = 4; }, [](auto& G) { G.bheight = 24; }, [](auto& G) { G.bheight = 128; },
        [](auto& G) { G.d_blk = nullptr; }, [](auto& G) { G.d_blk = (const svt_hip_inter_blk*)((const char*)G.d_blk + 2); },
        [](auto& G) { G.d_sse = nullptr; }, [](auto& G) { G.d_sse = (uint32_t*)((char*)G.d_sse + 2); },
        [](auto& G) { G.d_ref[0][0] = nullptr; }, [](auto& G) { G.d_ref[0][1] = nullptr; }, [](auto& G) { G.d_ref[0][2] = nullptr; },
        [](auto& G) { G.d_src[0] = nullptr; }, [](auto& G) { G.d_src[1] = nullptr; }, [](auto& G) { G.d_src[2] = nullptr; },
    };
    for (size_t gi = 0; gi < good.size(); gi++) {
        int k = 0;
        for (const Edit& e : edits) {
            std::vector<svt_hip_interp_sse_group> v = good;
            e(v[gi]);
            if (scheck(v) != INVALID) { fprintf(stderr, "sse edit %d of group %zu was accepted\n", k, gi); return 1; }
            k++;
        }
    }
    {   // allowed: no list 1 at all; without use_uv no chroma plane; a table at any 4-byte address; the search's missing table
        std::vector<svt_hip_interp_sse_group> v = good;
        for (int p = 0; p < 3; p++) v[0].d_ref[1][p] = nullptr;
        v[1].d_sse = (uint32_t*)((char*)v[1].d_sse + 4);
        CHECK(scheck(v) == SVT_HIP_OK);
        for (int p = 1; p < 3; p++) { v[2].d_ref[0][p] = nullptr; v[2].d_src[p] = nullptr; }
        CHECK(scheck(v) == INVALID && scheck(v, 128, 64, 8, 0) == SVT_HIP_OK);
        v = good;
        v[1].d_sse = nullptr;
        CHECK(interp_sse_check(v.data(), (int)v.size(), 128, 64, 8, 1, true) == SVT_HIP_OK && scheck(v) == INVALID);
    }
    {   // nblocks against one launch: 64x64 luma takes a workgroup per block, 8x8 sixteen blocks per workgroup
        std::vector<svt_hip_interp_sse_group> v = good;
        v[2].nblocks = 0x7fffffffu;
        CHECK(scheck(v) == SVT_HIP_OK);
        v[2].nblocks = 0x80000000u;
        CHECK(scheck(v) == INVALID);
        v[2].nblocks = 1; v[3].nblocks = 0xffffffffu;
        CHECK(scheck(v) == SVT_HIP_OK);
    }
    return 0;
}

static int decide_refusals() {
    const std::vector<svt_hip_interp_decide_group> good = {dgroup(16, 16, 10), dgroup(32, 8, 300), dgroup(64, 64, 0)};
    svt_hip_interp_params P = params();
    CHECK(interp_decide_check(good.data(), 3, &P) == SVT_HIP_OK);
    CHECK(interp_decide_check(nullptr, 0, &P) == SVT_HIP_OK && interp_decide_check(nullptr, 1, &P) == INVALID);
    CHECK(interp_decide_check(good.data(), 3, nullptr) == INVALID);
    for (int m : {-1, 3, 100}) { P = params(1, m); CHECK(interp_decide_check(good.data(), 3, &P) == INVALID); }
    for (int m : {SVT_HIP_INTERP_DUAL_FAST, SVT_HIP_INTERP_FULL, SVT_HIP_INTERP_SINGLE}) { P = params(0, m); CHECK(interp_decide_check(good.data(), 3, &P) == SVT_HIP_OK); }
    for (int uv : {-1, 2}) { P = params(uv); CHECK(interp_decide_check(good.data(), 3, &P) == INVALID); }
    for (int q : {-1, -8, 32768, 70000}) { P = params(); P.ac_dequant_q3 = q; CHECK(interp_decide_check(good.data(), 3, &P) == INVALID); }
    for (int q : {0, 4, 32767}) { P = params(); P.ac_dequant_q3 = q; CHECK(interp_decide_check(good.data(), 3, &P) == SVT_HIP_OK); }
    P = params(); P.d_rates = nullptr; CHECK(interp_decide_check(good.data(), 3, &P) == INVALID);
    P = params(); P.d_rates = (const int32_t*)((const char*)g_rates + 2); CHECK(interp_decide_check(good.data(), 3, &P) == INVALID);
    P = params();
    using Edit = std::function<void(svt_hip_interp_decide_group&)>;
    const Edit edits[] = {
        [](auto& G) { G.bwidth = 4; }, [](auto& G) { G.bwidth = 48; }, [](auto& G) { G.bheight = 0; }, [](auto& G) { G.bheight = 128; },
        [](auto& G) { G.d_sse = nullptr; }, [](auto& G) { G.d_sse = (const uint32_t*)((const char*)G.d_sse + 2); },
        [](auto& G) { G.d_ctx = nullptr; }, [](auto& G) { G.d_searchable = nullptr; },
        [](auto& G) { G.d_decision = nullptr; }, [](auto& G) { G.d_decision = (svt_hip_interp_decision*)((char*)G.d_decision + 4); },
        [](auto& G) { G.d_blk = nullptr; }, [](auto& G) { G.d_blk = (const svt_hip_inter_blk*)((const char*)G.d_blk + 2); },
        [](auto& G) { G.d_blk_out = (svt_hip_inter_blk*)((char*)G.d_blk_out + 2); },
    };
    for (size_t gi = 0; gi < good.size(); gi++) {
        int k = 0;
        for (const Edit& e : edits) {
            std::vector<svt_hip_interp_decide_group> v = good;
            e(v[gi]);
            if (interp_decide_check(v.data(), 3, &P) != INVALID) { fprintf(stderr, "decide edit %d of group %zu was accepted\n", k, gi); return 1; }
            k++;
        }
    }
    {   // allowed: no records at all; in place; only the search's empty group goes without a table
        std::vector<svt_hip_interp_decide_group> v = good;
        v[0].d_blk = nullptr; v[0].d_blk_out = nullptr;
        v[1].d_blk_out = (svt_hip_inter_blk*)v[1].d_blk;
        CHECK(interp_decide_check(v.data(), 3, &P) == SVT_HIP_OK);
        v[2].d_sse = nullptr;
        CHECK(interp_decide_check(v.data(), 3, &P) == INVALID && interp_decide_check(v.data(), 3, &P, true) == SVT_HIP_OK);
        v[1].d_sse = nullptr;
        CHECK(interp_decide_check(v.data(), 3, &P, true) == INVALID);
    }
    return 0;
}

struct SseLaunch { InterpSseDesc desc; uint32_t total; };
struct DecLaunch { InterpDecideDesc desc; uint32_t total; };

static int tables() {
    // 8x8 x 100, 64x64 x 3, an empty group, 8x32 x 17, 64x32 x 5
    const std::vector<svt_hip_interp_sse_group> v = {sgroup(8, 8, 100), sgroup(64, 64, 3), sgroup(16, 16, 0), sgroup(8, 32, 17), sgroup(64, 32, 5)};
    CHECK(scheck(v) == SVT_HIP_OK);
    std::vector<SseLaunch> got;
    auto rec = [&](const InterpSseDesc& fd, uint32_t total) -> int { got.push_back({fd, total}); return 0; };
    CHECK(interp_sse_enqueue(v.data(), (int)v.size(), 128, 64, 1, rec) == 0);
    CHECK(got.size() == 1 && got[0].desc.ngroups == 12 && got[0].desc.pic_w == 128 && got[0].desc.pic_h == 64);
    // per (group, plane): luma 8x8 16 blocks a workgroup, its 4x4 chroma 64; 64x64 one, its 32x32 chroma one; 8x32 four, 4x16 sixteen;
    // 64x32 one, 32x16 two
    const int src[4] = {0, 1, 3, 4};
    const int lw[4][2] = {{3, 2}, {6, 5}, {3, 2}, {6, 5}}, lh[4][2] = {{3, 2}, {6, 5}, {5, 4}, {5, 4}};
    const uint32_t wgs[4][2] = {{7, 2}, {3, 3}, {5, 2}, {5, 3}};
    uint32_t end = 0;
    for (int i = 0; i < 4; i++)
        for (int p = 0; p < 3; p++) {
            const svt_hip_interp_sse_group& G = v[src[i]];
            const InterpSseGroupDev& E = got[0].desc.g[3 * i + p];
            end += wgs[i][p > 0];
            CHECK(E.wg_end == end && E.lw == lw[i][p > 0] && E.lh == lh[i][p > 0] && E.ss == (p > 0) && E.nblocks == G.nblocks && E.sse_stride == 27);
            CHECK(E.ref[0] == G.d_ref[0][p] && E.ref[1] == G.d_ref[1][p] && E.src == G.d_src[p] && E.blk == G.d_blk && E.sse == G.d_sse + 9 * p);
            CHECK(E.ref_stride == G.ref_stride[p] && E.src_stride == G.src_stride[p]);
        }
    CHECK(got[0].total == end);
    // luma only: an entry per group, a block's entries 9 words apart
    got.clear();
    CHECK(interp_sse_enqueue(v.data(), (int)v.size(), 128, 64, 0, rec) == 0);
    CHECK(got.size() == 1 && got[0].desc.ngroups == 4 && got[0].total == 7 + 3 + 5 + 5 && got[0].desc.g[2].sse_stride == 9 && got[0].desc.g[2].ss == 0);
    // more entries than a table holds: with use_uv 2 * SVT_HIP_INTER_PRED_MAX_GROUPS + 5 groups are three times as many entries
    static_assert(SVT_HIP_INTER_PRED_MAX_GROUPS == IP_MAX_GROUPS, "svt_hip_dsp.h");
    std::vector<svt_hip_interp_sse_group> many;
    for (int i = 0; i < 2 * IP_MAX_GROUPS + 5; i++) many.push_back(sgroup(16, 16, (uint32_t)(4 * (i + 1))));
    got.clear();
    CHECK(interp_sse_enqueue(many.data(), (int)many.size(), 128, 64, 1, rec) == 0);
    const int entries = 3 * (2 * IP_MAX_GROUPS + 5);
    CHECK((int)got.size() == (entries + IP_MAX_GROUPS - 1) / IP_MAX_GROUPS);
    int seen = 0;
    for (const SseLaunch& L : got) {
        CHECK(L.desc.ngroups == (entries - seen < IP_MAX_GROUPS ? entries - seen : IP_MAX_GROUPS));
        uint32_t e = 0;
        for (int i = 0; i < L.desc.ngroups; i++, seen++) {
            const uint32_t n = 4u * (uint32_t)(seen / 3 + 1);
            e += seen % 3 ? (n + 15) / 16 : n / 4;                // 16x16 luma: four blocks a workgroup; 8x8 chroma: sixteen
            CHECK(L.desc.g[i].wg_end == e && L.desc.g[i].nblocks == n && L.desc.g[i].ss == (seen % 3 > 0));
        }
        CHECK(L.total == e);
    }
    got.clear();
    CHECK(interp_sse_enqueue(many.data(), (int)many.size(), 128, 64, 0, rec) == 0);
    CHECK(got.size() == 3 && got[0].desc.ngroups == IP_MAX_GROUPS && got[1].desc.ngroups == IP_MAX_GROUPS && got[2].desc.ngroups == 5);
    int calls = 0;
    CHECK(interp_sse_enqueue(many.data(), (int)many.size(), 128, 64, 1, [&](const InterpSseDesc&, uint32_t) { return ++calls == 2 ? -4 : 0; }) == -4);
    CHECK(calls == 2);
    got.clear();
    const std::vector<svt_hip_interp_sse_group> none = {sgroup(8, 8, 0), sgroup(16, 16, 0)};
    CHECK(interp_sse_enqueue(none.data(), 2, 128, 64, 1, rec) == 0 && interp_sse_enqueue(nullptr, 0, 128, 64, 1, rec) == 0 && got.empty());

    // the walk: a thread a block, ID_MAX_GROUPS groups a launch
    std::vector<svt_hip_interp_decide_group> dv = {dgroup(8, 8, 1), dgroup(64, 32, 257), dgroup(16, 16, 0), dgroup(8, 32, 512)};
    std::vector<DecLaunch> dgot;
    auto drec = [&](const InterpDecideDesc& fd, uint32_t total) -> int { dgot.push_back({fd, total}); return 0; };
    const svt_hip_interp_params P = params(0, SVT_HIP_INTERP_SINGLE);
    CHECK(interp_decide_enqueue(dv.data(), (int)dv.size(), P, drec) == 0);
    CHECK(dgot.size() == 1 && dgot[0].desc.ngroups == 3 && dgot[0].total == 1 + 2 + 2);
    const InterpDecideDesc& DD = dgot[0].desc;
    CHECK(DD.lambda == 3000 && DD.qstep == 50 && DD.use_uv == 0 && DD.mode == SVT_HIP_INTERP_SINGLE && DD.rates == g_rates);
    CHECK(DD.g[0].wg_end == 1 && DD.g[1].wg_end == 3 && DD.g[2].wg_end == 5 && DD.g[0].nlog2_y == 6 && DD.g[1].nlog2_y == 11 && DD.g[2].nlog2_y == 8);
    CHECK(DD.g[1].sse == dv[1].d_sse && DD.g[1].ctx == dv[1].d_ctx && DD.g[1].searchable == dv[1].d_searchable && (void*)DD.g[1].decision == (void*)dv[1].d_decision &&
          DD.g[1].blk == dv[1].d_blk && DD.g[1].blk_out == dv[1].d_blk_out && DD.g[1].nblocks == 257);
    std::vector<svt_hip_interp_decide_group> dmany;
    for (int i = 0; i < 2 * ID_MAX_GROUPS + 3; i++) dmany.push_back(dgroup(16, 16, 256u * (uint32_t)(i + 1)));
    dgot.clear();
    CHECK(interp_decide_enqueue(dmany.data(), (int)dmany.size(), P, drec) == 0);
    CHECK(dgot.size() == 3 && dgot[0].desc.ngroups == ID_MAX_GROUPS && dgot[2].desc.ngroups == 3 && dgot[2].desc.g[2].wg_end == 65 + 66 + 67);
    return 0;
}

static int scratch() {
    std::vector<svt_hip_interp_search_group> v(4);
    const uint32_t n[4] = {10, 0, 7, 33};
    for (int i = 0; i < 4; i++) {
        v[i] = svt_hip_interp_search_group{};
        v[i].sse = sgroup(16, 16, n[i]);
        v[i].sse.d_sse = nullptr;
        v[i].d_ctx = (const uint8_t*)dev(); v[i].d_searchable = (const uint8_t*)dev(); v[i].d_decision = (svt_hip_interp_decision*)dev();
    }
    uint32_t* const own = (uint32_t*)dev();
    v[2].sse.d_sse = own;                                                                       // this group keeps its table
    // per carved group nblocks * planes * 36 bytes, rounded up to 16
    CHECK(interp_search_scratch_bytes(v.data(), 4, 1) == 1088 + 3568 && interp_search_scratch_bytes(v.data(), 4, 0) == 368 + 1200);
    CHECK(interp_search_scratch_bytes(v.data(), 0, 1) == 0 && interp_search_scratch_bytes(nullptr, 4, 1) == 0 && interp_search_scratch_bytes(v.data(), 4, 2) == 0);
    CHECK(interp_sse_bytes(1, 0) == 48 && interp_sse_bytes(1, 1) == 112 && interp_sse_bytes(0, 1) == 0);
    alignas(16) static char buf[8192];
    svt_hip_interp_params P = params();
    InterpStages st;
    CHECK(interp_search_plan(v.data(), 4, &P, buf, sizeof(buf), &st) == SVT_HIP_OK);
    CHECK((char*)st.sg[0].d_sse == buf && st.sg[1].d_sse == nullptr && st.sg[2].d_sse == own && (char*)st.sg[3].d_sse == buf + 1088);
    for (int i = 0; i < 4; i++) {
        CHECK(st.dg[i].d_sse == st.sg[i].d_sse && st.dg[i].nblocks == n[i] && st.dg[i].bwidth == 16 && st.dg[i].bheight == 16 && st.dg[i].d_ctx == v[i].d_ctx &&
              st.dg[i].d_searchable == v[i].d_searchable && st.dg[i].d_decision == v[i].d_decision && st.dg[i].d_blk == v[i].sse.d_blk && st.dg[i].d_blk_out == nullptr);
    }
    CHECK(interp_sse_check(st.sg.data(), 4, 128, 64, 8, 1, true) == SVT_HIP_OK && interp_decide_check(st.dg.data(), 4, &P, true) == SVT_HIP_OK);
    // the scratch: exactly enough is enough; one byte less, NULL or misaligned is refused; nothing is needed when every table is the caller's
    CHECK(interp_search_plan(v.data(), 4, &P, buf, 1088 + 3568, &st) == SVT_HIP_OK);
    CHECK(interp_search_plan(v.data(), 4, &P, buf, 1088 + 3567, &st) == INVALID);
    CHECK(interp_search_plan(v.data(), 4, &P, nullptr, sizeof(buf), &st) == INVALID);
    CHECK(interp_search_plan(v.data(), 4, &P, buf + 8, sizeof(buf) - 8, &st) == INVALID);
    CHECK(interp_search_plan(v.data(), 4, nullptr, buf, sizeof(buf), &st) == INVALID);
    CHECK(interp_search_plan(nullptr, 4, &P, buf, sizeof(buf), &st) == INVALID);
    v[0].sse.d_sse = own; v[3].sse.d_sse = own;
    CHECK(interp_search_scratch_bytes(v.data(), 4, 1) == 0 && interp_search_plan(v.data(), 4, &P, nullptr, 0, &st) == SVT_HIP_OK);
    return 0;
}

int main() {
    if (sse_refusals() || decide_refusals() || tables() || scratch()) return 1;
    printf("ok\n");
    return 0;
}

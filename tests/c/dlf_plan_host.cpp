// csrc/dlf_plan.h on the CPU: dlf_check / dlf_search_check / dlf_mi_check (every refusal of the three deblocking calls: valid arguments
// are accepted, the same arguments with one field changed are refused, the neighbour of each bound accepted), the limit, level, side and
// length tables against closed forms written out here, the scratch size, and the level pick on synthetic tables (both branches, the
// rounds of SVT_HIP_DLF_NEED_LEVEL).  "Device" pointers are addresses inside a host array that nothing dereferences.
// Plain C++17 (g++), linked with csrc/host_err.cpp, built plain and under -fsanitize=address,undefined by tests/test_dlf_cpu.py and run
// directly.  Exit status 0 and "ok" when every case holds.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <functional>

#include "../../cidana-svt-av1_amd/csrc/dlf_plan.h"

using namespace svthost;

#define CHECK(c) do { if (!(c)) { fprintf(stderr, "%s:%d: %s (last error: %s)\n", __FILE__, __LINE__, #c, svt_hip_last_error()); return 1; } } while (0)
#define TRY(call) do { if (call) { fprintf(stderr, "  from %s:%d\n", __FILE__, __LINE__); return 1; } } while (0)
static const int INVALID = SVT_HIP_ERR_INVALID;

alignas(64) static char g_dev[64 << 20];
static char* at(size_t off) { return g_dev + off; }

static svt_hip_dlf_pic good_pic(bool in_place) {
    svt_hip_dlf_pic p{};
    const size_t plane = 4 << 20;
    for (int i = 0; i < 3; i++) {
        p.d_rec[i] = at(i * plane); p.d_src[i] = at((3 + i) * plane); p.d_dst[i] = in_place ? (void*)at(i * plane) : (void*)at((6 + i) * plane);
        p.rec_stride[i] = p.src_stride[i] = p.dst_stride[i] = i ? 960 : 1920;
        p.rec_pitch[i] = p.src_pitch[i] = p.dst_pitch[i] = 0;
    }
    p.d_mi = (const svt_hip_dlf_mi*)at(9 * plane); p.mi_stride = 480;
    p.width = 1920; p.height = 1080; p.bit_depth = 8; p.npics = 1;
    p.filter_level[0] = 20; p.filter_level[1] = 18; p.filter_level_u = 9; p.filter_level_v = 63;
    p.sharpness_level = 7; p.mode_ref_delta_enabled = 1;
    for (int i = 0; i < 8; i++) p.ref_deltas[i] = (int8_t)(i % 2 ? -63 : 63);
    p.mode_deltas[0] = -63; p.mode_deltas[1] = 63;
    return p;
}
using Change = std::function<void(svt_hip_dlf_pic&)>;
static int expect(const svt_hip_dlf_pic& good, bool search, const Change& change, int want, int line) {
    svt_hip_dlf_pic p = good;
    change(p);
    const int rc = dlf_check(&p, search);
    if (rc != want) { fprintf(stderr, "line %d: dlf_check gave %d, expected %d (%s)\n", line, rc, want, svt_hip_last_error()); return 1; }
    return 0;
}
#define REFUSED(search, ...) TRY(expect(good, search, [&](svt_hip_dlf_pic& a) { __VA_ARGS__; }, INVALID, __LINE__))
#define ACCEPTED(search, ...) TRY(expect(good, search, [&](svt_hip_dlf_pic& a) { __VA_ARGS__; }, SVT_HIP_OK, __LINE__))

static int test_check() {
    for (int in_place = 0; in_place < 2; in_place++) {
        const svt_hip_dlf_pic good = good_pic(in_place != 0);
        CHECK(dlf_check(&good, false) == SVT_HIP_OK && dlf_check(&good, true) == SVT_HIP_OK);
        CHECK(dlf_check(nullptr, false) == INVALID);
        for (int s = 0; s < 2; s++) {
            const bool search = s != 0;
            for (int i = 0; i < 3; i++) {
                REFUSED(search, a.d_rec[i] = nullptr);
                REFUSED(search, a.rec_stride[i] = (i ? 960 : 1920) - 1);
            }
            REFUSED(search, a.d_mi = nullptr);
            REFUSED(search, a.d_mi = (const svt_hip_dlf_mi*)((const char*)a.d_mi + 2));
            REFUSED(search, a.mi_stride = 479);
            ACCEPTED(search, a.mi_stride = 512);
            REFUSED(search, a.width = 1924);
            REFUSED(search, a.height = 1084);
            REFUSED(search, a.width = 0);
            REFUSED(search, a.height = 0);
            REFUSED(search, a.width = 65536; a.mi_stride = 16384; for (int i = 0; i < 3; i++) a.rec_stride[i] = a.src_stride[i] = a.dst_stride[i] = 65536);
            REFUSED(search, a.bit_depth = 12);
            REFUSED(search, a.bit_depth = 9);
            REFUSED(search, a.npics = 0);
            REFUSED(search, a.npics = 65536);
            REFUSED(search, a.sharpness_level = 8);
            REFUSED(search, a.sharpness_level = -1);
            ACCEPTED(search, a.sharpness_level = 0);
            for (int i = 0; i < 8; i++) {
                REFUSED(search, a.ref_deltas[i] = 64);
                REFUSED(search, a.ref_deltas[i] = -64);
            }
            for (int i = 0; i < 2; i++) {
                REFUSED(search, a.mode_deltas[i] = 64);
                REFUSED(search, a.mode_deltas[i] = -64);
            }
        }
        // a 10-bit plane at an odd address
        REFUSED(false, a.bit_depth = 10; a.d_rec[1] = (const char*)a.d_rec[1] + 1; a.d_dst[1] = (char*)a.d_dst[1] + 1);
        // the levels are the apply's; the search ignores them
        REFUSED(false, a.filter_level[0] = 64);
        REFUSED(false, a.filter_level[1] = -1);
        REFUSED(false, a.filter_level_u = 64);
        REFUSED(false, a.filter_level_v = 64);
        ACCEPTED(true, a.filter_level[0] = 64; a.filter_level_v = -5);
        ACCEPTED(false, a.filter_level[0] = a.filter_level[1] = a.filter_level_u = a.filter_level_v = 0);
        // the source is the search's, the output the apply's
        for (int i = 0; i < 3; i++) {
            REFUSED(true, a.d_src[i] = nullptr);
            REFUSED(true, a.src_stride[i] = 8);
            ACCEPTED(false, a.d_src[i] = nullptr);
            REFUSED(false, a.d_dst[i] = nullptr);
            ACCEPTED(true, a.d_dst[i] = nullptr);
            REFUSED(false, a.dst_stride[i] = 8);
        }
    }
    {   // in place is all three planes, with the input's stride; two buffers do not overlap the input
        const svt_hip_dlf_pic good = good_pic(false);
        REFUSED(false, a.d_dst[0] = (void*)a.d_rec[0]);
        REFUSED(false, a.d_dst[1] = (void*)a.d_rec[1]; a.d_dst[2] = (void*)a.d_rec[2]);
        REFUSED(false, a.d_dst[0] = (char*)a.d_rec[0] + 64);
        REFUSED(false, a.d_dst[2] = (char*)a.d_rec[0] + 1920 * 1079);
        ACCEPTED(false, a.d_dst[2] = (char*)a.d_rec[0] + 1920 * 1080);
        REFUSED(false, a.npics = 2; a.rec_pitch[0] = 1920 * 1080; a.d_dst[2] = (char*)a.d_rec[0] + 1920 * 1080);
        const svt_hip_dlf_pic same = good_pic(true);
        svt_hip_dlf_pic p = same;
        p.dst_stride[1] = 964;
        CHECK(dlf_check(&p, false) == INVALID);
    }
    {   // the search's own arguments
        const svt_hip_dlf_pic good = good_pic(false);
        const uint64_t mask[3] = {1, 2, 4};
        const size_t need = dlf_search_scratch_bytes(1920, 1080, 1);
        CHECK(need == (size_t)30 * 17 * 3 * 64 * 8);
        CHECK(dlf_search_scratch_bytes(1920, 1080, 3) == 3 * need && dlf_search_scratch_bytes(1924, 1080, 1) == 0 && dlf_search_scratch_bytes(8, 8, 1) == 3 * 64 * 8);
        CHECK(dlf_search_scratch_bytes(0, 8, 1) == 0 && dlf_search_scratch_bytes(8, 8, 0) == 0 && dlf_search_scratch_bytes(65536, 8, 1) == 0);
        void* sse = at(40 << 20); void* scratch = at(41 << 20);
        CHECK(dlf_search_check(&good, mask, sse, scratch, need) == SVT_HIP_OK);
        CHECK(dlf_search_check(&good, nullptr, sse, scratch, need) == INVALID);
        CHECK(dlf_search_check(&good, mask, nullptr, scratch, need) == INVALID);
        CHECK(dlf_search_check(&good, mask, (char*)sse + 4, scratch, need) == INVALID);
        CHECK(dlf_search_check(&good, mask, sse, nullptr, need) == INVALID);
        CHECK(dlf_search_check(&good, mask, sse, (char*)scratch + 4, need) == INVALID);
        CHECK(dlf_search_check(&good, mask, sse, scratch, need - 1) == INVALID);
    }
    {   // the scatter
        svt_hip_dlf_mi_args g{};
        g.d_final = (const svt_hip_part_final*)at(0); g.d_final_count = (const uint32_t*)at(1 << 20); g.d_info = (const svt_hip_dlf_info*)at(2 << 20);
        g.d_mi = (svt_hip_dlf_mi*)at(3 << 20); g.npics = 2; g.nsb = 510; g.sb_pitch = 0; g.nsrc = 1000; g.mi_cols = 480; g.mi_rows = 270; g.mi_stride = 480;
        CHECK(dlf_mi_check(&g) == SVT_HIP_OK && dlf_mi_check(nullptr) == INVALID);
        CHECK(dlf_mi_sb_pitch(&g) == 510 && dlf_mi_grid(1020) == 255 && dlf_mi_grid(1021) == 256);
#define MI_REFUSED(...) do { svt_hip_dlf_mi_args a = g; __VA_ARGS__; CHECK(dlf_mi_check(&a) == INVALID); } while (0)
#define MI_ACCEPTED(...) do { svt_hip_dlf_mi_args a = g; __VA_ARGS__; CHECK(dlf_mi_check(&a) == SVT_HIP_OK); } while (0)
        MI_REFUSED(a.d_final = nullptr); MI_REFUSED(a.d_final_count = nullptr); MI_REFUSED(a.d_info = nullptr); MI_REFUSED(a.d_mi = nullptr);
        MI_REFUSED(a.d_mi = (svt_hip_dlf_mi*)((char*)a.d_mi + 2));
        MI_REFUSED(a.npics = 0); MI_REFUSED(a.nsb = 0); MI_REFUSED(a.nsrc = 0);
        MI_REFUSED(a.sb_pitch = 509); MI_ACCEPTED(a.sb_pitch = 510); MI_ACCEPTED(a.sb_pitch = 600);
        MI_REFUSED(a.npics = 2057);            // 2057 * 510 > 2^20
        MI_ACCEPTED(a.npics = 2056);
        MI_REFUSED(a.mi_cols = 0); MI_REFUSED(a.mi_rows = 0); MI_REFUSED(a.mi_stride = 479);
        MI_REFUSED(a.mi_rows = 16385); MI_ACCEPTED(a.mi_rows = 16384);
    }
    return 0;
}

// closed forms, written out again
static int test_tables() {
    for (int sharp = 0; sharp < 8; sharp++)
        for (int level = 0; level < 64; level++) {
            int shift = sharp > 4 ? 2 : (sharp > 0 ? 1 : 0);
            int lim = level >> shift;
            if (sharp > 0 && lim > 9 - sharp) lim = 9 - sharp;
            if (lim < 1) lim = 1;
            CHECK(dlf_lim(level, sharp) == lim && dlf_mblim(level, sharp) == 2 * level + 4 + lim && dlf_hev(level) == level / 16);
            CHECK(dlf_mblim(level, sharp) <= 255);
        }
    const int lut[25] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 0, 1, 1, 1, 1, 1, 1, 1, 0, 1};
    for (int m = -3; m < 300; m++) CHECK(dlf_mode_lf(m) == (m >= 0 && m < 25 ? lut[m] : 0));
    for (int base = 0; base < 64; base++)
        for (int rd = -63; rd <= 63; rd += 7)
            for (int md = -63; md <= 63; md += 9) {
                const int scale = base >= 32 ? 2 : 1;
                int v = base + (rd + md) * scale;
                v = v < 0 ? 0 : (v > 63 ? 63 : v);
                CHECK(dlf_level(base, true, rd, md) == v && dlf_level(base, false, rd, md) == base);
            }
    // sides: the luma transform's own, the chroma block's halved, 4 at least, 32 at most
    for (int t = 0; t < 19; t++) CHECK(dlf_tx_side(0, 0, 0, t) == kTxW[t] && dlf_tx_side(0, 1, 0, t) == kTxH[t]);
    for (int b = 0; b < 22; b++)
        for (int d = 0; d < 2; d++) {
            const int s = d ? kBsizeH[b] : kBsizeW[b], half = s / 2 < 4 ? 4 : s / 2;
            CHECK(dlf_pu_side(0, d, b) == s && dlf_pu_side(1, d, b) == half && dlf_tx_side(1, d, b, 0) == (half > 32 ? 32 : half));
        }
    for (int plane = 0; plane < 2; plane++)
        for (int s = 4; s <= 64; s *= 2) CHECK(dlf_length(plane, s) == (s == 4 ? 4 : (plane ? 6 : (s == 8 ? 8 : 14))));
    CHECK(dlf_tiles_x(64) == 1 && dlf_tiles_x(72) == 2 && dlf_tiles_y(1080) == 17);
    return 0;
}

// the walk on synthetic tables: a bowl has its minimum found by the halving search; asking level by level converges to the same answer
static int test_pick() {
    for (int centre = 0; centre < 64; centre += 3)
        for (int start = 0; start < 64; start += 5)
            for (int mode = 1; mode <= 3; mode += 2)
                for (int only4 = 0; only4 < 2; only4++) {
                    int64_t full[64], lazy[64];
                    for (int l = 0; l < 64; l++) { full[l] = 1000000 + (int64_t)(l - centre) * (l - centre) * 4000; lazy[l] = -1; }
                    int want = -1, need = -1, got = -1, rounds = 0;
                    CHECK(dlf_pick_level(full, start, mode, only4 != 0, &want, &need) == SVT_HIP_OK && want >= 0 && want < 64);
                    for (;;) {
                        const int rc = dlf_pick_level(lazy, start, mode, only4 != 0, &got, &need);
                        if (rc == SVT_HIP_OK) break;
                        CHECK(rc == SVT_HIP_DLF_NEED_LEVEL && need >= 0 && need < 64 && lazy[need] < 0 && ++rounds <= 64);
                        lazy[need] = full[need];
                    }
                    CHECK(got == want);
                    if (mode <= 2) CHECK(abs(want - start) <= 2 && rounds <= 3);
                }
    int level = 0;
    CHECK(dlf_pick_level(nullptr, 0, 1, false, &level, nullptr) == INVALID);
    int64_t none[64];
    for (int l = 0; l < 64; l++) none[l] = -1;
    CHECK(dlf_pick_level(none, 99, 3, false, &level, nullptr) == SVT_HIP_DLF_NEED_LEVEL);      // need may be NULL; the start is clamped to 63
    int lv[4];
    dlf_level_from_q(4, 8, true, lv);
    CHECK(lv[0] == 0 && lv[1] == 0 && lv[2] == 0 && lv[3] == 0);                               // a negative guess clamps to 0
    dlf_level_from_q(1828, 8, false, lv);
    CHECK(lv[0] == ((1828 * 6017 + 650707 + (1 << 17)) >> 18) - 2 && lv[2] == lv[0] / 2);
    return 0;
}

int main() {
    TRY(test_check());
    TRY(test_tables());
    TRY(test_pick());
    printf("ok\n");
    return 0;
}

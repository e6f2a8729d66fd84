// csrc/me_subpel_plan.h on the CPU: every clause of the sub-pel calls' checks (valid arguments are accepted, the same arguments with one
// field changed are refused, the neighbour of each bound accepted), the padding rule derived from what the refinement reads, the LDS
// bound and the grid.  "Device" pointers are addresses inside a host array that nothing dereferences.  Plain C++17 (g++), linked with
// csrc/host_err.cpp, built plain and under -fsanitize=address,undefined by tests/test_me_subpel_plan_host.py and run directly.  Exit status
// 0 and "ok" when every case holds.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <functional>

#include "../../cidana-svt-av1_amd/csrc/me_subpel_plan.h"

using namespace svthost;

#define CHECK(c) do { if (!(c)) { fprintf(stderr, "%s:%d: %s (last error: %s)\n", __FILE__, __LINE__, #c, svt_hip_last_error()); return 1; } } while (0)
#define TRY(call) do { if (call) { fprintf(stderr, "  from %s:%d\n", __FILE__, __LINE__); return 1; } } while (0)
static const int INVALID = SVT_HIP_ERR_INVALID;

alignas(64) static char g_dev[1 << 16];
static size_t g_dev_next = 0;
template <typename T>
static T* dev() { return (T*)(g_dev + 64 * ++g_dev_next); }
template <typename T>
static T* off(T* p, int bytes) { return (T*)((char*)p + bytes); }

struct Args {
    svt_hip_me_pyramid src, ref0, ref1;
    const svt_hip_me_pyramid *psrc, *pref0, *pref1;
    svt_hip_me_frame_params P;
    svt_hip_me_subpel_params S;
    const svt_hip_me_subpel_params* pS;
    uint32_t n_pictures;
    uint32_t *sad, *mv, *ssd;
    uint8_t* dir;
};
static const int W = 1920, H = 1080 + 8, PAD = 68;

static svt_hip_me_pyramid good_pyramid() {
    svt_hip_me_pyramid p{};
    p.d_plane[0] = dev<uint8_t>();
    p.stride[0] = W + 2 * PAD; p.origin_x[0] = PAD; p.origin_y[0] = PAD;
    p.pitch[0] = (uint64_t)p.stride[0] * (H + 2 * PAD);
    return p;
}
static Args good_args() {
    Args a{};
    a.src = good_pyramid(); a.ref0 = good_pyramid(); a.ref1 = good_pyramid();
    a.P.picture_width = W; a.P.picture_height = H; a.P.slice_type = SVT_HIP_SLICE_B; a.P.max_number_of_pus_per_sb = SVT_HIP_ME_PUS_ALL;
    a.P.fractional_search_method = 1; a.P.cu8x8_mode = 0;
    a.S = svt_hip_me_subpel_params{1, 1, 1, 1, 1};
    a.n_pictures = 3;
    a.sad = dev<uint32_t>(); a.mv = dev<uint32_t>(); a.ssd = dev<uint32_t>(); a.dir = dev<uint8_t>();
    return a;
}
static int run(Args a) {       // (by value: the pointers are set from the copy's own members)
    a.psrc = a.psrc == (const svt_hip_me_pyramid*)1 ? nullptr : &a.src;
    a.pref0 = a.pref0 == (const svt_hip_me_pyramid*)1 ? nullptr : &a.ref0;
    a.pref1 = a.pref1 == (const svt_hip_me_pyramid*)1 ? nullptr : &a.ref1;
    a.pS = a.pS == (const svt_hip_me_subpel_params*)1 ? nullptr : &a.S;
    return me_subpel_check(a.psrc, a.pref0, a.pref1, &a.P, a.pS, a.n_pictures, a.sad, a.mv, a.ssd, a.dir);
}
using Change = std::function<void(Args&)>;
static int verdict(const Args& good, const Change& change, int want, int line) {
    Args a = good;
    change(a);
    const int rc = run(a);
    if (rc != want) { fprintf(stderr, "line %d: %s: %s\n", line, want == INVALID ? "changed arguments were accepted" : "refused", svt_hip_last_error()); return 1; }
    return 0;
}
#define REFUSED(...) TRY(verdict(good, [&](Args& a) { (void)a; __VA_ARGS__; }, INVALID, __LINE__))
#define ACCEPTED(...) TRY(verdict(good, [&](Args& a) { (void)a; __VA_ARGS__; }, SVT_HIP_OK, __LINE__))
#define ABSENT(p) a.p = (decltype(a.p))1

static int test_check() {
    const Args good = good_args();
    CHECK(run(good) == SVT_HIP_OK);
    CHECK(me_subpel_check(nullptr, nullptr, nullptr, nullptr, nullptr, 1, nullptr, nullptr, nullptr, nullptr) == INVALID);
    // the frame parameters the stage reads
    REFUSED(a.P.picture_width = 0); REFUSED(a.P.picture_width = 1916); REFUSED(a.P.picture_height = 1084); REFUSED(a.P.picture_width = 16392); REFUSED(a.P.picture_height = 16392);
    ACCEPTED(a.P.picture_width = 8); ACCEPTED(a.P.picture_height = 8);
    REFUSED(a.P.slice_type = 2); REFUSED(a.P.slice_type = -1);
    REFUSED(a.P.max_number_of_pus_per_sb = 84); REFUSED(a.P.max_number_of_pus_per_sb = 208); ACCEPTED(a.P.max_number_of_pus_per_sb = SVT_HIP_ME_PUS);
    REFUSED(a.P.fractional_search_method = -1); REFUSED(a.P.fractional_search_method = 3);
    ACCEPTED(a.P.fractional_search_method = 0); ACCEPTED(a.P.fractional_search_method = 2);
    REFUSED(a.P.cu8x8_mode = -1); ACCEPTED(a.P.cu8x8_mode = 1);
    ACCEPTED(a.P.search_area_width = 4096; a.P.search_area_height = 4096);      // no search window is too large for the stage: it keeps no window
    // the enables
    REFUSED(a.S.fractional_search64x64 = 2); REFUSED(a.S.enable_half_pel32x32 = -1); REFUSED(a.S.enable_half_pel16x16 = 2); REFUSED(a.S.enable_half_pel8x8 = 2);
    REFUSED(a.S.enable_quarter_pel = 256);
    ACCEPTED(a.S = svt_hip_me_subpel_params{0, 0, 0, 0, 0}); ACCEPTED(ABSENT(pS));
    // the stack
    REFUSED(a.n_pictures = 65536); ACCEPTED(a.n_pictures = 65535); ACCEPTED(a.n_pictures = 1); ACCEPTED(a.n_pictures = 0);
    // the pictures: pointers
    REFUSED(ABSENT(psrc)); REFUSED(ABSENT(pref0)); REFUSED(ABSENT(pref1));
    REFUSED(a.src.d_plane[0] = nullptr); REFUSED(a.ref0.d_plane[0] = nullptr); REFUSED(a.ref1.d_plane[0] = nullptr);
    ACCEPTED(a.src.d_plane[1] = a.src.d_plane[2] = nullptr);                 // level 0 only
    REFUSED(a.P.slice_type = SVT_HIP_SLICE_P); ACCEPTED(a.P.slice_type = SVT_HIP_SLICE_P; ABSENT(pref1));
    // the padding rule: 66 samples on every side of a reference, the search's 64 on the source
    for (svt_hip_me_pyramid Args::*pp : {&Args::ref0, &Args::ref1}) {
        REFUSED((a.*pp).origin_x[0] = 65); REFUSED((a.*pp).origin_y[0] = 65); REFUSED((a.*pp).origin_x[0] = 64); REFUSED((a.*pp).origin_x[0] = 32768);
        ACCEPTED((a.*pp).origin_x[0] = 66; (a.*pp).origin_y[0] = 66);
        REFUSED((a.*pp).stride[0] = PAD + W + 65); ACCEPTED((a.*pp).stride[0] = PAD + W + 66); REFUSED((a.*pp).stride[0] = (1u << 20) + 1);
        REFUSED((a.*pp).pitch[0] = (uint64_t)(W + 2 * PAD) * (PAD + H + 66) - 1); ACCEPTED((a.*pp).pitch[0] = (uint64_t)(W + 2 * PAD) * (PAD + H + 66));
        ACCEPTED((a.*pp).pitch[0] = 0; a.n_pictures = 1);
    }
    REFUSED(a.src.stride[0] = PAD + W + 63); ACCEPTED(a.src.stride[0] = PAD + W + 64);
    REFUSED(a.src.pitch[0] = (uint64_t)(W + 2 * PAD) * (PAD + H + 64) - 1); ACCEPTED(a.src.pitch[0] = (uint64_t)(W + 2 * PAD) * (PAD + H + 64));
    // the rows
    REFUSED(a.sad = nullptr); REFUSED(a.mv = nullptr); ACCEPTED(a.ssd = nullptr); ACCEPTED(a.dir = nullptr);
    REFUSED(a.sad = off(a.sad, 2)); REFUSED(a.mv = off(a.mv, 1)); REFUSED(a.ssd = off(a.ssd, 2)); ACCEPTED(a.dir = off(a.dir, 1));
    ACCEPTED(a.sad = off(a.sad, 4)); ACCEPTED(a.ssd = off(a.ssd, 4));
    return 0;
}

static int test_padding_lds_and_grid() {
    // the margin from the code: a search area starts at most 63 samples before the picture and its last point is the picture's last sample;
    // a PU's block is at most 64 long; the window adds ME_FILTER_TAP / 2 before and 3 after it
    CHECK(ME_SP_FILTER_TAP == 4 && ME_SP_AREA_PAD == 63 && ME_SP_BEFORE == 2 && ME_SP_AFTER == 3);
    CHECK(ME_SP_FIRST == -65 && ME_SP_LAST_PAST_SIDE == 65 && ME_SP_MARGIN == 66);
    for (int side : {8, 136, 1920, 16384}) {
        const int first_block = -ME_SP_AREA_PAD, last_block = side - 1;          // top-left sample of a block at its full-pel winner
        CHECK(first_block - ME_SP_BEFORE >= -ME_SP_MARGIN && last_block + 64 - 1 + ME_SP_AFTER <= side + ME_SP_MARGIN - 1);
        CHECK(last_block + 64 - 1 + ME_SP_AFTER == side + ME_SP_MARGIN - 1);        // the bound is met: one sample less of padding would be read past
    }
    CHECK(ME_SP_MARGIN <= 68);                                                       // the encoder's padding (sb size + ME_FILTER_TAP) passes
    // LDS: a wave's window holds a 64x64 block with its surround, plane B next to it; four waves, and the bi-prediction's blocks
    CHECK(ME_SP_WIN == 69 && ME_SP_IW >= ME_SP_WIN && ME_SP_IW % 4 == 0 && ME_SP_BW >= 66 && ME_SP_BW % 4 == 0);
    CHECK(ME_SP_WAVE_LDS >= ME_SP_WIN * (ME_SP_IW + ME_SP_BW) && ME_SP_WAVE_LDS % 16 == 0);
    CHECK(ME_SP_REFINE_LDS == 4 * ME_SP_WAVE_LDS && ME_SP_REFINE_LDS <= 64 * 1024);
    CHECK(ME_SP_BIPRED_LDS == 4 * (ME_SP_WAVE_LDS + 4096) && ME_SP_BIPRED_LDS + ME_SP_BIPRED_TABLES <= 64 * 1024);
    // the grid
    svt_hip_me_frame_params P{};
    uint32_t g[3];
    P.picture_width = 136; P.picture_height = 72; P.slice_type = SVT_HIP_SLICE_B;
    CHECK(me_subpel_grid(&P, 2, g) == SVT_HIP_OK && g[0] == 6 && g[1] == 2 && g[2] == 2);
    P.slice_type = SVT_HIP_SLICE_P; P.picture_width = 16384; P.picture_height = 16384;
    CHECK(me_subpel_grid(&P, 1, g) == SVT_HIP_OK && g[0] == 256 * 256 && g[1] == 1 && g[2] == 1);
    return 0;
}

static int test_planes_check() {
    const svt_hip_me_pyramid ref = good_pyramid();
    uint8_t* out = dev<uint8_t>();
    CHECK(me_subpel_planes_check(&ref, W, H, 0, 0, 64, 64, out) == SVT_HIP_OK);
    CHECK(me_subpel_planes_check(&ref, W, H, -64, -64, W + 129, 8, out) == SVT_HIP_OK);     // J at (y, x) reads I[y - 2 .. y + 1][x - 2 .. x + 1]
    CHECK(me_subpel_planes_check(&ref, W, H, -64, -64, W + 130, 8, out) == INVALID);
    CHECK(me_subpel_planes_check(&ref, W, H, -65, 0, 8, 8, out) == INVALID && me_subpel_planes_check(&ref, W, H, 0, -65, 8, 8, out) == INVALID);
    CHECK(me_subpel_planes_check(&ref, W, H, 0, H + 57, 8, 8, out) == SVT_HIP_OK && me_subpel_planes_check(&ref, W, H, 0, H + 58, 8, 8, out) == INVALID);
    CHECK(me_subpel_planes_check(nullptr, W, H, 0, 0, 8, 8, out) == INVALID && me_subpel_planes_check(&ref, W, H, 0, 0, 8, 8, nullptr) == INVALID);
    CHECK(me_subpel_planes_check(&ref, W, H, 0, 0, 0, 8, out) == INVALID && me_subpel_planes_check(&ref, W, H, 0, 0, 8, 4097, out) == INVALID);
    CHECK(me_subpel_planes_check(&ref, 4, H, 0, 0, 8, 8, out) == INVALID);
    svt_hip_me_pyramid thin = ref;
    thin.origin_x[0] = 64;
    CHECK(me_subpel_planes_check(&thin, W, H, 0, 0, 8, 8, out) == INVALID);
    return 0;
}

int main() {
    if (test_check() || test_padding_lds_and_grid() || test_planes_check()) return 1;
    printf("ok\n");
    return 0;
}

// csrc/search_plan.h on the CPU: the invariants of every plan a sweep of shapes accepts (the last byte a kernel can touch lies inside the
// LDS the plan asks for, computed from the layout functions the kernels call), the two refusals that 32-bit arithmetic missed, and the
// kernel, variant, grid, threads and LDS bytes of every shape the GPU tests and tools/bench_kernels.py run, as the routing had them before
// it moved into the plan (256 compute units).  Plain C++17 (g++), linked with csrc/host_err.cpp, built plain and under
// -fsanitize=address,undefined by tests/test_search_plan_host.py and run directly.  Exit status 0 and "ok" when every case holds.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "../../cidana-svt-av1_amd/csrc/search_plan.h"

using namespace svthost;

#define CHECK(c) do { if (!(c)) { fprintf(stderr, "%s:%d: %s (last error: %s)\n", __FILE__, __LINE__, #c, svt_hip_last_error()); return 1; } } while (0)
#define TRY(call) do { if (call) { fprintf(stderr, "  from %s:%d\n", __FILE__, __LINE__); return 1; } } while (0)
static const int INVALID = SVT_HIP_ERR_INVALID;
static const int NUM_CU = 256;

enum Knob { KNOB_NONE, KNOB_NO_QSAD, KNOB_NO_Q2, KNOB_NO_Q2P, KNOB_NO_Q16, KNOB_Q2_SU4, KNOBS };
static SadSearchKnobs knobs(int k) { return SadSearchKnobs{k == KNOB_NO_QSAD, k == KNOB_NO_Q2, k == KNOB_NO_Q2P, k == KNOB_NO_Q16, k == KNOB_Q2_SU4}; }

struct Shape { uint32_t w, h; int sw, sh; bool plain; size_t n; int knob; };

// One past the last byte of the dynamic LDS that the kernel of plan p can touch for this shape: the last block slot of a workgroup, the last
// window row, the staging's last chunk and the search's last sliding read, each from the kernel's own indexing (kernel_pixel.h).
static uint64_t lds_extent(const Shape& s, const SadSearchPlan& p) {
    const uint32_t win_w = s.w + (uint32_t)s.sw - 1, cpr = sad_cpr(win_w);
    const uint64_t last_row = p.nrows - 1;
    const uint32_t gx = ((uint32_t)s.sw + 3) >> 2;                    // groups of four candidates per search row
    switch (p.kernel) {
    case SAD_K_PLAIN: {
        // wave `slot` owns [slot * (src + ref), ..): the source at spitch, then window rows at wpitch; candidate xs reads dwords (xs >> 2) .. + spitch / 4
        const uint32_t wpitch = sad_plain_wpitch(win_w), spitch = sad_plain_spitch(s.w);
        const uint64_t stage = wpitch * (last_row + 1), read = last_row * wpitch + 4 * (((uint32_t)s.sw - 1) >> 2) + spitch + 4;
        return (uint64_t)(p.slots - 1) * (p.src_bytes + p.ref_bytes) + p.src_bytes + (stage > read ? stage : read);
    }
    case SAD_K_Q: {
        // block slot: the dense source, then window rows at wpitch; staging writes whole 16-byte chunks, group xg reads dwords xg .. xg + width / 4
        const uint32_t wpitch = sad_q_wpitch(win_w);
        const uint64_t stage = last_row * wpitch + 16 * cpr, read = last_row * wpitch + 4 * (gx - 1) + s.w + 4;
        return (uint64_t)(p.slots - 1) * (p.src_bytes + p.ref_bytes) + p.src_bytes + (stage > read ? stage : read);
    }
    case SAD_K_Q2: {
        // all source blocks first, then the windows ref_bytes apart; a row pair reads window rows ysA .. ysA + CH, the last of them row nrows - 1
        const uint32_t wpitch = sad_q_wpitch(win_w);
        const uint64_t stage = last_row * wpitch + 16 * cpr, read = last_row * wpitch + 4 * (gx - 1) + s.w + 4;
        return (uint64_t)p.slots * sad_q_src_bytes(s.w, s.h) + (uint64_t)(p.slots - 1) * p.ref_bytes + (stage > read ? stage : read);
    }
    case SAD_K_Q2P: {
        // a wave owns 64 / lpb blocks: their sources, then their windows wstride apart, every second pair of blocks 8 bytes further on
        const uint32_t bpw = 64 / p.lpb, waves = p.threads / 64, src = sad_q2p_src_bytes(s.w, s.h);
        const uint64_t stage = last_row * p.wpitch + 16 * cpr, read = last_row * p.wpitch + 4 * (gx - 1) + s.w + 4;
        uint64_t worst = 0;
        for (uint32_t wslot = 0; wslot < bpw; wslot++) {
            const uint64_t e = (uint64_t)bpw * src + (uint64_t)wslot * p.wstride + 8u * ((wslot >> 1) & 1u) + (stage > read ? stage : read);
            if (e > worst) worst = e;
        }
        return (uint64_t)(waves - 1) * bpw * (src + p.wstride) + worst;
    }
    default: {
        // block slot: the dense source, then window rows at wpitch; a task reads width / 16 + 1 aligned 16-byte chunks from column 16 * task
        const uint32_t xqn = ((uint32_t)s.sw + 15) >> 4, src = sad_q16_src_bytes(s.w, s.h);
        const uint64_t stage = last_row * p.wpitch + 16 * cpr, read = last_row * p.wpitch + 16 * (xqn - 1) + s.w + 16;
        return (uint64_t)(p.slots - 1) * (src + p.ref_bytes) + src + (stage > read ? stage : read);
    }
    }
}

static int fail(const Shape& s, const SadSearchPlan& p, const char* what) {
    fprintf(stderr, "block %ux%u, area %dx%d, plain %d, %zu blocks, knob %d -> kernel %d <%d, %d, %d>, grid %u x %u threads, %zu B: %s\n", s.w, s.h, s.sw, s.sh,
            (int)s.plain, s.n, s.knob, p.kernel, p.cw, p.ch, p.su, p.grid, p.threads, p.lds, what);
    return 1;
}
#define HOLDS(c) do { if (!(c)) return fail(s, p, #c); } while (0)

static int check_plan(const Shape& s, const SadSearchPlan& p) {
    HOLDS(p.lds <= SAD_LDS_MAX);
    HOLDS((uint64_t)p.slots * p.per_blk <= p.lds);
    HOLDS(lds_extent(s, p) <= p.lds);
    HOLDS(p.slots >= 1 && (uint64_t)p.slots * 8 <= p.lds);           // the results of a workgroup's blocks leave through the start of the LDS
    HOLDS(p.lpb >= 1 && p.lpb <= 64 && (p.lpb & (p.lpb - 1)) == 0);
    HOLDS(p.threads >= 1 && p.threads <= 256 && p.threads % p.lpb == 0);
    HOLDS(p.nrows == sad_nrows<uint64_t>(s.plain, (uint64_t)s.sh, (uint64_t)s.h));
    HOLDS(p.cpr_magic == sad_cpr_magic(sad_cpr(s.w + (uint32_t)s.sw - 1)));
    if (p.kernel == SAD_K_Q2P) {
        const uint32_t bpw = 64 / p.lpb, waves = p.threads / 64;
        const uint64_t nsets = (s.n + bpw - 1) / bpw;
        HOLDS(p.threads % 64 == 0 && p.slots == waves * bpw);
        // persistent: a wave strides over the sets of 64 / lpb blocks, so any grid covers them; no workgroup without a set, and either every set
        // at once or as many whole workgroups as the device holds (by waves: 16 per CU at 4 per SIMD; by LDS: 160 KiB per CU)
        const uint64_t need = (nsets + waves - 1) / waves, per_cu = p.grid / NUM_CU;
        HOLDS(p.grid >= 1 && p.grid <= need);
        HOLDS(p.grid == need || (p.grid % NUM_CU == 0 && per_cu * waves <= 16 && (per_cu == 1 || per_cu * p.lds <= 160 * 1024)));
        // what the kernel's eight 16-byte registers per lane must hold
        HOLDS(s.w * s.h / (s.w % 16 == 0 ? 16u : 8u) + (uint64_t)sad_cpr(s.w + (uint32_t)s.sw - 1) * p.nrows <= 8 * p.lpb);
        HOLDS(s.sw <= 256 && s.sh <= 256 && s.plain);                 // its 8-bit candidate coordinates
        HOLDS(p.wstride % 128 == 64 && p.wpitch == sad_q2p_wpitch(s.w + (uint32_t)s.sw - 1));
    } else {
        HOLDS(p.slots == p.threads / p.lpb);
        HOLDS((uint64_t)p.grid * p.slots >= s.n && (uint64_t)(p.grid - 1) * p.slots < s.n);
    }
    if (p.kernel == SAD_K_Q2) HOLDS(p.ref_bytes % 32 == 8 && (p.su == 4 || p.su == 8) && s.plain);
    if (p.kernel == SAD_K_Q16) HOLDS(((p.wpitch >> 4) & 1) == 1 && p.wpitch % 16 == 0 && (1u << p.tsh) <= p.lpb && s.plain && s.h % (256 / s.w) == 0);
    if (p.kernel == SAD_K_Q2 || p.kernel == SAD_K_Q2P) HOLDS(p.cw == (int)s.w && p.ch == (int)s.h && s.w * s.h <= 256);
    if (p.kernel == SAD_K_Q16) HOLDS(p.cw == (int)s.w);
    if (p.kernel == SAD_K_Q) HOLDS(s.w % 4 == 0 && (p.cw == 0 ? p.ch == 0 : p.cw == (int)s.w && p.ch == (int)s.h));
    return 0;
}

static int test_sweep() {
    static const uint32_t sides[] = {4, 8, 12, 16, 24, 32, 48, 64, 63};      // 63: no multiple of 4, the one-wave-per-block kernel
    static const size_t counts[] = {1, 7, 8, 9, 333, (size_t)1 << 20};
    int areas_w[82], areas_h[42];
    for (int i = 0; i < 80; i++) areas_w[i] = i + 1;
    for (int i = 0; i < 40; i++) areas_h[i] = i + 1;
    areas_w[80] = areas_h[40] = 256; areas_w[81] = areas_h[41] = 257;
    size_t accepted = 0, refused = 0;
    bool seen[5] = {};
    for (uint32_t w : sides) for (uint32_t h : sides) for (int sw : areas_w) for (int sh : areas_h) for (int plain = 0; plain < 2; plain++)
        for (int knob = 0; knob < KNOBS; knob++) for (size_t n : counts) {
            const Shape s{w, h, sw, sh, plain != 0, n, knob};
            SadSearchPlan p;
            const int rc = sad_search_plan(w, h, sw, sh, s.plain, n, knobs(knob), NUM_CU, p);
            if (rc != SVT_HIP_OK) { CHECK(rc == INVALID); refused++; continue; }
            accepted++;
            seen[p.kernel] = true;
            TRY(check_plan(s, p));
            if (w == 63) CHECK(p.kernel == SAD_K_PLAIN);
        }
    CHECK(accepted > 1000000 && refused > 1000);
    for (bool b : seen) CHECK(b);
    return 0;
}

static int test_refusals() {
    SadSearchPlan p;
    const SadSearchKnobs none = knobs(KNOB_NONE);
    // search_h * height = 2^20 rows at a pitch of 4096 bytes: 2^32 bytes, which 32-bit arithmetic took for 0 and passed
    CHECK(sad_q_wpitch(64 + 4017 - 1) == 4096 && sad_nrows<uint64_t>(false, 16384, 64) == (1u << 20));
    CHECK(sad_search_plan(64, 64, 4017, 16384, false, 1, none, NUM_CU, p) == INVALID);
    CHECK(sad_plain_wpitch(63 + 4023 - 1) == 4096);
    CHECK(sad_search_plan(63, 64, 4023, 16384, false, 1, none, NUM_CU, p) == INVALID);
    CHECK(sad_search_plan(64, 64, 4017, 16384, true, 1, none, NUM_CU, p) == INVALID);
    // the other refusals
    CHECK(sad_search_plan(0, 8, 8, 8, true, 1, none, NUM_CU, p) == INVALID && sad_search_plan(8, 65, 8, 8, true, 1, none, NUM_CU, p) == INVALID);
    CHECK(sad_search_plan(8, 8, 0, 8, true, 1, none, NUM_CU, p) == INVALID && sad_search_plan(8, 8, 8, -1, true, 1, none, NUM_CU, p) == INVALID);
    CHECK(sad_search_plan(64, 64, 1, 1, true, 1, none, NUM_CU, p) == SVT_HIP_OK);

    MeWindow w;
    CHECK(me_window(65536, 65536, 0, w) == INVALID);      // 2^32 points: a signed product that wrapped to 0
    CHECK(me_window(4097, 1, 0, w) == INVALID && me_window(1, 4097, 0, w) == INVALID && me_window(0, 1, 0, w) == INVALID && me_window(1, -1, 0, w) == INVALID);
    CHECK(me_window(64, 65, 0, w) == INVALID && me_window(4096, 2, 1, w) == INVALID);
    CHECK(me_window(4096, 1, 0, w) == SVT_HIP_OK && w.wpitch == me_window_pitch(64 + 4096 - 1) && w.lds == ME_SRC_LDS + (size_t)w.wpitch * 64);
    CHECK(me_window_check(4096, 1, 0, ME_LDS_MAX, w) == INVALID);      // ... up to its LDS check
    CHECK(me_window_check(64, 64, 0, ME_LDS_MAX, w) == SVT_HIP_OK && me_window_check(64, 64, 1, ME_NSQ_LDS_MAX, w) == SVT_HIP_OK);
    CHECK(me_window_check(64, 64, 1, w.lds, w) == SVT_HIP_OK && me_window_check(64, 64, 1, w.lds - 1, w) == INVALID);
    // every accepted window: rows of whole 16-byte chunks with a chunk of slack, 64 (mod 128), and the pairs behind the window
    for (int sw = 1; sw <= 4096; sw++)
        for (int sh = 1; sw * sh <= 4096; sh++)
            for (int nsq = 0; nsq < 2; nsq++) {
                CHECK(me_window(sw, sh, nsq, w) == SVT_HIP_OK);
                CHECK(w.wpitch % 128 == 64 && w.wpitch >= ((64u + sw - 1 + 15) & ~15u) + 16);
                const size_t win = ME_SRC_LDS + (size_t)w.wpitch * (64 + sh - 1);
                CHECK(nsq ? (w.pair_off >= win && w.pair_off % 16 == 0 && w.lds == w.pair_off + (size_t)8 * 7 * sh) : (w.pair_off == 0 && w.lds == win));
            }

    svt_hip_hme_params hp[4] = {};
    HmeWindow hw;
    for (auto& q : hp) { q.search_area_width = 16; q.search_area_height = 8; }
    CHECK(hme_window(hp, 4, hw) == SVT_HIP_OK && hw.wpitch == 88 && hw.lds == ME_SRC_LDS + 88 * 70);
    hp[2].search_area_width = 0; CHECK(hme_window(hp, 4, hw) == INVALID && hme_window(hp, 2, hw) == SVT_HIP_OK);
    hp[2].search_area_width = 4097; CHECK(hme_window(hp, 4, hw) == INVALID);
    hp[2].search_area_width = 16; hp[3].search_area_height = -3; CHECK(hme_window(hp, 4, hw) == INVALID);
    hp[3].search_area_height = 0x7fffffff; CHECK(hme_window(hp, 4, hw) == INVALID);
    // the widest region's pitch times the tallest region's rows
    hp[3].search_area_height = 8; hp[0].search_area_width = 64; hp[1].search_area_height = 40;
    CHECK(hme_window(hp, 4, hw) == SVT_HIP_OK && hw.wpitch == hme_window_pitch(127) && hw.wpitch == 136 && hw.lds == ME_SRC_LDS + 136 * 102);
    hp[1].search_area_height = 374; CHECK(hme_window(hp, 4, hw) == SVT_HIP_OK && hw.lds == ME_SRC_LDS + 136 * 436 && hw.lds + 136 > ME_LDS_MAX);
    hp[1].search_area_height = 375; CHECK(hme_window(hp, 4, hw) == INVALID);
    CHECK(hme_window(hp, 0, hw) == SVT_HIP_OK && hw.lds == ME_SRC_LDS);      // no level on: the source rows alone
    return 0;
}

// ---- the launches as they were before the routing moved into the plan --------------------------------------------------------------------
struct SadRow { uint32_t w, h; int sw, sh, plain; size_t n; int knob; int kernel, cw, ch, su; uint32_t grid, threads; size_t lds; };
static const SadRow kSadRows[] = {
    // test_gpu_parity.py::test_sad_search (23 blocks)
    {16, 16,  8,  8, 1,      23, KNOB_NONE,    SAD_K_Q2P,  16, 16, 0,      1, 256, 39424},
    {16, 16,  1,  1, 1,      23, KNOB_NONE,    SAD_K_Q2,   16, 16, 8,      1,  64, 53760},
    { 8,  8, 16,  7, 1,      23, KNOB_NONE,    SAD_K_Q2P,   8,  8, 0,      2, 256, 10496},
    {32, 32, 13,  5, 1,      23, KNOB_NONE,    SAD_K_Q16,  32,  0, 0,      3, 256, 22016},
    {64, 64,  9,  9, 1,      23, KNOB_NONE,    SAD_K_Q16,  64,  0, 0,      6, 256, 39424},
    { 4,  4,  8,  8, 1,      23, KNOB_NONE,    SAD_K_Q,     0,  0, 0,      2, 256,  6144},
    {24, 24,  8,  4, 1,      23, KNOB_NONE,    SAD_K_Q,     0,  0, 0,      1, 256, 60416},
    {48, 48,  5,  3, 1,      23, KNOB_NONE,    SAD_K_Q,     0,  0, 0,      3,  64, 50560},
    {16,  8, 32, 20, 1,      23, KNOB_NONE,    SAD_K_Q,     0,  0, 0,      6, 256,  7488},
    // test_gpu_parity.py::test_sad_search_line_skipping (5 blocks, ref_stride = 2 * ref_stride_raw)
    {16, 16,  8,  4, 0,       5, KNOB_NONE,    SAD_K_Q,    16, 16, 0,      1, 128, 53504},
    {24, 24,  5,  3, 0,       5, KNOB_NONE,    SAD_K_Q,     0,  0, 0,      1, 128, 64768},
    // test_gpu_parity.py::test_sad_search_tail_counts
    { 8,  8,  8,  8, 1,       1, KNOB_NONE,    SAD_K_Q2P,   8,  8, 0,      1, 256, 16896},
    { 8,  8,  8,  8, 1,       3, KNOB_NONE,    SAD_K_Q2P,   8,  8, 0,      1, 256, 16896},
    { 8,  8,  8,  8, 1,     257, KNOB_NONE,    SAD_K_Q2P,   8,  8, 0,      9, 256, 16896},
    {16, 16,  5,  3, 1,       1, KNOB_NONE,    SAD_K_Q2,   16, 16, 8,      1, 128, 40192},
    {16, 16,  5,  3, 1,       3, KNOB_NONE,    SAD_K_Q2,   16, 16, 8,      1, 128, 40192},
    {16, 16,  5,  3, 1,     257, KNOB_NONE,    SAD_K_Q2,   16, 16, 8,      9, 128, 40192},
    {32, 32,  9,  6, 1,       1, KNOB_NONE,    SAD_K_Q16,  32,  0, 0,      1, 256, 22400},
    {32, 32,  9,  6, 1,       3, KNOB_NONE,    SAD_K_Q16,  32,  0, 0,      1, 256, 22400},
    {32, 32,  9,  6, 1,     257, KNOB_NONE,    SAD_K_Q16,  32,  0, 0,     33, 256, 22400},
    {64, 64,  4,  4, 1,       1, KNOB_NONE,    SAD_K_Q16,  64,  0, 0,      1, 256, 37824},
    {64, 64,  4,  4, 1,       3, KNOB_NONE,    SAD_K_Q16,  64,  0, 0,      1, 256, 37824},
    {64, 64,  4,  4, 1,     257, KNOB_NONE,    SAD_K_Q16,  64,  0, 0,     65, 256, 37824},
    // test_gpu_variants.py::test_sad_search_pipelined_vs_one_shot, no_q2p off and on
    {16, 16,  8,  8, 1,       1, KNOB_NONE,    SAD_K_Q2P,  16, 16, 0,      1, 256, 39424},
    {16, 16,  8,  8, 1,       1, KNOB_NO_Q2P,  SAD_K_Q2,   16, 16, 8,      1, 256, 49408},
    {16, 16,  8,  8, 1,       7, KNOB_NONE,    SAD_K_Q2P,  16, 16, 0,      1, 256, 39424},
    {16, 16,  8,  8, 1,       7, KNOB_NO_Q2P,  SAD_K_Q2,   16, 16, 8,      1, 256, 49408},
    {16, 16,  8,  8, 1,       8, KNOB_NONE,    SAD_K_Q2P,  16, 16, 0,      1, 256, 39424},
    {16, 16,  8,  8, 1,       8, KNOB_NO_Q2P,  SAD_K_Q2,   16, 16, 8,      1, 256, 49408},
    {16, 16,  8,  8, 1,       9, KNOB_NONE,    SAD_K_Q2P,  16, 16, 0,      1, 256, 39424},
    {16, 16,  8,  8, 1,       9, KNOB_NO_Q2P,  SAD_K_Q2,   16, 16, 8,      1, 256, 49408},
    {16, 16,  8,  8, 1,    5000, KNOB_NONE,    SAD_K_Q2P,  16, 16, 0,    157, 256, 39424},
    {16, 16,  8,  8, 1,    5000, KNOB_NO_Q2P,  SAD_K_Q2,   16, 16, 8,    157, 256, 49408},
    { 8,  8,  8,  8, 1,    4099, KNOB_NONE,    SAD_K_Q2P,   8,  8, 0,    129, 256, 16896},
    { 8,  8,  8,  8, 1,    4099, KNOB_NO_Q2P,  SAD_K_Q2,    8,  8, 4,    129, 256, 22784},
    {16, 16,  5,  3, 1,     333, KNOB_NONE,    SAD_K_Q2,   16, 16, 8,     11, 128, 40192},
    {16, 16,  5,  3, 1,     333, KNOB_NO_Q2P,  SAD_K_Q2,   16, 16, 8,     11, 128, 40192},
    { 8,  8, 13,  5, 1,     333, KNOB_NONE,    SAD_K_Q2P,   8,  8, 0,     21, 256, 10496},
    { 8,  8, 13,  5, 1,     333, KNOB_NO_Q2P,  SAD_K_Q2,    8,  8, 4,     21, 256, 15488},
    {16, 16, 11,  8, 1,     333, KNOB_NONE,    SAD_K_Q2P,  16, 16, 0,     21, 256, 19712},
    {16, 16, 11,  8, 1,     333, KNOB_NO_Q2P,  SAD_K_Q2,   16, 16, 4,     21, 256, 26752},
    { 8,  8,  4,  2, 1,      77, KNOB_NONE,    SAD_K_Q2,    8,  8, 8,      1, 128, 54272},
    { 8,  8,  4,  2, 1,      77, KNOB_NO_Q2P,  SAD_K_Q2,    8,  8, 8,      1, 128, 54272},
    {16, 16,  1,  1, 1,      77, KNOB_NONE,    SAD_K_Q2,   16, 16, 8,      2,  64, 53760},
    {16, 16,  1,  1, 1,      77, KNOB_NO_Q2P,  SAD_K_Q2,   16, 16, 8,      2,  64, 53760},
    // test_gpu_variants.py::test_sad_search_variants (37 blocks), knob off and on
    {16, 16,  8,  8, 1,      37, KNOB_NONE,    SAD_K_Q2P,  16, 16, 0,      2, 256, 39424},
    {16, 16,  8,  8, 1,      37, KNOB_Q2_SU4,  SAD_K_Q2P,  16, 16, 0,      2, 256, 39424},
    { 8,  8, 16, 16, 1,      37, KNOB_NONE,    SAD_K_Q2P,   8,  8, 0,      5, 256,  8320},
    { 8,  8, 16, 16, 1,      37, KNOB_Q2_SU4,  SAD_K_Q2P,   8,  8, 0,      5, 256,  8320},
    {16, 16,  8,  8, 1,      37, KNOB_NO_Q2,   SAD_K_Q,    16, 16, 0,      3, 256, 22016},
    { 8,  8, 13,  5, 1,      37, KNOB_NONE,    SAD_K_Q2P,   8,  8, 0,      3, 256, 10496},
    { 8,  8, 13,  5, 1,      37, KNOB_NO_Q2,   SAD_K_Q,     8,  8, 0,      5, 256,  5248},
    {16, 16,  8,  8, 1,      37, KNOB_NO_QSAD, SAD_K_PLAIN, 0,  0, 0,     10, 256,  4032},
    {32, 32,  9,  6, 1,      37, KNOB_NONE,    SAD_K_Q16,  32,  0, 0,      5, 256, 22400},
    {32, 32,  9,  6, 1,      37, KNOB_NO_QSAD, SAD_K_PLAIN, 0,  0, 0,     10, 256, 11264},
    {32, 32,  9,  6, 1,      37, KNOB_NO_Q16,  SAD_K_Q,    32, 32, 0,      5, 256, 27264},
    {64, 64, 16, 16, 1,      37, KNOB_NONE,    SAD_K_Q16,  64,  0, 0,     10, 256, 41664},
    {64, 64, 16, 16, 1,      37, KNOB_NO_Q16,  SAD_K_Q,    64, 64, 0,     10, 256, 46784},
    {32, 32, 37,  3, 1,      37, KNOB_NONE,    SAD_K_Q16,  32,  0, 0,     10, 256, 14976},
    {32, 32, 37,  3, 1,      37, KNOB_NO_Q16,  SAD_K_Q,    32, 32, 0,      5, 256, 34432},
    // test_gpu_variants.py::test_sad_search_wide_variants (19 blocks), no_q16 off and on
    {32,  8, 16, 16, 1,      19, KNOB_NONE,    SAD_K_Q16,  32,  0, 0,      2, 256, 21760},
    {32,  8, 16, 16, 1,      19, KNOB_NO_Q16,  SAD_K_Q,     0,  0, 0,      5, 256,  6976},
    {32, 16,  5,  9, 1,      19, KNOB_NONE,    SAD_K_Q16,  32,  0, 0,      3, 256, 13312},
    {32, 16,  5,  9, 1,      19, KNOB_NO_Q16,  SAD_K_Q,     0,  0, 0,      3, 256, 16512},
    {32, 64, 33,  2, 1,      19, KNOB_NONE,    SAD_K_Q16,  32,  0, 0,      5, 256, 28992},
    {32, 64, 33,  2, 1,      19, KNOB_NO_Q16,  SAD_K_Q,     0,  0, 0,      3, 256, 58112},
    {64, 16, 16,  7, 1,      19, KNOB_NONE,    SAD_K_Q16,  64,  0, 0,      3, 256, 22272},
    {64, 16, 16,  7, 1,      19, KNOB_NO_Q16,  SAD_K_Q,     0,  0, 0,      3, 256, 25216},
    {64, 32, 70,  3, 1,      19, KNOB_NONE,    SAD_K_Q16,  64,  0, 0,      5, 256, 27776},
    {64, 32, 70,  3, 1,      19, KNOB_NO_Q16,  SAD_K_Q,     0,  0, 0,      5, 256, 30016},
    {64, 64,  1,  1, 1,      19, KNOB_NONE,    SAD_K_Q16,  64,  0, 0,      5,  64, 36864},
    {64, 64,  1,  1, 1,      19, KNOB_NO_Q16,  SAD_K_Q,    64, 64, 0,      5,   4, 36928},
    {32, 32,  1, 40, 1,      19, KNOB_NONE,    SAD_K_Q16,  32,  0, 0,      5, 256, 17728},
    {32, 32,  1, 40, 1,      19, KNOB_NO_Q16,  SAD_K_Q,    32, 32, 0,      5, 256, 17792},
    {64, 64, 64, 17, 1,      19, KNOB_NONE,    SAD_K_Q16,  64,  0, 0,      5, 256, 62464},
    {64, 64, 64, 17, 1,      19, KNOB_NO_Q16,  SAD_K_Q,    64, 64, 0,      5, 256, 62528},
    {16, 16, 16, 16, 1,      19, KNOB_NONE,    SAD_K_Q16,  16,  0, 0,      2, 256, 27904},
    {16, 16, 16, 16, 1,      19, KNOB_NO_Q16,  SAD_K_Q2P,  16, 16, 0,      3, 256, 12928},
    {16, 16, 32,  3, 1,      19, KNOB_NONE,    SAD_K_Q16,  16,  0, 0,      1, 256, 35840},
    {16, 16, 32,  3, 1,      19, KNOB_NO_Q16,  SAD_K_Q2P,  16, 16, 0,      2, 256, 21760},
    {16, 32,  7,  5, 1,      19, KNOB_NONE,    SAD_K_Q16,  16,  0, 0,      2, 256, 35840},
    {16, 32,  7,  5, 1,      19, KNOB_NO_Q16,  SAD_K_Q,     0,  0, 0,      2, 256, 36096},
    {16, 64, 24,  9, 1,      19, KNOB_NONE,    SAD_K_Q16,  16,  0, 0,      5, 256, 17920},
    {16, 64, 24,  9, 1,      19, KNOB_NO_Q16,  SAD_K_Q,     0,  0, 0,      5, 256, 22592},
    {16, 32, 80,  2, 1,      19, KNOB_NONE,    SAD_K_Q16,  16,  0, 0,      3, 256, 33664},
    {16, 32, 80,  2, 1,      19, KNOB_NO_Q16,  SAD_K_Q,     0,  0, 0,      5, 256, 16896},
    // test_gpu_frame_search.py::test_sad_search_on_planes_matches_oracle (a 256 x 128 picture in blocks)
    {16, 16,  8,  8, 1,     128, KNOB_NONE,    SAD_K_Q2P,  16, 16, 0,      4, 256, 39424},
    { 8,  8, 16,  5, 1,     512, KNOB_NONE,    SAD_K_Q2P,   8,  8, 0,     32, 256, 10496},
    {32, 32, 24,  9, 1,      32, KNOB_NONE,    SAD_K_Q16,  32,  0, 0,      8, 256, 16896},
    {64, 64, 16, 16, 1,       8, KNOB_NONE,    SAD_K_Q16,  64,  0, 0,      2, 256, 41664},
    // test_gpu_fullsize.py and tools/bench_kernels.py
    {16, 16,  8,  8, 1, 1048576, KNOB_NONE,    SAD_K_Q2P,  16, 16, 0,   1024, 256, 39424},
    {32, 32, 16, 16, 1,  131072, KNOB_NONE,    SAD_K_Q16,  32,  0, 0,  32768, 256, 13120},
    {64, 64, 16, 16, 1,   32768, KNOB_NONE,    SAD_K_Q16,  64,  0, 0,   8192, 256, 41664},
    {32, 32, 16, 16, 1,  131072, KNOB_NO_Q16,  SAD_K_Q,    32, 32, 0,  32768, 256, 16192},
    {64, 64, 16, 16, 1,   32768, KNOB_NO_Q16,  SAD_K_Q,    64, 64, 0,   8192, 256, 46784},
    // test_gpu_dropin.py::test_dropin_sad_loop_incl_line_skipping (one block)
    {16, 16, 16,  9, 1,       1, KNOB_NONE,    SAD_K_Q16,  16,  0, 0,      1, 256, 22528},
    {16,  8, 12,  6, 0,       1, KNOB_NONE,    SAD_K_Q,     0,  0, 0,      1, 256, 19584},
    {32, 32,  8,  8, 1,       1, KNOB_NONE,    SAD_K_Q16,  32,  0, 0,      1, 256, 23168},
    {64, 32,  5,  4, 0,       1, KNOB_NONE,    SAD_K_Q,     0,  0, 0,      1,  32, 57408},
};

// (sw, sh) of test_gpu_pins.py::test_me_fullpel_vs_oracle_batches and test_gpu_variants.py::test_me_sb_search_variants, square and all PUs
struct MeRow { int sw, sh, nsq; uint32_t wpitch; size_t lds; uint32_t pair_off; };
static const MeRow kMeRows[] = {
    { 8,  3, 0, 192, 14720,     0}, { 8,  3, 1, 192, 14888, 14720},
    {16,  5, 0, 192, 15104,     0}, {16,  5, 1, 192, 15384, 15104},
    {64, 64, 0, 192, 26432,     0}, {64, 64, 1, 192, 30016, 26432},
    {24,  7, 0, 192, 15488,     0}, {24,  7, 1, 192, 15880, 15488},
    { 7,  9, 0, 192, 15872,     0}, { 7,  9, 1, 192, 16376, 15872},
    {20,  4, 0, 192, 14912,     0}, {20,  4, 1, 192, 15136, 14912},
    {48, 16, 0, 192, 17216,     0}, {48, 16, 1, 192, 18112, 17216},
    { 1,  1, 0, 192, 14336,     0}, { 1,  1, 1, 192, 14392, 14336},
    {40, 33, 0, 192, 20480,     0}, {40, 33, 1, 192, 22328, 20480},
    {13,  7, 0, 192, 15488,     0}, {13,  7, 1, 192, 15880, 15488},
    {37, 21, 0, 192, 18176,     0}, {37, 21, 1, 192, 19352, 18176},
};

// the search areas svt_hip_hme_level_params derives for the launches of tests/test_gpu_hme.py and tools/bench_kernels.py (each set of areas once)
struct HmeRow { int nregions; int area[4][2]; uint32_t wpitch; size_t lds; };
static const HmeRow kHmeRows[] = {
    {1, {{48, 24}, {0, 0}, {0, 0}, {0, 0}}, 120, 12368},      // chained: level 0, region (0, 0); golden: level 0
    {1, {{32, 16}, {0, 0}, {0, 0}, {0, 0}}, 104, 10160},      // chained: level 0, region (1, 1)
    {1, {{16, 8}, {0, 0}, {0, 0}, {0, 0}},  88,  8208},       // chained: levels 1 and 2; the tasks outside the SB size range
    {4, {{32, 16}, {32, 16}, {32, 16}, {32, 16}}, 104, 10160},      // four regions in one launch, level 0
    {4, {{16, 8}, {16, 8}, {16, 8}, {16, 8}},  88,  8208},    // four regions in one launch, levels 1 and 2
    {1, {{48, 20}, {0, 0}, {0, 0}, {0, 0}}, 120, 11888},      // golden (tests/golden/hme.npz), level 0: regions x multipliers 100 / 150 % x 100 / 200 %
    {1, {{48, 40}, {0, 0}, {0, 0}, {0, 0}}, 120, 14288},
    {1, {{64, 20}, {0, 0}, {0, 0}, {0, 0}}, 136, 13200},
    {1, {{64, 40}, {0, 0}, {0, 0}, {0, 0}}, 136, 15920},
    {1, {{48, 12}, {0, 0}, {0, 0}, {0, 0}}, 120, 10928},
    {1, {{64, 12}, {0, 0}, {0, 0}, {0, 0}}, 136, 12112},
    {1, {{64, 24}, {0, 0}, {0, 0}, {0, 0}}, 136, 13744},
    {1, {{32, 20}, {0, 0}, {0, 0}, {0, 0}}, 104, 10576},
    {1, {{32, 40}, {0, 0}, {0, 0}, {0, 0}}, 104, 12656},
    {1, {{32, 12}, {0, 0}, {0, 0}, {0, 0}}, 104,  9744},
    {1, {{32, 24}, {0, 0}, {0, 0}, {0, 0}}, 104, 10992},
    {1, {{40, 20}, {0, 0}, {0, 0}, {0, 0}}, 112, 11232},      // golden, levels 1 and 2: the four regions
    {1, {{40, 12}, {0, 0}, {0, 0}, {0, 0}}, 112, 10336},
    {1, {{24, 20}, {0, 0}, {0, 0}, {0, 0}},  96,  9920},
    {1, {{24, 12}, {0, 0}, {0, 0}, {0, 0}},  96,  9152},
    {1, {{64, 32}, {0, 0}, {0, 0}, {0, 0}}, 136, 14832},      // tools/bench_kernels.py: level 0 of a 960 x 540 picture
};

static int test_pinned_launches() {
    bool kernel[5] = {}, su[9] = {};
    for (const SadRow& r : kSadRows) {
        const Shape s{r.w, r.h, r.sw, r.sh, r.plain != 0, r.n, r.knob};
        SadSearchPlan p;
        CHECK(sad_search_plan(r.w, r.h, r.sw, r.sh, s.plain, r.n, knobs(r.knob), NUM_CU, p) == SVT_HIP_OK);
        if (p.kernel != r.kernel || p.cw != r.cw || p.ch != r.ch || p.su != r.su || p.grid != r.grid || p.threads != r.threads || p.lds != r.lds)
            return fail(s, p, "not the launch of the routing before the plan");
        TRY(check_plan(s, p));
        kernel[r.kernel] = true;
        if (r.kernel == SAD_K_Q2) su[r.su] = true;
    }
    for (bool b : kernel) CHECK(b);                      // each of the five kernels, and both staging depths of q2
    CHECK(su[4] && su[8]);
    for (const MeRow& r : kMeRows) {
        MeWindow w;
        CHECK(me_window_check(r.sw, r.sh, r.nsq, r.nsq ? ME_NSQ_LDS_MAX : ME_LDS_MAX, w) == SVT_HIP_OK);
        CHECK(w.wpitch == r.wpitch && w.lds == r.lds && w.pair_off == r.pair_off);
    }
    for (const HmeRow& r : kHmeRows) {
        svt_hip_hme_params hp[4] = {};
        for (int i = 0; i < r.nregions; i++) { hp[i].search_area_width = r.area[i][0]; hp[i].search_area_height = r.area[i][1]; }
        HmeWindow w;
        CHECK(hme_window(hp, r.nregions, w) == SVT_HIP_OK);
        CHECK(w.wpitch == r.wpitch && w.lds == r.lds);
    }
    return 0;
}

int main() {
    TRY(test_refusals());
    TRY(test_pinned_launches());
    TRY(test_sweep());
    printf("ok\n");
    return 0;
}

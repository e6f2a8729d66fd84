// csrc/intra_plan.h on the CPU: the invariants of every plan a sweep of shapes accepts, each derived from the kernels' own indexing (the
// grid covers the batch and keeps a lane on its row and column, the exact DC division, the staged edges of the directional kernels inside
// their LDS slot and below zone 2's table, the angle split, the level map's row division), every refusal with its status and text, the
// 2^31 - 1 bound of every batch entry point, and the launch of every shape the GPU tests, bench.py's callers and tools/ab_kernels.py reach
// in this family as the entry points computed it before the plan existed (tests/c/intra_plan_pins.h).  Plain C++17 (g++), linked with
// csrc/host_err.cpp, built plain and under -fsanitize=address,undefined by tests/test_intra_plan_host.py and run directly.  Exit status 0
// and "ok" when every case holds.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <initializer_list>

#include "../../cidana-svt-av1_amd/csrc/intra_plan.h"
#include "../../cidana-svt-av1_amd/csrc/search_plan.h"
#include "intra_plan_pins.h"

using namespace svthost;
using namespace svtdev;

#define CHECK(c) do { if (!(c)) { fprintf(stderr, "%s:%d: %s (last error: %s)\n", __FILE__, __LINE__, #c, svt_hip_last_error()); return 1; } } while (0)
#define TRY(call) do { if (call) { fprintf(stderr, "  from %s:%d\n", __FILE__, __LINE__); return 1; } } while (0)
// the call is refused with SVT_HIP_ERR_INVALID and this text
#define REFUSED(call, text) do { CHECK((call) == SVT_HIP_ERR_INVALID); if (strcmp(svt_hip_last_error(), text)) { \
    fprintf(stderr, "%s:%d: \"%s\", expected \"%s\"\n", __FILE__, __LINE__, svt_hip_last_error(), text); return 1; } } while (0)
static const char* TOO_MANY = "too many blocks for one launch";
static const size_t N_MAX = 0x7fffffffu;
static const size_t kCounts[] = {1, 2, 3, 5, 300, 777, N_MAX};
static const size_t kOver[] = {(size_t)1 << 31, ((size_t)1 << 32) + 1};
static const IntraKnobs kKnobs[] = {{0, 4, 256}, {0, 4, 1}, {1, 4, 256}, {0, 1, 256}, {0, 16, 256}, {1, 4, 1}};
static char buf_a[64], buf_b[64], buf_c[64], buf_d[64];          // stand-ins for device buffers: compared and tested for alignment, never followed
static void* const A = buf_a; static void* const B = buf_b; static void* const C = buf_c; static void* const D = buf_d;

static bool pow2(uint32_t v) { return v && !(v & (v - 1)); }
static uint32_t umulhi(uint32_t a, uint32_t b) { return (uint32_t)(((uint64_t)a * b) >> 32); }

// ---- the plain predictors and the directional kernels ----
// the entry point's grid arithmetic before it moved into the plan
static uint64_t parent_grid(uint64_t per_block, uint64_t n, bool dir, bool wide, int iu) {
    uint64_t grid = (per_block * n + 255) / 256;
    if (per_block > 256) grid = (grid + 1) & ~(uint64_t)1;
    if (dir || !wide) return grid;
    const uint64_t gw = (grid + iu - 1) / iu;
    return per_block > 256 ? (gw + 1) & ~(uint64_t)1 : gw;
}

static size_t g_lds_max = 0;
static int g_lds_max_case[5];

static int check_dir_lds(const DirLds& L, int bw, int bh, int es, int ua, int ul, int npx) {
    const uint32_t per_block = intra_lanes(bw, bh, es).per_block;
    CHECK(L.lpb == (per_block >= 256 ? 256u : per_block) && pow2(L.lpb) && L.slots * L.lpb == 256);
    CHECK(L.lim_a == NB_ORIGIN + ((bw + bh - 1) << ua) && L.lim_l == NB_ORIGIN + ((bw + bh - 1) << ul));
    CHECK(L.estride % 8 == 0 && L.slot_stride % 2 == 0 && L.slot_stride >= 2 * L.estride);
    if (L.lpb < 32) CHECK((uint32_t)L.slot_stride % 32 == L.lpb % 32);
    // staging (intra_dir_body): groups of four pair dwords from array position NB_ORIGIN - 2 up to n_pad, above edge at the slot's start,
    // left edge estride behind it
    const int ng = (L.n_pad - (NB_ORIGIN - 2) + 3) >> 2;
    const int last_staged = NB_ORIGIN - 2 + 4 * (ng - 1) + 3;
    CHECK(last_staged >= L.n_pad - 1 && last_staged < L.estride);
    CHECK(L.estride + last_staged < L.slot_stride);
    CHECK((size_t)(L.slots - 1) * L.slot_stride + L.estride + last_staged < L.tab_dword);
    CHECK(L.tab_dword == (size_t)L.slots * L.slot_stride && L.bytes == (L.tab_dword + 128) * 4 && L.tab_dword % 2 == 0);
    // the furthest read: zone 1 / zone 3 clamp the start to lim - NB_ORIGIN (last row, last column, steepest angle) and read npx pairs
    // from it, every other one when up-sampled
    const int far_a = L.lim_a + ((npx - 1) << ua), far_l = L.lim_l + ((npx - 1) << ul);
    CHECK(far_a <= last_staged && far_l <= last_staged);
    // zone 2 starts at position -(1 << up) of either edge: the first staged dword
    CHECK(NB_ORIGIN - (1 << ua) >= NB_ORIGIN - 2 && NB_ORIGIN - (1 << ul) >= NB_ORIGIN - 2);
    CHECK(L.bytes <= SAD_LDS_MAX);
    if (L.bytes > g_lds_max) { g_lds_max = L.bytes; g_lds_max_case[0] = bw; g_lds_max_case[1] = bh; g_lds_max_case[2] = es; g_lds_max_case[3] = ua; g_lds_max_case[4] = ul; }
    return 0;
}

static int check_angle_split(int n, size_t grid, size_t want, bool no_split, int chunk, uint32_t gy) {
    CHECK(chunk >= 1);
    if (n == 0) return 0;
    CHECK((uint64_t)chunk * gy >= (uint64_t)n && (uint64_t)(gy - 1) * chunk < (uint64_t)n && gy >= 1);
    if (no_split || grid >= want) CHECK(gy == 1 && chunk == n);
    else CHECK((uint64_t)gy <= (want + grid - 1) / grid);           // no more parts than it takes to reach `want` workgroups
    return 0;
}

static int sweep_intra_pred() {
    static const int kMulti[] = {0, 1, 3, 20};
    for (int ts = 0; ts < SVT_TX_SIZES_ALL; ts++)
    for (int is16 = 0; is16 < 2; is16++)
    for (int mode = 0; mode < SVT_INTRA_MODES; mode++) {
        const int bw = kTxW[ts], bh = kTxH[ts], es = is16 ? 2 : 1, bd = is16 ? 10 : 8;
        const bool dir = mode >= SVT_INTRA_Z1;
        const IntraLanes L = intra_lanes(bw, bh, es);
        CHECK(L.ppl == (bw < 16 / es ? bw : 16 / es) && L.lanes_per_row * L.ppl == bw && L.per_block == (uint32_t)(bw / L.ppl * bh));
        CHECK(pow2(L.per_block) && L.per_block >= 4 && L.per_block <= 512);
        for (int up = 0; up < (dir ? 4 : 1); up++)
        for (int mi = 0; mi < (dir ? 4 : 1); mi++)
        for (const IntraKnobs& K : kKnobs)
        for (size_t n : kCounts) {
            const int ua = up & 1, ul = up >> 1, multi = kMulti[mi];
            IntraPredPlan P;
            const int rc = intra_pred_plan(P, A, B, C, 4096, mode, bw, bh, ua, ul, 3, 5, is16, bd, n, multi, K);
            const uint64_t need = ((uint64_t)L.per_block * n + 255) / 256;
            if (need > 0x7fffffffu) { REFUSED(rc, TOO_MANY); continue; }
            CHECK(rc == SVT_HIP_OK);
            CHECK(P.family == (dir ? INTRA_FAM_DIR : INTRA_FAM_PLAIN) && P.is_16bit == is16 && P.mode == mode && P.nblocks == n);
            const bool wide = bw >= 16 / es;
            const int iu = dir || !wide ? 1 : ((mode == SVT_INTRA_SMOOTH || mode == SVT_INTRA_SMOOTH_V || mode == SVT_INTRA_SMOOTH_H || mode == SVT_INTRA_PAETH) ? 4 : 2);
            if (!dir) CHECK(P.wide == wide && P.iu == iu && P.lds_bytes == 0 && P.grid_y == 1);
            // every item has a lane; a lane keeps its row and column from one of its items to the next; no smaller grid does both
            const uint64_t lanes = (uint64_t)P.grid_x * 256;
            CHECK(lanes * iu >= (uint64_t)L.per_block * n && lanes % L.per_block == 0);
            const uint64_t step = L.per_block > 256 ? 2 : 1;
            CHECK(P.grid_x >= step && ((uint64_t)P.grid_x - step) * 256 * iu < (uint64_t)L.per_block * n);
            CHECK(P.grid_x == parent_grid(L.per_block, n, dir, wide, iu));
            if (!dir) {
                CHECK(P.dc_magic == (uint32_t)(0x100000000ull / (uint64_t)(mode == SVT_INTRA_DC ? bw + bh : (mode == SVT_INTRA_DC_TOP ? bw : bh))) + 1u);
                continue;
            }
            CHECK(P.npx == L.ppl && P.lds_bytes == P.lds.bytes);
            CHECK(P.tab == (multi > 0 && mode == SVT_INTRA_Z2 && bw == L.ppl && !ua && !ul));
            TRY(check_dir_lds(P.lds, bw, bh, es, ua, ul, P.npx));
            if (multi == 0) CHECK(P.chunk == 1 && P.grid_y == 1);
            else TRY(check_angle_split(multi, P.grid_x, (size_t)K.dir_split_target * K.num_cu, K.dir_no_split != 0, P.chunk, P.grid_y));
        }
    }
    // The up-sampled 8-bit 4x4 block asks for 64 slots of 164 dwords and the table: 42 496 bytes, the largest request among the shapes
    // the reference up-samples (w + h <= 16; 8x4 asks for the same).  The entry point takes the flags for every shape, and a block of 4
    // lanes with a longer edge has 64 slots too: up-sampled 8-bit 16x4 (one 16-sample lane per row), 64 slots of 196 dwords, 50 688 bytes.
    size_t small_max = 0;
    for (int ts = 0; ts < SVT_TX_SIZES_ALL; ts++)
        for (int es = 1; es <= 2; es++)
            if (kTxW[ts] + kTxH[ts] <= 16 && dir_lds(kTxW[ts], kTxH[ts], es, 1, 1).bytes > small_max) small_max = dir_lds(kTxW[ts], kTxH[ts], es, 1, 1).bytes;
    CHECK(dir_lds(4, 4, 1, 1, 1).bytes == 42496 && small_max == 42496);
    CHECK(g_lds_max == 50688 && g_lds_max_case[0] == 16 && g_lds_max_case[1] == 4 && g_lds_max_case[2] == 1 && (g_lds_max_case[3] | g_lds_max_case[4]));
    return 0;
}

// umulhi(s + cnt / 2, dc_magic) == (s + cnt / 2) / cnt for every count of the DC modes and every sum below 2^20 (64 + 64 samples of 12 bits)
static int sweep_dc_magic() {
    bool seen[129] = {};
    for (int ts = 0; ts < SVT_TX_SIZES_ALL; ts++)
        for (int mode : {SVT_INTRA_DC, SVT_INTRA_DC_TOP, SVT_INTRA_DC_LEFT}) {
            const int cnt = intra_dc_count(mode, kTxW[ts], kTxH[ts]);
            CHECK(cnt >= 4 && cnt <= 128);
            if (seen[cnt]) continue;
            seen[cnt] = true;
            const uint32_t magic = intra_dc_magic(cnt);
            for (uint32_t s = 0; s < (1u << 20); s++)
                if (umulhi(s + (uint32_t)(cnt >> 1), magic) != (s + (uint32_t)(cnt >> 1)) / (uint32_t)cnt) { fprintf(stderr, "dc_magic: cnt %d sum %u\n", cnt, s); return 1; }
        }
    return 0;
}

// the three zones of the open-loop search in one launch
static int sweep_ois_dir3() {
    static const int kN[][3] = {{5, 7, 3}, {0, 4, 2}, {20, 0, 20}, {1, 1, 0}, {20, 20, 20}};
    for (uint32_t bsize : {8u, 16u})
    for (const IntraKnobs& K : kKnobs)
    for (size_t n : {(size_t)1, (size_t)2, (size_t)3, (size_t)5, (size_t)300, (size_t)32400, (size_t)(0x7fffffffu / 256)})
    for (const auto& nz : kN) {
        OisDir3Plan P;
        ois_dir3_plan(P, bsize, n, nz, K);
        TRY(check_dir_lds(P.lds, (int)bsize, (int)bsize, 1, 0, 0, (int)bsize));
        CHECK(P.lds.lpb == bsize && P.lds.lim_a == NB_ORIGIN + (int)(2 * bsize - 1) && P.lds.lim_l == P.lds.lim_a && P.lds.n_pad == P.lds.lim_a + 19);
        CHECK((uint64_t)P.grid_x * 256 >= (uint64_t)bsize * n && ((uint64_t)P.grid_x - 1) * 256 < (uint64_t)bsize * n && P.nblocks == n);
        uint32_t gy[3] = {P.y_end[0], P.y_end[1] - P.y_end[0], P.grid_y - P.y_end[1]};
        for (int z = 0; z < 3; z++) {
            TRY(check_angle_split(nz[z], P.grid_x, (size_t)K.num_cu, K.dir_no_split != 0, P.chunk[z], gy[z]));
            if (nz[z] == 0) CHECK(gy[z] == 0 && P.chunk[z] == 1);            // an empty zone takes no part of grid.y
        }
    }
    return 0;
}

// ---- chroma from luma, the level maps, build_intra_predictors, the ordering pass, the edges ----
static int sweep_rest() {
    static const uint32_t kSides[] = {4, 8, 16, 32, 64};
    for (uint32_t w : kSides) for (uint32_t h : kSides) for (size_t n : kCounts) {
        if (w != 64 && h != 64) {
            const CflLanes L = cfl_lanes(w, h);
            CHECK(L.nchunks == w / (w < 8 ? 4 : 8) * h && pow2(L.lpb) && L.lpb <= 64 && L.lpb * L.slots == 256 && 2 * L.lpb >= L.nchunks);      // (two passes of a block's lanes)
            for (int in_mode = 0; in_mode < 3; in_mode++) {
                CflAcPlan P;
                const int rc = cfl_ac_plan(P, in_mode, in_mode == 2 ? nullptr : A, B, w, (size_t)w * h, w, h, 5, n);
                if (n > 0x7fffffffu / 64) { REFUSED(rc, TOO_MANY); continue; }
                CHECK(rc == SVT_HIP_OK && P.in_mode == in_mode && P.lpb == L.lpb && P.nblocks == n);
                CHECK((uint64_t)P.grid * 256 >= (uint64_t)n * L.lpb && ((uint64_t)P.grid - 1) * 256 < (uint64_t)n * L.lpb);
            }
            for (int is16 = 0; is16 < 2; is16++) {
                CflPredictPlan P;
                const int rc = cfl_predict_plan(P, A, B, C, D, w, w, w, is16 ? 10 : 8, w, h, is16, n);
                CHECK(rc == SVT_HIP_OK && (1u << P.sh) == L.nchunks && P.nblocks == n && P.hi == (is16 ? 1023 : 255));
                CHECK((uint64_t)P.grid * 256 >= (uint64_t)n << P.sh && ((uint64_t)P.grid - 1) * 256 < (uint64_t)n << P.sh);
            }
            const Cfl420Shape S = cfl_420_shape(2 * w, 2 * h);
            CHECK(S.w == w && S.h == h && S.round_offset == (int)(w * h / 2) && (1u << S.num_pel_log2) == w * h);
        }
        // the level map
        for (size_t pitch_off : {(size_t)0, (size_t)4, (size_t)16}) for (uintptr_t ptr_off : {(uintptr_t)0, (uintptr_t)4, (uintptr_t)8}) {
            const size_t bytes = (size_t)(w + 4) * (h + 6) + 16, pitch = ((bytes + 15) & ~(size_t)15) + pitch_off;
            alignas(16) static char lv[32];
            LevelsPlan P;
            TRY(txb_init_levels_plan(P, A, (size_t)w * h, lv + ptr_off, pitch, w, h, n));
            const LevelsGeom& G = P.lg;
            CHECK(G.bytes == bytes && G.ndw * 4 == bytes && pow2(G.lpb) && G.lpb <= 256 && G.lpb * G.slots == 256);
            CHECK(G.wide == ((pitch & 15) == 0 && ptr_off == 0));
            const uint32_t items = G.wide ? (G.ndw + 3) / 4 : G.ndw;
            CHECK(G.lpb >= (items < 256 ? items : 256) && (G.lpb == 1 || G.lpb / 2 < items));      // the smallest power of two that gives every item a lane, up to a workgroup
            const uint32_t dpr = (w + 4) >> 2;
            for (uint32_t d = 0; d < G.ndw; d++) CHECK(umulhi(d, G.row_magic) == d / dpr);
            CHECK((uint64_t)P.grid * G.slots >= n && ((uint64_t)P.grid - 1) * G.slots < n && P.nblocks == n);
        }
    }
    CHECK(txb_side(64) == 32 && txb_side(32) == 32 && txb_side(4) == 4);
    for (int ts = 0; ts < SVT_TX_SIZES_ALL; ts++) for (size_t n : kCounts) for (int is16 = 0; is16 < 2; is16++) {
        const int w = kTxW[ts], h = kTxH[ts], lpb = bip_lanes_per_block(w, h);
        CHECK(pow2((uint32_t)lpb) && lpb >= 4 && lpb <= 64 && 3 * lpb >= w + h + 1 && (lpb == 4 || 3 * (lpb / 2) < w + h + 1));
        BipPlan P;
        TRY(bip_plan(P, A, w, (size_t)w * h, nullptr, B, C, 1 + 2 * (w > h ? w : h), D, ts, is16, is16 ? 10 : 8, n));
        const uint64_t per_wg = (uint64_t)BIP_WAVES * (64 / lpb);
        CHECK(P.w == w && P.h == h && P.threads == 256 && P.nblocks == n && (uint64_t)P.grid * per_wg >= n && ((uint64_t)P.grid - 1) * per_wg < n);
        BipOrderPlan O;
        TRY(bip_order_plan(O, A, B, ts, n));
        CHECK(O.w == w && O.h == h && O.threads == 1024 && O.nblocks == n && (uint64_t)O.grid * BIP_ORDER_TILE >= n && ((uint64_t)O.grid - 1) * BIP_ORDER_TILE < n);
    }
    for (size_t n : kCounts) {
        EdgePlan P;
        TRY(filter_edge_plan(P, A, 16 + 129, 129, 3, n));
        CHECK(P.grid == n && P.threads == 256 && P.nblocks == n);
        TRY(upsample_edge_plan(P, A, 16 + 32, 16, 1, 10, n));
        CHECK(P.grid == n && P.threads == 64 && P.nblocks == n && P.bd == 10);
        TRY(upsample_edge_plan(P, A, 16 + 32, 16, 0, 10, n));
        CHECK(P.bd == 8);
    }
    return 0;
}

// ---- svt_hip_encode_recon_frame_ex: the check enqueues nothing; the fill's wg_end are the running totals of the groups' workgroups ----
static int frame_call() {
    alignas(16) static char lv[64];
    svt_hip_frame_cfl_group cfl[4] = {};
    const uint32_t cw[4] = {4, 8, 16, 32}, ch[4] = {4, 16, 16, 8}, cn[4] = {1000, 0, 77, 5};
    for (int g = 0; g < 4; g++) {
        cfl[g].d_luma_recon = A; cfl[g].d_pred_cb = B; cfl[g].d_pred_cr = C; cfl[g].d_xy = (const uint32_t*)D; cfl[g].d_alpha_q3_cb = (const int32_t*)A;
        cfl[g].d_alpha_q3_cr = (const int32_t*)B; cfl[g].luma_stride = 2 * cw[g]; cfl[g].pred_stride_cb = cfl[g].pred_stride_cr = cw[g];
        cfl[g].width = cw[g]; cfl[g].height = ch[g]; cfl[g].nblocks = cn[g];
    }
    svt_hip_frame_group groups[3] = {};
    svt_hip_frame_levels levels[3] = {};
    const int tx[3] = {SVT_TX_4X4, SVT_TX_64X64, SVT_TX_16X8};
    const uint32_t gn[3] = {999, 3, 50};
    for (int g = 0; g < 3; g++) {
        groups[g].tx_size = tx[g]; groups[g].nblocks = gn[g]; groups[g].d_qcoeff = (int32_t*)A;
        levels[g].d_levels_buf = (uint8_t*)lv + (g == 2 ? 4 : 0);
        levels[g].levels_block_pitch = levels_geom(txb_side(kTxW[tx[g]]), txb_side(kTxH[tx[g]]), 0, nullptr).bytes + (g == 2 ? 4 : 12);
    }
    int launches = 0, live = -1;
    TRY(frame_ex_args_check(groups, 3, 1, cfl, 4, 0, 8));
    TRY(frame_ex_groups_check(groups, 3, cfl, 4, levels, live));
    CHECK(live == 3 && launches == 0);
    TRY(cfl_frame_enqueue(cfl, 4, [&](const CflFrameDesc& d, uint32_t total) {
        launches++;
        uint32_t run = 0;
        int i = 0;
        for (int g = 0; g < 4; g++) {
            if (!cn[g]) continue;
            const CflLanes L = cfl_lanes(cw[g], ch[g]);
            run += (cn[g] + L.slots - 1) / L.slots;
            if (d.g[i].wg_end != run || d.g[i].lpb != L.lpb || d.g[i].nblocks != cn[g] || d.g[i].w != cw[g] || d.g[i].h != ch[g] ||
                d.g[i].round_offset != (int)(cw[g] * ch[g] / 2) || (1u << d.g[i].num_pel_log2) != cw[g] * ch[g]) return 1;
            i++;
        }
        return d.ngroups == 3 && total == run ? 0 : 1;
    }));
    CHECK(launches == 1);
    TRY(levels_frame_enqueue(groups, levels, 3, [&](const LevelsFrameDesc& d, uint32_t total) {
        launches++;
        uint32_t run = 0;
        for (int g = 0; g < 3; g++) {
            const LevelsGeom lg = levels_geom(txb_side(kTxW[tx[g]]), txb_side(kTxH[tx[g]]), levels[g].levels_block_pitch, levels[g].d_levels_buf);
            run += (gn[g] + lg.slots - 1) / lg.slots;
            if (d.g[g].wg_end != run || d.g[g].lpb != lg.lpb || d.g[g].ndw != lg.ndw || d.g[g].row_magic != lg.row_magic || d.g[g].wide != (uint32_t)lg.wide ||
                d.g[g].w != txb_side(kTxW[tx[g]]) || d.g[g].nblocks != gn[g] || d.g[g].levels_pitch != levels[g].levels_block_pitch) return 1;
        }
        return d.ngroups == 3 && total == run ? 0 : 1;
    }));
    CHECK(launches == 2);
    // the call's refusals
    REFUSED(frame_ex_args_check(nullptr, 3, 1, cfl, 4, 0, 8), "group lists");
    REFUSED(frame_ex_args_check(groups, 257, 1, cfl, 4, 0, 8), "more than 256 groups in one call");
    REFUSED(frame_ex_args_check(groups, 3, 1, cfl, 17, 0, 8), "17 chroma-from-luma groups (at most 16: one per chroma transform size)");
    REFUSED(frame_ex_args_check(groups, 3, 4, cfl, 4, 0, 8), "first_chroma_group 4 of 3");
    REFUSED(frame_ex_args_check(groups, 3, 1, cfl, 4, 0, 10), "bit depth 10");
    { auto c = cfl[2]; cfl[2].d_xy = nullptr; REFUSED(frame_ex_groups_check(groups, 3, cfl, 4, levels, live), "chroma-from-luma group 2: NULL member"); cfl[2] = c; }
    { auto c = cfl[2]; cfl[2].width = 64; REFUSED(frame_ex_groups_check(groups, 3, cfl, 4, levels, live), "chroma-from-luma group 2: chroma block 64x16"); cfl[2] = c; }
    { auto c = cfl[2]; cfl[2].luma_stride = 31; REFUSED(frame_ex_groups_check(groups, 3, cfl, 4, levels, live), "chroma-from-luma group 2: stride smaller than the block"); cfl[2] = c; }
    { auto c = cfl[2]; auto e = cfl[3];                    // 32x32: 4 blocks per workgroup, 2^30 workgroups each - the launch's total passes 2^31 - 1 at the second
      for (int g = 2; g < 4; g++) { cfl[g].width = cfl[g].height = cfl[g].pred_stride_cb = cfl[g].pred_stride_cr = 32; cfl[g].luma_stride = 64; cfl[g].nblocks = 0xffffffffu; }
      REFUSED(frame_ex_groups_check(groups, 3, cfl, 4, levels, live), "chroma-from-luma group 3: too many blocks for one launch"); cfl[2] = c; cfl[3] = e; }
    { auto l = levels[1]; levels[1].levels_block_pitch = 1380;
      REFUSED(frame_ex_groups_check(groups, 3, cfl, 4, levels, live), "group 1: levels buffer 1380 B per block (need >= 1384, multiple of 4, 4-byte aligned)");
      levels[1].levels_block_pitch = ((size_t)1 << 32) + 1384;
      REFUSED(frame_ex_groups_check(groups, 3, cfl, 4, levels, live), "group 1: levels buffer 4294968680 B per block (need >= 1384, multiple of 4, 4-byte aligned)");
      levels[1] = l; }
    { groups[0].nblocks = 0x80000000u; REFUSED(frame_ex_groups_check(groups, 3, cfl, 4, levels, live), "group 0: too many blocks for one launch"); groups[0].nblocks = gn[0]; }
    TRY(frame_ex_groups_check(groups, 3, cfl, 4, nullptr, live));
    return 0;
}

// ---- refusals: a valid call, then each clause by its one field; the bound on the block count at 2^31 and 2^32 + 1 ----
static int refusals() {
    const IntraKnobs K = kKnobs[0];
    { CflAcPlan P;
      TRY(cfl_ac_plan(P, 0, A, B, 8, 64, 8, 8, 6, 10));
      REFUSED(cfl_ac_plan(P, 0, nullptr, B, 8, 64, 8, 8, 6, 10), "NULL buffer");
      TRY(cfl_ac_plan(P, 2, nullptr, B, 8, 64, 8, 8, 6, 10));
      REFUSED(cfl_ac_plan(P, 2, nullptr, nullptr, 8, 64, 8, 8, 6, 10), "NULL buffer");
      REFUSED(cfl_ac_plan(P, 0, A, B, 64, 64 * 8, 64, 8, 6, 10), "chroma block 64x8");
      REFUSED(cfl_ac_plan(P, 0, A, B, 8, 64, 8, 12, 6, 10), "chroma block 8x12");
      REFUSED(cfl_ac_plan(P, 0, A, B, 7, 64, 8, 8, 6, 10), "q3 layout: line 7, block pitch 64");
      REFUSED(cfl_ac_plan(P, 0, A, B, 8, 63, 8, 8, 6, 10), "q3 layout: line 8, block pitch 63");
      REFUSED(cfl_ac_plan(P, 0, A, B, 8, 64, 8, 8, 32, 10), "num_pel_log2 32");
      REFUSED(cfl_ac_plan(P, 0, A, B, 8, 64, 8, 8, -1, 10), "num_pel_log2 -1");
      REFUSED(cfl_ac_plan(P, 0, A, B, 8, 64, 8, 8, 6, 0x7fffffffu / 64 + 1), TOO_MANY);
      for (size_t n : kOver) REFUSED(cfl_ac_plan(P, 0, A, B, 4, 16, 4, 4, 4, n), TOO_MANY);
      const Cfl420Shape S = cfl_420_shape(128, 6);          // sides the plan refuses: nothing is derived from them
      CHECK(S.w == 64 && S.h == 3 && S.num_pel_log2 == 0);
      (void)cfl_420_shape(0xfffffffeu, 0xfffffffeu); }
    { CflPredictPlan P;
      TRY(cfl_predict_plan(P, A, B, C, D, 8, 8, 8, 8, 8, 8, 0, 10));
      REFUSED(cfl_predict_plan(P, A, B, C, nullptr, 8, 8, 8, 8, 8, 8, 0, 10), "NULL buffer");
      REFUSED(cfl_predict_plan(P, A, B, C, D, 8, 8, 8, 8, 8, 64, 0, 10), "chroma block 8x64");
      REFUSED(cfl_predict_plan(P, A, B, C, D, 8, 8, 8, 10, 8, 8, 0, 10), "bit depth 10");
      REFUSED(cfl_predict_plan(P, A, B, C, D, 8, 8, 7, 8, 8, 8, 0, 10), "stride smaller than the block");
      for (size_t n : kOver) REFUSED(cfl_predict_plan(P, A, B, C, D, 4, 4, 4, 8, 4, 4, 0, n), TOO_MANY);      // (4x4 at 2^32 + 1 blocks was taken as one block)
    }
    { LevelsPlan P;
      alignas(16) static char lv[32];
      TRY(txb_init_levels_plan(P, A, 16, lv, 96, 4, 4, 10));
      REFUSED(txb_init_levels_plan(P, nullptr, 16, lv, 96, 4, 4, 10), "NULL buffer");
      REFUSED(txb_init_levels_plan(P, A, 16, lv, 96, 4, 5, 10), "block 4x5");
      REFUSED(txb_init_levels_plan(P, A, 16, lv, 92, 4, 4, 10), "levels buffer: 92 B per block (need >= 96, multiple of 4, 4-byte aligned)");
      REFUSED(txb_init_levels_plan(P, A, 16, lv, 98, 4, 4, 10), "levels buffer: 98 B per block (need >= 96, multiple of 4, 4-byte aligned)");
      REFUSED(txb_init_levels_plan(P, A, 16, lv + 2, 96, 4, 4, 10), "levels buffer: 96 B per block (need >= 96, multiple of 4, 4-byte aligned)");
      REFUSED(txb_init_levels_plan(P, A, 15, lv, 96, 4, 4, 10), "coeff_block_pitch 15");
      for (size_t n : kOver) REFUSED(txb_init_levels_plan(P, A, 16, lv, 96, 4, 4, n), TOO_MANY); }
    { IntraPredPlan P;
      TRY(intra_pred_plan(P, A, B, C, 160, SVT_INTRA_Z2, 32, 32, 0, 0, 64, 64, 0, 8, 10, 0, K));
      REFUSED(intra_pred_plan(P, A, nullptr, C, 160, SVT_INTRA_Z2, 32, 32, 0, 0, 64, 64, 0, 8, 10, 0, K), "NULL buffer");
      REFUSED(intra_pred_plan(P, A, B, C, 160, SVT_INTRA_MODES, 32, 32, 0, 0, 64, 64, 0, 8, 10, 0, K), "intra mode 13");
      REFUSED(intra_pred_plan(P, A, B, C, 160, -1, 32, 32, 0, 0, 64, 64, 0, 8, 10, 0, K), "intra mode -1");
      REFUSED(intra_pred_plan(P, A, B, C, 160, SVT_INTRA_Z2, 64, 8, 0, 0, 64, 64, 0, 8, 10, 0, K), "block 64x8 is not an AV1 transform size");
      REFUSED(intra_pred_plan(P, A, B, C, 160, SVT_INTRA_Z2, 32, 12, 0, 0, 64, 64, 0, 8, 10, 0, K), "block 32x12 is not an AV1 transform size");
      REFUSED(intra_pred_plan(P, A, B, C, 160, SVT_INTRA_Z2, 32, 32, 0, 0, 64, 64, 0, 12, 10, 0, K), "bit depth 12");
      REFUSED(intra_pred_plan(P, A, B, C, 160, SVT_INTRA_Z2, 32, 32, 2, 0, 64, 64, 0, 8, 10, 0, K), "upsample flags");
      REFUSED(intra_pred_plan(P, A, B, C, 160, SVT_INTRA_Z2, 32, 32, 0, 0, 0, 64, 0, 8, 10, 0, K), "dx/dy must be positive");
      REFUSED(intra_pred_plan(P, A, B, C, 145, SVT_INTRA_Z2, 32, 32, 0, 0, 64, 64, 0, 8, 10, 0, K), "nb_pitch 145 < 146");
      TRY(intra_pred_plan(P, A, B, C, 48, SVT_INTRA_DC, 32, 16, 0, 0, 0, 0, 0, 8, 10, 0, K));              // (dx, dy are the directional modes')
      REFUSED(intra_pred_plan(P, A, B, C, 47, SVT_INTRA_DC, 32, 16, 0, 0, 0, 0, 0, 8, 10, 0, K), "nb_pitch 47 too small");
      for (size_t n : kOver) {
          REFUSED(intra_pred_plan(P, A, B, C, 160, SVT_INTRA_Z2, 4, 4, 0, 0, 64, 64, 0, 8, n, 0, K), TOO_MANY);      // (4 lanes per block: the grid alone admitted 2^37 blocks)
          REFUSED(intra_pred_plan(P, A, B, C, 160, SVT_INTRA_V, 4, 4, 0, 0, 64, 64, 0, 8, n, 0, K), TOO_MANY);
      } }
    { EdgePlan P;
      TRY(filter_edge_plan(P, A, 145, 129, 1, 10));
      REFUSED(filter_edge_plan(P, nullptr, 145, 129, 1, 10), "NULL buffer");
      REFUSED(filter_edge_plan(P, A, 145, 130, 1, 10), "edge sz 130 strength 1 pitch 145");
      REFUSED(filter_edge_plan(P, A, 145, 0, 1, 10), "edge sz 0 strength 1 pitch 145");
      REFUSED(filter_edge_plan(P, A, 145, 129, 4, 10), "edge sz 129 strength 4 pitch 145");
      REFUSED(filter_edge_plan(P, A, 145, 129, -1, 10), "edge sz 129 strength -1 pitch 145");
      REFUSED(filter_edge_plan(P, A, 144, 129, 1, 10), "edge sz 129 strength 1 pitch 144");
      TRY(upsample_edge_plan(P, A, 48, 16, 0, 8, 10));
      REFUSED(upsample_edge_plan(P, nullptr, 48, 16, 0, 8, 10), "NULL buffer");
      REFUSED(upsample_edge_plan(P, A, 48, 17, 0, 8, 10), "upsample sz 17 pitch 48");
      REFUSED(upsample_edge_plan(P, A, 47, 16, 0, 8, 10), "upsample sz 16 pitch 47");
      for (size_t n : kOver) {                              // (neither had a bound: a zero grid at 2^32 blocks, a runtime error)
          REFUSED(filter_edge_plan(P, A, 145, 129, 1, n), TOO_MANY);
          REFUSED(upsample_edge_plan(P, A, 48, 16, 0, 8, n), TOO_MANY);
      } }
    { BipPlan P;
      TRY(bip_plan(P, A, 16, 256, nullptr, B, C, 33, D, SVT_TX_16X16, 0, 8, 10));
      REFUSED(bip_plan(P, A, 16, 256, nullptr, B, C, 33, nullptr, SVT_TX_16X16, 0, 8, 10), "NULL buffer");
      REFUSED(bip_plan(P, A, 16, 256, nullptr, B, C, 33, D, SVT_TX_SIZES_ALL, 0, 8, 10), "tx_size 19");
      REFUSED(bip_plan(P, A, 16, 256, nullptr, B, C, 33, D, SVT_TX_16X16, 0, 10, 10), "bit depth 10");
      REFUSED(bip_plan(P, A, 16, 256, nullptr, B, C, 32, D, SVT_TX_16X16, 0, 8, 10), "neigh_pitch 32 < 33");
      REFUSED(bip_plan(P, A, 15, 256, nullptr, B, C, 33, D, SVT_TX_16X16, 0, 8, 10), "dst_stride 15 < width 16");
      REFUSED(bip_plan(P, A, 16, 0, nullptr, B, C, 33, D, SVT_TX_16X16, 0, 8, 10), "dst_block_pitch 0 without offsets");
      TRY(bip_plan(P, A, 16, 0, D, B, C, 33, D, SVT_TX_16X16, 0, 8, 10));
      for (size_t n : kOver) REFUSED(bip_plan(P, A, 4, 16, nullptr, B, C, 9, D, SVT_TX_4X4, 0, 8, n), TOO_MANY);       // (64 blocks per workgroup: the grid alone admitted 2^37)
      BipOrderPlan O;
      TRY(bip_order_plan(O, A, B, SVT_TX_16X16, 10));
      REFUSED(bip_order_plan(O, A, nullptr, SVT_TX_16X16, 10), "NULL buffer");
      REFUSED(bip_order_plan(O, A, B, -1, 10), "tx_size -1");
      for (size_t n : kOver) REFUSED(bip_order_plan(O, A, B, SVT_TX_16X16, n), "too many blocks"); }
    return 0;
}

// ---- the pinned rows: what the entry points launched before the plan existed ----
static int pins() {
    CHECK(kPinCu == kKnobs[0].num_cu && kKnobs[0].dir_split_target == 4 && !kKnobs[0].dir_no_split);      // the device and the knobs' defaults of the recorded run
    for (const PinCflAc& r : kPinCflAc) {
        CflAcPlan P;
        TRY(cfl_ac_plan(P, r.in_mode, r.in_mode == 2 ? nullptr : A, B, r.w, (size_t)r.w * r.h, r.w, r.h, 5, r.n));
        CHECK(P.grid == r.grid && P.lpb == r.lpb && P.nblocks == r.n && P.in_mode == r.in_mode);
    }
    for (const PinCflPredict& r : kPinCflPredict) {
        CflPredictPlan P;
        TRY(cfl_predict_plan(P, A, B, C, D, r.w, r.w, r.w, r.is16 ? 10 : 8, r.w, r.h, r.is16, r.n));
        CHECK(P.grid == r.grid && P.sh == r.sh && P.nblocks == r.n);
    }
    alignas(16) static char lv[32];
    for (const PinLevels& r : kPinLevels) {
        const size_t need = (size_t)(r.w + 4) * (r.h + 6) + 16;
        LevelsPlan P;
        TRY(txb_init_levels_plan(P, A, (size_t)r.w * r.h, lv + r.amod, ((need + 15) & ~(size_t)15) + 16 + r.pmod, r.w, r.h, r.n));
        CHECK(P.lg.wide == (r.wide != 0) && P.grid == r.grid && P.lg.lpb == r.lpb && P.lg.ndw == r.ndw && P.lg.row_magic == r.row_magic);
    }
    for (const PinLevelsFrame& r : kPinLevelsFrame) {
        svt_hip_frame_group G = {};
        G.tx_size = r.tx; G.nblocks = r.n;
        const uint32_t w = txb_side(kTxW[r.tx]), h = txb_side(kTxH[r.tx]);
        svt_hip_frame_levels L = {(uint8_t*)lv + r.amod, (((size_t)(w + 4) * (h + 6) + 16 + 15) & ~(size_t)15) + 16 + r.pmod};
        const LevelsGeom lg = levels_group_geom(G, L);
        CHECK(lg.wide == (r.wide != 0) && levels_group_wgs(r.n, lg) == r.wgs && lg.lpb == r.lpb && lg.ndw == r.ndw && lg.row_magic == r.row_magic);
    }
    for (const PinCflFrame& r : kPinCflFrame) {
        svt_hip_frame_cfl_group G = {};
        G.d_luma_recon = A; G.d_pred_cb = B; G.d_pred_cr = C; G.d_xy = (const uint32_t*)D; G.d_alpha_q3_cb = (const int32_t*)A; G.d_alpha_q3_cr = (const int32_t*)B;
        G.luma_stride = 2 * r.w; G.pred_stride_cb = G.pred_stride_cr = r.w; G.width = r.w; G.height = r.h; G.nblocks = r.n;
        bool ok = false;
        TRY(cfl_frame_enqueue(&G, 1, [&](const CflFrameDesc& d, uint32_t total) {
            ok = total == r.wgs && d.g[0].wg_end == r.wgs && d.g[0].lpb == r.lpb && d.g[0].round_offset == r.round_offset && d.g[0].num_pel_log2 == r.num_pel_log2;
            return 0;
        }));
        CHECK(ok);
    }
    for (const PinIntraPred& r : kPinIntraPred) {
        IntraPredPlan P;
        TRY(intra_pred_plan(P, A, B, C, 4096, r.mode, r.bw, r.bh, 0, 0, 1, 1, r.is16, r.is16 ? 10 : 8, r.n, 0, kKnobs[0]));
        CHECK(P.family == INTRA_FAM_PLAIN && P.wide == (r.wide != 0) && P.iu == r.iu && P.grid_x == r.gx && P.grid_y == 1 && P.lds_bytes == 0 && P.dc_magic == r.dc_magic);
    }
    for (const PinIntraDir& r : kPinIntraDir) {
        IntraPredPlan P;
        const IntraKnobs K = {r.nosplit, r.target, r.cu};
        TRY(intra_pred_plan(P, A, B, C, 4096, r.mode, r.bw, r.bh, r.ua, r.ul, 1, 1, r.is16, r.is16 ? 10 : 8, r.n, r.multi, K));
        CHECK(P.family == INTRA_FAM_DIR && P.npx == r.npx && P.tab == (r.tab != 0) && P.grid_x == r.gx && P.grid_y == r.gy && P.lds_bytes == r.lds);
        CHECK(P.lds.lim_a == r.lim_a && P.lds.lim_l == r.lim_l && P.lds.n_pad == r.n_pad && P.chunk == r.chunk);
    }
    for (const PinEdge& r : kPinEdge) {
        EdgePlan P;
        if (r.up) TRY(upsample_edge_plan(P, A, 4096, r.sz, r.is16, r.bd, r.n)); else TRY(filter_edge_plan(P, A, 4096, r.sz, r.bd /* strength */, r.n));
        CHECK(P.grid == r.grid && P.threads == r.threads && P.nblocks == r.n && (!r.up || P.bd == r.bd_arg));
    }
    for (const PinBip& r : kPinBip) {
        BipPlan P;
        TRY(bip_plan(P, A, 64, 4096, nullptr, B, C, 129, D, r.tx, r.is16, r.is16 ? 10 : 8, r.n));
        CHECK(P.grid == r.grid && P.threads == r.threads && P.w == kTxW[r.tx] && P.h == kTxH[r.tx]);
    }
    for (const PinOrder& r : kPinOrder) {
        BipOrderPlan P;
        TRY(bip_order_plan(P, A, B, r.tx, r.n));
        CHECK(P.grid == r.grid && P.threads == r.threads);
    }
    for (const PinOis3& r : kPinOis3) {
        OisDir3Plan P;
        const int nz[3] = {r.n1, r.n2, r.n3};
        ois_dir3_plan(P, r.bsize, r.n, nz, IntraKnobs{r.nosplit, 4, r.cu});
        CHECK(P.grid_x == r.gx && P.grid_y == r.gy && P.lds.bytes == r.lds && P.lds.lim_a == r.lim && P.lds.lim_l == r.lim && P.lds.n_pad == r.n_pad);
        CHECK(P.chunk[0] == r.c1 && P.chunk[1] == r.c2 && P.chunk[2] == r.c3 && P.y_end[0] == r.y0 && P.y_end[1] == r.y1);
    }
    return 0;
}

int main() {
    TRY(sweep_intra_pred());
    TRY(sweep_dc_magic());
    TRY(sweep_ois_dir3());
    TRY(sweep_rest());
    TRY(frame_call());
    TRY(refusals());
    TRY(pins());
    fprintf(stderr, "largest directional LDS request: %zu bytes (%dx%d, %d-byte samples, up-sampling %d / %d)\n", g_lds_max, g_lds_max_case[0], g_lds_max_case[1],
            g_lds_max_case[2], g_lds_max_case[3], g_lds_max_case[4]);
    printf("ok\n");
    return 0;
}

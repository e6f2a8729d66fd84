// csrc/md_plan.h on the CPU, the part of the decide of mode decision: md_decide_check (every refusal of svt_hip_md_decide_frame: a valid
// group is accepted, the same group with one field changed is refused, the neighbour of each bound accepted), md_geom / md_decide_bpul
// (the wave-unit of every block size and slot count inside the kernel's tile and gather budget), and md_search_walk, the single walk of
// svt_hip_md_search_frame: the scratch size against the hand formula of include/svt_hip_dsp.h, every piece inside a scratch of exactly
// that size, 16-byte aligned, in the documented order and overlapping nothing, supplied arrays passed through, the derived stage groups
// consistent with each other and accepted by their stages' checks.  "Device" pointers are addresses inside a host array that nothing
// dereferences; the scratch is a host allocation of exactly the reported size, so AddressSanitizer guards its end.
// Plain C++17 (g++), linked with csrc/host_tables.cpp and csrc/host_err.cpp, built plain and under -fsanitize=address,undefined by
// tests/test_md_decide_plan_host.py and run directly.  Exit status 0 and "ok" when every case holds.
#include <stdio.h>
#include <stdlib.h>

#include <functional>
#include <vector>

#include "../../cidana-svt-av1_amd/csrc/md_plan.h"

using namespace svthost;

#define CHECK(c) do { if (!(c)) { fprintf(stderr, "%s:%d: %s (last error: %s)\n", __FILE__, __LINE__, #c, svt_hip_last_error()); return 1; } } while (0)
#define TRY(call) do { if (call) { fprintf(stderr, "  from %s:%d\n", __FILE__, __LINE__); return 1; } } while (0)
static const int INVALID = SVT_HIP_ERR_INVALID;

alignas(64) static char g_dev[1 << 20];
static size_t g_dev_next = 0;
template <typename T>
static T* dev() {
    if (64 * (g_dev_next + 2) > sizeof(g_dev)) { fprintf(stderr, "g_dev too small\n"); exit(2); }
    return (T*)(g_dev + 64 * ++g_dev_next);
}
template <typename T>
static T* off(T* p, int bytes) { return (T*)((char*)p + bytes); }
template <typename T>
static const T* off(const T* p, int bytes) { return (const T*)((const char*)p + bytes); }
static size_t A(size_t v) { return (v + 15) & ~(size_t)15; }

struct Piece { const void* p; size_t bytes; };
static int pieces_ok(const std::vector<Piece>& v, const char* base, size_t size) {
    const char* at = base;
    size_t sum = 0;
    for (const Piece& P : v) {
        const char* p = (const char*)P.p;
        CHECK(p != nullptr && ((uintptr_t)p & 15) == 0);
        CHECK(p == at && p + P.bytes <= base + size);          // right after the piece before it, inside the scratch
        at = p + A(P.bytes);
        sum += A(P.bytes);
    }
    CHECK(sum == size);
    return 0;
}
struct Scratch {
    char* p;
    explicit Scratch(size_t size) : p(size ? (char*)malloc(size) : nullptr) {}
    ~Scratch() { free(p); }
};

static int16_t g_zbin[8], g_round[8], g_quant[8], g_shift[8], g_dequant[8];
static svt_hip_qrows good_rows() { return {g_zbin, g_round, g_quant, g_shift, g_dequant}; }

// ---- a valid decide group: everything given ----
static svt_hip_md_decide_group md_group(int bsize, int n, uint32_t nblocks) {
    svt_hip_md_decide_group g{};
    g.bsize = bsize; g.nblocks = nblocks; g.n = n; g.ninter = 5; g.nintra = 4; g.lambda = 29041; g.full_loop_escape = 1;
    for (int c = 0; c < 4; c++) g.modes[c] = (uint8_t)(3 * c);
    g.d_luma = dev<svt_hip_tx_decision>();
    g.d_dist_cb = dev<uint64_t>(); g.d_dist_cr = dev<uint64_t>(); g.d_bits_cb = dev<uint64_t>(); g.d_bits_cr = dev<uint64_t>();
    g.d_eob_cb = dev<uint16_t>(); g.d_eob_cr = dev<uint16_t>();
    g.d_rate = dev<uint32_t>(); g.d_cand = dev<uint8_t>(); g.d_cand_out = dev<svt_hip_inter_cand>(); g.d_cfl = dev<svt_hip_cfl_decision>();
    g.d_blk = dev<svt_hip_md_blk>(); g.d_rates = dev<svt_hip_md_rates>(); g.d_decision = dev<svt_hip_md_decision>(); g.d_full_cost = dev<uint64_t>();
    for (int p = 0; p < 3; p++) {
        g.d_pred[p] = dev<uint8_t>(); g.d_best_pred[p] = dev<uint8_t>();
        g.d_qcoeff[p] = dev<int32_t>(); g.d_dqcoeff[p] = dev<int32_t>(); g.d_best_qcoeff[p] = dev<int32_t>(); g.d_best_dqcoeff[p] = dev<int32_t>();
    }
    g.d_inter_blk = dev<svt_hip_inter_blk>(); g.d_best_inter_blk = dev<svt_hip_inter_blk>();
    return g;
}
using Change = std::function<void(svt_hip_md_decide_group&)>;
static int refused(const svt_hip_md_decide_group& good, const Change& change, int line) {
    static const svt_hip_md_decide_group other = md_group(6, 3, 9);
    svt_hip_md_decide_group bad = good;
    change(bad);
    for (int order = 0; order < 2; order++) {
        const svt_hip_md_decide_group gs[2] = {order ? bad : other, order ? other : bad};
        if (md_decide_check(gs, 2) != INVALID) { fprintf(stderr, "line %d: a changed group was accepted\n", line); return 1; }
    }
    return 0;
}
static int accepted(const svt_hip_md_decide_group& good, const Change& change, int line) {
    svt_hip_md_decide_group g = good;
    change(g);
    if (md_decide_check(&g, 1) != SVT_HIP_OK) { fprintf(stderr, "line %d: refused: %s\n", line, svt_hip_last_error()); return 1; }
    return 0;
}
#define REFUSED(...) TRY(refused(good, [&](svt_hip_md_decide_group& g) { __VA_ARGS__; }, __LINE__))
#define ACCEPTED(...) TRY(accepted(good, [&](svt_hip_md_decide_group& g) { __VA_ARGS__; }, __LINE__))

static int test_decide_check() {
    const svt_hip_md_decide_group good = md_group(3, 12, 7);
    CHECK(md_decide_check(&good, 1) == SVT_HIP_OK);
    CHECK(md_decide_check(nullptr, 0) == SVT_HIP_OK && md_decide_check(nullptr, 1) == INVALID && md_decide_check(&good, -1) == INVALID);
    // scalars, of empty groups too
    for (uint32_t nb : {7u, 0u}) {
        for (int b : {-1, 13, 14, 15, 22}) REFUSED(g.nblocks = nb; g.bsize = b);
        for (int n : {0, -1, 41}) REFUSED(g.nblocks = nb; g.n = n);
        REFUSED(g.nblocks = nb; g.ninter = 0; g.nintra = 0);
        REFUSED(g.nblocks = nb; g.ninter = -1);
        REFUSED(g.nblocks = nb; g.nintra = -1; g.ninter = 9);
        REFUSED(g.nblocks = nb; g.ninter = 60; g.nintra = 5);
        REFUSED(g.nblocks = nb; g.full_loop_escape = 3);
        REFUSED(g.nblocks = nb; g.full_loop_escape = -1);
        REFUSED(g.nblocks = nb; g.modes[3] = 13);
    }
    for (int b = 0; b < 22; b++)
        if (b < 13 || b > 15) ACCEPTED(g.bsize = b);
    ACCEPTED(g.n = 1); ACCEPTED(g.n = 40); ACCEPTED(g.ninter = 60; g.nintra = 4); ACCEPTED(g.ninter = 0; g.nintra = 1; g.d_cand_out = nullptr);
    ACCEPTED(g.ninter = 64; g.nintra = 0); ACCEPTED(g.full_loop_escape = 0); ACCEPTED(g.full_loop_escape = 2); ACCEPTED(g.modes[4] = 200);
    ACCEPTED(g.nblocks = 0; g.d_luma = nullptr; g.d_decision = nullptr);                 // an empty group's pointers are not looked at
    REFUSED(g.n = 40; g.nblocks = 0x7fffffffu / 40 + 1);
    ACCEPTED(g.n = 1; g.nblocks = 0x7fffffffu);
    REFUSED(g.n = 2; g.nblocks = 0x40000000u);
    // required members
    REFUSED(g.d_luma = nullptr); REFUSED(g.d_rate = nullptr); REFUSED(g.d_cand = nullptr); REFUSED(g.d_blk = nullptr);
    REFUSED(g.d_rates = nullptr); REFUSED(g.d_decision = nullptr); REFUSED(g.d_cand_out = nullptr);
    ACCEPTED(g.d_cfl = nullptr); ACCEPTED(g.d_full_cost = nullptr);
    // chroma: all six or none
    REFUSED(g.d_dist_cr = nullptr); REFUSED(g.d_bits_cr = nullptr); REFUSED(g.d_eob_cr = nullptr); REFUSED(g.d_dist_cb = nullptr);
    REFUSED(g.d_dist_cb = nullptr; g.d_bits_cb = nullptr; g.d_eob_cb = nullptr);          // Cr without Cb
    REFUSED(g.d_dist_cr = nullptr; g.d_bits_cr = nullptr; g.d_eob_cr = nullptr);          // Cb without Cr
    ACCEPTED(g.d_dist_cb = g.d_dist_cr = g.d_bits_cb = g.d_bits_cr = nullptr; g.d_eob_cb = g.d_eob_cr = nullptr);
    // gathers: each needs its input and is not its input; an input without its gather is fine
    for (int p = 0; p < 3; p++) {
        REFUSED(g.d_pred[p] = nullptr); REFUSED(g.d_qcoeff[p] = nullptr); REFUSED(g.d_dqcoeff[p] = nullptr);
        REFUSED(g.d_best_pred[p] = const_cast<uint8_t*>(g.d_pred[p])); REFUSED(g.d_best_qcoeff[p] = const_cast<int32_t*>(g.d_qcoeff[p]));
        REFUSED(g.d_best_dqcoeff[p] = const_cast<int32_t*>(g.d_dqcoeff[p]));
        ACCEPTED(g.d_best_pred[p] = nullptr); ACCEPTED(g.d_best_qcoeff[p] = nullptr; g.d_qcoeff[p] = nullptr);
        ACCEPTED(g.d_best_dqcoeff[p] = nullptr; g.d_dqcoeff[p] = nullptr; g.d_best_pred[p] = nullptr; g.d_pred[p] = nullptr);
        // 16 bytes
        for (int o : {4, 8}) {
            REFUSED(g.d_pred[p] = off(g.d_pred[p], o)); REFUSED(g.d_best_pred[p] = off(g.d_best_pred[p], o));
            REFUSED(g.d_qcoeff[p] = off(g.d_qcoeff[p], o)); REFUSED(g.d_best_qcoeff[p] = off(g.d_best_qcoeff[p], o));
            REFUSED(g.d_dqcoeff[p] = off(g.d_dqcoeff[p], o)); REFUSED(g.d_best_dqcoeff[p] = off(g.d_best_dqcoeff[p], o));
        }
        ACCEPTED(g.d_pred[p] = off(g.d_pred[p], 16); g.d_best_qcoeff[p] = off(g.d_best_qcoeff[p], 16));
    }
    REFUSED(g.d_inter_blk = nullptr); REFUSED(g.d_best_inter_blk = const_cast<svt_hip_inter_blk*>(g.d_inter_blk));
    REFUSED(g.d_inter_blk = off(g.d_inter_blk, 8)); REFUSED(g.d_best_inter_blk = off(g.d_best_inter_blk, 4));
    ACCEPTED(g.d_best_inter_blk = nullptr; g.d_inter_blk = nullptr);
    // 8 bytes: records and uint64 arrays
    REFUSED(g.d_luma = off(g.d_luma, 4)); REFUSED(g.d_dist_cb = off(g.d_dist_cb, 4)); REFUSED(g.d_dist_cr = off(g.d_dist_cr, 4));
    REFUSED(g.d_bits_cb = off(g.d_bits_cb, 4)); REFUSED(g.d_bits_cr = off(g.d_bits_cr, 4)); REFUSED(g.d_cfl = off(g.d_cfl, 4));
    REFUSED(g.d_decision = off(g.d_decision, 4)); REFUSED(g.d_full_cost = off(g.d_full_cost, 4));
    ACCEPTED(g.d_luma = off(g.d_luma, 8); g.d_decision = off(g.d_decision, 8); g.d_dist_cb = off(g.d_dist_cb, 8));
    // 4 bytes: the uint32 and int32 tables and the 4-byte records; 2 bytes: the eobs; d_cand is bytes
    REFUSED(g.d_rate = off(g.d_rate, 2)); REFUSED(g.d_rates = off(g.d_rates, 2)); REFUSED(g.d_blk = off(g.d_blk, 2)); REFUSED(g.d_cand_out = off(g.d_cand_out, 2));
    REFUSED(g.d_eob_cb = off(g.d_eob_cb, 1)); REFUSED(g.d_eob_cr = off(g.d_eob_cr, 1));
    ACCEPTED(g.d_rate = off(g.d_rate, 4); g.d_rates = off(g.d_rates, 4); g.d_blk = off(g.d_blk, 4); g.d_eob_cb = off(g.d_eob_cb, 2); g.d_cand = off(g.d_cand, 1));
    return 0;
}

static int test_geometry() {
    // per plane: prediction bytes and coefficients, hand values
    const MdGeom a = md_geom(0), b = md_geom(9), c = md_geom(12), d = md_geom(16), e = md_geom(21);
    CHECK(a.pred_bytes[0] == 16 && a.pred_bytes[1] == 16 && a.ncoeff[0] == 16 && a.ncoeff[2] == 16);                 // 4x4: chroma 4x4
    CHECK(b.pred_bytes[0] == 1024 && b.pred_bytes[1] == 256 && b.ncoeff[0] == 1024 && b.ncoeff[1] == 256);           // 32x32
    CHECK(c.pred_bytes[0] == 4096 && c.pred_bytes[2] == 1024 && c.ncoeff[0] == 1024 && c.ncoeff[2] == 1024);         // 64x64 packs to 32x32
    CHECK(d.pred_bytes[0] == 64 && d.pred_bytes[1] == 32 && d.ncoeff[1] == 32);                                      // 4x16: chroma 4x8
    CHECK(e.pred_bytes[0] == 1024 && e.ncoeff[0] == 512 && e.pred_bytes[1] == 256 && e.ncoeff[1] == 256);            // 64x16: 32x16 coefficients
    CHECK(md_decide_bpul(0, 1) == 6 && md_decide_bpul(0, 16) == 6 && md_decide_bpul(0, 17) == 5 && md_decide_bpul(0, 40) == 4);
    CHECK(md_decide_bpul(12, 1) == 1 && md_decide_bpul(12, 40) == 1 && md_decide_bpul(9, 3) == 1 && md_decide_bpul(6, 12) == 3 && md_decide_bpul(3, 12) == 5);
    for (int bs = 0; bs < 22; bs++) {
        if (!md_bsize_ok(bs)) continue;
        const MdGeom m = md_geom(bs);
        for (int n = 1; n <= SVT_HIP_MAX_NFL; n++) {
            const int bpul = md_decide_bpul(bs, n);
            CHECK(bpul >= 0 && bpul <= 6 && ((n + 1) << bpul) <= kMdTileWords);
            for (int p = 0; p < 3; p++) {
                CHECK(m.pred_bytes[p] >= 16 && (m.pred_bytes[p] & (m.pred_bytes[p] - 1)) == 0 && m.ncoeff[p] >= 16 && (m.ncoeff[p] & (m.ncoeff[p] - 1)) == 0);
                CHECK(((m.pred_bytes[p] / 16) << bpul) <= 512 && ((m.ncoeff[p] / 4) << bpul) <= 512);                    // quads of a unit's gather
            }
        }
    }
    return 0;
}

// ---- the composed search ----
static svt_hip_md_search_group ms_group(int bsize, int n, uint32_t nblocks, int tx, std::vector<int> types, int tx_uv, bool chroma, bool supplied, bool gathers) {
    svt_hip_md_search_group g{};
    g.md = md_group(bsize, n, nblocks);
    if (!gathers)
        for (int p = 0; p < 3; p++) { g.md.d_best_qcoeff[p] = nullptr; g.md.d_best_dqcoeff[p] = nullptr; }
    const uint32_t pairs = nblocks * (uint32_t)n;
    auto fl = [&](int tx_size, const std::vector<int>& ty) {
        svt_hip_full_loop_group f{};
        f.d_src = dev<uint8_t>(); f.d_pred = dev<uint8_t>(); f.nblocks = pairs; f.tx_size = tx_size; f.d_iscan = dev<int16_t>();
        for (int t : ty) f.tx_types[f.ntypes++] = (uint8_t)t;
        if (supplied) { f.d_dist = dev<uint64_t>(); f.d_eob = dev<uint16_t>(); f.d_qcoeff = dev<int32_t>(); f.d_dqcoeff = dev<int32_t>(); }
        return f;
    };
    g.luma.fl = fl(tx, types);
    g.luma.d_txb_skip_ctx = dev<uint8_t>(); g.luma.d_dc_sign_ctx = dev<uint8_t>(); g.luma.d_coeff_cost = dev<int32_t>(); g.luma.d_eob_cost = dev<int32_t>();
    g.luma.lambda = 29041;
    if (supplied) { g.luma.d_decision = dev<svt_hip_tx_decision>(); g.luma.d_best_qcoeff = dev<int32_t>(); g.luma.d_best_dqcoeff = dev<int32_t>(); }
    g.use_chroma = chroma;
    g.cb = fl(tx_uv, {0}); g.cr = fl(tx_uv, {0});
    for (int p = 0; p < 2; p++) {
        g.d_txb_skip_ctx_c[p] = dev<uint8_t>(); g.d_dc_sign_ctx_c[p] = dev<uint8_t>();
        g.d_bits_c[p] = supplied ? dev<uint64_t>() : nullptr;
    }
    g.d_coeff_cost_uv = dev<int32_t>(); g.d_eob_cost_uv = dev<int32_t>();
    return g;
}

static int test_search_walk() {
    // 8x8 with chroma and every gather, nothing supplied; an empty group; 64x64 without chroma, without gathers; 4x4 with everything supplied
    std::vector<svt_hip_md_search_group> gs = {ms_group(3, 3, 5, SVT_TX_8X8, {0, 9, 1}, SVT_TX_4X4, true, false, true),
                                               ms_group(6, 2, 0, SVT_TX_16X16, {0}, SVT_TX_8X8, true, false, true),
                                               ms_group(12, 2, 3, SVT_TX_64X64, {0}, SVT_TX_32X32, false, false, false),
                                               ms_group(0, 40, 2, SVT_TX_4X4, {3, 0}, SVT_TX_4X4, true, true, true)};
    const int ng = (int)gs.size();
    // group 0: 15 survivors; record 600, best_qcoeff / best_dqcoeff 15 * 64 * 4 = 3840; per chroma plane dist 240, eob 30, bits 120, qcoeff and dqcoeff 960
    const size_t g0 = A(600) + 3840 + 3840 + 2 * (240 + A(30) + A(120) + 960 + 960);
    // group 2: 6 survivors; record 240 only
    const size_t g2 = 240;
    // the luma searches, after all groups: group 0: 45 pairs: dist 720, eob 90, bits 360, qcoeff and dqcoeff 45 * 256; group 2: 6 pairs: dist 96,
    // eob 12, bits 48, qcoeff 6 * 4096 (no dqcoeff: nobody asks); group 3: 160 pairs, everything supplied but the bits: 1280
    const size_t lu = 720 + A(90) + A(360) + 2 * 11520 + 96 + A(12) + 48 + 24576 + 1280;
    const size_t want = g0 + g2 + lu;
    CHECK(scratch_bytes_of(md_search_walk, gs.data(), ng) == want);
    Scratch sc(want);
    MdSearchStages st;
    // refusals of the scratch itself
    CHECK(plan_stages(md_search_walk, gs.data(), ng, (void*)nullptr, want, &st) == INVALID);
    CHECK(plan_stages(md_search_walk, gs.data(), ng, (void*)(sc.p + 8), want, &st) == INVALID);
    CHECK(plan_stages(md_search_walk, gs.data(), ng, (void*)sc.p, want - 1, &st) == INVALID);
    CHECK(st.md.empty() && st.flc.empty() && st.tx.fl.empty());
    CHECK(plan_stages(md_search_walk, gs.data(), ng, (void*)sc.p, want, &st) == SVT_HIP_OK);
    CHECK((int)st.md.size() == ng && (int)st.tx.fl.size() == ng && (int)st.tx.cr.size() == ng && (int)st.tx.td.size() == ng);
    CHECK(st.flc.size() == 6 && st.crc.size() == 6);                                      // Cb, Cr of groups 0, 1, 3
    const svt_hip_md_decide_group &M0 = st.md[0], &M2 = st.md[2], &M3 = st.md[3];
    const svt_hip_full_loop_group &CB0 = st.flc[0], &CR0 = st.flc[1];
    std::vector<Piece> v = {{M0.d_luma, 600}, {M0.d_qcoeff[0], 3840}, {M0.d_dqcoeff[0], 3840},
                            {M0.d_dist_cb, 240}, {M0.d_eob_cb, 30}, {M0.d_bits_cb, 120}, {M0.d_qcoeff[1], 960}, {M0.d_dqcoeff[1], 960},
                            {M0.d_dist_cr, 240}, {M0.d_eob_cr, 30}, {M0.d_bits_cr, 120}, {M0.d_qcoeff[2], 960}, {M0.d_dqcoeff[2], 960},
                            {M2.d_luma, 240},
                            {st.tx.fl[0].d_dist, 720}, {st.tx.fl[0].d_eob, 90}, {st.tx.cr[0].d_bits, 360}, {st.tx.fl[0].d_qcoeff, 11520}, {st.tx.fl[0].d_dqcoeff, 11520},
                            {st.tx.fl[2].d_dist, 96}, {st.tx.fl[2].d_eob, 12}, {st.tx.cr[2].d_bits, 48}, {st.tx.fl[2].d_qcoeff, 24576},
                            {st.tx.cr[3].d_bits, 1280}};
    TRY(pieces_ok(v, sc.p, want));
    // the stages hand on what the stage before wrote
    CHECK(st.tx.td[0].d_decision == M0.d_luma && st.tx.td[0].d_best_qcoeff == M0.d_qcoeff[0] && st.tx.td[0].d_best_dqcoeff == M0.d_dqcoeff[0]);
    CHECK(CB0.d_dist == M0.d_dist_cb && CR0.d_dist == M0.d_dist_cr && CB0.d_eob == M0.d_eob_cb && CR0.d_eob == M0.d_eob_cr);
    CHECK(CB0.d_qcoeff == M0.d_qcoeff[1] && CR0.d_dqcoeff == M0.d_dqcoeff[2] && st.crc[0].d_qcoeff == CB0.d_qcoeff && st.crc[1].d_eob == CR0.d_eob);
    CHECK(st.crc[0].d_bits == M0.d_bits_cb && st.crc[1].d_bits == M0.d_bits_cr && st.crc[0].nblocks == 15 && st.crc[0].ntypes == 1);
    CHECK(st.crc[0].d_txb_skip_ctx == gs[0].d_txb_skip_ctx_c[0] && st.crc[1].d_dc_sign_ctx == gs[0].d_dc_sign_ctx_c[1] && st.crc[0].d_coeff_cost == gs[0].d_coeff_cost_uv);
    CHECK(st.tx.fl[2].d_dqcoeff == nullptr && M2.d_dqcoeff[0] == nullptr && M2.d_qcoeff[0] == nullptr && M2.d_dist_cb == nullptr && M2.d_eob_cr == nullptr);
    CHECK(M2.d_qcoeff[1] == nullptr && M2.d_dqcoeff[2] == nullptr);                         // what the caller put into the stage inputs of md is ignored
    // supplied arrays pass through
    CHECK(M3.d_luma == gs[3].luma.d_decision && M3.d_qcoeff[0] == gs[3].luma.d_best_qcoeff && M3.d_dist_cb == gs[3].cb.d_dist && M3.d_bits_cr == gs[3].d_bits_c[1]);
    CHECK(M3.d_dqcoeff[2] == gs[3].cr.d_dqcoeff && st.flc[4].d_dist == gs[3].cb.d_dist);
    // the caller's own members of md are kept
    CHECK(M0.d_decision == gs[0].md.d_decision && M0.d_rate == gs[0].md.d_rate && M0.d_best_pred[1] == gs[0].md.d_best_pred[1] && M0.d_pred[2] == gs[0].md.d_pred[2]);
    // every stage accepts its groups
    const svt_hip_qrows q = good_rows();
    CHECK(full_loop_check(st.tx.fl.data(), ng, SVT_HIP_FLAVOUR_AVX2, q) == SVT_HIP_OK && coeff_rate_check(st.tx.cr.data(), ng) == SVT_HIP_OK);
    CHECK(tx_decide_check(st.tx.td.data(), ng) == SVT_HIP_OK);
    CHECK(full_loop_check(st.flc.data(), 6, SVT_HIP_FLAVOUR_AVX2, q) == SVT_HIP_OK && coeff_rate_check(st.crc.data(), 6) == SVT_HIP_OK);
    CHECK(md_decide_check(st.md.data(), ng) == SVT_HIP_OK);
    // nothing to carve: everything supplied but the luma bits; no groups; only empty groups
    std::vector<svt_hip_md_search_group> one = {gs[3]};
    CHECK(scratch_bytes_of(md_search_walk, one.data(), 1) == 1280);
    CHECK(scratch_bytes_of(md_search_walk, (const svt_hip_md_search_group*)nullptr, 0) == 0);
    std::vector<svt_hip_md_search_group> empty = {gs[1]};
    MdSearchStages se;
    CHECK(scratch_bytes_of(md_search_walk, empty.data(), 1) == 0 && plan_stages(md_search_walk, empty.data(), 1, (void*)nullptr, 0, &se) == SVT_HIP_OK);
    // refusals of the walk: each with a valid neighbour in the list, sizes 0 and a plan that derives nothing usable
    auto bad = [&](const std::function<void(svt_hip_md_search_group&)>& change) {
        std::vector<svt_hip_md_search_group> b = {gs[0], gs[2]};
        change(b[1]);
        MdSearchStages s2;
        return scratch_bytes_of(md_search_walk, b.data(), 2) == 0 && plan_stages(md_search_walk, b.data(), 2, (void*)sc.p, want, &s2) == INVALID;
    };
    CHECK(scratch_bytes_of(md_search_walk, (const svt_hip_md_search_group*)nullptr, 1) == 0);
    CHECK(bad([](svt_hip_md_search_group& g) { g.md.bsize = 13; }));
    CHECK(bad([](svt_hip_md_search_group& g) { g.md.n = 41; }));
    CHECK(bad([](svt_hip_md_search_group& g) { g.md.full_loop_escape = 3; }));
    CHECK(bad([](svt_hip_md_search_group& g) { g.md.ninter = 0; g.md.nintra = 0; }));
    CHECK(bad([](svt_hip_md_search_group& g) { g.luma.fl.tx_types[0] = 9; g.luma.fl.tx_size = SVT_TX_16X16; g.md.bsize = 6; }));      // a list without DCT_DCT
    CHECK(bad([](svt_hip_md_search_group& g) { g.luma.fl.nblocks += 1; }));
    CHECK(bad([](svt_hip_md_search_group& g) { g.luma.fl.tx_size = SVT_TX_32X32; }));       // 1024 coefficients too, but not the 64x64 block's size
    CHECK(bad([](svt_hip_md_search_group& g) { g.use_chroma = 1; g.cb.tx_size = g.cr.tx_size = SVT_TX_16X16; }));      // a 64x64 block's chroma is 32x32
    CHECK(bad([](svt_hip_md_search_group& g) { g.use_chroma = 1; g.cr.ntypes = 2; g.cr.tx_types[1] = 9; }));
    CHECK(bad([](svt_hip_md_search_group& g) { g.use_chroma = 1; g.cb.nblocks -= 1; }));
    CHECK(!bad([](svt_hip_md_search_group& g) { g.md.n = 2; }));                             // (the unchanged pair is accepted)
    return 0;
}

int main() {
    for (int i = 0; i < 8; i++) { g_zbin[i] = 40; g_round[i] = 20; g_quant[i] = 1000; g_shift[i] = 64; g_dequant[i] = 80; }
    TRY(test_decide_check());
    TRY(test_geometry());
    TRY(test_search_walk());
    puts("ok");
    return 0;
}

// csrc/tx_plan.h on the CPU: the invariants of every plan a sweep of shapes accepts (the grid covers the batch and no more, the threads are
// the route's workgroup, a fused route never gets a table its arithmetic cannot take, a 16-byte route never a misaligned group), every
// refusal with its status, and the kernel instantiation, grid and threads of every shape the GPU tests, bench.py and the tools reach
// through svt_hip_txfm.hip, as the routing had them before it moved into the plan (256 compute units).  Plain C++17 (g++), linked with
// csrc/host_err.cpp, built plain and under -fsanitize=address,undefined by tests/test_tx_plan_host.py and run directly.  Exit status 0
// and "ok" when every case holds.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <initializer_list>

#include "../../cidana-svt-av1_amd/csrc/tx_plan.h"

using namespace svthost;

#define CHECK(c) do { if (!(c)) { fprintf(stderr, "%s:%d: %s (last error: %s)\n", __FILE__, __LINE__, #c, svt_hip_last_error()); return 1; } } while (0)
#define TRY(call) do { if (call) { fprintf(stderr, "  from %s:%d\n", __FILE__, __LINE__); return 1; } } while (0)
static const int INVALID = SVT_HIP_ERR_INVALID;
static const int NUM_CU = 256;
static const uint64_t N_MAX = 0x7fffffffu;

// ---- quantiser rows by class: 0 power-of-two quant_shift (the fused kernels' tables), 1 a non-power-of-two quant_shift, 2 a negative entry ----
static const int16_t kZbin[8] = {100, 120}, kRound[8] = {50, 60}, kQuant[8] = {-20000, 12000}, kDequant[8] = {40, 50}, kDequantNeg[8] = {40, -50};
static const int16_t kShift[8] = {16384, 16384}, kShiftOdd[8] = {12345, 16384};
static svt_hip_qrows rows(int cls) { return svt_hip_qrows{kZbin, kRound, kQuant, cls == 1 ? kShiftOdd : kShift, cls == 2 ? kDequantNeg : kDequant}; }

// ---- knob settings: the defaults, then each knob on its own ----
static constexpr TxKnobs kKnobSets[] = {
    {0, 0, 0, 0, 0, 0, 0, 0, 4, 0, -1},        // defaults
    {1, 0, 0, 0, 0, 0, 0, 0, 4, 0, -1},        // no_staged
    {0, 1, 0, 0, 0, 0, 0, 0, 4, 0, -1},        // no_f32p
    {0, 0, 1, 0, 0, 0, 0, 0, 4, 0, -1},        // no_inv_planes
    {0, 0, 0, 1, 0, 0, 0, 0, 4, 0, -1},        // no_enc_staged
    {0, 0, 0, 0, 1, 0, 0, 0, 4, 0, -1},        // no_enc64
    {0, 0, 0, 0, 0, 2, 0, 0, 4, 0, -1},        // f32_wg_per_cu
    {0, 0, 0, 0, 0, 0, 1, 0, 4, 0, -1},        // f32_nt
    {0, 0, 0, 0, 0, 0, 0, 1, 4, 0, -1},        // f32_qmode1
    {0, 0, 0, 0, 0, 0, 0, 0, 4, 1, -1},        // inv32 probes
    {0, 0, 0, 0, 0, 0, 0, 0, 2, 0, -1},
    {0, 0, 0, 0, 0, 0, 0, 0, 4, 8, -1},
    {0, 0, 0, 0, 0, 0, 0, 0, 4, 0, 0},         // frame_single_launch
    {0, 0, 0, 0, 0, 0, 0, 0, 4, 0, 1},
    {0, 0, 0, 0, 0, 0, 0, 0, 4, 0, 2},
};
static const int NKNOBS = (int)(sizeof kKnobSets / sizeof kKnobSets[0]);
static_assert(kKnobSets[0].inv32_waves == kTxKnobDefaults.inv32_waves && kKnobSets[0].frame_single_launch == kTxKnobDefaults.frame_single_launch, "the defaults");

// ---- a plan as the kernel instantiation it launches, "kernel:grid:threads" ----
static const char* tf(bool b) { return b ? "true" : "false"; }
static int render(const TxPlan& p, int ts, char* out, size_t cap) {
    const int w = kTxW[ts], h = kTxH[ts];
    const char* T = p.is16 ? "uint16_t" : "uint8_t";
    char k[160];
    switch (p.route) {
    case TXR_FWD32: snprintf(k, sizeof k, "fwd32_kernel<0,false,false>"); break;
    case TXR_FWD_STAGED: snprintf(k, sizeof k, "fwd_staged_kernel<%d,%d,0>", w, h); break;
    case TXR_FWD_GENERAL: snprintf(k, sizeof k, "fwd_txfm2d_kernel<%d,%d>", w, h); break;
    case TXR_PACK64_NONE: snprintf(k, sizeof k, "none"); break;
    case TXR_PACK64: snprintf(k, sizeof k, "pack64_kernel"); break;
    case TXR_INV32: snprintf(k, sizeof k, "inv32_kernel<%s,%d>", T, p.bd); break;
    case TXR_INV32_PROBE: snprintf(k, sizeof k, "inv32_kernel<uint8_t,8,%d,%d>", p.wv, p.vr); break;
    case TXR_INV_STAGED: snprintf(k, sizeof k, "inv_staged_kernel<%d,%d,%s,%s>", w, h, T, tf(p.t16)); break;
    case TXR_INV_GENERAL:
        if (p.wide) snprintf(k, sizeof k, "inv_txfm2d_add_kernel<%d,%d,uint16_t,true>", w, h);
        else snprintf(k, sizeof k, "inv_txfm2d_add_kernel<%d,%d,%s>", w, h, T);
        break;
    case TXR_QUANTIZE_B: snprintf(k, sizeof k, "quantize_b_kernel<%d>", p.lanes); break;
    case TXR_FQ32: snprintf(k, sizeof k, "fwd32_kernel<1,true,%s,%s,%d>", tf(p.sad), tf(p.nt), p.qmode); break;
    case TXR_FQ32_PLANES: snprintf(k, sizeof k, "fwd32_kernel<%d,true,%s,false,2,%s>", p.inm, tf(p.sad), tf(p.planes)); break;
    case TXR_FQ64: snprintf(k, sizeof k, "fq64_kernel<%s,%d>", T, p.bd); break;
    case TXR_FQ_STAGED: snprintf(k, sizeof k, "fwd_staged_kernel<%d,%d,1,%s>", w, h, T); break;
    case TXR_FQ_GENERAL: snprintf(k, sizeof k, "fwd_quant_generic_kernel<%d,%d,%s>", w, h, T); break;
    case TXR_ENC32: snprintf(k, sizeof k, "enc32_kernel<%s,%d,%s,%s>", T, p.bd, tf(p.keep), tf(p.sad)); break;
    case TXR_ENC4: snprintf(k, sizeof k, "enc4_kernel<%s,%d,%s>", T, p.bd, tf(p.keep)); break;
    case TXR_ENC64: snprintf(k, sizeof k, "enc64_kernel<%s,%d,%s,%s>", T, p.bd, tf(p.keep), tf(p.sad)); break;
    case TXR_ENC_STAGED: snprintf(k, sizeof k, "enc_staged_kernel<%d,%d,%s,%s,%d>", w, h, tf(p.keep), T, p.bd); break;
    case TXR_FWD32_QUANT: snprintf(k, sizeof k, "fwd32_kernel<0,true,false>"); break;
    default: snprintf(k, sizeof k, "route %d", p.route); break;
    }
    return snprintf(out, cap, "%s:%u:%u", k, p.grid, p.threads);
}
static void render_all(const TxPlan& p, const TxPlan* stage, int ts, char* out, size_t cap) {
    if (p.route == TXR_ENC_COMPOSED || p.route == TXR_FWD_THEN_QUANT) {
        const int n = render(stage[0], ts, out, cap);
        out[n] = '+';
        render(stage[1], ts, out + n + 1, cap - (size_t)n - 1);
    } else {
        render(p, ts, out, cap);
    }
}

// ---- the invariants of an accepted plan ----
// the workgroup size and blocks per workgroup of a route, from the kernels' own geometry (TxGeom, StagedGeom, F32_WAVES, E64_WAVES, enc4, quantize_b)
static void route_geometry(const TxPlan& p, int ts, uint32_t& threads, uint32_t& per_wg) {
    const int w = kTxW[ts], h = kTxH[ts], m = w > h ? w : h;
    const uint32_t staged_waves = w * h >= 4096 ? 2 : 4;
    switch (p.route) {
    case TXR_FWD32: case TXR_INV32: case TXR_FQ32: case TXR_FQ32_PLANES: case TXR_ENC32: case TXR_FWD32_QUANT: threads = 256; per_wg = 8; break;
    case TXR_INV32_PROBE: threads = 64u * (uint32_t)p.wv; per_wg = 2u * (uint32_t)p.wv; break;
    case TXR_FWD_STAGED: case TXR_INV_STAGED: case TXR_FQ_STAGED: case TXR_ENC_STAGED: threads = 64 * staged_waves; per_wg = staged_waves * (uint32_t)(64 / m); break;
    case TXR_FQ64: case TXR_ENC64: threads = 128; per_wg = 4; break;
    case TXR_ENC4: threads = 256; per_wg = 256; break;
    case TXR_PACK64: threads = 256; per_wg = 1; break;
    case TXR_QUANTIZE_B: threads = 256; per_wg = 4u * (uint32_t)(64 / p.lanes); break;
    default: threads = 256; per_wg = 4u * (uint32_t)(64 / m); break;      // the general kernels
    }
}
static int fail(const char* entry, int ts, uint64_t n, const TxPlan& p, const char* what) {
    fprintf(stderr, "%s: tx_size %d, %llu blocks -> route %d, grid %u x %u threads, %u per workgroup: %s\n", entry, ts, (unsigned long long)n, p.route, p.grid, p.threads,
            p.per_wg, what);
    return 1;
}
#define HOLDS(c) do { if (!(c)) return fail(entry, ts, n, p, #c); } while (0)
static int check_launch(const char* entry, const TxPlan& p, int ts, uint64_t n) {
    if (p.route == TXR_PACK64_NONE) return 0;
    uint32_t threads, per_wg;
    route_geometry(p, ts, threads, per_wg);
    HOLDS(p.threads == threads && p.per_wg == per_wg);
    HOLDS(p.grid >= 1);
    if (p.grid_capped) {
        HOLDS(p.route == TXR_FQ32 && (uint64_t)p.grid * per_wg < n);
    } else {
        HOLDS((uint64_t)p.grid * per_wg >= n && n > (uint64_t)(p.grid - 1) * per_wg);
    }
    return 0;
}
// n = 1, one block short of a workgroup, a full workgroup, one block more, and the largest batch
template <typename Plan, typename Check>
static int over_batches(Plan plan, Check check) {
    TxPlan p;
    if (plan((uint64_t)1, p)) return 0;      // refused: the refusals are the next part's
    // (a composed route has two launches, each with its own blocks per workgroup: every one a kernel of this family has)
    const uint64_t per = p.per_wg, ns[5] = {1, per - 1, per, per + 1, N_MAX};
    const uint64_t all[] = {1, 2, 3, 4, 5, 7, 8, 9, 15, 16, 17, 31, 32, 33, 63, 64, 65, 255, 256, 257, N_MAX};
    const int count = per ? 5 : (int)(sizeof all / sizeof all[0]);
    for (int i = 0; i < count; i++) {
        const uint64_t n = per ? ns[i] : all[i];
        if (n == 0) continue;
        if (plan(n, p)) { fprintf(stderr, "a plan accepted at 1 block is refused at %llu: %s\n", (unsigned long long)n, svt_hip_last_error()); return 1; }
        TRY(check(p, n));
    }
    return 0;
}
static const int kTypes[3] = {SVT_DCT_DCT, SVT_IDTX, 1 /* ADST_DCT */};

static int sweep() {
    for (int ts = 0; ts < SVT_TX_SIZES_ALL; ts++) {
        const int w = kTxW[ts], h = kTxH[ts];
        for (int tt : kTypes) {
            if (!tx_type_ok(ts, tt)) continue;
            for (int kn = 0; kn < NKNOBS; kn++) {
                const TxKnobs& k = kKnobSets[kn];
                // forward transform: dense and strided, aligned and not
                for (int bd : {8, 10}) for (int dense = 0; dense < 2; dense++) for (int al = 0; al < 2; al++) {
                    TRY(over_batches([&](uint64_t n, TxPlan& p) { return fwd_plan(ts, tt, bd, (uint32_t)(dense ? w : w + 8), (size_t)(dense ? w * h : 2 * w * h + 64), n, al != 0, k, p); },
                                     [&](const TxPlan& p, uint64_t n) {
                                         const char* entry = "fwd";
                                         HOLDS(p.route == TXR_FWD32 || p.route == TXR_FWD_STAGED || p.route == TXR_FWD_GENERAL);
                                         HOLDS(p.route == TXR_FWD_GENERAL || (dense && al));
                                         return check_launch(entry, p, ts, n);
                                     }));
                }
                // inverse: dense / offsets, 8- and 16-bit destinations, bd 8 / 10 / 12
                for (int bd : {8, 10, 12}) for (int is16 = 0; is16 < 2; is16++) for (int offs = 0; offs < 2; offs++) for (int al = 0; al < 4; al++) {
                    if (!is16 && bd != 8) continue;
                    TRY(over_batches([&](uint64_t n, TxPlan& p) { return inv_plan(ts, tt, bd, is16, w, (size_t)w * h, offs != 0, n, (al & 1) != 0, (al & 2) != 0, k, p); },
                                     [&](const TxPlan& p, uint64_t n) {
                                         const char* entry = "inv";
                                         HOLDS(p.route == TXR_INV32 || p.route == TXR_INV32_PROBE || p.route == TXR_INV_STAGED || p.route == TXR_INV_GENERAL);
                                         HOLDS(p.route == TXR_INV_GENERAL || (al & 1));                         // 16-byte coefficient loads
                                         HOLDS(p.route != TXR_INV_STAGED || offs || (al & 2));                    // dense destinations too
                                         HOLDS(bd <= 10 || (p.route == TXR_INV_GENERAL && p.wide));               // bd 12: the 64-bit sums only
                                         HOLDS(p.wide == (bd > 10));
                                         return check_launch(entry, p, ts, n);
                                     }));
                }
                for (int q = 0; q < 3; q++) {
                    const svt_hip_qrows qr = rows(q);
                    // forward + quantise on planes and dense batches
                    for (int is16 = 0; is16 < 2; is16++) for (int xy = 0; xy < 2; xy++) for (int sad = 0; sad < 2; sad++) for (int en = 0; en < 2; en++) for (int al = 0; al < 4; al++) {
                        TRY(over_batches([&](uint64_t n, TxPlan& p) { return fq_planes_plan(ts, tt, is16, is16 ? 10 : 8, 1920, 1984, xy != 0, sad != 0, en != 0, qr, n, (al & 1) != 0, (al & 2) != 0, k, p); },
                                         [&](const TxPlan& p, uint64_t n) {
                                             const char* entry = "fq_planes";
                                             HOLDS(q != 2);                                                       // a negative table is refused
                                             HOLDS(p.route == TXR_FQ32_PLANES || p.route == TXR_FQ64 || p.route == TXR_FQ_STAGED || p.route == TXR_FQ_GENERAL);
                                             HOLDS(p.route == TXR_FQ_GENERAL || (q == 0 && (al & 2)));            // fused: fast table, 16-byte coefficient stores
                                             HOLDS(p.route == TXR_FQ_GENERAL || p.route == TXR_FQ32_PLANES || xy || (al & 1));
                                             HOLDS(!en || p.route == TXR_FQ_STAGED || p.route == TXR_FQ_GENERAL);  // the kernels that form the energy
                                             HOLDS(xy ? p.src_stride == 1920 && p.pred_stride == 1984 : p.route == TXR_FQ_STAGED || p.route == TXR_FQ32_PLANES || p.src_stride == (uint32_t)w);
                                             return check_launch(entry, p, ts, n);
                                         }));
                    }
                    // the headline call
                    for (int sad = 0; sad < 2; sad++) for (int al = 0; al < 4; al++) {
                        TRY(over_batches([&](uint64_t n, TxPlan& p) { return fq_sad_plan(ts, tt, sad != 0, qr, n, (al & 1) != 0, (al & 2) != 0, k, NUM_CU, p); },
                                         [&](const TxPlan& p, uint64_t n) {
                                             const char* entry = "fq_sad";
                                             HOLDS(q != 2);
                                             HOLDS((p.route == TXR_FQ32) == tx_is_32x32_pair(ts, tt));
                                             HOLDS(p.route != TXR_FQ32 || (p.qmode == 2 ? q == 0 && !k.f32_qmode1 : q == 1 || k.f32_qmode1));
                                             HOLDS(p.route != TXR_FQ32 || (p.sad == (sad != 0) && p.nt == (k.f32_nt != 0)));
                                             HOLDS(!p.grid_capped || k.f32_wg_per_cu > 0);
                                             return check_launch(entry, p, ts, n);
                                         }));
                    }
                    // encode pass: dense and planes, every presence combination
                    for (int is16 = 0; is16 < 2; is16++) for (int xy = 0; xy < 2; xy++) for (int pres = 0; pres < 8; pres++) for (int al = 0; al < 8; al++) {
                        const bool co = pres & 1, dq = pres & 2, sad = pres & 4;
                        TxPlan stage[2];
                        TRY(over_batches([&](uint64_t n, TxPlan& p) {
                                             return encode_recon_plan(ts, tt, is16, is16 ? 10 : 8, xy != 0, co, dq, sad, false, qr, n, EncAligned{(al & 1) != 0, (al & 4) != 0, (al & 2) != 0, (al & 2) != 0}, k,
                                                                      NUM_CU, p, stage);
                                         },
                                         [&](const TxPlan& p, uint64_t n) {
                                             const char* entry = "encode_recon";
                                             if (p.route == TXR_ENC_COMPOSED) {
                                                 HOLDS(co && dq && !xy && !is16 && q != 2);
                                                 HOLDS(stage[0].route == TXR_FQ_GENERAL || stage[0].route == TXR_FQ32 || ((al & 1) && (al & 2)));      // each stage by its own groups
                                                 HOLDS(stage[1].route == TXR_INV_GENERAL || ((al & 2) && (stage[1].route == TXR_INV32 || stage[1].route == TXR_INV32_PROBE || (al & 4))));
                                                 TRY(check_launch("encode_recon stage 0", stage[0], ts, n));
                                                 return check_launch("encode_recon stage 1", stage[1], ts, n);
                                             }
                                             HOLDS(p.route == TXR_ENC32 || p.route == TXR_ENC4 || p.route == TXR_ENC64 || p.route == TXR_ENC_STAGED);
                                             HOLDS(co == dq && p.keep == co);                                      // both or neither
                                             HOLDS(p.route == TXR_ENC4 ? p.fast == (q == 0) : q == 0);
                                             HOLDS((p.route != TXR_ENC64 && p.route != TXR_ENC_STAGED) || ((al & 2) && (xy || (al & 5) == 5)));
                                             return check_launch(entry, p, ts, n);
                                         }));
                    }
                    // residual -> coefficients -> quantised
                    for (int bd : {8, 10}) for (int al = 0; al < 4; al++) {
                        TxPlan stage[2];
                        TRY(over_batches([&](uint64_t n, TxPlan& p) { return fwd_quant_plan(ts, tt, bd, qr, n, (al & 1) != 0, (al & 2) != 0, k, p, stage); },
                                         [&](const TxPlan& p, uint64_t n) {
                                             const char* entry = "fwd_quant";
                                             if (p.route == TXR_FWD_THEN_QUANT) {
                                                 HOLDS(w != 64 && h != 64 && stage[1].route == TXR_QUANTIZE_B && stage[1].lanes == (w * h / 4 >= 64 ? 64 : w * h / 4));
                                                 TRY(check_launch("fwd_quant stage 0", stage[0], ts, n));
                                                 return check_launch("fwd_quant stage 1", stage[1], ts, n);
                                             }
                                             HOLDS(p.route == TXR_FWD32_QUANT && bd == 8 && q == 0 && (al & 1));
                                             return check_launch(entry, p, ts, n);
                                         }));
                    }
                }
            }
        }
        TRY(over_batches([&](uint64_t n, TxPlan& p) { return pack64_plan(ts, n, p); },
                         [&](const TxPlan& p, uint64_t n) {
                             const char* entry = "pack64";
                             HOLDS((p.route == TXR_PACK64) == (w == 64 || h == 64));
                             return check_launch(entry, p, ts, n);
                         }));
    }
    for (size_t nc = 16; nc <= 4096; nc += 16) for (int ls = 0; ls < 3; ls++)
        TRY(over_batches([&](uint64_t n, TxPlan& p) { return quantize_plan(nc, ls, rows(1), n, p); },
                         [&](const TxPlan& p, uint64_t n) {
                             const char* entry = "quantize_b"; const int ts = 0;
                             HOLDS(p.lanes == 4 || p.lanes == 8 || p.lanes == 16 || p.lanes == 32 || p.lanes == 64);
                             HOLDS((size_t)p.lanes * 4 == nc || p.lanes == 64);
                             return check_launch(entry, p, ts, n);
                         }));
    return 0;
}

// ---- refusals ----
static int refused(int rc, int status, const char* text, int line) {
    if (rc == status && strstr(svt_hip_last_error(), text)) return 0;
    fprintf(stderr, "%s:%d: status %d \"%s\", expected %d \"%s\"\n", __FILE__, line, rc, rc ? svt_hip_last_error() : "", status, text);
    return 1;
}
#define REFUSED(call, status, text) TRY(refused(call, status, text, __LINE__))
static int refusals() {
    const TxKnobs k = kTxKnobDefaults;
    const svt_hip_qrows f = rows(0), odd = rows(1), neg = rows(2);
    TxPlan p, st[2];
    // forward
    REFUSED(fwd_plan(19, 0, 8, 4, 16, 1, true, k, p), INVALID, "not defined by the reference");
    REFUSED(fwd_plan(SVT_TX_64X64, SVT_IDTX, 8, 64, 4096, 1, true, k, p), INVALID, "not defined by the reference");
    REFUSED(fwd_plan(SVT_TX_32X32, 1, 8, 32, 1024, 1, true, k, p), INVALID, "not defined by the reference");
    REFUSED(fwd_plan(SVT_TX_8X8, 0, 12, 8, 64, 1, true, k, p), INVALID, "bit depth 12");
    REFUSED(fwd_plan(SVT_TX_8X8, 0, 8, 8, 64, N_MAX + 1, true, k, p), INVALID, "nblocks too large");
    // 64-point packing
    REFUSED(pack64_plan(-1, 1, p), INVALID, "bad argument");
    REFUSED(pack64_plan(SVT_TX_SIZES_ALL, 1, p), INVALID, "bad argument");
    // inverse
    REFUSED(inv_plan(SVT_TX_16X64, SVT_IDTX, 8, 0, 16, 1024, false, 1, true, true, k, p), INVALID, "not defined by the reference");
    REFUSED(inv_plan(SVT_TX_8X8, 0, 9, 1, 8, 64, false, 1, true, true, k, p), INVALID, "bit depth 9");
    REFUSED(inv_plan(SVT_TX_8X8, 0, 10, 0, 8, 64, false, 1, true, true, k, p), INVALID, "8-bit destination needs bd = 8");
    {
        TxKnobs probe = k;
        probe.inv32_var = 3;
        REFUSED(inv_plan(SVT_TX_32X32, 0, 8, 0, 32, 1024, false, 1, true, true, probe, p), INVALID, "inv32 probe variant not built");
        probe.inv32_waves = 2; probe.inv32_var = 1;
        REFUSED(inv_plan(SVT_TX_32X32, 0, 8, 0, 32, 1024, false, 1, true, true, probe, p), INVALID, "inv32 probe variant not built");
    }
    // quantiser
    REFUSED(quantize_plan(8, 0, f, 1, p), INVALID, "n_coeffs 8");
    REFUSED(quantize_plan(4112, 0, f, 1, p), INVALID, "n_coeffs 4112");
    REFUSED(quantize_plan(24, 0, f, 1, p), INVALID, "n_coeffs 24");
    REFUSED(quantize_plan(64, 3, f, 1, p), INVALID, "log_scale 3");
    REFUSED(quantize_plan(64, -1, f, 1, p), INVALID, "log_scale -1");
    // forward + quantise on planes
    REFUSED(fq_planes_plan(SVT_TX_64X32, SVT_IDTX, 0, 8, 64, 64, true, false, false, f, 1, true, true, k, p), INVALID, "not defined by the reference");
    REFUSED(fq_planes_plan(SVT_TX_8X8, 0, 1, 8, 64, 64, true, false, false, f, 1, true, true, k, p), INVALID, "bit depth 8 (16-bit planes)");
    REFUSED(fq_planes_plan(SVT_TX_8X8, 0, 0, 10, 64, 64, true, false, false, f, 1, true, true, k, p), INVALID, "bit depth 10 (8-bit planes)");
    REFUSED(fq_planes_plan(SVT_TX_8X8, 0, 1, 10, 64, 64, true, true, false, f, 1, true, true, k, p), INVALID, "SAD is defined for 8-bit planes only");
    REFUSED(fq_planes_plan(SVT_TX_8X8, 0, 0, 8, 64, 64, true, false, false, f, N_MAX + 1, true, true, k, p), INVALID, "nblocks too large");
    REFUSED(fq_planes_plan(SVT_TX_8X8, 0, 0, 8, 64, 64, true, false, false, neg, 1, true, true, k, p), INVALID, "negative quantizer table entry");
    // the headline call: its own two refusals, and the planes call's for the sizes it hands over
    REFUSED(fq_sad_plan(SVT_TX_32X32, 0, true, f, N_MAX + 1, true, true, k, NUM_CU, p), INVALID, "nblocks too large");
    REFUSED(fq_sad_plan(SVT_TX_32X32, SVT_IDTX, true, neg, 1, true, true, k, NUM_CU, p), INVALID, "negative quantizer table entry");
    REFUSED(fq_sad_plan(SVT_TX_32X32, 1, true, f, 1, true, true, k, NUM_CU, p), INVALID, "not defined by the reference");
    REFUSED(fq_sad_plan(SVT_TX_16X16, 0, true, neg, 1, true, true, k, NUM_CU, p), INVALID, "negative quantizer table entry");
    REFUSED(fq_sad_plan(SVT_TX_16X16, 0, true, f, N_MAX + 1, true, true, k, NUM_CU, p), INVALID, "nblocks too large");
    // encode pass
    REFUSED(encode_recon_plan(SVT_TX_64X64, 1, 0, 8, true, false, false, false, false, f, 1, EncAligned{true, true, true, true}, k, NUM_CU, p, st), INVALID, "not defined by the reference");
    REFUSED(encode_recon_plan(SVT_TX_8X8, 0, 0, 8, true, false, false, false, true, f, 1, EncAligned{true, true, true, true}, k, NUM_CU, p, st), INVALID, "d_recon must not alias d_src");
    REFUSED(encode_recon_plan(SVT_TX_8X8, 0, 1, 8, true, false, false, false, false, f, 1, EncAligned{true, true, true, true}, k, NUM_CU, p, st), INVALID, "bit depth 8 (16-bit samples)");
    REFUSED(encode_recon_plan(SVT_TX_8X8, 0, 0, 10, true, false, false, false, false, f, 1, EncAligned{true, true, true, true}, k, NUM_CU, p, st), INVALID, "bit depth 10 (8-bit samples)");
    REFUSED(encode_recon_plan(SVT_TX_8X8, 0, 1, 10, true, false, false, true, false, f, 1, EncAligned{true, true, true, true}, k, NUM_CU, p, st), INVALID, "SAD is defined for 8-bit planes only");
    REFUSED(encode_recon_plan(SVT_TX_8X8, 0, 0, 8, true, false, false, false, false, f, N_MAX + 1, EncAligned{true, true, true, true}, k, NUM_CU, p, st), INVALID, "nblocks too large");
    REFUSED(encode_recon_plan(SVT_TX_8X8, 0, 0, 8, false, false, false, false, false, odd, 1, EncAligned{true, true, true, true}, k, NUM_CU, p, st), INVALID, "needs d_coeff and d_dqcoeff");
    REFUSED(encode_recon_plan(SVT_TX_8X8, 0, 0, 8, false, true, false, false, false, f, 1, EncAligned{true, true, true, true}, k, NUM_CU, p, st), INVALID, "needs d_coeff and d_dqcoeff");
    REFUSED(encode_recon_plan(SVT_TX_8X8, 0, 0, 8, true, true, true, false, false, odd, 1, EncAligned{true, true, true, true}, k, NUM_CU, p, st), INVALID, "no fused kernel for this case");
    REFUSED(encode_recon_plan(SVT_TX_8X8, 0, 1, 10, false, true, true, false, false, f, 1, EncAligned{true, true, false, false}, k, NUM_CU, p, st), INVALID, "no fused kernel for this case");
    REFUSED(encode_recon_plan(SVT_TX_8X8, 0, 0, 8, false, true, true, false, false, neg, 1, EncAligned{true, true, true, true}, k, NUM_CU, p, st), INVALID, "negative quantizer table entry");
    // residual -> quantised
    REFUSED(fwd_quant_plan(SVT_TX_32X8, 1, 8, f, 1, true, true, k, p, st), INVALID, "not defined by the reference");
    REFUSED(fwd_quant_plan(SVT_TX_64X64, 0, 8, f, 1, true, true, k, p, st), SVT_HIP_ERR_UNSUPPORTED, "use svt_hip_fwd_quant_planes_batch for 64-pt sizes");
    REFUSED(fwd_quant_plan(SVT_TX_16X64, 0, 8, f, 1, true, true, k, p, st), SVT_HIP_ERR_UNSUPPORTED, "use svt_hip_fwd_quant_planes_batch for 64-pt sizes");
    REFUSED(fwd_quant_plan(SVT_TX_8X8, 0, 12, f, 1, true, true, k, p, st), INVALID, "bit depth 12");
    // the four entry points that cast nblocks unchecked before: one past the bound, and a count that wrapped to 1
    for (uint64_t n : {(uint64_t)0x80000000u, ((uint64_t)1 << 32) + 1}) {
        REFUSED(inv_plan(SVT_TX_8X8, 0, 8, 0, 8, 64, false, n, true, true, k, p), INVALID, "nblocks too large");
        REFUSED(quantize_plan(64, 0, f, n, p), INVALID, "nblocks too large");
        REFUSED(pack64_plan(SVT_TX_64X64, n, p), INVALID, "nblocks too large");
        REFUSED(pack64_plan(SVT_TX_8X8, n, p), INVALID, "nblocks too large");
        REFUSED(fwd_quant_plan(SVT_TX_32X32, 0, 8, f, n, true, true, k, p, st), INVALID, "nblocks too large");
        REFUSED(fwd_quant_plan(SVT_TX_8X8, 0, 8, f, n, true, true, k, p, st), INVALID, "nblocks too large");
    }
    // the frame call's groups
    char mem[64];
    svt_hip_frame_group g = {};
    g.d_src = mem; g.d_pred = mem + 16; g.d_recon = mem + 32; g.d_xy = (const uint32_t*)mem; g.d_iscan = (const int16_t*)mem; g.d_qcoeff = (int32_t*)mem; g.d_eob = (uint16_t*)mem;
    g.nblocks = 1; g.tx_size = SVT_TX_8X8; g.tx_type = 0;
    CHECK(frame_groups_check(&g, 1, k) == SVT_HIP_OK && frame_groups_check(nullptr, 0, k) == SVT_HIP_OK);
    REFUSED(frame_groups_check(nullptr, 1, k), INVALID, "NULL group list");
    REFUSED(frame_groups_check(&g, -1, k), INVALID, "NULL group list");
    REFUSED(frame_groups_check(&g, 257, k), INVALID, "more than 256 groups");
    { svt_hip_frame_group b = g; b.d_eob = nullptr; REFUSED(frame_groups_check(&b, 1, k), INVALID, "group 0: NULL member"); }
    { svt_hip_frame_group b = g; b.d_xy = nullptr; REFUSED(frame_groups_check(&b, 1, k), INVALID, "group 0: NULL member"); }
    { svt_hip_frame_group b = g; b.tx_size = SVT_TX_64X64; b.tx_type = SVT_IDTX; REFUSED(frame_groups_check(&b, 1, k), INVALID, "group 0: tx_size 4 / tx_type 9"); }
    { svt_hip_frame_group b = g; b.d_coeff = (int32_t*)mem; REFUSED(frame_groups_check(&b, 1, k), INVALID, "d_coeff and d_dqcoeff go together"); }
    {
        TxKnobs two_stage = k;
        two_stage.no_enc_staged = 1;
        svt_hip_frame_group b = g;
        b.tx_size = SVT_TX_4X4;
        REFUSED(frame_groups_check(&b, 1, two_stage), INVALID, "4x4 groups take the two-stage path");
        b.nblocks = 0;      // an empty group is not looked at
        CHECK(frame_groups_check(&b, 1, two_stage) == SVT_HIP_OK);
    }
    return 0;
}

// ---- the frame call ----
struct FrameGroupIn { int ts, tt; uint32_t n; int co, alias, qal; };
static char g_mem[64];
static int make_groups(const FrameGroupIn* in, int n, svt_hip_frame_group* out) {
    for (int i = 0; i < n; i++) {
        svt_hip_frame_group g = {};
        g.d_src = g_mem; g.d_pred = g_mem + 16; g.d_recon = in[i].alias ? (void*)g_mem : (void*)(g_mem + 32);
        g.d_xy = (const uint32_t*)g_mem; g.d_iscan = (const int16_t*)g_mem; g.d_eob = (uint16_t*)g_mem;
        g.d_qcoeff = (int32_t*)(((uintptr_t)g_mem + 15) / 16 * 16 + (in[i].qal ? 0 : 4));
        if (in[i].co) g.d_coeff = g.d_dqcoeff = (int32_t*)g_mem;
        g.nblocks = in[i].n; g.tx_size = in[i].ts; g.tx_type = in[i].tt;
        out[i] = g;
    }
    return n;
}
static int frame_invariants() {
    static FramePlan fp;
    svt_hip_frame_group gr[19];
    // every size in one call, below and above the two thresholds
    for (uint32_t scale : {1u, 64u, 4096u}) for (int kn = 0; kn < NKNOBS; kn++) for (int q = 0; q < 3; q++) for (int var = 0; var < 4; var++) {
        FrameGroupIn in[19];
        uint64_t pixels = 0;
        for (int ts = 0; ts < 19; ts++) {
            in[ts] = FrameGroupIn{ts, 0, scale * (uint32_t)(ts + 1) * 17u, var == 1 && ts == 7, var == 2 && ts == 3, !(var == 3 && ts == 18)};
            pixels += (uint64_t)in[ts].n * (uint64_t)(kTxW[ts] * kTxH[ts]);
        }
        make_groups(in, 19, gr);
        const TxKnobs& k = kKnobSets[kn];
        frame_plan(gr, 19, 0, 8, rows(q), k, fp);
        const int mode = k.frame_single_launch >= 0 ? k.frame_single_launch : (pixels <= kFrameOneLaunchMaxPixels ? 1 : (pixels <= kFrameClassLaunchMaxPixels ? 2 : 0));
        CHECK(fp.mode == (mode == 1 ? 2 : mode));                       // non-square sizes: never the one launch
        CHECK(fp.tables == (mode > 0 && q == 0 && var == 0));
        for (int ts = 0; ts < 19 && fp.tables; ts++) {
            const uint32_t per = frame_blocks_per_wg(ts);
            CHECK(fp.g[ts].table == tx_class(ts) && fp.g[ts].log_scale == tx_log_scale(ts));
            CHECK((uint64_t)fp.g[ts].wgs * per >= in[ts].n && in[ts].n > (uint64_t)(fp.g[ts].wgs - 1) * per);
        }
        frame_plan(gr, 19, 1, 8, rows(q), k, fp);                        // a depth the fused bodies are not built for
        CHECK(!fp.tables);
    }
    // the square sizes alone take the one launch up to 2^25 pixel passes, exactly
    for (uint32_t n64 : {8192u, 8193u, 65536u, 65537u}) {
        const FrameGroupIn in[2] = {{SVT_TX_64X64, 0, n64, 0, 0, 1}, {SVT_TX_4X4, 0, 0, 0, 0, 1}};
        make_groups(in, 2, gr);
        frame_plan(gr, 2, 0, 8, rows(0), kTxKnobDefaults, fp);
        CHECK(fp.mode == (n64 <= 8192 ? FRAME_ONE_LAUNCH : (n64 <= 65536 ? FRAME_BY_CLASS : FRAME_FAN_OUT)));
        CHECK(fp.tables == (fp.mode != FRAME_FAN_OUT) && (!fp.tables || fp.g[0].table == (fp.mode == FRAME_ONE_LAUNCH ? kFrameOneLaunchTable : 2)));
    }
    // a class with more groups than a launch holds sends the call to the fan-out
    {
        static svt_hip_frame_group many[kFrameMaxGroups + 1];
        FrameGroupIn in[kFrameMaxGroups + 1];
        for (int i = 0; i <= kFrameMaxGroups; i++) in[i] = FrameGroupIn{SVT_TX_8X8, i % 16, 100, 0, 0, 1};
        make_groups(in, kFrameMaxGroups + 1, many);
        frame_plan(many, kFrameMaxGroups, 0, 8, rows(0), kTxKnobDefaults, fp);
        CHECK(fp.tables);
        frame_plan(many, kFrameMaxGroups + 1, 0, 8, rows(0), kTxKnobDefaults, fp);
        CHECK(!fp.tables);
    }
    return 0;
}

// ---- the pinned tables: what the routing did before it moved into the plan ----
// From a throw-away build of the commit before this header that printed, at every launch site of svt_hip_txfm.hip, the kernel instantiation
// with its grid and threads, and at every entry point the shape that reached it; run under tests/test_gpu_parity.py, test_gpu_variants.py,
// test_gpu_encode_recon.py, test_gpu_frame_api.py, test_gpu_boundary.py, test_gpu_pins.py, bench.py, tools/bench_kernels.py, bench_frame.py,
// bench_c5.py and ab_kernels.py on a 256-CU device.  Each distinct shape once: the transform types that route alike (DCT_DCT, IDTX, any other)
// once, strides that only ride along once, and of the batch sizes the smallest and the largest.
// Reached by none of those callers; each has a row from the same print and, where it has a reference, a GPU parity case of
// blocks_per_wg + 1 blocks with the knob, table or operand that selects it (tests/test_gpu_parity.py, tests/test_gpu_encode_recon.py):
//   fwd_txfm2d_kernel (TXR_FWD_GENERAL)                 no_staged, 8x8, 33 blocks                    test_fwd_txfm2d_general_kernel
//   fwd32_kernel<1,true,SAD,NT,QMODE> but <true,false,*>  no d_sad, f32_nt, a non-power-of-two table, 9 blocks  test_fused_32x32_variants
//   fwd32_kernel<1,true,true,false,2,true>              8-bit planes, d_sad, no d_energy, 9 blocks   test_fwd_quant_planes_32x32_with_sad
//   fwd32_kernel<2,true,false,false,2,false>            dense 10-bit batch (no origin table), 9 blocks  test_fwd_quant_planes_32x32_dense_10bit
//   inv32_kernel<uint8_t,8,2,0> and <uint8_t,8,4,8>     inv32_waves / inv32_var, 5 and 9 blocks       test_inv32_probe_variants_that_compute
//   inv32_kernel<uint8_t,8,4,1|2|4|5>                   probes that leave a step out: no reference, rows only (tools/tune_inv32.py times them)
//   enc32_kernel<uint8_t,8,true,false>                  d_coeff without d_sad, 9 blocks              test_encode_recon_32x32_keeps_coefficients_without_the_sad
//   enc4_kernel<uint16_t,10,true>                       10-bit planes with d_coeff, 257 blocks       test_encode_recon_4x4_10bit_keeps_coefficients
// Built and reached by no shape at all: enc64_kernel<uint16_t,10,false,true> (a SAD of 16-bit samples is refused), enc_staged_kernel<4,4,..> and
// <32,32,..> and fwd_staged_kernel<4,4,1,..> (enc4 / enc32, the composed route and the general kernel take those sizes).
// flags: 1 origin table / offsets, 2 d_coeff, 4 d_dqcoeff, 8 d_sad, 16 d_energy.  al: bit 0 the first pointer group of the plan's arguments, bit 1
// the second, bit 2 the third; of the encode pass bit 0 d_src, d_pred and d_recon, bit 1 the coefficient buffers, bit 2 d_recon alone.  q: the class of the quantiser rows (rows()).  kn: index into kPinKnobs.
enum Entry { E_FWD, E_PACK64, E_INV, E_QUANT, E_FQSAD, E_FQP, E_ENC, E_FWDQ };
struct Pin { int entry, ts, tt, bd, is16; uint32_t s0, s1; size_t pitch; int flags; uint64_t n; int al, q, kn; const char* expect; };
struct FramePin { int is16, bd, q, kn; const char* groups; const char* expect; };
#include "tx_plan_pins.h"

static int pinned() {
    for (const Pin& r : kPins) {
        const TxKnobs& k = kPinKnobs[r.kn];
        const svt_hip_qrows q = rows(r.q);
        const bool a0 = r.al & 1, a1 = r.al & 2, a2 = r.al & 4, xy = r.flags & 1, co = r.flags & 2, dq = r.flags & 4, sad = r.flags & 8, en = r.flags & 16;
        TxPlan p, stage[2];
        int rc = -1;
        switch (r.entry) {
        case E_FWD: rc = fwd_plan(r.ts, r.tt, r.bd, r.s0, r.pitch, r.n, a0, k, p); break;
        case E_PACK64: rc = pack64_plan(r.ts, r.n, p); break;
        case E_INV: rc = inv_plan(r.ts, r.tt, r.bd, r.is16, (int32_t)r.s0, r.pitch, xy, r.n, a0, a1, k, p); break;
        case E_QUANT: rc = quantize_plan(r.pitch, r.bd /* log_scale */, q, r.n, p); break;
        case E_FQSAD: rc = fq_sad_plan(r.ts, r.tt, sad, q, r.n, a0, a1, k, NUM_CU, p); break;
        case E_FQP: rc = fq_planes_plan(r.ts, r.tt, r.is16, r.bd, r.s0, r.s1, xy, sad, en, q, r.n, a0, a1, k, p); break;
        case E_ENC: rc = encode_recon_plan(r.ts, r.tt, r.is16, r.bd, xy, co, dq, sad, false, q, r.n, EncAligned{a0 || !a2, a2, a1, a1}, k, NUM_CU, p, stage); break;
        case E_FWDQ: rc = fwd_quant_plan(r.ts, r.tt, r.bd, q, r.n, a0, a1, k, p, stage); break;
        }
        char got[400];
        if (rc) snprintf(got, sizeof got, "refused: %s", svt_hip_last_error());
        else render_all(p, stage, r.entry == E_QUANT || r.entry == E_PACK64 ? (r.entry == E_PACK64 ? r.ts : 0) : r.ts, got, sizeof got);
        if (strcmp(got, r.expect)) {
            fprintf(stderr, "pinned row %d (entry %d, tx_size %d, type %d, %llu blocks): %s, expected %s\n", (int)(&r - kPins), r.entry, r.ts, r.tt, (unsigned long long)r.n, got, r.expect);
            return 1;
        }
    }
    static FramePlan fp;
    for (const FramePin& r : kFramePins) {
        FrameGroupIn in[256];
        static svt_hip_frame_group gr[256];
        int n = 0, used = 0;
        for (const char* s = r.groups; n < 256 && sscanf(s, " %d:%d:%u:%d:%d:%d%n", &in[n].ts, &in[n].tt, &in[n].n, &in[n].co, &in[n].alias, &in[n].qal, &used) == 6; s += used) n++;
        make_groups(in, n, gr);
        frame_plan(gr, n, r.is16, r.bd, rows(r.q), kPinKnobs[r.kn], fp);
        char got[8192];
        int len = snprintf(got, sizeof got, "%s mode %d", fp.tables ? "tables" : "fanout", fp.mode);
        for (int i = 0; i < n && fp.tables; i++) len += snprintf(got + len, sizeof got - (size_t)len, " %d:%d:%u", in[i].ts, fp.g[i].table, fp.g[i].wgs);
        if (strcmp(got, r.expect)) {
            fprintf(stderr, "pinned frame row %d: %s, expected %s\n", (int)(&r - kFramePins), got, r.expect);
            return 1;
        }
    }
    return 0;
}

int main() {
    TRY(sweep());
    TRY(refusals());
    TRY(frame_invariants());
    TRY(pinned());
    printf("ok\n");
    return 0;
}

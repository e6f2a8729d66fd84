// ois_plan.h — the open-loop intra search of one (block size, candidate list) group, planned on the host: everything that follows from
// the list and the knobs without a device pointer, derived once.  svt_hip_intra.hip checks, plans, then enqueues from the plan.
// Plain C++17, no HIP header: a CPU program can include it (tests/c/ois_plan_host.cpp).
#pragma once
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include "../../include/svt_hip_dsp.h"

// ---- what the kernels of kernel_ois.h share with the host ----
namespace svtdev {
constexpr int OIS_NB_ORIGIN = 16;      // == NB_ORIGIN of kernel_intra.h (position p of an edge at index 16 + p)
constexpr int OIS_MAX_CAND = 61;       // MAX_OIS_CANDIDATES, EbCodingUnit.h:43
enum { OIS_K_DC = 0, OIS_K_V, OIS_K_H, OIS_K_SMOOTH, OIS_K_SMOOTH_V, OIS_K_SMOOTH_H, OIS_K_PAETH, OIS_K_FOLDED };
struct OisKinds {
    uint8_t k[OIS_MAX_CAND + 3];             // kind of candidate c; [OIS_MAX_CAND + 2] = the list has folded candidates
    uint8_t n_nd, nd_c[15], nd_kind[15];     // the candidates ois_nd_kernel computes itself, in list order (host-built: the kernel's loop
};                                           // then runs 7 times, not 45 with a scalar load and a branch per folded candidate)
}  // namespace svtdev

namespace svthost {
static_assert(svtdev::OIS_MAX_CAND == SVT_HIP_OIS_MAX_CANDIDATES && svtdev::OIS_MAX_CAND <= 64, "header constant; const_mask / fold_mask");

constexpr int kDirMaxAngles = 20;             // angles of one directional launch (DirMulti, kernel_intra.h: asserted in svt_hip_intra.hip)
constexpr int kOisMaxSegs = 6;                // 61 candidates: at most 3 full segments, or 2 and one open per zone

struct OisKnobs { bool no_fold, no_nd, no_dir3; };            // svt_hip_tune: ois_no_fold, ois_no_nd, ois_no_dir3
enum OisPath {
    OIS_PATH_ND,            // no directional candidate: the non-directional kernel alone, one launch
    OIS_PATH_FUSED,         // 8x8 / 16x16: gather, the directional kernels sum their SADs themselves, the non-directional kernel picks them up
    OIS_PATH_GENERAL,       // gather, a dense prediction batch per candidate (directional ones folded when `fold`), the SAD kernel
};
// Directional candidates of one zone that share a launch, in list order.  A zone's segment closes when its 21st angle arrives, at list
// position `before`; the general path enqueues it there, between the dense predictions.  Open segments follow (before = ncand), zone 1 first.
struct OisDirSeg {
    uint8_t zone, n, before;                  // zone 0 / 1 / 2: angle below 90 / below 180 / above
    uint8_t slot[kDirMaxAngles];              // candidate index
    int16_t dx[kDirMaxAngles], dy[kDirMaxAngles];
};
struct OisPlan {
    uint32_t bsize;
    int ncand, nseg;
    OisPath path;                             // (OIS_PATH_GENERAL predicts candidate c with ois_dense_mode(kinds.k[c]))
    bool nd_fits;                             // the non-directional candidates fit the fused kernel's list (15; a list may repeat kinds)
    bool dir3;                                // OIS_PATH_FUSED: the three zones in one launch (two or more non-empty, none split)
    bool fold;                                // OIS_PATH_GENERAL: the directional kernels sum their SADs (fold_mask) instead of storing
    uint64_t const_mask, fold_mask;           // OIS_PATH_GENERAL: DC candidates (constant prediction); folded ones
    svtdev::OisKinds kinds;
    OisDirSeg seg[kOisMaxSegs];               // in launch order
    char err[64];                             // why ois_plan refused
};

// dr_intra_derivative (AV1 spec 7.11.2.4; reference EbIntraPrediction.c:299), non-zero entries
inline int ois_dr_derivative(int angle) {
    static const uint16_t at[][2] = {{3, 1023}, {6, 547}, {9, 372}, {14, 273}, {17, 215}, {20, 178}, {23, 151}, {26, 132},
                                     {29, 116}, {32, 102}, {36, 90}, {39, 80}, {42, 71}, {45, 64}, {48, 57}, {51, 51},
                                     {54, 45}, {58, 40}, {61, 35}, {64, 31}, {67, 27}, {70, 23}, {73, 19}, {76, 15},
                                     {81, 11}, {84, 7}, {87, 3}};
    for (const auto& e : at)
        if (e[0] == angle) return e[1];
    return 0;
}
constexpr int kOisModeAngle[13] = {0, 90, 180, 45, 135, 113, 157, 203, 67, 0, 0, 0, 0};      // mode_to_angle_map, EbCodingUnit.h:129

// zone and (dx, dy) of a directional angle other than 90 / 180 (dr_predictor, EbIntraPrediction.c:3352-3383); false: no derivative
inline bool ois_dir_of(int angle, int& zone, int& dx, int& dy) {
    zone = angle < 90 ? 0 : (angle < 180 ? 1 : 2);
    dx = zone == 0 ? ois_dr_derivative(angle) : (zone == 1 ? ois_dr_derivative(180 - angle) : 1);
    dy = zone == 0 ? 1 : (zone == 1 ? ois_dr_derivative(angle - 90) : ois_dr_derivative(270 - angle));
    return dx && dy;
}

// the dense predictor of a non-directional kind (OIS_PATH_GENERAL); DC is a constant (const_mask), a folded kind goes with its segment
inline int ois_dense_mode(int kind) {
    using namespace svtdev;
    static_assert((int)OIS_K_V == SVT_INTRA_V && (int)OIS_K_H == SVT_INTRA_H && (int)OIS_K_SMOOTH == SVT_INTRA_SMOOTH && (int)OIS_K_SMOOTH_V == SVT_INTRA_SMOOTH_V &&
                  (int)OIS_K_SMOOTH_H == SVT_INTRA_SMOOTH_H && (int)OIS_K_PAETH == SVT_INTRA_PAETH, "kinds V .. PAETH are their SVT_INTRA_* modes");
    return kind >= OIS_K_V && kind <= OIS_K_PAETH ? kind : -1;
}

// Fills P from the list (HOST arrays) and the knobs.  0, or SVT_HIP_ERR_INVALID with P.err.
inline int ois_plan(OisPlan& P, uint32_t bsize, const uint8_t* modes, const int8_t* angle_deltas, int ncand, OisKnobs knobs) {
    using namespace svtdev;
    auto fail = [&](const char* fmt, int a, int b) { snprintf(P.err, sizeof(P.err), fmt, a, b); return (int)SVT_HIP_ERR_INVALID; };
    if (bsize != 8 && bsize != 16 && bsize != 32 && bsize != 64) return fail("block size %d", (int)bsize, 0);
    if (ncand <= 0 || ncand > OIS_MAX_CAND) return fail("%d candidates (1..%d, MAX_OIS_CANDIDATES)", ncand, OIS_MAX_CAND);
    P.bsize = bsize; P.ncand = ncand; P.nseg = 0; P.nd_fits = true; P.const_mask = 0; P.err[0] = 0;
    memset(&P.kinds, 0, sizeof(P.kinds));
    OisDirSeg open[3];                        // each zone's open segment
    for (int z = 0; z < 3; z++) { open[z].zone = (uint8_t)z; open[z].n = 0; open[z].before = (uint8_t)ncand; }
    uint64_t dir_mask = 0;
    for (int c = 0; c < ncand; c++) {
        const int m = modes[c];
        if (m > 12) return fail("candidate %d: prediction mode %d", c, m);
        int k = m == 0 ? OIS_K_DC : (m == 9 ? OIS_K_SMOOTH : (m == 10 ? OIS_K_SMOOTH_V : (m == 11 ? OIS_K_SMOOTH_H : OIS_K_PAETH)));
        if (m >= 1 && m <= 8) {
            const int a = kOisModeAngle[m] + 3 * angle_deltas[c];
            if (a <= 0 || a >= 270) return fail("candidate %d: angle %d", c, a);
            k = a == 90 ? OIS_K_V : (a == 180 ? OIS_K_H : OIS_K_FOLDED);
            if (k == OIS_K_FOLDED) {
                int zi, dx, dy;
                if (!ois_dir_of(a, zi, dx, dy)) return fail("candidate %d: angle %d has no derivative", c, a);
                OisDirSeg& S = open[zi];
                if (S.n == kDirMaxAngles) {                   // full: it goes out here, a new one opens
                    P.seg[P.nseg] = S; P.seg[P.nseg++].before = (uint8_t)c;
                    S.n = 0;
                }
                S.slot[S.n] = (uint8_t)c; S.dx[S.n] = (int16_t)dx; S.dy[S.n] = (int16_t)dy; S.n++;
                dir_mask |= 1ull << c;
            }
        }
        P.kinds.k[c] = (uint8_t)k;
        if (k == OIS_K_DC) P.const_mask |= 1ull << c;
        if (k == OIS_K_FOLDED) continue;
        if (P.kinds.n_nd >= sizeof(P.kinds.nd_c)) P.nd_fits = false;
        else { P.kinds.nd_c[P.kinds.n_nd] = (uint8_t)c; P.kinds.nd_kind[P.kinds.n_nd] = (uint8_t)k; P.kinds.n_nd++; }
    }
    const bool split = P.nseg > 0, any_dir = dir_mask != 0, can_fold = bsize <= 16 && !knobs.no_fold;
    for (const OisDirSeg& S : open) if (S.n) P.seg[P.nseg++] = S;
    P.kinds.k[OIS_MAX_CAND + 2] = any_dir ? 1 : 0;            // ois_nd_kernel: rows of dist hold folded sums to pick up
    const bool fused = !knobs.no_nd && P.nd_fits && (!any_dir || can_fold);
    P.path = !fused ? OIS_PATH_GENERAL : (any_dir ? OIS_PATH_FUSED : OIS_PATH_ND);
    P.dir3 = P.path == OIS_PATH_FUSED && !split && P.nseg >= 2 && !knobs.no_dir3;
    P.fold = P.path == OIS_PATH_GENERAL && can_fold; P.fold_mask = P.fold ? dir_mask : 0;
    return 0;
}

// ---- the work buffer: neighbour arrays (above, left; pitch ois_nb_pitch per block), a DC byte per block, ncand dense prediction batches ----
inline size_t ois_nb_pitch(uint32_t bsize) { return (size_t)svtdev::OIS_NB_ORIGIN + 4 * bsize + 16; }     // multiple of 16
struct OisWorkLayout { size_t above, left, dc, pred, cand_pitch, total; };      // byte offsets, each a multiple of 256; total 0: bad arguments
inline OisWorkLayout ois_work_layout(uint32_t bsize, int ncand, size_t nblocks) {
    if ((bsize != 8 && bsize != 16 && bsize != 32 && bsize != 64) || ncand <= 0 || ncand > svtdev::OIS_MAX_CAND) return {};
    auto align = [](size_t v) { return (v + 255) & ~(size_t)255; };
    const size_t nb = align(nblocks * ois_nb_pitch(bsize)), pred = 2 * nb + align(nblocks), cand_pitch = align(nblocks * (size_t)bsize * bsize);
    return {0, nb, 2 * nb, pred, cand_pitch, pred + (size_t)ncand * cand_pitch};
}

// ---- lane geometry of the launches (256 lanes per workgroup) ----
inline uint32_t ois_wgs(size_t nblocks, uint32_t slots) { return (uint32_t)((nblocks + slots - 1) / slots); }
inline uint32_t ois_gather_slots(uint32_t bsize) { return 256 / (2 * bsize); }       // blocks per workgroup of the gather
// the non-directional and SAD kernels: a lane takes cs = 8 (8x8) or 16 pixels; lpb lanes per block, slots blocks per workgroup, LDS for
// [slots][ncand] sums, [4][ncand] wave partials at 64x64 and `extra` words (the non-directional kernel: 4)
struct OisLanes { uint32_t cs, lpb, slots; size_t shmem; };
inline OisLanes ois_lanes(uint32_t bsize, int ncand = 0, int extra = 0) {
    const uint32_t cs = bsize < 16 ? 8 : 16, lpb = bsize * bsize / cs, slots = 256 / lpb;
    return {cs, lpb, slots, (((size_t)slots + (lpb > 64 ? 4 : 0)) * (size_t)ncand + (size_t)extra) * sizeof(uint32_t)};
}
}  // namespace svthost

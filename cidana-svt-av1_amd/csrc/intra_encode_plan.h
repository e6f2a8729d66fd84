// intra_encode_plan.h — what svt_hip_intra_encode_frame settles on the host before it enqueues: the checks, the scratch layout, the
// inverse-scan blob, the wavefront steps and THE SCHEDULE of launches inside a step.  Host only (no HIP header):
// tests/c/intra_encode_plan_host.cpp compiles it with g++; the kernels (kernel_intra_encode.h) read the same constants.
//
// Steps.  Superblock (r, c) reads reconstructed samples of (r, c - 1), (r - 1, c - 1), (r - 1, c) and (r - 1, c + 1).  In step c + 2 r all
// four lie in earlier steps, so the superblocks of a step are independent and launch order on the stream carries every dependency: no
// workgroup waits for another.  A grid of sb_cols x sb_rows takes sb_cols + 2 (sb_rows - 1) steps.
//
// Schedule.  Inside a step one workgroup per (picture, superblock, plane) walks the superblock's entries strictly in order.  A walker
// kernel holds the encode bodies of ONE launch kind (av1_geom.h's tx_launch_kind: 0 = both sides up to 16, 1 = a 32-sample side,
// 2 = a 64-sample side except 64x64, 3 = 64x64; all nineteen bodies in one function go to scratch, kernel_frame.h), advances the plane's
// cursor while the next entry's transform size is of its kind and stops at the first that is not.  A fixed sequence of kinds must
// therefore contain, as a subsequence, the kind runs of every partition tree of a 64x64 superblock:
//   luma    the root shapes give 3 (NONE), 2 .. 2 (HORZ, VERT, H4, V4), 1 1 2 (HORZ_A, VERT_A) or 2 1 1 (HORZ_B, VERT_B); a split root gives
//           four 32x32 quadrants, each of kinds 0 and 1 with at most one change (HORZ_A/B and VERT_A/B mix 16x16 with a 32-sample
//           side), so at most eight alternating runs: 0 1 0 1 0 1 0 1 0 holds every such sequence.
//   chroma  half the sides: only the root shapes reach kind 1 (1 .., 0 0 1 or 1 0 0), everything else is kind 0.
// tests/c/intra_encode_plan_host.cpp enumerates the trees (every root shape, and every choice of the four quadrants' shapes with all
// deeper blocks of kind 0) from the block geometry and proves both sequences sufficient.
//
// Scratch, per (picture, superblock) IE_SB_BYTES: a 32-byte header (the three planes' cursors, the three planes' block origins handed
// to the encode bodies), 256 plan records of 24 bytes (what the pre-pass settled per entry), the 16 x 16 smooth-mode grid in 4x4 units,
// 256 result records (used when the caller passes no d_result) and a 1024-coefficient dump per plane (the quantised coefficients of an
// entry with no place in the stream).
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "../../include/svt_hip_dsp.h"
#include "av1_geom.h"
#include "host_err.h"
#include "md_plan.h"
#include "partition_plan.h"

namespace svthost {

constexpr uint32_t IE_MAX_NSB = 1u << 20, IE_MAX_NPICS = 65535;      // pictures are a grid dimension of the walkers
constexpr int IE_THREADS = 256;

constexpr uint8_t kIeLumaSchedule[] = {3, 2, 0, 1, 0, 1, 0, 1, 0, 1, 0, 2};
constexpr uint8_t kIeChromaSchedule[] = {0, 1, 0};
constexpr int IE_LUMA_LAUNCHES = (int)sizeof(kIeLumaSchedule), IE_CHROMA_LAUNCHES = (int)sizeof(kIeChromaSchedule);

// does the sequence `sched` code a superblock whose coded plane blocks have the launch kinds `kinds`, in order (the walkers' rule)?
inline bool ie_schedule_covers(const uint8_t* kinds, int n, const uint8_t* sched, int ns) {
    int cur = 0;
    for (int s = 0; s < ns; s++)
        while (cur < n && kinds[cur] == sched[s]) cur++;
    return cur == n;
}

inline uint32_t intra_encode_steps(uint32_t sb_cols, uint32_t sb_rows) { return sb_cols + 2u * (sb_rows - 1u); }
// the superblock rows a step holds: r_first .. r_first + n - 1 with the column step - 2 r inside the grid
inline uint32_t intra_encode_step_rows(uint32_t sb_cols, uint32_t sb_rows, uint32_t step, uint32_t* r_first) {
    const uint32_t lo = step >= sb_cols ? (step - sb_cols + 2u) / 2u : 0u;          // the least r with step - 2 r <= sb_cols - 1
    const uint32_t hi = step / 2u < sb_rows - 1u ? step / 2u : sb_rows - 1u;
    *r_first = lo;
    return hi >= lo ? hi - lo + 1u : 0u;
}
// launches of a call: the pre-pass, the steps' schedules, the closing pass
inline int intra_encode_launches(uint32_t sb_cols, uint32_t sb_rows, int planes) {
    if (sb_cols == 0 || sb_rows == 0 || (uint64_t)sb_cols * sb_rows > IE_MAX_NSB || (planes != 1 && planes != 3)) return 0;
    int steps = 0;                                                           // (a grid of one column has empty steps: they launch nothing)
    uint32_t r_first = 0;
    for (uint32_t s = 0; s < intra_encode_steps(sb_cols, sb_rows); s++) steps += intra_encode_step_rows(sb_cols, sb_rows, s, &r_first) != 0;
    return 2 + steps * (IE_LUMA_LAUNCHES + (planes == 3 ? IE_CHROMA_LAUNCHES : 0));
}

// ---- scratch ---------------------------------------------------------------------------------------------------------------------
constexpr uint32_t IE_HDR_BYTES = 32, IE_PLAN_BYTES = 24, IE_PLAN_WORDS = IE_PLAN_BYTES / 4;
constexpr uint32_t IE_OFF_PLAN = IE_HDR_BYTES, IE_OFF_GRID = IE_OFF_PLAN + 256 * IE_PLAN_BYTES, IE_OFF_RESULT = IE_OFF_GRID + 256;
constexpr uint32_t IE_OFF_DUMP = IE_OFF_RESULT + 256 * 8, IE_DUMP_COEFFS = 1024, IE_SB_BYTES = IE_OFF_DUMP + 3 * IE_DUMP_COEFFS * 4;
static_assert(IE_OFF_DUMP % 16 == 0 && IE_SB_BYTES % 16 == 0 && IE_OFF_RESULT % 8 == 0, "alignment of the parts");
inline size_t intra_encode_scratch_bytes(uint32_t npics, uint32_t nsb) {
    if (npics == 0 || npics > IE_MAX_NPICS || nsb == 0 || nsb > IE_MAX_NSB || (uint64_t)npics * nsb > (1ull << 32) / 256) return 0;
    return (size_t)npics * nsb * IE_SB_BYTES;
}

// ---- the inverse scans: [transform size][type][min(w, 32) * min(h, 32)] int16, sizes back to back ---------------------------------------
constexpr uint32_t ie_ncoeff(int tx_size) { return (uint32_t)geom_min(kTxW[tx_size], 32) * (uint32_t)geom_min(kTxH[tx_size], 32); }
constexpr uint32_t ie_iscan_first(int tx_size) {
    uint32_t n = 0;
    for (int t = 0; t < tx_size; t++) n += 16u * ie_ncoeff(t);
    return n;
}
constexpr size_t IE_TABLE_BYTES = (size_t)ie_iscan_first(SVT_TX_SIZES_ALL) * 2;
static_assert(IE_TABLE_BYTES % 16 == 0, "the blob in 16-byte units");

inline int intra_encode_planes(const svt_hip_intra_encode_args* a) { return a->d_recon[1] || a->d_recon[2] || a->d_src[1] || a->d_src[2] ? 3 : 1; }
inline uint32_t intra_encode_sb_pitch(const svt_hip_intra_encode_args* a) { return a->sb_pitch ? a->sb_pitch : a->sb_cols * a->sb_rows; }

inline int intra_encode_check(const svt_hip_intra_encode_args* a) {
    if (!a) return set_err(SVT_HIP_ERR_INVALID, "NULL arguments");
    if (a->npics == 0 || a->npics > IE_MAX_NPICS || a->sb_cols == 0 || a->sb_rows == 0) return set_err(SVT_HIP_ERR_INVALID, "npics %u, sb_cols %u, sb_rows %u", a->npics, a->sb_cols, a->sb_rows);
    const uint64_t nsb = (uint64_t)a->sb_cols * a->sb_rows;
    if (nsb > IE_MAX_NSB) return set_err(SVT_HIP_ERR_INVALID, "nsb %llu (1 .. %u)", (unsigned long long)nsb, IE_MAX_NSB);
    if (a->sb_pitch != 0 && a->sb_pitch < nsb) return set_err(SVT_HIP_ERR_INVALID, "sb_pitch %u below nsb %llu", a->sb_pitch, (unsigned long long)nsb);
    if (a->nsrc == 0) return set_err(SVT_HIP_ERR_INVALID, "nsrc 0");
    if (!a->d_final || !a->d_final_count || !a->d_blk || !a->d_tables || !a->d_src[0] || !a->d_recon[0]) return set_err(SVT_HIP_ERR_INVALID, "NULL member");
    const int nchroma = (a->d_src[1] != nullptr) + (a->d_src[2] != nullptr) + (a->d_recon[1] != nullptr) + (a->d_recon[2] != nullptr);
    if (nchroma != 0 && nchroma != 4) return set_err(SVT_HIP_ERR_INVALID, "chroma planes: all of d_src[1], d_src[2], d_recon[1], d_recon[2] or none");
    const int planes = nchroma ? 3 : 1;
    int nstream = 0;
    for (int p = 0; p < planes; p++) {
        const uint32_t unit = p ? 4u : 8u;
        if (a->width[p] == 0 || a->height[p] == 0 || a->width[p] > 65535u || a->height[p] > 65535u || a->width[p] % unit || a->height[p] % unit)
            return set_err(SVT_HIP_ERR_INVALID, "plane %d: %u x %u (1 .. 65535, multiples of %u)", p, a->width[p], a->height[p], unit);
        if (p && (a->width[p] != a->width[0] / 2 || a->height[p] != a->height[0] / 2))
            return set_err(SVT_HIP_ERR_INVALID, "plane %d: %u x %u is not half the luma's %u x %u", p, a->width[p], a->height[p], a->width[0], a->height[0]);
        if (a->stride[p] < a->width[p] || a->src_stride[p] < a->width[p])
            return set_err(SVT_HIP_ERR_INVALID, "plane %d: stride %u / %u below the width %u", p, a->stride[p], a->src_stride[p], a->width[p]);
        if (a->d_src[p] == a->d_recon[p]) return set_err(SVT_HIP_ERR_INVALID, "plane %d: d_src is d_recon", p);
        if ((uintptr_t)a->d_sb_qcoeff[p] & 15) return set_err(SVT_HIP_ERR_INVALID, "plane %d: misaligned d_sb_qcoeff (16 bytes)", p);
        nstream += a->d_sb_qcoeff[p] != nullptr;
    }
    if (nstream != 0 && nstream != planes) return set_err(SVT_HIP_ERR_INVALID, "d_sb_qcoeff: all of the planes or none");
    if (((uintptr_t)a->d_tables & 15) || ((uintptr_t)a->d_result & 7) || (((uintptr_t)a->d_final | (uintptr_t)a->d_final_count | (uintptr_t)a->d_coeff_offset) & 3))
        return set_err(SVT_HIP_ERR_INVALID, "misaligned buffer (d_tables 16 bytes, d_result 8, d_final / d_final_count / d_coeff_offset 4)");
    if ((uintptr_t)a->d_blk & 7) return set_err(SVT_HIP_ERR_INVALID, "misaligned d_blk (8 bytes)");
    if (int rc = qrows_check(a->q_luma, "q_luma", 3)) return rc;
    if (planes == 3)
        if (int rc = qrows_check(a->q_chroma, "q_chroma", 3)) return rc;
    const size_t need = intra_encode_scratch_bytes(a->npics, (uint32_t)nsb);
    if (need == 0) return set_err(SVT_HIP_ERR_INVALID, "npics %u x nsb %llu: too many superblocks", a->npics, (unsigned long long)nsb);
    if (!a->d_scratch || ((uintptr_t)a->d_scratch & 15) || a->scratch_bytes < need)
        return set_err(SVT_HIP_ERR_INVALID, "scratch: NULL, misaligned or %zu bytes of %zu", a->scratch_bytes, need);
    return SVT_HIP_OK;
}

}  // namespace svthost

// lr_sgr_plan.h — what the self-guided search calls (svt_hip_lr_sgr_stats_frame, _walk_frame, _search_frame) settle on the host before
// they enqueue: the scratch layout, the grids and the checks.  Host only, on lr_plan.h's geometry; tests/c/lr_sgr_plan_host.cpp
// compiles it with g++, the kernels (kernel_lr_sgr.h) call the same functions.
//
// The scratch.  With S = width * height * 3 / 2 the samples of a picture and n = ep_hi - ep_lo:
//   sd      int16 [npics][S]            src - dat per sample
//   f       int16 [npics][n][S][2]      f1 = flt0 - u, f2 = flt1 - u per sample and ep (0 for a radius of 0)
//   stats   int64 [npics][units][16][5]         these four are the search call's own stages (the statistics and the walk call
//   walk    LrSgrWalkRec [npics][units][16]     take theirs as arguments)
//   cand    svt_hip_lr_cand [npics][units]
//   sse     int64 [npics][units]
// Inside a picture's S the samples are unit-contiguous: planes one after another, in a plane the units in index order, in a unit the
// samples row-major over the unit's rectangle.  A unit's samples start at lr_sgr_unit_offset: the unit rows above it cover v_start full
// rows of the plane, the units to its left h_start columns of its own rows.  Every side being a multiple of 4 samples, every unit
// starts on a multiple of 4 samples and holds a multiple of 4: the walk reads 16 bytes of f and 8 of sd at a time.
#pragma once
#include "lr_plan.h"
#include "lr_sgr_solve.h"

namespace svthost {

constexpr int LR_SGR_WALK_THREADS = 1024;
constexpr int LR_SGR_STATS = 5;                               // H00, H11, H01, C0, C1
constexpr size_t LR_SGR_ALIGN = 16;

struct LrSgrWalkRec { int64_t err; int16_t xqd[2], start[2]; int32_t evals, pad; };      // d_walk
struct LrSgrBestRec { int64_t sse, proj_err; int32_t ep; int16_t xqd[2]; };      // d_best
static_assert(sizeof(LrSgrWalkRec) == 24 && sizeof(LrSgrBestRec) == 24, "records of the C ABI");

constexpr uint64_t lr_sgr_pic_samples(uint32_t width, uint32_t height) { return (uint64_t)width * height * 3 / 2; }
constexpr uint64_t lr_sgr_plane_offset(uint32_t width, uint32_t height, int plane) {
    return plane == 0 ? 0 : (uint64_t)width * height + (plane == 2 ? (uint64_t)(width / 2) * (height / 2) : 0);
}
// where the samples of the unit [hs, ..) x [vs, ve) of a plane pw samples wide start inside the plane
constexpr uint64_t lr_sgr_unit_offset(int pw, int hs, int vs, int ve) { return (uint64_t)vs * (uint64_t)pw + (uint64_t)(ve - vs) * (uint64_t)hs; }

struct LrSgrLayout { uint64_t S, sd, f, stats, walk, cand, sse, bytes; };      // byte offsets into the scratch
inline bool lr_sgr_range_ok(int ep_lo, int ep_hi) { return 0 <= ep_lo && ep_lo <= ep_hi && ep_hi <= LR_SGR_PARAMS; }
inline LrSgrLayout lr_sgr_layout(uint32_t width, uint32_t height, const uint32_t us[3], uint32_t npics, int ep_lo, int ep_hi) {
    LrSgrLayout l{};
    const uint64_t units = (uint64_t)lr_units_per_pic(width, height, us) * npics, a = LR_SGR_ALIGN - 1;
    l.S = lr_sgr_pic_samples(width, height);
    l.sd = 0;
    l.f = (l.sd + npics * l.S * 2 + a) & ~a;
    l.stats = (l.f + npics * l.S * 4 * (uint64_t)(ep_hi - ep_lo) + a) & ~a;
    l.walk = l.stats + units * LR_SGR_PARAMS * LR_SGR_STATS * 8;
    l.cand = l.walk + units * LR_SGR_PARAMS * sizeof(LrSgrWalkRec);
    l.sse = (l.cand + units * sizeof(svt_hip_lr_cand) + a) & ~a;
    l.bytes = (l.sse + units * 8 + a) & ~a;
    return l;
}
inline size_t lr_sgr_scratch_bytes(uint32_t width, uint32_t height, const uint32_t us[3], uint32_t npics, int ep_lo, int ep_hi) {
    if (!lr_geometry_ok(width, height, us, npics) || !lr_sgr_range_ok(ep_lo, ep_hi)) return 0;
    if ((uint64_t)lr_units_per_pic(width, height, us) * npics > 0x7ffffu) return 0;
    return (size_t)lr_sgr_layout(width, height, us, npics, ep_lo, ep_hi).bytes;
}

enum { LR_SGR_STATS_WALK = 3, LR_SGR_SEARCH = 4 };      // svt_hip_lr_check's `what`, after LR_APPLY / LR_TRY / LR_STATS
// the picture descriptor under the search's calls: the CDEF picture and the source, for the whole search the deblocked picture too
inline int lr_sgr_pic_check(const svt_hip_lr_pic* p, int what) {
    if (int rc = lr_check(p, what == LR_SGR_SEARCH ? LR_TRY : LR_STATS, nullptr, nullptr, 0)) return rc;
    if ((uint64_t)lr_units_per_pic(p->width, p->height, p->unit_size) * p->npics > 0x7ffffu) return set_err(SVT_HIP_ERR_INVALID, "too many units");
    return SVT_HIP_OK;
}
inline int lr_sgr_common_check(const svt_hip_lr_pic* p, int what, int ep_lo, int ep_hi, const void* d_scratch, size_t scratch_bytes) {
    if (int rc = lr_sgr_pic_check(p, what)) return rc;
    if (!lr_sgr_range_ok(ep_lo, ep_hi)) return set_err(SVT_HIP_ERR_INVALID, "ep range [%d, %d) (0 <= ep_lo <= ep_hi <= 16)", ep_lo, ep_hi);
    const size_t need = lr_sgr_scratch_bytes(p->width, p->height, p->unit_size, p->npics, ep_lo, ep_hi);
    if (!d_scratch || ((uintptr_t)d_scratch & (LR_SGR_ALIGN - 1)) || scratch_bytes < need)
        return set_err(SVT_HIP_ERR_INVALID, "scratch: NULL, not %zu-byte aligned or %zu bytes of %zu", LR_SGR_ALIGN, scratch_bytes, need);
    return SVT_HIP_OK;
}
inline int lr_sgr_stats_check(const svt_hip_lr_pic* p, int ep_lo, int ep_hi, const void* d_stats, const void* d_scratch, size_t scratch_bytes) {
    if (int rc = lr_sgr_common_check(p, LR_SGR_STATS_WALK, ep_lo, ep_hi, d_scratch, scratch_bytes)) return rc;
    if (!d_stats || ((uintptr_t)d_stats & 7)) return set_err(SVT_HIP_ERR_INVALID, "NULL or misaligned d_stats (8 bytes)");
    return SVT_HIP_OK;
}
inline int lr_sgr_walk_check(const svt_hip_lr_pic* p, int ep_lo, int ep_hi, const void* d_stats, const void* d_start, const void* d_scratch, size_t scratch_bytes,
                             const void* d_walk) {
    if (int rc = lr_sgr_common_check(p, LR_SGR_STATS_WALK, ep_lo, ep_hi, d_scratch, scratch_bytes)) return rc;
    if (!d_start && (!d_stats || ((uintptr_t)d_stats & 7))) return set_err(SVT_HIP_ERR_INVALID, "NULL or misaligned d_stats (8 bytes) and no d_start");
    if (d_start && ((uintptr_t)d_start & 1)) return set_err(SVT_HIP_ERR_INVALID, "misaligned d_start (2 bytes)");
    if (!d_walk || ((uintptr_t)d_walk & 7)) return set_err(SVT_HIP_ERR_INVALID, "NULL or misaligned d_walk (8 bytes)");
    return SVT_HIP_OK;
}
inline int lr_sgr_search_check(const svt_hip_lr_pic* p, int ep_lo, int ep_hi, const void* d_best, const void* d_scratch, size_t scratch_bytes) {
    if (int rc = lr_sgr_common_check(p, LR_SGR_SEARCH, ep_lo, ep_hi, d_scratch, scratch_bytes)) return rc;
    if (!d_best || ((uintptr_t)d_best & 7)) return set_err(SVT_HIP_ERR_INVALID, "NULL or misaligned d_best (8 bytes)");
    return SVT_HIP_OK;
}

}  // namespace svthost

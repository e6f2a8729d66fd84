// svt_hip_lr.hip — loop restoration of whole pictures: svt_hip_lr_apply_frame (av1_loop_restoration_filter_frame),
// svt_hip_lr_try_frame (try_restoration_unit_seg per candidate) and svt_hip_lr_wiener_stats_frame (av1_compute_stats[_highbd] per
// unit), kernels in kernel_lr.h.  The geometry, the checks, the launch shapes and the scratch size are lr_plan.h's.
#include <stddef.h>

#include "host_common.h"
#include "kernel_lr.h"
#include "kernel_lr_sgr.h"

using namespace svtdev;
using namespace svthost;

static_assert(sizeof(svt_hip_lr_pic) == 288 && offsetof(svt_hip_lr_pic, d_dblk) == 40 && offsetof(svt_hip_lr_pic, width) == 160 &&
              offsetof(svt_hip_lr_pic, npics) == 184 && offsetof(svt_hip_lr_pic, cdef_pitch) == 192, "svt_hip_lr_pic layout");
static_assert(sizeof(svt_hip_lr_unit) == 24 && offsetof(svt_hip_lr_unit, hfilter) == 10 && offsetof(svt_hip_lr_unit, xqd) == 16 &&
              offsetof(svt_hip_lr_unit, ep) == 20, "lr_rec reads svt_hip_lr_unit as six words");
static_assert(sizeof(svt_hip_lr_cand) == 36 && offsetof(svt_hip_lr_cand, u) == 12, "lr_try_kernel reads svt_hip_lr_cand as nine words");

static uint32_t umax(uint32_t a, uint32_t b) { return a > b ? a : b; }

static LrDev lr_dev(const svt_hip_lr_pic* p) {
    LrDev d;
    memset(&d, 0, sizeof(d));
    for (int i = 0; i < 3; i++) {
        d.cdef[i] = p->d_cdef[i]; d.dblk[i] = p->d_dblk[i]; d.src[i] = p->d_src[i]; d.dst[i] = p->d_dst[i];
        d.cdef_stride[i] = p->cdef_stride[i]; d.dblk_stride[i] = p->dblk_stride[i]; d.src_stride[i] = p->src_stride[i]; d.dst_stride[i] = p->dst_stride[i];
        d.cdef_pitch[i] = p->cdef_pitch[i]; d.dblk_pitch[i] = p->dblk_pitch[i]; d.src_pitch[i] = p->src_pitch[i]; d.dst_pitch[i] = p->dst_pitch[i];
        d.pl[i] = lr_plane(p->width, p->height, p->unit_size, i);
    }
    d.bd = p->bit_depth; d.npics = p->npics; d.units_per_pic = lr_units_per_pic(p->width, p->height, p->unit_size);
    return d;
}

extern "C" int svt_hip_lr_check(const svt_hip_lr_pic* pic, int what, const int32_t frame_type[3], const svt_hip_lr_unit* h_units, uint32_t nunits) {
    if (what == LR_SGR_STATS_WALK || what == LR_SGR_SEARCH) return lr_sgr_pic_check(pic, what);
    return lr_check(pic, what, frame_type, h_units, nunits);
}
extern "C" size_t svt_hip_lr_stats_scratch_bytes(uint32_t width, uint32_t height, const uint32_t unit_size[3], uint32_t npics) {
    return lr_stats_scratch_bytes(width, height, unit_size, npics);
}
extern "C" int svt_hip_lr_unit_grid(uint32_t width, uint32_t height, const uint32_t unit_size[3], int plane, int32_t out[3]) {
    if (!out || plane < 0 || plane > 2 || !lr_geometry_ok(width, height, unit_size, 1)) return set_err(SVT_HIP_ERR_INVALID, "bad geometry, plane %d or NULL out", plane);
    const LrPlane g = lr_plane(width, height, unit_size, plane);
    out[0] = g.nh; out[1] = g.nv; out[2] = g.nh * g.nv;
    return SVT_HIP_OK;
}
extern "C" int svt_hip_lr_unit_limits(uint32_t width, uint32_t height, const uint32_t unit_size[3], int plane, uint32_t index, int32_t out[4]) {
    if (!out || plane < 0 || plane > 2 || !lr_geometry_ok(width, height, unit_size, 1)) return set_err(SVT_HIP_ERR_INVALID, "bad geometry, plane %d or NULL out", plane);
    const LrPlane g = lr_plane(width, height, unit_size, plane);
    if (index >= (uint32_t)(g.nh * g.nv)) return set_err(SVT_HIP_ERR_INVALID, "unit %u of %d", index, g.nh * g.nv);
    const int i = (int)index / g.nh, j = (int)index % g.nh, off = lr_stripe_off(g.ss);
    out[0] = lr_unit_start(j, g.us, 0); out[1] = lr_unit_end(j, g.nh, g.us, 0, g.w);
    out[2] = lr_unit_start(i, g.us, off); out[3] = lr_unit_end(i, g.nv, g.us, off, g.h);
    return SVT_HIP_OK;
}
extern "C" uint32_t svt_hip_lr_unit_offset(uint32_t width, uint32_t height, const uint32_t unit_size[3], int plane) {
    if (plane < 0 || plane > 2 || !lr_geometry_ok(width, height, unit_size, 1)) return 0;
    return lr_plane(width, height, unit_size, plane).unit0;
}
extern "C" uint32_t svt_hip_lr_units_per_pic(uint32_t width, uint32_t height, const uint32_t unit_size[3]) {
    return lr_geometry_ok(width, height, unit_size, 1) ? lr_units_per_pic(width, height, unit_size) : 0;
}

extern "C" int svt_hip_lr_apply_frame(const svt_hip_lr_pic* pic, const int32_t frame_type[3], const svt_hip_lr_unit* d_units, void* stream) {
    if (int rc = require_init()) return rc;
    if (int rc = lr_check(pic, LR_APPLY, frame_type, nullptr, 0)) return rc;
    if ((frame_type[0] || frame_type[1] || frame_type[2]) && (!d_units || ((uintptr_t)d_units & 3))) return set_err(SVT_HIP_ERR_INVALID, "NULL or misaligned d_units");
    LrDev d = lr_dev(pic);
    d.units = (const uint32_t*)d_units;
    uint32_t tiles = 0;
    for (int i = 0; i < 3; i++) {
        d.ftype[i] = frame_type[i];
        tiles = umax(tiles, (uint32_t)(d.pl[i].ntx * d.pl[i].nstripes));
    }
    if (pic->bit_depth == 8) hipLaunchKernelGGL(lr_apply_kernel<uint8_t>, dim3(tiles, 3, pic->npics), dim3(LR_NT), 0, (hipStream_t)stream, d);
    else hipLaunchKernelGGL(lr_apply_kernel<uint16_t>, dim3(tiles, 3, pic->npics), dim3(LR_NT), 0, (hipStream_t)stream, d);
    return launch_status("lr_apply_frame");
}

// the two launches of a try, for arguments the caller has checked
static int lr_try_enqueue(LrDev d, const void* d_cand, uint32_t ncand, void* d_sse, hipStream_t s) {
    d.cand = (const uint32_t*)d_cand; d.sse = (unsigned long long*)d_sse;
    for (int i = 0; i < 3; i++) d.try_tiles = umax(d.try_tiles, lr_try_tiles(d.pl[i]));
    hipLaunchKernelGGL(lr_zero_kernel, dim3((ncand + LR_NT - 1) / LR_NT), dim3(LR_NT), 0, s, d.sse, (size_t)ncand);
    if (int rc = launch_status("lr_try_frame (zero)")) return rc;
    if (d.bd == 8) hipLaunchKernelGGL(lr_try_kernel<uint8_t>, dim3(ncand * d.try_tiles), dim3(LR_NT), 0, s, d);
    else hipLaunchKernelGGL(lr_try_kernel<uint16_t>, dim3(ncand * d.try_tiles), dim3(LR_NT), 0, s, d);
    return launch_status("lr_try_frame");
}

extern "C" int svt_hip_lr_try_frame(const svt_hip_lr_pic* pic, const svt_hip_lr_cand* d_cand, uint32_t ncand, int64_t* d_sse, void* stream) {
    if (int rc = require_init()) return rc;
    if (int rc = lr_try_check(pic, d_cand, ncand, d_sse)) return rc;
    return lr_try_enqueue(lr_dev(pic), d_cand, ncand, d_sse, (hipStream_t)stream);
}

template <typename T>
static int lr_stats_launch(const LrDev& d, uint32_t units, hipStream_t s) {
    hipLaunchKernelGGL(lr_avg_kernel<T>, dim3(units), dim3(LR_NT), 0, s, d);
    if (int rc = launch_status("lr_wiener_stats_frame (average)")) return rc;
    bool have[8] = {};
    for (int i = 0; i < 3; i++) have[d.win[i]] = true;
    if (have[7]) hipLaunchKernelGGL((lr_stats_kernel<T, 7>), dim3(units * d.stats_tiles), dim3(LR_NT), 0, s, d);
    if (have[5]) hipLaunchKernelGGL((lr_stats_kernel<T, 5>), dim3(units * d.stats_tiles), dim3(LR_NT), 0, s, d);
    if (have[3]) hipLaunchKernelGGL((lr_stats_kernel<T, 3>), dim3(units * d.stats_tiles), dim3(LR_NT), 0, s, d);
    return launch_status("lr_wiener_stats_frame");
}

extern "C" int svt_hip_lr_wiener_stats_frame(const svt_hip_lr_pic* pic, const int32_t wiener_win[3], int64_t* d_M, int64_t* d_H, void* d_scratch,
                                             size_t scratch_bytes, void* stream) {
    if (int rc = require_init()) return rc;
    if (int rc = lr_stats_check(pic, wiener_win, d_M, d_H, d_scratch, scratch_bytes)) return rc;
    hipStream_t s = (hipStream_t)stream;
    LrDev d = lr_dev(pic);
    d.M = (long long*)d_M; d.H = (long long*)d_H; d.avg = (uint32_t*)d_scratch;
    for (int i = 0; i < 3; i++) {
        d.win[i] = wiener_win[i];
        d.stats_tiles = umax(d.stats_tiles, lr_stats_tiles(d.pl[i]));
    }
    const uint32_t units = d.units_per_pic * pic->npics;
    const size_t nm = (size_t)units * LR_WIN2, nh = (size_t)units * LR_WIN2 * LR_WIN2;
    hipLaunchKernelGGL(lr_zero_kernel, dim3((uint32_t)((nm + LR_NT - 1) / LR_NT)), dim3(LR_NT), 0, s, (unsigned long long*)d_M, nm);
    hipLaunchKernelGGL(lr_zero_kernel, dim3((uint32_t)((nh + LR_NT - 1) / LR_NT)), dim3(LR_NT), 0, s, (unsigned long long*)d_H, nh);
    if (int rc = launch_status("lr_wiener_stats_frame (zero)")) return rc;
    if (int rc = pic->bit_depth == 8 ? lr_stats_launch<uint8_t>(d, units, s) : lr_stats_launch<uint16_t>(d, units, s)) return rc;
    hipLaunchKernelGGL(lr_stats_finish_kernel, dim3(units), dim3(LR_NT), 0, s, d);
    return launch_status("lr_wiener_stats_frame (finish)");
}

// ---- the self-guided parameter search ---------------------------------------------------------------------------------------------
static_assert(sizeof(svt_hip_lr_sgr_walk) == sizeof(LrSgrWalkRec) && offsetof(svt_hip_lr_sgr_walk, xqd) == 8 && offsetof(svt_hip_lr_sgr_walk, start) == 12 && offsetof(svt_hip_lr_sgr_walk, evals) == 16 &&
              sizeof(svt_hip_lr_sgr_best) == sizeof(LrSgrBestRec) && offsetof(svt_hip_lr_sgr_best, ep) == 16 && offsetof(svt_hip_lr_sgr_best, xqd) == 20,
              "the kernels write svt_hip_lr_sgr_walk / svt_hip_lr_sgr_best through lr_sgr_plan.h's records");

static LrSgrDev lr_sgr_dev(const svt_hip_lr_pic* p, int ep_lo, int ep_hi, void* d_scratch) {
    const LrSgrLayout l = lr_sgr_layout(p->width, p->height, p->unit_size, p->npics, ep_lo, ep_hi);
    LrSgrDev g;
    memset(&g, 0, sizeof(g));
    g.ep_lo = ep_lo; g.ep_hi = ep_hi; g.S = l.S;
    g.sd = (short*)((char*)d_scratch + l.sd); g.f = (uint32_t*)((char*)d_scratch + l.f);
    return g;
}
static int lr_sgr_stats_enqueue(const LrDev& d, const LrSgrDev& g, hipStream_t s) {
    if (g.ep_lo == g.ep_hi) return SVT_HIP_OK;
    const size_t n = (size_t)d.npics * d.units_per_pic * (size_t)(g.ep_hi - g.ep_lo) * LR_SGR_STATS;
    hipLaunchKernelGGL(lr_sgr_zero_kernel, dim3((uint32_t)((n + LR_NT - 1) / LR_NT)), dim3(LR_NT), 0, s, d, g);
    if (int rc = launch_status("lr_sgr_stats_frame (zero)")) return rc;
    uint32_t tiles = 0;
    for (int i = 0; i < 3; i++) tiles = umax(tiles, (uint32_t)(d.pl[i].ntx * d.pl[i].nstripes));
    if (d.bd == 8) hipLaunchKernelGGL(lr_sgr_stats_kernel<uint8_t>, dim3(tiles, 3, d.npics), dim3(LR_NT), 0, s, d, g);
    else hipLaunchKernelGGL(lr_sgr_stats_kernel<uint16_t>, dim3(tiles, 3, d.npics), dim3(LR_NT), 0, s, d, g);
    return launch_status("lr_sgr_stats_frame");
}
static int lr_sgr_walk_enqueue(const LrDev& d, const LrSgrDev& g, hipStream_t s) {
    if (g.ep_lo == g.ep_hi) return SVT_HIP_OK;
    hipLaunchKernelGGL(lr_sgr_walk_kernel, dim3(d.npics * d.units_per_pic * (uint32_t)(g.ep_hi - g.ep_lo)), dim3(LR_SGR_NT), 0, s, d, g);
    return launch_status("lr_sgr_walk_frame");
}

extern "C" size_t svt_hip_lr_sgr_scratch_bytes(uint32_t width, uint32_t height, const uint32_t unit_size[3], uint32_t npics, int ep_lo, int ep_hi) {
    return lr_sgr_scratch_bytes(width, height, unit_size, npics, ep_lo, ep_hi);
}

extern "C" int svt_hip_lr_sgr_stats_frame(const svt_hip_lr_pic* pic, int ep_lo, int ep_hi, int64_t* d_stats, void* d_scratch, size_t scratch_bytes, void* stream) {
    if (int rc = require_init()) return rc;
    if (int rc = lr_sgr_stats_check(pic, ep_lo, ep_hi, d_stats, d_scratch, scratch_bytes)) return rc;
    LrSgrDev g = lr_sgr_dev(pic, ep_lo, ep_hi, d_scratch);
    g.stats = (long long*)d_stats;
    return lr_sgr_stats_enqueue(lr_dev(pic), g, (hipStream_t)stream);
}

extern "C" int svt_hip_lr_sgr_walk_frame(const svt_hip_lr_pic* pic, int ep_lo, int ep_hi, const int64_t* d_stats, const int16_t* d_start, const void* d_scratch,
                                         size_t scratch_bytes, svt_hip_lr_sgr_walk* d_walk, void* stream) {
    if (int rc = require_init()) return rc;
    if (int rc = lr_sgr_walk_check(pic, ep_lo, ep_hi, d_stats, d_start, d_scratch, scratch_bytes, d_walk)) return rc;
    LrSgrDev g = lr_sgr_dev(pic, ep_lo, ep_hi, (void*)d_scratch);
    g.stats = (long long*)d_stats; g.start = d_start; g.walk = (LrSgrWalkRec*)d_walk;
    return lr_sgr_walk_enqueue(lr_dev(pic), g, (hipStream_t)stream);
}

extern "C" int svt_hip_lr_sgr_search_frame(const svt_hip_lr_pic* pic, int ep_lo, int ep_hi, svt_hip_lr_sgr_best* d_best, void* d_scratch, size_t scratch_bytes,
                                           void* stream) {
    if (int rc = require_init()) return rc;
    if (int rc = lr_sgr_search_check(pic, ep_lo, ep_hi, d_best, d_scratch, scratch_bytes)) return rc;
    hipStream_t s = (hipStream_t)stream;
    const LrSgrLayout l = lr_sgr_layout(pic->width, pic->height, pic->unit_size, pic->npics, ep_lo, ep_hi);
    const LrDev d = lr_dev(pic);
    LrSgrDev g = lr_sgr_dev(pic, ep_lo, ep_hi, d_scratch);
    char* base = (char*)d_scratch;
    g.stats = (long long*)(base + l.stats); g.walk = (LrSgrWalkRec*)(base + l.walk); g.best = (LrSgrBestRec*)d_best;
    g.cand = (uint32_t*)(base + l.cand); g.sse = (const long long*)(base + l.sse);
    if (int rc = lr_sgr_stats_enqueue(d, g, s)) return rc;
    if (int rc = lr_sgr_walk_enqueue(d, g, s)) return rc;
    const uint32_t units = d.npics * d.units_per_pic;
    hipLaunchKernelGGL(lr_sgr_pick_kernel, dim3((units + LR_NT - 1) / LR_NT), dim3(LR_NT), 0, s, d, g);
    if (int rc = launch_status("lr_sgr_search_frame (pick)")) return rc;
    if (int rc = lr_try_enqueue(d, g.cand, units, base + l.sse, s)) return rc;
    hipLaunchKernelGGL(lr_sgr_sse_kernel, dim3((units + LR_NT - 1) / LR_NT), dim3(LR_NT), 0, s, d, g);
    return launch_status("lr_sgr_search_frame (sse)");
}

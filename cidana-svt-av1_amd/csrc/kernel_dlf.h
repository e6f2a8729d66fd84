// kernel_dlf.h — AV1 deblocking of whole pictures (svt_hip_dlf_apply_frame, svt_hip_dlf_search_frame) and the scatter of a final block
// list into the mode-info grid (svt_hip_dlf_mi_frame).
//
// Pass order and independence.  The reference's loop_filter_sb filters the vertical edges of a superblock and then the
// horizontal edges of the superblock to its left, which is every vertical edge of the picture before any horizontal edge that reads
// what it wrote: the same picture as all vertical edges, then all horizontal ones.  Inside a pass no edge reads a sample another edge
// of the pass modifies: a filter is at most as long as the smaller transform side it separates, it modifies 2 (4- and 6-tap), 3
// (8-tap) or 6 (14-tap) samples per side and reads 2, 3, 4 or 7, and the next edge on either side is at least that transform side
// away.  So every 4-sample edge unit of a pass is decided and filtered on its own.
//
//   dlf_decide        set_lpf_parameters for one edge unit: the length and the two units' level classes, nothing level-dependent
//   dlf_filter_line   filter4 / 6 / 8 / 14 on one line across an edge, any bit depth (thresholds shifted by bd - 8)
//   dlf_pass_kernel   in place: one pass (vertical or horizontal edges) over the three planes, straight on global memory
//   dlf_tile_kernel   two buffers / search: a 64x64 luma (32x32 chroma) tile with 8 samples of halo in the LDS, both passes there; the
//                     apply stores the tile, the search repeats the passes per level on a copy and sums the squared error
//   dlf_sum_kernel    the search's second launch: partial sums per tile -> d_sse[pic][plane][64]
//   dlf_mi_kernel     one wave per superblock: final entries -> grid records
// Why a halo of 8: the tile's right / bottom neighbours' first edges modify up to 6 samples inside the tile and read 7 past it; the
// horizontal edges read 7 rows above the tile, whose samples the vertical edges of those rows must have filtered first.  Edges further
// out cannot reach the tile on a grid whose blocks are aligned to their size.  Out-of-picture samples of the halo are zero and are
// never written back; every edge the tile filters lies at a local coordinate 8 .. 72, so a 14-tap filter stays inside the LDS tile
// whatever the grid holds.
#pragma once
#include "dev_common.h"
#include "dlf_plan.h"
#include "kernel_final_list.h"

namespace svtdev {

constexpr int DLF_T = svthost::DLF_TILE, DLF_H = svthost::DLF_HALO, DLF_NT = svthost::DLF_THREADS;
constexpr int DLF_SIDE = DLF_T + 2 * DLF_H;                 // 80 (luma); chroma uses 48 of it
template <typename T> constexpr int dlf_pitch() { return DLF_SIDE + (sizeof(T) == 1 ? 4 : 2); }      // an odd number of 4-byte words per row
constexpr int DLF_EDGES = DLF_T / 4 + 1;                    // edges a tile filters per row / column: its own and the next tile's first

struct DlfTab {
    uint8_t tx_side[2][SVT_TX_SIZES_ALL];          // [dir] luma transform side across the edge
    uint8_t uv_side[2][22];                        // [dir] chroma transform side, by block size
    uint8_t pu_side[2][2][22];                     // [chroma][dir] prediction block side
};
constexpr DlfTab dlf_tab() {
    DlfTab T{};
    for (int d = 0; d < 2; d++) {
        for (int t = 0; t < SVT_TX_SIZES_ALL; t++) T.tx_side[d][t] = (uint8_t)svthost::dlf_tx_side(0, d, 0, t);
        for (int b = 0; b < 22; b++) {
            T.uv_side[d][b] = (uint8_t)svthost::dlf_tx_side(1, d, b, 0);
            T.pu_side[0][d][b] = (uint8_t)svthost::dlf_pu_side(0, d, b);
            T.pu_side[1][d][b] = (uint8_t)svthost::dlf_pu_side(1, d, b);
        }
    }
    return T;
}
static __device__ const DlfTab kDlfTab = dlf_tab();

struct DlfDev {
    const void* rec[3]; const void* src[3]; void* dst[3];
    uint32_t rec_stride[3], src_stride[3], dst_stride[3];
    unsigned long long rec_pitch[3], src_pitch[3], dst_pitch[3], mi_pitch;      // samples / records between the pictures of a stack
    const uint32_t* mi; uint32_t mi_stride;          // svt_hip_dlf_mi as one word
    uint32_t width, height, ntx, nty;
    int sh, sharp, delta_on;
    unsigned long long rd;                           // ref_deltas, a byte each
    uint32_t md;                                     // mode_deltas, a byte each
    int lvl[3][2];                                   // apply: the base level per plane and direction
    int plane_mode[3];                               // apply: 0 leave alone, 1 copy, 2 filter
    unsigned long long mask[3];                      // search: the levels wanted per plane
    unsigned long long* partial;                     // search: [pic][plane][tile][64]
    unsigned long long* sse;                         // search: [pic][plane][64]
};

// set_lpf_parameters (EbDeblockingFilter.c:893-1012) for the edge unit whose first sample is (x, y) of `plane` (inside the plane, the
// coordinate across the edge not 0).  -> 0: no edge here; else length | class of the current unit << 4 | class of the previous << 8,
// a class being ref_frame[0] * 2 + mode_lf_lut[mode], which with the base level gives the unit's level.
__device__ __forceinline__ uint32_t dlf_decide(const uint32_t* mi, uint32_t mi_stride, int plane, int dir, uint32_t x, uint32_t y) {
    const uint32_t ss = plane ? 1u : 0u;
    const uint32_t mr = ss | ((y << ss) >> 2), mc = ss | ((x << ss) >> 2);       // chroma: the odd row and column of the 8x8
    const uint32_t cur = mi[(size_t)mr * mi_stride + mc];
    const uint32_t coord = dir == 0 ? x : y;
    const uint32_t cb = min(cur & 255u, 21u), ct = min(cur >> 8 & 255u, 18u);
    const uint32_t ts = plane ? kDlfTab.uv_side[dir][cb] : kDlfTab.tx_side[dir][ct];
    if (coord & (ts - 1)) return 0;                                               // not a transform edge
    const uint32_t prv = dir == 0 ? mi[(size_t)mr * mi_stride + mc - (1u << ss)] : mi[(size_t)(mr - (1u << ss)) * mi_stride + mc];
    const uint32_t pb = min(prv & 255u, 21u), pt = min(prv >> 8 & 255u, 18u);
    const uint32_t pv_ts = plane ? kDlfTab.uv_side[dir][pb] : kDlfTab.tx_side[dir][pt];
    const uint32_t cref = cur >> 16 & 7u, pref = prv >> 16 & 7u;
    const bool cskip = (cur >> 23 & 1u) && cref > 0, pskip = (prv >> 23 & 1u) && pref > 0;
    const bool pu_edge = !(coord & (kDlfTab.pu_side[ss][dir][cb] - 1u));
    if (pskip && cskip && !pu_edge) return 0;
    const uint32_t len = (uint32_t)svthost::dlf_length(plane, (int)min(ts, pv_ts));
    const uint32_t ccls = cref * 2 + (uint32_t)svthost::dlf_mode_lf((int)(cur >> 24)), pcls = pref * 2 + (uint32_t)svthost::dlf_mode_lf((int)(prv >> 24));
    return len | ccls << 4 | pcls << 8;
}

// the level of a decided edge under `base` (0: the edge is not filtered)
__device__ __forceinline__ int dlf_class_level(const DlfDev& F, uint32_t cls, int base) {
    const uint32_t ref = cls >> 1 & 7u;
    return svthost::dlf_level(base, F.delta_on != 0, (int8_t)(F.rd >> (8 * ref)), ref ? (int8_t)(F.md >> (8 * (cls & 1u))) : 0);
}
__device__ __forceinline__ int dlf_edge_level(const DlfDev& F, uint32_t d, int base) {
    const int cl = dlf_class_level(F, d >> 4, base);
    return cl ? cl : dlf_class_level(F, d >> 8, base);
}

// One line across an edge: s points at q0, the samples are `step` apart.  filter4 / filter6 / filter8 / filter14 (:133-366) and
// their highbd twins: sh = bd - 8 shifts every threshold and the clamp range.
template <typename T>
__device__ __forceinline__ void dlf_filter_line(T* s, int step, int len, int level, int sharp, int sh) {
    const int limit = svthost::dlf_lim(level, sharp) << sh, blimit = svthost::dlf_mblim(level, sharp) << sh;
    const int thresh = svthost::dlf_hev(level) << sh, flat_t = 1 << sh;
    const int p1 = s[-2 * step], p0 = s[-step], q0 = s[0], q1 = s[step];
    if (abs(p1 - p0) > limit || abs(q1 - q0) > limit || abs(p0 - q0) * 2 + abs(p1 - q1) / 2 > blimit) return;       // mask 0: nothing changes
    int p2 = 0, q2 = 0, p3 = 0, q3 = 0;
    bool flat = false;
    if (len >= 6) {
        p2 = s[-3 * step]; q2 = s[2 * step];
        if (abs(p2 - p1) > limit || abs(q2 - q1) > limit) return;
        flat = abs(p1 - p0) <= flat_t && abs(q1 - q0) <= flat_t && abs(p2 - p0) <= flat_t && abs(q2 - q0) <= flat_t;
    }
    if (len >= 8) {
        p3 = s[-4 * step]; q3 = s[3 * step];
        if (abs(p3 - p2) > limit || abs(q3 - q2) > limit) return;
        flat = flat && abs(p3 - p0) <= flat_t && abs(q3 - q0) <= flat_t;
    }
    if (flat && len == 14) {
        const int p4 = s[-5 * step], p5 = s[-6 * step], p6 = s[-7 * step], q4 = s[4 * step], q5 = s[5 * step], q6 = s[6 * step];
        if (abs(p4 - p0) <= flat_t && abs(q4 - q0) <= flat_t && abs(p5 - p0) <= flat_t && abs(q5 - q0) <= flat_t && abs(p6 - p0) <= flat_t &&
            abs(q6 - q0) <= flat_t) {
            s[-6 * step] = (T)((p6 * 7 + p5 * 2 + p4 * 2 + p3 + p2 + p1 + p0 + q0 + 8) >> 4);
            s[-5 * step] = (T)((p6 * 5 + p5 * 2 + p4 * 2 + p3 * 2 + p2 + p1 + p0 + q0 + q1 + 8) >> 4);
            s[-4 * step] = (T)((p6 * 4 + p5 + p4 * 2 + p3 * 2 + p2 * 2 + p1 + p0 + q0 + q1 + q2 + 8) >> 4);
            s[-3 * step] = (T)((p6 * 3 + p5 + p4 + p3 * 2 + p2 * 2 + p1 * 2 + p0 + q0 + q1 + q2 + q3 + 8) >> 4);
            s[-2 * step] = (T)((p6 * 2 + p5 + p4 + p3 + p2 * 2 + p1 * 2 + p0 * 2 + q0 + q1 + q2 + q3 + q4 + 8) >> 4);
            s[-step] = (T)((p6 + p5 + p4 + p3 + p2 + p1 * 2 + p0 * 2 + q0 * 2 + q1 + q2 + q3 + q4 + q5 + 8) >> 4);
            s[0] = (T)((p5 + p4 + p3 + p2 + p1 + p0 * 2 + q0 * 2 + q1 * 2 + q2 + q3 + q4 + q5 + q6 + 8) >> 4);
            s[step] = (T)((p4 + p3 + p2 + p1 + p0 + q0 * 2 + q1 * 2 + q2 * 2 + q3 + q4 + q5 + q6 * 2 + 8) >> 4);
            s[2 * step] = (T)((p3 + p2 + p1 + p0 + q0 + q1 * 2 + q2 * 2 + q3 * 2 + q4 + q5 + q6 * 3 + 8) >> 4);
            s[3 * step] = (T)((p2 + p1 + p0 + q0 + q1 + q2 * 2 + q3 * 2 + q4 * 2 + q5 + q6 * 4 + 8) >> 4);
            s[4 * step] = (T)((p1 + p0 + q0 + q1 + q2 + q3 * 2 + q4 * 2 + q5 * 2 + q6 * 5 + 8) >> 4);
            s[5 * step] = (T)((p0 + q0 + q1 + q2 + q3 + q4 * 2 + q5 * 2 + q6 * 7 + 8) >> 4);
            return;
        }
    }
    if (flat && len >= 8) {                               // 7-tap [1, 1, 1, 2, 1, 1, 1]
        s[-3 * step] = (T)((p3 + p3 + p3 + 2 * p2 + p1 + p0 + q0 + 4) >> 3);
        s[-2 * step] = (T)((p3 + p3 + p2 + 2 * p1 + p0 + q0 + q1 + 4) >> 3);
        s[-step] = (T)((p3 + p2 + p1 + 2 * p0 + q0 + q1 + q2 + 4) >> 3);
        s[0] = (T)((p2 + p1 + p0 + 2 * q0 + q1 + q2 + q3 + 4) >> 3);
        s[step] = (T)((p1 + p0 + q0 + 2 * q1 + q2 + q3 + q3 + 4) >> 3);
        s[2 * step] = (T)((p0 + q0 + q1 + 2 * q2 + q3 + q3 + q3 + 4) >> 3);
        return;
    }
    if (flat && len == 6) {                               // 5-tap [1, 2, 2, 2, 1]
        s[-2 * step] = (T)((p2 * 3 + p1 * 2 + p0 * 2 + q0 + 4) >> 3);
        s[-step] = (T)((p2 + p1 * 2 + p0 * 2 + q0 * 2 + q1 + 4) >> 3);
        s[0] = (T)((p1 + p0 * 2 + q0 * 2 + q1 * 2 + q2 + 4) >> 3);
        s[step] = (T)((p0 + q0 * 2 + q1 * 2 + q2 * 3 + 4) >> 3);
        return;
    }
    // filter4
    const int c = 0x80 << sh, lo = -(128 << sh), hi = (128 << sh) - 1;
    const int ps1 = p1 - c, ps0 = p0 - c, qs0 = q0 - c, qs1 = q1 - c;
    const bool hev = abs(p1 - p0) > thresh || abs(q1 - q0) > thresh;
    int f = hev ? svthost::dlf_clamp(ps1 - qs1, lo, hi) : 0;
    f = svthost::dlf_clamp(f + 3 * (qs0 - ps0), lo, hi);
    const int f1 = svthost::dlf_clamp(f + 4, lo, hi) >> 3, f2 = svthost::dlf_clamp(f + 3, lo, hi) >> 3;
    s[0] = (T)(svthost::dlf_clamp(qs0 - f1, lo, hi) + c);
    s[-step] = (T)(svthost::dlf_clamp(ps0 + f2, lo, hi) + c);
    f = hev ? 0 : (f1 + 1) >> 1;
    s[step] = (T)(svthost::dlf_clamp(qs1 - f, lo, hi) + c);
    s[-2 * step] = (T)(svthost::dlf_clamp(ps1 + f, lo, hi) + c);
}

// In place, one pass: dir 0 every vertical edge, dir 1 every horizontal edge of the three planes.  blockIdx.y = plane, .z = picture;
// one thread per line of an edge unit (dir 0: consecutive threads along a row of edges; dir 1: along a row of samples).
template <typename T>
__global__ __launch_bounds__(DLF_NT) void dlf_pass_kernel(DlfDev F, int dir) {
    const int plane = blockIdx.y;
    if (F.plane_mode[plane] != 2) return;
    const uint32_t pic = blockIdx.z, w = plane ? F.width / 2 : F.width, h = plane ? F.height / 2 : F.height;
    const uint32_t stride = F.dst_stride[plane];
    T* base = (T*)F.dst[plane] + pic * F.dst_pitch[plane];
    const uint32_t* mi = F.mi + pic * F.mi_pitch;
    const uint32_t per_row = dir == 0 ? w / 4 : w, rows = dir == 0 ? h : h / 4;
    const uint32_t t = blockIdx.x * DLF_NT + threadIdx.x;
    if (t >= per_row * rows) return;
    const uint32_t a = t % per_row, b = t / per_row;
    const uint32_t x = dir == 0 ? a * 4 : a, y = dir == 0 ? b : b * 4;
    if ((dir == 0 ? x : y) == 0) return;
    const uint32_t d = dlf_decide(mi, F.mi_stride, plane, dir, x, y);
    if (!d) return;
    const int level = dlf_edge_level(F, d, F.lvl[plane][dir]);
    if (!level) return;
    dlf_filter_line(base + (size_t)y * stride + x, dir == 0 ? 1 : (int)stride, (int)(d & 15u), level, F.sharp, F.sh);
}

template <typename T, bool SEARCH>
struct DlfLds {
    alignas(16) T work[DLF_SIDE * dlf_pitch<T>()];
    alignas(16) T pri[SEARCH ? DLF_SIDE * dlf_pitch<T>() : 4];      // the unfiltered tile, copied to work per level
    alignas(16) T src[SEARCH ? DLF_T * DLF_T : 4];
    uint16_t dec[2][(DLF_SIDE / 4) * DLF_EDGES];                    // [0] vertical edges [row unit][edge], [1] horizontal [edge][column unit]
    unsigned long long red[DLF_NT / 64];
};

// both passes on the tile in L (ts: the tile's side, 64 or 32)
template <typename T, bool SEARCH>
__device__ __forceinline__ void dlf_tile_passes(const DlfDev& F, DlfLds<T, SEARCH>& L, int ts, int base_v, int base_h) {
    constexpr int P = dlf_pitch<T>();
    const int ne = ts / 4 + 1, side = ts + 2 * DLF_H;
    for (int t = threadIdx.x; t < ne * side; t += DLF_NT) {
        const int ex = t % ne, row = t / ne;
        const uint32_t d = L.dec[0][(row >> 2) * DLF_EDGES + ex];
        if (!d) continue;
        const int level = dlf_edge_level(F, d, base_v);
        if (level) dlf_filter_line(&L.work[row * P + DLF_H + 4 * ex], 1, (int)(d & 15u), level, F.sharp, F.sh);
    }
    __syncthreads();
    for (int t = threadIdx.x; t < ne * ts; t += DLF_NT) {
        const int col = t % ts, ey = t / ts;
        const uint32_t d = L.dec[1][ey * DLF_EDGES + (col >> 2)];
        if (!d) continue;
        const int level = dlf_edge_level(F, d, base_h);
        if (level) dlf_filter_line(&L.work[(DLF_H + 4 * ey) * P + DLF_H + col], P, (int)(d & 15u), level, F.sharp, F.sh);
    }
    __syncthreads();
}

// blockIdx.x = tile (raster), .y = plane, .z = picture
template <typename T, bool SEARCH>
__global__ __launch_bounds__(DLF_NT) void dlf_tile_kernel(DlfDev F) {
    constexpr int P = dlf_pitch<T>();
    __shared__ DlfLds<T, SEARCH> L;
    const int plane = blockIdx.y;
    if (!SEARCH && F.plane_mode[plane] == 0) return;
    const uint32_t pic = blockIdx.z, tile = blockIdx.x;
    const int ts = plane ? DLF_T / 2 : DLF_T, side = ts + 2 * DLF_H, ne = ts / 4 + 1;
    const int w = (int)(plane ? F.width / 2 : F.width), h = (int)(plane ? F.height / 2 : F.height);
    const int x0 = (int)(tile % F.ntx) * ts, y0 = (int)(tile / F.ntx) * ts;
    const T* rec = (const T*)F.rec[plane] + pic * F.rec_pitch[plane];
    const uint32_t* mi = F.mi + pic * F.mi_pitch;
    T* first = SEARCH ? L.pri : L.work;
    for (int i = threadIdx.x; i < side * side; i += DLF_NT) {
        const int lx = i % side, ly = i / side, x = x0 - DLF_H + lx, y = y0 - DLF_H + ly;
        first[ly * P + lx] = (x >= 0 && x < w && y >= 0 && y < h) ? rec[(size_t)y * F.rec_stride[plane] + x] : (T)0;
    }
    if (SEARCH) {
        const T* src = (const T*)F.src[plane] + pic * F.src_pitch[plane];
        for (int i = threadIdx.x; i < ts * ts; i += DLF_NT) {
            const int lx = i % ts, ly = i / ts, x = x0 + lx, y = y0 + ly;
            L.src[i] = (x < w && y < h) ? src[(size_t)y * F.src_stride[plane] + x] : (T)0;
        }
    }
    // the decisions, once per tile: vertical edges of every row unit (halo rows included), horizontal edges of the tile's own columns
    const bool decide = SEARCH || F.plane_mode[plane] == 2;
    for (int i = threadIdx.x; decide && i < (side / 4) * ne; i += DLF_NT) {
        const int ex = i % ne, ry = i / ne, x = x0 + 4 * ex, y = y0 - DLF_H + 4 * ry;
        L.dec[0][ry * DLF_EDGES + ex] = (x > 0 && x < w && y >= 0 && y < h) ? (uint16_t)dlf_decide(mi, F.mi_stride, plane, 0, (uint32_t)x, (uint32_t)y) : (uint16_t)0;
    }
    for (int i = threadIdx.x; decide && i < ne * (ts / 4); i += DLF_NT) {
        const int cx = i % (ts / 4), ey = i / (ts / 4), x = x0 + 4 * cx, y = y0 + 4 * ey;
        L.dec[1][ey * DLF_EDGES + cx] = (y > 0 && y < h && x < w) ? (uint16_t)dlf_decide(mi, F.mi_stride, plane, 1, (uint32_t)x, (uint32_t)y) : (uint16_t)0;
    }
    __syncthreads();
    if (!SEARCH) {
        if (F.plane_mode[plane] == 2) dlf_tile_passes<T, SEARCH>(F, L, ts, F.lvl[plane][0], F.lvl[plane][1]);
        T* dst = (T*)F.dst[plane] + pic * F.dst_pitch[plane];
        for (int i = threadIdx.x; i < ts * ts; i += DLF_NT) {
            const int lx = i % ts, ly = i / ts, x = x0 + lx, y = y0 + ly;
            if (x < w && y < h) dst[(size_t)y * F.dst_stride[plane] + x] = L.work[(DLF_H + ly) * P + DLF_H + lx];
        }
        return;
    }
    unsigned long long* out = F.partial + (((size_t)pic * 3 + plane) * ((size_t)F.ntx * F.nty) + tile) * svthost::DLF_LEVELS;
    const unsigned long long mask = F.mask[plane];
    for (int level = 0; level < svthost::DLF_LEVELS; level++) {
        if (!(mask >> level & 1ull)) continue;                 // block-uniform
        const T* res = L.pri;
        if (level) {                                           // level 0: the plane is not filtered (loop_filter_sb's gate)
            constexpr int WORDS = DLF_SIDE * P * (int)sizeof(T) / 4;
            for (int i = threadIdx.x; i < WORDS; i += DLF_NT) ((uint32_t*)L.work)[i] = ((const uint32_t*)L.pri)[i];
            __syncthreads();
            dlf_tile_passes<T, SEARCH>(F, L, ts, level, level);
            res = L.work;
        }
        unsigned long long sum = 0;
        for (int i = threadIdx.x; i < ts * ts; i += DLF_NT) {
            const int lx = i % ts, ly = i / ts;
            if (x0 + lx < w && y0 + ly < h) {
                const int e = (int)res[(DLF_H + ly) * P + DLF_H + lx] - (int)L.src[i];
                sum += (unsigned)(e * e);
            }
        }
        sum = group_sum64<64>(sum);
        if ((threadIdx.x & 63) == 0) L.red[threadIdx.x >> 6] = sum;
        __syncthreads();
        if (threadIdx.x == 0) {
            unsigned long long s = 0;
            for (int i = 0; i < DLF_NT / 64; i++) s += L.red[i];
            out[level] = s;
        }
        __syncthreads();                                       // red and work are reused by the next level
    }
}
static_assert((DLF_SIDE * dlf_pitch<uint8_t>()) % 4 == 0 && (DLF_SIDE * dlf_pitch<uint16_t>() * 2) % 4 == 0, "the per-level copy moves whole words");

// blockIdx.x = picture * 3 + plane; thread = level
__global__ __launch_bounds__(64) void dlf_sum_kernel(DlfDev F) {
    const uint32_t pp = blockIdx.x, plane = pp % 3, level = threadIdx.x;
    const size_t ntiles = (size_t)F.ntx * F.nty;
    unsigned long long s = ~0ull;                              // not computed
    if (F.mask[plane] >> level & 1ull) {
        s = 0;
        const unsigned long long* in = F.partial + (size_t)pp * ntiles * svthost::DLF_LEVELS + level;
        for (size_t t = 0; t < ntiles; t++) s += in[t * svthost::DLF_LEVELS];
    }
    F.sse[(size_t)pp * svthost::DLF_LEVELS + level] = s;
}

struct DlfMiDev {
    const uint32_t* final_blk;       // svt_hip_part_final as three words
    const uint32_t* final_count;
    const uint32_t* info;            // svt_hip_dlf_info as one word
    uint32_t* mi;
    uint32_t npics, nsb, sb_pitch, nsrc, mi_cols, mi_rows, mi_stride;
    unsigned long long mi_pitch;
};

// one wave per (picture, superblock), one lane per final entry
__global__ __launch_bounds__(svthost::DLF_MI_THREADS) void dlf_mi_kernel(DlfMiDev F) {
    const uint32_t unit = blockIdx.x * svthost::DLF_MI_WAVES + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (unit >= F.npics * F.nsb) return;
    const uint32_t pic = unit / F.nsb, sb = unit % F.nsb;
    const size_t slot = (size_t)pic * F.sb_pitch + sb;
    const uint32_t count = final_count_of(F.final_count, slot);
    uint32_t* mi = F.mi + pic * F.mi_pitch;
    for (uint32_t k = lane; k < count; k += 64) {
        const FinalEntry e = final_entry_load(F.final_blk, slot, k);
        const uint32_t src = e.src;
        if (src >= F.nsrc) continue;                           // SVT_HIP_PART_NO_SRC among them
        const uint32_t bsize = kGeomTab.bsize_of[e.mds];       // the md-scan block's size, in 4x4 units on the grid
        const uint32_t c0 = e.x >> 2, r0 = e.y >> 2, nc = kGeomTab.bw[bsize] >> 2, nr = kGeomTab.bh[bsize] >> 2;
        if (c0 + nc > F.mi_cols || r0 + nr > F.mi_rows) continue;
        const uint32_t in = F.info[src];
        const uint32_t rec = bsize | (uint32_t)kGeomTab.tx[bsize] << 8 | ((in & 7u) | ((in >> 16 & 255u) ? 0x80u : 0u)) << 16 | (in >> 8 & 255u) << 24;
        for (uint32_t r = 0; r < nr; r++)
            for (uint32_t c = 0; c < nc; c++) mi[(size_t)(r0 + r) * F.mi_stride + c0 + c] = rec;
    }
}

}  // namespace svtdev

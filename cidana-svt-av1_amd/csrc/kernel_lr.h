// kernel_lr.h — loop restoration of whole pictures: the kernels of svt_hip_lr_apply_frame, svt_hip_lr_try_frame and
// svt_hip_lr_wiener_stats_frame.  The geometry, the halo rule and the launch shapes are lr_plan.h's; reference line numbers are
// EbRestoration.c's unless another file is named.
//
// Filter tiles.  A workgroup of 256 threads filters one tile: the whole height of one stripe (at most 64 rows, 32 in chroma) by 64
// columns (32 for a unit size of 32), so that a tile lies in one unit and the self-guided filter's row parity, which counts from the
// stripe's first row, is the tile's own.  The tile is staged once with its halo of three rows and columns, every halo row read from
// the picture lr_halo_row names and every column clamped to the plane (10 KB of LDS); then
//   Wiener        the horizontal pass over rows + 6 rows into 16-bit intermediates (9 KB), the vertical pass per sample
//   self-guided   per radius the A / B planes of (rows + 2) x (columns + 2) from direct box sums (A 16 bit, B 32 bit: 26 KB), then the
//                 weighted sums per sample; the first pass's result waits in registers while the second reuses the planes
// and every thread ends with the restored values of its 16 samples (column = thread % columns, rows thread / columns + k * 256 /
// columns), which apply stores and try squares against the source.  No filtered sample touches global memory in try.
//
// Statistics.  H = sum over the unit's samples of Y Y^T with Y the win x win window, k-major (column offset outer).  A thread owns one
// pair (a, b), a <= b, of window columns, that is a win x win block of H, and walks down a sample column: one step down brings one new
// sample per window column, so a step costs two LDS reads for win * win multiply-adds.  28 / 15 / 6 pairs times 9 / 17 / 42 sample
// columns side by side fill the workgroup; the threads of a == b also carry M.  Sums are exact in any order: 32-bit partial sums per
// tile (bounds at the loop), 64-bit LDS atomics across the column groups, 64-bit global atomics across the tiles of a unit, and a
// last kernel that divides (10 bit) and mirrors.
#pragma once
#include "dev_common.h"
#include "lr_plan.h"

namespace svtdev {

using svthost::LrPlane;
constexpr int LR_NT = svthost::LR_THREADS, LR_B = svthost::LR_BORDER;
constexpr int LR_TILE = 64;                                 // columns of a tile at the most, and rows (one luma stripe)
constexpr int LR_IN_ROWS = LR_TILE + 2 * LR_B, LR_IN_P = 72; // staged rows, and their pitch in samples
constexpr int LR_AB_P = LR_TILE + 2;                        // pitch of the A / B planes
constexpr int LR_PER_THREAD = LR_TILE * LR_TILE / LR_NT;    // 16 samples a thread

// sgr_params (:163-172), x_by_xplus1 (:742-763), one_by_x[8] and [24] (:765-768)
static __device__ const int8_t kSgrR[16][2] = {{2, 1}, {2, 1}, {2, 1}, {2, 1}, {2, 1}, {2, 1}, {2, 1}, {2, 1}, {2, 1}, {2, 1}, {0, 1}, {0, 1}, {0, 1}, {0, 1}, {2, 0}, {2, 0}};
static __device__ const int16_t kSgrS[16][2] = {{140, 3236}, {112, 2158}, {93, 1618}, {80, 1438}, {70, 1295}, {58, 1177}, {47, 1079}, {37, 996},
                                                {30, 925},   {25, 863},   {-1, 2589}, {-1, 1618}, {-1, 1177}, {-1, 925},  {56, -1},   {22, -1}};
static __device__ const uint16_t kXByXplus1[256] = {
    1,   128, 171, 192, 205, 213, 219, 224, 228, 230, 233, 235, 236, 238, 239, 240, 241, 242, 243, 243, 244, 244, 245, 245, 246, 246, 247, 247, 247, 247,
    248, 248, 248, 248, 249, 249, 249, 249, 249, 250, 250, 250, 250, 250, 250, 250, 251, 251, 251, 251, 251, 251, 251, 251, 251, 251, 252, 252, 252, 252,
    252, 252, 252, 252, 252, 252, 252, 252, 252, 252, 252, 252, 252, 253, 253, 253, 253, 253, 253, 253, 253, 253, 253, 253, 253, 253, 253, 253, 253, 253,
    253, 253, 253, 253, 253, 253, 253, 253, 253, 253, 253, 253, 254, 254, 254, 254, 254, 254, 254, 254, 254, 254, 254, 254, 254, 254, 254, 254, 254, 254,
    254, 254, 254, 254, 254, 254, 254, 254, 254, 254, 254, 254, 254, 254, 254, 254, 254, 254, 254, 254, 254, 254, 254, 254, 254, 254, 254, 254, 254, 254,
    254, 254, 254, 254, 254, 254, 254, 254, 254, 254, 254, 254, 254, 254, 254, 254, 254, 254, 254, 254, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255,
    255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255,
    255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255,
    255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 255, 256};
constexpr uint32_t kOneBy9 = 455, kOneBy25 = 164;

struct LrDev {
    const void* cdef[3]; const void* dblk[3]; const void* src[3]; void* dst[3];
    uint32_t cdef_stride[3], dblk_stride[3], src_stride[3], dst_stride[3];
    unsigned long long cdef_pitch[3], dblk_pitch[3], src_pitch[3], dst_pitch[3];
    LrPlane pl[3];
    int bd;
    uint32_t npics, units_per_pic;
    int ftype[3];                               // apply
    const uint32_t* units;                      // svt_hip_lr_unit as six words
    const uint32_t* cand; uint32_t try_tiles; unsigned long long* sse;             // try: svt_hip_lr_cand as nine words
    int win[3]; long long* M; long long* H; uint32_t* avg; uint32_t stats_tiles;   // statistics
};

// a record with every field inside its range; ftype: the plane's frame type, or 3 for "any"
struct LrRec { int type, ep; int vf[3], hf[3], xqd[2]; };
__device__ __forceinline__ LrRec lr_rec(const uint32_t* w, int ftype) {
    LrRec r;
    const int type = (int)w[0];
    r.type = (type < 1 || type > 2 || ftype == 0 || (ftype != 3 && ftype != type)) ? 0 : type;
    const int v[8] = {(int16_t)(w[1] & 0xffff), (int16_t)(w[1] >> 16), (int16_t)(w[2] & 0xffff), (int16_t)(w[2] >> 16),
                      (int16_t)(w[3] & 0xffff), (int16_t)(w[3] >> 16), (int16_t)(w[4] & 0xffff), (int16_t)(w[4] >> 16)};
#pragma unroll
    for (int i = 0; i < 3; i++) {
        r.vf[i] = svthost::lr_clamp(v[i], svthost::kLrTapMin[i], svthost::kLrTapMax[i]);
        r.hf[i] = svthost::lr_clamp(v[3 + i], svthost::kLrTapMin[i], svthost::kLrTapMax[i]);
    }
    r.xqd[0] = svthost::lr_clamp(v[6], svthost::kLrXqdMin[0], svthost::kLrXqdMax[0]);
    r.xqd[1] = svthost::lr_clamp(v[7], svthost::kLrXqdMin[1], svthost::kLrXqdMax[1]);
    r.ep = svthost::lr_clamp((int)w[5], 0, 15);
    return r;
}

template <typename T>
struct LrLds {
    T in[LR_IN_ROWS * LR_IN_P];
    union {
        uint16_t tmp[LR_IN_ROWS * LR_TILE];                                      // Wiener: the horizontal pass
        struct { uint32_t B[LR_AB_P * LR_AB_P]; uint16_t A[LR_AB_P * LR_AB_P]; } ab;      // self-guided
    };
    unsigned long long red[LR_NT / 64];
};

__device__ __forceinline__ uint32_t lr_rpot(uint32_t v, int n) { return (v + ((1u << n) >> 1)) >> n; }

// the tile's samples with their halo: rows y0 - 3 .. y1 + 2, columns x0 - 3 .. x0 + tw + 2.  CDEF_ONLY: the halo rule of the parameter
// search (kernel_lr_sgr.h), every row a row of the CDEF picture clamped to the plane; the deblocked picture is not touched
template <typename T, bool CDEF_ONLY = false>
__device__ __forceinline__ void lr_stage(const LrDev& F, LrLds<T>& L, int plane, uint32_t pic, int x0, int tw, int y0, int y1) {
    const LrPlane& P = F.pl[plane];
    const T* cdef = (const T*)F.cdef[plane] + pic * F.cdef_pitch[plane];
    const T* dblk = (const T*)F.dblk[plane] + pic * F.dblk_pitch[plane];
    const int cols = tw + 2 * LR_B, n = (y1 - y0 + 2 * LR_B) * cols;
    for (int i = threadIdx.x; i < n; i += LR_NT) {
        const int lx = i % cols, ly = i / cols;
        const svthost::LrRow hr = CDEF_ONLY ? svthost::LrRow{svthost::lr_clamp(y0 - LR_B + ly, 0, P.h - 1), false} : svthost::lr_halo_row(y0 - LR_B + ly, y0, y1, P.h);
        const int x = svthost::lr_clamp(x0 - LR_B + lx, 0, P.w - 1);
        L.in[ly * LR_IN_P + lx] = hr.dblk ? dblk[(size_t)hr.row * F.dblk_stride[plane] + x] : cdef[(size_t)hr.row * F.cdef_stride[plane] + x];
    }
}

// A and B of one radius (selfguided_restoration_[fast_]internal, :793-863 / :926-996) at rows -1 .. rows, columns -1 .. tw of the tile;
// FAST: every other row from -1
template <typename T, bool FAST>
__device__ __forceinline__ void lr_sgr_ab(LrLds<T>& L, int tw, int rows, int r, uint32_t s, int bd) {
    const int cols = tw + 2, nrows = FAST ? (rows + 3) / 2 : rows + 2;
    const uint32_t nn = (uint32_t)((2 * r + 1) * (2 * r + 1)), one_by = r == 2 ? kOneBy25 : kOneBy9;
    for (int i = threadIdx.x; i < nrows * cols; i += LR_NT) {
        const int j = i % cols, m = i / cols, ai = FAST ? 2 * m : m;      // ai, j: the A / B planes' own indices (sample row ai - 1, column j - 1)
        uint32_t sum = 0, sq = 0;
        for (int dy = -r; dy <= r; dy++)
            for (int dx = -r; dx <= r; dx++) {
                const uint32_t v = L.in[(ai - 1 + LR_B + dy) * LR_IN_P + (j - 1 + LR_B + dx)];
                sum += v; sq += v * v;
            }
        const uint32_t a = lr_rpot(sq, 2 * (bd - 8)), b = lr_rpot(sum, bd - 8);
        const uint32_t p = (a * nn < b * b) ? 0u : a * nn - b * b;
        const uint32_t z = lr_rpot(p * s, 20);                          // SGRPROJ_MTABLE_BITS
        const uint32_t A = kXByXplus1[z < 255 ? z : 255];
        L.ab.A[ai * LR_AB_P + j] = (uint16_t)A;
        L.ab.B[ai * LR_AB_P + j] = lr_rpot((256u - A) * sum * one_by, 12);      // SGRPROJ_SGR, SGRPROJ_RECIP_BITS
    }
}

// The two passes of the self-guided filter (selfguided_restoration_fast_internal, :770-900; selfguided_restoration_internal, :902-1020)
// on a staged tile, for the projection of apply / try (lr_filter_tile) and for the parameter search (kernel_lr_sgr.h).
// lr_sgr_pass0: r[0] > 0 only; flt0[k] = the first pass at column threadIdx.x % tw, row threadIdx.x / tw + k * (256 / tw); it ends with
// a barrier, after which the A / B planes may be rewritten.  lr_sgr_pass1_ab: r[1] > 0 only; the second pass's planes, ready for
// lr_sgr_flt1 (one sample; px: the staged sample).  Every thread of the workgroup calls the first two.
template <typename T>
__device__ __forceinline__ void lr_sgr_pass0(LrLds<T>& L, int ep, int bd, int tw, int rows, int flt0[LR_PER_THREAD]) {
    const int col = threadIdx.x % tw, row0 = threadIdx.x / tw, rstep = LR_NT / tw;
    lr_sgr_ab<T, true>(L, tw, rows, kSgrR[ep][0], (uint32_t)kSgrS[ep][0], bd);
    __syncthreads();
#pragma unroll
    for (int k = 0; k < LR_PER_THREAD; k++) {
        const int row = row0 + k * rstep;
        flt0[k] = 0;
        if (row < rows) {
            const int c = (row + 1) * LR_AB_P + col + 1, px = (int)L.in[(row + LR_B) * LR_IN_P + col + LR_B];
            const uint16_t* A = L.ab.A; const uint32_t* B = L.ab.B;
            if (!(row & 1)) {      // even row: the A / B rows above and below
                const int a = ((int)A[c - LR_AB_P] + (int)A[c + LR_AB_P]) * 6 +
                              ((int)A[c - 1 - LR_AB_P] + (int)A[c - 1 + LR_AB_P] + (int)A[c + 1 - LR_AB_P] + (int)A[c + 1 + LR_AB_P]) * 5;
                const int b = ((int)B[c - LR_AB_P] + (int)B[c + LR_AB_P]) * 6 +
                              ((int)B[c - 1 - LR_AB_P] + (int)B[c - 1 + LR_AB_P] + (int)B[c + 1 - LR_AB_P] + (int)B[c + 1 + LR_AB_P]) * 5;
                flt0[k] = (a * px + b + (1 << 8)) >> 9;
            } else {
                const int a = (int)A[c] * 6 + ((int)A[c - 1] + (int)A[c + 1]) * 5;
                const int b = (int)B[c] * 6 + ((int)B[c - 1] + (int)B[c + 1]) * 5;
                flt0[k] = (a * px + b + (1 << 7)) >> 8;
            }
        }
    }
    __syncthreads();                                                // the planes are reused
}
template <typename T>
__device__ __forceinline__ void lr_sgr_pass1_ab(LrLds<T>& L, int ep, int bd, int tw, int rows) {
    lr_sgr_ab<T, false>(L, tw, rows, kSgrR[ep][1], (uint32_t)kSgrS[ep][1], bd);
    __syncthreads();
}
template <typename T>
__device__ __forceinline__ int lr_sgr_flt1(const LrLds<T>& L, int row, int col, int px) {
    const int c = (row + 1) * LR_AB_P + col + 1;
    const uint16_t* A = L.ab.A; const uint32_t* B = L.ab.B;
    const int a = ((int)A[c] + (int)A[c - 1] + (int)A[c + 1] + (int)A[c - LR_AB_P] + (int)A[c + LR_AB_P]) * 4 +
                  ((int)A[c - 1 - LR_AB_P] + (int)A[c - 1 + LR_AB_P] + (int)A[c + 1 - LR_AB_P] + (int)A[c + 1 + LR_AB_P]) * 3;
    const int b = ((int)B[c] + (int)B[c - 1] + (int)B[c + 1] + (int)B[c - LR_AB_P] + (int)B[c + LR_AB_P]) * 4 +
                  ((int)B[c - 1 - LR_AB_P] + (int)B[c - 1 + LR_AB_P] + (int)B[c + 1 - LR_AB_P] + (int)B[c + 1 + LR_AB_P]) * 3;
    return (a * px + b + (1 << 8)) >> 9;
}

// Filters the staged tile under record R: out[k] = the restored sample at column threadIdx.x % tw, row threadIdx.x / tw + k * (256 /
// tw), for the rows below `rows`.  Every thread of the workgroup calls it (it synchronises).
template <typename T>
__device__ __forceinline__ void lr_filter_tile(LrLds<T>& L, const LrRec& R, int bd, int tw, int rows, int out[LR_PER_THREAD]) {
    const int col = threadIdx.x % tw, row0 = threadIdx.x / tw, rstep = LR_NT / tw, maxv = (1 << bd) - 1;
    __syncthreads();                                                    // the staged tile
    if (R.type == 0) {
#pragma unroll
        for (int k = 0; k < LR_PER_THREAD; k++) {
            const int row = row0 + k * rstep;
            out[k] = row < rows ? (int)L.in[(row + LR_B) * LR_IN_P + col + LR_B] : 0;
        }
        return;
    }
    if (R.type == 1) {
        // av1_[highbd_]wiener_convolve_add_src_c (convolve.c:64-143, 145-230): round_0 3, round_1 11 at 8 and 10 bit
        const int hc = -2 * (R.hf[0] + R.hf[1] + R.hf[2]), vc = -2 * (R.vf[0] + R.vf[1] + R.vf[2]);
        const int hlim = (1 << (bd + 1 + 7 - 3)) - 1;
        for (int i = threadIdx.x; i < (rows + 2 * LR_B) * tw; i += LR_NT) {
            const int lx = i % tw, ly = i / tw;
            const T* s = &L.in[ly * LR_IN_P + lx];
            int sum = R.hf[0] * ((int)s[0] + (int)s[6]) + R.hf[1] * ((int)s[1] + (int)s[5]) + R.hf[2] * ((int)s[2] + (int)s[4]) + hc * (int)s[3];
            sum += ((int)s[3] << 7) + (1 << (bd + 6));
            L.tmp[ly * LR_TILE + lx] = (uint16_t)svthost::lr_clamp((sum + 4) >> 3, 0, hlim);
        }
        __syncthreads();
#pragma unroll
        for (int k = 0; k < LR_PER_THREAD; k++) {
            const int row = row0 + k * rstep;
            out[k] = 0;
            if (row < rows) {
                const uint16_t* s = &L.tmp[row * LR_TILE + col];
                int sum = R.vf[0] * ((int)s[0] + (int)s[6 * LR_TILE]) + R.vf[1] * ((int)s[LR_TILE] + (int)s[5 * LR_TILE]) +
                          R.vf[2] * ((int)s[2 * LR_TILE] + (int)s[4 * LR_TILE]) + vc * (int)s[3 * LR_TILE];
                sum += ((int)s[3 * LR_TILE] << 7) - (1 << (bd + 10));
                out[k] = svthost::lr_clamp((sum + 1024) >> 11, 0, maxv);
            }
        }
        return;
    }
    // apply_selfguided_restoration_c (:1062-1099)
    const int r0 = kSgrR[R.ep][0], r1 = kSgrR[R.ep][1];
    int flt0[LR_PER_THREAD];
    if (r0 > 0) lr_sgr_pass0<T>(L, R.ep, bd, tw, rows, flt0);
    // decode_xq (:727-740)
    int xq0, xq1;
    if (r0 == 0) { xq0 = 0; xq1 = 128 - R.xqd[1]; }
    else if (r1 == 0) { xq0 = R.xqd[0]; xq1 = 0; }
    else { xq0 = R.xqd[0]; xq1 = 128 - xq0 - R.xqd[1]; }
    if (r1 > 0) lr_sgr_pass1_ab<T>(L, R.ep, bd, tw, rows);
#pragma unroll
    for (int k = 0; k < LR_PER_THREAD; k++) {
        const int row = row0 + k * rstep;
        out[k] = 0;
        if (row < rows) {
            const int px = (int)L.in[(row + LR_B) * LR_IN_P + col + LR_B];
            const int u = px << 4;                                      // SGRPROJ_RST_BITS
            int v = u << 7;                                             // SGRPROJ_PRJ_BITS
            if (r0 > 0) v += xq0 * (flt0[k] - u);
            if (r1 > 0) {
                const int flt1 = lr_sgr_flt1<T>(L, row, col, px);
                v += xq1 * (flt1 - u);
            }
            out[k] = svthost::lr_clamp((int)(int16_t)((v + (1 << 10)) >> 11), 0, maxv);
        }
    }
}

// blockIdx.x = tile (tile column + stripe * ntx), .y = plane, .z = picture
template <typename T>
__global__ __launch_bounds__(LR_NT) void lr_apply_kernel(LrDev F) {
    __shared__ LrLds<T> L;
    const int plane = blockIdx.y;
    const LrPlane& P = F.pl[plane];
    const uint32_t pic = blockIdx.z;
    const int tx = (int)(blockIdx.x % (uint32_t)P.ntx), s = (int)(blockIdx.x / (uint32_t)P.ntx);
    if (s >= P.nstripes) return;
    const int x0 = tx * P.tw, y0 = svthost::lr_stripe_start(s, P.ss), y1 = svthost::lr_stripe_end(s, P.ss, P.h);
    const int uj = svthost::lr_unit_of(x0, P.nh, P.us, 0), ui = svthost::lr_unit_of(y0, P.nv, P.us, svthost::lr_stripe_off(P.ss));
    const LrRec R = lr_rec(F.units + ((size_t)pic * F.units_per_pic + P.unit0 + (uint32_t)(ui * P.nh + uj)) * 6, F.ftype[plane]);
    lr_stage<T>(F, L, plane, pic, x0, P.tw, y0, y1);
    int out[LR_PER_THREAD];
    lr_filter_tile<T>(L, R, F.bd, P.tw, y1 - y0, out);
    T* dst = (T*)F.dst[plane] + pic * F.dst_pitch[plane];
    const int col = threadIdx.x % P.tw, row0 = threadIdx.x / P.tw, rstep = LR_NT / P.tw;
#pragma unroll
    for (int k = 0; k < LR_PER_THREAD; k++) {
        const int row = row0 + k * rstep;
        if (row < y1 - y0 && x0 + col < P.w) dst[(size_t)(y0 + row) * F.dst_stride[plane] + x0 + col] = (T)out[k];
    }
}

__global__ __launch_bounds__(LR_NT) void lr_zero_kernel(unsigned long long* p, size_t n) {
    const size_t i = (size_t)blockIdx.x * LR_NT + threadIdx.x;
    if (i < n) p[i] = 0;
}

// blockIdx.x = candidate * try_tiles + tile of the candidate's unit
template <typename T>
__global__ __launch_bounds__(LR_NT) void lr_try_kernel(LrDev F) {
    __shared__ LrLds<T> L;
    const uint32_t c = blockIdx.x / F.try_tiles, t = blockIdx.x % F.try_tiles;
    const uint32_t* cw = F.cand + (size_t)c * 9;
    const uint32_t pic = cw[0], plane = cw[1], unit = cw[2];
    if (pic >= F.npics || plane >= 3 || unit >= (uint32_t)(F.pl[plane < 3 ? plane : 0].nh * F.pl[plane < 3 ? plane : 0].nv)) {
        if (t == 0 && threadIdx.x == 0) F.sse[c] = 0x7fffffffffffffffull;
        return;
    }
    const LrPlane& P = F.pl[plane];
    const int off = svthost::lr_stripe_off(P.ss), ui = (int)unit / P.nh, uj = (int)unit % P.nh;
    const int hs = svthost::lr_unit_start(uj, P.us, 0), he = svthost::lr_unit_end(uj, P.nh, P.us, 0, P.w);
    const int vs = svthost::lr_unit_start(ui, P.us, off), ve = svthost::lr_unit_end(ui, P.nv, P.us, off, P.h);
    const int tiles_x = (he - hs + P.tw - 1) / P.tw, s0 = svthost::lr_stripe_of(vs, P.ss), ns = svthost::lr_stripe_of(ve - 1, P.ss) - s0 + 1;
    const int tx = (int)t % tiles_x, s = s0 + (int)t / tiles_x;
    if ((int)t / tiles_x >= ns) return;
    const int x0 = hs + tx * P.tw;
    const int y0 = svthost::lr_max(svthost::lr_stripe_start(s, P.ss), vs), y1 = svthost::lr_min(svthost::lr_stripe_end(s, P.ss, P.h), ve);
    const LrRec R = lr_rec(cw + 3, 3);
    lr_stage<T>(F, L, (int)plane, pic, x0, P.tw, y0, y1);
    int out[LR_PER_THREAD];
    lr_filter_tile<T>(L, R, F.bd, P.tw, y1 - y0, out);
    const T* src = (const T*)F.src[plane] + pic * F.src_pitch[plane];
    const int col = threadIdx.x % P.tw, row0 = threadIdx.x / P.tw, rstep = LR_NT / P.tw;
    unsigned long long sum = 0;
#pragma unroll
    for (int k = 0; k < LR_PER_THREAD; k++) {
        const int row = row0 + k * rstep;
        if (row < y1 - y0 && x0 + col < he) {
            const int e = out[k] - (int)src[(size_t)(y0 + row) * F.src_stride[plane] + x0 + col];
            sum += (unsigned)(e * e);
        }
    }
    sum = group_sum64<64>(sum);
    if ((threadIdx.x & 63) == 0) L.red[threadIdx.x >> 6] = sum;
    __syncthreads();
    if (threadIdx.x == 0) {
        unsigned long long tot = 0;
        for (int i = 0; i < LR_NT / 64; i++) tot += L.red[i];
        atomicAdd(&F.sse[c], tot);
    }
}

// ---- Wiener statistics ----------------------------------------------------------------------------------------------------------
struct LrUnitRect { int plane, hs, he, vs, ve; };
__device__ __forceinline__ LrUnitRect lr_unit_rect(const LrDev& F, uint32_t u) {      // u: index inside a picture's block
    LrUnitRect r;
    r.plane = u >= F.pl[2].unit0 ? 2 : (u >= F.pl[1].unit0 ? 1 : 0);
    const LrPlane& P = F.pl[r.plane];
    const int k = (int)(u - P.unit0), ui = k / P.nh, uj = k % P.nh, off = svthost::lr_stripe_off(P.ss);
    r.hs = svthost::lr_unit_start(uj, P.us, 0); r.he = svthost::lr_unit_end(uj, P.nh, P.us, 0, P.w);
    r.vs = svthost::lr_unit_start(ui, P.us, off); r.ve = svthost::lr_unit_end(ui, P.nv, P.us, off, P.h);
    return r;
}

// find_average (EbRestorationPick.h:33): blockIdx.x = picture * units_per_pic + unit
template <typename T>
__global__ __launch_bounds__(LR_NT) void lr_avg_kernel(LrDev F) {
    __shared__ unsigned long long red[LR_NT / 64];
    const uint32_t pic = blockIdx.x / F.units_per_pic, u = blockIdx.x % F.units_per_pic;
    const LrUnitRect r = lr_unit_rect(F, u);
    const T* cdef = (const T*)F.cdef[r.plane] + pic * F.cdef_pitch[r.plane];
    const int w = r.he - r.hs, n = w * (r.ve - r.vs);
    unsigned long long sum = 0;
    for (int i = threadIdx.x; i < n; i += LR_NT) sum += cdef[(size_t)(r.vs + i / w) * F.cdef_stride[r.plane] + r.hs + i % w];
    sum = group_sum64<64>(sum);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = sum;
    __syncthreads();
    if (threadIdx.x == 0) {
        unsigned long long tot = 0;
        for (int i = 0; i < LR_NT / 64; i++) tot += red[i];
        F.avg[blockIdx.x] = (uint32_t)(tot / (unsigned long long)n);
    }
}

template <int WIN>
struct LrStatsLds {
    int16_t y[LR_IN_ROWS * LR_IN_P];                         // d_cdef - avg with the window's halo
    int16_t x[LR_TILE * LR_TILE];                            // d_src - avg
    unsigned long long h[(WIN * (WIN + 1) / 2) * WIN * WIN];
    unsigned long long m[WIN * WIN];
};

// blockIdx.x = (picture * units_per_pic + unit) * stats_tiles + tile; the unit's plane must have window WIN (others leave)
template <typename T, int WIN>
__global__ __launch_bounds__(LR_NT) void lr_stats_kernel(LrDev F) {
    constexpr int HALF = WIN / 2, NP = WIN * (WIN + 1) / 2, G = LR_NT / NP, WIN2 = WIN * WIN, SH = LR_B - HALF;
    __shared__ LrStatsLds<WIN> L;
    const uint32_t pu = blockIdx.x / F.stats_tiles, t = blockIdx.x % F.stats_tiles;
    const uint32_t pic = pu / F.units_per_pic, u = pu % F.units_per_pic;
    const LrUnitRect r = lr_unit_rect(F, u);
    if (F.win[r.plane] != WIN) return;
    const LrPlane& P = F.pl[r.plane];
    const int tiles_x = (r.he - r.hs + LR_TILE - 1) / LR_TILE, tx = (int)t % tiles_x, ty = (int)t / tiles_x;
    const int x0 = r.hs + tx * LR_TILE, y0 = r.vs + ty * LR_TILE;
    if (y0 >= r.ve) return;
    const int cols = svthost::lr_min(LR_TILE, r.he - x0), rows = svthost::lr_min(LR_TILE, r.ve - y0);
    const int avg = (int)F.avg[pu];
    const T* cdef = (const T*)F.cdef[r.plane] + pic * F.cdef_pitch[r.plane];
    const T* src = (const T*)F.src[r.plane] + pic * F.src_pitch[r.plane];
    for (int i = threadIdx.x; i < (rows + 2 * LR_B) * (cols + 2 * LR_B); i += LR_NT) {
        const int lx = i % (cols + 2 * LR_B), ly = i / (cols + 2 * LR_B);
        const int x = svthost::lr_clamp(x0 - LR_B + lx, 0, P.w - 1), y = svthost::lr_clamp(y0 - LR_B + ly, 0, P.h - 1);
        L.y[ly * LR_IN_P + lx] = (int16_t)((int)cdef[(size_t)y * F.cdef_stride[r.plane] + x] - avg);
    }
    for (int i = threadIdx.x; i < rows * cols; i += LR_NT) {
        const int lx = i % cols, ly = i / cols;
        L.x[ly * LR_TILE + lx] = (int16_t)((int)src[(size_t)(y0 + ly) * F.src_stride[r.plane] + x0 + lx] - avg);
    }
    for (int i = threadIdx.x; i < NP * WIN2; i += LR_NT) L.h[i] = 0;
    for (int i = threadIdx.x; i < WIN2; i += LR_NT) L.m[i] = 0;
    __syncthreads();
    const int g = threadIdx.x / NP;
    int p = threadIdx.x % NP, a = 0;
    while (p >= WIN - a) { p -= WIN - a; a++; }
    const int b = a + p;
    if (g < G) {
        // 32-bit partial sums: a thread adds at most 64 rows x ceil(64 / G) columns = 512 (7x7), 256 (5x5), 128 (3x3) terms per
        // accumulator, each |Y Y| <= 65 025 at 8 bit (room for 33 025 terms) and <= 1 046 529 at 10 bit (room for 2 052 terms)
        static_assert(LR_TILE * ((LR_TILE + G - 1) / G) <= 2052, "an int32 accumulator would overflow at 10 bit");
        int acc[WIN2], m[WIN];
#pragma unroll
        for (int i = 0; i < WIN2; i++) acc[i] = 0;
#pragma unroll
        for (int i = 0; i < WIN; i++) m[i] = 0;
        for (int col = g; col < cols; col += G) {
            int ya[WIN], yb[WIN];
            const int16_t* ca = &L.y[SH * LR_IN_P + col + SH + a];
            const int16_t* cb = &L.y[SH * LR_IN_P + col + SH + b];
#pragma unroll
            for (int i = 1; i < WIN; i++) { ya[i] = ca[(i - 1) * LR_IN_P]; yb[i] = cb[(i - 1) * LR_IN_P]; }
            for (int row = 0; row < rows; row++) {
#pragma unroll
                for (int i = 0; i < WIN - 1; i++) { ya[i] = ya[i + 1]; yb[i] = yb[i + 1]; }
                ya[WIN - 1] = ca[(row + WIN - 1) * LR_IN_P];
                yb[WIN - 1] = cb[(row + WIN - 1) * LR_IN_P];
#pragma unroll
                for (int i = 0; i < WIN; i++)
#pragma unroll
                    for (int j = 0; j < WIN; j++) acc[i * WIN + j] += ya[i] * yb[j];
                if (a == b) {
                    const int x = L.x[row * LR_TILE + col];
#pragma unroll
                    for (int i = 0; i < WIN; i++) m[i] += ya[i] * x;
                }
            }
        }
        const int pair = (int)(threadIdx.x % NP);
#pragma unroll
        for (int i = 0; i < WIN2; i++) atomicAdd(&L.h[pair * WIN2 + i], (unsigned long long)(long long)acc[i]);
        if (a == b)
#pragma unroll
            for (int i = 0; i < WIN; i++) atomicAdd(&L.m[a * WIN + i], (unsigned long long)(long long)m[i]);
    }
    __syncthreads();
    // the tile's sums into the unit's: block (a, b) entry (i, j) is H[a * WIN + i][b * WIN + j]
    unsigned long long* H = (unsigned long long*)F.H + (size_t)pu * (svthost::LR_WIN2 * svthost::LR_WIN2);
    unsigned long long* M = (unsigned long long*)F.M + (size_t)pu * svthost::LR_WIN2;
    for (int i = threadIdx.x; i < NP * WIN2; i += LR_NT) {
        int pp = i / WIN2, aa = 0;
        while (pp >= WIN - aa) { pp -= WIN - aa; aa++; }
        const int bb = aa + pp, e = i % WIN2;
        atomicAdd(&H[(aa * WIN + e / WIN) * WIN2 + bb * WIN + e % WIN], L.h[i]);
    }
    for (int i = threadIdx.x; i < WIN2; i += LR_NT) atomicAdd(&M[i], L.m[i]);
}

// the truncating division at 10 bit and the mirror (EbRestorationPick.c:799-803, :850-857): blockIdx.x = picture * units_per_pic + unit
__global__ __launch_bounds__(LR_NT) void lr_stats_finish_kernel(LrDev F) {
    const uint32_t pu = blockIdx.x, u = pu % F.units_per_pic;
    const LrUnitRect r = lr_unit_rect(F, u);
    const int win2 = F.win[r.plane] * F.win[r.plane];
    const long long div = F.bd == 10 ? 4 : 1;
    long long* H = F.H + (size_t)pu * (svthost::LR_WIN2 * svthost::LR_WIN2);
    long long* M = F.M + (size_t)pu * svthost::LR_WIN2;
    for (int i = threadIdx.x; i < win2; i += LR_NT) M[i] /= div;
    for (int i = threadIdx.x; i < win2 * win2; i += LR_NT) {
        const int k = i / win2, l = i % win2;
        if (k <= l) {
            const long long v = H[k * win2 + l] / div;
            H[k * win2 + l] = v;
            H[l * win2 + k] = v;
        }
    }
}

}  // namespace svtdev

// kernel_me_subpel.h — sub-pel motion estimation: the half- and quarter-pel refinement of MotionEstimateLcu (EbMotionEstimation.c:8162-8236)
// and BiPredictionSearch on the refined vectors (:6210-6632), for every SB of a picture or of a stack of pictures (svt_hip_me_subpel.hip):
//   me_subpel_refine_kernel  one workgroup per (SB, reference list, picture): InterpolateSearchRegionAVC (:3409, the AVCCODEL branch),
//                            HalfPelSearch_LCU (:3829) and QuarterPelSearch_LCU (:4746) on the SB's result rows, in place
//   me_subpel_bipred_kernel  one workgroup per (SB, picture): BiPredictionCompensation / BiPredAverging / SelectBuffer /
//                            QuarterPelCompensation on the fractional vectors of both lists, and the me_results rows (me_result_row)
//   me_subpel_planes_kernel  the three half-pel planes of a window by themselves, for pinning the interpolation
//
// The planes.  With I the reference's integer samples at absolute picture coordinates and f the taps (-2, 18, 18, -2), + 16 >> 5, clipped
// to 8 bits (the frac_pos = 2 row of AvcStyleLumaIFCoeff8_SSSE3):
//   B(y, x) = f(I[y][x - 2 .. x + 1])     the half-pel sample LEFT of (y, x)
//   H(y, x) = f(I[y - 2 .. y + 1][x])     the half-pel sample ABOVE (y, x)
//   J(y, x) = f(B[y - 2 .. y + 1][x])     above-left of (y, x): the vertical filter over the ROUNDED plane B, not a 2-D filter on I
// The reference's pos_b / pos_h / pos_j pointers of a search area (its call site hands on pos_b + 2 * stride, pos_h + 1, pos_j + 0,
// :8194-8201) hold exactly B / H / J at the absolute position of each search point, so nothing here depends on the search area but the
// vectors themselves: the planes are computed per PU around its winner, never for a whole window.
//
// Mapping: a wave owns one PU at a time.  It stages the integer samples of the PU's block at the full-pel winner with 2 samples before and
// 3 after it into its own LDS window (69 x 69 at most), computes plane B of those rows next to it, and takes H and J from the two on the
// fly (four LDS reads and one filter each).  A candidate's distortion is summed over the PU's samples strided over the 64 lanes and
// reduced over the wave; the running best is then updated in the reference's order with strict '<' by every lane alike.
#pragma once
#include "kernel_me_steps.h"
#include "me_subpel_plan.h"

namespace svtdev {

using svthost::ME_SP_BW;
using svthost::ME_SP_IW;
using svthost::ME_SP_MARGIN;
using svthost::ME_SP_THREADS;
using svthost::ME_SP_WAVE_LDS;
using svthost::ME_SP_WAVES;
using svthost::ME_SP_WIN;
static_assert(ME_SP_THREADS == ME_THREADS, "the bi-prediction shares me_result_row's numbering");

struct MeSubpelDev {
    const uint8_t* src;                 // sample (0, 0) of the source's full-resolution luma picture
    const uint8_t* ref[2];              // the same of list 0 / list 1
    uint32_t src_stride, ref_stride[2];
    unsigned long long src_pitch, ref_pitch[2];           // bytes between the pictures of a stack
    int32_t width, height;
    int32_t nlists, npus, method;       // fractional_search_method: 0 every other row, doubled; 1 every row; 2 SSE decides
    int32_t f64, h32, h16, h8, qp, no8; // fractional_search64x64, the three half-pel enables, the quarter-pel enable, disable8x8CuInMeFlag
    uint32_t nsbx, nsb;
};

enum { SP_F = 0, SP_B = 1, SP_H = 2, SP_J = 3 };
// a plane sample relative to a window's base position: kind | (dy + 1) << 2 | (dx + 1) << 4
constexpr unsigned sp_at(int kind, int dy, int dx) { return (unsigned)kind | (unsigned)(dy + 1) << 2 | (unsigned)(dx + 1) << 4; }
// the eight neighbours in the order the reference tries them: L R T B TL TR BR BL
__device__ constexpr int8_t kSpDx[8] = {-1, 1, 0, 0, -1, 1, 1, -1}, kSpDy[8] = {0, 0, -1, 1, -1, -1, 1, 1};
// psubPelDirection of each neighbour (TOP_LEFT 0, TOP 1, TOP_RIGHT 2, RIGHT 3, BOTTOM_RIGHT 4, BOTTOM 5, BOTTOM_LEFT 6, LEFT 7) and the order
// in which the reference looks for the first equality with the minimum: L R T B TL TR BL BR (:3795-3821), as neighbour indices
__device__ constexpr uint8_t kSpDir[8] = {7, 3, 1, 5, 0, 2, 4, 6}, kSpDirOrder[8] = {0, 1, 2, 3, 4, 5, 7, 6};
// SetQuarterPelRefinementInputsOnTheFly (:4655): [case (y & 2) + ((x & 2) >> 1)][neighbour][the two planes averaged], at ((mv + 2) >> 2)
__device__ constexpr uint8_t kSpQuarter[4][8][2] = {
    {{sp_at(SP_B, 0, 0), sp_at(SP_F, 0, 0)}, {sp_at(SP_F, 0, 0), sp_at(SP_B, 0, 1)}, {sp_at(SP_H, 0, 0), sp_at(SP_F, 0, 0)}, {sp_at(SP_F, 0, 0), sp_at(SP_H, 1, 0)},
     {sp_at(SP_B, 0, 0), sp_at(SP_H, 0, 0)}, {sp_at(SP_H, 0, 0), sp_at(SP_B, 0, 1)}, {sp_at(SP_H, 1, 0), sp_at(SP_B, 0, 1)}, {sp_at(SP_B, 0, 0), sp_at(SP_H, 1, 0)}},
    {{sp_at(SP_F, 0, -1), sp_at(SP_B, 0, 0)}, {sp_at(SP_B, 0, 0), sp_at(SP_F, 0, 0)}, {sp_at(SP_J, 0, 0), sp_at(SP_B, 0, 0)}, {sp_at(SP_B, 0, 0), sp_at(SP_J, 1, 0)},
     {sp_at(SP_H, 0, -1), sp_at(SP_B, 0, 0)}, {sp_at(SP_B, 0, 0), sp_at(SP_H, 0, 0)}, {sp_at(SP_B, 0, 0), sp_at(SP_H, 1, 0)}, {sp_at(SP_H, 1, -1), sp_at(SP_B, 0, 0)}},
    {{sp_at(SP_J, 0, 0), sp_at(SP_H, 0, 0)}, {sp_at(SP_H, 0, 0), sp_at(SP_J, 0, 1)}, {sp_at(SP_F, -1, 0), sp_at(SP_H, 0, 0)}, {sp_at(SP_H, 0, 0), sp_at(SP_F, 0, 0)},
     {sp_at(SP_B, -1, 0), sp_at(SP_H, 0, 0)}, {sp_at(SP_H, 0, 0), sp_at(SP_B, -1, 1)}, {sp_at(SP_H, 0, 0), sp_at(SP_B, 0, 1)}, {sp_at(SP_B, 0, 0), sp_at(SP_H, 0, 0)}},
    {{sp_at(SP_H, 0, -1), sp_at(SP_J, 0, 0)}, {sp_at(SP_J, 0, 0), sp_at(SP_H, 0, 0)}, {sp_at(SP_B, -1, 0), sp_at(SP_J, 0, 0)}, {sp_at(SP_J, 0, 0), sp_at(SP_B, 0, 0)},
     {sp_at(SP_H, 0, -1), sp_at(SP_B, -1, 0)}, {sp_at(SP_B, -1, 0), sp_at(SP_H, 0, 0)}, {sp_at(SP_B, 0, 0), sp_at(SP_H, 0, 0)}, {sp_at(SP_H, 0, -1), sp_at(SP_B, 0, 0)}}};
// valid* of PU_QuarterPelRefinementOnTheFly (:4396-4418): [half-pel winner fractional][neighbour] -> the three directions that admit it
constexpr unsigned sp_dirs(int a, int b, int c) { return 1u << a | 1u << b | 1u << c; }
__device__ constexpr uint8_t kSpValid[2][8] = {
    {sp_dirs(6, 7, 0), sp_dirs(2, 3, 4), sp_dirs(0, 1, 2), sp_dirs(4, 5, 6), sp_dirs(7, 0, 1), sp_dirs(1, 2, 3), sp_dirs(3, 4, 5), sp_dirs(5, 6, 7)},
    {sp_dirs(2, 3, 4), sp_dirs(6, 7, 0), sp_dirs(4, 5, 6), sp_dirs(0, 1, 2), sp_dirs(3, 4, 5), sp_dirs(5, 6, 7), sp_dirs(7, 0, 1), sp_dirs(1, 2, 3)}};
// SelectBuffer (:6181) / QuarterPelCompensation (:6236-6302): [fractional position x + 4 y] -> one plane, or two to average (0xff: none),
// at the vector's integer part (there the reference's pos_b / pos_h / pos_j are B(0, +1), H(+1, 0), J(+1, +1))
constexpr uint8_t SP_NONE = 0xff;
__device__ constexpr uint8_t kSpBipred[16][2] = {
    {sp_at(SP_F, 0, 0), SP_NONE}, {sp_at(SP_F, 0, 0), sp_at(SP_B, 0, 1)}, {sp_at(SP_B, 0, 1), SP_NONE}, {sp_at(SP_B, 0, 1), sp_at(SP_F, 0, 1)},
    {sp_at(SP_F, 0, 0), sp_at(SP_H, 1, 0)}, {sp_at(SP_B, 0, 1), sp_at(SP_H, 1, 0)}, {sp_at(SP_B, 0, 1), sp_at(SP_J, 1, 1)}, {sp_at(SP_B, 0, 1), sp_at(SP_H, 1, 1)},
    {sp_at(SP_H, 1, 0), SP_NONE}, {sp_at(SP_H, 1, 0), sp_at(SP_J, 1, 1)}, {sp_at(SP_J, 1, 1), SP_NONE}, {sp_at(SP_J, 1, 1), sp_at(SP_H, 1, 1)},
    {sp_at(SP_H, 1, 0), sp_at(SP_F, 1, 0)}, {sp_at(SP_H, 1, 0), sp_at(SP_B, 1, 1)}, {sp_at(SP_J, 1, 1), sp_at(SP_B, 1, 1)}, {sp_at(SP_H, 1, 1), sp_at(SP_B, 1, 1)}};

__host__ __device__ __forceinline__ int sp_taps(int a0, int a1, int a2, int a3) {
    const int v = (18 * (a1 + a2) - 2 * (a0 + a3) + 16) >> 5;
    return v < 0 ? 0 : (v > 255 ? 255 : v);
}
// One sample's term of the half-pel pass's SSE, as spatial_full_distortion_kernel_func_ptr_array computes it (both asm rows hold the SSSE3
// kernels, EbPictureOperators_Intrinsic_SSE4_1.c:532-621): the difference wraps to 8 bits before it is squared (_mm_sub_epi8 /
// _mm_sign_epi8), so |d| above 128 counts as 256 - |d|.  The 8-wide kernel also sums 8 rows whatever the height it is given: 8x16 and
// 8x32 PUs are measured on their upper 8x8 (the caller's `w > 8 || r < 8`).  The quarter pass's combined_averaging_ssd is exact.
__device__ __forceinline__ unsigned sp_sse8(int d) {
    const unsigned a = (unsigned)(d < 0 ? -d : d), b = a > 128u ? 256u - a : a;
    return b * b;
}
__device__ __forceinline__ unsigned sp_wave_sum(unsigned v) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) v += (unsigned)__shfl_xor((int)v, m, 64);
    return v;
}

// A wave's window: iw[r][c] = I(y0 - 2 + r, x0 - 2 + c) for r < h + 5, c < w + 5, bw[r][c] = B(y0 - 2 + r, x0 + c) for r < h + 5, c < w + 2,
// where (y0, x0) is the block's top-left sample at the floor of its vector.  Samples are addressed relative to (y0, x0):
//   F: dy, dx in [-2, h + 2] x [-2, w + 2]    B: [-2, h + 2] x [0, w + 1]    H: [0, h + 1] x [-2, w + 2]    J: [0, h + 1] x [0, w + 1]
struct SpWin { const uint8_t* iw; const uint8_t* bw; };
__device__ __forceinline__ int sp_sample(const SpWin& w, int kind, int dy, int dx) {
    if (kind == SP_F) return w.iw[(dy + 2) * ME_SP_IW + dx + 2];
    if (kind == SP_B) return w.bw[(dy + 2) * ME_SP_BW + dx];
    if (kind == SP_H) {
        const uint8_t* p = w.iw + dy * ME_SP_IW + dx + 2;
        return sp_taps(p[0], p[ME_SP_IW], p[2 * ME_SP_IW], p[3 * ME_SP_IW]);
    }
    const uint8_t* p = w.bw + dy * ME_SP_BW + dx;
    return sp_taps(p[0], p[ME_SP_BW], p[2 * ME_SP_BW], p[3 * ME_SP_BW]);
}
// stage the integer samples (all lanes of the wave; the caller separates this from sp_plane_b by a barrier)
__device__ __forceinline__ void sp_stage(uint8_t* iw, const uint8_t* __restrict__ g /* I(y0 - 2, x0 - 2) */, uint32_t stride, int w, int h, int lane) {
    const int cw = w + 5, n = cw * (h + 5);
    for (int i = lane; i < n; i += 64) {
        const int r = i / cw, c = i - r * cw;
        iw[r * ME_SP_IW + c] = g[(ptrdiff_t)r * (ptrdiff_t)stride + c];
    }
}
__device__ __forceinline__ void sp_plane_b(const uint8_t* iw, uint8_t* bw, int w, int h, int lane) {
    const int cw = w + 2, n = cw * (h + 5);
    for (int i = lane; i < n; i += 64) {
        const int r = i / cw, c = i - r * cw;
        const uint8_t* p = iw + r * ME_SP_IW + c;
        bw[r * ME_SP_BW + c] = (uint8_t)sp_taps(p[0], p[1], p[2], p[3]);
    }
}
// whether the window of a w x h block at (y0, x0) lies inside what the padding holds (svthost::ME_SP_MARGIN on every side)
__device__ __forceinline__ bool sp_window_inside(int x0, int y0, int w, int h, int width, int height) {
    return x0 - 2 >= -ME_SP_MARGIN && y0 - 2 >= -ME_SP_MARGIN && x0 + w + 2 <= width + ME_SP_MARGIN - 1 && y0 + h + 2 <= height + ME_SP_MARGIN - 1;
}
__device__ __forceinline__ uint32_t sp_pack_mv(int x, int y) { return ((uint32_t)(uint16_t)y << 16) | (uint32_t)(uint16_t)x; }

// which passes run for the PU at index n of the result rows (HalfPelSearch_LCU / QuarterPelSearch_LCU's flags)
__device__ __forceinline__ void sp_enabled(const MeSubpelDev& d, int n, bool& half, bool& quarter) {
    if (n == 0) { half = quarter = d.f64 != 0; }
    else if (n < 5) { half = d.h32 != 0; quarter = d.qp != 0; }
    else if (n < 21) { half = d.h16 != 0; quarter = d.qp != 0; }
    else if (n < ME_PUS) { half = d.h8 != 0 && !d.no8; quarter = d.qp != 0 && !d.no8; }
    else { half = quarter = true; }
}

__global__ __launch_bounds__(ME_SP_THREADS) void me_subpel_refine_kernel(const MeSubpelDev d, uint32_t* __restrict__ best_sad, uint32_t* __restrict__ best_mv,
                                                                         uint32_t* __restrict__ best_ssd, uint8_t* __restrict__ half_dir) {
    __shared__ __attribute__((aligned(16))) uint8_t s_win[ME_SP_WAVES][ME_SP_WAVE_LDS];
    const uint32_t sb = blockIdx.x, list = blockIdx.y, pic = blockIdx.z;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int ox = (int)(sb % d.nsbx) * 64, oy = (int)(sb / d.nsbx) * 64;
    const size_t row = (((size_t)pic * d.nsb + sb) * d.nlists + list) * ME_PUS_ALL;
    const uint8_t* src = d.src + (size_t)pic * d.src_pitch;
    const uint8_t* ref = d.ref[list] + (size_t)pic * d.ref_pitch[list];
    const uint32_t rstride = d.ref_stride[list];
    uint8_t* iw = s_win[wave];
    uint8_t* bw = iw + ME_SP_WIN * ME_SP_IW;
    const SpWin win{iw, bw};
    const int method = d.method;
    // the optional outputs are defined for every entry: 0 where a PU is not refined
    for (int i = tid; i < ME_PUS_ALL; i += ME_SP_THREADS) {
        if (best_ssd) best_ssd[row + i] = 0u;
        if (half_dir) half_dir[row + i] = 0;
    }
    const int iters = (d.npus + ME_SP_WAVES - 1) / ME_SP_WAVES;
#pragma unroll 1
    for (int it = 0; it < iters; it++) {
        const int n = it * ME_SP_WAVES + wave;
        bool half = false, quarter = false;
        int px = 0, py = 0, w = 8, h = 8;
        if (n < d.npus) {
            sp_enabled(d, n, half, quarter);
            me_pu_rect(n, px, py, w, h);
            px *= 8; py *= 8; w *= 8; h *= 8;
        }
        uint32_t sad = 0, mv = 0, ssd = 0;
        int xm = 0, ym = 0, x0 = 0, y0 = 0;
        if (half || quarter) {
            sad = best_sad[row + n]; mv = best_mv[row + n];
            xm = (int16_t)(mv & 0xffffu); ym = (int16_t)(mv >> 16);
            x0 = ox + px + (xm >> 2); y0 = oy + py + (ym >> 2);
            if (!sp_window_inside(x0, y0, w, h, d.width, d.height)) half = quarter = false;
        }
        const bool act = half || quarter;
        __syncthreads();                                  // the PU before is done with the window
        if (act) sp_stage(iw, ref + (ptrdiff_t)(y0 - 2) * (ptrdiff_t)rstride + (x0 - 2), rstride, w, h, lane);
        __syncthreads();
        if (act) sp_plane_b(iw, bw, w, h, lane);
        __syncthreads();
        if (!act) continue;                               // (no barrier below this line)
        const uint8_t* sp = src + (ptrdiff_t)(oy + py) * (ptrdiff_t)d.src_stride + (ox + px);
        const int lw = 31 - __clz(w);
        const int rs = method == 0 ? 2 : 1;               // SUB_SAD_SEARCH: every other row
        int dirn = 0;
        if (half) {
            unsigned dist[8], sadf[8], ssd0 = 0;
#pragma unroll
            for (int k = 0; k < 8; k++) { dist[k] = 0; sadf[k] = 0; }
            const int np = w * (h / rs);
            for (int i = lane; i < np; i += 64) {
                const int r = (i >> lw) * rs, c = i & (w - 1);
                const int s = sp[(ptrdiff_t)r * (ptrdiff_t)d.src_stride + c];
                // L R: B(0, 0), B(0, 1); T B: H(0, 0), H(1, 0); TL TR BR BL: J(0, 0), J(0, 1), J(1, 1), J(1, 0)
                int v[8];
                v[0] = sp_sample(win, SP_B, r, c); v[1] = sp_sample(win, SP_B, r, c + 1);
                {
                    const uint8_t* p = iw + r * ME_SP_IW + c + 2;
                    const int a0 = p[0], a1 = p[ME_SP_IW], a2 = p[2 * ME_SP_IW], a3 = p[3 * ME_SP_IW], a4 = p[4 * ME_SP_IW];
                    v[2] = sp_taps(a0, a1, a2, a3); v[3] = sp_taps(a1, a2, a3, a4);
                    if (method == 2 && (w > 8 || r < 8)) ssd0 += sp_sse8(s - a2);
                }
                {
                    const uint8_t* p = bw + r * ME_SP_BW + c;
                    const int a0 = p[0], a1 = p[ME_SP_BW], a2 = p[2 * ME_SP_BW], a3 = p[3 * ME_SP_BW], a4 = p[4 * ME_SP_BW];
                    const int b0 = p[1], b1 = p[ME_SP_BW + 1], b2 = p[2 * ME_SP_BW + 1], b3 = p[3 * ME_SP_BW + 1], b4 = p[4 * ME_SP_BW + 1];
                    v[4] = sp_taps(a0, a1, a2, a3); v[5] = sp_taps(b0, b1, b2, b3); v[6] = sp_taps(b1, b2, b3, b4); v[7] = sp_taps(a1, a2, a3, a4);
                }
#pragma unroll
                for (int k = 0; k < 8; k++) {
                    const int e = s - v[k];
                    const unsigned a = (unsigned)(e < 0 ? -e : e);
                    if (method == 2) { if (w > 8 || r < 8) dist[k] += sp_sse8(e); sadf[k] += a; } else dist[k] += a;
                }
            }
#pragma unroll
            for (int k = 0; k < 8; k++) {
                dist[k] = sp_wave_sum(dist[k]) << (method == 0 ? 1 : 0);
                if (method == 2) sadf[k] = sp_wave_sum(sadf[k]);
            }
            if (method == 2) ssd = sp_wave_sum(ssd0);      // *pBestSsd starts from the SSE of the full-pel winner
            unsigned best = 0xffffffffu;
#pragma unroll
            for (int k = 0; k < 8; k++) {
                best = min(best, dist[k]);
                const uint32_t nmv = sp_pack_mv(xm + 2 * kSpDx[k], ym + 2 * kSpDy[k]);
                if (method == 2) {
                    if (dist[k] < ssd) { sad = sadf[k]; mv = nmv; ssd = dist[k]; }
                } else if (dist[k] < sad) { sad = dist[k]; mv = nmv; }
            }
            bool found = false;
#pragma unroll
            for (int q = 0; q < 8; q++) {
                const int k = kSpDirOrder[q];
                if (!found && dist[k] == best) { dirn = kSpDir[k]; found = true; }
            }
        }
        if (quarter) {
            const int hx = (int16_t)(mv & 0xffffu), hy = (int16_t)(mv >> 16);
            const int cs = (hy & 2) + ((hx & 2) >> 1);
            // the base of the quarter pass relative to the window's: ((mv + 2) >> 2) - (full-pel mv >> 2), 0 or 1
            const int bx = ((hx + 2) >> 2) - (xm >> 2), by = ((hy + 2) >> 2) - (ym >> 2);
            const int qw = n == 0 ? 32 : w, qh = n == 0 ? 32 : h;        // the 64x64 PU's pass measures a 32x32 block (:4809)
            const int qlw = 31 - __clz(qw);
            const int np = qw * (qh / rs);
            const unsigned valid_row = cs ? 1u : 0u;
#pragma unroll 1
            for (int k = 0; k < 8; k++) {
                if (!((kSpValid[valid_row][k] >> dirn) & 1u)) continue;
                const unsigned e1 = kSpQuarter[cs][k][0], e2 = kSpQuarter[cs][k][1];
                const int k1 = e1 & 3, dy1 = (int)((e1 >> 2) & 3) - 1 + by, dx1 = (int)((e1 >> 4) & 3) - 1 + bx;
                const int k2 = e2 & 3, dy2 = (int)((e2 >> 2) & 3) - 1 + by, dx2 = (int)((e2 >> 4) & 3) - 1 + bx;
                unsigned acc = 0, accs = 0;
                for (int i = lane; i < np; i += 64) {
                    const int r = (i >> qlw) * rs, c = i & (qw - 1);
                    const int s = sp[(ptrdiff_t)r * (ptrdiff_t)d.src_stride + c];
                    const int pr = (sp_sample(win, k1, dy1 + r, dx1 + c) + sp_sample(win, k2, dy2 + r, dx2 + c) + 1) >> 1;
                    const int e = s - pr;
                    const unsigned a = (unsigned)(e < 0 ? -e : e);
                    if (method == 2) { acc += a * a; accs += a; } else acc += a;
                }
                acc = sp_wave_sum(acc) << (method == 0 ? 1 : 0);
                const uint32_t nmv = sp_pack_mv(hx + kSpDx[k], hy + kSpDy[k]);
                if (method == 2) {
                    accs = sp_wave_sum(accs);
                    if (acc < ssd) { sad = accs; mv = nmv; ssd = acc; }
                } else if (acc < sad) { sad = acc; mv = nmv; }
            }
        }
        if (lane == 0) {
            best_sad[row + n] = sad; best_mv[row + n] = mv;
            if (best_ssd) best_ssd[row + n] = ssd;
            if (half_dir) half_dir[row + n] = (uint8_t)dirn;
        }
    }
}

// BiPredictionSearch on fractional vectors and the me_results rows.  A wave owns one raster PU at a time: it stages list 0's window,
// leaves that list's compensated block in its LDS block, stages list 1's window over the first and sums |src - avg(block 0, block 1)|.
__global__ __launch_bounds__(ME_SP_THREADS) void me_subpel_bipred_kernel(const MeSubpelDev d, int bipred_all_pus, int sub_sad, const MePuMap map,
                                                                         const uint32_t* __restrict__ best_sad, const uint32_t* __restrict__ best_mv,
                                                                         uint32_t* __restrict__ bipred_sad /* [picture][SB][ME_PUS_ALL] */,
                                                                         MeResult* __restrict__ results /* [picture][SB][ME_PUS_ALL] */) {
    __shared__ __attribute__((aligned(16))) uint8_t s_win[ME_SP_WAVES][ME_SP_WAVE_LDS];
    __shared__ __attribute__((aligned(16))) uint8_t s_blk[ME_SP_WAVES][64 * 64];
    __shared__ unsigned s_bi[ME_PUS_ALL];
    __shared__ MePuMap s_map;
    static_assert(sizeof(MePuMap) % 2 == 0 && alignof(MePuMap) >= 2 && sizeof(MePuMap) + sizeof(unsigned) * ME_PUS_ALL <= svthost::ME_SP_BIPRED_TABLES, "copied as 16-bit words");
    const uint32_t sb = blockIdx.x, pic = blockIdx.z;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int ox = (int)(sb % d.nsbx) * 64, oy = (int)(sb / d.nsbx) * 64;
    const size_t sbi = (size_t)pic * d.nsb + sb, row = sbi * d.nlists * ME_PUS_ALL;
    const bool two = d.nlists == 2;
    // every entry of the two outputs is defined after the call: PUs without a bi-prediction SAD and rows past the PU count are zero
    for (int i = tid; i < ME_PUS_ALL; i += ME_SP_THREADS) {
        bipred_sad[sbi * ME_PUS_ALL + i] = 0u;
        s_bi[i] = 0;
        if (i >= d.npus) {
            MeResult z;
            __builtin_memset(&z, 0, sizeof(z));
            results[sbi * ME_PUS_ALL + i] = z;
        }
    }
    for (int i = tid; i < (int)(sizeof(MePuMap) / 2); i += ME_SP_THREADS) reinterpret_cast<uint16_t*>(&s_map)[i] = reinterpret_cast<const uint16_t*>(&map)[i];
    __syncthreads();
    const uint32_t* bs0 = best_sad + row;
    const uint32_t* bm0 = best_mv + row;
    const uint32_t* bs1 = two ? bs0 + ME_PUS_ALL : nullptr;
    const uint32_t* bm1 = two ? bm0 + ME_PUS_ALL : nullptr;
    if (two) {
        const uint8_t* src = d.src + (size_t)pic * d.src_pitch;
        uint8_t* iw = s_win[wave];
        uint8_t* bw = iw + ME_SP_WIN * ME_SP_IW;
        uint8_t* blk = s_blk[wave];
        const SpWin win{iw, bw};
        const int nbi = bipred_all_pus ? d.npus : min(d.npus, 21);
        const int iters = (nbi + ME_SP_WAVES - 1) / ME_SP_WAVES;
        const int rs = sub_sad ? 2 : 1;
#pragma unroll 1
        for (int it = 0; it < iters; it++) {
            const int p = it * ME_SP_WAVES + wave;
            bool act = p < nbi;
            const int pc = act ? p : 0, n = s_map.storage[pc];
            const int px = 8 * s_map.x8[pc], py = 8 * s_map.y8[pc], w = 8 * s_map.w8[pc], h = 8 * s_map.h8[pc];
            const int lw = 31 - __clz(w);
            int x0[2], y0[2], frac[2];
#pragma unroll
            for (int l = 0; l < 2; l++) {
                const uint32_t m = l ? bm1[n] : bm0[n];
                const int x = (int16_t)(m & 0xffffu), y = (int16_t)(m >> 16);
                x0[l] = ox + px + (x >> 2); y0[l] = oy + py + (y >> 2);
                frac[l] = (x & 3) + ((y & 3) << 2);
                if (!sp_window_inside(x0[l], y0[l], w, h, d.width, d.height)) act = false;
            }
            unsigned acc = 0;
#pragma unroll 1
            for (int l = 0; l < 2; l++) {
                const uint8_t* ref = d.ref[l] + (size_t)pic * d.ref_pitch[l];
                __syncthreads();                              // the window's last readers are done
                if (act) sp_stage(iw, ref + (ptrdiff_t)(y0[l] - 2) * (ptrdiff_t)d.ref_stride[l] + (x0[l] - 2), d.ref_stride[l], w, h, lane);
                __syncthreads();
                if (act) sp_plane_b(iw, bw, w, h, lane);
                __syncthreads();
                if (act) {
                    const unsigned e1 = kSpBipred[frac[l]][0], e2 = kSpBipred[frac[l]][1];
                    const int k1 = e1 & 3, dy1 = (int)((e1 >> 2) & 3) - 1, dx1 = (int)((e1 >> 4) & 3) - 1;
                    const int k2 = e2 & 3, dy2 = (int)((e2 >> 2) & 3) - 1, dx2 = (int)((e2 >> 4) & 3) - 1;
                    const int np = w * (h / rs);
                    for (int i = lane; i < np; i += 64) {
                        const int r = (i >> lw) * rs, c = i & (w - 1);
                        int v = sp_sample(win, k1, dy1 + r, dx1 + c);
                        if (e2 != SP_NONE) v = (v + sp_sample(win, k2, dy2 + r, dx2 + c) + 1) >> 1;
                        if (l == 0) blk[r * 64 + c] = (uint8_t)v;
                        else {
                            const int s = src[(ptrdiff_t)(oy + py + r) * (ptrdiff_t)d.src_stride + (ox + px + c)];
                            const int e = s - ((blk[r * 64 + c] + v + 1) >> 1);   // (each lane reads back what it wrote itself)
                            acc += (unsigned)(e < 0 ? -e : e);
                        }
                    }
                }
            }
            acc = sp_wave_sum(acc) << (sub_sad ? 1 : 0);
            if (act && lane == 0) s_bi[n] = acc;
        }
    }
    __syncthreads();
    if (tid < d.npus) me_result_row(tid, s_map.storage[tid], bs0, bm0, bs1, bm1, bipred_all_pus, s_bi[s_map.storage[tid]], bipred_sad + sbi * ME_PUS_ALL, results + sbi * ME_PUS_ALL);
}

// B / H / J of a window, each sample straight from the plane: out [3][h][w], entry [k][r][c] at (y0 + r, x0 + c)
__global__ __launch_bounds__(256) void me_subpel_planes_kernel(const uint8_t* __restrict__ ref /* sample (0, 0) */, uint32_t stride, int x0, int y0, uint32_t w,
                                                               uint32_t h, uint8_t* __restrict__ out) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= w * h) return;
    const int r = (int)(i / w), c = (int)(i - (uint32_t)r * w);
    const uint8_t* p = ref + (ptrdiff_t)(y0 + r) * (ptrdiff_t)stride + (x0 + c);
    const ptrdiff_t s = (ptrdiff_t)stride;
    int b[4];
#pragma unroll
    for (int k = 0; k < 4; k++) { const uint8_t* q = p + (k - 2) * s; b[k] = sp_taps(q[-2], q[-1], q[0], q[1]); }
    out[i] = (uint8_t)b[2];
    out[(size_t)w * h + i] = (uint8_t)sp_taps(p[-2 * s], p[-s], p[0], p[s]);
    out[(size_t)2 * w * h + i] = (uint8_t)sp_taps(b[0], b[1], b[2], b[3]);
}

}  // namespace svtdev

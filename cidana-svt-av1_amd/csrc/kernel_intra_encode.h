// kernel_intra_encode.h — svt_hip_intra_encode_frame: the intra encode pass in coding order (EbCodingLoop.c:2853-3005 with Av1EncodeLoop
// :545-980 and Av1EncodeGenerateRecon :1408-1500) on the device.
//
//   ie_prepass_kernel    one wave per (picture, superblock): clears the superblock's cursors and smooth-mode grid, applies the rules of
//           the call to every final entry (d_status), takes the running stream offsets (a wave prefix sum, as recon_bin_kernel), leaves
//           one 24-byte plan record per entry in scratch, a cleared result record per coded entry, and scatters the coded entries'
//           smooth flags (is_smooth of the luma mode, of the chroma mode) into the grid of 4x4 units get_filt_type will consult.
//   ie_walk_kernel<KIND> one workgroup per (superblock of the step, picture, plane).  It takes the plane's cursor and codes entry after
//           entry while the entry's transform size is of launch kind KIND (av1_geom.h): availability (intra_avail.h) ->
//           neighbour row / column from the reconstruction plane into LDS -> build_intra_predictors with run-time sizes into the plane
//           -> (chroma, uv_mode 13) the CfL step -> the size's encode body (enc4_body / enc_staged_body / enc32_body / enc64_body, as
//           enc_frame_kernel runs them) with pred == recon, one block.  It stops at the first entry of another kind and stores the
//           cursor.  Entries that are not coded, and chroma of entries without has_uv, are passed by whatever the kind.
//   ie_finish_kernel     one wave per (picture, superblock): entries a cursor did not pass get status _SCHEDULE.
//
// No workgroup waits for another: launch order on the stream carries the dependencies between superblocks (the steps) and between a
// block's luma and its chroma (the luma launches of a step precede its chroma launches).  Inside a workgroup the stores of one entry
// are visible to the loads of the next through __syncthreads().  Everything read from device memory - the plan records included - is
// clamped or checked before it forms an address.
#pragma once
#include "intra_avail.h"
#include "intra_encode_plan.h"
#include "kernel_bip.h"
#include "kernel_final_list.h"
#include "kernel_frame.h"

namespace svtdev {

constexpr int IE_FINAL = FL_MAX_FINAL;
// the walkers' own, per transform size: the quantiser's log scale, and where the size's inverse scans start in the blob and how long
// one is (the geometry and the launch kinds are kGeomTab's, kernel_final_list.h)
struct IeWalkTab {
    uint8_t ls[SVT_TX_SIZES_ALL];
    uint32_t iscan_first[SVT_TX_SIZES_ALL], ncoeff[SVT_TX_SIZES_ALL];
};
constexpr IeWalkTab ie_walk_tab() {
    IeWalkTab T{};
    for (int t = 0; t < SVT_TX_SIZES_ALL; t++) {
        const int pels = svthost::kTxW[t] * svthost::kTxH[t];
        T.ls[t] = (uint8_t)(pels > 1024 ? 2 : (pels > 256 ? 1 : 0));
        T.iscan_first[t] = svthost::ie_iscan_first(t); T.ncoeff[t] = svthost::ie_ncoeff(t);
    }
    return T;
}
static __device__ const IeWalkTab kIeTab = ie_walk_tab();

struct IeDesc {
    const uint32_t* final_blk;             // svt_hip_part_final as three words
    const uint32_t* final_count;
    const uint2* blk;                      // svt_hip_intra_enc_blk as two words
    const uint8_t* src[3];
    uint8_t* recon[3];
    int32_t* sbq[3];
    uint8_t* status;
    uint32_t* coeff_offset;
    uint2* result;                         // the caller's, or nullptr: the scratch's
    char* scratch;
    const int16_t* iscan;
    unsigned long long src_pitch[3], recon_pitch[3];
    uint32_t src_stride[3], stride[3], width[3], height[3];
    uint32_t npics, sb_cols, sb_rows, nsb, sb_pitch, nsrc, blk_pitch, planes;
    QParams qp[2][3];                      // [luma | chroma][log scale]
};
static_assert(sizeof(IeDesc) <= 3900, "kernel arguments");

__device__ __forceinline__ char* ie_sb_scratch(const IeDesc& D, uint32_t pic, uint32_t sb) {
    return D.scratch + ((size_t)pic * D.nsb + sb) * svthost::IE_SB_BYTES;
}

// ---- the pre-pass ---------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void ie_prepass_kernel(const IeDesc in_kernarg) {
    (void)in_kernarg;
    const IeDesc& D = *(const IeDesc*)__builtin_amdgcn_kernarg_segment_ptr();
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const uint32_t unit = blockIdx.x * 4u + (uint32_t)wave;
    if (unit >= D.npics * D.nsb) return;                                    // wave-uniform
    const uint32_t pic = unit / D.nsb, sb = unit - pic * D.nsb;
    const size_t gsb = (size_t)pic * D.sb_pitch + sb;
    char* S = ie_sb_scratch(D, pic, sb);
    uint32_t* hdr = reinterpret_cast<uint32_t*>(S);
    uint32_t* plan = reinterpret_cast<uint32_t*>(S + svthost::IE_OFF_PLAN);
    uint8_t* grid = reinterpret_cast<uint8_t*>(S + svthost::IE_OFF_GRID);
    uint2* result = D.result ? D.result + gsb * IE_FINAL : reinterpret_cast<uint2*>(S + svthost::IE_OFF_RESULT);
    if (lane < 8) hdr[lane] = 0;
    reinterpret_cast<uint32_t*>(grid)[lane] = 0;
    __threadfence_block();
    const uint32_t count = final_count_of(D.final_count, gsb);
    const uint32_t sbx = (sb % D.sb_cols) * 16u, sby = (sb / D.sb_cols) * 16u;      // the superblock's origin in 4x4 units
    uint32_t run_y = 0, run_uv = 0;
#pragma unroll 1
    for (uint32_t base = 0; base < count; base += 64) {
        const uint32_t k = base + (uint32_t)lane;
        const bool live = k < count;
        FinalEntry e;
        if (live) e = final_entry_load(D.final_blk, gsb, k);
        const uint32_t src = e.src, x = e.x, y = e.y, part = e.part;
        // the block size of the md-scan block; chroma inside plane 1 (the host requires both chroma planes to be exactly half)
        const uint32_t b = kGeomTab.bsize_of[e.mds];
        const EntryGeom g = entry_geom(e, b);
        const uint32_t bw = g.bw, bh = g.bh;
        const bool has_uv = g.has_uv;
        uint32_t reason = SVT_HIP_INTRA_ENC_OK;
        if (src == SVT_HIP_PART_NO_SRC || src >= D.nsrc) reason = SVT_HIP_INTRA_ENC_NO_SRC;
        if (reason == SVT_HIP_INTRA_ENC_OK && !entry_inside(e, g, D.width, D.height, D.planes == 3 ? 2u : 1u)) reason = SVT_HIP_INTRA_ENC_OUTSIDE;
        uint2 bl = make_uint2(0, 0);
        if (reason == SVT_HIP_INTRA_ENC_OK) bl = D.blk[(size_t)pic * D.blk_pitch + src];
        const uint32_t is_intra = bl.x & 0xffu, mode = (bl.x >> 8) & 0xffu, uv_mode = bl.x >> 24;
        const int delta = (int)(int8_t)((bl.x >> 16) & 0xffu);
        const uint32_t type = (bl.y >> 16) & 0xffu, type_uv = bl.y >> 24;
        if (reason == SVT_HIP_INTRA_ENC_OK) {
            if (!svthost::tx_type_ok_sides(bw, bh, type) || (has_uv && !svthost::tx_type_ok_sides(g.cw, g.ch, type_uv))) reason = SVT_HIP_INTRA_ENC_TX_TYPE;
            else if (!is_intra) reason = SVT_HIP_INTRA_ENC_NOT_INTRA;
            else if (mode > 12u || uv_mode > 13u || delta < -3 || delta > 3 || (delta != 0 && !(mode >= 1 && mode <= 8))) reason = SVT_HIP_INTRA_ENC_MODE;
            else if (uv_mode == 13u && (bw > 32 || bh > 32 || bw < 8 || bh < 8)) reason = SVT_HIP_INTRA_ENC_CFL_SIZE;
        }
        const bool coded = live && reason == SVT_HIP_INTRA_ENC_OK;
        const bool adv = coded || (live && reason == SVT_HIP_INTRA_ENC_NOT_INTRA);      // the offsets advance over the coded entries and the ones that are not intra
        uint32_t off_y, off_uv;
        stream_offsets(adv ? bw * bh : 0u, adv && has_uv ? g.cw * g.ch : 0u, lane, run_y, run_uv, off_y, off_uv);
        if (live) {
            if (D.status) D.status[gsb * IE_FINAL + k] = (uint8_t)reason;
            if (D.coeff_offset) { uint32_t* o = D.coeff_offset + 2 * (gsb * IE_FINAL + k); o[0] = off_y; o[1] = off_uv; }
            uint32_t* p = plan + svthost::IE_PLAN_WORDS * k;
            p[0] = x | y << 16; p[1] = b | (part & 0xffu) << 8 | reason << 16 | (has_uv ? 1u : 0u) << 24; p[2] = src; p[3] = off_y; p[4] = off_uv; p[5] = 0;
        }
        if (coded) {
            result[k] = make_uint2(0u, type << 16);
            const uint32_t flags = (mode >= 9 && mode <= 11 ? 1u : 0u) | (uv_mode >= 9 && uv_mode <= 11 ? 2u : 0u);
            if (flags) {
                const uint32_t ux = (x >> 2) - sbx, uy = (y >> 2) - sby;     // (wraps to huge for a block left of / above its superblock)
                for (uint32_t r = 0; r < bh / 4; r++)
                    for (uint32_t c = 0; c < bw / 4; c++)
                        if (ux + c < 16u && uy + r < 16u) grid[(uy + r) * 16 + ux + c] = (uint8_t)flags;
            }
        }
    }
}

__global__ __launch_bounds__(256) void ie_finish_kernel(const IeDesc in_kernarg) {
    (void)in_kernarg;
    const IeDesc& D = *(const IeDesc*)__builtin_amdgcn_kernarg_segment_ptr();
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const uint32_t unit = blockIdx.x * 4u + (uint32_t)wave;
    if (unit >= D.npics * D.nsb || !D.status) return;
    const uint32_t pic = unit / D.nsb, sb = unit - pic * D.nsb;
    const size_t gsb = (size_t)pic * D.sb_pitch + sb;
    const char* S = ie_sb_scratch(D, pic, sb);
    const uint32_t* hdr = reinterpret_cast<const uint32_t*>(S);
    const uint32_t* plan = reinterpret_cast<const uint32_t*>(S + svthost::IE_OFF_PLAN);
    const uint32_t count = final_count_of(D.final_count, gsb);
    const uint32_t c0 = hdr[0], c1 = hdr[1], c2 = hdr[2];
    for (uint32_t k = (uint32_t)lane; k < count; k += 64) {
        const uint32_t w1 = plan[svthost::IE_PLAN_WORDS * k + 1];
        const bool ok = ((w1 >> 16) & 0xffu) == SVT_HIP_INTRA_ENC_OK, has_uv = (w1 >> 24) & 1u;
        if (ok && (k >= c0 || (D.planes == 3 && has_uv && (k >= c1 || k >= c2)))) D.status[gsb * IE_FINAL + k] = SVT_HIP_INTRA_ENC_SCHEDULE;
    }
}

// ---- the prediction: build_intra_predictors (EbIntraPrediction.c:3667-3855) with run-time sizes ------------------------------------------
constexpr int IE_EDGE = 192, IE_EDGE_ORG = 32;          // an edge in LDS: positions [-32, 160); the reference's arrays hold [-16, 144)
struct IePredArgs { int w, h, mode, delta, filt_type, n_top, n_tr, n_left, n_bl; };

// `dst` points at the block's first sample on its plane; the neighbour row is dst - stride, the column dst - 1.  Only samples the counts
// admit are read.  All threads of the workgroup call it; ends with a barrier after the stores.
__device__ __forceinline__ void ie_predict(uint8_t* dst, uint32_t stride, const IePredArgs& a, uint8_t* s_edge, int* s_red) {
    const int tid = threadIdx.x, w = a.w, h = a.h, mode = a.mode;
    uint8_t* A = s_edge + IE_EDGE_ORG;
    uint8_t* L = s_edge + IE_EDGE + IE_EDGE_ORG;
    const uint8_t* above_ref = dst - stride;
    const int n_top = a.n_top, n_left = a.n_left, n_tr = a.n_tr, n_bl = a.n_bl;
    const bool is_dr = mode >= 1 && mode <= 8;
    bool need_left = true, need_above = true, need_above_left = mode == 12, need_right = false, need_bottom = false;
    int p_angle = 0;
    if (is_dr) {
        const int ang[9] = {0, 90, 180, 45, 135, 113, 157, 203, 67};        // mode_to_angle_map
        int a0 = 0;
#pragma unroll
        for (int i = 1; i < 9; i++) a0 = i == mode ? ang[i] : a0;
        p_angle = a0 + 3 * a.delta;
        need_above = p_angle < 180; need_left = p_angle > 90; need_above_left = true;
        need_right = p_angle < 90; need_bottom = p_angle > 180;
    }
    const int npix = w * h, wl = __builtin_ctz((unsigned)w);
    if ((!need_above && n_left == 0) || (!need_left && n_top == 0)) {       // (:3718-3731)
        const int val = need_left ? (n_top > 0 ? (int)above_ref[0] : 129) : (n_left > 0 ? (int)dst[-1] : 127);
        for (int i = tid; i < npix; i += svthost::IE_THREADS) dst[(size_t)(i >> wl) * stride + (i & (w - 1))] = (uint8_t)val;
        __syncthreads();
        return;
    }
    // ---- the edges (:3733-3801) ----
    const int need_l = need_left ? h + (need_bottom ? w : 0) : 0, need_a = need_above ? w + (need_right ? h : 0) : 0;      // <= 128
    if (tid < need_l) {
        int v;
        if (n_left > 0) { const int avail = n_left + (need_bottom && n_bl > 0 ? n_bl : 0); v = dst[(size_t)min(tid, avail - 1) * stride - 1]; }
        else v = n_top > 0 ? (int)above_ref[0] : 129;
        L[tid] = (uint8_t)v;
    }
    if (tid >= 128 && tid - 128 < need_a) {
        const int i = tid - 128;
        int v;
        if (n_top > 0) { const int avail = n_top + (need_right && n_tr > 0 ? n_tr : 0); v = above_ref[min(i, avail - 1)]; }
        else v = n_left > 0 ? (int)dst[-1] : 127;
        A[i] = (uint8_t)v;
    }
    if (tid == 0 && need_above_left) {
        const int c = (n_top > 0 && n_left > 0) ? (int)above_ref[-1] : (n_top > 0 ? (int)above_ref[0] : (n_left > 0 ? (int)dst[-1] : 128));
        A[-1] = (uint8_t)c; L[-1] = (uint8_t)c;
    }
    __syncthreads();
    int up_a = 0, up_l = 0;
    if (is_dr) {                                                             // disable_edge_filter is 0 (:3812-3847)
        const int ft = a.filt_type;
        if (p_angle != 90 && p_angle != 180) {
            if (need_above && need_left && w + h >= 24) {                   // filter_intra_edge_corner
                if (tid == 0) {
                    const int s = ((int)L[0] * 5 + (int)A[-1] * 6 + (int)A[0] * 5 + 8) >> 4;
                    A[-1] = (uint8_t)s; L[-1] = (uint8_t)s;
                }
                __syncthreads();
            }
            // av1_filter_intra_edge on both edges at once: threads 0 .. 127 the above edge, 128 .. 255 the left one (the 129th sample
            // of an edge, where there is one, by thread 0 / 128 as a second value)
            const int sa = need_above && n_top > 0 ? bip_filter_strength(w, h, p_angle - 90, ft) : 0;
            const int sl = need_left && n_left > 0 ? bip_filter_strength(h, w, p_angle - 180, ft) : 0;
            const int na = n_top + 1 + (need_right ? h : 0), nl = n_left + 1 + (need_bottom ? w : 0);      // ab_le is 1 for every directional mode
            const bool left_half = tid >= 128;
            const uint8_t* p = (left_half ? L : A) - 1;
            const int st = left_half ? sl : sa, sz = left_half ? nl : na, i0 = tid & 127;
            int v0 = -1, v1 = -1;
            if (st) {
                const int k0 = st == 3 ? 2 : 0, k1 = st == 2 ? 5 : 4, k2 = st == 1 ? 8 : (st == 2 ? 6 : 4);
                auto tap = [&](int i) {
                    auto at = [&](int q) { return (int)p[min(max(q, 0), sz - 1)]; };
                    return (k0 * at(i - 2) + k1 * at(i - 1) + k2 * at(i) + k1 * at(i + 1) + k0 * at(i + 2) + 8) >> 4;
                };
                if (i0 >= 1 && i0 < sz) v0 = tap(i0);
                if (i0 == 0 && sz > 128) v1 = tap(128);
            }
            __syncthreads();
            uint8_t* pw = (left_half ? L : A) - 1;
            if (v0 >= 0) pw[i0] = (uint8_t)v0;
            if (v1 >= 0) pw[128] = (uint8_t)v1;
            __syncthreads();
        }
        up_a = need_above ? bip_use_upsample(w, h, p_angle - 90, ft) : 0;
        up_l = need_left ? bip_use_upsample(h, w, p_angle - 180, ft) : 0;
        if (up_a | up_l) {                                                   // av1_upsample_intra_edge: w + h <= 16
            const bool left_half = tid >= 128;
            uint8_t* p = left_half ? L : A;
            const int on = left_half ? up_l : up_a, sz = left_half ? need_l : need_a, i = tid & 127;
            int in[4] = {0, 0, 0, 0};
            const bool mine = on && i < sz;
            if (mine) {
#pragma unroll
                for (int k = 0; k < 4; k++) { const int q = i + k; in[k] = p[q < 2 ? -1 : (q < sz + 2 ? q - 2 : sz - 1)]; }
            }
            __syncthreads();
            if (mine) {
                if (i == 0) p[-2] = (uint8_t)in[0];
                p[2 * i - 1] = (uint8_t)min(max((-in[0] + 9 * in[1] + 9 * in[2] - in[3] + 8) >> 4, 0), 255);
                p[2 * i] = (uint8_t)in[2];
            }
            __syncthreads();
        }
    }
    // ---- DC by availability (dc_pred[left][top], :3854) ----
    int dc = 128;
    if (mode == 0 && (n_top > 0 || n_left > 0)) {
        const int na = n_top > 0 ? w : 0, nl = n_left > 0 ? h : 0;
        if (tid < 64) {
            int sum = 0;
            for (int i = tid; i < na + nl; i += 64) sum += i < na ? (int)A[i] : (int)L[i - na];
            for (int m = 32; m >= 1; m >>= 1) sum += __shfl_xor(sum, m, 64);
            if (tid == 0) s_red[0] = sum;
        }
        __syncthreads();
        dc = (s_red[0] + ((na + nl) >> 1)) / (na + nl);
    }
    // ---- the samples ----
    const int dx = bip_dr_derivative(p_angle < 90 ? p_angle : 180 - p_angle), dy = bip_dr_derivative(p_angle < 180 ? p_angle - 90 : 270 - p_angle);
    const int bl_s = L[h - 1], tr_s = A[w - 1], tl_s = A[-1];
    for (int i = tid; i < npix; i += svthost::IE_THREADS) {
        const int r = i >> wl, c = i & (w - 1);
        int v;
        if (is_dr) {
            if (p_angle == 90) v = A[c];
            else if (p_angle == 180) v = L[r];
            else if (p_angle < 90) {                                         // av1_dr_prediction_z1
                const int max_base = (w + h - 1) << up_a, x = dx * (r + 1), base = (x >> (6 - up_a)) + (c << up_a), sh = ((x << up_a) & 0x3f) >> 1;
                v = base < max_base ? ((int)A[base] * (32 - sh) + (int)A[base + 1] * sh + 16) >> 5 : (int)A[max_base];
            } else if (p_angle > 180) {                                      // av1_dr_prediction_z3
                const int max_base = (w + h - 1) << up_l, yy = dy * (c + 1), base = (yy >> (6 - up_l)) + (r << up_l), sh = ((yy << up_l) & 0x3f) >> 1;
                v = base < max_base ? ((int)L[base] * (32 - sh) + (int)L[base + 1] * sh + 16) >> 5 : (int)L[max_base];
            } else {                                                         // av1_dr_prediction_z2
                const int x = -dx * (r + 1), base1 = (x >> (6 - up_a)) + (c << up_a);
                if (base1 >= -(1 << up_a)) {
                    const int sh = ((x * (1 << up_a)) & 0x3f) >> 1;
                    v = ((int)A[base1] * (32 - sh) + (int)A[base1 + 1] * sh + 16) >> 5;
                } else {
                    const int yy = (r << 6) - dy * (c + 1), base2 = yy >> (6 - up_l), sh = ((yy * (1 << up_l)) & 0x3f) >> 1;
                    v = ((int)L[base2] * (32 - sh) + (int)L[base2 + 1] * sh + 16) >> 5;
                }
            }
            v = min(max(v, 0), 255);
        } else if (mode == 0) v = dc;
        else if (mode == 12) {                                               // paeth
            const int t = A[c], l = L[r], pb = t + l - tl_s;
            const int pl = abs(pb - l), pt = abs(pb - t), ptl = abs(pb - tl_s);
            v = (pl <= pt && pl <= ptl) ? l : (pt <= ptl ? t : tl_s);
        } else {
            const int whr = kSmWeights[h + r], ww = kSmWeights[w + c], ac = A[c], lr = L[r];
            if (mode == 9) v = (whr * ac + (256 - whr) * bl_s + ww * lr + (256 - ww) * tr_s + 256) >> 9;
            else if (mode == 10) v = (whr * ac + (256 - whr) * bl_s + 128) >> 8;
            else v = (ww * lr + (256 - ww) * tr_s + 128) >> 8;
        }
        dst[(size_t)r * stride + c] = (uint8_t)v;
    }
    __syncthreads();
}

// the smooth flags of the 4x4 unit (r, c) of the picture: 0 outside the grid of superblocks
__device__ __forceinline__ uint32_t ie_grid(const IeDesc& D, uint32_t pic, int r, int c) {
    if (r < 0 || c < 0) return 0;
    const uint32_t sr = (uint32_t)r >> 4, sc = (uint32_t)c >> 4;
    if (sr >= D.sb_rows || sc >= D.sb_cols) return 0;
    return reinterpret_cast<const uint8_t*>(ie_sb_scratch(D, pic, sr * D.sb_cols + sc) + svthost::IE_OFF_GRID)[(r & 15) * 16 + (c & 15)];
}

template <int KIND> struct IeLds { static constexpr int BYTES = FrameLds<uint8_t, KIND == 0 ? 0 : (KIND == 3 ? 2 : 1)>::BYTES; };

// ---- the walker -----------------------------------------------------------------------------------------------------------------------
template <int KIND>
__global__ __launch_bounds__(svthost::IE_THREADS) void ie_walk_kernel(const IeDesc in_kernarg, uint32_t step, uint32_t r_first, uint32_t plane_first) {
    (void)in_kernarg; (void)step; (void)r_first; (void)plane_first;
    const IeDesc& D = *(const IeDesc*)__builtin_amdgcn_kernarg_segment_ptr();
    __shared__ __attribute__((aligned(16))) char lds[IeLds<KIND>::BYTES];
    __shared__ __attribute__((aligned(16))) uint8_t s_edge[2 * IE_EDGE];
    __shared__ int s_red[8];
    const int tid = threadIdx.x;
    const uint32_t sbr = r_first + blockIdx.x, sbc = step - 2u * sbr, pic = blockIdx.y, plane = plane_first + blockIdx.z;
    if (sbr >= D.sb_rows || sbc >= D.sb_cols || pic >= D.npics || plane >= D.planes) return;       // workgroup-uniform
    const uint32_t sb = sbr * D.sb_cols + sbc;
    const size_t gsb = (size_t)pic * D.sb_pitch + sb;
    char* S = ie_sb_scratch(D, pic, sb);
    uint32_t* hdr = reinterpret_cast<uint32_t*>(S);
    const uint32_t* plan = reinterpret_cast<const uint32_t*>(S + svthost::IE_OFF_PLAN);
    uint2* result = D.result ? D.result + gsb * IE_FINAL : reinterpret_cast<uint2*>(S + svthost::IE_OFF_RESULT);
    const uint32_t count = final_count_of(D.final_count, gsb);
    const uint8_t* src = D.src[plane] + (size_t)pic * D.src_pitch[plane];
    uint8_t* recon = D.recon[plane] + (size_t)pic * D.recon_pitch[plane];
    const uint32_t stride = D.stride[plane], src_stride = D.src_stride[plane];
    const uint32_t span = plane == 0 ? svthost::kSbLumaSpan : svthost::kSbChromaSpan;
    uint32_t k = min(hdr[plane], count);
#pragma unroll 1
    for (; k < count; k++) {
        const uint32_t* pl = plan + svthost::IE_PLAN_WORDS * k;
        const uint32_t w0 = pl[0], w1 = pl[1], srci = pl[2], off = plane == 0 ? pl[3] : pl[4];
        const uint32_t bsize = min(w1 & 0xffu, 21u), part = (w1 >> 8) & 0xffu;
        const bool has_uv = (w1 >> 24) & 1u;
        if (((w1 >> 16) & 0xffu) != SVT_HIP_INTRA_ENC_OK || (plane != 0 && !has_uv) || srci >= D.nsrc) continue;
        const uint32_t txs = min((uint32_t)(plane == 0 ? kGeomTab.tx[bsize] : kGeomTab.tx_uv[bsize]), (uint32_t)SVT_TX_SIZES_ALL - 1);
        if (kGeomTab.kind[txs] != KIND) break;
        const uint32_t x = w0 & 0xffffu, y = w0 >> 16;
        const uint32_t w = plane == 0 ? kGeomTab.bw[bsize] : kGeomTab.cw[bsize], h = plane == 0 ? kGeomTab.bh[bsize] : kGeomTab.ch[bsize];
        const uint32_t px = plane == 0 ? x : ((x >> 3) << 3) >> 1, py = plane == 0 ? y : ((y >> 3) << 3) >> 1;
        if (w == 0 || px + w > D.width[plane] || py + h > D.height[plane] || x + kGeomTab.bw[bsize] > D.width[0] || y + kGeomTab.bh[bsize] > D.height[0]) continue;
        const uint2 bl = D.blk[(size_t)pic * D.blk_pitch + srci];
        const uint32_t uv_mode = min(bl.x >> 24, 13u);
        const bool cfl = plane != 0 && uv_mode == 13u;
        IePredArgs pa;
        pa.w = (int)w; pa.h = (int)h;
        pa.mode = plane == 0 ? (int)min((bl.x >> 8) & 0xffu, 12u) : (cfl ? 0 : (int)min(uv_mode, 12u));
        pa.delta = plane == 0 ? max(-3, min(3, (int)(int8_t)((bl.x >> 16) & 0xffu))) : 0;
        const uint32_t type = min(plane == 0 ? (bl.y >> 16) & 0xffu : bl.y >> 24, 15u);
        // availability
        svtavail::Pos q{};
        q.sb_mi = 16; q.bsize = (int)bsize; q.partition = (int)min(part, 9u); q.plane = (int)plane; q.mi_rows = (int)(D.height[0] >> 2); q.mi_cols = (int)(D.width[0] >> 2);
        q.bl_org_x_pict = (int)x; q.bl_org_y_pict = (int)y; q.wpx = (int)w; q.hpx = (int)h; q.txw = (int)w; q.txh = (int)h;
        svtavail::Px av;
        if (!svtavail::neighbor_px(q, av)) continue;
        pa.n_top = av.n_top; pa.n_tr = av.n_topright; pa.n_left = av.n_left; pa.n_bl = av.n_bottomleft;
        if ((pa.n_top > 0 && py == 0) || (pa.n_left > 0 && px == 0) || px + w + (uint32_t)pa.n_tr > D.width[plane] || py + h + (uint32_t)pa.n_bl > D.height[plane]) continue;
        const int mirow = (int)(y >> 2), micol = (int)(x >> 2);
        if (plane == 0) {
            pa.filt_type = (int)(((av.up ? ie_grid(D, pic, mirow - 1, micol) : 0u) | (av.left ? ie_grid(D, pic, mirow, micol - 1) : 0u)) & 1u);
        } else {
            const int r0 = mirow & ~1, c0 = micol & ~1;
            pa.filt_type = (int)((((av.up ? ie_grid(D, pic, r0 - 1, c0 + 1) : 0u) | (av.left ? ie_grid(D, pic, r0 + 1, c0 - 1) : 0u)) >> 1) & 1u);
        }
        uint8_t* dst = recon + (size_t)py * stride + px;
        ie_predict(dst, stride, pa, s_edge, s_red);
        if (cfl) {                                                           // (:736-846) w, h <= 16: one sample per thread
            const uint8_t* luma = D.recon[0] + (size_t)pic * D.recon_pitch[0] + (size_t)y * D.stride[0] + x;
            const int npix = (int)(w * h), wl = __builtin_ctz(w);
            const int r = tid >> wl, c = tid & ((int)w - 1);
            int v = 0;
            if (tid < npix) {
                const uint8_t* s0 = luma + (size_t)(2 * r) * D.stride[0] + 2 * c;
                v = ((int)s0[0] + s0[1] + s0[D.stride[0]] + s0[D.stride[0] + 1]) << 1;
            }
            int sum = v;
            for (int m = 32; m >= 1; m >>= 1) sum += __shfl_xor(sum, m, 64);
            if ((tid & 63) == 0) s_red[4 + (tid >> 6)] = sum;
            __syncthreads();
            sum = s_red[4] + s_red[5] + s_red[6] + s_red[7];
            const int avg = (int)(int16_t)((sum + npix / 2) >> __builtin_ctz((unsigned)npix));
            const uint32_t js = min((bl.y >> 8) & 0xffu, 7u), idx = bl.y & 0xffu;      // cfl_idx_to_alpha
            const uint32_t su = ((js + 1) * 11) >> 5, sign = plane == 1 ? su : (js + 1) - 3 * su;
            const int mag = (int)(plane == 1 ? idx >> 4 : idx & 15u) + 1, alpha = sign == 0 ? 0 : (sign == 2 ? mag : -mag);
            if (tid < npix) {
                const int q6 = alpha * (int)(int16_t)(v - avg), m6 = ((q6 < 0 ? -q6 : q6) + 32) >> 6;
                uint8_t* o = dst + (size_t)r * stride + c;
                *o = (uint8_t)min(max((int)*o + (q6 < 0 ? -m6 : m6), 0), 255);
            }
            __syncthreads();
        }
        // ---- residual -> transform -> quantiser -> inverse -> reconstruction: the size's body on one block ----
        const uint32_t area = w * h;
        int32_t* qcoeff = (D.sbq[0] && off + area <= span) ? D.sbq[plane] + gsb * span + off
                                                           : reinterpret_cast<int32_t*>(S + svthost::IE_OFF_DUMP) + plane * svthost::IE_DUMP_COEFFS;
        uint16_t* eob = reinterpret_cast<uint16_t*>(result + k) + plane;
        const int16_t* iscan = D.iscan + kIeTab.iscan_first[txs] + (size_t)type * kIeTab.ncoeff[txs];
        const QParams& qp = D.qp[plane != 0][kIeTab.ls[txs]];
        if (tid == 0) hdr[3 + plane] = px | py << 16;
        __syncthreads();
        const uint32_t* xy = hdr + 3 + plane;
#define SVT_IE_STAGED(W, H) enc_staged_body<W, H, false, uint8_t, 8>(src, recon, recon, nullptr, qcoeff, nullptr, eob, nullptr, iscan, qp, (int)type, 1u, xy, src_stride, stride, stride, 0u, lds)
#define SVT_IE_CASE(N, W, H) case N: SVT_IE_STAGED(W, H); break;
#define SVT_IE_DEFAULT(N, W, H) default: SVT_IE_STAGED(W, H); break;
        if constexpr (KIND == 0) {
            switch (txs) {
            case 0: enc4_body<uint8_t, 8, false>(src, recon, recon, nullptr, qcoeff, nullptr, eob, nullptr, iscan, qp, 1, (int)type, 1u, xy, src_stride, stride, stride, 0u); break;
            SVT_IE_CASE(1, 8, 8) SVT_IE_CASE(2, 16, 16) SVT_IE_CASE(5, 4, 8) SVT_IE_CASE(6, 8, 4) SVT_IE_CASE(7, 8, 16) SVT_IE_CASE(8, 16, 8) SVT_IE_CASE(13, 4, 16)
            SVT_IE_DEFAULT(14, 16, 4)
            }
        } else if constexpr (KIND == 1) {
            switch (txs) {
            case 3: enc32_body<uint8_t, 8, false, false>(src, recon, recon, nullptr, qcoeff, nullptr, eob, nullptr, iscan, qp, type == 9 ? 1 : 0, 1u, xy, src_stride, stride, stride, 0u, reinterpret_cast<int32_t*>(lds)); break;
            SVT_IE_CASE(9, 16, 32) SVT_IE_CASE(10, 32, 16) SVT_IE_CASE(15, 8, 32)
            SVT_IE_DEFAULT(16, 32, 8)
            }
        } else if constexpr (KIND == 2) {
            switch (txs) { SVT_TX_CLASS1B(SVT_IE_CASE, SVT_IE_DEFAULT) }
        } else {
            enc64_body<uint8_t, 8, false>(src, recon, recon, nullptr, qcoeff, nullptr, eob, nullptr, iscan, qp, 1u, xy, src_stride, stride, stride, 0u, lds);
        }
#undef SVT_IE_STAGED
#undef SVT_IE_CASE
#undef SVT_IE_DEFAULT
        __syncthreads();
        if (plane == 0 && tid == 0 && *eob == 0) result[k].y &= 0xffffu;   // the luma type becomes DCT_DCT (:700-709)
    }
    __syncthreads();
    if (tid == 0) hdr[plane] = k;
}

}  // namespace svtdev

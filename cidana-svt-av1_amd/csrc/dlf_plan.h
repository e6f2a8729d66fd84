// dlf_plan.h — what the deblocking calls (svt_hip_dlf_mi_frame, svt_hip_dlf_apply_frame, svt_hip_dlf_search_frame) settle on the host
// before they enqueue: the checks, the limit and level tables (update_sharpness, av1_loop_filter_frame_init), the tile grid and the
// scratch size; and the two host helpers of the level pick (search_filter_level's walk over a table, the LPF_PICK_FROM_Q guess).
// Host only (no HIP header): tests/c/dlf_plan_host.cpp compiles it with g++; the kernels (kernel_dlf.h) call the same constexpr
// functions.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "../../include/svt_hip_dsp.h"
#include "av1_geom.h"
#include "host_err.h"

namespace svthost {

constexpr int DLF_TILE = 64, DLF_HALO = 8;               // luma samples; a chroma tile is 32 with the same halo
constexpr int DLF_LEVELS = 64, DLF_MAX_LEVEL = 63;
constexpr int DLF_THREADS = 256;
constexpr uint32_t DLF_MAX_SIDE = 65535, DLF_MAX_PICS = 65535;      // the pictures of a stack are the grid's z
constexpr int DLF_MODES = 25;                            // MB_MODE_COUNT
constexpr uint32_t DLF_MI_MAX_SIDE = 16384, DLF_MI_MAX_SB = 1u << 20;
constexpr int DLF_MI_THREADS = 256, DLF_MI_WAVES = DLF_MI_THREADS / 64;      // the scatter: one wave per superblock

constexpr int dlf_clamp(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

// update_sharpness (EbDeblockingFilter.c:608-627) and the hev threshold (:691-692) of a level
constexpr int dlf_lim(int level, int sharp) {
    int v = level >> ((sharp > 0) + (sharp > 4));
    if (sharp > 0 && v > 9 - sharp) v = 9 - sharp;
    return v < 1 ? 1 : v;
}
constexpr int dlf_mblim(int level, int sharp) { return 2 * (level + 2) + dlf_lim(level, sharp); }
constexpr int dlf_hev(int level) { return level >> 4; }

// mode_lf_lut (:602): NEARESTMV, NEARMV, NEWMV and the compound modes but GLOBAL_GLOBALMV are 1; a mode outside the table reads as DC_PRED
constexpr uint32_t kDlfModeLfBits = 0x17F6000u;
constexpr int dlf_mode_lf(int mode) { return mode >= 0 && mode < DLF_MODES ? (int)(kDlfModeLfBits >> mode & 1u) : 0; }
static_assert(dlf_mode_lf(13) == 1 && dlf_mode_lf(14) == 1 && dlf_mode_lf(15) == 0 && dlf_mode_lf(16) == 1 && dlf_mode_lf(17) == 1 && dlf_mode_lf(22) == 1 &&
              dlf_mode_lf(23) == 0 && dlf_mode_lf(24) == 1 && dlf_mode_lf(12) == 0 && dlf_mode_lf(0) == 0 && dlf_mode_lf(26) == 0, "mode_lf_lut");

// av1_loop_filter_frame_init (:698-764): the level of a unit under base level `base`, ref_delta = ref_deltas[ref_frame[0]] and
// mode_delta = mode_deltas[mode_lf_lut[mode]] for an inter unit, 0 for an intra one
constexpr int dlf_level(int base, bool delta_on, int ref_delta, int mode_delta) {
    if (!delta_on) return base;
    const int scale = 1 << (base >> 5);
    return dlf_clamp(base + ref_delta * scale + mode_delta * scale, 0, DLF_MAX_LEVEL);
}

// the transform side across an edge (txsize_horz_map / txsize_vert_map of the plane's transform size) and the prediction block's side
constexpr int dlf_tx_side(int plane, int dir, int bsize, int tx_size) {
    if (plane == 0) return dir == 0 ? kTxW[tx_size] : kTxH[tx_size];
    return dir == 0 ? bsize_uv_w(bsize) : bsize_uv_h(bsize);       // av1_get_max_uv_txsize: the 4:2:0 block's largest transform, 64 -> 32
}
constexpr int dlf_pu_side(int plane, int dir, int bsize) {
    const int s = dir == 0 ? kBsizeW[bsize] : kBsizeH[bsize];
    return plane == 0 ? s : geom_max(s / 2, 4);                // get_plane_block_size (ss_size_lookup)
}
// the filter length from the smaller of the two transform sides
constexpr int dlf_length(int plane, int min_side) { return min_side <= 4 ? 4 : (plane ? 6 : (min_side == 8 ? 8 : 14)); }

inline uint32_t dlf_tiles_x(uint32_t width) { return (width + DLF_TILE - 1) / DLF_TILE; }
inline uint32_t dlf_tiles_y(uint32_t height) { return (height + DLF_TILE - 1) / DLF_TILE; }

inline bool dlf_geometry_ok(uint32_t width, uint32_t height, uint32_t npics) {
    if (width == 0 || height == 0 || (width & 7) || (height & 7) || width > DLF_MAX_SIDE || height > DLF_MAX_SIDE || npics == 0 || npics > DLF_MAX_PICS) return false;
    return (uint64_t)dlf_tiles_x(width) * dlf_tiles_y(height) * npics <= 0x3fffffffull;
}
// per (picture, plane, tile) 64 partial sums
inline size_t dlf_search_scratch_bytes(uint32_t width, uint32_t height, uint32_t npics) {
    if (!dlf_geometry_ok(width, height, npics)) return 0;
    return (size_t)dlf_tiles_x(width) * dlf_tiles_y(height) * npics * 3 * DLF_LEVELS * sizeof(uint64_t);
}

inline bool dlf_in_place(const svt_hip_dlf_pic* p) { return p->d_dst[0] == p->d_rec[0] && p->d_dst[1] == p->d_rec[1] && p->d_dst[2] == p->d_rec[2]; }

// bytes a stack of planes spans, for the overlap check
inline uint64_t dlf_span(uint32_t rows, uint32_t stride, uint32_t width, uint32_t npics, uint64_t pitch, int bytes) {
    return ((uint64_t)(npics - 1) * pitch + (uint64_t)(rows - 1) * stride + width) * (uint64_t)bytes;
}

inline int dlf_check(const svt_hip_dlf_pic* p, bool search) {
    if (!p) return set_err(SVT_HIP_ERR_INVALID, "NULL picture descriptor");
    if (p->bit_depth != 8 && p->bit_depth != 10) return set_err(SVT_HIP_ERR_INVALID, "bit depth %d (8 or 10)", p->bit_depth);
    if (p->npics < 1 || p->npics > DLF_MAX_PICS) return set_err(SVT_HIP_ERR_INVALID, "npics %u (1 .. %u)", p->npics, DLF_MAX_PICS);
    if (!dlf_geometry_ok(p->width, p->height, p->npics))
        return set_err(SVT_HIP_ERR_INVALID, "picture %u x %u: both sides must be non-zero multiples of 8, at most %u", p->width, p->height, DLF_MAX_SIDE);
    if (!p->d_mi || ((uintptr_t)p->d_mi & 3) || p->mi_stride < p->width / 4) return set_err(SVT_HIP_ERR_INVALID, "grid NULL, misaligned or mi_stride below width / 4");
    if (p->sharpness_level < 0 || p->sharpness_level > 7) return set_err(SVT_HIP_ERR_INVALID, "sharpness %d (0 .. 7)", p->sharpness_level);
    if (!search) {
        const int lv[4] = {p->filter_level[0], p->filter_level[1], p->filter_level_u, p->filter_level_v};
        for (int i = 0; i < 4; i++)
            if (lv[i] < 0 || lv[i] > DLF_MAX_LEVEL) return set_err(SVT_HIP_ERR_INVALID, "filter level %d (0 .. 63)", lv[i]);
    }
    for (int i = 0; i < 8; i++)
        if (p->ref_deltas[i] < -63 || p->ref_deltas[i] > 63) return set_err(SVT_HIP_ERR_INVALID, "ref_deltas[%d] = %d (-63 .. 63)", i, p->ref_deltas[i]);
    for (int i = 0; i < 2; i++)
        if (p->mode_deltas[i] < -63 || p->mode_deltas[i] > 63) return set_err(SVT_HIP_ERR_INVALID, "mode_deltas[%d] = %d (-63 .. 63)", i, p->mode_deltas[i]);
    const int bytes = p->bit_depth == 8 ? 1 : 2;
    int same = 0;
    for (int i = 0; i < 3; i++) {
        const uint32_t w = i ? p->width / 2 : p->width;
        if (!p->d_rec[i] || p->rec_stride[i] < w || ((uintptr_t)p->d_rec[i] & (bytes - 1)))
            return set_err(SVT_HIP_ERR_INVALID, "plane %d: input NULL, misaligned or stride below the width", i);
        if (search && (!p->d_src[i] || p->src_stride[i] < w || ((uintptr_t)p->d_src[i] & (bytes - 1))))
            return set_err(SVT_HIP_ERR_INVALID, "plane %d: source NULL, misaligned or stride below the width", i);
        if (!search) {
            if (!p->d_dst[i] || p->dst_stride[i] < w || ((uintptr_t)p->d_dst[i] & (bytes - 1)))
                return set_err(SVT_HIP_ERR_INVALID, "plane %d: output NULL, misaligned or stride below the width", i);
            same += p->d_dst[i] == p->d_rec[i];
        }
    }
    if (!search) {
        if (same != 0 && same != 3) return set_err(SVT_HIP_ERR_INVALID, "in place means all three planes: %d of d_dst equal d_rec", same);
        if (same == 3) {
            for (int i = 0; i < 3; i++)
                if (p->dst_stride[i] != p->rec_stride[i] || (p->npics > 1 && p->dst_pitch[i] != p->rec_pitch[i]))
                    return set_err(SVT_HIP_ERR_INVALID, "plane %d: in place with another stride or pitch", i);
        } else {
            for (int i = 0; i < 3; i++)
                for (int j = 0; j < 3; j++) {
                    const uint32_t wi = i ? p->width / 2 : p->width, hi = i ? p->height / 2 : p->height;
                    const uint32_t wj = j ? p->width / 2 : p->width, hj = j ? p->height / 2 : p->height;
                    const uintptr_t d0 = (uintptr_t)p->d_dst[i], d1 = d0 + dlf_span(hi, p->dst_stride[i], wi, p->npics, p->dst_pitch[i], bytes);
                    const uintptr_t r0 = (uintptr_t)p->d_rec[j], r1 = r0 + dlf_span(hj, p->rec_stride[j], wj, p->npics, p->rec_pitch[j], bytes);
                    if (d0 < r1 && r0 < d1) return set_err(SVT_HIP_ERR_INVALID, "d_dst[%d] overlaps d_rec[%d] without being equal", i, j);
                }
        }
    }
    return SVT_HIP_OK;
}

inline int dlf_search_check(const svt_hip_dlf_pic* p, const uint64_t* mask, const void* d_sse, const void* d_scratch, size_t scratch_bytes) {
    if (int rc = dlf_check(p, true)) return rc;
    if (!mask) return set_err(SVT_HIP_ERR_INVALID, "NULL mask");
    if (!d_sse || ((uintptr_t)d_sse & 7)) return set_err(SVT_HIP_ERR_INVALID, "NULL or misaligned d_sse");
    if (!d_scratch || ((uintptr_t)d_scratch & 7) || scratch_bytes < dlf_search_scratch_bytes(p->width, p->height, p->npics))
        return set_err(SVT_HIP_ERR_INVALID, "scratch: NULL, misaligned or %zu bytes of %zu", scratch_bytes, dlf_search_scratch_bytes(p->width, p->height, p->npics));
    return SVT_HIP_OK;
}

inline uint32_t dlf_mi_sb_pitch(const svt_hip_dlf_mi_args* a) { return a->sb_pitch ? a->sb_pitch : a->nsb; }
inline uint32_t dlf_mi_grid(uint32_t units) { return (units + DLF_MI_WAVES - 1) / DLF_MI_WAVES; }
inline int dlf_mi_check(const svt_hip_dlf_mi_args* a) {
    if (!a) return set_err(SVT_HIP_ERR_INVALID, "NULL arguments");
    if (!a->d_final || !a->d_final_count || !a->d_info || !a->d_mi) return set_err(SVT_HIP_ERR_INVALID, "NULL member");
    if ((((uintptr_t)a->d_final | (uintptr_t)a->d_final_count | (uintptr_t)a->d_info | (uintptr_t)a->d_mi) & 3)) return set_err(SVT_HIP_ERR_INVALID, "misaligned buffer (4 bytes)");
    if (a->npics == 0 || a->nsb == 0 || a->nsrc == 0) return set_err(SVT_HIP_ERR_INVALID, "npics %u, nsb %u, nsrc %u", a->npics, a->nsb, a->nsrc);
    if (a->sb_pitch && a->sb_pitch < a->nsb) return set_err(SVT_HIP_ERR_INVALID, "sb_pitch %u below nsb %u", a->sb_pitch, a->nsb);
    if ((uint64_t)a->npics * dlf_mi_sb_pitch(a) > DLF_MI_MAX_SB) return set_err(SVT_HIP_ERR_INVALID, "npics * sb_pitch above %u", DLF_MI_MAX_SB);
    if (a->mi_cols == 0 || a->mi_rows == 0 || a->mi_cols > DLF_MI_MAX_SIDE || a->mi_rows > DLF_MI_MAX_SIDE || a->mi_stride < a->mi_cols)
        return set_err(SVT_HIP_ERR_INVALID, "grid %u x %u, stride %u", a->mi_cols, a->mi_rows, a->mi_stride);
    return SVT_HIP_OK;
}

// ---- the level pick -------------------------------------------------------------------------------------------------------------
// search_filter_level (:1711-1848) over a table; an entry below 0 is "not computed"
inline int dlf_pick_level(const int64_t* ss_err, int start_level, int loop_filter_mode, bool only_4x4, int* level, int* need) {
    if (!ss_err || !level) return set_err(SVT_HIP_ERR_INVALID, "NULL table or output");
    int filt_mid = dlf_clamp(start_level, 0, DLF_MAX_LEVEL);
    int filter_step = filt_mid < 16 ? 4 : filt_mid / 4;
    int filt_direction = 0;
#define DLF_NEED(l) do { if (ss_err[l] < 0) { if (need) *need = (l); return SVT_HIP_DLF_NEED_LEVEL; } } while (0)
    DLF_NEED(filt_mid);
    int64_t best_err = ss_err[filt_mid];
    int filt_best = filt_mid;
    const bool one_step = loop_filter_mode <= 2;
    if (one_step) filter_step = 2;
    while (filter_step > 0) {
        const int filt_high = filt_mid + filter_step > DLF_MAX_LEVEL ? DLF_MAX_LEVEL : filt_mid + filter_step;
        const int filt_low = filt_mid - filter_step < 0 ? 0 : filt_mid - filter_step;
        int64_t bias = (best_err >> (15 - (filt_mid / 8))) * filter_step;      // against raising the level
        if (!only_4x4) bias >>= 1;
        if (filt_direction <= 0 && filt_low != filt_mid) {
            DLF_NEED(filt_low);
            if (ss_err[filt_low] < best_err + bias) {                           // close to the best: prefer the lower level
                if (ss_err[filt_low] < best_err) best_err = ss_err[filt_low];
                filt_best = filt_low;
            }
        }
        if (filt_direction >= 0 && filt_high != filt_mid) {
            DLF_NEED(filt_high);
            if (ss_err[filt_high] < best_err - bias) {                          // significantly better
                best_err = ss_err[filt_high];
                filt_best = filt_high;
            }
        }
        if (one_step) break;
        if (filt_best == filt_mid) {
            filter_step /= 2;
            filt_direction = 0;
        } else {
            filt_direction = filt_best < filt_mid ? -1 : 1;
            filt_mid = filt_best;
        }
    }
#undef DLF_NEED
    *level = filt_best;
    return SVT_HIP_OK;
}

// the LPF_PICK_FROM_Q branch of av1_pick_filter_level (:1867-1909); q = av1_ac_quant_Q3(base_qindex, 0, bit_depth)
inline void dlf_level_from_q(int q, int bit_depth, bool key, int levels[4]) {
    auto rpot = [](int64_t v, int n) { return (int)((v + ((int64_t)1 << (n - 1))) >> n); };
    int guess;
    if (bit_depth == 8) guess = key ? rpot((int64_t)q * 17563 - 421574, 18) : rpot((int64_t)q * 6017 + 650707, 18);
    else if (bit_depth == 10) guess = rpot((int64_t)q * 20723 + 4060632, 20);
    else guess = rpot((int64_t)q * 20723 + 16242526, 22);
    if (bit_depth != 8 && key) guess -= 4;
    guess = guess > 2 ? guess - 2 : (guess > 1 ? guess - 1 : guess);
    const int chroma = guess > 1 ? guess / 2 : guess;
    levels[0] = levels[1] = dlf_clamp(guess, 0, DLF_MAX_LEVEL);
    levels[2] = levels[3] = dlf_clamp(chroma, 0, DLF_MAX_LEVEL);
}

}  // namespace svthost

// svt_hip_dlf.hip — deblocking of whole pictures: svt_hip_dlf_mi_frame (final list -> mode-info grid), svt_hip_dlf_apply_frame
// (av1_loop_filter_frame) and svt_hip_dlf_search_frame (ss_err[level] per plane), kernels in kernel_dlf.h; the host helpers of the
// level pick.  The checks, the tables and the scratch size are dlf_plan.h's.
#include <stddef.h>

#include "gen/qlookup_gen.h"
#include "host_common.h"
#include "kernel_dlf.h"

using namespace svtdev;
using namespace svthost;

static_assert(sizeof(svt_hip_dlf_pic) == 272 && offsetof(svt_hip_dlf_pic, rec_pitch) == 152 && offsetof(svt_hip_dlf_pic, filter_level) == 232 &&
              offsetof(svt_hip_dlf_pic, ref_deltas) == 256, "svt_hip_dlf_pic layout");
static_assert(sizeof(svt_hip_dlf_mi) == 4 && offsetof(svt_hip_dlf_mi, tx_size) == 1 && offsetof(svt_hip_dlf_mi, ref_frame_skip) == 2 &&
              offsetof(svt_hip_dlf_mi, mode) == 3, "svt_hip_dlf_mi as one word");
static_assert(sizeof(svt_hip_dlf_info) == 4 && offsetof(svt_hip_dlf_info, mode) == 1 && offsetof(svt_hip_dlf_info, skip) == 2, "svt_hip_dlf_info as one word");
static_assert(sizeof(svt_hip_dlf_mi_args) == 72, "svt_hip_dlf_mi_args layout");
static_assert(sizeof(svt_hip_part_final) == 12 && offsetof(svt_hip_part_final, x) == 2 && offsetof(svt_hip_part_final, y) == 4 &&
              offsetof(svt_hip_part_final, src) == 8, "dlf_mi_kernel reads svt_hip_part_final as three words");

static DlfDev dlf_dev(const svt_hip_dlf_pic* p) {
    DlfDev d;
    memset(&d, 0, sizeof(d));
    for (int i = 0; i < 3; i++) {
        d.rec[i] = p->d_rec[i]; d.src[i] = p->d_src[i]; d.dst[i] = p->d_dst[i];
        d.rec_stride[i] = p->rec_stride[i]; d.src_stride[i] = p->src_stride[i]; d.dst_stride[i] = p->dst_stride[i];
        d.rec_pitch[i] = p->rec_pitch[i]; d.src_pitch[i] = p->src_pitch[i]; d.dst_pitch[i] = p->dst_pitch[i];
    }
    d.mi = (const uint32_t*)p->d_mi; d.mi_stride = p->mi_stride; d.mi_pitch = p->mi_pitch;
    d.width = p->width; d.height = p->height; d.ntx = dlf_tiles_x(p->width); d.nty = dlf_tiles_y(p->height);
    d.sh = p->bit_depth - 8; d.sharp = p->sharpness_level; d.delta_on = p->mode_ref_delta_enabled != 0;
    for (int i = 0; i < 8; i++) d.rd |= (unsigned long long)(uint8_t)p->ref_deltas[i] << (8 * i);
    for (int i = 0; i < 2; i++) d.md |= (uint32_t)(uint8_t)p->mode_deltas[i] << (8 * i);
    return d;
}

extern "C" int svt_hip_dlf_check(const svt_hip_dlf_pic* pic, int for_search) { return dlf_check(pic, for_search != 0); }
extern "C" int svt_hip_dlf_mi_check(const svt_hip_dlf_mi_args* a) { return dlf_mi_check(a); }
extern "C" size_t svt_hip_dlf_search_scratch_bytes(uint32_t width, uint32_t height, uint32_t npics) { return dlf_search_scratch_bytes(width, height, npics); }

extern "C" int svt_hip_dlf_limits(int level, int sharpness_level, uint8_t out[3]) {
    if (level < 0 || level > DLF_MAX_LEVEL || sharpness_level < 0 || sharpness_level > 7 || !out)
        return set_err(SVT_HIP_ERR_INVALID, "level %d (0 .. 63), sharpness %d (0 .. 7) or NULL out", level, sharpness_level);
    out[0] = (uint8_t)dlf_lim(level, sharpness_level); out[1] = (uint8_t)dlf_mblim(level, sharpness_level); out[2] = (uint8_t)dlf_hev(level);
    return SVT_HIP_OK;
}

extern "C" int svt_hip_dlf_levels(const svt_hip_dlf_pic* p, uint8_t out[3][2][8][2]) {
    if (!p || !out) return set_err(SVT_HIP_ERR_INVALID, "NULL argument");
    const int base[3][2] = {{p->filter_level[0], p->filter_level[1]}, {p->filter_level_u, p->filter_level_u}, {p->filter_level_v, p->filter_level_v}};
    for (int pl = 0; pl < 3; pl++)
        for (int dir = 0; dir < 2; dir++) {
            if (base[pl][dir] < 0 || base[pl][dir] > DLF_MAX_LEVEL) return set_err(SVT_HIP_ERR_INVALID, "filter level %d (0 .. 63)", base[pl][dir]);
            for (int ref = 0; ref < 8; ref++)
                for (int m = 0; m < 2; m++)
                    out[pl][dir][ref][m] = (uint8_t)dlf_level(base[pl][dir], p->mode_ref_delta_enabled != 0, p->ref_deltas[ref], ref ? p->mode_deltas[m] : 0);
        }
    return SVT_HIP_OK;
}

extern "C" int svt_hip_dlf_pick_level(const int64_t ss_err[64], int start_level, int loop_filter_mode, int tx_mode_is_only_4x4, int* level, int* need) {
    return dlf_pick_level(ss_err, start_level, loop_filter_mode, tx_mode_is_only_4x4 != 0, level, need);
}

extern "C" int svt_hip_dlf_level_from_q(int base_qindex, int bit_depth, int is_key_frame, int levels[4]) {
    if (base_qindex < 0 || base_qindex > 255 || (bit_depth != 8 && bit_depth != 10 && bit_depth != 12) || !levels)
        return set_err(SVT_HIP_ERR_INVALID, "base_qindex %d (0 .. 255), bit depth %d (8, 10, 12) or NULL levels", base_qindex, bit_depth);
    dlf_level_from_q(kAcQLookup[(bit_depth - 8) / 2][base_qindex], bit_depth, is_key_frame != 0, levels);
    return SVT_HIP_OK;
}

extern "C" int svt_hip_dlf_mi_frame(const svt_hip_dlf_mi_args* a, void* stream) {
    if (int rc = require_init()) return rc;
    if (int rc = dlf_mi_check(a)) return rc;
    DlfMiDev D;
    D.final_blk = (const uint32_t*)a->d_final; D.final_count = a->d_final_count; D.info = (const uint32_t*)a->d_info; D.mi = (uint32_t*)a->d_mi;
    D.npics = a->npics; D.nsb = a->nsb; D.sb_pitch = dlf_mi_sb_pitch(a); D.nsrc = a->nsrc;
    D.mi_cols = a->mi_cols; D.mi_rows = a->mi_rows; D.mi_stride = a->mi_stride; D.mi_pitch = a->mi_pitch;
    hipLaunchKernelGGL(dlf_mi_kernel, dim3(dlf_mi_grid(a->npics * a->nsb)), dim3(DLF_MI_THREADS), 0, (hipStream_t)stream, D);
    return launch_status("dlf_mi_frame");
}

extern "C" int svt_hip_dlf_apply_frame(const svt_hip_dlf_pic* pic, void* stream) {
    if (int rc = require_init()) return rc;
    if (int rc = dlf_check(pic, false)) return rc;
    hipStream_t s = (hipStream_t)stream;
    DlfDev d = dlf_dev(pic);
    const bool in_place = dlf_in_place(pic);
    // loop_filter_sb's gate (:1297-1303): both luma levels 0 end the plane loop; a chroma level 0 skips that plane
    const bool luma = pic->filter_level[0] || pic->filter_level[1];
    const bool on[3] = {luma, luma && pic->filter_level_u != 0, luma && pic->filter_level_v != 0};
    const int base[3][2] = {{pic->filter_level[0], pic->filter_level[1]}, {pic->filter_level_u, pic->filter_level_u}, {pic->filter_level_v, pic->filter_level_v}};
    for (int i = 0; i < 3; i++) {
        d.plane_mode[i] = on[i] ? 2 : (in_place ? 0 : 1);
        d.lvl[i][0] = base[i][0]; d.lvl[i][1] = base[i][1];
    }
    if (!in_place) {
        if (pic->bit_depth == 8) hipLaunchKernelGGL((dlf_tile_kernel<uint8_t, false>), dim3(d.ntx * d.nty, 3, pic->npics), dim3(DLF_NT), 0, s, d);
        else hipLaunchKernelGGL((dlf_tile_kernel<uint16_t, false>), dim3(d.ntx * d.nty, 3, pic->npics), dim3(DLF_NT), 0, s, d);
        return launch_status("dlf_apply_frame");
    }
    if (!luma) return SVT_HIP_OK;                              // nothing is filtered
    const uint32_t wgs = (uint32_t)(((uint64_t)(pic->width / 4) * pic->height + DLF_NT - 1) / DLF_NT);
    for (int dir = 0; dir < 2; dir++) {
        if (pic->bit_depth == 8) hipLaunchKernelGGL(dlf_pass_kernel<uint8_t>, dim3(wgs, 3, pic->npics), dim3(DLF_NT), 0, s, d, dir);
        else hipLaunchKernelGGL(dlf_pass_kernel<uint16_t>, dim3(wgs, 3, pic->npics), dim3(DLF_NT), 0, s, d, dir);
        if (int rc = launch_status("dlf_apply_frame (in place)")) return rc;
    }
    return SVT_HIP_OK;
}

extern "C" int svt_hip_dlf_search_frame(const svt_hip_dlf_pic* pic, const uint64_t mask[3], uint64_t* d_sse, void* d_scratch, size_t scratch_bytes,
                                        void* stream) {
    if (int rc = require_init()) return rc;
    if (int rc = dlf_search_check(pic, mask, d_sse, d_scratch, scratch_bytes)) return rc;
    hipStream_t s = (hipStream_t)stream;
    DlfDev d = dlf_dev(pic);
    for (int i = 0; i < 3; i++) d.mask[i] = mask[i];
    d.partial = (unsigned long long*)d_scratch; d.sse = (unsigned long long*)d_sse;
    if (mask[0] | mask[1] | mask[2]) {
        if (pic->bit_depth == 8) hipLaunchKernelGGL((dlf_tile_kernel<uint8_t, true>), dim3(d.ntx * d.nty, 3, pic->npics), dim3(DLF_NT), 0, s, d);
        else hipLaunchKernelGGL((dlf_tile_kernel<uint16_t, true>), dim3(d.ntx * d.nty, 3, pic->npics), dim3(DLF_NT), 0, s, d);
        if (int rc = launch_status("dlf_search_frame")) return rc;
    }
    hipLaunchKernelGGL(dlf_sum_kernel, dim3(pic->npics * 3), dim3(64), 0, s, d);
    return launch_status("dlf_search_frame (sum)");
}

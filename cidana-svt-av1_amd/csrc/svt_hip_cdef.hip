// svt_hip_cdef.hip — svt_hip_cdef_search_frame / svt_hip_cdef_apply_frame: the CDEF strength search and the CDEF apply for whole
// pictures (cdef_kernel, kernel_cdef.h), one launch per call.
#include "host_common.h"
#include "kernel_cdef.h"

using namespace svtdev;
using namespace svthost;

static_assert(sizeof(svt_hip_cdef_pic) == 232, "svt_hip_cdef_pic layout");

static int cdef_check(const svt_hip_cdef_pic* p, bool apply) {
    if (!p) return set_err(SVT_HIP_ERR_INVALID, "NULL picture descriptor");
    if (p->bit_depth != 8 && p->bit_depth != 10) return set_err(SVT_HIP_ERR_INVALID, "bit depth %d (8 or 10)", p->bit_depth);
    if (p->width == 0 || p->height == 0 || (p->width & 7) || (p->height & 7) || p->width > 65536 || p->height > 65536)
        return set_err(SVT_HIP_ERR_INVALID, "picture %u x %u: both sides must be multiples of 8 (at most 65536)", p->width, p->height);
    if (p->base_qindex < 0 || p->base_qindex > 255) return set_err(SVT_HIP_ERR_INVALID, "base_qindex %d", p->base_qindex);
    if (p->npics < 1) return set_err(SVT_HIP_ERR_INVALID, "npics %u", p->npics);
    if (!p->d_skip || p->skip_stride < p->width / 8) return set_err(SVT_HIP_ERR_INVALID, "skip map NULL or skip_stride below width / 8");
    for (int i = 0; i < 3; i++) {
        const uint32_t w = i ? p->width / 2 : p->width;
        if (!p->d_rec[i] || p->rec_stride[i] < w) return set_err(SVT_HIP_ERR_INVALID, "plane %d: input NULL or stride below the width", i);
        if (!apply && (!p->d_src[i] || p->src_stride[i] < w)) return set_err(SVT_HIP_ERR_INVALID, "plane %d: source NULL or stride below the width", i);
        if (apply && (!p->d_dst[i] || p->dst_stride[i] < w)) return set_err(SVT_HIP_ERR_INVALID, "plane %d: output NULL or stride below the width", i);
        if (apply && p->d_dst[i] == p->d_rec[i]) return set_err(SVT_HIP_ERR_INVALID, "plane %d: the apply does not run in place", i);
    }
    const uint64_t nfb = (uint64_t)((p->width + 63) / 64) * ((p->height + 63) / 64);
    if (nfb * p->npics > 0x7fffffffull) return set_err(SVT_HIP_ERR_INVALID, "too many filter blocks");
    return SVT_HIP_OK;
}

static CdefDev cdef_dev(const svt_hip_cdef_pic* p) {
    CdefDev d;
    memset(&d, 0, sizeof(d));
    for (int i = 0; i < 3; i++) {
        d.rec[i] = p->d_rec[i]; d.src[i] = p->d_src[i]; d.dst[i] = p->d_dst[i];
        d.rec_stride[i] = p->rec_stride[i]; d.src_stride[i] = p->src_stride[i]; d.dst_stride[i] = p->dst_stride[i];
        d.rec_pitch[i] = p->rec_pitch[i]; d.src_pitch[i] = p->src_pitch[i]; d.dst_pitch[i] = p->dst_pitch[i];
    }
    d.skip = p->d_skip; d.skip_stride = p->skip_stride; d.skip_pitch = p->skip_pitch;
    d.width = p->width; d.height = p->height;
    d.nhfb = (p->width + 63) / 64; d.nvfb = (p->height + 63) / 64;
    d.cs = p->bit_depth - 8;
    d.damping = 3 + (p->base_qindex >> 6);
    return d;
}

// waves wanted in flight: a small picture splits the strength window over blockIdx.z until it has about this many
static constexpr uint32_t kCdefTargetWaves = 8192;
static constexpr int kCdefMinChunk = 8;        // strengths per chunk at least: the tile, directions and source sums are per chunk

extern "C" int svt_hip_cdef_search_frame(const svt_hip_cdef_pic* pic, int start_gi, int end_gi, uint64_t* d_mse, int32_t* d_count, void* stream) {
    if (int rc = require_init()) return rc;
    if (int rc = cdef_check(pic, false)) return rc;
    if (start_gi < 0 || end_gi > 64 || start_gi >= end_gi) return set_err(SVT_HIP_ERR_INVALID, "strength window %d .. %d (inside 0 .. 64, not empty)", start_gi, end_gi);
    if (!d_mse || !d_count || ((uintptr_t)d_mse & 7) || ((uintptr_t)d_count & 3)) return set_err(SVT_HIP_ERR_INVALID, "NULL or misaligned output");
    CdefDev d = cdef_dev(pic);
    d.start_gi = start_gi; d.end_gi = end_gi;
    d.mse = (unsigned long long*)d_mse; d.count = d_count;
    const uint32_t wgs = d.nhfb * d.nvfb * pic->npics;
    const int ngi = end_gi - start_gi;
    int chunks = (int)((kCdefTargetWaves + wgs * 8 - 1) / (wgs * 8));
    chunks = chunks > ngi / kCdefMinChunk ? ngi / kCdefMinChunk : chunks;
    chunks = chunks < 1 ? 1 : chunks;
    d.gpc = (ngi + chunks - 1) / chunks;
    chunks = (ngi + d.gpc - 1) / d.gpc;
    if (pic->bit_depth == 8)
        hipLaunchKernelGGL((cdef_kernel<uint8_t, false>), dim3(wgs, 2, chunks), dim3(CDEF_THREADS), 0, (hipStream_t)stream, d);
    else
        hipLaunchKernelGGL((cdef_kernel<uint16_t, false>), dim3(wgs, 2, chunks), dim3(CDEF_THREADS), 0, (hipStream_t)stream, d);
    return launch_status("cdef_search_frame");
}

extern "C" int svt_hip_cdef_apply_frame(const svt_hip_cdef_pic* pic, const int8_t* d_luma_strength, const int8_t* d_chroma_strength, void* stream) {
    if (int rc = require_init()) return rc;
    if (int rc = cdef_check(pic, true)) return rc;
    if (!d_luma_strength || !d_chroma_strength) return set_err(SVT_HIP_ERR_INVALID, "NULL strength array");
    CdefDev d = cdef_dev(pic);
    d.ystr = d_luma_strength; d.uvstr = d_chroma_strength;
    const uint32_t wgs = d.nhfb * d.nvfb * pic->npics;
    if (pic->bit_depth == 8)
        hipLaunchKernelGGL((cdef_kernel<uint8_t, true>), dim3(wgs, 2, 1), dim3(CDEF_THREADS), 0, (hipStream_t)stream, d);
    else
        hipLaunchKernelGGL((cdef_kernel<uint16_t, true>), dim3(wgs, 2, 1), dim3(CDEF_THREADS), 0, (hipStream_t)stream, d);
    return launch_status("cdef_apply_frame");
}

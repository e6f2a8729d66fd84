// pixel_plan.h — what the simple pixel calls of svt_hip_pixel.hip (svt_hip_sad_* / svt_hip_sse_batch, svt_hip_residual*_batch,
// svt_hip_full_distortion32_batch and its picture form) settle on the host before they enqueue: every clause after the empty-batch return,
// in the order a caller observes it, the kernel variant and the grid.  Host only (no HIP header): tests/c/me_plan_host.cpp compiles it
// with g++ next to me_plan.h.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "../../include/svt_hip_dsp.h"
#include "host_err.h"
#include "me_plan.h"

namespace svthost {

// ---- SAD / SSE / averaging SAD: 16 blocks (of 16 lanes) per workgroup -----------------------------------------------------------------
enum { SAD_MODE_SAD = 0, SAD_MODE_SSE = 1, SAD_MODE_AVG = 2 };
enum { SAD_NEEDS_A_OFFS = 1, SAD_NEEDS_B_OFFS = 2 };     // the *_planes_batch form needs both tables, x4d the references'
struct SadSsePlan { int mode; uint32_t grid, n; const char* name; };
// a_shift = 2: four references per source block (x4d), n source blocks -> 4 n kernel blocks.  (Without it the count has no bound: the
// kernel's 32-bit count is the cast of n, as it always was)
inline int sad_sse_plan(SadSsePlan& p, int mode, int needs_offs, int a_shift, const void* a, const void* a_offs, const void* b, const void* b_offs, const void* c,
                        const void* out, uint32_t w, uint32_t h, size_t n) {
    p = SadSsePlan{};
    if (((needs_offs & SAD_NEEDS_A_OFFS) && !a_offs) || ((needs_offs & SAD_NEEDS_B_OFFS) && !b_offs)) return set_err(SVT_HIP_ERR_INVALID, "NULL offset table");
    if (a_shift && n > 0x3fffffffu) return set_err(SVT_HIP_ERR_INVALID, "too many blocks");
    n <<= a_shift;
    if (!a || !b || !out || (mode == SAD_MODE_AVG && !c)) return set_err(SVT_HIP_ERR_INVALID, "NULL buffer");
    if (w == 0 || h == 0 || w > 128 || h > 128) return set_err(SVT_HIP_ERR_INVALID, "block %ux%u", w, h);
    p.mode = mode == SAD_MODE_SSE || mode == SAD_MODE_AVG ? mode : SAD_MODE_SAD;
    p.grid = (uint32_t)((n + 15) / 16);
    p.n = (uint32_t)n;
    p.name = p.mode == SAD_MODE_SSE ? "sse" : (p.mode == SAD_MODE_AVG ? "sad_avg" : "sad");
    return SVT_HIP_OK;
}

// ---- residual: one lane per group of rcs samples of a row -----------------------------------------------------------------------------
// rcs: samples per lane - 16 bytes of input where the width allows it (es: bytes per sample), else 8, 4 or 1 samples; cpr lanes per row;
// pow2: lanes per row and per block are powers of two (the kernel then shifts where it would divide)
struct ResidualPlan { uint32_t rcs, cpr, grid; bool pow2; };
inline int residual_plan(ResidualPlan& p, uint32_t es, const void* d_src, const void* d_pred, const void* d_res, uint32_t width, uint32_t height, size_t nblocks) {
    p = ResidualPlan{};
    if (!d_src || !d_pred || !d_res) return set_err(SVT_HIP_ERR_INVALID, "NULL buffer");
    if (width == 0 || height == 0) return set_err(SVT_HIP_ERR_INVALID, "empty block");
    const uint32_t maxcs = 16 / es;
    p.rcs = (width % maxcs) == 0 ? maxcs : ((width & 7) == 0 ? 8u : ((width & 3) == 0 ? 4u : 1u));
    p.cpr = width / p.rcs;
    const size_t per = (size_t)p.cpr * height, total = per * nblocks, grid = (total + 255) / 256;
    if (grid > 0x7fffffffu) return set_err(SVT_HIP_ERR_INVALID, "too many blocks for one launch");
    p.grid = (uint32_t)grid;
    p.pow2 = (p.cpr & (p.cpr - 1)) == 0 && (per & (per - 1)) == 0;
    return SVT_HIP_OK;
}

// ---- coefficient-domain distortion: 16 blocks per workgroup ---------------------------------------------------------------------------
// picture_full_distortion32_bits (EbPictureOperators.c:349-457): a 64-sample dimension covers 32 coefficients
inline uint32_t dist32_picture_side(uint32_t side) { return side < 64 ? side : 32; }
struct Dist32Plan { int avx2; uint32_t grid; };
inline int full_distortion32_plan(Dist32Plan& p, const void* d_coeff, const void* d_recon, const void* d_out, uint32_t width, uint32_t height, int cbf_zero,
                                  int flavour, size_t nblocks) {
    p = Dist32Plan{};
    if (!d_coeff || !d_out || (!cbf_zero && !d_recon)) return set_err(SVT_HIP_ERR_INVALID, "NULL buffer");
    if (width == 0 || height == 0 || width > 128 || height > 128) return set_err(SVT_HIP_ERR_INVALID, "area %ux%u", width, height);
    if (int rc = me_flavour_check(flavour)) return rc;
    if (flavour == SVT_HIP_FLAVOUR_AVX2 && (width & 3)) return set_err(SVT_HIP_ERR_INVALID, "the AVX2 kernel is defined for widths that are a multiple of 4");
    p.avx2 = flavour == SVT_HIP_FLAVOUR_AVX2;
    p.grid = (uint32_t)((nblocks + 15) / 16);
    return SVT_HIP_OK;
}

}  // namespace svthost

// kernel_frame.h — enc_frame_kernel: the encode pass of the (plane, transform size) groups of a picture in ONE launch, or in one
// launch per REGISTER CLASS (SURVEY 8f n3 "one fused frame kernel"; BASELINE configs[3]).
//
// A launch covers the workgroups of all its groups back to back; a workgroup finds its group in a table that rides in the
// kernel arguments (no device-side descriptor memory: the call stays a pure enqueue and is graph-capturable), takes its index
// inside the group and runs that size's body - the same bodies the per-size kernels run (enc4_body, enc_staged_body<W, H>,
// enc32_body, enc64_body), so results are identical by construction.  A workgroup is homogeneous (one size); groups are ordered
// largest blocks first so the long workgroups start early.
//
// Registers.  The register file and the LDS of a launch are the maximum over the bodies it contains.  Round 2's single launch ran at
// the 64x64 body's budget (168 VGPRs at 3 waves / SIMD) and that body still spilled 20 B (8-bit) / 36 B (10-bit) per lane to
// SCRATCH.  With this round's LDS layouts (kernel_txfm_staged.h) every body fits 3 waves / SIMD without scratch, and the sizes can
// also be launched by register class (tools/kernel_resources.py):
//     class 0  every size up to 16 in both dimensions (4x4 .. 16x16, 4x8 .. 16x4)     <= 80 VGPRs, 6 waves / SIMD, 17 KiB LDS
//     class 1  32x32 and every rectangle with a 32- or 64-sample side                   <= 139 VGPRs, 3 - 4 waves / SIMD, 33 KiB LDS
//     class 2  64x64 (two blocks per wave, pruned 64-point networks)                    169 / 192 VGPRs, 2 waves / SIMD
//     class 3  the five square sizes in ONE launch at 3 waves / SIMD                    147 / 160 VGPRs
// One picture takes class 3 (three back-to-back launches each drain before the next fills the GPU: 0.066 against 0.049 ms for a
// 1080p picture, A/B on one box); a call with many pictures takes the class launches, where the small sizes - three fifths of a
// picture's pixel passes in configs[3] - run at twice the occupancy.  No kernel of this file uses scratch
// (tests/test_kernel_resources.py).  Covered: all 19 transform sizes, every transform type the reference defines for them,
// qcoeff + eob + recon outputs, 8 / 10 bit, power-of-two quant_shift tables.
#pragma once
#include "group_table.h"
#include "kernel_enc64.h"
#include "kernel_fused32.h"
#include "kernel_txfm_staged.h"

namespace svtdev {

constexpr int FRAME_MAX_GROUPS = 22;        // per launch: what fits the 4 KiB of kernel arguments
struct FrameGroupDev {
    const void* src; const void* pred; void* recon;
    int32_t* qcoeff; uint16_t* eob;
    const uint32_t* xy; const int16_t* iscan;
    uint32_t src_stride, pred_stride, recon_stride, nblocks;
    int32_t tx_size;                 // SVT_TX_4X4 .. SVT_TX_64X16 (0 .. 18)
    int32_t tx_type;                 // any type the reference defines for the size (32-point sides: DCT_DCT / IDTX, 64: DCT_DCT)
    uint32_t wg_end;                 // one past the last workgroup of this group in the launch
    QParams qp;                      // per group: log_scale differs with the size
};
struct FrameDesc {
    int32_t ngroups;
    FrameGroupDev g[FRAME_MAX_GROUPS];
};
static_assert(sizeof(FrameDesc) <= 4000, "kernel arguments");

// LDS of a size's body: enc4_body none, enc32_body the tuned kernel's, the staged bodies their own
#define SVT_FRAME_LDS(N, W, H) (W * H == 16 ? 0 : (W == 32 && H == 32 ? ENC32_LDS_BYTES : EncStagedLds<W, H, PixT>::BYTES)),
template <typename PixT, int CLS> struct FrameLds;
template <typename PixT> struct FrameLds<PixT, 0> { static constexpr int BYTES = cmax_of({SVT_TX_CLASS0(SVT_FRAME_LDS, SVT_FRAME_LDS)}); };
template <typename PixT> struct FrameLds<PixT, 1> { static constexpr int BYTES = cmax_of({SVT_TX_CLASS1(SVT_FRAME_LDS, SVT_FRAME_LDS)}); };
template <typename PixT> struct FrameLds<PixT, 2> { static constexpr int BYTES = E64_WAVES * E64_WAVE_LDS; };
template <typename PixT> struct FrameLds<PixT, 3> {       // every size in one launch
    static constexpr int BYTES = cmax(cmax(FrameLds<PixT, 0>::BYTES, FrameLds<PixT, 1>::BYTES), FrameLds<PixT, 2>::BYTES);
};
#undef SVT_FRAME_LDS

#define SVT_FRAME_STAGED(W, H)                                                                                                         \
    enc_staged_body<W, H, false, PixT, BD>(src, pred, recon, nullptr, G.qcoeff, nullptr, G.eob, nullptr, G.iscan, G.qp, G.tx_type, G.nblocks, G.xy, \
                                           G.src_stride, G.pred_stride, G.recon_stride, bid, lds)

// CLS 0 / 1 / 2: one register class; CLS 3: every size in ONE launch at 3 waves / SIMD (<= 168 registers: with the LDS layouts of
// this round the 64x64 body fits, 147 / 160 VGPRs, no scratch) - what a single picture takes: measured A/B on one box (configs[3],
// 1080p, five sizes) 0.049 ms against 0.066 ms for three class launches back to back, each of which drains before the next fills
// the GPU; the classes are for calls large enough to amortise that (a GOP per call).
template <int CLS> struct FrameWaves { static constexpr int MIN = CLS == 3 ? 3 : 1; };
template <typename PixT, int BD, int CLS>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(FrameWaves<CLS>::MIN))) void enc_frame_kernel(const FrameDesc fd) {
    __shared__ __attribute__((aligned(16))) char lds[FrameLds<PixT, CLS>::BYTES];
    uint32_t bid;
    const int gi = group_of(fd, bid);
    if (gi >= fd.ngroups) return;
    const FrameGroupDev& G = fd.g[gi];
    const PixT* src = reinterpret_cast<const PixT*>(G.src);
    const PixT* pred = reinterpret_cast<const PixT*>(G.pred);
    PixT* recon = reinterpret_cast<PixT*>(G.recon);
// a size's body: 4x4 and 32x32 have kernels of their own, every other size of classes 0 and 1 is staged
#define SVT_FRAME_BODY(W, H) if constexpr (W * H == 16) SVT_FRAME_ENC4; else if constexpr (W == 32 && H == 32) SVT_FRAME_ENC32; else SVT_FRAME_STAGED(W, H)
#define SVT_FRAME_CASE(N, W, H) case N: SVT_FRAME_BODY(W, H); break;
#define SVT_FRAME_DEFAULT(N, W, H) default: SVT_FRAME_BODY(W, H); break;          // the last size of a class
#define SVT_FRAME_ENC4 enc4_body<PixT, BD, false>(src, pred, recon, nullptr, G.qcoeff, nullptr, G.eob, nullptr, G.iscan, G.qp, 1, G.tx_type, G.nblocks, G.xy, G.src_stride, \
                                                  G.pred_stride, G.recon_stride, bid)
#define SVT_FRAME_ENC32 enc32_body<PixT, BD, false, false>(src, pred, recon, nullptr, G.qcoeff, nullptr, G.eob, nullptr, G.iscan, G.qp, G.tx_type == 9 /* IDTX */ ? 1 : 0, \
                                                           G.nblocks, G.xy, G.src_stride, G.pred_stride, G.recon_stride, bid, reinterpret_cast<int32_t*>(lds))
#define SVT_FRAME_ENC64 enc64_body<PixT, BD, false>(src, pred, recon, nullptr, G.qcoeff, nullptr, G.eob, nullptr, G.iscan, G.qp, G.nblocks, G.xy, G.src_stride, \
                                                    G.pred_stride, G.recon_stride, bid, lds)
    if constexpr (CLS == 3) {
        // the five SQUARE sizes only: with all nineteen bodies inlined into one function the compiler left their register arrays
        // in scratch (2.7 KiB per lane); a call with rectangular groups is launched by class
        switch (G.tx_size) {
        SVT_FRAME_CASE(0, 4, 4) SVT_FRAME_CASE(1, 8, 8) SVT_FRAME_CASE(2, 16, 16) SVT_FRAME_CASE(3, 32, 32)
        default: SVT_FRAME_ENC64; break;
        }
    } else if constexpr (CLS == 0) {
        switch (G.tx_size) { SVT_TX_CLASS0(SVT_FRAME_CASE, SVT_FRAME_DEFAULT) }
    } else if constexpr (CLS == 1) {
        switch (G.tx_size) { SVT_TX_CLASS1(SVT_FRAME_CASE, SVT_FRAME_DEFAULT) }
    } else {
        SVT_FRAME_ENC64;
    }
#undef SVT_FRAME_CASE
#undef SVT_FRAME_DEFAULT
#undef SVT_FRAME_BODY
#undef SVT_FRAME_ENC4
#undef SVT_FRAME_ENC32
#undef SVT_FRAME_ENC64
}
#undef SVT_FRAME_STAGED

}  // namespace svtdev

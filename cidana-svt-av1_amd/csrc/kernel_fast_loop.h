// kernel_fast_loop.h — the intra candidates of the mode-decision fast loop (perform_fast_loop, EbProductCodingLoop.c:1152-1300),
// fused: per block of a group and per candidate of the group's list, the prediction of build_intra_predictors (the bip steps of
// kernel_bip.h) and its distortion against the source block, 8 bytes out per (block, candidate).
//
// Same lane layout as bip_kernel: LPB lanes per block, 64 / LPB blocks per wave, BIP_WAVES waves per workgroup.  A block's raw edges,
// descriptor and source rows are loaded once, before the candidate loop, and stay in registers (the source: NI items of PPL bytes per
// lane, at most 16 VGPRs at 64x64).  Per candidate the edge stages run again from the raw registers (they filter the LDS edges in
// place, and strength and up-sampling depend on the angle), then the pixel step predicts into registers and the distortion is summed
// per lane and reduced over the block's lanes with shuffles.  The prediction reaches HBM only when the caller asks for it.
//
// Every block of a group shares the candidate list, so the mode and delta of a candidate are wave-uniform (read from the kernel
// arguments on a scalar): no ordering pass is needed for the waves' predictor kinds to agree.  Only availability, filt_type and
// disable_edge_filter vary per block; they can turn a block's kind into the constant fill or another DC variant.  The DC variants
// share one pixel code (v = dc) and dispatch as IM_DC; a wave whose blocks still differ runs the run-time switch (bip_by_kind).
// blockIdx.y splits the list into chunks of `cpc` candidates, so that a group of few large blocks still fills the device.
#pragma once
#include "kernel_bip.h"

namespace svtdev {

constexpr int FAST_MAX_CAND = 64;
enum { FAST_SAD = 0, FAST_SSD = 1, FAST_SSD_WRAP = 2 };      // device metrics: plain SAD, exact SSD, the SSSE3 kernels' wrapped-byte SSD

struct FastLoopDev {
    const uint8_t* src;
    const uint32_t* src_xy;                                   // NULL: dense W * H blocks
    const uint8_t* top;
    const uint8_t* left;
    const BipBlk* blks;
    unsigned long long* dist;                                 // [nblocks][ncand]
    uint8_t* pred;                                            // NULL, or [nblocks][ncand][H][W]
    uint32_t src_stride, nblocks;
    int32_t neigh_pitch, ncand, cpc, metric;
    uint8_t modes[FAST_MAX_CAND];
    int8_t deltas[FAST_MAX_CAND];
};

// sum over the N = 4 * NW samples of one item: s = the source bytes (packed), px = the prediction
template <int NW>
__device__ __forceinline__ uint32_t fast_item_dist(int metric, const uint32_t (&s)[NW], const int (&px)[4 * NW]) {
    uint32_t acc = 0;
    if (metric == FAST_SAD) {
#pragma unroll
        for (int k = 0; k < NW; k++) {
            const uint32_t pw = (uint32_t)px[4 * k] | ((uint32_t)px[4 * k + 1] << 8) | ((uint32_t)px[4 * k + 2] << 16) | ((uint32_t)px[4 * k + 3] << 24);
            acc = __builtin_amdgcn_sad_u8(s[k], pw, acc);
        }
    } else if (metric == FAST_SSD) {
#pragma unroll
        for (int k = 0; k < 4 * NW; k++) {
            const int d = (int)((s[k >> 2] >> (8 * (k & 3))) & 0xffu) - px[k];
            acc += (uint32_t)(d * d);
        }
    } else {
        // _mm_sub_epi8 then _mm_sign_epi8 (EbPictureOperators_Intrinsic_SSE4_1.c:495-620): the byte difference modulo 256 read as a
        // signed byte; its square equals the square of the zero-extended |.| the kernels go on with (-128 -> 128)
#pragma unroll
        for (int k = 0; k < 4 * NW; k++) {
            const int d = (int)(int8_t)(uint8_t)((int)((s[k >> 2] >> (8 * (k & 3))) & 0xffu) - px[k]);
            acc += (uint32_t)(d * d);
        }
    }
    return acc;
}

template <int W, int H>
__global__ __launch_bounds__(64 * BIP_WAVES) void fast_loop_kernel(const FastLoopDev fd) {
    using G = BipGeom<W, H>;
    constexpr int LPB = G::LPB, bpw = G::BPW, EL = G::EL, PPL = G::PPL, CPR = G::CPR, items = G::ITEMS, NI = G::NI, NW = PPL / 4;
    __shared__ __attribute__((aligned(16))) uint16_t s_edge[BIP_WAVES * bpw * 2 * EL];          // as bip_kernel
    __shared__ __attribute__((aligned(16))) uint32_t s_pair[BIP_WAVES * bpw * 2 * EL];
    const int wv = threadIdx.x >> 6, sub = (threadIdx.x & 63) >> G::LSH;
    const int lane = threadIdx.x & (LPB - 1);
    const uint32_t blk_id = (blockIdx.x * BIP_WAVES + (uint32_t)wv) * (uint32_t)bpw + (uint32_t)sub;
    const bool live = blk_id < fd.nblocks;
    const uint32_t b = live ? blk_id : 0u;                    // a spare group replays block 0 without storing
    // all global loads of the block side by side: raw edges, descriptor, source rows
    BipRaw<W, H> R;
    bip_load_raw<uint8_t, W, H>(R, fd.top + (size_t)b * fd.neigh_pitch + 1, fd.left + (size_t)b * fd.neigh_pitch + 1, lane);
    const BipBlk d = fd.blks[b];
    const uint8_t* sp;
    uint32_t sst;
    if (fd.src_xy) {
        const uint32_t xy = fd.src_xy[b];
        sp = fd.src + (size_t)(xy >> 16) * fd.src_stride + (xy & 0xffffu);
        sst = fd.src_stride;
    } else {
        sp = fd.src + (size_t)b * (W * H);
        sst = W;
    }
    uint32_t sw[NI][NW];
#pragma unroll
    for (int i = 0; i < NI; i++) {
        const int q = lane + i * LPB;
        const int r = q / CPR, c0 = (q % CPR) * PPL;
        const uint8_t* p = sp + (size_t)r * sst + c0;
        const bool in = items % LPB == 0 || q < items;
#pragma unroll
        for (int k = 0; k < NW; k++) sw[i][k] = 0;
        if (in) {
            if ((reinterpret_cast<uintptr_t>(p) & 3) == 0) {
#pragma unroll
                for (int k = 0; k < NW; k++) sw[i][k] = reinterpret_cast<const uint32_t*>(p)[k];
            } else {
#pragma unroll
                for (int k = 0; k < 4 * NW; k++) sw[i][k >> 2] |= (uint32_t)p[k] << (8 * (k & 3));
            }
        }
    }
    uint16_t* A = s_edge + (size_t)((wv * bpw + sub) * 2) * EL + 16;
    uint16_t* L = A + EL;
    uint32_t* PA = s_pair + (size_t)((wv * bpw + sub) * 2) * EL + 16;
    uint32_t* PL = PA + EL;
    const int c_begin = (int)blockIdx.y * fd.cpc, c_end = min(fd.ncand, c_begin + fd.cpc);
    for (int c = c_begin; c < c_end; c++) {
        wave_lds_fence();                                     // the previous candidate's pixel reads before this one's edge writes
        BipBlk dc = d;
        dc.mode = fd.modes[c];
        dc.angle_delta = fd.deltas[c];
        const BipPred P = bip_edges<W, H>(R, dc, A, L, PA, PL, 8, lane);
        uint8_t* pout = fd.pred ? fd.pred + ((size_t)b * fd.ncand + c) * (W * H) : nullptr;
        const int k = P.kind;
        const int kd = (k == IM_DC_TOP || k == IM_DC_LEFT || k == IM_DC_128) ? IM_DC : k;
        uint32_t acc = 0;
        bip_by_kind(kd, [&](auto KC) {
            constexpr int KU = decltype(KC)::value;
#pragma unroll
            for (int i = 0; i < NI; i++) {
                const int q = lane + i * LPB;
                if (items % LPB != 0 && q >= items) break;
                const int r = q / CPR, c0 = (q % CPR) * PPL;
                int px[PPL];
                bip_pixels<KU, uint8_t, W, H>(P, A, L, PA, PL, 8, r, c0, px);
                acc += fast_item_dist<NW>(fd.metric, sw[i], px);
                if (pout && live) bip_store_row<uint8_t, PPL>(pout + r * W + c0, px);
            }
        });
#pragma unroll
        for (int m = LPB >> 1; m >= 1; m >>= 1) acc += __shfl_xor(acc, m, 64);
        if (live && lane == 0) fd.dist[(size_t)b * fd.ncand + c] = acc;
    }
}

}  // namespace svtdev

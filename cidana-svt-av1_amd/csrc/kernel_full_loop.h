// kernel_full_loop.h — full_loop_kernel: the luma mode-decision full loop (ProductFullLoop / ProductFullLoopTxSearch,
// EbFullLoop.c:724-1100) for many (transform size, type list) groups in one launch per REGISTER CLASS.
//
// Per block and per type of its group:  residual = src - pred (ResidualKernel)  ->  av1_estimate_transform (DEFAULT_SHAPE, the
// 64-point re-pack and three_quad_energy)  ->  aom_highbd_quantize_b{,_32x32,_64x64} (flat qmatrix)  ->  picture_full_distortion32_bits
// (EbPictureOperators.c:349-400)  ->  dist[i] += three_quad_energy, RIGHT_SIGNED_SHIFT by (1 - tx_scale) * 2 (EbFullLoop.c:829-835).
// Outputs per (block, type): the two distortions, the eob (== count_non_zero_coeffs) and, on request, qcoeff / dqcoeff.
//
// A workgroup finds its group in a table in the kernel arguments (as enc_frame_kernel, kernel_frame.h: no device-side descriptor
// memory, graph-capturable).  Its waves stage src and pred ONCE in LDS (stage_planes with the source and the prediction addressed
// independently, or stage_dense when both are dense; kernel_txfm_staged.h) and keep that image for the whole type loop; each type
// then runs the staged kernels' forward steps (fwd_col_pass, fwd1d, fwd_col_store -> transpose tile -> fwd1d, fwd_row_scale), and the row pass's
// outputs are quantised IN REGISTERS, lane = coefficient row: no out tile, no HBM store.  The distortion
// sums and the eob are accumulated there and reduced over the block's lanes with shuffles.
//   C flavour     resid = sum (c - dq)^2, pred = sum c^2, both exact 64-bit (full_distortion_kernel32_bits)
//   AVX2 flavour  resid as the AVX2 kernel accumulates it (full_distortion32_kernel<true>, kernel_pixel.h): per column class x & 3 the
//                 square of the low 32 bits of the difference, its low and high words summed with wrapping 32-bit adds.  The low
//                 words need a sum per class; the high words land in bits 63:32 where the wrap is the 64-bit wrap, so one sum does.
//   eob == 0      both = sum c^2 (the cbf_zero kernel)
// Register classes (launch bounds as the frame kernel's): 0 both sides <= 16, 1 a 32- or 64-sample side except 64x64, 2 64x64.
#pragma once
#include "group_table.h"
#include "kernel_txfm_staged.h"

namespace svtdev {

constexpr int FL_MAX_GROUPS = 16;          // per launch: what fits the kernel arguments
constexpr int FL_MAX_TYPES = 16;
struct FullLoopGroupDev {
    const uint8_t* src; const uint8_t* pred;
    const uint32_t* src_xy; const uint32_t* pred_xy;       // NULL: dense W * H per block
    const int16_t* iscan;                                  // ntypes x NC
    unsigned long long* dist;                              // [nblocks][ntypes][2]
    uint16_t* eob;                                         // [nblocks][ntypes]
    int32_t* qcoeff; int32_t* dqcoeff;                     // optional, [nblocks][ntypes][NC]
    uint32_t src_stride, pred_stride, nblocks, wg_end;
    int32_t tx_size, ntypes;
    uint8_t types[FL_MAX_TYPES];
    QParams qp;
};
struct FullLoopDesc {
    int32_t ngroups;
    int32_t avx2;                                          // distortion flavour
    FullLoopGroupDev g[FL_MAX_GROUPS];
};
static_assert(sizeof(FullLoopDesc) <= 4000, "kernel arguments");

template <int W, int H>
struct FullLoopLds {
    using I = StagedIn<W, H, 1>;                                          // 8-bit samples
    static constexpr int WAVE = (2 * I::ONE + TxGeom<W, H>::BPW * TxGeom<W, H>::TILE * 4 + 15) & ~15;      // staging image kept + transpose tile
    static constexpr int BYTES = StagedGeom<W, H>::WAVES * WAVE;
};
template <int CLS> struct FullLoopClass;
#define SVT_FL_LDS(N, W, H) FullLoopLds<W, H>::BYTES,
template <> struct FullLoopClass<0> {
    static constexpr int THREADS = 256;
    static constexpr int LDS = cmax_of({SVT_TX_CLASS0(SVT_FL_LDS, SVT_FL_LDS)});
};
template <> struct FullLoopClass<1> {
    static constexpr int THREADS = 256;
    static constexpr int LDS = cmax_of({SVT_TX_CLASS1(SVT_FL_LDS, SVT_FL_LDS)});
};
#undef SVT_FL_LDS
template <> struct FullLoopClass<2> {
    static constexpr int THREADS = 128;                   // 64x64: two waves of one block each
    static constexpr int LDS = FullLoopLds<64, 64>::BYTES;
};
// One candidate of a wave whose staging image (source, prediction) is in place: the forward transform of the type, then the row
// pass's outputs quantised in registers.  Shared by full_loop_body and cfl_search_body (kernel_cfl_search.h).  bs = the block's
// staging image, tile = its transpose tile, is = the type's iscan; store(s, q, d) receives the four quantised / dequantised
// coefficients 4 s .. 4 s + 3 of row l (l < KH).  Out, valid in every lane of the block: e the eob, sc = sum c^2, sr the residual sum
// of the flavour, en three_quad_energy.  Reads the staging image, writes and reads the tile: the caller owes a fence before either
// is overwritten.
template <int W, int H, typename Store>
__device__ __forceinline__ void full_loop_candidate(const char* bs, int32_t* tile, int l, int tx_type, const int16_t* is, const QParams& qp,
                                                    int avx2, Store&& store, int& e, unsigned long long& sc, unsigned long long& sr,
                                                    unsigned long long& en) {
    using S = StagedGeom<W, H>;
    using G = TxGeom<W, H>;
    constexpr int KW = S::KW, KH = S::KH;
    const int vk = kVKind[tx_type], hk = kHKind[tx_type];
    {
        int x[H];
        fwd_col_pass<W, H, uint8_t, true>(bs, l, vk, x);
        if (l < W) fwd1d<H, fwd_cos_col(W, H)>(vk, x);
        fwd_col_store<W, H>(tile, l, hk, x);
    }
    wave_lds_fence();
    // ---- row pass, then quantise / distortion / eob in registers: lane l holds coefficient row l ----
    sc = 0; sr = 0;
    uint32_t lo0 = 0, lo1 = 0, lo2 = 0, lo3 = 0, hi = 0;
    e = 0;
    int y[W];
    if (l < H) {
#pragma unroll
        for (int c = 0; c < W; c++) y[c] = tile[l * G::PITCH + c];
        fwd1d<W, fwd_cos_row(W, H)>(hk, y);
    }
    en = fwd_row_scale<W, H>(l, y);
    if (l < KH) {
        const int16_t* isr = is + l * KW;
#pragma unroll
        for (int s = 0; s < KW / 4; s++) {
            int q[4], d[4];
#pragma unroll
            for (int j = 0; j < 4; j++) {
                const int c = y[4 * s + j];
                quant_one<2>(c, (l == 0 && s == 0 && j == 0) ? 0 : 1, qp, q[j], d[j]);      // host-checked power-of-two quant_shift
                const long long cc = c, df = (long long)c - d[j];
                sc += (unsigned long long)(cc * cc);
                if (avx2) {
                    const long long dl = (int)(uint32_t)df;
                    const unsigned long long sq = (unsigned long long)(dl * dl);
                    hi += (uint32_t)(sq >> 32);
                    if (j == 0) lo0 += (uint32_t)sq; else if (j == 1) lo1 += (uint32_t)sq; else if (j == 2) lo2 += (uint32_t)sq; else lo3 += (uint32_t)sq;
                } else {
                    sr += (unsigned long long)(df * df);
                }
            }
            const uint2 iv = *reinterpret_cast<const uint2*>(isr + 4 * s);
            e = max(e, max(max(q[0] ? (int)(iv.x & 0xffffu) + 1 : 0, q[1] ? (int)(iv.x >> 16) + 1 : 0),
                           max(q[2] ? (int)(iv.y & 0xffffu) + 1 : 0, q[3] ? (int)(iv.y >> 16) + 1 : 0)));
            store(s, q, d);
        }
    }
    // ---- reduce over the block's lanes ----
    e = group_max<G::LPB>(e);
    sc = group_sum64<G::LPB>(sc);
    if (W > 32 || H > 32) en = group_sum64<G::LPB>(en);
    if (avx2) {
        lo0 = group_sum<G::LPB>(lo0); lo1 = group_sum<G::LPB>(lo1); lo2 = group_sum<G::LPB>(lo2); lo3 = group_sum<G::LPB>(lo3);
        hi = group_sum<G::LPB>(hi);
        sr = ((unsigned long long)hi << 32) + lo0 + lo1 + lo2 + lo3;
    } else {
        sr = group_sum64<G::LPB>(sr);
    }
}

template <int W, int H>
__device__ __forceinline__ void full_loop_body(const FullLoopGroupDev& F, int avx2, uint32_t bid, char* lds) {
    using S = StagedGeom<W, H>;
    using G = TxGeom<W, H>;
    using I = StagedIn<W, H, 1>;
    constexpr int KW = S::KW, NC = S::NC;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (wave >= S::WAVES) return;                         // (inside a larger workgroup of the class: the spare waves have nothing to do)
    char* wl = lds + wave * FullLoopLds<W, H>::WAVE;
    const uint32_t nblocks = F.nblocks;
    const uint32_t first = (bid * S::WAVES + wave) * G::BPW;
    if (first >= nblocks) return;                         // wave-uniform
    const int sub = lane / G::LPB, l = lane % G::LPB;
    const uint32_t blk = first + sub;
    const bool valid = blk < nblocks;
    // RIGHT_SIGNED_SHIFT(dist, (1 - av1_get_tx_scale(tx_size)) * 2): tx_scale 0 / 1 / 2 above 256 / 1024 pixels
    constexpr int DSH = W * H > 1024 ? -2 : (W * H > 256 ? 0 : 2);

    // ---- stage the wave's source and prediction once ----
    uint32_t org[I::NIT];
    uint4 pv[I::NIT > I::NCHI ? I::NIT : I::NCHI];
    if (F.src_xy || F.pred_xy) stage_planes<W, H, 1>(wl, lane, first, nblocks, F.src, F.src_xy, F.src_stride, F.pred, F.pred_xy, F.pred_stride, org, pv);
    else stage_dense<W, H, 1, 2>(wl, lane, first, nblocks, F.src, F.pred, pv);
    wave_lds_fence();
    int32_t* tile = reinterpret_cast<int32_t*>(wl + 2 * I::ONE) + sub * G::TILE;

#pragma unroll 1
    for (int t = 0; t < F.ntypes; t++) {
        const size_t o = ((size_t)blk * F.ntypes + t) * NC + (size_t)l * KW;
        unsigned long long sc, sr, en;
        int e;
        full_loop_candidate<W, H>(wl + sub * (I::BB + I::PADI), tile, l, F.types[t], F.iscan + t * NC, F.qp, avx2,
            [&](int s, const int (&q)[4], const int (&d)[4]) {
                if (valid && F.qcoeff) *reinterpret_cast<int4*>(F.qcoeff + o + 4 * s) = make_int4(q[0], q[1], q[2], q[3]);
                if (valid && F.dqcoeff) *reinterpret_cast<int4*>(F.dqcoeff + o + 4 * s) = make_int4(d[0], d[1], d[2], d[3]);
            }, e, sc, sr, en);
        if (valid && l == 0) {
            unsigned long long d0 = (e == 0 ? sc : sr) + en, d1 = sc + en;
            if (DSH > 0) { d0 >>= DSH; d1 >>= DSH; }
            if (DSH < 0) { d0 <<= -DSH; d1 <<= -DSH; }
            const size_t o = (size_t)blk * F.ntypes + t;
            *reinterpret_cast<ulonglong2*>(F.dist + 2 * o) = make_ulonglong2(d0, d1);
            F.eob[o] = (uint16_t)e;
        }
        wave_lds_fence();                                 // the next type's column pass rewrites the tile
    }
}

template <int CLS>
__global__ __launch_bounds__(FullLoopClass<CLS>::THREADS) void full_loop_kernel(const FullLoopDesc fd) {
    __shared__ __attribute__((aligned(16))) char lds[FullLoopClass<CLS>::LDS];
    uint32_t bid;
    const int gi = group_of(fd, bid);
    if (gi >= fd.ngroups) return;
    const FullLoopGroupDev& F = fd.g[gi];
#define SVT_FL_CASE(N, W, H) case N: full_loop_body<W, H>(F, fd.avx2, bid, lds); break;
#define SVT_FL_DEFAULT(N, W, H) default: full_loop_body<W, H>(F, fd.avx2, bid, lds); break;      // the last size of a class
    if constexpr (CLS == 0) {
        switch (F.tx_size) { SVT_TX_CLASS0(SVT_FL_CASE, SVT_FL_DEFAULT) }
    } else if constexpr (CLS == 1) {
        switch (F.tx_size) { SVT_TX_CLASS1(SVT_FL_CASE, SVT_FL_DEFAULT) }
    } else {
        full_loop_body<64, 64>(F, fd.avx2, bid, lds);
    }
#undef SVT_FL_CASE
#undef SVT_FL_DEFAULT
}

}  // namespace svtdev

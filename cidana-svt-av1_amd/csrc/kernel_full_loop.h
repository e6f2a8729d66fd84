// kernel_full_loop.h — full_loop_kernel: the luma mode-decision full loop (ProductFullLoop / ProductFullLoopTxSearch,
// EbFullLoop.c:724-1100) for many (transform size, type list) groups in one launch per REGISTER CLASS.
//
// Per block and per type of its group:  residual = src - pred (ResidualKernel)  ->  av1_estimate_transform (DEFAULT_SHAPE, the
// 64-point re-pack and three_quad_energy)  ->  aom_highbd_quantize_b{,_32x32,_64x64} (flat qmatrix)  ->  picture_full_distortion32_bits
// (EbPictureOperators.c:349-400)  ->  dist[i] += three_quad_energy, RIGHT_SIGNED_SHIFT by (1 - tx_scale) * 2 (EbFullLoop.c:829-835).
// Outputs per (block, type): the two distortions, the eob (== count_non_zero_coeffs) and, on request, qcoeff / dqcoeff.
//
// A workgroup finds its group in a table in the kernel arguments (as enc_frame_kernel, kernel_frame.h: no device-side descriptor
// memory, graph-capturable).  Its waves stage src and pred ONCE in LDS (the staging of fwd_staged_kernel MODE 1, kernel_txfm_staged.h,
// with the source and the prediction addressed independently: planes or dense) and keep that image for the whole type loop; each type
// then runs the staged forward networks of that kernel (column pass -> transpose tile -> row pass, the same fwd1d / shift / rect2
// steps), and the row pass's outputs are quantised IN REGISTERS, lane = coefficient row: no out tile, no HBM store.  The distortion
// sums and the eob are accumulated there and reduced over the block's lanes with shuffles.
//   C flavour     resid = sum (c - dq)^2, pred = sum c^2, both exact 64-bit (full_distortion_kernel32_bits)
//   AVX2 flavour  resid as the AVX2 kernel accumulates it (full_distortion32_kernel<true>, kernel_pixel.h): per column class x & 3 the
//                 square of the low 32 bits of the difference, its low and high words summed with wrapping 32-bit adds.  The low
//                 words need a sum per class; the high words land in bits 63:32 where the wrap is the 64-bit wrap, so one sum does.
//   eob == 0      both = sum c^2 (the cbf_zero kernel)
// Register classes (launch bounds as the frame kernel's): 0 both sides <= 16, 1 a 32- or 64-sample side except 64x64, 2 64x64.
#pragma once
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
    using G = TxGeom<W, H>;
    static constexpr int BB = W * H;                                      // 8-bit samples
    static constexpr int PADI = W >= 32 ? 32 : 16;                        // staging pad per block (fwd_staged_kernel's)
    static constexpr int IN_ONE = G::BPW * (BB + PADI);
    static constexpr int WAVE = (2 * IN_ONE + G::BPW * G::TILE * 4 + 15) & ~15;      // staging image kept + transpose tile
    static constexpr int BYTES = StagedGeom<W, H>::WAVES * WAVE;
};
template <int CLS> struct FullLoopClass;
template <> struct FullLoopClass<0> {
    static constexpr int THREADS = 256;
    static constexpr int LDS = cmax(cmax(cmax(FullLoopLds<16, 16>::BYTES, FullLoopLds<8, 8>::BYTES), cmax(FullLoopLds<4, 4>::BYTES, FullLoopLds<8, 16>::BYTES)),
                                    cmax(cmax(FullLoopLds<16, 8>::BYTES, FullLoopLds<4, 8>::BYTES), cmax(cmax(FullLoopLds<8, 4>::BYTES, FullLoopLds<4, 16>::BYTES),
                                                                                                         FullLoopLds<16, 4>::BYTES)));
};
template <> struct FullLoopClass<1> {
    static constexpr int THREADS = 256;
    static constexpr int LDS = cmax(cmax(cmax(FullLoopLds<32, 32>::BYTES, FullLoopLds<16, 32>::BYTES), cmax(FullLoopLds<32, 16>::BYTES, FullLoopLds<8, 32>::BYTES)),
                                    cmax(cmax(FullLoopLds<32, 8>::BYTES, FullLoopLds<32, 64>::BYTES), cmax(cmax(FullLoopLds<64, 32>::BYTES, FullLoopLds<16, 64>::BYTES),
                                                                                                           FullLoopLds<64, 16>::BYTES)));
};
template <> struct FullLoopClass<2> {
    static constexpr int THREADS = 128;                   // 64x64: two waves of one block each
    static constexpr int LDS = FullLoopLds<64, 64>::BYTES;
};
// (the register classes of enc_frame_kernel: sizes with both sides <= 16 are TX_4X4 0, 8X8 1, 16X16 2, 4X8 5, 8X4 6, 8X16 7, 16X8 8, 4X16 13, 16X4 14)
constexpr int full_loop_class_of(int tx_size) {
    constexpr unsigned small = (1u << 0) | (1u << 1) | (1u << 2) | (1u << 5) | (1u << 6) | (1u << 7) | (1u << 8) | (1u << 13) | (1u << 14);
    return tx_size == 4 ? 2 : (((small >> tx_size) & 1u) ? 0 : 1);
}
inline uint32_t full_loop_blocks_per_wg(int w, int h) {   // host only: StagedGeom<W, H>::WAVES * TxGeom<W, H>::BPW
    const int m = w > h ? w : h;
    return (uint32_t)((w * h >= 4096 ? 2 : 4) * (64 / m));
}

template <int W, int H>
__device__ __forceinline__ void full_loop_body(const FullLoopGroupDev& F, int avx2, uint32_t bid, char* lds) {
    using S = StagedGeom<W, H>;
    using G = TxGeom<W, H>;
    using L = FullLoopLds<W, H>;
    constexpr int KW = S::KW, KH = S::KH, NC = S::NC;
    constexpr int BB = L::BB, PADI = L::PADI, IN_ONE = L::IN_ONE;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (wave >= S::WAVES) return;                         // (inside a larger workgroup of the class: the spare waves have nothing to do)
    char* wl = lds + wave * L::WAVE;
    const uint32_t nblocks = F.nblocks;
    const uint32_t first = (bid * S::WAVES + wave) * G::BPW;
    if (first >= nblocks) return;                         // wave-uniform
    const int sub = lane / G::LPB, l = lane % G::LPB;
    const uint32_t blk = first + sub;
    const bool valid = blk < nblocks;
    constexpr int CBC = fwd_cos_col(W, H), CBR = fwd_cos_row(W, H);
    constexpr int S0 = fwd_shift(W, H, 0), S1 = fwd_shift(W, H, 1), S2 = fwd_shift(W, H, 2);
    // RIGHT_SIGNED_SHIFT(dist, (1 - av1_get_tx_scale(tx_size)) * 2): tx_scale 0 / 1 / 2 above 256 / 1024 pixels
    constexpr int DSH = W * H > 1024 ? -2 : (W * H > 256 ? 0 : 2);

    // ---- stage the wave's source and prediction once: chunks of CS bytes that never cross a block row ----
    {
        constexpr int CS = W >= 16 ? 16 : W, CPR = W / CS, CPBP = BB / CS, NCHP = G::BPW * CPBP, NIT = (NCHP + 63) / 64;
        uint4 v0[NIT], v1[NIT];
#pragma unroll
        for (int it = 0; it < NIT; it++) {
            const int q = it * 64 + lane, b = q / CPBP, w = q % CPBP;
            const int row = w / CPR, cb = (w % CPR) * CS;
            v0[it] = make_uint4(0, 0, 0, 0); v1[it] = v0[it];
            if ((NCHP % 64 == 0 || q < NCHP) && first + b < nblocks) {
                const uint8_t* ps;
                const uint8_t* pp;
                if (F.src_xy) { const uint32_t o = F.src_xy[first + b]; ps = F.src + ((size_t)(o >> 16) + row) * F.src_stride + (o & 0xffffu) + cb; }
                else ps = F.src + (size_t)(first + b) * BB + row * W + cb;
                if (F.pred_xy) { const uint32_t o = F.pred_xy[first + b]; pp = F.pred + ((size_t)(o >> 16) + row) * F.pred_stride + (o & 0xffffu) + cb; }
                else pp = F.pred + (size_t)(first + b) * BB + row * W + cb;
                __builtin_memcpy(&v0[it], ps, CS);
                __builtin_memcpy(&v1[it], pp, CS);
            }
        }
#pragma unroll
        for (int it = 0; it < NIT; it++) {
            const int q = it * 64 + lane, b = q / CPBP;
            if (NCHP % 64 == 0 || q < NCHP) {
                __builtin_memcpy(wl + q * CS + b * PADI, &v0[it], CS);
                __builtin_memcpy(wl + IN_ONE + q * CS + b * PADI, &v1[it], CS);
            }
        }
    }
    wave_lds_fence();
    int32_t* tile = reinterpret_cast<int32_t*>(wl + 2 * IN_ONE) + sub * G::TILE;
    const char* bs = wl + sub * (BB + PADI);

#pragma unroll 1
    for (int t = 0; t < F.ntypes; t++) {
        const int tx_type = F.types[t];
        const int vk = kVKind[tx_type], hk = kHKind[tx_type];
        const bool ud = vk == K1D_FLIPADST, lr = hk == K1D_FLIPADST;
        // ---- column pass (fwd_staged_kernel's) ----
        {
            int x[H];
            if (l < W) {
#pragma unroll
                for (int r = 0; r < H; r++) {
                    const int idx = (ud ? H - 1 - r : r) * W + l;
                    x[r] = round_shift_c<-S0>((int)*reinterpret_cast<const uint8_t*>(bs + idx) - (int)*reinterpret_cast<const uint8_t*>(bs + IN_ONE + idx));
                }
                fwd1d<H, CBC>(vk, x);
                const int cdst = lr ? W - 1 - l : l;
#pragma unroll
                for (int r = 0; r < H; r++) tile[r * G::PITCH + cdst] = round_shift_c<-S1>(x[r]);
            }
        }
        wave_lds_fence();
        // ---- row pass, then quantise / distortion / eob in registers: lane l holds coefficient row l ----
        unsigned long long en = 0, sc = 0, sr = 0;
        uint32_t lo0 = 0, lo1 = 0, lo2 = 0, lo3 = 0, hi = 0;
        int e = 0;
        if (l < H) {
            int y[W];
#pragma unroll
            for (int c = 0; c < W; c++) y[c] = tile[l * G::PITCH + c];
            fwd1d<W, CBR>(hk, y);
#pragma unroll
            for (int c = 0; c < W; c++) {
                int v = round_shift_c<-S2>(y[c]);
                if (G::RECT2) v = mul_q12(v, 5793);
                y[c] = v;
            }
            if (W > 32 || H > 32) {                       // three_quad_energy: the coefficients the 64-point re-pack drops
#pragma unroll
                for (int c = 0; c < W; c++)
                    if (l >= KH || c >= KW) { const long long v = y[c]; en += (unsigned long long)(v * v); }
            }
            if (l < KH) {
                const int16_t* is = F.iscan + t * NC + l * KW;
                const size_t o = ((size_t)blk * F.ntypes + t) * NC + (size_t)l * KW;
#pragma unroll
                for (int s = 0; s < KW / 4; s++) {
                    int q[4], d[4];
#pragma unroll
                    for (int j = 0; j < 4; j++) {
                        const int c = y[4 * s + j];
                        quant_one<2>(c, (l == 0 && s == 0 && j == 0) ? 0 : 1, F.qp, q[j], d[j]);      // host-checked power-of-two quant_shift
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
                    const uint2 iv = *reinterpret_cast<const uint2*>(is + 4 * s);
                    e = max(e, max(max(q[0] ? (int)(iv.x & 0xffffu) + 1 : 0, q[1] ? (int)(iv.x >> 16) + 1 : 0),
                                   max(q[2] ? (int)(iv.y & 0xffffu) + 1 : 0, q[3] ? (int)(iv.y >> 16) + 1 : 0)));
                    if (valid && F.qcoeff) *reinterpret_cast<int4*>(F.qcoeff + o + 4 * s) = make_int4(q[0], q[1], q[2], q[3]);
                    if (valid && F.dqcoeff) *reinterpret_cast<int4*>(F.dqcoeff + o + 4 * s) = make_int4(d[0], d[1], d[2], d[3]);
                }
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
    int gi = 0;
    uint32_t start = 0;
#pragma unroll 1
    for (int i = 0; i < fd.ngroups; i++) {
        if (blockIdx.x >= fd.g[i].wg_end) { gi = i + 1; start = fd.g[i].wg_end; }
    }
    if (gi >= fd.ngroups) return;
    const FullLoopGroupDev& F = fd.g[gi];
    const uint32_t bid = blockIdx.x - start;
#define SVT_FL_CASE(N, W, H) case N: full_loop_body<W, H>(F, fd.avx2, bid, lds); break;
    if constexpr (CLS == 0) {
        switch (F.tx_size) {
        SVT_FL_CASE(0, 4, 4) SVT_FL_CASE(1, 8, 8) SVT_FL_CASE(2, 16, 16) SVT_FL_CASE(5, 4, 8) SVT_FL_CASE(6, 8, 4)
        SVT_FL_CASE(7, 8, 16) SVT_FL_CASE(8, 16, 8) SVT_FL_CASE(13, 4, 16)
        default: full_loop_body<16, 4>(F, fd.avx2, bid, lds); break;       // 14
        }
    } else if constexpr (CLS == 1) {
        switch (F.tx_size) {
        SVT_FL_CASE(3, 32, 32) SVT_FL_CASE(9, 16, 32) SVT_FL_CASE(10, 32, 16) SVT_FL_CASE(11, 32, 64) SVT_FL_CASE(12, 64, 32)
        SVT_FL_CASE(15, 8, 32) SVT_FL_CASE(16, 32, 8) SVT_FL_CASE(17, 16, 64)
        default: full_loop_body<64, 16>(F, fd.avx2, bid, lds); break;      // 18
        }
    } else {
        full_loop_body<64, 64>(F, fd.avx2, bid, lds);
    }
#undef SVT_FL_CASE
}

}  // namespace svtdev

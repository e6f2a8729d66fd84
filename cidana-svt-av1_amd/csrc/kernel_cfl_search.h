// kernel_cfl_search.h — the CfL alpha search of mode decision (CflPrediction / cfl_rd_pick_alpha / AV1CostCalcCfl,
// EbProductCodingLoop.c:1395-1860), for many chroma-size groups in one launch.
//
// cfl_search_kernel   the table: per chroma block, per plane and per alpha candidate a (SVT_HIP_CFL_NALPHA = 33: a = 0 alpha_q3 0,
//                     a = 1 .. 16 alpha_q3 -a, a = 17 .. 32 alpha_q3 a - 16)
//                       pred = cfl_predict_lbd(ac, dc_pred, alpha_q3)  ->  residual = src - pred  ->  av1_estimate_transform  ->  the
//                       production quantiser with the PLANE's rows  ->  eob, picture_full_distortion32_bits >> 2
//                     and the candidate's qcoeff and context bytes into the scratch, where coeff_rate_kernel (kernel_coeff_rate.h) reads
//                     (block, plane, a) as a block with one type.
//   A wave takes TxGeom::BPW blocks of ONE plane (wave-unit u: blocks (u >> 1) * BPW .., plane u & 1), so the source and the DC
//   prediction are staged once per wave (stage_planes, kernel_txfm_staged.h) and a block's 66 candidates run on two waves.  The lane
//   that staged chunk q of the prediction keeps that chunk's DC samples and its Q3 AC values (cfl_luma_subsampling_420_lbd of the
//   luma reconstruction, subtract_average; computed as cfl_frame_kernel does, kernel_cfl.h) in registers, and per candidate rewrites
//   only the prediction half of the staging image.  The candidate itself is full_loop_candidate (kernel_full_loop.h), the body
//   full_loop_body runs per transform type.  No prediction and no dqcoeff is ever stored to memory.
// cfl_decide_kernel   cfl_rd_pick_alpha's walk over that table (:1587-1735), one lane per block.  plane / pn_sign / i are unrolled,
//                     so the joint sign indexes best_rd_uv / best_c at compile time and both stay in registers.
#pragma once
#include "dev_common.h"
#include "kernel_full_loop.h"

namespace svtdev {

constexpr int CFS_NALPHA = 33;
constexpr int CFS_MAX_GROUPS = 16;         // per launch: what fits the kernel arguments
struct CflSearchGroupDev {
    const uint8_t* luma;
    const uint8_t* src[2]; const uint8_t* pred[2];
    const uint32_t* xy;
    const int16_t* iscan;
    const uint8_t* skip_ctx[2]; const uint8_t* dc_ctx[2];  // [nblocks] per plane
    unsigned long long* dist;                              // [nblocks][2][33][2]
    uint16_t* eob;                                         // [nblocks][2][33]
    int32_t* qcoeff;                                       // scratch [nblocks][2][33][NC]
    uint8_t* skip_out; uint8_t* dc_out;                    // scratch [nblocks][2][33]: the contexts per candidate
    uint32_t luma_stride, src_stride[2], pred_stride[2], nblocks, wg_end;
    int32_t tx_size, tx_type;
};
struct CflSearchDesc {
    int32_t ngroups;
    int32_t avx2;                                          // distortion flavour
    QParams qp[2];                                         // Cb, Cr rows (log_scale 0: no CfL size is above 256 pixels)
    CflSearchGroupDev g[CFS_MAX_GROUPS];
};
static_assert(sizeof(CflSearchDesc) <= 4000, "kernel arguments");

// the members quant_one<2> reads, from the second set when `second`
__device__ __forceinline__ QParams cfs_pick(bool second, const QParams& a, const QParams& b) {
    QParams q = a;
#pragma unroll
    for (int i = 0; i < 2; i++) {
        q.round2[i] = second ? b.round2[i] : a.round2[i];
        q.zbin2[i] = second ? b.zbin2[i] : a.zbin2[i];
        q.quant_hi[i] = second ? b.quant_hi[i] : a.quant_hi[i];
        q.dequant[i] = second ? b.dequant[i] : a.dequant[i];
    }
    q.log_scale = second ? b.log_scale : a.log_scale;
    return q;
}

template <int W, int H>
__device__ __forceinline__ void cfl_search_body(const CflSearchGroupDev& F, const QParams& qp_cb, const QParams& qp_cr, int avx2, uint32_t bid,
                                                char* lds) {
    using S = StagedGeom<W, H>;
    using G = TxGeom<W, H>;
    using I = StagedIn<W, H, 1>;
    constexpr int KW = S::KW, NC = S::NC, PPC = I::PPC, CPBP = I::CPBP, CPR = I::CPR;
    static_assert(I::NIT == 1 && W * H <= 256 && CPBP <= 64, "one chunk per lane; chromaShift == the full loop's shift");
    constexpr int PEL_LOG2 = W * H == 256 ? 8 : (W * H == 128 ? 7 : (W * H == 64 ? 6 : (W * H == 32 ? 5 : 4)));
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));      // scalar: so is the plane
    if (wave >= S::WAVES) return;
    char* wl = lds + wave * FullLoopLds<W, H>::WAVE;
    const uint32_t nblocks = F.nblocks;
    const uint32_t unit = bid * S::WAVES + wave;
    const bool plane = (unit & 1u) != 0;
    const uint32_t first = (unit >> 1) * G::BPW;
    if (first >= nblocks) return;                         // wave-uniform
    const int sub = lane / G::LPB, l = lane % G::LPB;
    const uint32_t blk = first + sub;
    const bool valid = blk < nblocks;
    // the plane's members picked one by one: indexing the descriptor (kernel arguments) with the plane makes the compiler copy it to scratch
    const QParams qp = cfs_pick(plane, qp_cb, qp_cr);
    const uint8_t* srcp = plane ? F.src[1] : F.src[0];
    const uint8_t* predp = plane ? F.pred[1] : F.pred[0];
    const uint32_t src_stride = plane ? F.src_stride[1] : F.src_stride[0], pred_stride = plane ? F.pred_stride[1] : F.pred_stride[0];
    const uint8_t* skip_ctx = plane ? F.skip_ctx[1] : F.skip_ctx[0];
    const uint8_t* dc_ctx = plane ? F.dc_ctx[1] : F.dc_ctx[0];

    // ---- stage the plane's source and DC prediction once; the lane keeps its prediction chunk ----
    uint32_t org[1];
    uint4 pv[1];
    stage_planes<W, H, 1>(wl, lane, first, nblocks, srcp, F.xy, src_stride, predp, F.xy, pred_stride, org, pv);

    // ---- the chunk's Q3 AC values: 2x2 luma sums * 2, minus the block average (round_offset W * H / 2) ----
    int ac[PPC];
    {
        const int w = lane % CPBP;
        int sum = 0;
#pragma unroll
        for (int i = 0; i < PPC; i++) ac[i] = 0;
        if (org[0] != 0xffffffffu) {
            const uint32_t row = w / CPR, col = (w % CPR) * PPC;
            const uint8_t* s = F.luma + (size_t)(2 * ((org[0] >> 16) + row)) * F.luma_stride + 2 * ((org[0] & 0xffffu) + col);
            uint8_t r0[2 * PPC], r1[2 * PPC];
            cfl_ld<2 * PPC>(r0, s); cfl_ld<2 * PPC>(r1, s + F.luma_stride);
#pragma unroll
            for (int i = 0; i < PPC; i++) {
                ac[i] = ((int)r0[2 * i] + r0[2 * i + 1] + r1[2 * i] + r1[2 * i + 1]) << 1;
                sum += ac[i];
            }
        }
#pragma unroll
        for (int m = CPBP / 2; m >= 1; m >>= 1) sum += __shfl_xor(sum, m, 64);      // a block's chunks: CPBP consecutive lanes
        const int avg = (sum + W * H / 2) >> PEL_LOG2;
#pragma unroll
        for (int i = 0; i < PPC; i++) ac[i] = (int)(int16_t)(ac[i] - avg);
    }
    const uint32_t pw[4] = {pv[0].x, pv[0].y, pv[0].z, pv[0].w};
    const bool stager = lane < I::NCHP;
    char* pdst = wl + I::ONE + lane * I::CS + (lane / CPBP) * I::PADI;
    const char* bs = wl + sub * (I::BB + I::PADI);
    int32_t* tile = reinterpret_cast<int32_t*>(wl + 2 * I::ONE) + sub * G::TILE;
    const size_t cand0 = ((size_t)blk * 2 + (plane ? 1 : 0)) * CFS_NALPHA;
    const uint8_t skc = valid ? skip_ctx[blk] : (uint8_t)0, dcc = valid ? dc_ctx[blk] : (uint8_t)0;

#pragma unroll 1
    for (int a = 0; a < CFS_NALPHA; a++) {
        const int alpha = a <= 16 ? -a : a - 16;
        // ---- cfl_predict_lbd into the prediction half of the staging image ----
        if (stager) {
            uint32_t ow[4] = {0, 0, 0, 0};
#pragma unroll
            for (int i = 0; i < PPC; i++) {
                const int q6 = alpha * ac[i];
                const int mag = ((q6 < 0 ? -q6 : q6) + 32) >> 6;
                int v = (int)((pw[i >> 2] >> (8 * (i & 3))) & 0xffu) + (q6 < 0 ? -mag : mag);
                v = v < 0 ? 0 : (v > 255 ? 255 : v);
                ow[i >> 2] |= (uint32_t)v << (8 * (i & 3));
            }
            __builtin_memcpy(pdst, ow, I::CS);
        }
        wave_lds_fence();
        unsigned long long sc, sr, en;
        int e;
        full_loop_candidate<W, H>(bs, tile, l, F.tx_type, F.iscan, qp, avx2,
            [&](int s, const int (&q)[4], const int (&)[4]) {
                if (valid) *reinterpret_cast<int4*>(F.qcoeff + (cand0 + a) * NC + (size_t)l * KW + 4 * s) = make_int4(q[0], q[1], q[2], q[3]);
            }, e, sc, sr, en);
        if (valid && l == 0) {
            const size_t o = cand0 + a;
            *reinterpret_cast<ulonglong2*>(F.dist + 2 * o) = make_ulonglong2((e == 0 ? sc : sr) >> 2, sc >> 2);      // chromaShift
            F.eob[o] = (uint16_t)e;
            F.skip_out[o] = skc;
            F.dc_out[o] = dcc;
        }
        wave_lds_fence();                                 // the next candidate rewrites the prediction and the tile
    }
}

__global__ __launch_bounds__(FullLoopClass<0>::THREADS) void cfl_search_kernel(const CflSearchDesc fd) {
    __shared__ __attribute__((aligned(16))) char lds[FullLoopClass<0>::LDS];
    uint32_t bid;
    const int gi = group_of(fd, bid);
    if (gi >= fd.ngroups) return;
    const CflSearchGroupDev& F = fd.g[gi];
#define SVT_CFS_CASE(N, W, H) case N: cfl_search_body<W, H>(F, fd.qp[0], fd.qp[1], fd.avx2, bid, lds); break;
#define SVT_CFS_DEFAULT(N, W, H) default: cfl_search_body<W, H>(F, fd.qp[0], fd.qp[1], fd.avx2, bid, lds); break;
    switch (F.tx_size) { SVT_TX_CLASS0(SVT_CFS_CASE, SVT_CFS_DEFAULT) }      // the nine CfL chroma sizes are exactly class 0
#undef SVT_CFS_CASE
#undef SVT_CFS_DEFAULT
}

// ---- the walk ----------------------------------------------------------------------------------------------------------------
constexpr int CFD_MAX_GROUPS = 32;
constexpr int CFD_THREADS = 256;
struct CflDecideGroupDev {
    const unsigned long long* dist;                        // [nblocks][2][33][2]
    const unsigned long long* bits;                        // [nblocks][2][33]
    const int32_t* alpha_rate;                             // cflAlphaFacBits[8][2][16]
    const int32_t* cfl_mode_bits; const int32_t* dc_mode_bits;      // [nblocks]
    unsigned long long* decision;                          // [nblocks][4]: svt_hip_cfl_decision as words
    int32_t* alpha_cb; int32_t* alpha_cr;                  // optional [nblocks]
    uint32_t nblocks, wg_end, lambda;
};
struct CflDecideDesc {
    int32_t ngroups;
    CflDecideGroupDev g[CFD_MAX_GROUPS];
};
static_assert(sizeof(CflDecideDesc) <= 4000, "kernel arguments");

// RDCOST (EbRateDistortionCost.h:73) in uint64 arithmetic that wraps
__device__ __forceinline__ unsigned long long cfd_rdcost(unsigned long long lambda, unsigned long long r, unsigned long long d) {
    return ((r * lambda + 256ull) >> 9) + d * 128ull;
}
// PLANE_SIGN_TO_JOINT_SIGN (:1574)
__host__ __device__ constexpr int cfd_joint_sign(int plane, int a, int b) { return plane == 0 ? a * 3 + b - 1 : b * 3 + a - 1; }

__global__ __launch_bounds__(CFD_THREADS) void cfl_decide_kernel(const CflDecideDesc fd) {
    uint32_t bid;
    const int gi = group_of(fd, bid);
    if (gi >= fd.ngroups) return;
    const CflDecideGroupDev& F = fd.g[gi];
    const uint32_t blk = bid * CFD_THREADS + threadIdx.x;
    if (blk >= F.nblocks) return;
    const unsigned long long lambda = F.lambda;
    const unsigned long long* dist = F.dist + (size_t)blk * (2 * CFS_NALPHA * 2);
    const unsigned long long* bits = F.bits + (size_t)blk * (2 * CFS_NALPHA);
    constexpr long long I64_MAX = 0x7fffffffffffffffll;
    const long long mode_rd = (long long)cfd_rdcost(lambda, (unsigned long long)(long long)F.cfl_mode_bits[blk], 0);
    long long best_rd = I64_MAX;
    long long best_rd_uv[8][2];
    int best_c[8][2];
    // ---- alpha zero in each plane (:1598-1634) ----
#pragma unroll
    for (int plane = 0; plane < 2; plane++) {
#pragma unroll
        for (int js = 0; js < 8; js++) { best_rd_uv[js][plane] = I64_MAX; best_c[js][plane] = 0; }
        const unsigned long long b0 = bits[plane * CFS_NALPHA], d0 = dist[plane * CFS_NALPHA * 2];
#pragma unroll
        for (int i = 1; i < 3; i++) {
            const int js = cfd_joint_sign(plane, 0, i);
            best_rd_uv[js][plane] = (long long)cfd_rdcost(lambda, b0 + (unsigned long long)(long long)F.alpha_rate[(js * 2 + plane) * 16], d0);
        }
    }
    // ---- the walk (:1636-1686) ----
    int best_joint_sign = -1;
#pragma unroll
    for (int plane = 0; plane < 2; plane++) {
#pragma unroll
        for (int pn = 1; pn < 3; pn++) {
            int progress = 0;
#pragma unroll 1
            for (int c = 0; c < 16; c++) {
                int flag = 0;
                if (c > 2 && progress < c) break;
                // AV1CostCalcCfl with cfl_alpha_idx (c << 4) + c and the joint sign of i = 0: alpha_q3 -/+ (c + 1) in this plane, except
                // that its "To check DC" test (idx 0 and signs 0, :1511) also meets Cr, CFL_SIGN_NEG, c = 0, which it costs at alpha 0
                const int a = (plane == 1 && pn == 1 && c == 0) ? 0 : 1 + 16 * (pn - 1) + c;
                const unsigned long long cb = bits[plane * CFS_NALPHA + a], cd = dist[(plane * CFS_NALPHA + a) * 2];
#pragma unroll
                for (int i = 0; i < 3; i++) {
                    const int js = cfd_joint_sign(plane, pn, i);
                    long long this_rd = (long long)cfd_rdcost(lambda, cb + (unsigned long long)(long long)F.alpha_rate[(js * 2 + plane) * 16 + c], cd);
                    if (this_rd >= best_rd_uv[js][plane]) continue;
                    best_rd_uv[js][plane] = this_rd;
                    best_c[js][plane] = c;
                    flag = 2;
                    if (best_rd_uv[js][!plane] == I64_MAX) continue;
                    this_rd = (long long)((unsigned long long)this_rd + (unsigned long long)mode_rd + (unsigned long long)best_rd_uv[js][!plane]);
                    if (this_rd >= best_rd) continue;
                    best_rd = this_rd;
                    best_joint_sign = js;
                }
                progress += flag;
            }
        }
    }
    // ---- against DC (:1688-1735) ----
    const long long dc_mode_rd = (long long)cfd_rdcost(lambda, (unsigned long long)(long long)F.dc_mode_bits[blk], 0);
    const long long dc_rd = (long long)(cfd_rdcost(lambda, bits[0] + bits[CFS_NALPHA], dist[0] + dist[CFS_NALPHA * 2]) + (unsigned long long)dc_mode_rd);
    uint32_t uv_mode = 0, idx = 0, signs = 0;
    int a_cb = 0, a_cr = 0;
    if (!(dc_rd <= best_rd)) {
        uv_mode = 13;                                      // UV_CFL_PRED
        if (best_joint_sign >= 0) {
            int u = 0, v = 0;
#pragma unroll
            for (int js = 0; js < 8; js++)
                if (js == best_joint_sign) { u = best_c[js][0]; v = best_c[js][1]; }
            idx = (uint32_t)((u << 4) + v);
        } else {
            best_joint_sign = 0;
        }
        signs = (uint32_t)best_joint_sign;
        // cfl_idx_to_alpha (EbIntraPrediction.h:609-617)
        const int su = ((best_joint_sign + 1) * 11) >> 5, sv = (best_joint_sign + 1) - 3 * su;
        a_cb = su == 0 ? 0 : (su == 2 ? (int)(idx >> 4) + 1 : -(int)(idx >> 4) - 1);
        a_cr = sv == 0 ? 0 : (sv == 2 ? (int)(idx & 15u) + 1 : -(int)(idx & 15u) - 1);
    }
    unsigned long long* rec = F.decision + 4 * (size_t)blk;
    rec[0] = (unsigned long long)best_rd;
    rec[1] = (unsigned long long)dc_rd;
    rec[2] = (unsigned long long)(uint32_t)a_cb | ((unsigned long long)(uint32_t)a_cr << 32);
    rec[3] = (unsigned long long)(uv_mode | (idx << 8) | (signs << 16));
    if (F.alpha_cb) F.alpha_cb[blk] = a_cb;
    if (F.alpha_cr) F.alpha_cr[blk] = a_cr;
}

}  // namespace svtdev

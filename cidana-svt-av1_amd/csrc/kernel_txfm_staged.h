// kernel_txfm_staged.h — forward transforms / fused chain for DENSE block batches of
// every size: same math as kernel_txfm.h, but all HBM traffic is 16 B per lane and
// fully coalesced.  A wave's 64/max(W,H) blocks are contiguous in memory, so
//   in : linear 16-B chunks -> LDS staging (padded per block: conflict-free column reads)
//   out: rows -> XOR-swizzled LDS tile -> linear 16-B chunks (quantised in that order)
// MODE 0: int16 residual -> coeff (av1_fwd_txfm2d_WxH, full W*H output)
// MODE 1: u8 src + pred -> coeff, qcoeff, dqcoeff (packed min(W,32)*min(H,32)), eob, sad,
//         three_quad_energy  (the headline chain for sizes other than 32x32)
#pragma once
#include <initializer_list>
#include <type_traits>

#include "av1_geom.h"
#include "group_table.h"
#include "kernel_txfm.h"
#include "tx_plan.h"

namespace svtdev {

constexpr int cmax(int a, int b) { return a > b ? a : b; }
template <int PELS> struct StagedWaves { static constexpr int N = PELS >= 4096 ? 2 : 4; };

template <int W, int H>
struct StagedGeom {
    using G = TxGeom<W, H>;
    static constexpr int WAVES = StagedWaves<W * H>::N;
    static constexpr int KW = W > 32 ? 32 : W, KH = H > 32 ? 32 : H, NC = KW * KH;
    static constexpr int NQ = (G::BPW * NC / 4 + 63) / 64;          // 16-B coefficient chunks per lane of a wave (quant_out_tile)
    static constexpr int P16 = W + 2;                    // int16 transpose tile row pitch: (W+2)/2 is odd -> conflict-free row writes
    // out tile: row r, 16-B slot s -> slot s ^ ((r / RDIV) & SMASK)   (conflict-free b128 row writes)
    static constexpr int NS = W / 4;
    static constexpr int RDIV = (8 / NS) > 1 ? (8 / NS) : 1;
    static constexpr int SMASK = (NS < 8 ? NS : 8) - 1;
    __device__ static __forceinline__ int out_addr(int sub, int r, int s) {
        return sub * (W * H * 4) + r * (W * 4) + ((s ^ ((r / RDIV) & SMASK)) << 4);
    }
};

// LDS layouts shared by the inverse / encode kernels below, chosen against the PMC (profiles/r02_pmc_c_enc8.json: 26 % of the LDS
// cycles of the 8x8 encode kernel were bank conflicts, 14 % at 16x16):
//  * coefficient tile (linear 16-byte stores -> one-row-per-lane b128 reads): rows of KW * 4 bytes whose 16-byte slots are
//    XOR-swizzled by the row (the out tile's rule): stores AND reads are conflict-free.  The first version padded the row pitch
//    by one slot instead, which kept the reads clean and made every linear store a 2-way conflict;
//  * residual tile (column pass -> reconstruction): int16, W * H + ResPad<W> per block: with the dense pitch the column stores
//    of all the wave's blocks fell on the same W / 2 banks (8-way at 8x8, 4-way at 16x16).
template <int KW, int KH>
__device__ __forceinline__ int coef_tile_addr(int b, int r, int sl) {
    constexpr int NS = KW / 4, RDIV = (8 / NS) > 1 ? (8 / NS) : 1, SMASK = (NS < 8 ? NS : 8) - 1;
    return (b * KH + r) * (KW * 4) + ((sl ^ ((r / RDIV) & SMASK)) << 4);
}
template <int W> struct ResPad { static constexpr int N = W > 8 ? W : 8; };

// Staging image of a wave's input, ES bytes per sample: per array, G::BPW blocks of BB bytes, each followed by PADI bytes (the pad
// spreads the column pass's per-sample reads over the banks); the second array (the prediction) starts ONE bytes above the first.
// Dense batches are fetched in 16-B chunks (NCH per wave), planes in chunks of CS bytes that never cross a block row (NCHP per wave,
// CPR per row); both fill the same image.
template <int W, int H, int ES>
struct StagedIn {
    using G = TxGeom<W, H>;
    static constexpr int BB = W * H * ES, PADI = W * ES >= 32 ? 32 : 16, ONE = G::BPW * (BB + PADI);
    static constexpr int NCH = G::BPW * BB / 16, NCHI = (NCH + 63) / 64;
    static constexpr int ROWB = W * ES, CS = ROWB >= 16 ? 16 : ROWB, PPC = CS / ES, CPR = ROWB / CS, CPBP = BB / CS;
    static constexpr int NCHP = G::BPW * CPBP, NIT = (NCHP + 63) / 64;
};

// ---- per-wave steps of the staged kernels ------------------------------------------------------------------------------------
// fwd_staged_kernel, inv_staged_kernel, enc_staged_body and full_loop_body (kernel_full_loop.h) are sequences of these steps.  A wave
// takes the G::BPW blocks first, first + 1, ...; lane = sub * G::LPB + l (block sub, row or column l); wl is the wave's LDS.  No step
// fences: the caller owes a wave_lds_fence() between a step that writes an LDS region and the next one that reads it, and between
// a step that reads a region and the next one that overwrites it.

// Dense staging: the arrays hold the blocks back to back (BB bytes each); 16-B chunk q of the wave goes to q * 16 + b * PADI.  NA: 1
// (in0 only) or 2 (in0 and in1).  Predicated loads go into zeroed registers (`ok ? *p : zero` makes the compiler park the zero in
// scratch and select the POINTER - a flat load through private memory).  keep[it] (NA == 2): the in1 chunk of iteration it.
// Writes the staging image; the caller owes a fence before the column pass reads it.
template <int W, int H, int ES, int NA>
__device__ __forceinline__ void stage_dense(char* wl, int lane, uint32_t first, uint32_t nblocks, const void* in0, const void* in1,
                                            uint4* keep) {
    using I = StagedIn<W, H, ES>;
    constexpr int NCH = I::NCH;
    const char* g0 = static_cast<const char*>(in0) + (size_t)first * I::BB;
    const char* g1 = NA == 2 ? static_cast<const char*>(in1) + (size_t)first * I::BB : nullptr;
#pragma unroll
    for (int q0 = 0; q0 < NCH; q0 += 64) {
        const int q = q0 + lane;
        uint4 va = make_uint4(0, 0, 0, 0), vb = va;
        if (NCH % 64 == 0 || q < NCH) {
            const int b = (q * 16) / I::BB;
            if (first + b < nblocks) { va = *reinterpret_cast<const uint4*>(g0 + (size_t)q * 16); if (NA == 2) vb = *reinterpret_cast<const uint4*>(g1 + (size_t)q * 16); }
            *reinterpret_cast<uint4*>(wl + q * 16 + b * I::PADI) = va;
            if (NA == 2) *reinterpret_cast<uint4*>(wl + I::ONE + q * 16 + b * I::PADI) = vb;
        }
        if (NA == 2) keep[q0 / 64] = vb;
    }
}

// Plane staging of a source and a prediction array: block b's origin (x, y) = (xy[b] & 0xffff, xy[b] >> 16) on a plane with the
// given row stride (samples); an array whose xy is NULL is dense (as in stage_dense).  Every origin load, then every sample load of
// the lane is issued before the first LDS write.  Out: org[it] = the source origin of chunk it (0 when dense), 0xffffffff past the
// wave's blocks; keep[it] = its prediction chunk.  Writes the staging image; the caller owes a fence before the column pass.
template <int W, int H, int ES>
__device__ __forceinline__ void stage_planes(char* wl, int lane, uint32_t first, uint32_t nblocks, const void* src,
                                             const uint32_t* src_xy, uint32_t src_stride, const void* pred, const uint32_t* pred_xy,
                                             uint32_t pred_stride, uint32_t* org, uint4* keep) {
    using I = StagedIn<W, H, ES>;
    constexpr int NIT = I::NIT, CPBP = I::CPBP;
    uint32_t porg[NIT];
#pragma unroll
    for (int it = 0; it < NIT; it++) {
        const int q = it * 64 + lane, b = q / CPBP;
        const bool ok = q < I::NCHP && first + b < nblocks;
        org[it] = ok ? (src_xy ? src_xy[first + b] : 0u) : 0xffffffffu;
        porg[it] = ok ? (pred_xy ? pred_xy[first + b] : 0u) : 0xffffffffu;
    }
    auto chunk = [&](const void* p, const uint32_t* xy, uint32_t stride, uint32_t o, int q) {
        const int w = q % CPBP;
        const size_t s = xy ? ((o >> 16) + w / I::CPR) * (size_t)stride + (o & 0xffffu) + (w % I::CPR) * I::PPC
                            : (size_t)(first + q / CPBP) * (W * H) + w * I::PPC;
        return static_cast<const char*>(p) + s * ES;
    };
    uint4 v0[NIT];
#pragma unroll
    for (int it = 0; it < NIT; it++) {
        const int q = it * 64 + lane;
        v0[it] = make_uint4(0, 0, 0, 0); keep[it] = v0[it];
        if (org[it] != 0xffffffffu) {
            __builtin_memcpy(&v0[it], chunk(src, src_xy, src_stride, org[it], q), I::CS);
            __builtin_memcpy(&keep[it], chunk(pred, pred_xy, pred_stride, porg[it], q), I::CS);
        }
    }
#pragma unroll
    for (int it = 0; it < NIT; it++) {
        const int q = it * 64 + lane, b = q / CPBP;
        if (I::NCHP % 64 == 0 || q < I::NCHP) {
            __builtin_memcpy(wl + q * I::CS + b * I::PADI, &v0[it], I::CS);
            __builtin_memcpy(wl + I::ONE + q * I::CS + b * I::PADI, &keep[it], I::CS);
        }
    }
}

// Forward column pass, lane l < W: column l of the residual (DIFF: source - prediction of the staging image, InT samples; else the
// int16 residual) with the ud flip and the S0 shift; the caller then runs fwd1d<H, fwd_cos_col(W, H)> on it (see fwd_row_scale for why
// the networks stay in the callers).  bs = wl + sub * (BB + PADI).  Returns the column's SAD (DIFF).
// Reads the staging image; the caller owes a fence before anything overwrites it.
template <int W, int H, typename InT, bool DIFF>
__device__ __forceinline__ unsigned fwd_col_pass(const char* bs, int l, int vk, int (&x)[H]) {
    constexpr int ES = (int)sizeof(InT), ONE = StagedIn<W, H, ES>::ONE, S0 = fwd_shift(W, H, 0);
    unsigned sad = 0;
    if (l < W) {
        const bool ud = vk == K1D_FLIPADST;
#pragma unroll
        for (int r = 0; r < H; r++) {
            const int idx = (ud ? H - 1 - r : r) * W + l;
            int d = (int)*reinterpret_cast<const InT*>(bs + idx * ES);
            if (DIFF) {
                d -= (int)*reinterpret_cast<const InT*>(bs + ONE + idx * ES);
                sad += (unsigned)(d < 0 ? -d : d);
            }
            x[r] = round_shift_c<-S0>(d);
        }
    }
    return sad;
}

// Lane l < W: the column pass's output, S1 shift, into column l (lr flip) of the transpose tile (row pitch G::PITCH).  Writes the
// tile; the caller owes a fence before the row pass.
template <int W, int H>
__device__ __forceinline__ void fwd_col_store(int32_t* tile, int l, int hk, const int (&x)[H]) {
    constexpr int S1 = fwd_shift(W, H, 1);
    if (l < W) {
        const int cdst = hk == K1D_FLIPADST ? W - 1 - l : l;
#pragma unroll
        for (int r = 0; r < H; r++) tile[r * TxGeom<W, H>::PITCH + cdst] = round_shift_c<-S1>(x[r]);
    }
}

// Forward row pass, lane l < H, after the caller's fwd1d<W, fwd_cos_row(W, H)> over row l of the transpose tile: the S2 shift and
// RECT2.  Returns the row's part of three_quad_energy (64-point sizes: the squares of the coefficients outside the KW x KH corner the
// re-pack keeps; 0 otherwise).  Registers only.  (The 1-D networks stay in the callers: called from inside a helper that takes the
// row by reference, they cost up to 60 more VGPRs.)
template <int W, int H>
__device__ __forceinline__ unsigned long long fwd_row_scale(int l, int (&y)[W]) {
    using S = StagedGeom<W, H>;
    constexpr int S2 = fwd_shift(W, H, 2);
    unsigned long long en = 0;
    if (l < H) {
#pragma unroll
        for (int c = 0; c < W; c++) {
            int t = round_shift_c<-S2>(y[c]);
            if (TxGeom<W, H>::RECT2) t = mul_q12(t, 5793);
            y[c] = t;
        }
        if (W > 32 || H > 32) {
#pragma unroll
            for (int c = 0; c < W; c++)
                if (l >= S::KH || c >= S::KW) { const long long v = y[c]; en += (unsigned long long)(v * v); }
        }
    }
    return en;
}

// Lane l < H: row l of the row pass into the out tile (StagedGeom::out_addr).  Writes the out tile; the caller owes a fence before
// the linear phase reads it.
template <int W, int H>
__device__ __forceinline__ void store_out_row(char* wl, int sub, int l, const int (&y)[W]) {
    if (l < H) {
#pragma unroll
        for (int s = 0; s < W / 4; s++)
            *reinterpret_cast<int4*>(wl + StagedGeom<W, H>::out_addr(sub, l, s)) = make_int4(y[4 * s], y[4 * s + 1], y[4 * s + 2], y[4 * s + 3]);
    }
}

// Quantises the wave's KW x KH coefficients per block from the out tile in linear 16-B chunk order (lane = chunk, packed KW * KH per
// block in HBM) and stores qcoeff - and coeff, dqcoeff when CD - and the eob.  dq[it] keeps the lane's dequantised chunk of
// iteration it.  QMODE 2: the host only takes the staged kernels when quant_shift is a power of two.  Reads the out tile; the caller
// owes a fence before anything overwrites it.
template <int W, int H, bool CD>
__device__ __forceinline__ void quant_out_tile(const char* wl, int lane, uint32_t first, uint32_t nblocks, const int16_t* __restrict__ iscan,
                                               const QParams& qp, int32_t* __restrict__ coeff, int32_t* __restrict__ qcoeff,
                                               int32_t* __restrict__ dqcoeff, uint16_t* __restrict__ eob, int4 (&dq)[StagedGeom<W, H>::NQ]) {
    using S = StagedGeom<W, H>;
    constexpr int CPB = S::NC / 4, NOUT = TxGeom<W, H>::BPW * CPB;
    int eob_acc = 0;
#pragma unroll
    for (int it = 0; it < S::NQ; it++) {
        const int q = it * 64 + lane;
        const bool act = (NOUT % 64 == 0) || q < NOUT;
        const int b = act ? q / CPB : 0, w4 = act ? q % CPB : 0;
        const bool ok = act && (first + b < nblocks);
        const int4 c = *reinterpret_cast<const int4*>(wl + S::out_addr(b, w4 / (S::KW / 4), w4 % (S::KW / 4)));
        int4 qv, dv;
        quant_one<2>(c.x, w4 == 0 ? 0 : 1, qp, qv.x, dv.x);
        quant_one<2>(c.y, 1, qp, qv.y, dv.y);
        quant_one<2>(c.z, 1, qp, qv.z, dv.z);
        quant_one<2>(c.w, 1, qp, qv.w, dv.w);
        dq[it] = dv;
        const uint2 is = *reinterpret_cast<const uint2*>(iscan + w4 * 4);
        int e = max(max(qv.x ? (int)(is.x & 0xffffu) + 1 : 0, qv.y ? (int)(is.x >> 16) + 1 : 0),
                    max(qv.z ? (int)(is.y & 0xffffu) + 1 : 0, qv.w ? (int)(is.y >> 16) + 1 : 0));
        if (!act) e = 0;
        if (ok) {
            const size_t o = (size_t)(first + b) * S::NC + (size_t)w4 * 4;
            *reinterpret_cast<int4*>(qcoeff + o) = qv;
            if (CD) { *reinterpret_cast<int4*>(coeff + o) = c; *reinterpret_cast<int4*>(dqcoeff + o) = dv; }
        }
        if constexpr (CPB >= 64) {                        // one block spans CPB/64 iterations of the whole wave
            eob_acc = max(eob_acc, e);
            if ((it + 1) % (CPB / 64) == 0) {
                const int m = group_max<64>(eob_acc);
                if (lane == 0 && ok) eob[first + b] = (uint16_t)m;
                eob_acc = 0;
            }
        } else {                                          // 64/CPB blocks per iteration
            const int m = group_max<(CPB < 64 ? CPB : 64)>(e);
            if (ok && w4 == 0) eob[first + b] = (uint16_t)m;
        }
    }
}

// Inverse row pass, lane l < H: row l of block sub's coefficient tile (coef_tile_addr; rows >= KH and columns >= KW are zero), RECT2,
// clamp to bd + 8 bits, inv1d clamped to the row range (av1_gen_inv_stage_range, EbTransforms.c:5404-5456).  Reads the coefficient
// tile; the caller owes a fence before anything overwrites it.
template <int W, int H>
__device__ __forceinline__ void inv_row_pass(const char* wl, int sub, int l, int hk, int bd, int (&x)[W]) {
    using S = StagedGeom<W, H>;
    constexpr int KW = S::KW;
    const int in_bits = bd + 8, row_bits = bd == 8 ? 16 : (bd == 10 ? 18 : 20);
    if (l < H) {
        if (l < S::KH) {
#pragma unroll
            for (int s = 0; s < KW / 4; s++) {
                const int4 v = *reinterpret_cast<const int4*>(wl + coef_tile_addr<KW, S::KH>(sub, l, s));
                x[4 * s] = v.x; x[4 * s + 1] = v.y; x[4 * s + 2] = v.z; x[4 * s + 3] = v.w;
            }
#pragma unroll
            for (int c = 0; c < W; c++) {
                int v = c < KW ? x[c] : 0;
                if (TxGeom<W, H>::RECT2) v = mul_q12(v, 2896);
                x[c] = svtgen::svt_clamp(v, -(1 << (in_bits - 1)), (1 << (in_bits - 1)) - 1);
            }
            inv1d<W>(hk, x, -(1 << (row_bits - 1)), (1 << (row_bits - 1)) - 1);
        } else {
#pragma unroll
            for (int c = 0; c < W; c++) x[c] = 0;
        }
    }
}

// Lane l < H: row l of the inverse row pass, shifted by inv_shift0, into block sub's transpose tile: int32 at row pitch G::PITCH,
// or (TILE16) clamped to 16 bits at row pitch P16.  Writes the tile; the caller owes a fence before the column pass.
template <int W, int H, bool TILE16>
__device__ __forceinline__ void inv_row_store(char* wl, int sub, int l, const int (&x)[W]) {
    using G = TxGeom<W, H>;
    constexpr int S0 = inv_shift0(W, H), P16 = StagedGeom<W, H>::P16;
    if (l < H) {
        if (TILE16) {
            short* tile16 = reinterpret_cast<short*>(wl) + sub * (H * P16);
            const int lo16 = svtgen::svt_vgpr(-32768), hi16 = svtgen::svt_vgpr(32767);
#pragma unroll
            for (int c = 0; c < W; c++) tile16[l * P16 + c] = (short)svtgen::svt_clamp(round_shift_c<-S0>(x[c]), lo16, hi16);
        } else {
            int32_t* tile = reinterpret_cast<int32_t*>(wl) + sub * G::TILE;
#pragma unroll
            for (int c = 0; c < W; c++) tile[l * G::PITCH + c] = round_shift_c<-S0>(x[c]);
        }
    }
}

// Inverse column pass, lane l < W: column l (lr flip) of block sub's transpose tile clamped to the column input range (TILE16: already
// clamped to 16 bits, which is that range for bd <= 10), inv1d clamped to the column range.  Reads the tile; the caller owes a fence
// before anything overwrites it.
template <int W, int H, bool TILE16>
__device__ __forceinline__ void inv_col_pass(const char* wl, int sub, int l, int vk, int hk, int bd, int (&y)[H]) {
    using G = TxGeom<W, H>;
    constexpr int P16 = StagedGeom<W, H>::P16;
    const int colin_bits = bd + 6 > 16 ? bd + 6 : 16, col_bits = bd == 12 ? 18 : 16;
    if (l < W) {
        const int csrc = hk == K1D_FLIPADST ? W - 1 - l : l;
        if (TILE16) {
            const short* tile16 = reinterpret_cast<const short*>(wl) + sub * (H * P16);
#pragma unroll
            for (int r = 0; r < H; r++) y[r] = tile16[r * P16 + csrc];
        } else {
            const int32_t* tile = reinterpret_cast<const int32_t*>(wl) + sub * G::TILE;
#pragma unroll
            for (int r = 0; r < H; r++) y[r] = svtgen::svt_clamp(tile[r * G::PITCH + csrc], -(1 << (colin_bits - 1)), (1 << (colin_bits - 1)) - 1);
        }
        inv1d<H>(vk, y, -(1 << (col_bits - 1)), (1 << (col_bits - 1)) - 1);
    }
}

// Lane l < W: column l of the inverse column pass, shifted by 4 (ud flip), into block sub's int16 residual tile (row-major, W * H +
// ResPad<W> per block).  The add to the sample runs on 16-bit lanes (the reference adds in int32, highbd_clip_pixel_add): exact for
// bd <= 10, where every column kernel's output is at most 16 bits (12 after this shift, identities 14); bd 12 takes the general
// kernel (svt_hip_inv_txfm2d_add_batch), so no wrap can occur here.  Writes the residual tile; the caller owes a fence before
// add_clip reads it.
template <int W, int H>
__device__ __forceinline__ void inv_res_write(char* wl, int sub, int l, int vk, const int (&y)[H]) {
    if (l < W) {
        short* res = reinterpret_cast<short*>(wl) + sub * (W * H + ResPad<W>::N);
        if (vk == K1D_FLIPADST) {
#pragma unroll
            for (int r = 0; r < H; r++) res[r * W + l] = (short)round_shift_c<4>(y[H - 1 - r]);
        } else {
#pragma unroll
            for (int r = 0; r < H; r++) res[r * W + l] = (short)round_shift_c<4>(y[r]);
        }
    }
}

// Reconstruction of one chunk of CS bytes (CS / sizeof(PixT) samples, CS <= 16): prediction p + the int16 residuals at res (residual
// tile, LDS), clipped.  The add / clip runs on 16-bit lanes (v_pk_add_i16, v_sat_pk_u8_i16 or v_pk_max/min_i16) - SDWA / bfe byte
// arithmetic costs ~4x as much.  Words of the result past CS are 0.
template <typename PixT, int CS>
__device__ __forceinline__ uint4 add_clip(uint4 p, const short* res, int maxpix) {
    constexpr int ES = (int)sizeof(PixT), NRW = CS / (2 * ES);          // residual words: (r0,r1) (r2,r3) ...
    uint32_t rw[8];
    if constexpr (NRW >= 4) {
#pragma unroll
        for (int i = 0; i < NRW / 4; i++) {
            const uint4 v = reinterpret_cast<const uint4*>(res)[i];
            rw[4 * i] = v.x; rw[4 * i + 1] = v.y; rw[4 * i + 2] = v.z; rw[4 * i + 3] = v.w;
        }
    } else {
        const uint2 v = *reinterpret_cast<const uint2*>(res);
        rw[0] = v.x; rw[1] = v.y;
    }
    const uint32_t pw[4] = {p.x, p.y, p.z, p.w};
    uint32_t ow[4] = {0, 0, 0, 0};
#pragma unroll
    for (int k = 0; k < CS / 4; k++) {
        if constexpr (ES == 1) {
            const uint32_t p01 = __builtin_amdgcn_perm(0u, pw[k], 0x0c010c00u);       // bytes 0,1 -> 16-bit lanes
            const uint32_t p23 = __builtin_amdgcn_perm(0u, pw[k], 0x0c030c02u);       // bytes 2,3
            const uint32_t u01 = sat_pk_u8_i16(pk_add_i16(p01, rw[2 * k])), u23 = sat_pk_u8_i16(pk_add_i16(p23, rw[2 * k + 1]));
            ow[k] = (u23 << 16) | (u01 & 0xffffu);
        } else {
            ow[k] = pk_clamp_i16(pk_add_i16(pw[k], rw[k]), maxpix);
        }
    }
    return make_uint4(ow[0], ow[1], ow[2], ow[3]);
}

// Register classes of the group-table launches (enc_frame_kernel, kernel_frame.h; full_loop_kernel, kernel_full_loop.h): 0 both sides
// <= 16, 1 a 32- or 64-sample side except 64x64, 2 64x64.  THE list of sizes per class, entries (TxSize number, W, H) in the
// reference's numbering (EbDefinitions.h:615-650); tx_class_of, the kernels' LDS maxima and the case lists of their switches are
// generated from it.  X takes every entry but the last, L the last one (a switch's default:).
#define SVT_TX_CLASS0(X, L) X(0, 4, 4) X(1, 8, 8) X(2, 16, 16) X(5, 4, 8) X(6, 8, 4) X(7, 8, 16) X(8, 16, 8) X(13, 4, 16) L(14, 16, 4)
// Class 1 in two halves, without and with a 64-sample side: the kernels that walk the final block list (recon_final_kernel,
// ie_walk_kernel) launch them apart.  With class 0 and 64x64 they are the launch kinds 0 .. 3 of av1_geom.h's tx_launch_kind.
#define SVT_TX_CLASS1A(X, L) X(3, 32, 32) X(9, 16, 32) X(10, 32, 16) X(15, 8, 32) L(16, 32, 8)
#define SVT_TX_CLASS1B(X, L) X(11, 32, 64) X(12, 64, 32) X(17, 16, 64) L(18, 64, 16)
#define SVT_TX_CLASS1(X, L) SVT_TX_CLASS1A(X, X) SVT_TX_CLASS1B(X, L)
#define SVT_TX_BIT(N, W, H) | (1u << N)
constexpr unsigned kTxClass0 = 0u SVT_TX_CLASS0(SVT_TX_BIT, SVT_TX_BIT), kTxClass1 = 0u SVT_TX_CLASS1(SVT_TX_BIT, SVT_TX_BIT), kTxClass2 = 1u << 4;
#undef SVT_TX_BIT
static_assert((kTxClass0 ^ kTxClass1 ^ kTxClass2) == (1u << 19) - 1 && !(kTxClass0 & kTxClass1), "each of the sizes 0 .. 18 lands in exactly one class");
#define SVT_TX_KIND_IS(K, N, W, H) &&svthost::tx_launch_kind(N) == K && svthost::kTxW[N] == W && svthost::kTxH[N] == H
#define SVT_TX_KIND0(N, W, H) SVT_TX_KIND_IS(0, N, W, H)
#define SVT_TX_KIND1(N, W, H) SVT_TX_KIND_IS(1, N, W, H)
#define SVT_TX_KIND2(N, W, H) SVT_TX_KIND_IS(2, N, W, H)
static_assert(svthost::tx_launch_kind(4) == 3 SVT_TX_CLASS0(SVT_TX_KIND0, SVT_TX_KIND0) SVT_TX_CLASS1A(SVT_TX_KIND1, SVT_TX_KIND1) SVT_TX_CLASS1B(SVT_TX_KIND2, SVT_TX_KIND2),
              "av1_geom.h and the four lists (class 1 being its two halves) agree on sizes, sides and launch kinds");
#undef SVT_TX_KIND_IS
#undef SVT_TX_KIND0
#undef SVT_TX_KIND1
#undef SVT_TX_KIND2
// bit masks, not a table: usable on the device with a run-time size
__host__ __device__ constexpr int tx_class_of(int tx_size) {
    return tx_size == 4 ? 2 : (((kTxClass0 >> tx_size) & 1u) ? 0 : 1);
}
// the launch geometry the host plans with (tx_plan.h) is the kernels', for every one of the 19 sizes
#define SVT_TX_GEOM_IS(N, W, H)                                                                                                                   \
    &&svthost::tx_general_blocks_per_wg(N) == TX_WAVES * TxGeom<W, H>::BPW && svthost::tx_staged_waves(W, H) == StagedGeom<W, H>::WAVES &&         \
        svthost::tx_staged_blocks_per_wg(N) == StagedGeom<W, H>::WAVES * TxGeom<W, H>::BPW && svthost::tx_class(N) == tx_class_of(N)
static_assert(svthost::kTxWaves == TX_WAVES SVT_TX_CLASS0(SVT_TX_GEOM_IS, SVT_TX_GEOM_IS) SVT_TX_CLASS1(SVT_TX_GEOM_IS, SVT_TX_GEOM_IS) SVT_TX_GEOM_IS(4, 64, 64),
              "tx_plan.h and the kernels agree on waves, blocks per workgroup and register class");
#undef SVT_TX_GEOM_IS
// the largest of a list: cmax_of({SVT_TX_CLASS0(V, V)}) with V(N, W, H) = a size's value and a comma
constexpr int cmax_of(std::initializer_list<int> v) {
    int m = 0;
    for (int x : v) m = cmax(m, x);
    return m;
}

// PixT: sample type of src / pred in MODE 1 (uint8_t, or uint16_t for 10-bit).  xy != NULL: the blocks are
// addressed on picture planes (origin (x, y) = (xy[b] & 0xffff, xy[b] >> 16), row strides in samples) and are
// fetched row segment by row segment into the same linear staging image; NULL: dense batches.
template <int W, int H, int MODE, typename PixT = uint8_t>
__global__ __launch_bounds__(StagedWaves<W * H>::N * 64) void fwd_staged_kernel(
    const void* __restrict__ in0, const void* __restrict__ pred, int32_t* __restrict__ coeff,
    int32_t* __restrict__ qcoeff, int32_t* __restrict__ dqcoeff, uint16_t* __restrict__ eob,
    uint32_t* __restrict__ sad, unsigned long long* __restrict__ energy, const int16_t* __restrict__ iscan,
    QParams qp, int tx_type, uint32_t nblocks, const uint32_t* __restrict__ xy = nullptr, uint32_t src_stride = 0,
    uint32_t pred_stride = 0) {
    using S = StagedGeom<W, H>;
    using G = TxGeom<W, H>;
    constexpr bool FUSED = MODE == 1;
    using InT = std::conditional_t<FUSED, PixT, int16_t>;
    constexpr int ES = (int)sizeof(InT);
    using I = StagedIn<W, H, ES>;
    constexpr int IN_BYTES = I::ONE * (FUSED ? 2 : 1);
    constexpr int TILE_BYTES = G::BPW * G::TILE * 4;
    constexpr int OUT_BYTES = G::BPW * W * H * 4;
    constexpr int WAVE_LDS = (cmax(cmax(IN_BYTES, TILE_BYTES), OUT_BYTES) + 15) & ~15;
    __shared__ __attribute__((aligned(16))) char lds[S::WAVES * WAVE_LDS];

    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    char* wl = lds + wave * WAVE_LDS;
    const uint32_t first = (blockIdx.x * S::WAVES + wave) * G::BPW;
    if (first >= nblocks) return;                         // wave-uniform
    const int sub = lane / G::LPB, l = lane % G::LPB;
    const uint32_t blk = first + sub;
    const bool valid = blk < nblocks;
    const int vk = kVKind[tx_type], hk = kHKind[tx_type];

    uint32_t org[I::NIT];
    uint4 pv[I::NIT > I::NCHI ? I::NIT : I::NCHI];
    if (FUSED && xy) stage_planes<W, H, ES>(wl, lane, first, nblocks, in0, xy, src_stride, pred, xy, pred_stride, org, pv);
    else stage_dense<W, H, ES, FUSED ? 2 : 1>(wl, lane, first, nblocks, in0, pred, pv);
    wave_lds_fence();
    int x[H];
    unsigned sad_acc = fwd_col_pass<W, H, InT, FUSED>(wl + sub * (I::BB + I::PADI), l, vk, x);
    if (l < W) fwd1d<H, fwd_cos_col(W, H)>(vk, x);
    wave_lds_fence();                                     // staging is dead: the tile may overwrite it
    int32_t* tile = reinterpret_cast<int32_t*>(wl) + sub * G::TILE;
    fwd_col_store<W, H>(tile, l, hk, x);
    wave_lds_fence();
    int y[W];
    if (l < H) {
#pragma unroll
        for (int c = 0; c < W; c++) y[c] = tile[l * G::PITCH + c];
        fwd1d<W, fwd_cos_row(W, H)>(hk, y);
    }
    unsigned long long en = fwd_row_scale<W, H>(l, y);
    wave_lds_fence();                                     // tile is dead: the out tile may overwrite it
    store_out_row<W, H>(wl, sub, l, y);
    wave_lds_fence();
    if (FUSED) {
        sad_acc = group_sum<G::LPB>(sad_acc);
        if (W > 32 || H > 32) en = group_sum64<G::LPB>(en);
        if (valid && l == 0) {
            if (sad) sad[blk] = sad_acc;
            if (energy) energy[blk] = en;
        }
    }
    // ---- linear phase: coalesced stores (and quantisation) ----------------------------------
    if (!FUSED) {
        constexpr int CPB = W * H / 4;                    // chunks per block
        constexpr int NOUT = G::BPW * CPB;
        int4* o4 = reinterpret_cast<int4*>(coeff + (size_t)first * (W * H));
#pragma unroll
        for (int q0 = 0; q0 < NOUT; q0 += 64) {
            const int q = q0 + lane;
            if (NOUT % 64 == 0 || q < NOUT) {
                const int b = q / CPB, w4 = q % CPB;
                const int4 v = *reinterpret_cast<const int4*>(wl + S::out_addr(b, w4 / (W / 4), w4 % (W / 4)));
                if (first + b < nblocks) o4[q] = v;
            }
        }
    } else {
        int4 dq[S::NQ];
        quant_out_tile<W, H, true>(wl, lane, first, nblocks, iscan, qp, coeff, qcoeff, dqcoeff, eob, dq);
    }
}

// ---------------------------------------------------------------------------
// inverse + add for DENSE batches (coefficients packed KW*KH per block, destination
// blocks W*H samples back to back): linear coefficient chunks -> padded LDS rows ->
// row pass -> transpose tile -> column pass -> int16 residual tile in row order ->
// destination read / add / clip / write in linear 16-B chunks.
// Math == inv_txfm2d_add_kernel (kernel_txfm.h) == inv_txfm2d_add_c (EbTransforms.c:8180).
// ---------------------------------------------------------------------------
// dst_offsets != NULL: destination block b starts at dst + dst_offsets[b] (samples) with row stride dst_stride
// (reconstruction written in place into a picture plane); NULL: dense W*H blocks back to back.
// TILE16 (bd <= 10: the column pass clamps its input to 16 bits anyway): the transpose tile holds the row-pass output
// already clamped, as int16 - half the LDS, which is what limits the 64-point sizes to 2 waves per SIMD.
template <int W, int H, typename PixT, bool TILE16 = false>
__global__ __launch_bounds__(StagedWaves<W * H>::N * 64) void inv_staged_kernel(
    const int32_t* __restrict__ in, PixT* __restrict__ dst, int tx_type, int bd, uint32_t nblocks,
    const uint32_t* __restrict__ dst_offsets = nullptr, int32_t dst_stride = 0) {
    using S = StagedGeom<W, H>;
    using G = TxGeom<W, H>;
    constexpr int KW = S::KW, KH = S::KH, NC = S::NC;
    constexpr int IN_BYTES = G::BPW * KH * KW * 4;        // coefficient tile, slots swizzled by the row (coef_tile_addr)
    constexpr int RPAD = ResPad<W>::N;
    constexpr int TILE_BYTES = TILE16 ? G::BPW * H * S::P16 * 2 : G::BPW * G::TILE * 4;
    constexpr int RES_BYTES = G::BPW * (W * H + RPAD) * 2;
    constexpr int WAVE_LDS = (cmax(cmax(IN_BYTES, TILE_BYTES), RES_BYTES) + 15) & ~15;
    __shared__ __attribute__((aligned(16))) char lds[S::WAVES * WAVE_LDS];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    char* wl = lds + wave * WAVE_LDS;
    const uint32_t first = (blockIdx.x * S::WAVES + wave) * G::BPW;
    if (first >= nblocks) return;
    const int sub = lane / G::LPB, l = lane % G::LPB;
    const int vk = kVKind[tx_type], hk = kHKind[tx_type];
    const int maxpix = (1 << bd) - 1;
    // ---- stage coefficients ----------------------------------------------------------------
    {
        constexpr int CPB = NC / 4, NCH = G::BPW * CPB;
        const int4* g = reinterpret_cast<const int4*>(in + (size_t)first * NC);
#pragma unroll
        for (int q0 = 0; q0 < NCH; q0 += 64) {
            const int q = q0 + lane;
            if (NCH % 64 == 0 || q < NCH) {
                const int b = q / CPB, w4 = q % CPB;
                int4 v = make_int4(0, 0, 0, 0);
                if (first + b < nblocks) v = g[q];
                *reinterpret_cast<int4*>(wl + coef_tile_addr<KW, KH>(b, w4 / (KW / 4), w4 % (KW / 4))) = v;
            }
        }
    }
    wave_lds_fence();
    int x[W];
    inv_row_pass<W, H>(wl, sub, l, hk, bd, x);
    wave_lds_fence();
    inv_row_store<W, H, TILE16>(wl, sub, l, x);
    wave_lds_fence();
    int y[H];
    inv_col_pass<W, H, TILE16>(wl, sub, l, vk, hk, bd, y);
    wave_lds_fence();
    inv_res_write<W, H>(wl, sub, l, vk, y);
    wave_lds_fence();
    const short* res = reinterpret_cast<const short*>(wl);
    if (dst_offsets) {
        // ---- destination on a plane: chunks of CS bytes that never cross a block row ---------------------
        using I = StagedIn<W, H, (int)sizeof(PixT)>;
        constexpr int NIT = I::NIT, CPBP = I::CPBP;
        uint32_t org[NIT];
#pragma unroll
        for (int it = 0; it < NIT; it++) {
            const int q = it * 64 + lane, b = q / CPBP;
            org[it] = (q < I::NCHP && first + b < nblocks) ? dst_offsets[first + b] : 0xffffffffu;
        }
        uint4 pvv[NIT];
        PixT* dp[NIT];
#pragma unroll
        for (int it = 0; it < NIT; it++) {
            const int q = it * 64 + lane, w = q % CPBP;
            pvv[it] = make_uint4(0, 0, 0, 0);
            dp[it] = dst + (size_t)(org[it] == 0xffffffffu ? 0u : org[it]) + (size_t)(w / I::CPR) * dst_stride + (w % I::CPR) * I::PPC;
            if (org[it] != 0xffffffffu) __builtin_memcpy(&pvv[it], dp[it], I::CS);
        }
#pragma unroll
        for (int it = 0; it < NIT; it++) {
            const int q = it * 64 + lane;
            if (org[it] != 0xffffffffu) {
                // q-th chunk of the wave = PPC consecutive residuals of the row-major int16 tile
                const uint4 o = add_clip<PixT, I::CS>(pvv[it], res + (size_t)q * I::PPC + (q / CPBP) * RPAD, maxpix);
                __builtin_memcpy(dp[it], &o, I::CS);
            }
        }
    } else {
        // ---- destination: linear 16-B chunks --------------------------------------------------------
        constexpr int PPL = 16 / (int)sizeof(PixT);
        constexpr int CPB = W * H / PPL, NCH = G::BPW * CPB;
        static_assert(W * H % PPL == 0, "block must be a whole number of 16-B chunks");
        uint4* d4 = reinterpret_cast<uint4*>(dst + (size_t)first * (W * H));
#pragma unroll
        for (int q0 = 0; q0 < NCH; q0 += 64) {
            const int q = q0 + lane;
            if ((NCH % 64 == 0 || q < NCH) && (first + q / CPB < nblocks))
                d4[q] = add_clip<PixT, 16>(d4[q], res + (size_t)q * PPL + (q / CPB) * RPAD, maxpix);
        }
    }
}

// ---------------------------------------------------------------------------
// enc_staged_kernel<W, H, KEEP> — the encode-pass chain (see enc32_kernel in kernel_fused32.h) for every
// other size, 8-bit dense batches: fwd_staged_kernel<W, H, 1> up to the quantiser, whose dequantised 16-B
// chunks are written straight into the coefficient rows inv_staged_kernel starts from; the prediction
// chunks loaded for the residual stay in registers and are the destination of the reconstruction.
// HBM traffic: 2*W*H in + 4*KW*KH (qcoeff) + W*H (recon) + 6 B out (+ coeff, dqcoeff when KEEP).
// ---------------------------------------------------------------------------
template <int W, int H, typename PixT>
struct EncStagedLds {                                    // LDS bytes per wave / per workgroup of enc_staged_body<W, H, ., PixT>
    using G = TxGeom<W, H>;
    // input staging (StagedIn).  For 64-byte blocks - 8x8 8-bit - the pad makes the linear 16-byte staging stores 2-way conflicts;
    // the unpadded form with the chunks of block b XOR-swizzled by b >> 1 is conflict-free on both sides and was measured 2 %
    // SLOWER, A/B on one box: the kernel is bound by VALU issue, and the swizzle puts address arithmetic into the column pass.
    static constexpr int IN_ONE = StagedIn<W, H, (int)sizeof(PixT)>::ONE;
    static constexpr int WAVE = (cmax(cmax(IN_ONE * 2, G::BPW * G::TILE * 4), G::BPW * W * H * 4) + 15) & ~15;
    static constexpr int BYTES = StagedGeom<W, H>::WAVES * WAVE;
};
template <int W, int H, bool KEEP, typename PixT, int BD>
__device__ __forceinline__ void enc_staged_body(
    const PixT* __restrict__ src, const PixT* __restrict__ pred, PixT* __restrict__ recon,
    int32_t* __restrict__ coeff, int32_t* __restrict__ qcoeff, int32_t* __restrict__ dqcoeff,
    uint16_t* __restrict__ eob, uint32_t* __restrict__ sad, const int16_t* __restrict__ iscan, const QParams& qp,
    int tx_type, uint32_t nblocks, const uint32_t* __restrict__ xy, uint32_t src_stride,
    uint32_t pred_stride, uint32_t recon_stride, uint32_t bid, char* lds) {
    // xy != NULL: blocks addressed on picture planes (origin (x, y) = (xy[b] & 0xffff, xy[b] >> 16), row strides
    // in samples; recon may be the prediction plane itself); NULL: dense batches.
    using S = StagedGeom<W, H>;
    using G = TxGeom<W, H>;
    constexpr int KW = S::KW, KH = S::KH;
    constexpr int ES = (int)sizeof(PixT);                // 1, or 2 for 10-bit samples (BD = 10)
    using I = StagedIn<W, H, ES>;
    constexpr int RPAD = ResPad<W>::N, WAVE_LDS = EncStagedLds<W, H, PixT>::WAVE, maxpix = (1 << BD) - 1;
    static_assert(W * H % 16 == 0, "block must be a whole number of 16-B chunks");

    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    char* wl = lds + wave * WAVE_LDS;
    if (wave >= S::WAVES) return;                           // (run inside a larger workgroup: the spare waves have nothing to do)
    const uint32_t first = (bid * S::WAVES + wave) * G::BPW;
    if (first >= nblocks) return;                         // wave-uniform
    const int sub = lane / G::LPB, l = lane % G::LPB;
    const uint32_t blk = first + sub;
    const bool valid = blk < nblocks;
    const int vk = kVKind[tx_type], hk = kHKind[tx_type];
    int32_t* tile = reinterpret_cast<int32_t*>(wl) + sub * G::TILE;

    // ---- stage the wave's input; the prediction chunks stay in registers ----
    uint4 pk[I::NIT > I::NCHI ? I::NIT : I::NCHI];
    uint32_t org[I::NIT];
    if (xy) stage_planes<W, H, ES>(wl, lane, first, nblocks, src, xy, src_stride, pred, xy, pred_stride, org, pk);
    else stage_dense<W, H, ES, 2>(wl, lane, first, nblocks, src, pred, pk);
    wave_lds_fence();
    // ---- forward ----
    unsigned sad_acc;
    {
        int x[H];
        sad_acc = fwd_col_pass<W, H, PixT, true>(wl + sub * (I::BB + I::PADI), l, vk, x);
        if (l < W) fwd1d<H, fwd_cos_col(W, H)>(vk, x);
        wave_lds_fence();                                 // staging is dead: the tile may overwrite it
        fwd_col_store<W, H>(tile, l, hk, x);
    }
    wave_lds_fence();
    {
        int y[W];
        if (l < H) {
#pragma unroll
            for (int c = 0; c < W; c++) y[c] = tile[l * G::PITCH + c];
            fwd1d<W, fwd_cos_row(W, H)>(hk, y);
        }
        fwd_row_scale<W, H>(l, y);
        wave_lds_fence();                                 // tile is dead: the out tile may overwrite it
        store_out_row<W, H>(wl, sub, l, y);
    }
    wave_lds_fence();
    sad_acc = group_sum<G::LPB>(sad_acc);
    if (valid && l == 0 && sad) sad[blk] = sad_acc;
    // ---- quantise; the dequantised chunks, from registers, become the coefficient rows of the inverse ----
    int4 dvs[S::NQ];
    quant_out_tile<W, H, KEEP>(wl, lane, first, nblocks, iscan, qp, coeff, qcoeff, dqcoeff, eob, dvs);
    wave_lds_fence();                                     // the out tile is dead: coefficient rows may overwrite it
    {
        constexpr int CPB = S::NC / 4, NOUT = G::BPW * CPB;
#pragma unroll
        for (int it = 0; it < S::NQ; it++) {
            const int q = it * 64 + lane;
            if (NOUT % 64 == 0 || q < NOUT) {
                const int b = q / CPB, w4 = q % CPB;
                *reinterpret_cast<int4*>(wl + coef_tile_addr<KW, KH>(b, w4 / (KW / 4), w4 % (KW / 4))) = dvs[it];
            }
        }
    }
    wave_lds_fence();
    // ---- inverse (inv_staged_kernel<W, H, PixT>, bd = BD) ----
    {
        int x[W];
        inv_row_pass<W, H>(wl, sub, l, hk, BD, x);
        wave_lds_fence();
        inv_row_store<W, H, false>(wl, sub, l, x);
    }
    wave_lds_fence();
    {
        int y[H];
        inv_col_pass<W, H, false>(wl, sub, l, vk, hk, BD, y);
        wave_lds_fence();
        inv_res_write<W, H>(wl, sub, l, vk, y);
    }
    wave_lds_fence();
    // ---- reconstruction = prediction (still in registers) + residual ----
    const short* res = reinterpret_cast<const short*>(wl);
    if (xy) {
#pragma unroll
        for (int it = 0; it < I::NIT; it++) {
            const int q = it * 64 + lane, w = q % I::CPBP;
            if (org[it] != 0xffffffffu) {
                const uint4 o = add_clip<PixT, I::CS>(pk[it], res + (size_t)q * I::PPC + (q / I::CPBP) * RPAD, maxpix);
                const size_t y = (org[it] >> 16) + w / I::CPR, x = (org[it] & 0xffffu) + (w % I::CPR) * I::PPC;
                __builtin_memcpy(recon + y * recon_stride + x, &o, I::CS);
            }
        }
    } else {
        uint4* d4 = reinterpret_cast<uint4*>(reinterpret_cast<char*>(recon) + (size_t)first * I::BB);
        constexpr int NCH = I::NCH, PP16 = 16 / ES;       // pixels per 16-B chunk
#pragma unroll
        for (int it = 0; it < I::NCHI; it++) {
            const int q = it * 64 + lane;
            if ((NCH % 64 == 0 || q < NCH) && (first + (q * 16) / I::BB < nblocks))
                d4[q] = add_clip<PixT, 16>(pk[it], res + (size_t)q * PP16 + ((q * 16) / I::BB) * RPAD, maxpix);
        }
    }
}

template <int W, int H, bool KEEP, typename PixT = uint8_t, int BD = 8>
__global__ __launch_bounds__(StagedWaves<W * H>::N * 64) void enc_staged_kernel(
    const PixT* __restrict__ src, const PixT* __restrict__ pred, PixT* __restrict__ recon,
    int32_t* __restrict__ coeff, int32_t* __restrict__ qcoeff, int32_t* __restrict__ dqcoeff,
    uint16_t* __restrict__ eob, uint32_t* __restrict__ sad, const int16_t* __restrict__ iscan, QParams qp,
    int tx_type, uint32_t nblocks, const uint32_t* __restrict__ xy = nullptr, uint32_t src_stride = 0,
    uint32_t pred_stride = 0, uint32_t recon_stride = 0) {
    __shared__ __attribute__((aligned(16))) char lds[EncStagedLds<W, H, PixT>::BYTES];
    enc_staged_body<W, H, KEEP, PixT, BD>(src, pred, recon, coeff, qcoeff, dqcoeff, eob, sad, iscan, qp, tx_type, nblocks, xy, src_stride,
                                          pred_stride, recon_stride, blockIdx.x, lds);
}


// ---------------------------------------------------------------------------
// enc4_kernel<PixT, BD, KEEP> — the encode-pass chain for TX_4X4, all 16 transform types: ONE LANE PER BLOCK, the whole
// block in registers (16 residuals, two passes of four 4-point transforms each way), no LDS.  Adjacent lanes take adjacent
// blocks, so on planes a row of 64 blocks is fetched as 64 adjacent 4-sample loads per block row.  Replaces the two-stage
// path (forward + quantise kernel, device copy, inverse kernel) the 4x4 blocks took in round 1: 2 x 16 B in, 64 B qcoeff +
// 16 B reconstruction out per block instead of two launches and the coeff / dqcoeff round trip through HBM.
// Reference chain: Av1EncodeLoop (EbCodingLoop.c:617-753) with av1_fwd_txfm2d_4x4 (shift {2, 0, 0}, cos_bit 13 / 13,
// EbTransforms.h:120-156), aom_highbd_quantize_b (log_scale 0) and av1_inv_txfm2d_add_4x4 (shift {0, -4}).
// qfast: the quantiser table has power-of-two quant_shift (host-checked): one-product form; else the exact 64-bit form.
// ---------------------------------------------------------------------------
template <typename PixT, int BD, bool KEEP>
__device__ __forceinline__ void enc4_body(
    const PixT* __restrict__ src, const PixT* __restrict__ pred, PixT* __restrict__ recon,
    int32_t* __restrict__ coeff, int32_t* __restrict__ qcoeff, int32_t* __restrict__ dqcoeff,
    uint16_t* __restrict__ eob, uint32_t* __restrict__ sad, const int16_t* __restrict__ iscan, const QParams& qp, int qfast,
    int tx_type, uint32_t nblocks, const uint32_t* __restrict__ xy, uint32_t src_stride, uint32_t pred_stride,
    uint32_t recon_stride, uint32_t bid) {
    const uint32_t blk = bid * 256u + threadIdx.x;
    if (blk >= nblocks) return;
    constexpr int in_bits = BD + 8, row_bits = BD == 8 ? 16 : (BD == 10 ? 18 : 20);      // av1_gen_inv_stage_range (:5404-5456)
    constexpr int cin_bits = BD + 6 > 16 ? BD + 6 : 16, col_bits = BD == 12 ? 18 : 16, maxpix = (1 << BD) - 1;
    const int vk = kVKind[tx_type], hk = kHKind[tx_type];
    const bool ud = vk == K1D_FLIPADST, lr = hk == K1D_FLIPADST;
    size_t so, po, ro;
    uint32_t ss = 4, ps = 4, rs = 4;
    if (xy) {
        const uint32_t o = xy[blk];
        const size_t x = o & 0xffffu, y = o >> 16;
        ss = src_stride; ps = pred_stride; rs = recon_stride;
        so = y * ss + x; po = y * ps + x; ro = y * rs + x;
    } else {
        so = po = ro = (size_t)blk * 16;
    }
    PixT sv[4][4], pv[4][4];
#pragma unroll
    for (int r = 0; r < 4; r++) {
        __builtin_memcpy(sv[r], src + so + (size_t)r * ss, 4 * sizeof(PixT));
        __builtin_memcpy(pv[r], pred + po + (size_t)r * ps, 4 * sizeof(PixT));
    }
    int d[4][4];
    unsigned sad_acc = 0;
#pragma unroll
    for (int r = 0; r < 4; r++)
#pragma unroll
        for (int c = 0; c < 4; c++) {
            d[r][c] = (int)sv[r][c] - (int)pv[r][c];
            sad_acc += (unsigned)(d[r][c] < 0 ? -d[r][c] : d[r][c]);
        }
    if (sad) sad[blk] = sad_acc;
    // ---- forward: columns (up-shift 2, ud flip on the way in, lr flip on the way out), then rows ----
    int t[4][4];
#pragma unroll
    for (int c = 0; c < 4; c++) {
        int x[4];
#pragma unroll
        for (int r = 0; r < 4; r++) x[r] = (ud ? d[3 - r][c] : d[r][c]) * 4;
        fwd1d<4, 13>(vk, x);
#pragma unroll
        for (int r = 0; r < 4; r++) t[r][c] = x[r];
    }
    int co[16];
#pragma unroll
    for (int r = 0; r < 4; r++) {
        int y[4];
#pragma unroll
        for (int c = 0; c < 4; c++) y[c] = lr ? t[r][3 - c] : t[r][c];      // column c of the pass-1 output went to 3 - c
        fwd1d<4, 13>(hk, y);
#pragma unroll
        for (int c = 0; c < 4; c++) co[r * 4 + c] = y[c];
    }
    // ---- quantise / dequantise / eob ----
    int q[16], dq[16];
    int e = 0;
#pragma unroll
    for (int i = 0; i < 16; i++) {
        if (qfast) quant_one<2>(co[i], i == 0 ? 0 : 1, qp, q[i], dq[i]);
        else quant_one<0>(co[i], i == 0 ? 0 : 1, qp, q[i], dq[i]);
        e = max(e, q[i] ? (int)iscan[i] + 1 : 0);
    }
    eob[blk] = (uint16_t)e;
    {
        int4* qo = reinterpret_cast<int4*>(qcoeff + (size_t)blk * 16);
#pragma unroll
        for (int r = 0; r < 4; r++) __builtin_memcpy(qo + r, &q[4 * r], 16);
        if (KEEP) {
            int4* c4 = reinterpret_cast<int4*>(coeff + (size_t)blk * 16);
            int4* d4 = reinterpret_cast<int4*>(dqcoeff + (size_t)blk * 16);
#pragma unroll
            for (int r = 0; r < 4; r++) { __builtin_memcpy(c4 + r, &co[4 * r], 16); __builtin_memcpy(d4 + r, &dq[4 * r], 16); }
        }
    }
    // ---- inverse: rows (clamp bd + 8, shift 0), columns (clamp, shift 4), flips, add, clip ----
#pragma unroll
    for (int r = 0; r < 4; r++) {
        int x[4];
#pragma unroll
        for (int c = 0; c < 4; c++) x[c] = svtgen::svt_clamp(dq[r * 4 + c], -(1 << (in_bits - 1)), (1 << (in_bits - 1)) - 1);
        inv1d<4>(hk, x, -(1 << (row_bits - 1)), (1 << (row_bits - 1)) - 1);
#pragma unroll
        for (int c = 0; c < 4; c++) t[r][c] = x[c];
    }
    PixT ov[4][4];
#pragma unroll
    for (int c = 0; c < 4; c++) {
        int y[4];
#pragma unroll
        for (int r = 0; r < 4; r++) y[r] = svtgen::svt_clamp(lr ? t[r][3 - c] : t[r][c], -(1 << (cin_bits - 1)), (1 << (cin_bits - 1)) - 1);
        inv1d<4>(vk, y, -(1 << (col_bits - 1)), (1 << (col_bits - 1)) - 1);
#pragma unroll
        for (int r = 0; r < 4; r++) {
            const int res = round_shift_c<4>(ud ? y[3 - r] : y[r]);
            ov[r][c] = (PixT)min(max((int)pv[r][c] + res, 0), maxpix);
        }
    }
#pragma unroll
    for (int r = 0; r < 4; r++) __builtin_memcpy(recon + ro + (size_t)r * rs, ov[r], 4 * sizeof(PixT));
}

template <typename PixT, int BD, bool KEEP>
__global__ __launch_bounds__(256) void enc4_kernel(
    const PixT* __restrict__ src, const PixT* __restrict__ pred, PixT* __restrict__ recon,
    int32_t* __restrict__ coeff, int32_t* __restrict__ qcoeff, int32_t* __restrict__ dqcoeff,
    uint16_t* __restrict__ eob, uint32_t* __restrict__ sad, const int16_t* __restrict__ iscan, QParams qp, int qfast,
    int tx_type, uint32_t nblocks, const uint32_t* __restrict__ xy, uint32_t src_stride, uint32_t pred_stride,
    uint32_t recon_stride) {
    enc4_body<PixT, BD, KEEP>(src, pred, recon, coeff, qcoeff, dqcoeff, eob, sad, iscan, qp, qfast, tx_type, nblocks, xy, src_stride, pred_stride,
                              recon_stride, blockIdx.x);
}

}  // namespace svtdev

// kernel_recon_final.h — svt_hip_recon_final_frame: AV1PerformInverseTransformRecon (EbProductCodingLoop.c:871-1020) over the final
// block list of every superblock, in two stages on one stream.
//
//   recon_bin_kernel        one wave per superblock (as partition_kernel): lanes stride the superblock's final entries, apply the rules
//           of the call (source, block size, plane bounds, transform type), write d_status and, after a wave prefix sum over the
//           reconstructed entries, the running stream offsets; then append one 16-byte work item per (entry, plane) to the list of
//           that plane block's transform size in scratch.  The append is wave-aggregated: per size present in the wave one
//           global_atomic_add by one lane for all of the wave's items of that size, ranks from the ballot.  The blocks of a tiling do
//           not overlap, so list order cannot change the output.
//   recon_final_kernel<CLS> one launch per register class (SVT_TX_CLASS0 / SVT_TX_CLASS1 / 64x64, kernel_txfm_staged.h), class 1 in two
//           halves (without and with a 64-sample side: its nine bodies in one function left 2 392 bytes per lane in scratch, the
//           halves none).  A workgroup reads the counts the bin stage left and strides over the workgroup-sized pieces of its class's lists; a size's body is the
//           per-wave steps of inv_staged_kernel (inv_row_pass, inv_row_store, inv_col_pass, inv_res_write, add_clip) with a new staging:
//           coefficients and prediction from per-item addresses, destination chunks on a plane as the dst_offsets branch writes them.
//
// Mixed transform types in one wave.  A list is ordered by superblock, not by type, and a wave of 64 / max(W, H) blocks can hold several
// types.  The steps take hk / vk as plain ints, so a wave runs a pass once per 1-D kind PRESENT among its blocks (a wave-uniform loop
// over the kinds, skipped when no block has it), each time with the lanes of the other kinds switched off (their lane index is passed as
// 64: every step begins with l < W or l < H).  The kind is then a scalar as in the other kernels, and the ballot of inv1d's clamp-free
// test (kernel_txfm.h) runs inside the step's l < H branch: it counts the active lanes only, all of one kind, so "no active lane exceeds
// the bound of THIS kind" is exactly what it decides; a lane of another kind is neither tested against the wrong bound nor run through
// the wrong network.  A wave of one type (every wave of the sizes with a 32- or 64-sample side: one block per wave, or two) runs each
// pass once.  A block with eob 0 takes no pass at all: its residual row is zero; a wave of such blocks copies the prediction.
//
// An item: word 0 = group | plane << 5 | tx_type << 7 | (eob == 0) << 11, word 1 = the block's index in its group, word 2 = x | y << 16
// on the plane, word 3 = the element offset of its span in d_sb_qcoeff[plane] (0xFFFFFFFF: no copy).
#pragma once
#include "kernel_final_list.h"
#include "kernel_txfm_staged.h"
#include "recon_final_plan.h"

namespace svtdev {

constexpr int RF_SIZES = SVT_TX_SIZES_ALL, RF_GROUPS = svthost::RF_MAX_GROUPS, RF_FINAL = FL_MAX_FINAL;
constexpr uint32_t RF_NO_COPY = 0xFFFFFFFFu;

// the lists' own: per transform size the list's start and capacity per superblock, from the host plan's constexpr functions (the
// geometry is kGeomTab's, kernel_final_list.h)
struct RfListTab { uint16_t list_first[RF_SIZES + 1], cap[RF_SIZES]; };
constexpr RfListTab rf_list_tab() {
    RfListTab T{};
    for (int t = 0; t < RF_SIZES; t++) { T.list_first[t] = (uint16_t)svthost::rf_list_first(t); T.cap[t] = (uint16_t)svthost::rf_cap(t); }
    T.list_first[RF_SIZES] = (uint16_t)svthost::RF_ITEMS_PER_SB;
    return T;
}
static __device__ const RfListTab kReconLists = rf_list_tab();

// vtx_tab / htx_tab as two bits per type
constexpr uint32_t rf_pack_kinds(const uint8_t (&k)[16]) {
    uint32_t v = 0;
    for (int i = 0; i < 16; i++) v |= (uint32_t)k[i] << (2 * i);
    return v;
}
constexpr uint32_t RF_VKINDS = rf_pack_kinds(kVKind), RF_HKINDS = rf_pack_kinds(kHKind);

struct ReconBinGroup { uint32_t src_first, nblocks; uint8_t bsize, tx_type_uv, pad[2]; };
struct ReconBinDesc {
    const uint32_t* final_blk;             // svt_hip_part_final as three words
    const uint32_t* final_count;
    const uint32_t* decision;              // svt_hip_md_decision as eighteen words
    uint8_t* status;
    uint32_t* coeff_offset;
    uint32_t* counters;
    uint4* items;
    uint32_t nsb, nsrc, planes, stream;
    int32_t ngroups;
    uint32_t width[3], height[3];
    ReconBinGroup g[RF_GROUPS];
};
static_assert(sizeof(ReconBinDesc) <= 4000, "kernel arguments");
constexpr int RF_DEC_WORDS = 18, RF_DEC_EOB01 = 11, RF_DEC_EOB2 = 12, RF_DEC_TX_TYPE = 15;      // words of the record

__global__ __launch_bounds__(svthost::RF_BIN_THREADS) void recon_bin_kernel(const ReconBinDesc F) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const uint32_t sb = blockIdx.x * svthost::RF_BIN_WAVES + wave;
    if (sb >= F.nsb) return;                                                // wave-uniform
    const uint32_t count = final_count_of(F.final_count, sb);
    uint32_t run_y = 0, run_uv = 0;                                         // coded_area_sb / coded_area_sb_uv so far
#pragma unroll 1
    for (uint32_t base = 0; base < count; base += 64) {
        const uint32_t k = base + (uint32_t)lane;
        const bool live = k < count;
        FinalEntry e;
        if (live) e = final_entry_load(F.final_blk, sb, k);
        const uint32_t src = e.src;
        uint32_t reason = SVT_HIP_RECON_OK;
        // the source group: scalar compares against the table (the groups cover [0, nsrc))
        uint32_t gi = 0, local = 0, gbsize = 0xffffu, uvtype = 0;
        if (src == SVT_HIP_PART_NO_SRC || src >= F.nsrc) reason = SVT_HIP_RECON_NO_SRC;
#pragma unroll 1
        for (int i = 0; i < F.ngroups; i++) {
            const ReconBinGroup G = F.g[i];
            if (src - G.src_first < G.nblocks) { gi = (uint32_t)i; local = src - G.src_first; gbsize = G.bsize; uvtype = G.tx_type_uv; }
        }
        if (reason == SVT_HIP_RECON_OK && gbsize != e.bsize_byte) reason = SVT_HIP_RECON_BSIZE;
        // the entry's own block size (a matched group's bsize is one the host accepted); chroma inside both chroma planes
        const EntryGeom g = entry_geom(e, reason == SVT_HIP_RECON_OK ? e.bsize_byte : 0u);
        if (reason == SVT_HIP_RECON_OK && !entry_inside(e, g, F.width, F.height, F.planes)) reason = SVT_HIP_RECON_OUTSIDE;
        uint32_t eob01 = 0, eob2 = 0, type = 0;
        if (reason == SVT_HIP_RECON_OK) {
            const uint32_t* d = F.decision + RF_DEC_WORDS * (size_t)src;
            eob01 = d[RF_DEC_EOB01]; eob2 = d[RF_DEC_EOB2] & 0xffffu; type = d[RF_DEC_TX_TYPE] & 0xffu;
            if (!svthost::tx_type_ok_sides(g.bw, g.bh, type)) reason = SVT_HIP_RECON_TX_TYPE;      // the luma size only: the host checked the group's chroma type
        }
        const bool ok = live && reason == SVT_HIP_RECON_OK;
        // the stream offsets advance over the reconstructed entries only
        uint32_t off_y, off_uv;
        stream_offsets(ok ? g.bw * g.bh : 0u, ok && g.has_uv ? g.cw * g.ch : 0u, lane, run_y, run_uv, off_y, off_uv);
        if (live) {
            if (F.status) F.status[(size_t)sb * RF_FINAL + k] = (uint8_t)reason;
            if (F.coeff_offset) { uint32_t* o = F.coeff_offset + 2 * ((size_t)sb * RF_FINAL + k); o[0] = off_y; o[1] = off_uv; }
        }
        // the work items, plane by plane
#pragma unroll 1
        for (uint32_t p = 0; p < F.planes; p++) {
            const bool has = ok && (p == 0 || g.has_uv);
            const uint32_t size = p == 0 ? g.txs : g.txs_uv;
            const uint32_t eob = p == 0 ? (eob01 & 0xffffu) : (p == 1 ? eob01 >> 16 : eob2);
            const uint32_t span = p == 0 ? svthost::kSbLumaSpan : svthost::kSbChromaSpan, off = p == 0 ? off_y : off_uv, area = p == 0 ? g.bw * g.bh : g.cw * g.ch;
            uint4 item;
            item.x = gi | p << 5 | (p == 0 ? type : uvtype) << 7 | (eob == 0 ? 1u : 0u) << 11;
            item.y = local;
            item.z = p == 0 ? (e.x | e.y << 16) : (g.cx | g.cy << 16);
            item.w = F.stream && off + area <= span ? sb * span + off : RF_NO_COPY;
            unsigned long long pend = __ballot(has);
            while (pend) {                                                  // wave-uniform: one round per size present
                const int leader = __ffsll((long long)pend) - 1;
                const uint32_t s = (uint32_t)__builtin_amdgcn_readfirstlane(__shfl((int)size, leader, 64));
                const bool mine = has && size == s;
                const unsigned long long m = __ballot(mine);
                uint32_t at = 0;
                if (lane == leader) at = atomicAdd(F.counters + s, (uint32_t)__popcll(m));
                at = (uint32_t)__shfl((int)at, leader, 64) + (uint32_t)__popcll(m & ((1ull << lane) - 1ull));
                const uint32_t room = (uint32_t)kReconLists.cap[s] * F.nsb;
                if (mine && at < room) F.items[(size_t)kReconLists.list_first[s] * F.nsb + at] = item;
                pend &= ~m;
            }
        }
    }
}

// ---- reconstruct -------------------------------------------------------------------------------------------------------------------
// txs: the transform size of the group's plane blocks, a byte per plane (what an item of plane p must be listed under)
struct ReconFinalGroupDev { const uint8_t* pred[3]; const int32_t* dq[3]; const int32_t* q[3]; uint32_t nblocks, txs; };
struct ReconFinalDesc {
    const uint32_t* counters;
    const uint4* items;
    uint8_t* recon[3];
    int32_t* sbq[3];
    uint32_t stride[3], width[3], height[3];
    uint32_t nsb, ngroups, planes, stream;
    ReconFinalGroupDev g[RF_GROUPS];
};
static_assert(sizeof(ReconFinalDesc) <= 4000, "kernel arguments");

// the counters of the lists: cleared by a launch of the call's own (one wave, vector stores), so that the call is kernels only
__global__ __launch_bounds__(64) void recon_clear_kernel(uint32_t* counters) {
    if (threadIdx.x < svthost::RF_COUNTER_BYTES / 4) counters[threadIdx.x] = 0;
}

// LDS of a size's body per wave (inv_staged_kernel's: coefficient tile, transpose tile, residual tile share it) and of a class
template <int W, int H>
struct RfLds {
    using S = StagedGeom<W, H>;
    using G = TxGeom<W, H>;
    static constexpr bool T16 = W >= 64 || H >= 64;      // as launch_inv_staged (svt_hip_txfm.hip)
    static constexpr int IN_BYTES = G::BPW * S::KH * S::KW * 4;
    static constexpr int TILE_BYTES = T16 ? G::BPW * H * S::P16 * 2 : G::BPW * G::TILE * 4;
    static constexpr int RES_BYTES = G::BPW * (W * H + ResPad<W>::N) * 2;
    static constexpr int WAVE = (cmax(cmax(IN_BYTES, TILE_BYTES), RES_BYTES) + 15) & ~15;
};
#define SVT_RF_LDS(N, W, H) RfLds<W, H>::WAVE,
template <int CLS> struct RfClass;
template <> struct RfClass<0> { static constexpr int WAVES = 4, WAVE_LDS = cmax_of({SVT_TX_CLASS0(SVT_RF_LDS, SVT_RF_LDS)}); };
template <> struct RfClass<1> { static constexpr int WAVES = 4, WAVE_LDS = cmax_of({SVT_TX_CLASS1A(SVT_RF_LDS, SVT_RF_LDS)}); };
template <> struct RfClass<2> { static constexpr int WAVES = 4, WAVE_LDS = cmax_of({SVT_TX_CLASS1B(SVT_RF_LDS, SVT_RF_LDS)}); };
template <> struct RfClass<3> { static constexpr int WAVES = 2, WAVE_LDS = RfLds<64, 64>::WAVE; };
#undef SVT_RF_LDS

__device__ __forceinline__ const ReconFinalGroupDev& rf_group(const ReconFinalDesc& D, uint32_t item0) { return D.g[item0 & 31u]; }
template <typename T>
__device__ __forceinline__ T rf_pick(T a, T b, T c, uint32_t p) { return p == 0 ? a : (p == 1 ? b : c); }

// An item is device memory like any other: it is checked before it forms an address, and one that fails is left out as if the list
// ended before it.  It passes when it names a group of the call, a block of that group, a requested plane whose blocks are listed under
// this size, a block wholly inside that plane, and a span inside the stream (or none).  Every item the bin stage writes passes.
template <int N, int W, int H>
__device__ __forceinline__ bool rf_item_ok(const ReconFinalDesc& D, const uint4& ib) {
    const uint32_t gi = ib.x & 31u, p = (ib.x >> 5) & 3u;             // (gi indexes inside g[] whatever the word holds)
    const ReconFinalGroupDev& G = rf_group(D, ib.x);
    const uint32_t nblocks = G.nblocks, tx = (G.txs >> (8 * p)) & 0xffu, pc = min(p, 2u);
    const uint32_t x = ib.z & 0xffffu, y = ib.z >> 16;
    const unsigned long long room = (unsigned long long)D.nsb * (p == 0 ? svthost::kSbLumaSpan : svthost::kSbChromaSpan);
    const bool span_ok = ib.w == RF_NO_COPY || (D.stream != 0 && (unsigned long long)ib.w + StagedGeom<W, H>::NC <= room);
    return gi < D.ngroups && p < D.planes && ib.y < nblocks && tx == (uint32_t)N && x + W <= D.width[pc] && y + H <= D.height[pc] && span_ok;
}

// The pieces [piece * WAVES * BPW, ...) of the list of transform size N: wave `wave` takes BPW items.  wl: the wave's LDS.
template <int N, int W, int H, int WAVES>
__device__ __forceinline__ void recon_final_body(const ReconFinalDesc& D, uint32_t count, uint32_t piece, char* wl, int lane, int wave) {
    using S = StagedGeom<W, H>;
    using G = TxGeom<W, H>;
    using I = StagedIn<W, H, 1>;
    constexpr bool T16 = RfLds<W, H>::T16;
    constexpr int KW = S::KW, KH = S::KH, NC = S::NC, RPAD = ResPad<W>::N, OFF = 64;      // OFF: a lane index no step works on
    static_assert(S::WAVES == WAVES, "a class's sizes share the workgroup shape");
    const uint32_t first = (piece * WAVES + (uint32_t)wave) * G::BPW;
    if (first >= count) return;                                             // wave-uniform
    const uint4* items = D.items + (size_t)kReconLists.list_first[N] * D.nsb;
    const int sub = lane / G::LPB, l = lane % G::LPB;
    bool valid = first + sub < count;
    uint32_t it0 = 1u << 11;
    if (valid) {
        const uint4 mine = items[first + sub];
        valid = rf_item_ok<N, W, H>(D, mine);
        if (valid) it0 = mine.x;
    }
    const bool act = valid && !((it0 >> 11) & 1u);                          // the block has coefficients
    const uint32_t type = (it0 >> 7) & 15u;
    const int vk = act ? (int)((RF_VKINDS >> (2 * type)) & 3u) : K1D_DCT, hk = act ? (int)((RF_HKINDS >> (2 * type)) & 3u) : K1D_DCT;
    const bool any = __ballot(act) != 0;
    constexpr int CPB = NC / 4, NCH = G::BPW * CPB;
    // ---- the coefficient tile (zeros for a block with eob 0: its array is not read) and the stream copy ----
    if (any || D.sbq[0]) {
#pragma unroll
        for (int q0 = 0; q0 < NCH; q0 += 64) {
            const int q = q0 + lane;
            if (NCH % 64 == 0 || q < NCH) {
                const int b = q / CPB, w4 = q % CPB;
                int4 v = make_int4(0, 0, 0, 0), qv = v;
                uint32_t span = RF_NO_COPY, p = 0;
                uint4 ib = make_uint4(0, 0, 0, 0);
                bool ok = first + b < count;
                if (ok) { ib = items[first + b]; ok = rf_item_ok<N, W, H>(D, ib); }
                if (ok) {
                    const ReconFinalGroupDev& Gd = rf_group(D, ib.x);
                    p = (ib.x >> 5) & 3u;
                    if (D.sbq[0]) span = ib.w;
                    if (!((ib.x >> 11) & 1u)) {
                        v = reinterpret_cast<const int4*>(rf_pick(Gd.dq[0], Gd.dq[1], Gd.dq[2], p) + (size_t)ib.y * NC)[w4];
                        if (span != RF_NO_COPY) qv = reinterpret_cast<const int4*>(rf_pick(Gd.q[0], Gd.q[1], Gd.q[2], p) + (size_t)ib.y * NC)[w4];
                    }
                }
                if (span != RF_NO_COPY) reinterpret_cast<int4*>(rf_pick(D.sbq[0], D.sbq[1], D.sbq[2], p) + (size_t)span)[w4] = qv;
                if (any) *reinterpret_cast<int4*>(wl + coef_tile_addr<KW, KH>(b, w4 / (KW / 4), w4 % (KW / 4))) = v;
            }
        }
    }
    if (any) {
        wave_lds_fence();
        {
            int x[W];
#pragma unroll 1
            for (int k = 0; k < 4; k++) {                                   // the row kinds present
                const bool mine = act && hk == k;
                if (__ballot(mine) == 0) continue;
                inv_row_pass<W, H>(wl, sub, mine ? l : OFF, k, 8, x);
            }
            wave_lds_fence();
            inv_row_store<W, H, T16>(wl, sub, act ? l : OFF, x);
        }
        wave_lds_fence();
        int y[H];
#pragma unroll
        for (int r = 0; r < H; r++) y[r] = 0;                               // a block without coefficients: a zero residual
#pragma unroll 1
        for (int k = 0; k < 8; k++) {                                       // the column kinds present, with the row kind's flip or without
            const bool mine = act && vk == (k >> 1) && (hk == K1D_FLIPADST) == ((k & 1) != 0);
            if (__ballot(mine) == 0) continue;
            inv_col_pass<W, H, T16>(wl, sub, mine ? l : OFF, k >> 1, (k & 1) ? K1D_FLIPADST : K1D_DCT, 8, y);
        }
        wave_lds_fence();
#pragma unroll 1
        for (int k = 0; k < 2; k++) {                                       // upside down or not
            const bool mine = valid && (vk == K1D_FLIPADST) == (k != 0);
            if (__ballot(mine) == 0) continue;
            inv_res_write<W, H>(wl, sub, mine ? l : OFF, k ? K1D_FLIPADST : K1D_DCT, y);
        }
        wave_lds_fence();
    }
    // ---- prediction chunks (dense blocks) + residual -> destination chunks on the plane ----
    const short* res = reinterpret_cast<const short*>(wl);
    constexpr int NIT = I::NIT, CPBP = I::CPBP;
    uint4 pv[NIT];
    uint8_t* dp[NIT];
    bool okc[NIT];
#pragma unroll
    for (int it = 0; it < NIT; it++) {
        const int q = it * 64 + lane, b = q / CPBP, w = q % CPBP;
        okc[it] = (I::NCHP % 64 == 0 || q < I::NCHP) && first + b < count;
        pv[it] = make_uint4(0, 0, 0, 0);
        dp[it] = nullptr;
        uint4 ib = make_uint4(0, 0, 0, 0);
        if (okc[it]) { ib = items[first + b]; okc[it] = rf_item_ok<N, W, H>(D, ib); }
        if (okc[it]) {
            const ReconFinalGroupDev& Gd = rf_group(D, ib.x);
            const uint32_t p = (ib.x >> 5) & 3u;
            __builtin_memcpy(&pv[it], rf_pick(Gd.pred[0], Gd.pred[1], Gd.pred[2], p) + (size_t)ib.y * (W * H) + (size_t)w * I::CS, I::CS);
            dp[it] = rf_pick(D.recon[0], D.recon[1], D.recon[2], p) + ((size_t)(ib.z >> 16) + w / I::CPR) * rf_pick(D.stride[0], D.stride[1], D.stride[2], p) +
                     (ib.z & 0xffffu) + (w % I::CPR) * I::PPC;
        }
    }
#pragma unroll
    for (int it = 0; it < NIT; it++) {
        const int q = it * 64 + lane;
        if (okc[it]) {
            const uint4 o = any ? add_clip<uint8_t, I::CS>(pv[it], res + (size_t)q * I::PPC + (q / CPBP) * RPAD, 255) : pv[it];
            __builtin_memcpy(dp[it], &o, I::CS);
        }
    }
    wave_lds_fence();                                                       // the residual tile is dead: the wave's next piece may overwrite it
}

// items of a size the reconstruct stage takes: what the bin stage counted, at most the list's room
template <int N>
__device__ __forceinline__ uint32_t rf_count(const ReconFinalDesc& D) { return min(D.counters[N], (uint32_t)svthost::rf_cap(N) * D.nsb); }

template <int CLS>
__global__ __launch_bounds__(RfClass<CLS>::WAVES * 64) void recon_final_kernel(const ReconFinalDesc in_kernarg) {
    // The descriptor is read where it lies, in the kernel argument segment (it is the only argument: offset 0).  Read through the
    // by-value parameter, its table of groups, indexed per lane from many bodies, was copied to scratch: 2 688 bytes per lane in the
    // launches with five and nine bodies.
    (void)in_kernarg;
    const ReconFinalDesc& D = *(const ReconFinalDesc*)__builtin_amdgcn_kernarg_segment_ptr();
    constexpr int WAVES = RfClass<CLS>::WAVES;
    __shared__ __attribute__((aligned(16))) char lds[WAVES * RfClass<CLS>::WAVE_LDS];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    char* wl = lds + wave * RfClass<CLS>::WAVE_LDS;                         // one region per wave for every size: the waves do not meet
    // the pieces of the class's lists are numbered through; workgroup w takes the pieces w, w + gridDim.x, ...
    uint32_t before = 0;
#define SVT_RF_SIZE(N, W, H)                                                                                              \
    {                                                                                                                     \
        const uint32_t count = rf_count<N>(D), per = WAVES * TxGeom<W, H>::BPW, pieces = (count + per - 1) / per;        \
        const uint32_t skip = (blockIdx.x + gridDim.x - before % gridDim.x) % gridDim.x;                                  \
        _Pragma("unroll 1") for (uint32_t piece = skip; piece < pieces; piece += gridDim.x)                               \
            recon_final_body<N, W, H, WAVES>(D, count, piece, wl, lane, wave);                                            \
        before += pieces;                                                                                                 \
    }
    if constexpr (CLS == 0) { SVT_TX_CLASS0(SVT_RF_SIZE, SVT_RF_SIZE) }
    else if constexpr (CLS == 1) { SVT_TX_CLASS1A(SVT_RF_SIZE, SVT_RF_SIZE) }
    else if constexpr (CLS == 2) { SVT_TX_CLASS1B(SVT_RF_SIZE, SVT_RF_SIZE) }
    else { SVT_RF_SIZE(4, 64, 64) }
#undef SVT_RF_SIZE
}

}  // namespace svtdev

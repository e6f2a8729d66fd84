// kernel_inter_fast_pick.h — inter_pick_kernel: the end of the fast loop for the combined list of a P / B picture (ninter inter
// candidates, then nintra intra candidates).  Per block: av1_inter_fast_cost (EbRateDistortionCost.c:971-1318, with
// EstimateRefFramesNumBits :741-947 and Av1ModeContextAnalyzer :951-969) of every inter candidate, the intra candidates' costs as given,
// the buffer walk and the sorted array (fast_walk, fast_sorted: kernel_fast_walk.h, which also states the mapping of a block to a
// wave), the inter-before-intra pass of sort_fast_loop_candidates (EbModeDecision.c:458-469), and the survivors' records.  It reads
// what inter_pred_kernel writes (dist) and writes what it reads (blk).  The 383 words of rate tables are staged in LDS; the MV cost
// table (2 x 32767 words) stays in global memory: a candidate reads at most four of its words.  What is this kernel's own:
//   cost     lane = candidate of the combined list.  Inter lanes: the two 16-byte records, the rates out of the LDS tables (every
//            context byte clamped first), cost, luma rate -> the wave's LDS rows.  Intra lanes: d_intra_cost / d_intra_rate.
//   order    positions 0 .. n-1 of best_candidate_index_array are the held buffers in buffer order.  The :458-469 pass is, with M the
//            set of positions that hold an inter entry, K = |M| and p_k the k-th member of M: for k = 0 .. K-1 in order, exchange
//            positions k and p_k (DESIGN.md 4.34 derives it).  So destination d < K takes the entry of p_d; d >= K outside M keeps its
//            entry; d >= K in M takes the entry found by following m -> |M below m| from d until m leaves M.  A lane follows its own
//            chain on the 64-bit mask alone (no cross-lane traffic, at most n short steps); the inverse map goes through one LDS row.
//            The sorted array is bubble-swapped on BUFFER costs and does not see the pass.
#pragma once
#include "kernel_fast_walk.h"

namespace svtdev {

constexpr int IFP_MV_MAX = 16383, IFP_MV_VALS = 2 * IFP_MV_MAX + 1;
// svt_hip_inter_fast_rates as words
constexpr int IFP_SKIP = 0, IFP_NEWMV = IFP_SKIP + 3 * 3, IFP_ZEROMV = IFP_NEWMV + 6 * 3, IFP_REFMV = IFP_ZEROMV + 2 * 3,
              IFP_DRL = IFP_REFMV + 6 * 3, IFP_COMPMODE = IFP_DRL + 3 * 3, IFP_SINGLE = IFP_COMPMODE + 8 * 9, IFP_CRT = IFP_SINGLE + 3 * 6 * 3,
              IFP_CREF = IFP_CRT + 5 * 3, IFP_CBWD = IFP_CREF + 3 * 3 * 3, IFP_CINTER = IFP_CBWD + 3 * 2 * 3, IFP_MM = IFP_CINTER + 5 * 3,
              IFP_MM1 = IFP_MM + 22 * 3, IFP_II = IFP_MM1 + 22 * 2, IFP_JOINT = IFP_II + 4 * 2, IFP_RATE_WORDS = IFP_JOINT + 4;

// a 16-byte record at a 4-byte-aligned address, as one access
typedef unsigned ifp_rec __attribute__((ext_vector_type(4), aligned(4)));

// ref_frame_map (EbAdaptiveMotionVectorPrediction.c:214-233): rf[0] | rf[1] << 4 of ref_frame_type 8 .. 28
static __device__ const uint8_t kIfpRefFrameMap[21] = {0x51, 0x52, 0x53, 0x54, 0x61, 0x62, 0x63, 0x64, 0x71, 0x72, 0x73,
                                                       0x74, 0x21, 0x31, 0x41, 0x75, 0x32, 0x42, 0x43, 0x65, 0x76};
// compound_mode_ctx_map_2 (EbRateDistortionCost.c:951-955), three bits an entry
constexpr uint32_t kIfpCompCtxMap[3] = {0 | 1 << 3 | 1 << 6 | 1 << 9 | 1 << 12, 1 | 2 << 3 | 3 << 6 | 4 << 9 | 4 << 12, 4 | 4 << 3 | 5 << 6 | 6 << 9 | 7 << 12};

struct InterFastPickDev {
    const uint32_t* blk;                                   // [nblocks][ninter] svt_hip_inter_blk, four words each
    const uint32_t* cand_in;                               // [nblocks][ninter] svt_hip_inter_cand, four words each
    const uint32_t* ctx;                                   // [nblocks] svt_hip_inter_fast_blk, four words each
    const int32_t* rates;                                  // svt_hip_inter_fast_rates
    const int32_t* mv_cost;                                // [2][IFP_MV_VALS]
    const unsigned long long* dist; const unsigned long long* dist_cb; const unsigned long long* dist_cr;      // [nblocks][ninter]
    const unsigned long long* intra_cost;                  // [nblocks][nintra]
    const uint32_t* intra_rate;                            // optional [nblocks][nintra][2]
    uint8_t* cand_out; uint8_t* sorted;                    // [nblocks][n]
    unsigned long long* cost;                              // [nblocks][n]
    uint32_t* rate;                                        // [nblocks][n][2]
    unsigned long long* ref_fast_cost;                     // [nblocks]
    unsigned long long* all_cost;                          // optional [nblocks][ninter]
    uint32_t* blk_out;                                     // [nblocks][n] records
    uint32_t* cand_rec_out;                                // optional [nblocks][n] records
    uint32_t* src_xy_out;                                  // optional [nblocks][n]
    uint32_t nblocks, lambda, qstep;
    uint8_t ninter, nintra, n, nbuf, ssd, bsize, nlog2_y, nlog2_uv;
    uint8_t comp_inter;                                    // reference_mode_select && min(bw, bh) >= 8
    uint8_t switchable_motion_mode;
    uint8_t bpw;                                           // blocks per wave, 1 .. FW_MAX_BPW
};

// av1_mv_bit_cost (:91-95) with MV_COST_WEIGHT 108; the differences clamped to the table
__device__ __forceinline__ uint32_t ifp_mv_bits(const int32_t* mv_cost, const int32_t* s_rates, int mvx, int mvy, int px, int py) {
    const int row = max(-IFP_MV_MAX, min(IFP_MV_MAX, mvy - py)), col = max(-IFP_MV_MAX, min(IFP_MV_MAX, mvx - px));
    const int joint = (row != 0 ? 2 : 0) | (col != 0 ? 1 : 0);
    const int32_t c = s_rates[IFP_JOINT + joint] + mv_cost[IFP_MV_MAX + row] + mv_cost[IFP_MV_VALS + IFP_MV_MAX + col];
    return (uint32_t)((c * 108 + 64) >> 7);
}

__global__ __launch_bounds__(FW_THREADS) void inter_pick_kernel(const InterFastPickDev F) {
    __shared__ int32_t s_rates[IFP_RATE_WORDS];
    __shared__ unsigned long long s_cost[FW_WAVES][64];
    __shared__ uint32_t s_lr[FW_WAVES][64], s_cr[FW_WAVES][64];
    __shared__ uint8_t s_dest[FW_WAVES][64];
    for (int i = threadIdx.x; i < IFP_RATE_WORDS; i += FW_THREADS) s_rates[i] = F.rates[i];
    __syncthreads();
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int ninter = F.ninter, ncand = F.ninter + F.nintra, n = F.n, nbuf = F.nbuf;

#pragma unroll 1
    for (int j = 0; j < F.bpw; j++) {
        const uint32_t blk = (blockIdx.x * FW_WAVES + (uint32_t)wave) * F.bpw + (uint32_t)j;
        if (blk >= F.nblocks) break;                                             // wave-uniform
        wave_lds_fence();                                                        // the previous block's LDS reads before these writes
        // ---- cost: lane = candidate ----
        const ifp_rec cx = reinterpret_cast<const ifp_rec*>(F.ctx)[blk];
        const uint32_t skip_ctx = min(cx.x & 0xffu, 2u), inter_ctx = min((cx.x >> 8) & 0xffu, 3u);
        unsigned long long cost = ~0ull;
        uint32_t lr = 0, cr = 0;
        if (lane < ninter) {
            const size_t at = (size_t)blk * ninter + lane;
            const uint32_t* bw = F.blk + at * 4;
            const uint32_t* cw = F.cand_in + at * 4;
            const uint32_t b1 = bw[1], b2 = bw[2], b3 = bw[3], c0 = cw[0], c1 = cw[1], c2 = cw[2], c3 = cw[3];
            const int mvx0 = (int16_t)(b1 & 0xffff), mvy0 = (int16_t)(b1 >> 16), mvx1 = (int16_t)(b2 & 0xffff), mvy1 = (int16_t)(b2 >> 16);
            const int px0 = (int16_t)(c0 & 0xffff), py0 = (int16_t)(c0 >> 16), px1 = (int16_t)(c1 & 0xffff), py1 = (int16_t)(c1 >> 16);
            const uint32_t dir = b3 & 0xff;
            const bool comp = dir == 2;                                          // is_compound
            const uint32_t mc = (uint32_t)(int32_t)(int16_t)(c2 & 0xffff);        // inter_mode_ctx[ref_frame_type], int16 -> uint32
            const int mode = (int)max(13u, min(24u, (c2 >> 16) & 0xffu));
            const int rft = (int)max(1u, min(28u, c2 >> 24));
            const int drl_index = (int)(c3 & 0xff), ref_mv_count = (int)((c3 >> 8) & 0xff);
            const uint32_t drl_ctx = (c3 >> 16) & 0xff, flags = c3 >> 24;
            // av1_set_ref_frame; rf1 = -1 is NONE_FRAME
            int rf0 = rft, rf1 = -1;
            if (rft >= 8) { const uint32_t e = kIfpRefFrameMap[rft - 8]; rf0 = (int)(e & 15u); rf1 = (int)(e >> 4); }
            // EstimateRefFramesNumBits
            uint32_t bits = 0;
            if (F.comp_inter) bits += (uint32_t)s_rates[IFP_CINTER + min((cx.x >> 16) & 0xffu, 4u) * 3 + (comp ? 1 : 0)];
            if (comp) {
                bits += (uint32_t)s_rates[IFP_CRT + min(cx.x >> 24, 4u) * 3 + 1];                     // BIDIR_COMP_REFERENCE
                const int bit = rf0 == 4 || rf0 == 3;
                bits += (uint32_t)s_rates[IFP_CREF + (min(cx.y & 0xffu, 2u) * 3 + 0) * 3 + bit];
                if (!bit) bits += (uint32_t)s_rates[IFP_CREF + (min((cx.y >> 8) & 0xffu, 2u) * 3 + 1) * 3 + (rf0 == 2)];
                else bits += (uint32_t)s_rates[IFP_CREF + (min((cx.y >> 16) & 0xffu, 2u) * 3 + 2) * 3 + (rf0 == 4)];
                const int bit_bwd = rf1 == 7;
                bits += (uint32_t)s_rates[IFP_CBWD + (min(cx.y >> 24, 2u) * 2 + 0) * 3 + bit_bwd];
                if (!bit_bwd) bits += (uint32_t)s_rates[IFP_CBWD + (min(cx.z & 0xffu, 2u) * 2 + 1) * 3 + (rf1 == 6)];
            } else {
                const uint32_t p1 = min((cx.z >> 8) & 0xffu, 2u), p2 = min((cx.z >> 16) & 0xffu, 2u), p3 = min(cx.z >> 24, 2u);
                const uint32_t p4 = min(cx.w & 0xffu, 2u), p5 = min((cx.w >> 8) & 0xffu, 2u), p6 = min((cx.w >> 16) & 0xffu, 2u);
                const int bit0 = rft <= 7 && rft >= 5;
                bits += (uint32_t)s_rates[IFP_SINGLE + (p1 * 6 + 0) * 3 + bit0];
                if (bit0) {
                    const int bit1 = rft == 7;
                    bits += (uint32_t)s_rates[IFP_SINGLE + (p2 * 6 + 1) * 3 + bit1];
                    if (!bit1) bits += (uint32_t)s_rates[IFP_SINGLE + (p6 * 6 + 5) * 3 + (rft == 6)];
                } else {
                    const int bit2 = rft == 3 || rft == 4;
                    bits += (uint32_t)s_rates[IFP_SINGLE + (p3 * 6 + 2) * 3 + bit2];
                    if (!bit2) bits += (uint32_t)s_rates[IFP_SINGLE + (p4 * 6 + 3) * 3 + (rft != 1)];
                    else bits += (uint32_t)s_rates[IFP_SINGLE + (p5 * 6 + 4) * 3 + (rft != 3)];
                }
            }
            // Av1ModeContextAnalyzer
            uint32_t mode_ctx = mc;
            if (rf1 > 0) {
                const uint32_t newmv = mc & 7u, refmv = (mc >> 4) & 15u;
                mode_ctx = (kIfpCompCtxMap[min(refmv >> 1, 2u)] >> (3 * min(newmv, 4u))) & 7u;
            }
            // the mode bits
            if (comp) {
                bits += (uint32_t)s_rates[IFP_COMPMODE + min(mode_ctx, 7u) * 9 + min((uint32_t)(uint8_t)(mode - 17), 7u)];
            } else {
                bits += (uint32_t)s_rates[IFP_NEWMV + min(mode_ctx & 7u, 5u) * 3 + (mode != 16)];
                if (mode != 16) {
                    bits += (uint32_t)s_rates[IFP_ZEROMV + ((mode_ctx >> 3) & 1u) * 3 + (mode != 15)];
                    if (mode != 15) bits += (uint32_t)s_rates[IFP_REFMV + min((mode_ctx >> 4) & 15u, 5u) * 3 + (mode != 13)];
                }
            }
            // the DRL bits: have_nearmv_in_inter_mode = NEARMV, NEAR_NEARMV, NEAR_NEWMV, NEW_NEARMV
            const bool new_mv = mode == 16 || mode == 24, near_mv = mode == 14 || mode == 18 || mode == 21 || mode == 22;
            if (new_mv) {
#pragma unroll
                for (int idx = 0; idx < 2; idx++) {
                    if (ref_mv_count > idx + 1) {
                        bits += (uint32_t)s_rates[IFP_DRL + min((drl_ctx >> (2 * idx)) & 3u, 2u) * 3 + (drl_index != idx)];
                        if (drl_index == idx) break;
                    }
                }
            }
            if (near_mv) {
#pragma unroll
                for (int idx = 1; idx < 3; idx++) {
                    if (ref_mv_count > idx + 1) {
                        bits += (uint32_t)s_rates[IFP_DRL + min((drl_ctx >> (2 * idx)) & 3u, 2u) * 3 + (drl_index != idx - 1)];
                        if (drl_index == idx - 1) break;
                    }
                }
            }
            // the MV rate: have_newmv_in_inter_mode = NEWMV, NEAREST_NEWMV, NEW_NEARESTMV, NEAR_NEWMV, NEW_NEARMV, NEW_NEWMV
            if (mode == 16 || mode == 19 || mode == 20 || mode == 21 || mode == 22 || mode == 24) {
                bool l0, l1;
                if (comp) { l0 = mode != 19 && mode != 21; l1 = mode == 24 || !l0; }
                else { l0 = dir == 0; l1 = !l0; }
                if (l0) bits += ifp_mv_bits(F.mv_cost, s_rates, mvx0, mvy0, px0, py0);
                if (l1) bits += ifp_mv_bits(F.mv_cost, s_rates, mvx1, mvy1, px1, py1);
            }
            // the motion-mode bits (rf[1] is never INTRA_FRAME)
            if (mode <= 16 && F.switchable_motion_mode) {
                const uint32_t allowed = (flags >> 3) & 3u, mm = (flags >> 1) & 3u;
                if (allowed == 1) bits += (uint32_t)s_rates[IFP_MM1 + F.bsize * 2 + min(mm, 1u)];
                else if (allowed != 0) bits += (uint32_t)s_rates[IFP_MM + F.bsize * 3 + min(mm, 2u)];
            }
            lr = bits + (uint32_t)s_rates[IFP_SKIP + skip_ctx * 3] + (uint32_t)s_rates[IFP_II + inter_ctx * 2 + 1];
            const unsigned long long luma = F.dist[at];
            unsigned long long chroma = 0;
            if (F.dist_cb) chroma += F.dist_cb[at];
            if (F.dist_cr) chroma += F.dist_cr[at];
            uint32_t rate;
            unsigned long long d;
            fast_cost_tail(F.ssd, luma, chroma, lr, 0u, F.nlog2_y, F.nlog2_uv, F.qstep, rate, d);
            unsigned long long r64 = rate;
            if (flags & 1u) {                                                    // merge_flag
                const unsigned long long skip1 = (unsigned long long)(long long)s_rates[IFP_SKIP + skip_ctx * 3 + 1];
                if (skip1 < r64) r64 = skip1;
            }
            cost = ((r64 * F.lambda + 256ull) >> 9) + d * 128ull;
            if (F.all_cost) F.all_cost[at] = cost;
        } else if (lane < ncand) {
            const size_t at = (size_t)blk * F.nintra + (size_t)(lane - ninter);
            cost = F.intra_cost[at];
            if (F.intra_rate) { lr = F.intra_rate[2 * at]; cr = F.intra_rate[2 * at + 1]; }
        }
        s_cost[wave][lane] = cost; s_lr[wave][lane] = lr; s_cr[wave][lane] = cr; s_dest[wave][lane] = (uint8_t)lane;
        wave_lds_fence();
        // ---- walk: lane = buffer ----
        const FastWalk w = fast_walk(s_cost[wave], cost, ncand, n, nbuf, lane, F.ref_fast_cost + blk);
        const bool held = w.held;
        const int bcand = w.bcand, empty = w.empty;
        const int pos = lane - (lane > empty ? 1 : 0);                           // best_candidate_index_array: the empty buffer goes last
        // ---- order: the inter-before-intra pass over positions 0 .. n-1 ----
        const unsigned long long inter_lanes = __ballot(held && bcand < ninter);
        // the mask by position: the emptied buffer's bit (clear) taken out
        const unsigned long long M = empty < 64 ? ((inter_lanes & ((1ull << empty) - 1ull)) | ((inter_lanes >> (empty + 1)) << empty)) : inter_lanes;
        const int K = __popcll(M);
        // lane = destination d: where its entry comes from, for the destinations from K up (an inter entry's own destination is its rank)
        if (lane >= K && lane < n) {
            int m = lane;
            while ((M >> m) & 1ull) m = __popcll(M & ((1ull << m) - 1ull));
            s_dest[wave][m] = (uint8_t)lane;
        }
        wave_lds_fence();
        int slot = pos;
        if (held) slot = bcand < ninter ? __popcll(M & ((1ull << pos) - 1ull)) : s_dest[wave][pos];
        const int sval = fast_sorted(w.brank, n, lane);
        const size_t row = (size_t)blk * n;
        const uint32_t xy = F.blk[(size_t)blk * ninter * 4];                      // x | y << 16 of the block's first record
        if (held && slot < n) {
            const size_t o = row + slot;
            F.cand_out[o] = (uint8_t)bcand;
            F.cost[o] = w.bcost;
            F.rate[2 * o] = s_lr[wave][bcand];
            F.rate[2 * o + 1] = s_cr[wave][bcand];
            ifp_rec rec = {xy, 0u, 0u, 0u}, crec = {0u, 0u, 0u, 0u};             // an intra slot: zero vectors, list 0, filter 0
            if (bcand < ninter) {
                rec = reinterpret_cast<const ifp_rec*>(F.blk)[(size_t)blk * ninter + bcand];
                crec = reinterpret_cast<const ifp_rec*>(F.cand_in)[(size_t)blk * ninter + bcand];
            }
            reinterpret_cast<ifp_rec*>(F.blk_out)[o] = rec;
            if (F.cand_rec_out) reinterpret_cast<ifp_rec*>(F.cand_rec_out)[o] = crec;
        }
        if (lane < n) {
            F.sorted[row + lane] = (uint8_t)sval;
            if (F.src_xy_out) F.src_xy_out[row + lane] = xy;
        }
    }
}

// the intra survivors' luma predictions into the one-call search's prediction array: one workgroup per (block, slot), 16 bytes a lane
struct InterFastGatherDev {
    const uint8_t* cand;                                   // [nblocks][n]
    const uint4* intra_pred;                               // [nblocks][nintra][quads]
    uint4* pred_out;                                       // [nblocks][n][quads]
    uint32_t n, ninter, nintra, quads;
};
__global__ __launch_bounds__(64) void inter_fast_gather_kernel(const InterFastGatherDev F) {
    const uint32_t blk = blockIdx.x / F.n;
    const uint32_t c = F.cand[blockIdx.x];
    if (c < F.ninter || c - F.ninter >= F.nintra) return;                        // workgroup-uniform
    const uint4* in = F.intra_pred + ((size_t)blk * F.nintra + (c - F.ninter)) * F.quads;
    uint4* out = F.pred_out + (size_t)blockIdx.x * F.quads;
    for (uint32_t q = threadIdx.x; q < F.quads; q += 64) out[q] = in[q];
}

}  // namespace svtdev

// kernel_fast_walk.h — what the two kernels that end the fast loop share: fast_pick_kernel (kernel_fast_pick.h, an all-intra list) and
// inter_pick_kernel (kernel_inter_fast_pick.h, inter + intra).  Their geometry, the tail of the fast cost, and the buffer walk of
// perform_fast_loop (EbProductCodingLoop.c:1225-1363) with sort_fast_loop_candidates (EbModeDecision.c:436-489) for one block on one
// wave: fast_walk, then fast_sorted.  Functions only, no __global__: both translation units include it.
//
// Both kernels: one wave per block, bpw blocks per wave one after the other (1 .. FW_MAX_BPW: the host grows it once the group has more
// blocks than the device holds waves, md_plan.h's pick_bpw), FW_WAVES waves per workgroup, the rate tables staged in LDS once per
// workgroup (the only workgroup barrier), the phases of a block fenced per wave.  The caller's cost phase (lane = candidate) leaves the
// block's costs in the wave's LDS row, ~0 in the lanes from ncand up.  Then fast_walk (rank, walk, ref) and fast_sorted (order):
//   rank     lane = candidate.  The number of the block's costs below its own (ncand broadcast reads).  Equal costs share a rank, so
//            every later comparison of two costs is the comparison of two 7-bit ranks; 127 = MAX_CU_COST, an empty buffer.
//   walk     lane = buffer.  The reference's re-scan (strict >, stops at the first buffer at MAX_CU_COST) returns the first empty
//            buffer, else the first buffer holding the maximum.  So the last nbuf list entries fill the buffers in order (one
//            ds_bpermute), and from then on the set of ranks held is a 64-bit mask on the scalar unit: its top bit is the largest rank,
//            one ballot gives the lanes that hold it, the first of them is the buffer to overwrite, and the bit is cleared when that
//            lane was the only one.  ncand - nbuf steps of a ballot, a v_readlane and a handful of SALU instructions.  With a scratch
//            buffer (nbuf == n + 1) the first buffer of the largest rank is emptied at the end (:1361).
//   ref      ref_fast_cost: the minimum over buffers 0 .. n-1 BY BUFFER INDEX (the emptied one counts as MAX_CU_COST), not the true
//            minimum of the survivors.
//   order    sort_fast_loop_candidates' bubble pass i swaps position i with every j > i whose BUFFER cost is below buffer i's, in
//            ascending j: a rotation of the entries at {i} + J, one ballot and one ds_bpermute per i.
#pragma once
#include "dev_common.h"
#include "model_rd.h"

namespace svtdev {

constexpr int FW_THREADS = 256, FW_WAVES = FW_THREADS / 64;
constexpr int FW_MAX_BPW = 4;                              // blocks per wave, at most
constexpr int FW_EMPTY = 127;                              // the rank of MAX_CU_COST
constexpr unsigned long long FW_MAX_CU_COST = ~0ull >> 1, FW_MAX_MODE_COST = 13616969489728ull * 8ull;

// The tail of av1_intra_fast_cost / av1_inter_fast_cost: rate and distortion of a candidate from its luma and chroma rates and
// distortions.  Under SSD both distortions go through model_rd and the model's chroma rate replaces chromaRate
// (EbRateDistortionCost.c:704-710).
__device__ __forceinline__ void fast_cost_tail(bool ssd, unsigned long long luma, unsigned long long chroma, uint32_t lr, uint32_t cr, uint32_t nlog2_y,
                                               uint32_t nlog2_uv, uint32_t qstep, uint32_t& rate, unsigned long long& d) {
    rate = lr + cr;
    d = luma + chroma;
    if (ssd) {
        uint32_t r1, r2;
        unsigned long long d1, d2;
        fp_model_rd(luma, nlog2_y, qstep, r1, d1);
        fp_model_rd(chroma, nlog2_uv, qstep, r2, d2);
        rate = lr + r1 + r2;
        d = d1 + d2;
    }
}

struct FastWalk {                                          // lane = buffer
    int bcand, brank;                                      // the list position and the rank it holds; FW_EMPTY: emptied, or lane >= nbuf
    bool held;                                             // lane < nbuf and not the emptied buffer
    unsigned long long bcost;                              // the cost of bcand
    int empty;                                             // the emptied buffer, wave-uniform; 64: none
    int pos;                                               // a held buffer's position in best_candidate_index_array: the empty one goes last
};

// s_cost: the wave's LDS row, written and fenced; cost: this lane's entry of it.  Stores *ref_fast_cost from lane 0.  pos is the
// number of held buffers below the lane, popcount(ballot(held) & below); for a held lane that is lane - (lane > empty).
// fast_pick_kernel takes pos; inter_pick_kernel, which needs empty for its mask anyway, takes the closed form: each form measured
// slower in the other kernel.
__device__ __forceinline__ FastWalk fast_walk(const unsigned long long* s_cost, unsigned long long cost, int ncand, int n, int nbuf, int lane,
                                              unsigned long long* ref_fast_cost) {
    const unsigned long long below = (1ull << lane) - 1ull;
    int rank = 0;
#pragma unroll 8
    for (int c = 0; c < ncand; c++) rank += s_cost[c] < cost;

    FastWalk w;
    // while a buffer is empty the re-scan stops at the first empty one: the last nbuf list entries fill the buffers in order
    w.bcand = lane < nbuf ? ncand - 1 - lane : 0;
    w.brank = __shfl(rank, w.bcand, 64);
    if (lane >= nbuf) w.brank = FW_EMPTY;
    w.empty = 64;
    if (nbuf > n) {
        // from here every buffer is full and the re-scan returns the first buffer of the largest rank.  The ranks held, as a bit set on
        // the scalar unit: its top bit is that rank, one ballot finds the lanes that hold it
        unsigned long long bits = lane < nbuf ? 1ull << w.brank : 0ull;
#pragma unroll
        for (int x = 32; x >= 1; x >>= 1) {
            const uint32_t lo = __shfl_xor((uint32_t)bits, x, 64), hw = __shfl_xor((uint32_t)(bits >> 32), x, 64);
            bits |= ((unsigned long long)hw << 32) | lo;
        }
        unsigned long long held_ranks = ((unsigned long long)(uint32_t)__builtin_amdgcn_readfirstlane((int)(bits >> 32)) << 32) |
                                        (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)bits);
#pragma unroll 1
        for (int c = ncand - nbuf - 1;; c--) {
            const int top = 63 - __builtin_clzll(held_ranks);
            const unsigned long long eq = __ballot(w.brank == top);              // (lanes from nbuf up hold FW_EMPTY)
            const int hi = __builtin_ctzll(eq);
            if (c < 0) {
                if (lane == hi) w.brank = FW_EMPTY;                              // :1361
                w.empty = hi;
                break;
            }
            const int rc = __builtin_amdgcn_readlane(rank, c);
            if ((eq & (eq - 1ull)) == 0) held_ranks &= ~(1ull << top);           // the only buffer of that rank is overwritten
            held_ranks |= 1ull << rc;
            if (lane == hi) { w.brank = rc; w.bcand = c; }
        }
    }
    w.held = lane < nbuf && w.brank != FW_EMPTY;
    w.pos = __popcll(__ballot(w.held) & below);
    w.bcost = s_cost[w.bcand];
    // ref_fast_cost: buffers 0 .. n-1 by buffer index
    unsigned long long ref = lane < n ? (w.brank == FW_EMPTY ? FW_MAX_CU_COST : w.bcost) : ~0ull;
#pragma unroll
    for (int x = 32; x >= 1; x >>= 1) {
        const uint32_t lo = __shfl_xor((uint32_t)ref, x, 64), hw = __shfl_xor((uint32_t)(ref >> 32), x, 64);
        const unsigned long long o = ((unsigned long long)hw << 32) | lo;
        ref = o < ref ? o : ref;
    }
    if (lane == 0) *ref_fast_cost = ref < FW_MAX_MODE_COST ? ref : FW_MAX_MODE_COST;
    return w;
}

// The order phase on fast_walk's brank: sorted_candidate_index_array[lane] as a slot, for lane < n.  Position i starts as slot i.  A
// function of its own so that inter_pick_kernel can run its inter-before-intra pass, which ends in an LDS round trip, in front of it:
// measured faster there than behind it.
__device__ __forceinline__ int fast_sorted(int brank, int n, int lane) {
    const unsigned long long below = (1ull << lane) - 1ull;
    int sval = lane;
#pragma unroll 1
    for (int i = 0; i + 1 < n; i++) {
        const int ri = __builtin_amdgcn_readlane(brank, i);
        const bool in_j = lane > i && lane < n && brank < ri;
        const unsigned long long J = __ballot(in_j);
        if (J) {
            const unsigned long long jb = J & below;
            const int from = in_j ? (jb ? 63 - __builtin_clzll(jb) : i) : (lane == i ? 63 - __builtin_clzll(J) : lane);
            sval = __shfl(sval, from, 64);
        }
    }
    return sval;
}

}  // namespace svtdev

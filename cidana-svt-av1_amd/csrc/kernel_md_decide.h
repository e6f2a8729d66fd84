// kernel_md_decide.h — md_decide_kernel: the join of mode decision, the rest of AV1PerformFullLoop (EbProductCodingLoop.c:1877-2184) and
// product_full_mode_decision (EbModeDecision.c:2653-2690): the full cost of every (block, slot), the full loop's early exit, the best
// slot of every block and the gather of that slot's prediction, coefficients and inter record, for many groups in one launch.  It reads
// what tx_decide_kernel (the luma record), full_loop_kernel / coeff_rate_kernel (chroma), the pick kernels (rates, list indices, inter
// candidates) and cfl_decide_kernel write.
//
//   cost     md_slot (below) is Av1FullCost (EbRateDistortionCost.c:1456-1534) and Av1MergeSkipFullCost (:1551-1692) as
//            av1_inter_full_cost (:1761-1811) chooses between them, in uint64 arithmetic that wraps.
//   walk     escape (:1935-1941, :2170-2181) and arg-min (EbModeDecision.c:2674-2690) in one pass over a block's slots.
//
// The unit / tile / owner-lane shape of tx_decide_kernel (kernel_tx_decide.h): a wave-unit is 2^bpul consecutive blocks of one group,
// bpul chosen by the host so that the largest gather of the block size is at most 512 quads per array and the unit's costs fit the
// wave's tile.  Two phases, no barrier between waves (tiles are per wave):
//   decide   the unit's nb * n (block, slot) pairs are consecutive in every per-slot table: lane j of step k computes pair 64 k + j from
//            contiguous loads and stores its cost into the wave's LDS tile (rows of n + 1 words) and its two walk bits (intra,
//            y_has_coeff) into a byte tile.  Then lane b OWNS block b: it walks its row, computes the winner's md_slot again and reads
//            the best intra slot's list index (the reads addressed by device data: slots below n by construction; the lines were
//            fetched a moment ago)
//            and stores the 72-byte record as nine 8-byte words.
//   gather   td_gather, 16 bytes per lane, all loads before the first store, once per requested array with the array's own log2 size.
// Everything about the size is wave-uniform runtime data: one kernel for every block size.
#pragma once
#include "dev_common.h"
#include "group_table.h"
#include "kernel_winner_gather.h"

namespace svtdev {

constexpr int MD_MAX_GROUPS = 10;          // per launch: what fits the kernel arguments
constexpr int MD_MAX_SLOTS = 40;           // SVT_HIP_MAX_NFL
constexpr int MD_THREADS = 256, MD_WAVES = MD_THREADS / 64;
constexpr int MD_COST_WORDS = 64 * 17;     // a wave's cost tile: nb rows of n + 1 words (host: md_decide_bpul keeps nb * (n + 1) inside)
constexpr int MD_DEC_WORDS = 9;            // svt_hip_md_decision as 8-byte words

struct MdDecideGroupDev {
    const unsigned long long* luma;        // [nblocks][n][5]: svt_hip_tx_decision as words
    const unsigned long long* cdist[2];    // optional [nblocks][n][2]: Cb, Cr
    const unsigned long long* cbits[2];    // [nblocks][n]
    const uint16_t* ceob[2];               // [nblocks][n]
    const uint32_t* rate;                  // [nblocks][n][2]
    const uint8_t* cand;                   // [nblocks][n]
    const uint32_t* cand_out;              // [nblocks][n][4]: svt_hip_inter_cand as words; NULL: no inter candidate
    const unsigned long long* cfl;         // optional [nblocks][n][4]: svt_hip_cfl_decision as words
    const uint32_t* blk;                   // [nblocks]: svt_hip_md_blk as a word
    const int32_t* rates;                  // svt_hip_md_rates
    unsigned long long* decision;          // [nblocks][9]
    unsigned long long* full_cost;         // optional [nblocks][n]
    const int32_t* gin[10]; int32_t* gout[10];             // gathers: pred Y Cb Cr, qcoeff Y Cb Cr, dqcoeff Y Cb Cr, inter record; NULL out: none
    unsigned long long modes4[4];          // intra mode i in bits 4 (i & 15) .. of word i >> 4
    uint32_t nblocks, wg_end;
    uint32_t lambda;
    uint8_t n, ninter;
    uint8_t cfl_allowed, slice_is_intra, escape;
    uint8_t bpul;                          // log2 blocks per wave-unit, 0 .. 6
    uint8_t nql[10];                       // log2 quads (16 bytes) of one (block, slot) of each gathered array, 0 .. 8
};
struct MdDecideDesc {
    int32_t ngroups;
    MdDecideGroupDev g[MD_MAX_GROUPS];
};
static_assert(sizeof(MdDecideDesc) <= 4000, "kernel arguments");

// offsets into svt_hip_md_rates, in words
constexpr int MD_RATE_SKIP = 0, MD_RATE_UV = 9, MD_RATE_CFL = 9 + 2 * 13 * 15;

struct MdSlot {
    unsigned long long cost, cost_luma, merge_cost, skip_cost, lambda_rate, y_dist;
    uint32_t eob[3];
    uint32_t cand, mode;                   // list index; the intra slot's pred_mode
    uint32_t intra, skip, merge, yhc, tx_type, uv_mode, cfl_idx, cfl_signs;
};

__device__ __forceinline__ unsigned long long md_rdcost(unsigned long long lambda, unsigned long long r, unsigned long long d) {
    return ((r * lambda + 256ull) >> 9) + (d << 7);
}

// the pred_mode of the slot whose list index is cand: 0 for an inter slot, else the intra list's entry, clamped to 12
__device__ __forceinline__ uint32_t md_intra_mode(const MdDecideGroupDev& F, uint32_t cand) {
    if (cand < F.ninter) return 0u;
    const uint32_t mi = (cand - F.ninter) & 63u, mw = mi >> 4;
    const unsigned long long mword = mw == 0 ? F.modes4[0] : (mw == 1 ? F.modes4[1] : (mw == 2 ? F.modes4[2] : F.modes4[3]));
    return min((uint32_t)(mword >> (4 * (mi & 15u))) & 15u, 12u);
}

// everything the reference computes for one (block, slot) after the planes' transform loops; pair = block * n + slot
__device__ __forceinline__ MdSlot md_slot(const MdDecideGroupDev& F, uint32_t pair, uint32_t blkword) {
    MdSlot s;
    const unsigned long long lambda = F.lambda;
    const unsigned long long* L = F.luma + 5 * (size_t)pair;
    const unsigned long long yd0 = L[1], yd1 = L[2], ybits = L[3], tail = L[4];
    s.y_dist = yd0;
    s.eob[0] = (uint32_t)tail & 0xffffu; s.tx_type = (uint32_t)(tail >> 16) & 0xffu; s.yhc = ((uint32_t)(tail >> 32) & 0xffu) != 0;
    const uint32_t skip_ctx = min(blkword & 0xffu, 2u);
    const bool has_uv = ((blkword >> 8) & 0xffu) != 0;
    unsigned long long cd0 = 0, cd1 = 0, cbits = 0;                         // Cb + Cr
    s.eob[1] = s.eob[2] = 0;
    if (F.cdist[0] && has_uv) {
#pragma unroll
        for (int p = 0; p < 2; p++) {
            cd0 += F.cdist[p][2 * (size_t)pair]; cd1 += F.cdist[p][2 * (size_t)pair + 1];
            cbits += F.cbits[p][pair];
            s.eob[1 + p] = F.ceob[p][pair];
        }
    }
    const unsigned long long luma_rate = F.rate[2 * (size_t)pair];
    unsigned long long chroma_rate = F.rate[2 * (size_t)pair + 1];
    s.cand = F.cand[pair];
    s.intra = s.cand >= F.ninter;
    s.mode = md_intra_mode(F, s.cand);
    s.merge = !s.intra && F.cand_out && (F.cand_out[4 * (size_t)pair + 3] >> 24 & 1u);
    s.uv_mode = s.cfl_idx = s.cfl_signs = 0;
    if (F.cfl && s.intra && has_uv) {
        const unsigned long long c = F.cfl[4 * (size_t)pair + 3];
        s.uv_mode = (uint32_t)c & 0xffu; s.cfl_idx = (uint32_t)(c >> 8) & 0xffu; s.cfl_signs = (uint32_t)(c >> 16) & 0xffu;
    }
    const unsigned long long coeff_rate = ybits + cbits, dist = yd0 + cd0;
    s.cost_luma = s.merge_cost = s.skip_cost = 0;
    s.skip = 0;
    if (s.merge) {                                                          // Av1MergeSkipFullCost
        const unsigned long long skip_rate = (unsigned long long)(long long)F.rates[MD_RATE_SKIP + skip_ctx * 3 + 1];
        const unsigned long long skip_dist = yd1 + cd1;
        s.merge_cost = md_rdcost(lambda, luma_rate + chroma_rate + coeff_rate, dist);
        s.skip_cost = md_rdcost(lambda, skip_rate, skip_dist);
        s.skip = s.skip_cost <= s.merge_cost;
        s.cost = s.skip ? s.skip_cost : s.merge_cost;
        s.lambda_rate = s.cost - (s.skip ? skip_dist : dist);
    } else {                                                                // Av1FullCost
        if (s.uv_mode == 13) {                                              // (set only for an intra slot of a has_uv block)
            const uint32_t signs = min(s.cfl_signs, 7u);
            const int32_t* A = F.rates + MD_RATE_CFL + signs * 32;
            const int32_t* U = F.rates + MD_RATE_UV + (F.cfl_allowed * 13 + s.mode) * 15;
            chroma_rate += (unsigned long long)(long long)(int32_t)((uint32_t)A[s.cfl_idx >> 4] + (uint32_t)A[16 + (s.cfl_idx & 15u)]);
            chroma_rate += (unsigned long long)(long long)U[13];
            chroma_rate -= (unsigned long long)(long long)U[0];
        }
        s.cost = md_rdcost(lambda, luma_rate + chroma_rate + coeff_rate, dist);
        s.lambda_rate = s.cost - dist;
        s.cost_luma = md_rdcost(lambda, luma_rate + ybits, yd0);
    }
    return s;
}

__global__ __launch_bounds__(MD_THREADS) void md_decide_kernel(const MdDecideDesc fd) {
    __shared__ unsigned long long cost_all[MD_WAVES * MD_COST_WORDS];
    __shared__ uint8_t bits_all[MD_WAVES * MD_COST_WORDS];
    uint32_t bid;
    const int gi = group_of(fd, bid);
    if (gi >= fd.ngroups) return;
    const MdDecideGroupDev& F = fd.g[gi];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int n = F.n, bpul = F.bpul;
    const uint32_t blk0 = (bid * MD_WAVES + wave) << bpul;                 // (below nblocks + 2^8: no wrap)
    if (blk0 >= F.nblocks) return;                                          // wave-uniform; no workgroup barrier below
    const int nb = (int)min(F.nblocks - blk0, 1u << bpul);                  // blocks of this unit, 1 .. 64
    const uint32_t pair0 = blk0 * (uint32_t)n;                              // host-checked: nblocks * n below 2^31
    const int npairs = nb * n;                                              // 1 .. MD_COST_WORDS - nb
    unsigned long long* tile = cost_all + wave * MD_COST_WORDS;
    uint8_t* wbits = bits_all + wave * MD_COST_WORDS;

    // ---- decide: the costs of the unit's pairs, contiguous loads ----
#pragma unroll 1
    for (int k = 0; k * 64 < npairs; k++) {
        const int idx = k * 64 + lane;
        if (idx < npairs) {
            const uint32_t pair = pair0 + (uint32_t)idx;
            const int b = idx / n, t = idx - b * n;
            const MdSlot s = md_slot(F, pair, F.blk[blk0 + b]);
            tile[b * (n + 1) + t] = s.cost;
            wbits[b * (n + 1) + t] = (uint8_t)(s.intra | s.yhc << 1);
            if (F.full_cost) F.full_cost[pair] = s.cost;
        }
    }
    wave_lds_fence();

    // ---- walk: lane b owns block blk0 + b ----
    int win = 0;
    uint32_t weob[3] = {0, 0, 0};
    if (lane < nb) {
        const bool escapes = !F.slice_is_intra;
        unsigned long long lowest = ~0ull, lowest_intra = ~0ull, best_full = 0xFFFFFFFFull;
        uint32_t zero_coeff = 1;                                            // best_inter_luma_zero_coeff
        int count = n, bi = -1;
#pragma unroll 1
        for (int k = 0; k < n; k++) {
            const unsigned long long c = tile[lane * (n + 1) + k];
            const uint32_t wb = wbits[lane * (n + 1) + k], intra = wb & 1u;
            if (escapes && (intra || F.escape == 2) && zero_coeff == 0) { count = k; break; }
            if (escapes && F.escape && !intra && c < best_full) { zero_coeff = wb >> 1; best_full = c; }
            if (intra && c < lowest_intra) { bi = k; lowest_intra = c; }
            if (c < lowest) { win = k; lowest = c; }
        }
        const uint32_t blkword = F.blk[blk0 + lane], row = pair0 + (uint32_t)(lane * n);
        const MdSlot w = md_slot(F, row + (uint32_t)win, blkword);
        const uint32_t best_intra_mode = bi >= 0 ? md_intra_mode(F, F.cand[row + (uint32_t)bi]) : 0xffu;
        const uint32_t uhc = w.eob[1] != 0, vhc = w.eob[2] != 0;
        weob[0] = w.eob[0]; weob[1] = w.eob[1]; weob[2] = w.eob[2];
        unsigned long long* rec = F.decision + MD_DEC_WORDS * (size_t)(blk0 + lane);
        rec[0] = w.cost; rec[1] = w.cost_luma; rec[2] = w.merge_cost; rec[3] = w.skip_cost; rec[4] = w.lambda_rate;
        rec[5] = (w.y_dist & 0xffffffffull) | (unsigned long long)w.eob[0] << 32 | (unsigned long long)w.eob[1] << 48;
        rec[6] = (unsigned long long)w.eob[2] | (unsigned long long)win << 16 | (unsigned long long)w.cand << 24 |
                 (unsigned long long)count << 32 | (unsigned long long)w.intra << 40 | (unsigned long long)w.skip << 48 |
                 (unsigned long long)w.merge << 56;
        rec[7] = (unsigned long long)w.yhc | (unsigned long long)uhc << 8 | (unsigned long long)vhc << 16 |
                 (unsigned long long)(w.yhc | uhc | vhc) << 24 | (unsigned long long)w.tx_type << 32 |
                 (unsigned long long)best_intra_mode << 40 | (unsigned long long)w.uv_mode << 48 | (unsigned long long)w.cfl_idx << 56;
        rec[8] = w.cfl_signs;
    }

    // ---- gather: the winners' predictions, coefficients and inter records ----
#pragma unroll
    for (int a = 0; a < 10; a++) {
        if (F.gout[a]) {
            const int nql = F.nql[a], uql = bpul + nql;                     // log2 quads of a full unit, <= TD_UNIT_QUADS_LOG2
            const int src = (a >= 3 && a < 9 && weob[a % 3] == 0) ? -1 : win;       // a coefficient plane with eob 0: zeros, nothing read
            td_gather(F.gin[a], F.gout[a], blk0, nb, n, nql, uql > 6 ? 1 << (uql - 6) : 1, lane, src);
        }
    }
}

}  // namespace svtdev

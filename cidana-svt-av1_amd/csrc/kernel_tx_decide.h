// kernel_tx_decide.h — tx_decide_kernel: the end of ProductFullLoopTxSearch (EbFullLoop.c:927-1124), the RD cost of every
// (block, transform type), the best type of every block and the gather of that type's coefficients, for many groups in one launch.
// It reads what full_loop_kernel (dist, eob, qcoeff, dqcoeff) and coeff_rate_kernel (bits) write.
//
//   cost     av1_tu_calc_cost_luma (EbRateDistortionCost.c:2120-2194): RDCOST(lambda, bits, dist[DIST_CALC_RESIDUAL]) =
//            ((bits * lambda + 256) >> 9) + dist * 128 in uint64 arithmetic that wraps; the zero-cbf branch is compiled to UINT64_MAX.
//   skip     a type other than DCT_DCT whose eob is 0 is no candidate (:1034).  Its cost is stored as UINT64_MAX, which can never pass
//            the strict < against a best that starts at UINT64_MAX (nor could a computed cost of that value): exact.
//   pick     the first i with cost_i < best (:1102).
//
// A wave-unit is 2^bpul consecutive blocks of one group, bpul chosen by the host so that the unit's gather is 512 quads, 8 KiB, per array
// (2 blocks of 1024 coefficients .. 64 blocks of 32; 64 blocks of 16 are 4 KiB: a lane owns a block, so 64 is the most).  Two phases,
// no barrier between waves (tiles are per wave):
//   decide   the unit's nb * ntypes (block, type) pairs are consecutive in all three tables: lane j of step k loads pair 64 k + j
//            (dist[DIST_CALC_RESIDUAL], 8 bytes at a 16-byte stride, 8 of bits, 2 of eob: every instruction reads inside one contiguous
//            run; dist[DIST_CALC_PREDICTION] is read for the winner only) and stores the pair's cost into the wave's LDS tile, rows of ntypes + 1 words so that the next step's column walk is spread over the banks.  Then lane b
//            OWNS block b: it walks its row, keeps the first strict minimum, fetches the winner's dist / bits / eob again (the one read
//            addressed by device data: the winner's position, below ntypes by construction; the lines were fetched a moment ago) and
//            stores the 40-byte record as five 8-byte words.
//   gather   16 bytes per lane.  Quad q of the unit (q = 64 g + lane) belongs to block q >> nql at quad q & (2^nql - 1), nql = log2(NC / 4):
//            for NC >= 256 a wave instruction is 1 KiB of one block, smaller blocks share it on aligned lane groups.  The winner's
//            position comes from the owning lane by ds_bpermute (__shfl).  A winner with eob 0, or no winner, stores zeros and reads
//            nothing.  At most TD_GATHER instructions per array, all loads issued before the first store.
// Everything about the size is wave-uniform runtime data (shifts): one kernel for the 19 sizes.
#pragma once
#include "dev_common.h"
#include "group_table.h"
#include "kernel_winner_gather.h"

namespace svtdev {

constexpr int TD_MAX_GROUPS = 32;          // per launch: what fits the kernel arguments
constexpr int TD_MAX_TYPES = 16;
constexpr int TD_THREADS = 256, TD_WAVES = TD_THREADS / 64;
constexpr int TD_COST_WORDS = 64 * (TD_MAX_TYPES + 1);     // a wave's cost tile: up to 64 rows of ntypes + 1

struct TxDecideGroupDev {
    const unsigned long long* dist;        // [nblocks][ntypes][2]
    const uint16_t* eob;                   // [nblocks][ntypes]
    const unsigned long long* bits;        // [nblocks][ntypes]
    const int32_t* qcoeff; const int32_t* dqcoeff;         // optional [nblocks][ntypes][NC]
    unsigned long long* decision;          // [nblocks][5]: svt_hip_tx_decision as words
    int32_t* best_qcoeff; int32_t* best_dqcoeff;           // optional [nblocks][NC]
    unsigned long long types;              // tx_types[i] in bits 4 i .. 4 i + 3
    uint32_t nblocks, wg_end;
    uint32_t lambda;
    uint8_t ntypes;
    int8_t dct_index;                      // DCT_DCT's position in the list, -1: not listed
    uint8_t nql;                           // log2(NC / 4), 2 .. 8
    uint8_t bpul;                          // log2 blocks per wave-unit, 1 .. 6 (host: tx_decide_bpul)
};
struct TxDecideDesc {
    int32_t ngroups;
    TxDecideGroupDev g[TD_MAX_GROUPS];
};
static_assert(sizeof(TxDecideDesc) <= 4000, "kernel arguments");

__global__ __launch_bounds__(TD_THREADS) void tx_decide_kernel(const TxDecideDesc fd) {
    __shared__ unsigned long long cost_all[TD_WAVES * TD_COST_WORDS];
    uint32_t bid;
    const int gi = group_of(fd, bid);
    if (gi >= fd.ngroups) return;
    const TxDecideGroupDev& F = fd.g[gi];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int ntypes = F.ntypes, nql = F.nql, bpul = F.bpul;
    const uint32_t blk0 = (bid * TD_WAVES + wave) << bpul;                 // (below nblocks + 2^8: no wrap)
    if (blk0 >= F.nblocks) return;                                          // wave-uniform; no workgroup barrier below
    const int nb = (int)min(F.nblocks - blk0, 1u << bpul);                  // blocks of this unit, 1 .. 64
    const uint32_t pair0 = blk0 * (uint32_t)ntypes;                         // host-checked: nblocks * ntypes below 2^31
    const int npairs = nb * ntypes;                                         // 1 .. 1024
    unsigned long long* tile = cost_all + wave * TD_COST_WORDS;
    const unsigned long long lambda = F.lambda;

    // ---- decide: the costs of the unit's pairs, contiguous loads ----
#pragma unroll 1
    for (int k = 0; k * 64 < npairs; k++) {
        const int idx = k * 64 + lane;
        if (idx < npairs) {
            const uint32_t pair = pair0 + (uint32_t)idx;
            const int b = idx / ntypes, t = idx - b * ntypes;
            const unsigned long long d0 = F.dist[2 * (size_t)pair], bits = F.bits[pair];
            const bool skip = F.eob[pair] == 0 && t != F.dct_index;
            const unsigned long long cost = ((bits * lambda + 256ull) >> 9) + d0 * 128ull;
            tile[b * (ntypes + 1) + t] = skip ? ~0ull : cost;
        }
    }
    wave_lds_fence();

    // ---- pick: lane b owns block blk0 + b ----
    int src = -1;                                                           // the gather's source position; -1: zeros
    if (lane < nb) {
        unsigned long long best = ~0ull;
        int win = -1;
#pragma unroll 1
        for (int i = 0; i < ntypes; i++) {
            const unsigned long long c = tile[lane * (ntypes + 1) + i];
            if (c < best) { best = c; win = i; }
        }
        unsigned long long d0 = 0, d1 = 0, bits = 0, tail = 0xffull << 24;   // no candidate: DCT_DCT, type_index 0xFF
        if (win >= 0) {
            const uint32_t pair = pair0 + (uint32_t)(lane * ntypes + win);
            const ulonglong2 d = *reinterpret_cast<const ulonglong2*>(F.dist + 2 * (size_t)pair);
            const uint32_t eob = F.eob[pair];
            d0 = d.x; d1 = d.y; bits = F.bits[pair];
            const uint32_t ty = (uint32_t)(F.types >> (4 * win)) & 15u;
            tail = eob | ((unsigned long long)ty << 16) | ((unsigned long long)win << 24) | ((unsigned long long)(eob != 0) << 32);
            src = eob ? win : -1;
        }
        unsigned long long* rec = F.decision + 5 * (size_t)(blk0 + lane);
        rec[0] = best; rec[1] = d0; rec[2] = d1; rec[3] = bits; rec[4] = tail;
    }

    // ---- gather: the winners' coefficients ----
    const int uql = bpul + nql;                                             // log2 quads of a full unit, <= TD_UNIT_QUADS_LOG2
    const int ngather = uql > 6 ? 1 << (uql - 6) : 1;
    if (F.best_qcoeff) td_gather(F.qcoeff, F.best_qcoeff, blk0, nb, ntypes, nql, ngather, lane, src);
    if (F.best_dqcoeff) td_gather(F.dqcoeff, F.best_dqcoeff, blk0, nb, ntypes, nql, ngather, lane, src);
}

}  // namespace svtdev

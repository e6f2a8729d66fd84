// kernel_fast_pick.h — fast_pick_kernel: the end of the fast loop for an all-intra candidate list.  Per block: av1_intra_fast_cost
// (EbRateDistortionCost.c:598-728) of every candidate, the buffer walk of perform_fast_loop (EbProductCodingLoop.c:1225-1363),
// sort_fast_loop_candidates (EbModeDecision.c:436-489) and the gather of the surviving predictions.  It reads what fast_loop_kernel
// writes (dist, pred) and writes what full_loop_kernel reads (pred, src_xy).
//
// One wave per block, bpw blocks per wave one after the other (1 .. FP_MAX_BPW: the host grows it once the group has more blocks than
// the device holds waves), FP_WAVES waves per workgroup; the 877 words of rate tables are
// staged in LDS once per workgroup (the only workgroup barrier).  Three phases per block, fenced per wave:
//   cost     lane = candidate.  Rates from the LDS tables (the context bytes clamped first), the two model_rd evaluations under SSD
//            (one 64-bit division each), cost, luma / chroma rate -> the wave's LDS rows.  Then the candidate's RANK: the number of
//            the block's costs below its own (ncand broadcast reads).  Equal costs share a rank, so every later comparison of two
//            costs is the comparison of two 7-bit ranks; 127 = MAX_CU_COST, an empty buffer.
//   walk     lane = buffer.  The reference's re-scan (strict >, stops at the first buffer at MAX_CU_COST) returns the first empty
//            buffer, else the first buffer holding the maximum.  So the last nbuf list entries fill the buffers in order (one
//            ds_bpermute), and from then on the set of ranks held is a 64-bit mask on the scalar unit: its top bit is the largest rank,
//            one ballot gives the lanes that hold it, the first of them is the buffer to overwrite, and the bit is cleared when that
//            lane was the only one.  ncand - nbuf steps of a ballot, a v_readlane and a handful of SALU instructions.
//            sort_fast_loop_candidates' bubble pass i swaps position i with every j > i whose BUFFER cost is below buffer i's, in
//            ascending j: a rotation of the entries at {i} + J, one ballot and one ds_bpermute per i.
//   gather   the whole wave copies the n winners, 16 bytes per lane, four loads in flight before the first store.  The winners' list
//            positions (below ncand by construction; the row is zeroed first) are the only device data that addresses memory.
#pragma once
#include "dev_common.h"
#include "model_rd.h"

namespace svtdev {

constexpr int FP_THREADS = 256, FP_WAVES = FP_THREADS / 64;
constexpr int FP_MAX_BPW = 4;                              // blocks per wave, at most
constexpr int FP_EMPTY = 127;                              // the rank of MAX_CU_COST
constexpr unsigned long long FP_MAX_CU_COST = ~0ull >> 1, FP_MAX_MODE_COST = 13616969489728ull * 8ull;
// svt_hip_fast_rates as words
constexpr int FP_Y = 0, FP_MB = FP_Y + 5 * 5 * 14, FP_UV = FP_MB + 4 * 14, FP_ANG = FP_UV + 2 * 13 * 15, FP_SKIP = FP_ANG + 8 * 8,
              FP_II = FP_SKIP + 3 * 3, FP_RATE_WORDS = FP_II + 4 * 2;

struct FastPickDev {
    const unsigned long long* dist;                        // [nblocks][ncand]
    const unsigned long long* dist_cb; const unsigned long long* dist_cr;      // optional
    const unsigned long long* blk;                         // [nblocks]: svt_hip_fast_pick_blk as a word
    const int32_t* rates;                                  // svt_hip_fast_rates
    const uint8_t* pred;                                   // optional [nblocks][ncand][H][W]
    const uint32_t* src_xy;                                // optional [nblocks]
    uint8_t* cand_out; uint8_t* sorted;                    // [nblocks][n]
    unsigned long long* cost;                              // [nblocks][n]
    uint32_t* rate;                                        // [nblocks][n][2]
    unsigned long long* ref_fast_cost;                     // [nblocks]
    unsigned long long* all_cost;                          // optional [nblocks][ncand]
    uint8_t* pred_out;                                     // optional [nblocks][n][H][W]
    uint32_t* src_xy_out;                                  // optional [nblocks][n]
    uint32_t nblocks, lambda, intrabc_bits, qstep;
    uint16_t cand[64];                                     // mode | (delta + 3) << 4 | uv mode (CfL as DC) << 8 | (uv delta + 3) << 12
    uint8_t ncand, n, nbuf, ssd, slice_is_intra, use_angle_delta, cfl_allowed, size_group, nlog2_y, nlog2_uv;
    uint8_t ql;                                            // log2(W * H / 16)
    uint8_t bpw;                                           // blocks per wave, 1 .. FP_MAX_BPW (host: enough waves to fill the device first)
};

__global__ __launch_bounds__(FP_THREADS) void fast_pick_kernel(const FastPickDev F) {
    __shared__ int32_t s_rates[FP_RATE_WORDS];
    __shared__ unsigned long long s_cost[FP_WAVES][64];
    __shared__ uint32_t s_lr[FP_WAVES][64], s_cr[FP_WAVES][64];
    __shared__ uint8_t s_win[FP_WAVES][64];
    for (int i = threadIdx.x; i < FP_RATE_WORDS; i += FP_THREADS) s_rates[i] = F.rates[i];
    __syncthreads();
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int ncand = F.ncand, n = F.n, nbuf = F.nbuf, ql = F.ql;
    const bool scratch = nbuf > n;
    const unsigned long long below = (1ull << lane) - 1ull;
    // the candidate of this lane
    const uint32_t c16 = F.cand[lane];
    const int m = c16 & 15, dl = (c16 >> 4) & 7, uvm = (c16 >> 8) & 15, uvd = (c16 >> 12) & 7;
    const bool use_delta = F.use_angle_delta && m >= 1 && m <= 8;                // the candidate field (EbModeDecision.c:2444, :2490)
    constexpr unsigned long long kIntraModeContext = 0ull | 1ull << 3 | 2ull << 6 | 3ull << 9 | 4ull << 12 | 4ull << 15 | 4ull << 18 |
                                                     4ull << 21 | 3ull << 24 | 0ull << 27 | 1ull << 30 | 2ull << 33 | 0ull << 36;

#pragma unroll 1
    for (int j = 0; j < F.bpw; j++) {
        const uint32_t blk = (blockIdx.x * FP_WAVES + (uint32_t)wave) * F.bpw + (uint32_t)j;
        if (blk >= F.nblocks) break;                                             // wave-uniform
        wave_lds_fence();                                                        // the previous block's LDS reads before these writes
        // ---- cost: lane = candidate ----
        const unsigned long long rec = F.blk[blk];
        const uint32_t top = min((uint32_t)(rec & 0xff), 12u), left = min((uint32_t)((rec >> 8) & 0xff), 12u);
        const uint32_t skip_ctx = min((uint32_t)((rec >> 16) & 0xff), 2u), inter_ctx = min((uint32_t)((rec >> 24) & 0xff), 3u);
        const bool has_chroma = ((rec >> 32) & 0xff) != 0;
        unsigned long long cost = ~0ull;
        uint32_t lr = 0, cr = 0;
        if (lane < ncand) {
            if (F.slice_is_intra) {
                const uint32_t a = (uint32_t)(kIntraModeContext >> (3 * top)) & 7u, l = (uint32_t)(kIntraModeContext >> (3 * left)) & 7u;
                lr = (uint32_t)s_rates[FP_Y + (a * 5 + l) * 14 + m];
            } else {
                lr = (uint32_t)s_rates[FP_MB + F.size_group * 14 + m] + (uint32_t)s_rates[FP_SKIP + skip_ctx * 3] +
                     (uint32_t)s_rates[FP_II + inter_ctx * 2];
            }
            if (use_delta) lr += (uint32_t)s_rates[FP_ANG + (m - 1) * 8 + dl];
            lr += F.intrabc_bits;
            if (has_chroma) {
                cr = (uint32_t)s_rates[FP_UV + (F.cfl_allowed * 13 + m) * 15 + uvm];
                if (use_delta && uvm >= 1 && uvm <= 8) cr += (uint32_t)s_rates[FP_ANG + (uvm - 1) * 8 + uvd];
            }
            const size_t at = (size_t)blk * ncand + lane;
            const unsigned long long luma = F.dist[at];
            unsigned long long chroma = 0;
            if (F.dist_cb) chroma += F.dist_cb[at];
            if (F.dist_cr) chroma += F.dist_cr[at];
            uint32_t rate = lr + cr;
            unsigned long long d = luma + chroma;
            if (F.ssd) {
                uint32_t r1, r2;
                unsigned long long d1, d2;
                fp_model_rd(luma, F.nlog2_y, F.qstep, r1, d1);
                fp_model_rd(chroma, F.nlog2_uv, F.qstep, r2, d2);
                rate = lr + r1 + r2;                                             // the model's chroma rate replaces chromaRate (:704-710)
                d = d1 + d2;
            }
            cost = (((unsigned long long)rate * F.lambda + 256ull) >> 9) + d * 128ull;
            if (F.all_cost) F.all_cost[at] = cost;
        }
        s_cost[wave][lane] = cost; s_lr[wave][lane] = lr; s_cr[wave][lane] = cr; s_win[wave][lane] = 0;
        wave_lds_fence();
        int rank = 0;
#pragma unroll 8
        for (int c = 0; c < ncand; c++) rank += s_cost[wave][c] < cost;

        // ---- walk: lane = buffer ----
        // while a buffer is empty the re-scan stops at the first empty one: the last nbuf list entries fill the buffers in order
        int bcand = lane < nbuf ? ncand - 1 - lane : 0;
        int brank = __shfl(rank, bcand, 64);
        if (lane >= nbuf) brank = FP_EMPTY;
        if (scratch) {
            // from here every buffer is full and the re-scan returns the first buffer of the largest rank.  The ranks held, as a bit set on
            // the scalar unit: its top bit is that rank, one ballot finds the lanes that hold it
            unsigned long long bits = lane < nbuf ? 1ull << brank : 0ull;
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
                const unsigned long long eq = __ballot(brank == top);            // (lanes from nbuf up hold FP_EMPTY)
                const int hi = __builtin_ctzll(eq);
                if (c < 0) {
                    if (lane == hi) brank = FP_EMPTY;                            // :1361
                    break;
                }
                const int rc = __builtin_amdgcn_readlane(rank, c);
                if ((eq & (eq - 1ull)) == 0) held_ranks &= ~(1ull << top);       // the only buffer of that rank is overwritten
                held_ranks |= 1ull << rc;
                if (lane == hi) { brank = rc; bcand = c; }
            }
        }
        const bool held = lane < nbuf && brank != FP_EMPTY;
        const int slot = __popcll(__ballot(held) & below);                       // best_candidate_index_array: the empty buffer goes last
        const unsigned long long bcost = s_cost[wave][bcand];
        // ref_fast_cost: buffers 0 .. n-1 by buffer index
        unsigned long long ref = lane < n ? (brank == FP_EMPTY ? FP_MAX_CU_COST : bcost) : ~0ull;
#pragma unroll
        for (int x = 32; x >= 1; x >>= 1) {
            const uint32_t lo = __shfl_xor((uint32_t)ref, x, 64), hw = __shfl_xor((uint32_t)(ref >> 32), x, 64);
            const unsigned long long o = ((unsigned long long)hw << 32) | lo;
            ref = o < ref ? o : ref;
        }
        if (lane == 0) F.ref_fast_cost[blk] = ref < FP_MAX_MODE_COST ? ref : FP_MAX_MODE_COST;
        // sorted_candidate_index_array, as slots: position i starts as slot i
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
        const size_t row = (size_t)blk * n;
        if (held && slot < n) {
            F.cand_out[row + slot] = (uint8_t)bcand;
            F.cost[row + slot] = bcost;
            F.rate[2 * (row + slot)] = s_lr[wave][bcand];
            F.rate[2 * (row + slot) + 1] = s_cr[wave][bcand];
            s_win[wave][slot] = (uint8_t)bcand;
        }
        if (lane < n) {
            F.sorted[row + lane] = (uint8_t)sval;
            if (F.src_xy_out) F.src_xy_out[row + lane] = F.src_xy[blk];
        }

        // ---- gather: the winners' predictions ----
        if (F.pred_out) {
            wave_lds_fence();
            const uint4* in = reinterpret_cast<const uint4*>(F.pred) + (((size_t)blk * ncand) << ql);
            uint4* out = reinterpret_cast<uint4*>(F.pred_out) + (row << ql);
            const int total = n << ql, qmask = (1 << ql) - 1;                     // <= 40 * 256 quads
#pragma unroll 1
            for (int q0 = 0; q0 < total; q0 += 256) {
                uint4 v[4];
#pragma unroll
                for (int u = 0; u < 4; u++) {
                    const int q = q0 + u * 64 + lane;
                    v[u] = make_uint4(0, 0, 0, 0);
                    if (q < total) v[u] = in[((size_t)s_win[wave][q >> ql] << ql) + (q & qmask)];
                }
#pragma unroll
                for (int u = 0; u < 4; u++) {
                    const int q = q0 + u * 64 + lane;
                    if (q < total) out[q] = v[u];
                }
            }
        }
    }
}

}  // namespace svtdev

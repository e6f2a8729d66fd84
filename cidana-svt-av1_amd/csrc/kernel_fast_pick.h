// kernel_fast_pick.h — fast_pick_kernel: the end of the fast loop for an all-intra candidate list.  Per block: av1_intra_fast_cost
// (EbRateDistortionCost.c:598-728) of every candidate, the buffer walk and the order (fast_walk, fast_sorted: kernel_fast_walk.h, which
// also states the mapping of a block to a wave) and the gather of the surviving predictions.  It reads what fast_loop_kernel writes (dist, pred) and
// writes what full_loop_kernel reads (pred, src_xy).  The 877 words of rate tables are staged in LDS.  What is this kernel's own:
//   cost     lane = candidate.  Rates from the LDS tables (the context bytes clamped first), the two model_rd evaluations under SSD
//            (one 64-bit division each), cost, luma / chroma rate -> the wave's LDS rows.
//   gather   the whole wave copies the n winners, 16 bytes per lane, four loads in flight before the first store.  The winners' list
//            positions (below ncand by construction; the row is zeroed first) are the only device data that addresses memory.
#pragma once
#include "kernel_fast_walk.h"

namespace svtdev {

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
    uint8_t bpw;                                           // blocks per wave, 1 .. FW_MAX_BPW (host: enough waves to fill the device first)
};

__global__ __launch_bounds__(FW_THREADS) void fast_pick_kernel(const FastPickDev F) {
    __shared__ int32_t s_rates[FP_RATE_WORDS];
    __shared__ unsigned long long s_cost[FW_WAVES][64];
    __shared__ uint32_t s_lr[FW_WAVES][64], s_cr[FW_WAVES][64];
    __shared__ uint8_t s_win[FW_WAVES][64];
    for (int i = threadIdx.x; i < FP_RATE_WORDS; i += FW_THREADS) s_rates[i] = F.rates[i];
    __syncthreads();
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int ncand = F.ncand, n = F.n, nbuf = F.nbuf, ql = F.ql;
    // the candidate of this lane
    const uint32_t c16 = F.cand[lane];
    const int m = c16 & 15, dl = (c16 >> 4) & 7, uvm = (c16 >> 8) & 15, uvd = (c16 >> 12) & 7;
    const bool use_delta = F.use_angle_delta && m >= 1 && m <= 8;                // the candidate field (EbModeDecision.c:2444, :2490)
    constexpr unsigned long long kIntraModeContext = 0ull | 1ull << 3 | 2ull << 6 | 3ull << 9 | 4ull << 12 | 4ull << 15 | 4ull << 18 |
                                                     4ull << 21 | 3ull << 24 | 0ull << 27 | 1ull << 30 | 2ull << 33 | 0ull << 36;

#pragma unroll 1
    for (int j = 0; j < F.bpw; j++) {
        const uint32_t blk = (blockIdx.x * FW_WAVES + (uint32_t)wave) * F.bpw + (uint32_t)j;
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
            uint32_t rate;
            unsigned long long d;
            fast_cost_tail(F.ssd, luma, chroma, lr, cr, F.nlog2_y, F.nlog2_uv, F.qstep, rate, d);
            cost = (((unsigned long long)rate * F.lambda + 256ull) >> 9) + d * 128ull;
            if (F.all_cost) F.all_cost[at] = cost;
        }
        s_cost[wave][lane] = cost; s_lr[wave][lane] = lr; s_cr[wave][lane] = cr; s_win[wave][lane] = 0;
        wave_lds_fence();
        // ---- walk and order: lane = buffer ----
        const FastWalk w = fast_walk(s_cost[wave], cost, ncand, n, nbuf, lane, F.ref_fast_cost + blk);
        const int slot = w.pos, sval = fast_sorted(w.brank, n, lane);
        const size_t row = (size_t)blk * n;
        if (w.held && slot < n) {
            F.cand_out[row + slot] = (uint8_t)w.bcand;
            F.cost[row + slot] = w.bcost;
            F.rate[2 * (row + slot)] = s_lr[wave][w.bcand];
            F.rate[2 * (row + slot) + 1] = s_cr[wave][w.bcand];
            s_win[wave][slot] = (uint8_t)w.bcand;
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

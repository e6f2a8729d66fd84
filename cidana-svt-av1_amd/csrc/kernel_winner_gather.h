// kernel_winner_gather.h — td_gather: the winners' rows of a per-(block, position) array, for one wave-unit.  Shared by tx_decide_kernel
// (kernel_tx_decide.h: the best type's coefficients) and md_decide_kernel (kernel_md_decide.h: the best slot's prediction, coefficients
// and inter record).  The arrays are addressed in quads of 16 bytes, so the element type does not matter: nql is log2 quads of one row.
#pragma once
#include "dev_common.h"

namespace svtdev {

constexpr int TD_UNIT_QUADS_LOG2 = 9;      // quads (16 bytes) of one array a wave-unit gathers, at most
constexpr int TD_GATHER = (1 << TD_UNIT_QUADS_LOG2) / 64;

// one array's gather for a wave-unit: blocks blk0 .. blk0 + nb - 1, winner positions in src (lane b: block b's, -1: zeros)
__device__ __forceinline__ void td_gather(const int32_t* __restrict__ in, int32_t* __restrict__ out, uint32_t blk0, int nb, int ntypes, int nql,
                                          int ngather, int lane, int src) {
    int4 v[TD_GATHER];
    const int qmask = (1 << nql) - 1;
#pragma unroll
    for (int g = 0; g < TD_GATHER; g++) {
        if (g < ngather) {
            const int q = g * 64 + lane, jb = q >> nql;                      // jb < 64
            const int w = __shfl(src, jb, 64);
            v[g] = make_int4(0, 0, 0, 0);
            if (jb < nb && w >= 0)
                v[g] = *reinterpret_cast<const int4*>(in + ((((size_t)(blk0 + jb) * ntypes + w) << nql) + (q & qmask)) * 4);
        }
    }
#pragma unroll
    for (int g = 0; g < TD_GATHER; g++) {
        if (g < ngather) {
            const int q = g * 64 + lane, jb = q >> nql;
            if (jb < nb) *reinterpret_cast<int4*>(out + ((((size_t)(blk0 + jb)) << nql) + (q & qmask)) * 4) = v[g];
        }
    }
}

}  // namespace svtdev

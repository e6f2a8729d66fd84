// recon_final_plan.h — what svt_hip_recon_final_frame settles on the host before it enqueues: the checks, the capacities and starts of
// the per-size work lists, the scratch layout and the launch shapes.  The block and transform sizes are av1_geom.h's.
// Host only (no HIP header): tests/c/recon_final_plan_host.cpp compiles it with g++; the kernels (kernel_recon_final.h) read the same
// constexpr functions.
//
// Scratch: 32 uint32 counters (one per transform size, the rest spare), then per transform size a list of 16-byte work items with room
// for rf_cap(size) items per superblock: what a tiling of a 64x64 superblock can hold of plane blocks of that size, 4096 / (w * h) luma
// blocks and twice 1024 / (w * h) chroma blocks.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "../../include/svt_hip_dsp.h"
#include "av1_geom.h"
#include "host_err.h"

namespace svthost {

constexpr int RF_MAX_GROUPS = SVT_HIP_RECON_FINAL_MAX_GROUPS;
constexpr uint32_t RF_MAX_NSB = 1u << 20;                // nsb * 4096 (a stream offset) and nsb * RF_ITEMS_PER_SB stay below 2^32
constexpr int RF_BIN_THREADS = 256, RF_BIN_WAVES = RF_BIN_THREADS / 64;      // the bin stage: one wave per superblock
constexpr uint32_t RF_MAX_GRID = 2048;                   // workgroups of a reconstruct launch: they stride over the lists
constexpr int RF_COUNTER_BYTES = 128;

// work items a superblock can add to a size's list, and where the size's list starts (in items per superblock)
constexpr uint32_t rf_cap(int tx_size) { return 4096u / ((uint32_t)kTxW[tx_size] * kTxH[tx_size]) + 2u * (1024u / ((uint32_t)kTxW[tx_size] * kTxH[tx_size])); }
constexpr uint32_t rf_list_first(int tx_size) {
    uint32_t n = 0;
    for (int t = 0; t < tx_size; t++) n += rf_cap(t);
    return n;
}
constexpr uint32_t RF_ITEMS_PER_SB = rf_list_first(SVT_TX_SIZES_ALL);
static_assert(RF_ITEMS_PER_SB == 1271 && (uint64_t)RF_MAX_NSB * RF_ITEMS_PER_SB < (1ull << 32) && (uint64_t)RF_MAX_NSB * kSbLumaSpan <= (1ull << 32), "32-bit offsets");

inline size_t recon_final_scratch_bytes(uint32_t nsb) {
    if (nsb == 0 || nsb > RF_MAX_NSB) return 0;
    return (size_t)RF_COUNTER_BYTES + (size_t)nsb * RF_ITEMS_PER_SB * 16;
}

// the reconstruct launches: one per launch kind of a transform size (av1_geom.h)
constexpr int RF_LAUNCHES = kTxLaunchKinds;
// plane blocks a workgroup takes at a time: 64 / max(w, h) per wave, four waves, two for 64x64
constexpr uint32_t rf_per_wg(int tx_size) {
    return (uint32_t)((kTxW[tx_size] * kTxH[tx_size] >= 4096 ? 2 : 4) * (64 / geom_max(kTxW[tx_size], kTxH[tx_size])));
}
inline uint32_t recon_final_bin_grid(uint32_t nsb) { return (nsb + RF_BIN_WAVES - 1) / RF_BIN_WAVES; }
// workgroups of reconstruct launch cls: every workgroup's worth of items its lists can hold, at most RF_MAX_GRID (the workgroups stride)
inline uint32_t recon_final_class_grid(int cls, uint32_t nsb) {
    uint64_t n = 0;
    for (int t = 0; t < SVT_TX_SIZES_ALL; t++)
        if (tx_launch_kind(t) == cls) n += ((uint64_t)rf_cap(t) * nsb + rf_per_wg(t) - 1) / rf_per_wg(t);
    return (uint32_t)(n < RF_MAX_GRID ? n : RF_MAX_GRID);
}

inline int recon_final_check(const svt_hip_recon_final_args* a) {
    if (!a) return set_err(SVT_HIP_ERR_INVALID, "NULL arguments");
    if (a->nsb == 0 || a->nsb > RF_MAX_NSB) return set_err(SVT_HIP_ERR_INVALID, "nsb %u (1 .. %u)", a->nsb, RF_MAX_NSB);
    if (a->nsrc == 0) return set_err(SVT_HIP_ERR_INVALID, "nsrc 0");
    if (a->planes != 1 && a->planes != 3) return set_err(SVT_HIP_ERR_INVALID, "planes %d (1 or 3)", a->planes);
    if (!a->d_final || !a->d_final_count || !a->d_decision || !a->groups) return set_err(SVT_HIP_ERR_INVALID, "NULL member");
    if (a->ngroups < 1 || a->ngroups > RF_MAX_GROUPS) return set_err(SVT_HIP_ERR_INVALID, "ngroups %d (1 .. %d)", a->ngroups, RF_MAX_GROUPS);
    if (((uintptr_t)a->d_decision & 7) || (((uintptr_t)a->d_final | (uintptr_t)a->d_final_count | (uintptr_t)a->d_coeff_offset) & 3))
        return set_err(SVT_HIP_ERR_INVALID, "misaligned buffer (d_decision 8 bytes, d_final / d_final_count / d_coeff_offset 4)");
    int nstream = 0;
    for (int p = 0; p < a->planes; p++) {
        if (!a->d_recon[p]) return set_err(SVT_HIP_ERR_INVALID, "plane %d: NULL d_recon", p);
        if (a->width[p] > 65535u || a->height[p] > 65535u || a->stride[p] < a->width[p])
            return set_err(SVT_HIP_ERR_INVALID, "plane %d: %u x %u, stride %u", p, a->width[p], a->height[p], a->stride[p]);
        if ((uintptr_t)a->d_sb_qcoeff[p] & 15) return set_err(SVT_HIP_ERR_INVALID, "plane %d: misaligned d_sb_qcoeff (16 bytes)", p);
        nstream += a->d_sb_qcoeff[p] != nullptr;
    }
    if (nstream != 0 && nstream != a->planes) return set_err(SVT_HIP_ERR_INVALID, "d_sb_qcoeff: all of the requested planes or none");
    uint64_t next = 0;
    for (int g = 0; g < a->ngroups; g++) {
        const svt_hip_recon_final_group& G = a->groups[g];
        if (G.src_first != next) return set_err(SVT_HIP_ERR_INVALID, "group %d: src_first %u, expected %llu", g, G.src_first, (unsigned long long)next);
        next += G.nblocks;
        if (next > a->nsrc) return set_err(SVT_HIP_ERR_INVALID, "group %d ends at %llu, past nsrc %u", g, (unsigned long long)next, a->nsrc);
        if (!bsize_ok(G.bsize)) return set_err(SVT_HIP_ERR_INVALID, "group %d: bsize %d", g, G.bsize);
        if (!tx_type_ok(bsize_tx_uv(G.bsize), G.tx_type_uv)) return set_err(SVT_HIP_ERR_INVALID, "group %d: tx_type_uv %d for bsize %d", g, G.tx_type_uv, G.bsize);
        for (int p = 0; p < a->planes && G.nblocks; p++) {
            if (!G.d_best_pred[p] || !G.d_best_dqcoeff[p] || (nstream && !G.d_best_qcoeff[p]))
                return set_err(SVT_HIP_ERR_INVALID, "group %d, plane %d: NULL array", g, p);
            if (((uintptr_t)G.d_best_pred[p] | (uintptr_t)G.d_best_dqcoeff[p] | (nstream ? (uintptr_t)G.d_best_qcoeff[p] : 0)) & 15)
                return set_err(SVT_HIP_ERR_INVALID, "group %d, plane %d: misaligned array (16 bytes)", g, p);
        }
    }
    if (next != a->nsrc) return set_err(SVT_HIP_ERR_INVALID, "the groups end at %llu, nsrc is %u", (unsigned long long)next, a->nsrc);
    if (!a->d_scratch || ((uintptr_t)a->d_scratch & 15) || a->scratch_bytes < recon_final_scratch_bytes(a->nsb))
        return set_err(SVT_HIP_ERR_INVALID, "scratch: NULL, misaligned or %zu bytes of %zu", a->scratch_bytes, recon_final_scratch_bytes(a->nsb));
    return SVT_HIP_OK;
}

}  // namespace svthost

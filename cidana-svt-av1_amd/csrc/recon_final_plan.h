// recon_final_plan.h — what svt_hip_recon_final_frame settles on the host before it enqueues: the checks, the block size -> transform
// size tables (blocksize_to_txsize / av1_get_max_uv_txsize, EbUtility.c:110-138, :760-779), the scratch layout and the launch shapes.
// Host only (no HIP header): tests/c/recon_final_plan_host.cpp compiles it with g++; the kernels (kernel_recon_final.h) read the same
// constexpr tables.
//
// Scratch: 32 uint32 counters (one per transform size, the rest spare), then per transform size a list of 16-byte work items with room
// for rf_cap(size) items per superblock: what a tiling of a 64x64 superblock can hold of plane blocks of that size, 4096 / (w * h) luma
// blocks and twice 1024 / (w * h) chroma blocks.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "../../include/svt_hip_dsp.h"
#include "host_err.h"

namespace svthost {

constexpr int RF_TX_SIZES = 19, RF_MAX_GROUPS = SVT_HIP_RECON_FINAL_MAX_GROUPS, RF_MAX_FINAL = SVT_HIP_SB_MAX_FINAL;
constexpr uint32_t RF_MAX_NSB = 1u << 20;                // nsb * 4096 (a stream offset) and nsb * RF_ITEMS_PER_SB stay below 2^32
constexpr int RF_BIN_THREADS = 256, RF_BIN_WAVES = RF_BIN_THREADS / 64;      // the bin stage: one wave per superblock
constexpr uint32_t RF_MAX_GRID = 2048;                   // workgroups of a reconstruct launch: they stride over the lists
constexpr int RF_COUNTER_BYTES = 128;
constexpr uint32_t RF_LUMA_SPAN = SVT_HIP_SB_QCOEFF_LUMA, RF_CHROMA_SPAN = SVT_HIP_SB_QCOEFF_LUMA / 4;

// the sides of the 19 transform sizes (tx_size_wide / tx_size_high) and of the 22 block sizes (block_size_wide / block_size_high)
constexpr uint8_t kRfTxW[RF_TX_SIZES] = {4, 8, 16, 32, 64, 4, 8, 8, 16, 16, 32, 32, 64, 4, 16, 8, 32, 16, 64};
constexpr uint8_t kRfTxH[RF_TX_SIZES] = {4, 8, 16, 32, 64, 8, 4, 16, 8, 32, 16, 64, 32, 16, 4, 32, 8, 64, 16};
constexpr uint8_t kRfBsW[22] = {4, 4, 8, 8, 8, 16, 16, 16, 32, 32, 32, 64, 64, 64, 128, 128, 4, 16, 8, 32, 16, 64};
constexpr uint8_t kRfBsH[22] = {4, 8, 4, 8, 16, 8, 16, 32, 16, 32, 64, 32, 64, 128, 64, 128, 16, 4, 32, 8, 64, 16};
constexpr bool rf_bsize_ok(int bsize) { return bsize >= 0 && bsize < 22 && !(bsize >= 13 && bsize <= 15); }
constexpr int rf_tx_of(int w, int h) {
    for (int t = 0; t < RF_TX_SIZES; t++)
        if (kRfTxW[t] == w && kRfTxH[t] == h) return t;
    return -1;
}
constexpr int rf_max(int a, int b) { return a > b ? a : b; }
constexpr int rf_min(int a, int b) { return a < b ? a : b; }
// blk_geom->txsize[0]: the block size's own transform size (block sizes up to 64x64)
constexpr int rf_txsize(int bsize) { return rf_tx_of(kRfBsW[bsize], kRfBsH[bsize]); }
// blk_geom->txsize_uv[0]: the largest transform of the 4:2:0 chroma block (a side of at least 4), TX_64X64 adjusted to 32x32
constexpr int rf_uv_w(int bsize) { return rf_min(rf_max(kRfBsW[bsize] / 2, 4), 32); }
constexpr int rf_uv_h(int bsize) { return rf_min(rf_max(kRfBsH[bsize] / 2, 4), 32); }
constexpr int rf_txsize_uv(int bsize) { return rf_tx_of(rf_uv_w(bsize), rf_uv_h(bsize)); }
// is_txfm_allowed for a transform size
constexpr bool rf_type_ok(int tx_size, int tx_type) {
    if (tx_type < 0 || tx_type > 15) return false;
    const int m = rf_max(kRfTxW[tx_size], kRfTxH[tx_size]);
    return m == 64 ? tx_type == 0 : (m == 32 ? (tx_type == 0 || tx_type == 9) : true);
}

// work items a superblock can add to a size's list, and where the size's list starts (in items per superblock)
constexpr uint32_t rf_cap(int tx_size) { return 4096u / ((uint32_t)kRfTxW[tx_size] * kRfTxH[tx_size]) + 2u * (1024u / ((uint32_t)kRfTxW[tx_size] * kRfTxH[tx_size])); }
constexpr uint32_t rf_list_first(int tx_size) {
    uint32_t n = 0;
    for (int t = 0; t < tx_size; t++) n += rf_cap(t);
    return n;
}
constexpr uint32_t RF_ITEMS_PER_SB = rf_list_first(RF_TX_SIZES);
static_assert(RF_ITEMS_PER_SB == 1271 && (uint64_t)RF_MAX_NSB * RF_ITEMS_PER_SB < (1ull << 32) && (uint64_t)RF_MAX_NSB * RF_LUMA_SPAN <= (1ull << 32), "32-bit offsets");

inline size_t recon_final_scratch_bytes(uint32_t nsb) {
    if (nsb == 0 || nsb > RF_MAX_NSB) return 0;
    return (size_t)RF_COUNTER_BYTES + (size_t)nsb * RF_ITEMS_PER_SB * 16;
}

// the reconstruct launch of a transform size: 0 = both sides up to 16, 1 = a 32-sample side, 2 = a 64-sample side except 64x64, 3 = 64x64.
// 0 and 3 are register classes 0 and 2 of kernel_txfm_staged.h's tx_class_of, 1 and 2 the two halves of its class 1 (the kernels assert
// that they agree): the nine bodies of class 1 in one function left their register arrays in scratch, 2 392 bytes per lane.
constexpr int RF_LAUNCHES = 4;
constexpr int rf_class_of(int tx_size) {
    if (tx_size == 4) return 3;
    if (kRfTxW[tx_size] <= 16 && kRfTxH[tx_size] <= 16) return 0;
    return kRfTxW[tx_size] == 64 || kRfTxH[tx_size] == 64 ? 2 : 1;
}
// plane blocks a workgroup takes at a time: 64 / max(w, h) per wave, four waves, two for 64x64
constexpr uint32_t rf_per_wg(int tx_size) {
    return (uint32_t)((kRfTxW[tx_size] * kRfTxH[tx_size] >= 4096 ? 2 : 4) * (64 / rf_max(kRfTxW[tx_size], kRfTxH[tx_size])));
}
inline uint32_t recon_final_bin_grid(uint32_t nsb) { return (nsb + RF_BIN_WAVES - 1) / RF_BIN_WAVES; }
// workgroups of reconstruct launch cls: every workgroup's worth of items its lists can hold, at most RF_MAX_GRID (the workgroups stride)
inline uint32_t recon_final_class_grid(int cls, uint32_t nsb) {
    uint64_t n = 0;
    for (int t = 0; t < RF_TX_SIZES; t++)
        if (rf_class_of(t) == cls) n += ((uint64_t)rf_cap(t) * nsb + rf_per_wg(t) - 1) / rf_per_wg(t);
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
        if (!rf_bsize_ok(G.bsize)) return set_err(SVT_HIP_ERR_INVALID, "group %d: bsize %d", g, G.bsize);
        if (!rf_type_ok(rf_txsize_uv(G.bsize), G.tx_type_uv)) return set_err(SVT_HIP_ERR_INVALID, "group %d: tx_type_uv %d for bsize %d", g, G.tx_type_uv, G.bsize);
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

// av1_geom.h — what is AV1's and not any one call's: the sides of the 19 transform sizes and of the 22 block sizes, the block size of
// a width and height, the transform size of a block size and of its 4:2:0 chroma block (blocksize_to_txsize / av1_get_max_uv_txsize,
// EbUtility.c:110-138, :760-779), is_txfm_allowed, and the launch kind of a transform size.  THE statement of each: the host plans
// (md_plan.h, partition_plan.h, recon_final_plan.h, intra_encode_plan.h, dlf_plan.h) and host_tables.cpp read it as it is, the device
// table of the final-list readers (kernel_final_list.h) is built from it.  Host only (no HIP header), all constexpr.
#pragma once
#include <stdint.h>

#include "../../include/svt_hip_dsp.h"

namespace svthost {

// tx_size_wide / tx_size_high, and block_size_wide / block_size_high, size_group_lookup, num_pels_log2_lookup (EbDefinitions.h:1311, :1315)
constexpr int kTxW[SVT_TX_SIZES_ALL] = {4, 8, 16, 32, 64, 4, 8, 8, 16, 16, 32, 32, 64, 4, 16, 8, 32, 16, 64};
constexpr int kTxH[SVT_TX_SIZES_ALL] = {4, 8, 16, 32, 64, 8, 4, 16, 8, 32, 16, 64, 32, 16, 4, 32, 8, 64, 16};
constexpr uint8_t kBsizeW[22] = {4, 4, 8, 8, 8, 16, 16, 16, 32, 32, 32, 64, 64, 64, 128, 128, 4, 16, 8, 32, 16, 64};
constexpr uint8_t kBsizeH[22] = {4, 8, 4, 8, 16, 8, 16, 32, 16, 32, 64, 32, 64, 128, 64, 128, 16, 4, 32, 8, 64, 16};
constexpr uint8_t kSizeGroup[22] = {0, 0, 0, 1, 1, 1, 2, 2, 2, 3, 3, 3, 3, 3, 3, 3, 0, 0, 1, 1, 2, 2};
constexpr uint8_t kNumPelsLog2[22] = {4, 5, 5, 6, 7, 7, 8, 9, 9, 10, 11, 11, 12, 13, 13, 14, 6, 6, 8, 8, 10, 10};

constexpr int geom_max(int a, int b) { return a > b ? a : b; }
constexpr int geom_min(int a, int b) { return a < b ? a : b; }

// the block sizes of a 64x64 superblock: all but the three with a 128-sample side
constexpr bool bsize_ok(int bsize) { return bsize >= 0 && bsize < 22 && !(bsize >= 13 && bsize <= 15); }
// AV1 block_size of a width and height; 255: there is none
constexpr int bsize_of(int w, int h) {
    for (int b = 0; b < 22; b++)
        if (kBsizeW[b] == w && kBsizeH[b] == h) return b;
    return 255;
}
constexpr int tx_of(int w, int h) {
    for (int t = 0; t < SVT_TX_SIZES_ALL; t++)
        if (kTxW[t] == w && kTxH[t] == h) return t;
    return -1;
}
// blk_geom->txsize[0]: the block size's own transform size (block sizes up to 64x64)
constexpr int bsize_tx(int bsize) { return tx_of(kBsizeW[bsize], kBsizeH[bsize]); }
// blk_geom->txsize_uv[0]: the largest transform of the 4:2:0 chroma block (a side of at least 4), TX_64X64 adjusted to 32x32
constexpr int bsize_uv_w(int bsize) { return geom_min(geom_max(kBsizeW[bsize] / 2, 4), 32); }
constexpr int bsize_uv_h(int bsize) { return geom_min(geom_max(kBsizeH[bsize] / 2, 4), 32); }
constexpr int bsize_tx_uv(int bsize) { return tx_of(bsize_uv_w(bsize), bsize_uv_h(bsize)); }
// every block size bsize_ok admits has both: its transform has the block's sides, its chroma transform the chroma block's
constexpr bool bsize_tx_defined() {
    for (int b = 0; b < 22; b++)
        if (bsize_ok(b) && (bsize_tx(b) < 0 || bsize_tx_uv(b) < 0)) return false;
    return true;
}
static_assert(bsize_tx_defined(), "a transform size for every block size up to 64x64 and for its 4:2:0 chroma block");

// is_txfm_allowed (test/TxfmCommon.h:172-181; av1_estimate_transform's switch): a 64-sample side takes DCT_DCT only, a 32-sample
// side DCT_DCT and IDTX, the others all sixteen types.  By the transform's sides (no table: a kernel that holds a block's sides
// asks without a load that depends on another) and by its size.
constexpr bool tx_type_ok_sides(uint32_t w, uint32_t h, uint32_t tx_type) {
    const uint32_t m = w > h ? w : h;
    return tx_type < (uint32_t)SVT_TX_TYPES && (m == 64 ? tx_type == SVT_DCT_DCT : (m == 32 ? (tx_type == SVT_DCT_DCT || tx_type == SVT_IDTX) : true));
}
constexpr bool tx_type_ok(int tx_size, int tx_type) {
    return tx_size >= 0 && tx_size < SVT_TX_SIZES_ALL && tx_type >= 0 && tx_type_ok_sides((uint32_t)kTxW[tx_size], (uint32_t)kTxH[tx_size], (uint32_t)tx_type);
}

// the quantiser's log_scale of a transform size (av1_get_tx_scale): 1 above 256 pixels, 2 above 1024
constexpr int tx_log_scale(int tx_size) { return kTxW[tx_size] * kTxH[tx_size] > 1024 ? 2 : (kTxW[tx_size] * kTxH[tx_size] > 256 ? 1 : 0); }

// the launch kind of a transform size: 0 = both sides up to 16, 1 = a 32-sample side, 2 = a 64-sample side except 64x64, 3 = 64x64.
// 0 and 3 are register classes 0 and 2 of kernel_txfm_staged.h, 1 and 2 the two halves of its class 1 (asserted there, against the
// lists SVT_TX_CLASS0 / 1A / 1B): the nine bodies of class 1 in one function left their register arrays in scratch in the kernels
// that walk the final block list, the halves none.
constexpr int kTxLaunchKinds = 4;
constexpr int tx_launch_kind(int tx_size) {
    if (tx_size == SVT_TX_64X64) return 3;
    if (kTxW[tx_size] <= 16 && kTxH[tx_size] <= 16) return 0;
    return kTxW[tx_size] == 64 || kTxH[tx_size] == 64 ? 2 : 1;
}

// the quantised coefficients a superblock streams out per plane (d_sb_qcoeff): 4096 luma, a quarter for each chroma plane
constexpr uint32_t kSbLumaSpan = SVT_HIP_SB_QCOEFF_LUMA, kSbChromaSpan = SVT_HIP_SB_QCOEFF_LUMA / 4;

}  // namespace svthost

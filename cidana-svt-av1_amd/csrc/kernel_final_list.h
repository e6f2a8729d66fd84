// kernel_final_list.h — the final block list of a superblock (svt_hip_part_final, [slot][256] in coding order) on the device, stated
// once for its writer (partition_kernel) and its readers (recon_bin_kernel, ie_prepass_kernel, dlf_mi_kernel, and whatever walks the
// coded blocks next):
//   kGeomTab        the block and transform sizes of av1_geom.h and the md-scan blocks of partition_plan.h as one device table
//   FinalEntry      the 12-byte entry as three words: its load (mds clamped to 1 100), its store, the clamp of final_count
//   entry_geom      an entry's sides, chroma sides, has_uv, chroma origin and transform sizes; entry_inside, the plane-bounds test
//   stream_offsets  the running offsets of the entries' coefficients in the superblock's streams (a wave prefix sum)
// Which entries a reader skips, in which order it tests them and which advance the offsets are the reader's own rules.
#pragma once
#include <stddef.h>

#include "av1_geom.h"
#include "dev_common.h"
#include "partition_plan.h"

namespace svtdev {

constexpr int FL_MAX_FINAL = SVT_HIP_SB_MAX_FINAL, FL_BLOCKS = svthost::PART_BLOCKS, FL_TX_SIZES = SVT_TX_SIZES_ALL;

// per block size (zeros for the three bsize_ok refuses): luma and chroma transform size, sides, chroma sides; per md-scan block: its
// block size, has_uv as bits; per transform size: the launch kind
struct GeomDevTab {
    uint8_t tx[22], tx_uv[22], bw[22], bh[22], cw[22], ch[22];
    uint8_t kind[FL_TX_SIZES];
    uint8_t bsize_of[FL_BLOCKS];
    uint32_t has_uv[(FL_BLOCKS + 31) / 32];
};
constexpr GeomDevTab geom_dev_tab() {
    GeomDevTab T{};
    for (int b = 0; b < 22; b++) {
        if (!svthost::bsize_ok(b)) continue;
        T.tx[b] = (uint8_t)svthost::bsize_tx(b); T.tx_uv[b] = (uint8_t)svthost::bsize_tx_uv(b);
        T.bw[b] = svthost::kBsizeW[b]; T.bh[b] = svthost::kBsizeH[b];
        T.cw[b] = (uint8_t)svthost::bsize_uv_w(b); T.ch[b] = (uint8_t)svthost::bsize_uv_h(b);
    }
    for (int t = 0; t < FL_TX_SIZES; t++) T.kind[t] = (uint8_t)svthost::tx_launch_kind(t);
    const svthost::PartGeomTab G = svthost::part_geom_tab();
    for (int i = 0; i < FL_BLOCKS; i++) {
        T.bsize_of[i] = G.blk[i].bsize;
        if (G.blk[i].has_uv) T.has_uv[i >> 5] |= 1u << (i & 31);
    }
    return T;
}
static __device__ const GeomDevTab kGeomTab = geom_dev_tab();

// ---- the entry: mds | x << 16, y | bsize << 16 | part << 24, src ------------------------------------------------------------------------
static_assert(sizeof(svt_hip_part_final) == 12 && offsetof(svt_hip_part_final, mds_idx) == 0 && offsetof(svt_hip_part_final, x) == 2 &&
              offsetof(svt_hip_part_final, y) == 4 && offsetof(svt_hip_part_final, bsize) == 6 && offsetof(svt_hip_part_final, part) == 7 &&
              offsetof(svt_hip_part_final, src) == 8, "svt_hip_part_final as three words");
struct FinalEntry { uint32_t mds = 0, x = 0, y = 0, bsize_byte = 0, part = 0, src = SVT_HIP_PART_NO_SRC; };      // as built: no entry

__device__ __forceinline__ uint32_t final_count_of(const uint32_t* final_count, size_t slot) { return min(final_count[slot], (uint32_t)FL_MAX_FINAL); }
// entry k (below 256) of the superblock in `slot`; mds indexes inside the geometry whatever the word holds
__device__ __forceinline__ FinalEntry final_entry_load(const uint32_t* final_blk, size_t slot, uint32_t k) {
    const uint32_t* w = final_blk + 3 * (slot * FL_MAX_FINAL + k);
    const uint32_t w0 = w[0], w1 = w[1];
    FinalEntry e;
    e.mds = min(w0 & 0xffffu, (uint32_t)FL_BLOCKS - 1); e.x = w0 >> 16; e.y = w1 & 0xffffu; e.bsize_byte = (w1 >> 16) & 0xffu; e.part = w1 >> 24; e.src = w[2];
    return e;
}
__device__ __forceinline__ void final_entry_store(uint32_t* final_blk, size_t slot, uint32_t k, const FinalEntry& e) {
    uint32_t* w = final_blk + 3 * (slot * FL_MAX_FINAL + k);
    w[0] = e.mds | (e.x & 0xffffu) << 16;
    w[1] = (e.y & 0xffffu) | e.bsize_byte << 16 | e.part << 24;
    w[2] = e.src;
}

// ---- the geometry of an entry under a block size (the entry's own byte or the md-scan block's: the reader's choice) --------------------------
// (a block bsize_ok admits has its own transform size's sides, its chroma block the chroma transform's: is_txfm_allowed of either is
// svthost::tx_type_ok_sides of bw, bh / cw, ch)
struct EntryGeom { uint32_t bw, bh, cw, ch, cx, cy, txs, txs_uv; bool has_uv; };
__device__ __forceinline__ EntryGeom entry_geom(const FinalEntry& e, uint32_t bsize) {
    EntryGeom g;
    g.bw = kGeomTab.bw[bsize]; g.bh = kGeomTab.bh[bsize]; g.cw = kGeomTab.cw[bsize]; g.ch = kGeomTab.ch[bsize];
    g.txs = kGeomTab.tx[bsize]; g.txs_uv = kGeomTab.tx_uv[bsize];
    g.has_uv = (kGeomTab.has_uv[e.mds >> 5] >> (e.mds & 31)) & 1u;
    g.cx = ((e.x >> 3) << 3) >> 1; g.cy = ((e.y >> 3) << 3) >> 1;         // the chroma block of the 8x8 the block lies in
    return g;
}
// the luma block inside plane 0 and, for an entry with chroma, the chroma block inside each of the planes 1 .. nplanes - 1
__device__ __forceinline__ bool entry_inside(const FinalEntry& e, const EntryGeom& g, const uint32_t* width, const uint32_t* height, uint32_t nplanes) {
    bool inside = e.x + g.bw <= width[0] && e.y + g.bh <= height[0];
    if (nplanes >= 2 && g.has_uv) inside = inside && g.cx + g.cw <= width[1] && g.cy + g.ch <= height[1];
    if (nplanes >= 3 && g.has_uv) inside = inside && g.cx + g.cw <= width[2] && g.cy + g.ch <= height[2];
    return inside;
}

// ---- the stream offsets: exclusive prefix sums, in coding order, of what the entries before this one add ------------------------------------------
// add_y / add_uv: the lane's entry's coefficients (0 for an entry that adds none); run_y / run_uv: the totals of the wave's earlier rounds
__device__ __forceinline__ void stream_offsets(uint32_t add_y, uint32_t add_uv, int lane, uint32_t& run_y, uint32_t& run_uv, uint32_t& off_y, uint32_t& off_uv) {
    const uint32_t in_y = wave_scan_incl(add_y, lane), in_uv = wave_scan_incl(add_uv, lane);
    off_y = run_y + in_y - add_y; off_uv = run_uv + in_uv - add_uv;
    run_y += wave_scan_total(in_y); run_uv += wave_scan_total(in_uv);
}

}  // namespace svtdev

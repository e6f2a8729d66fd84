// svt_hip_partition.hip — svt_hip_partition_decide_frame: the d1 / d2 partition decision and the final block list of every superblock
// of a picture (partition_kernel, kernel_partition.h), one launch; svt_hip_blk_geom_mds, the block geometry on the host.  The checks,
// the launch shape and the geometry builder are partition_plan.h's.
#include <stddef.h>

#include "host_common.h"
#include "kernel_partition.h"

using namespace svtdev;
using namespace svthost;

static_assert(sizeof(svt_hip_md_decision) == 8 * PT_DEC_WORDS && offsetof(svt_hip_md_decision, cost) == 0, "partition_kernel reads the cost as word 0 of nine");
static_assert(sizeof(svt_hip_part_leaf) == 12 && offsetof(svt_hip_part_leaf, split_flag) == 2 && offsetof(svt_hip_part_leaf, tot_d1_blocks) == 3 &&
              offsetof(svt_hip_part_leaf, left_partition) == 4 && offsetof(svt_hip_part_leaf, above_partition) == 5 && offsetof(svt_hip_part_leaf, src) == 8,
              "svt_hip_part_leaf as three words");
static_assert(sizeof(svt_hip_part_sb) == 12 && offsetof(svt_hip_part_sb, leaf_count) == 4 && offsetof(svt_hip_part_sb, origin_x) == 6 &&
              offsetof(svt_hip_part_sb, origin_y) == 8, "svt_hip_part_sb as three words");
static_assert(sizeof(svt_hip_part_sq) == 16 && alignof(svt_hip_part_sq) == 8 && offsetof(svt_hip_part_sq, best_d1_blk) == 8 && offsetof(svt_hip_part_sq, part) == 10 &&
              offsetof(svt_hip_part_sq, split_flag) == 11 && offsetof(svt_hip_part_sq, tested) == 12, "svt_hip_part_sq as two words");
static_assert(sizeof(svt_hip_part_final) == 12 && offsetof(svt_hip_part_final, x) == 2 && offsetof(svt_hip_part_final, y) == 4 &&
              offsetof(svt_hip_part_final, bsize) == 6 && offsetof(svt_hip_part_final, part) == 7 && offsetof(svt_hip_part_final, src) == 8,
              "svt_hip_part_final as three words");
static_assert(sizeof(svt_hip_blk_geom) == 16, "svt_hip_blk_geom");

static const PartGeomTab g_geom = part_geom_tab();
static_assert(part_geom_tab().nblk == PART_BLOCKS && part_geom_tab().nsq == PART_SQUARES, "the scan of a 64x64 superblock");

extern "C" int svt_hip_blk_geom_mds(uint32_t mds_idx, svt_hip_blk_geom* out) {
    if (mds_idx >= (uint32_t)PART_BLOCKS || !out) return set_err(SVT_HIP_ERR_INVALID, "mds_idx %u (0 .. %d) or NULL out", mds_idx, PART_BLOCKS - 1);
    *out = g_geom.blk[mds_idx];
    return SVT_HIP_OK;
}

extern "C" int svt_hip_partition_decide_frame(const svt_hip_partition_args* a, void* stream) {
    if (int rc = require_init()) return rc;
    if (int rc = partition_check(a)) return rc;
    PartitionDesc D;
    D.sb = (const uint32_t*)a->d_sb; D.leaf = (const uint32_t*)a->d_leaf;
    D.decision = (const unsigned long long*)a->d_decision; D.cost = (const unsigned long long*)a->d_cost;
    D.bits = a->d_partition_bits;
    D.sq = (unsigned long long*)a->d_sq; D.final_count = a->d_final_count; D.final_blk = (uint32_t*)a->d_final;
    D.final_decision = (unsigned long long*)a->d_final_decision;
    D.nsb = a->nsb; D.nleaves = a->nleaves; D.nsrc = a->nsrc; D.lambda = a->lambda; D.pic_width = a->pic_width; D.pic_height = a->pic_height;
    D.slice_is_intra = a->slice_is_intra != 0;
    hipLaunchKernelGGL(partition_kernel, dim3(partition_grid(a->nsb)), dim3(PT_THREADS), 0, (hipStream_t)stream, D);
    return launch_status("partition_decide");
}

// svt_hip_fast_loop.hip — svt_hip_intra_fast_loop_frame: the intra candidates of the mode-decision fast loop (fast_loop_kernel,
// kernel_fast_loop.h), one launch per non-empty group.  What is left here: the candidate chunks and the launches (fast_loop_enqueue); the
// argument check is md_plan.h's.
#include "host_common.h"
#include "kernel_fast_loop.h"

using namespace svtdev;
using namespace svthost;

static_assert(sizeof(svt_hip_intra_blk) == sizeof(BipBlk), "svt_hip_intra_blk layout");

template <int W, int H>
static int fast_loop_launch(const FastLoopDev& fd, uint32_t wgs, uint32_t chunks, hipStream_t s) {
    hipLaunchKernelGGL((fast_loop_kernel<W, H>), dim3(wgs, chunks), dim3(64 * BIP_WAVES), 0, s, fd);
    return launch_status("intra_fast_loop");
}

// waves wanted in flight: a group of few large blocks splits its candidate list over blockIdx.y until it has about this many
static constexpr uint32_t kFastLoopTargetWaves = 8192;

int svthost::fast_loop_enqueue(const svt_hip_fast_loop_group* groups, int ngroups, int metric, int flavour, hipStream_t s) {
    for (int g = 0; g < ngroups; g++) {
        const svt_hip_fast_loop_group& G = groups[g];
        if (G.nblocks == 0) continue;
        const int w = kTxW[G.tx_size], h = kTxH[G.tx_size];
        FastLoopDev fd;
        memset(&fd, 0, sizeof(fd));
        fd.src = G.d_src; fd.src_xy = G.d_src_xy; fd.top = G.d_top_neigh; fd.left = G.d_left_neigh;
        fd.blks = (const BipBlk*)G.d_blocks; fd.dist = (unsigned long long*)G.d_dist; fd.pred = G.d_pred;
        fd.src_stride = G.src_stride; fd.nblocks = G.nblocks; fd.neigh_pitch = G.neigh_pitch; fd.ncand = G.ncand;
        fd.metric = metric == SVT_HIP_FAST_SAD ? FAST_SAD : (flavour == SVT_HIP_FLAVOUR_C ? FAST_SSD : FAST_SSD_WRAP);
        memcpy(fd.modes, G.modes, sizeof(fd.modes));
        memcpy(fd.deltas, G.angle_deltas, sizeof(fd.deltas));
        const uint32_t bpw = 64u / (uint32_t)bip_lanes_per_block(w, h);
        const uint32_t waves = (G.nblocks + bpw - 1) / bpw, wgs = (waves + BIP_WAVES - 1) / BIP_WAVES;
        uint32_t chunks = (kFastLoopTargetWaves + waves - 1) / waves;
        chunks = chunks < 1 ? 1 : (chunks > (uint32_t)G.ncand ? (uint32_t)G.ncand : chunks);
        fd.cpc = (int)(((uint32_t)G.ncand + chunks - 1) / chunks);
        chunks = ((uint32_t)G.ncand + (uint32_t)fd.cpc - 1) / (uint32_t)fd.cpc;
#define FL_LAUNCH(W, H) fast_loop_launch<W, H>(fd, wgs, chunks, s)
        auto launch = [&]() -> int { TX_SWITCH(G.tx_size, FL_LAUNCH) };
#undef FL_LAUNCH
        if (int rc = launch()) return rc;
    }
    return SVT_HIP_OK;
}

extern "C" int svt_hip_intra_fast_loop_frame(const svt_hip_fast_loop_group* groups, int ngroups, int metric, int flavour, void* stream) {
    if (int rc = require_init()) return rc;
    if (int rc = fast_loop_check(groups, ngroups, metric, flavour)) return rc;
    return fast_loop_enqueue(groups, ngroups, metric, flavour, (hipStream_t)stream);
}

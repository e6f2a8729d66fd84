// svt_hip_fast_loop.hip — svt_hip_intra_fast_loop_frame: the intra candidates of the mode-decision fast loop (fast_loop_kernel,
// kernel_fast_loop.h), one launch per non-empty group.
#include "host_common.h"
#include "kernel_fast_loop.h"

using namespace svtdev;
using namespace svthost;

static_assert(sizeof(svt_hip_intra_blk) == sizeof(BipBlk), "svt_hip_intra_blk layout");

int svthost::fast_loop_check(const svt_hip_fast_loop_group* groups, int ngroups, int metric, int flavour) {
    if (ngroups < 0 || (ngroups > 0 && !groups)) return set_err(SVT_HIP_ERR_INVALID, "NULL group list");
    if (metric != SVT_HIP_FAST_SAD && metric != SVT_HIP_FAST_SSD) return set_err(SVT_HIP_ERR_INVALID, "metric %d", metric);
    if (flavour != SVT_HIP_FLAVOUR_C && flavour != SVT_HIP_FLAVOUR_AVX2) return set_err(SVT_HIP_ERR_INVALID, "flavour %d", flavour);
    for (int g = 0; g < ngroups; g++) {
        const svt_hip_fast_loop_group& G = groups[g];
        if (G.tx_size < 0 || G.tx_size >= SVT_TX_SIZES_ALL) return set_err(SVT_HIP_ERR_INVALID, "group %d: tx_size %d", g, G.tx_size);
        const int w = kTxW[G.tx_size], h = kTxH[G.tx_size];
        if (metric == SVT_HIP_FAST_SSD && flavour == SVT_HIP_FLAVOUR_AVX2 && w != h)
            return set_err(SVT_HIP_ERR_INVALID, "group %d: AVX2-flavour SSD is defined for square sizes only (%dx%d)", g, w, h);
        if (G.ncand < 1 || G.ncand > SVT_HIP_FAST_LOOP_MAX_CANDIDATES) return set_err(SVT_HIP_ERR_INVALID, "group %d: ncand %d (1 .. 64)", g, G.ncand);
        for (int c = 0; c < G.ncand; c++) {
            const int m = G.modes[c], a = G.angle_deltas[c];
            if (m > 12) return set_err(SVT_HIP_ERR_INVALID, "group %d: candidate %d: mode %d", g, c, m);
            if (a < -3 || a > 3) return set_err(SVT_HIP_ERR_INVALID, "group %d: candidate %d: angle delta %d", g, c, a);
            if (a != 0 && (m < 1 || m > 8)) return set_err(SVT_HIP_ERR_INVALID, "group %d: candidate %d: angle delta on mode %d", g, c, m);
        }
        if (G.nblocks == 0) continue;
        if (G.nblocks > 0x7fffffffu) return set_err(SVT_HIP_ERR_INVALID, "group %d: nblocks too large", g);
        if (!G.d_src || !G.d_top_neigh || !G.d_left_neigh || !G.d_blocks || !G.d_dist) return set_err(SVT_HIP_ERR_INVALID, "group %d: NULL member", g);
        if (((uintptr_t)G.d_dist & 7) || ((uintptr_t)G.d_pred & 15))
            return set_err(SVT_HIP_ERR_INVALID, "group %d: misaligned output (d_dist 8 bytes, d_pred 16 bytes)", g);
        if (G.neigh_pitch < 1 + 2 * (w > h ? w : h))
            return set_err(SVT_HIP_ERR_INVALID, "group %d: neigh_pitch %d < %d", g, G.neigh_pitch, 1 + 2 * (w > h ? w : h));
        if (G.d_src_xy && G.src_stride < (uint32_t)w) return set_err(SVT_HIP_ERR_INVALID, "group %d: src_stride below the block width", g);
    }
    return SVT_HIP_OK;
}

template <int W, int H>
static int fast_loop_launch(const FastLoopDev& fd, uint32_t wgs, uint32_t chunks, hipStream_t s) {
    hipLaunchKernelGGL((fast_loop_kernel<W, H>), dim3(wgs, chunks), dim3(64 * BIP_WAVES), 0, s, fd);
    return launch_status("intra_fast_loop");
}

// waves wanted in flight: a group of few large blocks splits its candidate list over blockIdx.y until it has about this many
static constexpr uint32_t kFastLoopTargetWaves = 8192;

extern "C" int svt_hip_intra_fast_loop_frame(const svt_hip_fast_loop_group* groups, int ngroups, int metric, int flavour, void* stream) {
    if (int rc = require_init()) return rc;
    if (int rc = fast_loop_check(groups, ngroups, metric, flavour)) return rc;
    hipStream_t s = (hipStream_t)stream;
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

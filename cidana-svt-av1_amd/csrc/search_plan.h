// search_plan.h — what the SAD search (svt_hip_sad_search_batch / _planes_batch) and the motion-search calls (svt_hip_me_sb_search_*,
// svt_hip_me_fullpel_search_*, svt_hip_hme_level_*, svt_hip_motion_estimate_frame) settle on the host before they enqueue: the LDS layout
// of each kernel, the kernel a shape is routed to with its grid, threads and dynamic LDS, and the window of the motion search.  The layout
// functions are constexpr and are called by the kernels too (kernel_pixel.h, kernel_me_steps.h), so a pitch has one statement.  Host
// only otherwise (no HIP header): tests/c/search_plan_host.cpp compiles it with g++.  Everything else the motion-search calls decide - their
// refusals in order, the kernel of a full-pel search, the grids, the frame call's plan - is me_plan.h's, which builds on the windows here;
// the SAD / SSE / residual / distortion calls' is pixel_plan.h's.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "../../include/svt_hip_dsp.h"
#include "host_err.h"

namespace svthost {

// ---- SAD search: LDS layout (host and kernels) ------------------------------------------------------------------------------------------
constexpr uint32_t SAD_LDS_MAX = 64 * 1024;              // a workgroup's LDS

// rows of the window a block's candidates touch: search_h + height - 1 overlapping rows, or, for a line-skipping caller (ref_stride !=
// ref_stride_raw), row ys * height + y = address ys * ref_stride_raw + y * ref_stride, search_h * height of them
// (T: uint64_t on the host, where the product of two caller values must not wrap; uint32_t in the kernels, which run accepted shapes only)
template <typename T>
constexpr T sad_nrows(bool plain, T search_h, T height) { return plain ? search_h + height - 1 : search_h * height; }
// 16-byte chunks of a window row, and the multiplier that makes j / cpr one __umulhi for j < 2^16 (cpr <= 8 there): floor(2^32 / cpr) + 1
constexpr uint32_t sad_cpr(uint32_t win_w) { return (win_w + 15) >> 4; }
constexpr uint32_t sad_cpr_magic(uint32_t cpr) { return (uint32_t)(0x100000000ull / cpr) + 1u; }

// sad_search_kernel: rows of a multiple of 4 bytes + 4 spare; the source block at a pitch of whole dwords
constexpr uint32_t sad_plain_wpitch(uint32_t win_w) { return (win_w + 3 + 8) & ~3u; }
constexpr uint32_t sad_plain_spitch(uint32_t width) { return (width + 3) & ~3u; }
constexpr uint32_t sad_plain_src_bytes(uint32_t width, uint32_t height) { return (sad_plain_spitch(width) * height + 15) & ~15u; }
// sad_search_q_kernel, sad_search_q2_kernel: whole 16-byte chunks + one chunk of slack for the sliding reads; the source block dense
constexpr uint32_t sad_q_wpitch(uint32_t win_w) { return ((win_w + 15) & ~15u) + 16; }
constexpr uint32_t sad_q_src_bytes(uint32_t width, uint32_t height) { return (width * height + 15) & ~15u; }
// window bytes of the plain and the q kernel: the rows + 16 bytes that the last row's sliding read may touch
constexpr uint64_t sad_ref_bytes(uint32_t wpitch, uint64_t nrows) { return (wpitch * nrows + 16 + 15) & ~(uint64_t)15; }
// sad_search_q2_kernel: window + one spare row (a row pair without a second row) + 16 spare bytes per lane, padded to 8 (mod 32) bytes: the
// stride from one block's window to the next (LDS bank spread, see the kernel)
constexpr uint64_t sad_q2_ref_bytes(uint32_t wpitch, uint64_t nrows, uint32_t lpb) { return ((wpitch * (nrows + 1) + 16 * lpb + 31) & ~(uint64_t)31) + 8; }
// sad_search_q2p_kernel: source blocks 16 bytes apart from a multiple of 256; window rows of 16 * cpr + 8 bytes; the stride from one
// block's window to the next == 64 (mod 128), the window + 8 bytes (every second pair of blocks starts 8 bytes further on) fitting in it
constexpr uint32_t sad_q2p_src_bytes(uint32_t width, uint32_t height) { return sad_q_src_bytes(width, height) + 16; }
constexpr uint32_t sad_q2p_wpitch(uint32_t win_w) { return 16 * sad_cpr(win_w) + 8; }
constexpr uint64_t sad_q2p_wstride(uint32_t wpitch, uint64_t nrows) {
    const uint64_t need = wpitch * nrows + 8, s = ((need + 63) & ~(uint64_t)127) + 64;
    return s < need ? s + 128 : s;
}
// sad_search_q16_kernel: the search width in whole 16-byte chunks + the block width, an odd multiple of 16 bytes (bank spread over search
// rows); the source block dense
constexpr uint32_t sad_q16_wpitch(uint32_t search_w, uint32_t width) {
    const uint32_t p = ((search_w + 15) & ~15u) + width;
    return ((p >> 4) & 1) == 0 ? p + 16 : p;
}
constexpr uint32_t sad_q16_src_bytes(uint32_t width, uint32_t height) { return width * height; }

// ---- SAD search: the routing --------------------------------------------------------------------------------------------------------------
enum SadSearchKernel { SAD_K_PLAIN, SAD_K_Q, SAD_K_Q16, SAD_K_Q2, SAD_K_Q2P };
struct SadSearchKnobs { int no_qsad, no_q2, no_q2p, no_q16, q2_su4; };       // svt_hip_tune
struct SadSearchPlan {
    int kernel;                      // SadSearchKernel
    int cw, ch, su;                  // the template variant: <CW, CH> of q (0, 0: any size) / q2 / q2p, <CW> of q16, <.., Q2_SU> of q2
    uint32_t grid, threads;
    size_t lds;                      // dynamic LDS of a workgroup
    // what the launch passes that follows from the shape (each kernel takes the ones it names)
    uint32_t src_bytes, ref_bytes;   // src_lds_bytes / ref_lds_bytes
    uint32_t wpitch, wstride;        // q16, q2p
    uint32_t lpb, tsh, cpr_magic;
    // the layout behind lds (tests/c/search_plan_host.cpp): blocks of a workgroup, their bytes, window rows
    uint32_t slots, per_blk, nrows;
};

// lanes of a block: the power of two >= groups, at most a wave
constexpr uint32_t sad_lanes(uint64_t groups) {
    uint32_t lpb = 1;
    while (lpb < groups && lpb < 64) lpb <<= 1;
    return lpb;
}
// threads of a workgroup of `lpb`-lane blocks of per_blk bytes: 256, halved until the blocks fit the LDS or one block is left
constexpr uint32_t sad_threads(uint32_t lpb, uint64_t per_blk, uint32_t floor) {
    uint32_t threads = 256;
    while (threads > floor && (threads / lpb) * per_blk > SAD_LDS_MAX) threads >>= 1;
    return threads;
}

// the *_planes_batch form of a search addresses its blocks by two offset tables
inline int search_offsets_check(bool need_offs, const void* d_src_offs, const void* d_ref_offs) {
    if (need_offs && (!d_src_offs || !d_ref_offs)) return set_err(SVT_HIP_ERR_INVALID, "NULL offset table");
    return SVT_HIP_OK;
}
// the SAD search's pointers
inline int sad_search_args_check(bool need_offs, const void* d_src_offs, const void* d_ref_offs, const void* d_src, const void* d_ref, const void* d_best_sad,
                                 const void* d_x, const void* d_y) {
    if (int rc = search_offsets_check(need_offs, d_src_offs, d_ref_offs)) return rc;
    if (!d_src || !d_ref || !d_best_sad || !d_x || !d_y) return set_err(SVT_HIP_ERR_INVALID, "NULL buffer");
    return SVT_HIP_OK;
}

// Every refusal of the SAD search that needs no pointer, then the kernel and its launch.  All byte and row counts are 64-bit: a
// line-skipping window of search_h * height rows can pass 2^32 bytes, and is refused like any other window over 64 KiB.
inline int sad_search_plan(uint32_t width, uint32_t height, int search_w, int search_h, bool plain, size_t nblocks, const SadSearchKnobs& k, int num_cu,
                           SadSearchPlan& p) {
    p = SadSearchPlan{};
    if (width == 0 || height == 0 || width > 64 || height > 64) return set_err(SVT_HIP_ERR_INVALID, "block %ux%u", width, height);
    if (search_w <= 0 || search_h <= 0 || search_w > 32767 || search_h > 32767) return set_err(SVT_HIP_ERR_INVALID, "empty search area");
    const uint32_t sw = (uint32_t)search_w, sh = (uint32_t)search_h;
    const uint32_t win_w = width + sw - 1, cpr = sad_cpr(win_w);
    const uint64_t nrows = sad_nrows<uint64_t>(plain, sh, height);
    p.nrows = (uint32_t)nrows;                            // (exact in every accepted plan: nrows * pitch <= 64 KiB)
    p.cpr_magic = sad_cpr_magic(cpr);
    auto launch = [&](int kernel, int cw, int ch, int su, uint32_t threads, uint32_t slots, uint64_t per_blk) {
        p.kernel = kernel; p.cw = cw; p.ch = ch; p.su = su;
        p.threads = threads; p.slots = slots; p.per_blk = (uint32_t)per_blk;
        p.lds = (size_t)(slots * per_blk);
        p.grid = (uint32_t)((nblocks + slots - 1) / slots);
        return SVT_HIP_OK;
    };
    const bool q16_for_16x16 = !k.no_q16 && width == 16 && sw % 16 == 0;      // see the q16 routing below
    if (plain && !k.no_qsad && !k.no_q2 && ((width == 16 && height == 16 && !q16_for_16x16) || (width == 8 && height == 8))) {
        // small blocks: source block in registers, 4 x 2 candidates per lane
        const uint32_t src_bytes = sad_q_src_bytes(width, height);
        const uint32_t lpb = sad_lanes((uint64_t)((sw + 3) / 4) * ((sh + 1) / 2));
        const uint64_t ref_bytes = sad_q2_ref_bytes(sad_q_wpitch(win_w), nrows, lpb), per_blk = src_bytes + ref_bytes;
        if (per_blk <= SAD_LDS_MAX) {
            p.lpb = lpb;
            // staging depth: all of a lane's chunks in ONE batch of loads when that takes at most 8 per lane (one memory
            // latency per block instead of two: the kernel is latency-bound at 3 waves per SIMD)
            const uint64_t nchunk = cpr * nrows;
            const bool deep = !k.q2_su4 && nchunk > 4 * lpb;
            // persistent, software-pipelined form (loads of the next set of blocks in flight during the search): whenever a
            // lane's share of one block's chunks fits 8 registers-of-16-B
            const uint32_t nsrc_chunks = width * height / (width % 16 == 0 ? 16u : 8u);
            if (!k.no_q2p && nsrc_chunks + nchunk <= 8 * lpb && sw <= 256 && sh <= 256) {
                const uint32_t wpitch_p = sad_q2p_wpitch(win_w);
                const uint64_t wstride = sad_q2p_wstride(wpitch_p, nrows), per_blk_p = sad_q2p_src_bytes(width, height) + wstride;
                const uint32_t pthreads = sad_threads(lpb, per_blk_p, 64), pslots = pthreads / lpb, pwaves = pthreads / 64;
                const uint64_t plds = pslots * per_blk_p;
                if (pslots >= pwaves && plds <= SAD_LDS_MAX) {
                    launch(SAD_K_Q2P, (int)width, (int)height, 0, pthreads, pslots, per_blk_p);
                    p.wpitch = wpitch_p; p.wstride = (uint32_t)wstride;
                    // a wave owns 64 / lpb blocks at a time (a set); as many workgroups as the device holds at once, by LDS (160 KiB per
                    // CU) and by waves (4 per SIMD at 124 VGPRs), or fewer when the sets run out
                    const uint32_t nsets = (uint32_t)((nblocks + 64 / lpb - 1) / (64 / lpb));
                    const uint32_t wg_per_cu = (uint32_t)(160 * 1024 / plds), by_waves = 16 / pwaves;
                    const uint32_t need = (nsets + pwaves - 1) / pwaves;
                    p.grid = (uint32_t)num_cu * (wg_per_cu < by_waves ? (wg_per_cu ? wg_per_cu : 1) : by_waves);
                    if (p.grid > need) p.grid = need;
                    return SVT_HIP_OK;
                }
            }
            p.ref_bytes = (uint32_t)ref_bytes;
            const uint32_t threads = sad_threads(lpb, per_blk, lpb);
            return launch(SAD_K_Q2, (int)width, (int)height, deep ? 8 : 4, threads, threads / lpb, per_blk);
        }
    }
    // 16-wide blocks: 16x32 / 16x64 always (measured 2.1-2.3x over sad_search_q_kernel); 16x16 when no candidate
    // of a lane is masked (search width % 16 == 0: 10 % over q2, equal otherwise)
    if (plain && !k.no_qsad && !k.no_q16 && height % (256 / width) == 0 &&
        (width == 32 || width == 64 || (width == 16 && (height != 16 || sw % 16 == 0)))) {
        // wide blocks: 16 candidates per lane on b128 LDS reads (sad_search_q16_kernel)
        const uint32_t wpitch = sad_q16_wpitch(sw, width);
        const uint64_t ref_bytes = wpitch * nrows, per_blk = sad_q16_src_bytes(width, height) + ref_bytes;
        if (per_blk <= SAD_LDS_MAX) {
            // 2^tsh lanes take the tasks (16 candidates of a search row); a block with few tasks still fills its lanes by splitting its
            // row groups over lpb >> tsh lanes per task
            const uint64_t tasks = (uint64_t)((sw + 15) / 16) * sh;
            uint32_t tsh = 0;
            while ((1u << tsh) < tasks && tsh < 6) tsh++;
            const uint32_t row_groups = height / (256 / width);
            uint32_t lpb = 1u << tsh;
            while (lpb < 64 && (lpb >> tsh) * 2 <= row_groups) lpb <<= 1;
            p.wpitch = wpitch; p.ref_bytes = (uint32_t)ref_bytes; p.lpb = lpb; p.tsh = tsh;
            const uint32_t threads = sad_threads(lpb, per_blk, lpb);
            return launch(SAD_K_Q16, (int)width, 0, 0, threads, threads / lpb, per_blk);
        }
    }
    if ((width & 3) == 0 && !k.no_qsad) {
        // quad-SAD kernel: 4 candidates per lane
        const uint32_t src_bytes = sad_q_src_bytes(width, height);
        const uint64_t ref_bytes = sad_ref_bytes(sad_q_wpitch(win_w), nrows), per_blk = src_bytes + ref_bytes;
        if (per_blk > SAD_LDS_MAX)
            return set_err(SVT_HIP_ERR_INVALID, "search window needs %llu B of LDS per block (> 64 KiB)", (unsigned long long)per_blk);
        const uint32_t lpb = sad_lanes((uint64_t)((sw + 3) / 4) * sh);
        p.src_bytes = src_bytes; p.ref_bytes = (uint32_t)ref_bytes; p.lpb = lpb;
        const bool sq = width == height && (width == 8 || width == 16 || width == 32 || width == 64);
        const uint32_t threads = sad_threads(lpb, per_blk, lpb);
        return launch(SAD_K_Q, sq ? (int)width : 0, sq ? (int)height : 0, 0, threads, threads / lpb, per_blk);
    }
    // one wave per block, up to four blocks per workgroup
    const uint32_t src_bytes = sad_plain_src_bytes(width, height);
    const uint64_t ref_bytes = sad_ref_bytes(sad_plain_wpitch(win_w), nrows), per_wave = src_bytes + ref_bytes;
    if (per_wave > SAD_LDS_MAX)
        return set_err(SVT_HIP_ERR_INVALID, "search window needs %llu B of LDS per block (> 64 KiB)", (unsigned long long)per_wave);
    p.src_bytes = src_bytes; p.ref_bytes = (uint32_t)ref_bytes; p.lpb = 64;
    const uint32_t waves = SAD_LDS_MAX / per_wave > 4 ? 4 : (uint32_t)(SAD_LDS_MAX / per_wave);
    return launch(SAD_K_PLAIN, 0, 0, 0, waves * 64, waves, per_wave);
}

// ---- motion search: the window in LDS (host and kernels) ----------------------------------------------------------------------------------
// Every motion-search kernel keeps the even rows of the 64x64 source block at the start of its dynamic LDS and the reference window behind them.
constexpr uint32_t ME_SRC_LDS = 32 * 64;
// The dynamic LDS a launch may ask for.  No reason is recorded for either figure; what they leave of a workgroup's 64 KiB goes to the kernels'
// static tables (the per-wave keys of the 85 square PUs, 1 360 B; the all-PU search's batches, 3 840 B more).
constexpr size_t ME_LDS_MAX = 60 * 1024;                 // the square-PU search (me_sb_search16_kernel) and the HME levels
constexpr size_t ME_NSQ_LDS_MAX = 58 * 1024;             // the all-PU search (me_nsq4_kernel) and the per-SB areas (me_fullpel_areas_kernel, svt_hip_motion_estimate_frame)

// Row pitch of the reference window the motion-search kernels stage in LDS: whole 16-byte chunks + one chunk of slack for the
// sliding reads, and == 64 (mod 128) so that the lanes of consecutive SEARCH ROWS fall on different halves of the 32 banks.  A
// wave's b128 reads are served eight lanes at a time - four 16-point groups of one search row and four of the next - and with
// the first pitch (144 B for a 64-wide area, == 16 mod 128) the second row's lanes landed on the first row's banks: 31 % of the
// kernel's LDS cycles were bank conflicts (profiles/r03_a_pmc_me_sb.json); the 4-points-per-lane kernel's dword reads (16 lanes
// per search row) collide the same way.
constexpr uint32_t me_window_pitch(uint32_t win_w) {
    uint32_t p = ((win_w + 15) & ~15u) + 16;
    while ((p & 127) != 64) p += 16;
    return p;
}
// the HME levels read dwords: rows of whole dwords + 8 bytes of slack
constexpr uint32_t hme_window_pitch(uint32_t win_w) { return ((win_w + 3) & ~3u) + 8; }

struct MeWindow { uint32_t wpitch, pair_off; size_t lds; };
struct HmeWindow { uint32_t wpitch; size_t lds; };

// The window of a search_w x search_h area round a 64x64 block.  Each side is bounded before the two are multiplied: 1 .. 4096 points (the
// kernels' 12-bit point index).  nsq_pairs: room behind the window for the (64x32_1, 32x16_5) pairs of the narrow single-point areas,
// <= 7 x search_h points of 8 bytes (me_nsq4_body).  The LDS limit is the caller's: me_window_check, or a fall-through to another kernel.
inline int me_window(int search_w, int search_h, int nsq_pairs, MeWindow& w) {
    w = MeWindow{};
    if (search_w < 1 || search_h < 1 || search_w > 4096 || search_h > 4096 || search_w * search_h > 4096)
        return set_err(SVT_HIP_ERR_INVALID, "search area %dx%d (1..4096 points)", search_w, search_h);
    const uint32_t win_w = 64 + (uint32_t)search_w - 1, win_h = 64 + (uint32_t)search_h - 1;
    w.wpitch = me_window_pitch(win_w);
    w.lds = ME_SRC_LDS + (size_t)w.wpitch * win_h;
    if (nsq_pairs) {
        w.pair_off = (uint32_t)((w.lds + 15) & ~(size_t)15);
        w.lds = w.pair_off + (size_t)8 * 7 * (uint32_t)search_h;
    }
    return SVT_HIP_OK;
}
inline int me_window_check(int search_w, int search_h, int nsq_pairs, size_t lds_max, MeWindow& w) {
    if (int rc = me_window(search_w, search_h, nsq_pairs, w)) return rc;
    if (w.lds > lds_max)
        return set_err(SVT_HIP_ERR_INVALID, "search window of %dx%d needs %zu B of LDS (> %zu KiB)", search_w, search_h, w.lds, lds_max / 1024);
    return SVT_HIP_OK;
}

// The window of one HME launch: the widest region's pitch for all of them, the tallest window at that pitch.  The clipped area never exceeds
// the nominal one; blocks are at most 64 x 64 (32 compared rows, every other one: search_area_height + 62 window rows).
inline int hme_window(const svt_hip_hme_params* params, int nregions, HmeWindow& w) {
    w = HmeWindow{0, ME_SRC_LDS};
    for (int r = 0; r < nregions; r++) {
        if (params[r].search_area_width < 1 || params[r].search_area_height < 1 || params[r].search_area_width > 4096 || params[r].search_area_height > 4096)
            return set_err(SVT_HIP_ERR_INVALID, "HME search area %dx%d (1..4096 each)", params[r].search_area_width, params[r].search_area_height);
        const uint32_t wp = hme_window_pitch(64 + (uint32_t)params[r].search_area_width - 1);
        if (wp > w.wpitch) w.wpitch = wp;
    }
    for (int r = 0; r < nregions; r++) {
        const size_t need = ME_SRC_LDS + (size_t)w.wpitch * ((uint32_t)params[r].search_area_height + 62);
        if (need > w.lds) w.lds = need;
    }
    if (w.lds > ME_LDS_MAX) return set_err(SVT_HIP_ERR_INVALID, "HME search window needs %zu B of LDS (> %zu KiB)", w.lds, ME_LDS_MAX / 1024);
    return SVT_HIP_OK;
}

}  // namespace svthost

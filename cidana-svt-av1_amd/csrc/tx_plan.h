// tx_plan.h — what the transform family (svt_hip_txfm.hip: forward / inverse transforms, 64-point packing, quantiser, the fused chains and the
// frame call) settles on the host before it enqueues: the launch geometry of every kernel family, stated once, and one plan per public entry
// point: every refusal that needs no pointer, then the kernel a shape is routed to with its template variant, grid and threads.  A plan
// sees values only: shapes, which optional members are present, whether a pointer group is 16-byte aligned.  Host only (no HIP header):
// tests/c/tx_plan_host.cpp compiles it with g++; the kernel headers static_assert their constants against the geometry below.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "../../include/svt_hip_dsp.h"
#include "av1_geom.h"
#include "host_err.h"
#include "quant_params.h"

namespace svthost {
using svtdev::QParams;

// ---- launch geometry: waves and blocks per workgroup of each kernel family ------------------------------------------------------------------
// general kernels (kernel_txfm.h: TX_WAVES waves, a wave takes the 64 / max(W, H) blocks of TxGeom<W, H>::BPW)
constexpr int kTxWaves = 4;
constexpr uint32_t tx_blocks_per_wave(int w, int h) { return (uint32_t)(64 / geom_max(w, h)); }
constexpr uint32_t tx_general_blocks_per_wg(int tx_size) { return kTxWaves * tx_blocks_per_wave(kTxW[tx_size], kTxH[tx_size]); }
// staged kernels and bodies (kernel_txfm_staged.h, enc_staged_body, full_loop_body): StagedGeom<W, H>::WAVES waves of TxGeom<W, H>::BPW blocks
constexpr int tx_staged_waves(int w, int h) { return w * h >= 4096 ? 2 : 4; }
constexpr uint32_t tx_staged_blocks_per_wg(int w, int h) { return (uint32_t)tx_staged_waves(w, h) * tx_blocks_per_wave(w, h); }
constexpr uint32_t tx_staged_blocks_per_wg(int tx_size) { return tx_staged_blocks_per_wg(kTxW[tx_size], kTxH[tx_size]); }
// the 32x32 pair kernels (kernel_fused32.h): F32_WAVES waves of two blocks; the inverse's tuning probes run `waves` of them
constexpr int kF32Waves = 4;
constexpr uint32_t f32_blocks_per_wg(int waves = kF32Waves) { return 2u * (uint32_t)waves; }
// the 64x64 pair kernels (kernel_enc64.h): E64_WAVES waves of two blocks
constexpr int kE64Waves = 2;
constexpr uint32_t kE64BlocksPerWg = 2 * kE64Waves;
// enc4_kernel: one block per lane of a 256-thread workgroup
constexpr uint32_t kEnc4BlocksPerWg = 256;
// quantize_b_kernel<L>: L = min(64, n_coeffs / 4) lanes per block when that is a power of two, else a wave; four waves of 64 / L blocks
constexpr int quantize_b_lanes(int n_coeffs) {
    const int l = n_coeffs / 4;
    return l == 4 || l == 8 || l == 16 || l == 32 ? l : 64;
}
constexpr uint32_t quantize_b_blocks_per_wg(int lanes) { return 4u * (uint32_t)(64 / lanes); }
// blocks one 256-thread workgroup of an enc_frame_kernel body takes: 4x4 one block per lane; 32x32 and 64x64 the pair kernels'; the staged bodies'
constexpr uint32_t frame_blocks_per_wg(int tx_size) {
    return tx_size == SVT_TX_4X4 ? kEnc4BlocksPerWg : tx_size == SVT_TX_32X32 ? f32_blocks_per_wg() : tx_size == SVT_TX_64X64 ? kE64BlocksPerWg
                                                                                                                             : tx_staged_blocks_per_wg(tx_size);
}
// register class of the group-table launches (kernel_txfm_staged.h's tx_class_of, asserted there): 0 both sides <= 16, 2 64x64, 1 the rest
constexpr int tx_class(int tx_size) { return tx_launch_kind(tx_size) == 0 ? 0 : (tx_launch_kind(tx_size) == 3 ? 2 : 1); }

// ---- the knobs this family reads (svt_hip_tune) ----------------------------------------------------------------------------------------------
struct TxKnobs {
    int no_staged, no_f32p, no_inv_planes, no_enc_staged, no_enc64, f32_wg_per_cu, f32_nt, f32_qmode1, inv32_waves, inv32_var, frame_single_launch;
};
constexpr TxKnobs kTxKnobDefaults = {0, 0, 0, 0, 0, 0, 0, 0, 4, 0, -1};

// ---- routes ---------------------------------------------------------------------------------------------------------------------------------
enum TxRoute {
    TXR_FWD32,             // fwd32_kernel<0, false, false>
    TXR_FWD_STAGED,        // fwd_staged_kernel<W, H, 0>
    TXR_FWD_GENERAL,       // fwd_txfm2d_kernel<W, H>
    TXR_PACK64_NONE,       // no 64-sample side: the energy (if asked for) is zeroed, nothing is launched
    TXR_PACK64,            // pack64_kernel
    TXR_INV32,             // inv32_kernel<T, BD>
    TXR_INV32_PROBE,       // inv32_kernel<uint8_t, 8, WV, VR>
    TXR_INV_STAGED,        // inv_staged_kernel<W, H, T, T16>
    TXR_INV_GENERAL,       // inv_txfm2d_add_kernel<W, H, T, WIDE>
    TXR_QUANTIZE_B,        // quantize_b_kernel<L>
    TXR_FQ32,              // fwd32_kernel<1, true, SAD, NT, QMODE>: the headline chain
    TXR_FQ32_PLANES,       // fwd32_kernel<INM, true, SAD, false, 2, PLANES>
    TXR_FQ64,              // fq64_kernel<T, BD>
    TXR_FQ_STAGED,         // fwd_staged_kernel<W, H, 1, T>
    TXR_FQ_GENERAL,        // fwd_quant_generic_kernel<W, H, T>
    TXR_ENC32,             // enc32_kernel<T, BD, KEEP, SAD>
    TXR_ENC4,              // enc4_kernel<T, BD, KEEP>
    TXR_ENC64,             // enc64_kernel<T, BD, KEEP, SAD>
    TXR_ENC_STAGED,        // enc_staged_kernel<W, H, KEEP, T, BD>
    TXR_ENC_COMPOSED,      // stage[0]: forward + quantise; a device copy of the prediction; stage[1]: inverse
    TXR_FWD32_QUANT,       // fwd32_kernel<0, true, false>
    TXR_FWD_THEN_QUANT,    // stage[0]: forward transform into d_coeff; stage[1]: quantize_b
    TXR_COUNT
};

struct TxPlan {
    int route;             // TxRoute
    uint32_t grid, threads;
    uint32_t per_wg;       // blocks of a workgroup (tests/c/tx_plan_host.cpp)
    bool grid_capped;      // f32_wg_per_cu holds the grid below nblocks / per_wg on purpose (the kernel strides)
    // the template variant
    int is16, bd;          // sample type (uint8_t / uint16_t) and the depth the kernel is built for
    bool keep, sad, nt, planes, wide, t16, fast;
    int qmode, inm, wv, vr, lanes;
    // what the launch passes that follows from the shape
    int idtx, log_scale;
    uint32_t src_stride, pred_stride;
    QParams qp;            // the routes that quantise
};

constexpr uint64_t kTxMaxBlocks = 0x7fffffffu;
constexpr uint32_t tx_grid(uint64_t nblocks, uint32_t per_wg) { return (uint32_t)((nblocks + per_wg - 1) / per_wg); }      // (nblocks bounded first)

// a negative quant_shift, dequant or (rounded) round entry: outside the 24-bit arithmetic of the fused kernels (dev_common.h
// quant_one<1 / 2>).  Each plan decides what that means: an error, or another kernel.
inline bool qparams_negative(const QParams& qp) {
    for (int i = 0; i < 2; i++)
        if (qp.quant_shift[i] < 0 || qp.dequant[i] < 0 || qp.round[i] < 0) return true;
    return false;
}
inline QParams tx_qparams(const svt_hip_qrows& q, int log_scale) { return svtdev::make_qparams(q.zbin, q.round, q.quant, q.quant_shift, q.dequant, log_scale); }
constexpr bool tx_is_32x32_pair(int tx_size, int tx_type) { return tx_size == SVT_TX_32X32 && (tx_type == SVT_DCT_DCT || tx_type == SVT_IDTX); }

namespace txplan_detail {
inline int launch(TxPlan& p, int route, uint64_t nblocks, uint32_t per_wg, uint32_t threads) {
    p.route = route; p.per_wg = per_wg; p.threads = threads; p.grid = tx_grid(nblocks, per_wg);
    return SVT_HIP_OK;
}
inline int bad_type(int tx_size, int tx_type) { return set_err(SVT_HIP_ERR_INVALID, "tx_size %d / tx_type %d not defined by the reference", tx_size, tx_type); }
inline int too_many() { return set_err(SVT_HIP_ERR_INVALID, "nblocks too large"); }
}  // namespace txplan_detail

// ---- svt_hip_fwd_txfm2d_batch ------------------------------------------------------------------------------------------------------------------
// io_aligned: d_in and d_out both 16-byte aligned
inline int fwd_plan(int tx_size, int tx_type, int bd, uint32_t in_stride, size_t in_block_pitch, uint64_t nblocks, bool io_aligned, const TxKnobs& k, TxPlan& p) {
    using namespace txplan_detail;
    p = TxPlan{};
    if (!tx_type_ok(tx_size, tx_type)) return bad_type(tx_size, tx_type);
    if (bd != 8 && bd != 10) return set_err(SVT_HIP_ERR_INVALID, "bit depth %d", bd);
    if (nblocks > kTxMaxBlocks) return too_many();
    const int w = kTxW[tx_size], h = kTxH[tx_size];
    const bool dense = in_stride == (uint32_t)w && in_block_pitch == (size_t)w * h && io_aligned;
    if (tx_is_32x32_pair(tx_size, tx_type) && dense) {
        p.idtx = tx_type == SVT_IDTX;
        return launch(p, TXR_FWD32, nblocks, f32_blocks_per_wg(), kF32Waves * 64);
    }
    if (!k.no_staged && dense) return launch(p, TXR_FWD_STAGED, nblocks, tx_staged_blocks_per_wg(tx_size), tx_staged_waves(w, h) * 64);
    return launch(p, TXR_FWD_GENERAL, nblocks, tx_general_blocks_per_wg(tx_size), kTxWaves * 64);
}

// ---- svt_hip_pack64_batch ------------------------------------------------------------------------------------------------------------------------
inline int pack64_plan(int tx_size, uint64_t nblocks, TxPlan& p) {
    using namespace txplan_detail;
    p = TxPlan{};
    if (tx_size < 0 || tx_size >= SVT_TX_SIZES_ALL) return set_err(SVT_HIP_ERR_INVALID, "bad argument");
    if (nblocks > kTxMaxBlocks) return too_many();
    if (kTxW[tx_size] != 64 && kTxH[tx_size] != 64) { p.route = TXR_PACK64_NONE; return SVT_HIP_OK; }
    return launch(p, TXR_PACK64, nblocks, 1, 256);      // one workgroup per block
}

// ---- svt_hip_inv_txfm2d_add_batch ----------------------------------------------------------------------------------------------------------------
inline int inv_plan(int tx_size, int tx_type, int bd, int is16, int32_t dst_stride, size_t dst_block_pitch, bool has_offsets, uint64_t nblocks, bool coeff_aligned,
                    bool dst_aligned, const TxKnobs& k, TxPlan& p) {
    using namespace txplan_detail;
    p = TxPlan{};
    if (!tx_type_ok(tx_size, tx_type)) return bad_type(tx_size, tx_type);
    if (bd != 8 && bd != 10 && bd != 12) return set_err(SVT_HIP_ERR_INVALID, "bit depth %d", bd);
    if (!is16 && bd != 8) return set_err(SVT_HIP_ERR_INVALID, "8-bit destination needs bd = 8");
    if (nblocks > kTxMaxBlocks) return too_many();
    const int w = kTxW[tx_size], h = kTxH[tx_size];
    p.is16 = is16 != 0; p.bd = bd;
    if (bd > 10) {
        // bd 12 (not an encoder configuration, only the C inverse kernels define it): the general kernel with 64-bit
        // half_btf sums (txfm1d_gen.h, WIDE); the tuned kernels' 32-bit multiply-accumulate chains are exact for bd <= 10 only
        p.wide = true;
        return launch(p, TXR_INV_GENERAL, nblocks, tx_general_blocks_per_wg(tx_size), kTxWaves * 64);
    }
    if (tx_is_32x32_pair(tx_size, tx_type) && coeff_aligned) {
        p.idtx = tx_type == SVT_IDTX;
        if (!is16 && (k.inv32_waves != 4 || k.inv32_var != 0)) {     // tuning probes (tools/tune_inv32.py): the variants the library builds
            const int wv = k.inv32_waves, vr = k.inv32_var;
            if (!((wv == 4 && (vr == 1 || vr == 2 || vr == 4 || vr == 5 || vr == 8)) || (wv == 2 && vr == 0)))
                return set_err(SVT_HIP_ERR_INVALID, "inv32 probe variant not built");
            p.wv = wv; p.vr = vr;
            return launch(p, TXR_INV32_PROBE, nblocks, f32_blocks_per_wg(wv), (uint32_t)wv * 64);
        }
        return launch(p, TXR_INV32, nblocks, f32_blocks_per_wg(), kF32Waves * 64);
    }
    const bool dense_dst = !has_offsets && dst_stride == w && dst_block_pitch == (size_t)w * h && dst_aligned && (w * h * (is16 ? 2 : 1)) % 16 == 0;
    // 4-sample-wide 8-bit rows would be 4-B chunks of an unaligned plane: leave those to the general kernel
    const bool plane_dst = has_offsets && w * (is16 ? 2 : 1) >= 8 && !k.no_inv_planes;
    if (!k.no_staged && (dense_dst || plane_dst) && coeff_aligned) {
        // 64-point sizes at bd <= 10: 16-bit transpose tile (the column input is clamped to 16 bits there anyway), which lifts
        // their LDS-limited 2 waves per SIMD to 4; smaller sizes are not LDS-limited and sub-dword LDS writes are slower
        p.t16 = w >= 64 || h >= 64;
        return launch(p, TXR_INV_STAGED, nblocks, tx_staged_blocks_per_wg(tx_size), tx_staged_waves(w, h) * 64);
    }
    return launch(p, TXR_INV_GENERAL, nblocks, tx_general_blocks_per_wg(tx_size), kTxWaves * 64);
}

// ---- svt_hip_quantize_b_batch --------------------------------------------------------------------------------------------------------------------
inline int quantize_plan(size_t n_coeffs, int log_scale, const svt_hip_qrows& q, uint64_t nblocks, TxPlan& p) {
    using namespace txplan_detail;
    p = TxPlan{};
    if (n_coeffs < 16 || n_coeffs > 4096 || (n_coeffs & 15)) return set_err(SVT_HIP_ERR_INVALID, "n_coeffs %zu", n_coeffs);
    if (log_scale < 0 || log_scale > 2) return set_err(SVT_HIP_ERR_INVALID, "log_scale %d", log_scale);
    if (nblocks > kTxMaxBlocks) return too_many();
    p.log_scale = log_scale; p.qp = tx_qparams(q, log_scale);
    p.lanes = quantize_b_lanes((int)n_coeffs);
    return launch(p, TXR_QUANTIZE_B, nblocks, quantize_b_blocks_per_wg(p.lanes), 256);
}

// ---- svt_hip_fwd_quant_planes_batch ----------------------------------------------------------------------------------------------------------------
// px_aligned: d_src and d_pred; co_aligned: d_coeff, d_qcoeff and d_dqcoeff
inline int fq_planes_plan(int tx_size, int tx_type, int is16, int bd, uint32_t src_stride, uint32_t pred_stride, bool has_xy, bool has_sad, bool has_energy,
                          const svt_hip_qrows& q, uint64_t nblocks, bool px_aligned, bool co_aligned, const TxKnobs& k, TxPlan& p) {
    using namespace txplan_detail;
    p = TxPlan{};
    if (!tx_type_ok(tx_size, tx_type)) return bad_type(tx_size, tx_type);
    if ((is16 && bd != 10) || (!is16 && bd != 8)) return set_err(SVT_HIP_ERR_INVALID, "bit depth %d (%d-bit planes)", bd, is16 ? 16 : 8);
    if (is16 && has_sad) return set_err(SVT_HIP_ERR_INVALID, "SAD is defined for 8-bit planes only (the reference searches on the 8-bit MSB plane)");
    if (nblocks > kTxMaxBlocks) return too_many();
    const int w = kTxW[tx_size], h = kTxH[tx_size];
    p.log_scale = tx_log_scale(tx_size); p.qp = tx_qparams(q, p.log_scale);
    if (qparams_negative(p.qp)) return set_err(SVT_HIP_ERR_INVALID, "negative quantizer table entry");
    p.is16 = is16 != 0; p.bd = bd; p.sad = has_sad;
    p.src_stride = src_stride; p.pred_stride = pred_stride;
    const bool fast = p.qp.fast_ok != 0;
    if (tx_is_32x32_pair(tx_size, tx_type) && fast && !has_energy && !k.no_f32p && (has_xy || is16) && co_aligned) {
        // the tuned 32x32 kernel on planes / 10-bit samples (dense 16-bit batches are "planes" of stride 32 with a NULL table)
        p.idtx = tx_type == SVT_IDTX; p.inm = is16 ? 2 : 1; p.qmode = 2; p.planes = is16 ? has_xy : true;
        return launch(p, TXR_FQ32_PLANES, nblocks, f32_blocks_per_wg(), kF32Waves * 64);
    }
    // dense batches need 16-B aligned inputs, plane-addressed blocks do not
    const bool b128 = fast && (has_xy || px_aligned) && co_aligned;
    if (tx_size == SVT_TX_64X64 && !k.no_staged && !k.no_enc64 && !has_energy && b128) {
        // two blocks per wave, forward networks pruned to the 32 kept outputs (the forward half of enc64_kernel); callers that
        // want three_quad_energy keep the one-block kernel, which forms the discarded coefficients
        if (!has_xy) p.src_stride = p.pred_stride = 64;
        return launch(p, TXR_FQ64, nblocks, kE64BlocksPerWg, kE64Waves * 64);
    }
    // staged (coalesced) kernels
    if (!k.no_staged && w * h > 16 && b128) return launch(p, TXR_FQ_STAGED, nblocks, tx_staged_blocks_per_wg(tx_size), tx_staged_waves(w, h) * 64);
    if (!has_xy) p.src_stride = p.pred_stride = (uint32_t)w;
    return launch(p, TXR_FQ_GENERAL, nblocks, tx_general_blocks_per_wg(tx_size), kTxWaves * 64);
}

// ---- svt_hip_fwd_quant_sad_batch: the headline chain on dense 8-bit 32x32 batches; every other size and type is the planes call's ---------------------
inline int fq_sad_plan(int tx_size, int tx_type, bool has_sad, const svt_hip_qrows& q, uint64_t nblocks, bool px_aligned, bool co_aligned, const TxKnobs& k,
                       int num_cu, TxPlan& p) {
    using namespace txplan_detail;
    if (!tx_is_32x32_pair(tx_size, tx_type)) return fq_planes_plan(tx_size, tx_type, 0, 8, 0, 0, false, has_sad, false, q, nblocks, px_aligned, co_aligned, k, p);
    p = TxPlan{};
    if (nblocks > kTxMaxBlocks) return too_many();
    p.log_scale = 1; p.qp = tx_qparams(q, 1);
    if (qparams_negative(p.qp)) return set_err(SVT_HIP_ERR_INVALID, "negative quantizer table entry");
    // QMODE 2 needs power-of-two quant_shift (every av1_build_quantizer table); else the 24-bit general form
    p.idtx = tx_type == SVT_IDTX; p.inm = 1; p.sad = has_sad; p.nt = k.f32_nt != 0; p.qmode = p.qp.fast_ok && !k.f32_qmode1 ? 2 : 1;
    launch(p, TXR_FQ32, nblocks, f32_blocks_per_wg(), kF32Waves * 64);
    const uint32_t max_grid = (uint32_t)num_cu * (uint32_t)k.f32_wg_per_cu;
    if (k.f32_wg_per_cu > 0 && p.grid > max_grid) { p.grid = max_grid; p.grid_capped = true; }
    return SVT_HIP_OK;
}

// ---- svt_hip_encode_recon_batch / _planes_batch ------------------------------------------------------------------------------------------------------
// recon_aliases: d_recon is d_src, or, in a dense batch, d_pred.  stage[2]: the composed route's launches.
// 16-byte alignment of: d_src and d_pred; d_recon; d_qcoeff, d_coeff and d_dqcoeff (an absent one counts as aligned); d_dqcoeff alone.  The fused
// kernels ask for the first three, the stages of the composed route each for the groups it touches.
struct EncAligned { bool src_pred, recon, coeffs, dqcoeff; };
inline int encode_recon_plan(int tx_size, int tx_type, int is16, int bd, bool has_xy, bool has_coeff, bool has_dqcoeff, bool has_sad, bool recon_aliases,
                             const svt_hip_qrows& q, uint64_t nblocks, const EncAligned& al, const TxKnobs& k, int num_cu, TxPlan& p, TxPlan stage[2]) {
    using namespace txplan_detail;
    p = TxPlan{};
    const bool px_aligned = al.src_pred && al.recon, co_aligned = al.coeffs;
    if (!tx_type_ok(tx_size, tx_type)) return bad_type(tx_size, tx_type);
    if (recon_aliases) return set_err(SVT_HIP_ERR_INVALID, "d_recon must not alias d_src (or, for dense batches, d_pred)");
    if ((is16 && bd != 10) || (!is16 && bd != 8)) return set_err(SVT_HIP_ERR_INVALID, "bit depth %d (%d-bit samples)", bd, is16 ? 16 : 8);
    if (is16 && has_sad) return set_err(SVT_HIP_ERR_INVALID, "SAD is defined for 8-bit planes only (the reference searches on the 8-bit MSB plane)");
    if (nblocks > kTxMaxBlocks) return too_many();
    const int w = kTxW[tx_size], h = kTxH[tx_size];
    const bool pair = has_coeff == has_dqcoeff;      // a fused kernel keeps both or neither
    p.is16 = is16 != 0; p.bd = bd; p.keep = has_coeff; p.sad = has_sad;
    p.log_scale = tx_log_scale(tx_size); p.qp = tx_qparams(q, p.log_scale);
    const bool fast = p.qp.fast_ok && !qparams_negative(p.qp);
    if (tx_is_32x32_pair(tx_size, tx_type) && fast && pair) {
        p.idtx = tx_type == SVT_IDTX;
        return launch(p, TXR_ENC32, nblocks, f32_blocks_per_wg(), kF32Waves * 64);
    }
    if (tx_size == SVT_TX_4X4 && pair && !k.no_enc_staged) {
        // one lane per block, everything in registers (enc4_kernel); any quantiser table
        p.fast = fast;
        return launch(p, TXR_ENC4, nblocks, kEnc4BlocksPerWg, 256);
    }
    // every other size: the staged fused kernel (power-of-two quant_shift tables, 16-B aligned coefficient buffers and, for dense batches, samples)
    if (fast && w * h > 16 && !k.no_enc_staged && pair && co_aligned && (has_xy || px_aligned)) {
        if (tx_size == SVT_TX_64X64 && !k.no_enc64) {
            // two blocks per wave, pruned 64-point networks (kernel_enc64.h); the kernel that keeps the coefficients also forms the SAD
            p.sad = has_coeff || has_sad;
            return launch(p, TXR_ENC64, nblocks, kE64BlocksPerWg, kE64Waves * 64);
        }
        return launch(p, TXR_ENC_STAGED, nblocks, tx_staged_blocks_per_wg(tx_size), tx_staged_waves(w, h) * 64);
    }
    // composed path: the two batched stages around a device copy of the prediction
    if (!has_coeff || !has_dqcoeff) return set_err(SVT_HIP_ERR_INVALID, "this size/type/quantizer needs d_coeff and d_dqcoeff");
    if (has_xy || is16)
        return set_err(SVT_HIP_ERR_INVALID, "no fused kernel for this case (4x4, non-power-of-two quant_shift or misaligned coefficient buffers); use svt_hip_fwd_quant_planes_batch + svt_hip_inv_txfm2d_add_batch");
    if (int rc = fq_sad_plan(tx_size, tx_type, has_sad, q, nblocks, al.src_pred, al.coeffs, k, num_cu, stage[0])) return rc;
    if (int rc = inv_plan(tx_size, tx_type, 8, 0, w, (size_t)w * h, false, nblocks, al.dqcoeff, al.recon, k, stage[1])) return rc;
    p.route = TXR_ENC_COMPOSED;
    return SVT_HIP_OK;
}

// ---- svt_hip_fwd_quant_batch ------------------------------------------------------------------------------------------------------------------------
// in_aligned: d_residual; out_aligned: d_coeff (the forward stage of the composed route writes it).  stage[2]: the composed route's launches.
inline int fwd_quant_plan(int tx_size, int tx_type, int bd, const svt_hip_qrows& q, uint64_t nblocks, bool in_aligned, bool out_aligned, const TxKnobs& k, TxPlan& p,
                          TxPlan stage[2]) {
    using namespace txplan_detail;
    p = TxPlan{};
    if (!tx_type_ok(tx_size, tx_type)) return bad_type(tx_size, tx_type);
    if (nblocks > kTxMaxBlocks) return too_many();
    const int w = kTxW[tx_size], h = kTxH[tx_size];
    p.log_scale = tx_log_scale(tx_size); p.qp = tx_qparams(q, p.log_scale);
    if (tx_is_32x32_pair(tx_size, tx_type) && bd == 8 && p.qp.fast_ok && in_aligned) {
        // 24-bit quantiser arithmetic needs 8-bit-range residuals (|coeff| < 2^17)
        p.idtx = tx_type == SVT_IDTX;
        return launch(p, TXR_FWD32_QUANT, nblocks, f32_blocks_per_wg(), kF32Waves * 64);
    }
    // general sizes: transform into d_coeff, quantise (two more passes over d_coeff)
    if (w == 64 || h == 64) return set_err(SVT_HIP_ERR_UNSUPPORTED, "use svt_hip_fwd_quant_planes_batch for 64-pt sizes (packed coefficient layout)");
    if (int rc = fwd_plan(tx_size, tx_type, bd, (uint32_t)w, (size_t)w * h, nblocks, in_aligned && out_aligned, k, stage[0])) return rc;
    if (int rc = quantize_plan((size_t)w * h, p.log_scale, q, nblocks, stage[1])) return rc;
    p.route = TXR_FWD_THEN_QUANT;
    return SVT_HIP_OK;
}

// ---- svt_hip_encode_recon_frame ------------------------------------------------------------------------------------------------------------------------
// argument checks of a frame call's groups (also svt_hip_encode_recon_frame_ex's, before it enqueues its first phase): members are read for NULL, never through
inline int frame_groups_check(const svt_hip_frame_group* groups, int ngroups, const TxKnobs& k) {
    if (ngroups == 0) return SVT_HIP_OK;
    if (!groups || ngroups < 0) return set_err(SVT_HIP_ERR_INVALID, "NULL group list");
    if (ngroups > 256) return set_err(SVT_HIP_ERR_INVALID, "more than 256 groups in one call");
    for (int g = 0; g < ngroups; g++) {
        const svt_hip_frame_group& G = groups[g];
        if (G.nblocks == 0) continue;
        if (!G.d_src || !G.d_pred || !G.d_recon || !G.d_xy || !G.d_iscan || !G.d_qcoeff || !G.d_eob)
            return set_err(SVT_HIP_ERR_INVALID, "group %d: NULL member", g);
        if (!tx_type_ok(G.tx_size, G.tx_type)) return set_err(SVT_HIP_ERR_INVALID, "group %d: tx_size %d / tx_type %d", g, G.tx_size, G.tx_type);
        if ((G.d_coeff != nullptr) != (G.d_dqcoeff != nullptr)) return set_err(SVT_HIP_ERR_INVALID, "group %d: d_coeff and d_dqcoeff go together", g);
        if (G.tx_size == SVT_TX_4X4 && k.no_enc_staged && (!G.d_coeff || !G.d_offsets || G.d_recon != G.d_pred || G.recon_stride != G.pred_stride))
            return set_err(SVT_HIP_ERR_INVALID, "group %d: with no_enc_staged set, 4x4 groups take the two-stage path and need d_coeff, d_dqcoeff, d_offsets and in-place reconstruction", g);
    }
    return SVT_HIP_OK;
}

// How a frame call is launched.  ONE launch per REGISTER CLASS (enc_frame_kernel, kernel_frame.h) or one launch in all, when every group is one
// the fused bodies cover: any of the 19 sizes and their types, qcoeff + recon outputs, power-of-two quant_shift tables.  Measured
// (tools/bench_frame.py, tools/bench_c5.py): a 1080p picture as 13 per-size launches on 8 streams 0.160 ms, those captured into a graph 0.101,
// ONE launch at the 64x64 body's register budget (round 2) 0.044; by class see DESIGN 4.17.
enum FrameMode { FRAME_FAN_OUT = 0, FRAME_ONE_LAUNCH = 1, FRAME_BY_CLASS = 2 };      // (the values of the frame_single_launch knob)
// frame_single_launch -1 (default): one launch up to 2^25 pixel passes per call (two 1080p pictures with five sizes; measured cross-over between 2
// and 4, tools/bench_frame.py), class launches above ...
constexpr uint64_t kFrameOneLaunchMaxPixels = (uint64_t)1 << 25;
// ... and per-size launches on the fan-out streams above 2^28 (a GOP of 4K pictures: every size fills the GPU on its own at its own kernel's
// occupancy; configs[4], 30 pictures per call, tools/bench_c5.py: 6 162 pictures/s against 5 756 by class and 4 888 in one launch)
constexpr uint64_t kFrameClassLaunchMaxPixels = (uint64_t)1 << 28;
constexpr int kFrameMaxGroups = 22;                      // groups of one launch (kernel_frame.h FRAME_MAX_GROUPS)
constexpr uint32_t kFrameMaxLaunchWgs = 0x7fffffffu;      // workgroups of one launch (group_table.h kMaxLaunchWgs)
constexpr int kFrameOneLaunchTable = 3;                  // the table of the one launch, behind those of classes 0 .. 2

struct FrameGroupPlan { uint8_t table, log_scale; uint32_t wgs; };      // of a non-empty group: its table (its class, or the one launch's), workgroups
struct FramePlan {
    int mode;                  // FrameMode after the demotion (the one-launch kernel holds the square sizes)
    bool tables;               // the group tables apply; false: the call takes the fan-out
    QParams qp[3];             // by log_scale, built when a group has it
    FrameGroupPlan g[256];     // [i] of groups[i], set for the non-empty ones when `tables`
};

// For groups frame_groups_check accepted.  Pointers are compared and tested for alignment, never followed.
inline void frame_plan(const svt_hip_frame_group* groups, int ngroups, int is16, int bd, const svt_hip_qrows& q, const TxKnobs& k, FramePlan& fp) {
    uint64_t call_pixels = 0;
    bool non_square = false;
    for (int g = 0; g < ngroups; g++) {
        if (groups[g].nblocks == 0) continue;
        call_pixels += (uint64_t)groups[g].nblocks * (uint64_t)(kTxW[groups[g].tx_size] * kTxH[groups[g].tx_size]);
        non_square |= groups[g].tx_size > SVT_TX_64X64;
    }
    fp.mode = k.frame_single_launch >= 0 ? k.frame_single_launch
                                         : (call_pixels <= kFrameOneLaunchMaxPixels ? FRAME_ONE_LAUNCH : (call_pixels <= kFrameClassLaunchMaxPixels ? FRAME_BY_CLASS : FRAME_FAN_OUT));
    if (fp.mode == FRAME_ONE_LAUNCH && non_square) fp.mode = FRAME_BY_CLASS;
    fp.tables = fp.mode > 0 && ((is16 && bd == 10) || (!is16 && bd == 8));
    bool have_qp[3] = {false, false, false};
    int count[4] = {0, 0, 0, 0};
    uint64_t wgs[4] = {0, 0, 0, 0};
    for (int g = 0; g < ngroups && fp.tables; g++) {
        const svt_hip_frame_group& G = groups[g];
        if (G.nblocks == 0) continue;
        const int ls = tx_log_scale(G.tx_size), t = fp.mode == FRAME_ONE_LAUNCH ? kFrameOneLaunchTable : tx_class(G.tx_size);
        if (!have_qp[ls]) { fp.qp[ls] = tx_qparams(q, ls); have_qp[ls] = true; }
        fp.g[g] = FrameGroupPlan{(uint8_t)t, (uint8_t)ls, (G.nblocks - 1) / frame_blocks_per_wg(G.tx_size) + 1};
        wgs[t] += fp.g[g].wgs;
        // a group the fused bodies do not cover, or a table with no room for it, sends the whole call to the fan-out: nothing is launched
        // before every group has its slot
        fp.tables = !G.d_coeff && G.d_recon != G.d_src && ((uintptr_t)G.d_qcoeff & 15) == 0 && fp.qp[ls].fast_ok && !qparams_negative(fp.qp[ls]) &&
                    ++count[t] <= kFrameMaxGroups && wgs[t] <= kFrameMaxLaunchWgs;
    }
}

}  // namespace svthost

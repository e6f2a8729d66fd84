/*
 * svt_hip_dsp.h — C ABI of libsvt_hip_dsp.so: the MI355X (gfx950) implementation
 * of SVT-AV1's block-DSP hot path.  Plain C, plain pointers and sizes; no HIP or
 * torch types appear in any signature (streams travel as void*).
 *
 * Two layers:
 *
 *  (A) DROP-IN entry points — the exact signatures of the reference's dispatch
 *      slots (RTCD globals in Source/Lib/Common/Codec/aom_dsp_rtcd.h and the
 *      *_funcPtrArray[asm_type] tables).  HOST pointers, synchronous, re-entrant
 *      (per-thread stream + staging).  They exist so that the reference's own
 *      call sites and unit tests can run unchanged against this library; one
 *      block per call cannot be fast on a GPU.
 *
 *  (B) BATCHED entry points — arrays of blocks per launch on DEVICE-resident
 *      buffers with an explicit stream; this is where the throughput is.
 *
 * There is no CPU fallback anywhere: when the HIP runtime / device is not
 * usable, (B) returns SVT_HIP_ERR_* and (A), whose reference signatures have no
 * error channel, print the error to stderr and abort().
 *
 * Numeric contract: every output is bit-exact with the reference's C / AVX2
 * kernels (all arithmetic on this path is integer).  8-bit quantisation follows
 * the reference's PRODUCTION slot, i.e. the high-bit-depth algorithm that
 * setup_rtcd_internal installs under AVX2 (aom_dsp_rtcd.h:3330-3334), not the
 * INT16-clamping aom_quantize_b_c_II.
 */
#ifndef SVT_HIP_DSP_H
#define SVT_HIP_DSP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ---- reference types (Source/Lib/Common/Codec/EbDefinitions.h) ------------- */
typedef uint8_t svt_tx_size_t;   /* TxSize, packed enum  (EbDefinitions.h:615-650) */
typedef uint8_t svt_tx_type_t;   /* TxType, packed enum  (EbDefinitions.h:727-746) */
typedef int32_t svt_tran_low_t;  /* tran_low_t           (EbDefinitions.h:662)     */

enum { SVT_TX_4X4, SVT_TX_8X8, SVT_TX_16X16, SVT_TX_32X32, SVT_TX_64X64, SVT_TX_4X8, SVT_TX_8X4,
       SVT_TX_8X16, SVT_TX_16X8, SVT_TX_16X32, SVT_TX_32X16, SVT_TX_32X64, SVT_TX_64X32,
       SVT_TX_4X16, SVT_TX_16X4, SVT_TX_8X32, SVT_TX_32X8, SVT_TX_16X64, SVT_TX_64X16, SVT_TX_SIZES_ALL };
enum { SVT_DCT_DCT, SVT_ADST_DCT, SVT_DCT_ADST, SVT_ADST_ADST, SVT_FLIPADST_DCT, SVT_DCT_FLIPADST,
       SVT_FLIPADST_FLIPADST, SVT_ADST_FLIPADST, SVT_FLIPADST_ADST, SVT_IDTX, SVT_V_DCT, SVT_H_DCT,
       SVT_V_ADST, SVT_H_ADST, SVT_V_FLIPADST, SVT_H_FLIPADST, SVT_TX_TYPES };

/* TxfmParam (EbDefinitions.h:764-776), same layout */
typedef struct svt_txfm_param {
    svt_tx_type_t tx_type;
    svt_tx_size_t tx_size;
    int32_t lossless;
    int32_t bd;
    int32_t is_hbd;
    uint8_t tx_set_type;
    int32_t eob;
} svt_txfm_param;

/* ---- status ---------------------------------------------------------------- */
enum {
    SVT_HIP_OK = 0,
    SVT_HIP_ERR_NO_DEVICE = -1,     /* HIP runtime or gfx950 device unavailable */
    SVT_HIP_ERR_INVALID = -2,       /* bad argument (size/type not defined by AV1, NULL, ...) */
    SVT_HIP_ERR_UNSUPPORTED = -3,   /* defined by the reference but not built yet */
    SVT_HIP_ERR_RUNTIME = -4        /* a HIP call failed; see svt_hip_last_error() */
};

/* Initialise on HIP device `device` (call once per process, before any worker
 * thread uses the library — mirrors eb_init_encoder's single-threaded RTCD fill,
 * EbEncHandle.c:917).  Idempotent. */
int svt_hip_init(int device);
void svt_hip_shutdown(void);
/* thread-local, NUL-terminated, never NULL */
const char *svt_hip_last_error(void);
/* "gfx950 ..." description of the device in use (empty string before init) */
const char *svt_hip_device_name(void);

/* Performance-tuning / A-B knobs; they never change results, only which kernel variant runs
 * (process-wide, not thread-safe: set them before the worker threads start).  Keys:
 *   "f32_wg_per_cu" (persistent grid = CUs x
 *   this; 0 = one-shot grid), "f32_nt" (non-temporal stores), "f32_qmode1" (general 24-bit quantiser form),
 *   "no_staged", "no_f32p", "no_enc_staged", "no_inv_planes" (1 = take the general un-staged / two-kernel path),
 *   "no_qsad", "no_q2", "no_q16" (1 = take the first-generation search kernels), "me_exact" (1 = svt_hip_me_fullpel_search_batch always takes its general search-point-by-search-point kernel), "q2_su4" (1 = two-step window staging), "ois_no_fold" (1 = directional predictions through scratch),
 *   "ois_no_dir3" (1 = the open-loop search's three directional zones as three launches instead of one),
 *   "ois_no_nd_multi" (1 = svt_hip_ois_search_frame: one non-directional launch per block size instead of one for the picture),
 *   "frame_single_launch" (svt_hip_encode_recon_frame: 0 = per-size launches, 1 = one launch, 2 = one launch per register class, -1 = by call size),
 *   "inv32_waves", "inv32_var" (probe variants of the inverse 32x32 kernel, tools/tune_inv32.py).
 * Unknown keys return SVT_HIP_ERR_INVALID. */
int svt_hip_tune(const char *key, int value);

/* device memory helpers for C hosts that do not link the HIP runtime */
void *svt_hip_malloc(size_t bytes);
void svt_hip_free(void *dptr);
int svt_hip_memcpy_h2d(void *dptr, const void *hptr, size_t bytes, void *stream);
int svt_hip_memcpy_d2h(void *hptr, const void *dptr, size_t bytes, void *stream);
int svt_hip_stream_sync(void *stream);
/* Allocates n device buffers as SEPARATE allocations with a temporary spacer of `gap_bytes` (0 = the default, 32 GiB) between
 * consecutive ones, freed again before the call returns.  Why: a kernel that writes several large arrays at once (the fused chain:
 * coeff, qcoeff, dqcoeff, 4 GiB each at 2^20 blocks) runs 20 - 25 % slower when those arrays are slices of ONE allocation - one
 * contiguous block of device memory - than when at least one of them lies in another block (MI355X: 350 - 375 against 420 - 460 M
 * blocks/s; no skew or offset inside the block changes it; DESIGN.md 5, profiles/r03_placement_probe*.log).  Separate allocations
 * are in the fast band either way (420 - 455 measured for three plain svt_hip_malloc calls and for this call alike); with torch's
 * allocator 32 GiB spacers were the reliable recipe.  If a spacer cannot be allocated the buffers simply follow each other.
 * Each pointer is freed with svt_hip_free. */
int svt_hip_malloc_spread(const size_t *bytes, int n, size_t gap_bytes, void **ptrs);
/* Box calibration for the roofline report (bench.py): streams `bytes` through HBM in the access shape the kernels of this
 * library use (one 16-byte access per lane, a grid as large as the job, non-temporal stores) so that a measured kernel rate
 * can be put next to what THIS device delivers today.  mode 0 = fill `bytes` of dst; 1 = copy `bytes` from src to dst;
 * 2 = the headline kernel's 1 : 6 read / write mix (reads `bytes` from src, writes 6 x `bytes` to dst).  `bytes` is a
 * multiple of 16, pointers 16-byte aligned.  Enqueues one kernel on `stream`. */
int svt_hip_membw_probe(int mode, void *dst, const void *src, size_t bytes, void *stream);
/* ... and the fused 32x32 chain's own traffic, nothing else: per block 1 KiB read from each of d_in0 / d_in1 (nblocks x 1 KiB each) and
 * 4 KiB written to each of d_out0 / d_out1 / d_out2 (nblocks x 4 KiB each) as 1 KiB stores of one wave - the time of this launch on
 * the caller's own arrays is what the memory system gives that stream pattern in that placement. */
int svt_hip_membw_probe_chain(const void *d_in0, const void *d_in1, void *d_out0, void *d_out1, void *d_out2, size_t nblocks,
                              void *stream);

/* ---- host-side tables for callers outside the encoder (csrc/host_tables.cpp; no device involved) ------------------
 * y-plane quantiser rows of av1_build_quantizer(bit_depth, 0, 0, 0, 0, 0) (EbModeDecisionConfigurationProcess.c:429-520):
 * five int16 [256][8] tables indexed [qindex][0 = DC, 1..7 = AC], the rows the quantiser entry points take. */
int svt_hip_build_quantizer(int bit_depth, int16_t (*zbin)[8], int16_t (*round)[8], int16_t (*quant)[8],
                            int16_t (*quant_shift)[8], int16_t (*dequant)[8]);
/* av1_scan_orders[tx_size][tx_type] (EbTransforms.h:3349-3870): scan / iscan over the kept min(W,32) x min(H,32)
 * coefficients (either pointer may be NULL); returns their number (<= 1024) or SVT_HIP_ERR_INVALID. */
int svt_hip_get_scan(int tx_size, int tx_type, int16_t *scan, int16_t *iscan);
/* the candidate list open_loop_intra_search_sb enumerates for one block size (EbMotionEstimation.c:8747-8846): modes in AV1
 * PredictionMode numbering, angle deltas -2..2; arrays of SVT_HIP_OIS_MAX_CANDIDATES; returns the count. */
#define SVT_HIP_OIS_MAX_CANDIDATES 61
int svt_hip_ois_candidates(uint32_t bsize, int temporal_layer_index, int intra_pred_mode, int is_used_as_reference,
                           int is_16bit, uint8_t *modes, int8_t *angle_deltas);
/* the luma candidate list inject_intra_candidates enumerates for one block (EbModeDecision.c:2364-2530, MR_MODE 0): DC_PRED ..
 * PAETH_PRED (.. SMOOTH_H_PRED when is_16bit, encoder_bit_depth > 8), 7 angle deltas -3..3 per directional mode when bsize >=
 * BLOCK_8X8 (AV1 block_size enum order), thinned by the picture's intra_pred_mode 0..3 (disable_z2_prediction /
 * disable_angle_refinement / disable_angle_prediction from sq_size > 16 and 4-sample sides).  sq_size is blk_geom->sq_size, the
 * side of the enclosing square partition block.  Arrays of SVT_HIP_FAST_LOOP_MAX_CANDIDATES; returns the count (<= 61) or
 * SVT_HIP_ERR_INVALID. */
int svt_hip_md_intra_candidates(uint32_t bwidth, uint32_t bheight, uint32_t sq_size, int bsize, int intra_pred_mode, int is_16bit,
                                uint8_t *modes, int8_t *angle_deltas);

/* ============================================================================
 * (B) batched API — device pointers, `stream` is a hipStream_t (NULL = default)
 * Every call only enqueues work; it returns before the GPU finishes.
 * A batch holds at most 2^31 - 1 blocks: every call of this section returns
 * SVT_HIP_ERR_INVALID ("nblocks too large") above that, before it launches
 * anything (svt_hip_inv_txfm2d_add_batch, svt_hip_quantize_b_batch,
 * svt_hip_pack64_batch and svt_hip_fwd_quant_batch included, which once took
 * the count modulo 2^32).
 * ==========================================================================*/

/* K1 forward 2-D transform.  Replaces av1_fwd_txfm2d_WxH
 * (aom_dsp_rtcd.h:160-255; C: EbTransforms.c:4410-4910; AVX2:
 * highbd_fwd_txfm_avx2.c:762-5814) over `nblocks` blocks.
 * d_in: int16 residual, block b at d_in + b*in_block_pitch, row stride in_stride
 * (elements).  d_out: dense W*H int32 per block, row-major, full size (64-pt
 * outputs are NOT packed; see svt_hip_pack64_batch). */
int svt_hip_fwd_txfm2d_batch(const int16_t *d_in, uint32_t in_stride, size_t in_block_pitch,
                             int32_t *d_out, size_t nblocks, int tx_size, int tx_type, int bd,
                             void *stream);

/* 64-pt handling of av1_estimate_transform (EbTransforms.c:4377-4408,
 * 4580-4731, 5157-5175): per block, energy of the discarded region -> d_energy
 * (may be NULL), then re-pack the kept min(W,32) x min(H,32) region in place and
 * zero the tail.  No-op (energy 0) for sizes without a 64 dimension. */
int svt_hip_pack64_batch(int32_t *d_coeff, uint64_t *d_energy, size_t nblocks, int tx_size,
                         void *stream);

/* K2 inverse 2-D transform + add.  Replaces av1_inv_txfm2d_add_WxH
 * (aom_dsp_rtcd.h:350-417; C: EbTransforms.c:8180-8458) and, with
 * dst_is_16bit = 0, the 8-bit recon entry av1_inv_txfm_add (:8882-8903).
 * d_coeff: dense packed min(W,32)*min(H,32) int32 per block.
 * d_dst: uint16 (dst_is_16bit) or uint8 samples; block b lives at
 * d_dst + (d_dst_offsets ? d_dst_offsets[b] : b*dst_block_pitch), row stride
 * dst_stride (all in elements).  Blocks must not overlap. */
int svt_hip_inv_txfm2d_add_batch(const int32_t *d_coeff, void *d_dst, int dst_is_16bit,
                                 int32_t dst_stride, size_t dst_block_pitch,
                                 const uint32_t *d_dst_offsets, size_t nblocks, int tx_size,
                                 int tx_type, int bd, void *stream);

/* K3 quantize + dequantize + eob.  Replaces aom_highbd_quantize_b{,_32x32,_64x64}
 * (aom_dsp_rtcd.h:323-342; C: EbFullLoop.c:239-333; AVX2:
 * highbd_quantize_intrin_avx2.c:127-484) over nblocks dense blocks of n_coeffs.
 * zbin/round/quant/quant_shift/dequant: HOST pointers to the reference's
 * int16[8] table rows ([0] = DC, [1] = AC).  d_iscan: DEVICE int16[n_coeffs].
 * log_scale: 0 (aom_highbd_quantize_b), 1 (_32x32), 2 (_64x64). */
int svt_hip_quantize_b_batch(const int32_t *d_coeff, size_t n_coeffs, int skip_block,
                             const int16_t *zbin, const int16_t *round, const int16_t *quant,
                             const int16_t *quant_shift, int32_t *d_qcoeff, int32_t *d_dqcoeff,
                             const int16_t *dequant, uint16_t *d_eob, const int16_t *d_iscan,
                             int log_scale, size_t nblocks, void *stream);

/* Headline chain (BASELINE.json metric), fused in one kernel: per block
 *   residual = src - pred            ResidualKernel   (EbCodingLoop.c:617)
 *   coeff    = FwdTxfm2d(residual)   av1_estimate_transform (EbFullLoop.c:763)
 *   q,dq,eob = quantize_b(coeff)     av1_quantize_inv_quantize (EbFullLoop.c:780)
 *   sad      = SAD(src, pred)        NxMSadKernel     (EbProductCodingLoop.c:1259)
 * d_src/d_pred: dense W*H uint8 per block.  Outputs dense per block (packed
 * min(W,32)*min(H,32) for 64-pt sizes); d_sad may be NULL.  TX_32X32/DCT_DCT runs the
 * tuned fused kernel, every other size/type the generic fused kernel. */
int svt_hip_fwd_quant_sad_batch(const uint8_t *d_src, const uint8_t *d_pred, size_t nblocks,
                                int tx_size, int tx_type, const int16_t *zbin,
                                const int16_t *round, const int16_t *quant,
                                const int16_t *quant_shift, const int16_t *dequant,
                                const int16_t *d_iscan, int32_t *d_coeff, int32_t *d_qcoeff,
                                int32_t *d_dqcoeff, uint16_t *d_eob, uint32_t *d_sad, void *stream);

/* Encode-pass chain of the transform blocks of one prediction, as the reference runs it per block
 * in Av1EncodeLoop (EbCodingLoop.c:545-950):
 *   residual = src - pred              ResidualKernel                 (EbCodingLoop.c:617)
 *   coeff    = FwdTxfm2d(residual)     av1_estimate_transform         (EbCodingLoop.c:632)
 *   q,dq,eob = quantize_b(coeff)       av1_quantize_inv_quantize      (EbCodingLoop.c:647)
 *   recon    = pred + InvTxfm2d(dq)    av1_inv_transform_recon8bit    (EbCodingLoop.c:753)
 * (+ sad = SAD(src, pred) when d_sad != NULL).  8-bit, dense W*H blocks; d_recon must not alias
 * d_src / d_pred.  TX_32X32 with DCT_DCT or IDTX runs ONE fused kernel in which coefficients and
 * residual never leave the CU (7 174 B of HBM traffic per block instead of 20 486); every other size
 * except 4x4 runs the generic fused kernel of the same structure.  d_coeff and d_dqcoeff are optional in
 * the fused kernels (both NULL = not written).  TX_4X4 runs one lane per block with the whole block in registers (any
 * quantiser table).  For the other sizes, quantiser tables whose quant_shift is not a power of two and buffers that are
 * not 16-B aligned run svt_hip_fwd_quant_sad_batch + a device copy + svt_hip_inv_txfm2d_add_batch and need both buffers. */
int svt_hip_encode_recon_batch(const uint8_t *d_src, const uint8_t *d_pred, size_t nblocks, int tx_size,
                               int tx_type, const int16_t *zbin, const int16_t *round,
                               const int16_t *quant, const int16_t *quant_shift, const int16_t *dequant,
                               const int16_t *d_iscan, int32_t *d_coeff, int32_t *d_qcoeff,
                               int32_t *d_dqcoeff, uint16_t *d_eob, uint32_t *d_sad, uint8_t *d_recon,
                               void *stream);

/* The same chain on picture planes: block b has its top-left sample at (x, y) = (d_xy[b] & 0xffff,
 * d_xy[b] >> 16) of the source, prediction and reconstruction planes (row strides in samples); the
 * reconstruction may be written in place into the prediction plane (d_recon == d_pred with equal
 * strides), as the reference does after pic_copy_kernel (EbCodingLoop.c:741-753).  is_16bit / bd: uint8
 * samples (bd 8) or uint16 samples (bd 10; d_sad must be NULL).  Fused kernels only: for sizes other than 4x4,
 * non-standard quantiser tables return SVT_HIP_ERR_INVALID (use svt_hip_fwd_quant_planes_batch +
 * svt_hip_inv_txfm2d_add_batch there). */
int svt_hip_encode_recon_planes_batch(const void *d_src, uint32_t src_stride, const void *d_pred,
                                      uint32_t pred_stride, void *d_recon, uint32_t recon_stride,
                                      const uint32_t *d_xy, size_t nblocks, int is_16bit, int bd,
                                      int tx_size, int tx_type,
                                      const int16_t *zbin, const int16_t *round, const int16_t *quant,
                                      const int16_t *quant_shift, const int16_t *dequant,
                                      const int16_t *d_iscan, int32_t *d_coeff, int32_t *d_qcoeff,
                                      int32_t *d_dqcoeff, uint16_t *d_eob, uint32_t *d_sad, void *stream);

/* The encode-pass chain for a whole FRAME (or many frames) in ONE call: every (plane, transform size) group of blocks the
 * frame is cut into - BASELINE.json configs[3] / [4], the per-SB loop of AV1EncodePass (EbCodingLoop.c:2249) turned inside
 * out.  A group is what svt_hip_encode_recon_planes_batch takes; the groups of a call are independent (disjoint blocks), so
 * the library issues them CONCURRENTLY on internal streams forked from, and joined back into, `stream` (a lone 1080p frame
 * gives each size's kernel less than one workgroup per CU: run one after the other the frame is launch-latency-bound).
 * The call only enqueues work and can be captured into a HIP graph by the caller (the fork / join becomes graph branches).
 * One quantiser row set per call (one qindex), as in the per-plane entry point. */
typedef struct svt_hip_frame_group {
    const void *d_src;  uint32_t src_stride;     /* planes: pointer to sample (0, 0), stride in samples */
    const void *d_pred; uint32_t pred_stride;
    void *d_recon;      uint32_t recon_stride;   /* may be d_pred with the same stride: reconstruct in place */
    const uint32_t *d_xy;                        /* block origins x | y << 16 */
    const uint32_t *d_offsets;                   /* unused (NULL) unless svt_hip_tune("no_enc_staged", 1): y * recon_stride + x */
    uint32_t nblocks;
    int32_t tx_size, tx_type;
    const int16_t *d_iscan;                      /* DEVICE int16 [min(W,32) * min(H,32)] for this size / type */
    int32_t *d_qcoeff;  uint16_t *d_eob;         /* dense per-group outputs */
    int32_t *d_coeff, *d_dqcoeff;                /* optional, both or neither */
} svt_hip_frame_group;
int svt_hip_encode_recon_frame(const svt_hip_frame_group *groups, int ngroups, int is_16bit, int bd,
                               const int16_t *zbin, const int16_t *round, const int16_t *quant,
                               const int16_t *quant_shift, const int16_t *dequant, void *stream);

/* The frame call with the two encode-pass pieces that sit beside the transform chain:
 *
 *   chroma from luma  (Av1EncodeLoop, EbCodingLoop.c:736-846; 16-bit :1198-1250).  For a chroma block predicted with
 *       UV_CFL_PRED the reference, after the luma transform block's reconstruction, calls cfl_luma_subsampling_420_{lbd,hbd}
 *       on the luma RECONSTRUCTION, subtract_average, and cfl_predict_{lbd,hbd} on the Cb and the Cr prediction IN PLACE with
 *       the block's two alphas; the chroma residual / transform / quantisation then runs on that prediction.  Here: groups
 *       [0, first_chroma_group) are encoded first (the luma groups), then ONE launch does the three steps for every block of
 *       every cfl group (Q3 values stay in registers), then groups [first_chroma_group, ngroups) are encoded.  With ncfl == 0
 *       the split is ignored and all groups go out together.
 *   av1_txb_init_levels  (EbRateDistortionCost.c:125-150, called per coded block by the coefficient cost / entropy stage,
 *       :450) of every group's quantised coefficients: levels[g] (NULL, or one entry per group; an entry with a NULL buffer
 *       skips its group) names one whole padded level buffer per block, (w + 4) * (h + 6) + 16 bytes with w, h the packed
 *       coefficient block's sides (min(.., 32)), as in svt_hip_txb_init_levels_batch.  ONE launch after the encode launches.
 *
 * Everything is enqueued on `stream`, in the order above (stream order carries the dependencies); arguments are validated
 * before the first launch. */
typedef struct svt_hip_frame_cfl_group {
    const void *d_luma_recon; uint32_t luma_stride;     /* the plane the luma groups reconstruct into; samples as the groups' */
    void *d_pred_cb; uint32_t pred_stride_cb;           /* chroma prediction planes (the chroma groups' d_pred): the DC prediction */
    void *d_pred_cr; uint32_t pred_stride_cr;           /* on entry, the chroma-from-luma prediction on return */
    const uint32_t *d_xy;                               /* chroma block origins x | y << 16; the luma area starts at (2x, 2y) */
    const int32_t *d_alpha_q3_cb, *d_alpha_q3_cr;       /* cfl_idx_to_alpha(.., CFL_PRED_U / CFL_PRED_V) per block */
    uint32_t width, height;                             /* chroma block (tx_width_uv x tx_height_uv): 4 .. 32 */
    uint32_t nblocks;
} svt_hip_frame_cfl_group;
typedef struct svt_hip_frame_levels {
    uint8_t *d_levels_buf; size_t levels_block_pitch;   /* >= (w + 4) * (h + 6) + 16, a multiple of 4; 16-byte alignment is faster */
} svt_hip_frame_levels;
int svt_hip_encode_recon_frame_ex(const svt_hip_frame_group *groups, int ngroups, int first_chroma_group,
                                  const svt_hip_frame_cfl_group *cfl, int ncfl, const svt_hip_frame_levels *levels,
                                  int is_16bit, int bd, const int16_t *zbin, const int16_t *round, const int16_t *quant,
                                  const int16_t *quant_shift, const int16_t *dequant, void *stream);

/* BASELINE.json configs[1]: FwdTxfm2d + quantize on a batch of int16 residual blocks
 * (dense W*H per block) — av1_estimate_transform + av1_quantize_inv_quantize
 * (EbFullLoop.c:763, 780).  TX_32X32 8-bit runs the tuned fused kernel. */
int svt_hip_fwd_quant_batch(const int16_t *d_residual, size_t nblocks, int tx_size, int tx_type,
                            int bd, const int16_t *zbin, const int16_t *round, const int16_t *quant,
                            const int16_t *quant_shift, const int16_t *dequant,
                            const int16_t *d_iscan, int32_t *d_coeff, int32_t *d_qcoeff,
                            int32_t *d_dqcoeff, uint16_t *d_eob, void *stream);

/* The same chain for EVERY transform size / type and for 8- or 16-bit sample planes
 * (Av1EncodeLoop EbCodingLoop.c:545-950, Av1EncodeLoop16bit :1020-1351): blocks are
 * addressed inside planes by d_xy[b] = (y << 16) | x (or, when d_xy == NULL, block b
 * starts at b * W*H elements with row stride W: the dense layout above).  Outputs are
 * dense, PACKED min(W,32)*min(H,32) coefficients per block; for 64-pt sizes d_energy
 * (may be NULL) receives av1_estimate_transform's three_quad_energy.  d_sad (may be
 * NULL) is defined for 8-bit planes only. */
int svt_hip_fwd_quant_planes_batch(const void *d_src, uint32_t src_stride, const void *d_pred,
                                   uint32_t pred_stride, const uint32_t *d_xy, size_t nblocks,
                                   int is_16bit, int bd, int tx_size, int tx_type,
                                   const int16_t *zbin, const int16_t *round, const int16_t *quant,
                                   const int16_t *quant_shift, const int16_t *dequant,
                                   const int16_t *d_iscan, int32_t *d_coeff, int32_t *d_qcoeff,
                                   int32_t *d_dqcoeff, uint16_t *d_eob, uint32_t *d_sad,
                                   uint64_t *d_energy, void *stream);

/* K4 NxM SAD (NxMSadKernel_funcPtrArray, EbComputeSAD.h:105-160; C:
 * EbComputeSAD_C.c:48) and K7 SSE (spatial_full_distortion_kernel,
 * EbPictureOperators_C.c:40) over nblocks block pairs; d_out: uint32 / uint64. */
int svt_hip_sad_batch(const uint8_t *d_src, uint32_t src_stride, size_t src_block_pitch,
                      const uint8_t *d_ref, uint32_t ref_stride, size_t ref_block_pitch,
                      uint32_t width, uint32_t height, uint32_t *d_out, size_t nblocks, void *stream);
int svt_hip_sse_batch(const uint8_t *d_a, uint32_t a_stride, size_t a_block_pitch,
                      const uint8_t *d_b, uint32_t b_stride, size_t b_block_pitch, uint32_t width,
                      uint32_t height, uint64_t *d_out, size_t nblocks, void *stream);
/* K8 residual (ResidualKernel, aom_dsp_rtcd.h:2372; C: EbPictureOperators.c:166) */
int svt_hip_residual_batch(const uint8_t *d_src, uint32_t src_stride, size_t src_block_pitch,
                           const uint8_t *d_pred, uint32_t pred_stride, size_t pred_block_pitch,
                           int16_t *d_res, uint32_t res_stride, size_t res_block_pitch,
                           uint32_t width, uint32_t height, size_t nblocks, void *stream);

/* residual_kernel16bit (EbPictureOperators.c:134-164): the same on 16-bit samples (Av1EncodeLoop16bit, EbCodingLoop.c:1085) */
int svt_hip_residual16_batch(const uint16_t *d_src, uint32_t src_stride, size_t src_block_pitch,
                             const uint16_t *d_pred, uint32_t pred_stride, size_t pred_block_pitch,
                             int16_t *d_res, uint32_t res_stride, size_t res_block_pitch,
                             uint32_t width, uint32_t height, size_t nblocks, void *stream);
/* K4 on picture planes (block b at plane + d_*_offsets[b], byte offsets) */
int svt_hip_sad_planes_batch(const uint8_t *d_src_plane, uint32_t src_stride, const uint32_t *d_src_offsets,
                             const uint8_t *d_ref_plane, uint32_t ref_stride, const uint32_t *d_ref_offsets,
                             uint32_t width, uint32_t height, uint32_t *d_out, size_t nblocks, void *stream);
/* aom_sadMxNx4d (aom_dsp_rtcd.h:1328-1500; C: C_DEFAULT/EbComputeSAD_C.c:151-160): per source block, SADs against FOUR
 * reference positions, d_ref_plane + d_ref_offsets[4*b + i]; d_out uint32 [nblocks][4].  Source blocks dense
 * (d_src_offsets == NULL: b * src_block_pitch) or at d_src + d_src_offsets[b]. */
int svt_hip_sad_x4d_batch(const uint8_t *d_src, uint32_t src_stride, size_t src_block_pitch,
                          const uint32_t *d_src_offsets, const uint8_t *d_ref_plane, uint32_t ref_stride,
                          const uint32_t *d_ref_offsets, uint32_t width, uint32_t height, uint32_t *d_out,
                          size_t nblocks, void *stream);
/* combined_averaging_sad (NxMSadAveragingKernel_funcPtrArray, EbComputeSAD.h:162-197; C: C_DEFAULT/EbComputeSAD_C.c:13-40;
 * called by BiPredictionSearch, EbMotionEstimation.c:6639): SAD(src, (ref1 + ref2 + 1) >> 1) */
int svt_hip_sad_avg_batch(const uint8_t *d_src, uint32_t src_stride, size_t src_block_pitch, const uint8_t *d_ref1,
                          uint32_t ref1_stride, size_t ref1_block_pitch, const uint8_t *d_ref2,
                          uint32_t ref2_stride, size_t ref2_block_pitch, uint32_t width, uint32_t height,
                          uint32_t *d_out, size_t nblocks, void *stream);

/* K5 SAD search (NxMSadLoopKernel_funcPtrArray, EbComputeSAD.h:199; C:
 * sad_loop_kernel, EbComputeSAD_C.c:72-120).  Per block b: source block at
 * d_src + b*src_block_pitch, reference window origin at d_ref + b*ref_block_pitch.
 * Outputs: best_sad (uint64), x/y search centre (int16), first minimum in raster
 * order.  Limits: width, height <= 64; window must fit the LDS budget
 * (else SVT_HIP_ERR_INVALID). */
int svt_hip_sad_search_batch(const uint8_t *d_src, uint32_t src_stride, size_t src_block_pitch,
                             const uint8_t *d_ref, uint32_t ref_stride, uint32_t ref_stride_raw,
                             size_t ref_block_pitch, uint32_t width, uint32_t height,
                             int16_t search_area_width, int16_t search_area_height,
                             uint64_t *d_best_sad, int16_t *d_x, int16_t *d_y, size_t nblocks,
                             void *stream);

/* The same search addressed on picture planes (frame-level HME): block b's source
 * block starts at d_src_plane + d_src_offsets[b] and its search window at d_ref_plane +
 * d_ref_offsets[b] (uint32 byte offsets; the caller clips windows to the padded picture exactly as
 * HmeLevel0 does, EbMotionEstimation.c:5720-5798). */
int svt_hip_sad_search_planes_batch(const uint8_t *d_src_plane, uint32_t src_stride,
                                    const uint32_t *d_src_offsets, const uint8_t *d_ref_plane,
                                    uint32_t ref_stride, uint32_t ref_stride_raw,
                                    const uint32_t *d_ref_offsets, uint32_t width, uint32_t height,
                                    int16_t search_area_width, int16_t search_area_height,
                                    uint64_t *d_best_sad, int16_t *d_x, int16_t *d_y, size_t nblocks,
                                    void *stream);

/* K6 ME multi-size SAD: full-pel search of 64x64 superblocks for all 85 PUs.
 * Replaces FullPelSearch_LCU's inner calls (EbMotionEstimation.c:3199-3247 ->
 * GetSearchPointResults :2932 -> SadCalculation_8x8_16x16 / _32x32_64x64 tables :145-199;
 * C: :208-311).  Per SB b: source d_src + b*src_block_pitch (64x64, src_stride),
 * reference window origin d_ref + b*ref_block_pitch (ref_stride), search area
 * search_w x search_h (<= 4096 points), area origin (x, y) from d_origins[b][2] or,
 * when NULL, the uniform x_origin / y_origin.  d_best_sad / d_best_mv: uint32[n][85],
 * IN/OUT running bests exactly like the reference's p_best_sad8x8[64] | 16x16[16] |
 * 32x32[4] | 64x64[1] (and p_best_mv*) arrays back to back; the caller initialises
 * them (reference: MAX_SAD_VALUE, EbMotionEstimation.h:79). */
#define SVT_HIP_ME_PUS 85
int svt_hip_me_sb_search_batch(const uint8_t *d_src, uint32_t src_stride, size_t src_block_pitch,
                               const uint8_t *d_ref, uint32_t ref_stride, size_t ref_block_pitch,
                               int search_w, int search_h, const int16_t *d_origins, int x_origin,
                               int y_origin, uint32_t *d_best_sad, uint32_t *d_best_mv,
                               size_t nblocks, void *stream);

/* K6 on picture planes: SB b's source at d_src_plane + d_src_offsets[b], window origin at d_ref_plane +
 * d_ref_offsets[b] (all SBs x reference pictures of a segment in one launch; FullPelSearch_LCU's
 * pointer arithmetic, EbMotionEstimation.c:3210-3225, done once on the host). */
int svt_hip_me_sb_search_planes_batch(const uint8_t *d_src_plane, uint32_t src_stride,
                                      const uint32_t *d_src_offsets, const uint8_t *d_ref_plane,
                                      uint32_t ref_stride, const uint32_t *d_ref_offsets, int search_w,
                                      int search_h, const int16_t *d_origins, int x_origin, int y_origin,
                                      uint32_t *d_best_sad, uint32_t *d_best_mv, size_t nblocks,
                                      void *stream);

/* Hierarchical motion estimation, one LEVEL per call for all SBs (x references x search regions, as separate tasks) of a
 * picture: HmeLevel0 / HmeLevel1 / HmeLevel2 (EbMotionEstimation.c:5689, 5883, 6016; called per SB at :7739-7830) INCLUDING
 * the search-area placement and clipping the reference does per SB on the host (:5729-5798).  Per task t:
 *   d_sb_origin[t] = (x, y) of the SB and d_sb_size[t] = (width, height), at the level's resolution (origin >> 2 / >> 1 / >> 0);
 *   width 1..64, height 2..64 (the reference's SBs); an entry outside that range gets best_sad = 2^64 - 1 and mv = (0, 0);
 *   search centre  = d_centers[t] >> center_shift (NULL: (0, 0)): level 0 takes the caller's centre, level 1 the level-0
 *                    result >> 1, level 2 the level-1 result (the reference's call sites), so the levels chain ON THE DEVICE;
 *   d_src_pic / d_ref_pic point at sample (0, 0) of the level's source / padded reference picture (the reference buffer
 *                    must be readable from -pad to size + pad, as the encoder's padded pictures are);
 *   outputs        d_best_sad[t] (uint64: SAD on every other row x 2) and d_mv[t] = (x, y) scaled to full resolution -
 *                    exactly hmeLevelNSad[][] and x/yHmeLevelNSearchCenter[][] of MotionEstimateLcu.
 * params: svt_hip_hme_level_params() derives them from the encoder's context values. */
typedef struct svt_hip_hme_params {
    int32_t search_area_width, search_area_height;    /* before clipping: L0 ((w * mult / 100) + 15) & ~15, h * mult / 100; L1 / L2 (w + 7) & ~7, h */
    int32_t x_origin_offset, y_origin_offset;         /* origin = offset + centre: L0 -(total * mult / 100 >> 1) + preceding regions; L1 / L2 -(area >> 1) */
    int32_t pad_width, pad_height;                    /* reference origin - 1 (L0, L1), BLOCK_SIZE_64 - 1 (L2) */
    int32_t ref_width, ref_height;                    /* reference picture size at this level */
    int32_t round_down;                               /* 16 (L0) or 8: width rounded down after clipping unless smaller */
    int32_t mv_shift;                                 /* 2, 1, 0 */
} svt_hip_hme_params;
int svt_hip_hme_level_params(int level, const uint16_t *hme_search_area_in_width_array,
                             const uint16_t *hme_search_area_in_height_array, uint32_t region_in_width,
                             uint32_t region_in_height, uint32_t level0_total_search_area_width,
                             uint32_t level0_total_search_area_height, uint32_t search_area_multiplier_x,
                             uint32_t search_area_multiplier_y, uint32_t ref_origin_x, uint32_t ref_origin_y,
                             uint32_t ref_width, uint32_t ref_height, svt_hip_hme_params *params);
int svt_hip_hme_level_batch(const uint8_t *d_src_pic, uint32_t src_stride, const uint8_t *d_ref_pic, uint32_t ref_stride,
                            const int16_t *d_sb_origin, const uint16_t *d_sb_size, const int16_t *d_centers,
                            int center_shift, const svt_hip_hme_params *params, uint64_t *d_best_sad, int16_t *d_mv,
                            size_t ntasks, void *stream);
/* The same for 1 .. 4 search regions of the level in ONE launch (the reference walks number_hme_search_region_in_width x
 * _in_height regions per SB and carries each region's vector through the next levels, EbMotionEstimation.c:7700-7950):
 * params[nregions]; d_centers / d_best_sad / d_mv are [region][task] planes (d_centers may be NULL at level 0). */
int svt_hip_hme_level_regions_batch(const uint8_t *d_src_pic, uint32_t src_stride, const uint8_t *d_ref_pic,
                                    uint32_t ref_stride, const int16_t *d_sb_origin, const uint16_t *d_sb_size,
                                    const int16_t *d_centers, int center_shift, const svt_hip_hme_params *params, int nregions,
                                    uint64_t *d_best_sad, int16_t *d_mv, size_t ntasks, void *stream);

/* K6 with the encoder's own result rows: d_best_sad / d_best_mv hold, per SB, pu_pitch uint32 whose first 85 (nsq = 0)
 * or 209 (nsq != 0) entries are MeContext_t.p_sb_best_sad[list][ref][..] / p_sb_best_mv[..] in EbMeTierZeroPu order
 * (EbMotionEstimationContext.h:47-270): 64x64, 32x32 x4, 16x16 x16, 8x8 x64 and, for the non-square search
 * open_loop_me_fullpel_search_sblock (EbMotionEstimation.c:3251; picked at :8114 when nsq_search_level is between LEVEL1 and
 * FULL), 64x32 x2, 32x16 x8, 16x8 x32, 32x64 x2, 16x32 x8, 8x16 x32, 32x8 x16, 8x32 x16, 64x16 x4, 16x64 x4.  IN/OUT running
 * bests as in svt_hip_me_sb_search_batch (initialise with MAX_SAD_VALUE = 128*128*255).  Sources / windows are dense
 * (d_*_offsets == NULL: block b at b * *_block_pitch) or addressed on planes by byte offsets.
 *
 * flavour: which of the reference's kernel sets the results are bit-identical to.
 *   SVT_HIP_FLAVOUR_C     its scalar C / SSE4.1 kernels (asm_type 0) - the parity target BASELINE.json names;
 *   SVT_HIP_FLAVOUR_AVX2  its AVX2 kernels as GCC / clang compile them (asm_type 1, the only value the encoder accepts,
 *                         EbEncHandle.c:2676).  They differ from the C kernels in three places, all restated exactly
 *                         (oracle/pixel.c, pinned by tests/golden/me.npz): the 32x32 motion vectors of the 8-search-point
 *                         kernel (lane swap under __GNUC__, EbComputeSAD_Intrinsic_AVX2.c:3989-4001) and, for the
 *                         non-square search on widths that are not a multiple of 8, ExtSadCalculation's stale-`sad` test
 *                         (both flavours, EbMotionEstimation.c:732-736) and the AVX2 single-point kernel's source-stride
 *                         row fetch (EbComputeSAD_Intrinsic_AVX2.c:50-52).  With the last one the kernel reads reference
 *                         bytes up to 8 * src_stride + 64 past a 16x16 block's window origin: the caller's reference
 *                         buffer must cover that, as the encoder's padded pictures do. */
enum { SVT_HIP_FLAVOUR_C = 0, SVT_HIP_FLAVOUR_AVX2 = 1 };
#define SVT_HIP_ME_PUS_ALL 209
int svt_hip_me_fullpel_search_batch(const uint8_t *d_src, uint32_t src_stride, size_t src_block_pitch,
                                    const uint32_t *d_src_offsets, const uint8_t *d_ref, uint32_t ref_stride,
                                    size_t ref_block_pitch, const uint32_t *d_ref_offsets, int search_w,
                                    int search_h, const int16_t *d_origins, int x_origin, int y_origin,
                                    int flavour, int nsq, uint32_t *d_best_sad, uint32_t *d_best_mv,
                                    uint32_t pu_pitch, size_t nblocks, void *stream);

/* ---- MotionEstimateLcu's per-SB glue around the full-pel search (EbMotionEstimation.c:7527) ---------------------
 * (1) svt_hip_me_setup_batch: between the HME levels and the search - per task (SB x reference picture) the search centre
 *     (first strict minimum of the last enabled HME level's SADs over its search regions, :7849-7941; for list 1 of a picture
 *     whose two references are the same picture the second entry of the reference's region sort, :7906-7936; SBs that are not
 *     64 rows high take no HME result, :7678), CheckZeroZeroCenter (:6844-6930, run when zz_check = is_used_as_reference_flag)
 *     and the search area: width rounded up to 8, centred, clipped against the picture in the reference's statement order,
 *     width rounded down to 8 unless below 8 (:7955-8040).
 *       d_src_pic / d_ref_pic    sample (0, 0) of the padded 8-bit source / reference luma planes (>= 63 + 64 samples of padding)
 *       d_sb_origin / d_sb_size  [n][2] (x, y) / (width, height) of the SBs
 *       d_hme_sad / d_hme_mv     [region][n] / [region][n][2] outputs of the last enabled level (svt_hip_hme_level_regions_batch),
 *                                region r = rh * regions_w + rw; NULL (or regions 0 x 0): no HME, every centre is (0, 0)
 *       d_center (may be NULL)   [n][2] the centre after CheckZeroZeroCenter;  d_area  [n][4] x_origin, y_origin, width, height
 * (2) svt_hip_me_fullpel_search_areas_batch: svt_hip_me_fullpel_search_batch with ONE AREA PER SB, read on the device from
 *     d_areas (so a picture's interior and clipped edge SBs share one launch and nothing returns to the host in between).
 *     d_ref_offsets[b] is the byte offset of the SB's CO-LOCATED position in the reference plane; the window starts at that
 *     position + the area's origin.  max_search_w / _h bound every area of the call (they size the LDS window: the nominal
 *     area, width rounded up to 8); an area outside 1 .. max is skipped (its rows keep their incoming values).
 * (3) svt_hip_me_bipred_batch: BiPredictionSearch (:6639, integer vectors: the SAD of each PU against the rounded average of
 *     its two lists' best blocks; sub_sad = fractionalSearchMethod == SUB_SAD_SEARCH: every other row, doubled) and the
 *     me_results rows MotionEstimateLcu writes (:8308-8440): vectors, up to three (distortion, direction) candidates in the
 *     reference's order (Sort3Elements :6809), candidate count.  Result rows are in RASTER PU order (partitionWidth /
 *     puSearchIndexMap, EbMotionEstimation.h:178-315) and read the SAD / vector rows at the storage index of the same rectangle
 *     (svt_hip_me_pu_storage_index).  d_best_sad1 / d_best_mv1 NULL: P picture, one candidate.  bipred_all_pus = (cu8x8_mode ==
 *     CU_8x8_MODE_0 || pic_depth_mode <= PIC_ALL_C_DEPTH_MODE): otherwise only PUs 0 .. 20 are bi-predicted (:8297).  npus 85 or
 *     209.  me_nsq[] of the reference's rows is not produced (the reference forces is_nsq_table_used off, :7633).
 *     Every entry of both outputs is written: all pu_pitch entries of an SB's d_bipred_sad row (may be NULL), 0 where no
 *     bi-prediction is made (P pictures, PUs past 20 without bipred_all_pus, entries past the PU count), and all npus result rows. */
typedef struct svt_hip_me_setup_params {
    int32_t picture_width, picture_height;        /* SequenceControlSet luma_width / luma_height: the search area's clip */
    int32_t ref_width, ref_height;                /* refPicPtr->width / height: the clip of the HME centre in CheckZeroZeroCenter */
    int32_t search_area_width, search_area_height;/* MeContext_t values, before the round-up to 8 */
    int32_t regions_w, regions_h;                 /* number_hme_search_region_in_width / _height (1 or 2 each; 0: no HME) */
    int32_t second_best;                          /* HME level 2 on && list 1 && ref_pic_poc_array[0] == [1] (needs regions_w == regions_h) */
    int32_t zz_check;                             /* is_used_as_reference_flag */
} svt_hip_me_setup_params;
int svt_hip_me_setup_batch(const uint8_t *d_src_pic, uint32_t src_stride, const uint8_t *d_ref_pic, uint32_t ref_stride,
                           const int16_t *d_sb_origin, const uint16_t *d_sb_size, const uint64_t *d_hme_sad,
                           const int16_t *d_hme_mv, const svt_hip_me_setup_params *params, int16_t *d_center, int16_t *d_area,
                           size_t ntasks, void *stream);
int svt_hip_me_fullpel_search_areas_batch(const uint8_t *d_src, uint32_t src_stride, const uint32_t *d_src_offsets,
                                          const uint8_t *d_ref, uint32_t ref_stride, const uint32_t *d_ref_offsets,
                                          const int16_t *d_areas, int max_search_w, int max_search_h, int flavour, int nsq,
                                          uint32_t *d_best_sad, uint32_t *d_best_mv, uint32_t pu_pitch, size_t nblocks,
                                          void *stream);
typedef struct svt_hip_me_result {                /* MeCuResults_t (EbMotionEstimationLcuResults.h:62-77) without me_nsq */
    int16_t x_mv_l0, y_mv_l0, x_mv_l1, y_mv_l1;
    uint32_t distortion[3];
    uint8_t direction[3];                         /* UNI_PRED_LIST_0 0, UNI_PRED_LIST_1 1, BI_PRED 2 */
    uint8_t total_me_candidate_index;
} svt_hip_me_result;
int svt_hip_me_bipred_batch(const uint8_t *d_src_pic, uint32_t src_stride, const uint8_t *d_ref0_pic, uint32_t ref0_stride,
                            const uint8_t *d_ref1_pic, uint32_t ref1_stride, const int16_t *d_sb_origin,
                            const uint32_t *d_best_sad0, const uint32_t *d_best_mv0, const uint32_t *d_best_sad1,
                            const uint32_t *d_best_mv1, uint32_t pu_pitch, int npus, int bipred_all_pus, int sub_sad,
                            uint32_t *d_bipred_sad, svt_hip_me_result *d_results, size_t nsb, void *stream);
/* HOST helper: index in the SAD / vector rows (EbMeTierZeroPu order) of raster PU `pu_index` (0 .. 208), or -1; the
 * reference's tab8x8 / tab16x16 / tab32x16 ... tables (EbMotionEstimation.h:90-175), derived from the rectangles */
int svt_hip_me_pu_storage_index(int pu_index);

/* ---- MotionEstimateLcu for a whole picture (EbMotionEstimation.c:7527; the per-picture entry of the motion estimation stage) ----
 * svt_hip_motion_estimate_frame runs, for every 64x64 SB of a picture in raster order and for list 0 (P) or lists 0 and 1 (B),
 * what the stage calls above run when they are chained: the enabled HME levels over all search regions, the best region (the
 * second entry of the reference's region sort for list 1 of a picture whose two references are the same picture; no HME centre
 * at all for that list on a base-layer picture, :7656), CheckZeroZeroCenter, the search area's round-up / clip / round-down, the
 * full-pel search over that area (85 or 209 PUs) and BiPredictionSearch with the me_results rows.  It derives the SB origins,
 * the plane offsets and the svt_hip_hme_params rows itself and issues three launches (prologue, search, bi-prediction); nothing
 * is allocated, nothing returns to the host, the call only enqueues and can be captured into a HIP graph.  Sub-pel refinement
 * is outside this call (use_subpel_flag = 0), as for the stage calls; svt_hip_motion_estimate_subpel_frame below runs it.
 *
 * Pictures: a pyramid is the padded 8-bit luma picture and its 1/4 and 1/16 decimations (svt_hip_picture_pad / _decimate), level
 * k = 0 full, 1 quarter, 2 sixteenth: d_plane[k] is the START of the padded buffer, the picture's sample (0, 0) sits at
 * (origin_x[k], origin_y[k]), rows are stride[k] bytes apart.  Level k's picture is (picture_width >> k) x (picture_height >> k).
 * The padding must be at least 64 >> k samples on every side (origin_x[k], origin_y[k] >= 64 >> k, stride[k] >= origin_x[k] +
 * width + (64 >> k), as many rows below the picture), which the encoder's pictures have (68 / 34 / 17).  n_pictures > 1: a stack
 * of pictures under one parameter set, picture i of every plane at pitch[k] * i bytes (each against ITS OWN references, picture i
 * of ref0 / ref1).  ref1 is NULL for a P picture and required for a B picture.
 *
 * Outputs, all on the device, SB index s = picture * nsb + sb_y * nsbx + sb_x (nsbx = (width + 63) / 64, nsb = nsbx * nsby),
 * nl = 1 (P) or 2 (B):
 *   d_best_sad, d_best_mv  uint32 [s][nl][209]  p_sb_best_sad / p_sb_best_mv of each list in EbMeTierZeroPu order (the order
 *                          svt_hip_me_pu_storage_index maps to); with 85 PUs the entries 85 .. 208 are 0
 *   d_area_origin          int16 [s][nl][2]     x_search_area_origin / y_search_area_origin of each list
 *   d_bipred_sad           uint32 [s][209]      p_sb_bipred_sad (storage order); 0 where no bi-prediction is made (P pictures,
 *                                               PUs past 20 when cu8x8_mode != 0 with 85 PUs)
 *   d_results              [s][209]             the me_results rows in raster PU order, rows past the PU count zeroed
 * d_scratch: svt_hip_motion_estimate_frame_scratch_bytes(params, n_pictures) bytes, 16-byte aligned (the per-SB search areas).
 *
 * Every argument is checked before the first launch (SVT_HIP_ERR_INVALID): NULL planes or outputs, a picture whose sides are not
 * multiples of 8 or exceed 16384, padding or strides below the above, a slice type other than B / P, temporal_layer_index outside
 * 0 .. hierarchical_levels (<= 5), region counts outside 1 .. 2, HME on with no level on, a level's area arrays with a zero,
 * search areas beyond what the stage calls take (more than 4096 points after the width's round-up to 8, or windows beyond their
 * LDS), a PU count other than 85 / 209, an unknown flavour, the same-POC second-best rule on a non-square region grid, and
 * SVT_HIP_FLAVOUR_AVX2 on a picture whose width is not a multiple of 64 while HME level 0 is on: the reference's AVX2 HME kernels
 * are undefined on the 2- .. 12-wide sixteenth blocks of a partial SB column.  n_pictures = 0 is a successful no-op. */
enum { SVT_HIP_SLICE_B = 0, SVT_HIP_SLICE_P = 1 };           /* EB_SLICE */
typedef struct svt_hip_me_pyramid {
    const uint8_t *d_plane[3];
    uint32_t stride[3], origin_x[3], origin_y[3];
    uint64_t pitch[3];                                /* between the pictures of a stack (ignored for n_pictures 1) */
} svt_hip_me_pyramid;
typedef struct svt_hip_me_frame_params {              /* what MotionEstimateLcu reads of its picture, sequence and ME context */
    int32_t picture_width, picture_height;            /* luma_width / luma_height */
    int32_t slice_type;                               /* SVT_HIP_SLICE_B / SVT_HIP_SLICE_P */
    int32_t temporal_layer_index, hierarchical_levels;/* HME_LEVEL_0_SEARCH_AREA_MULTIPLIER_X / _Y [levels][layer] widen level 0 */
    int32_t enable_hme_flag, enable_hme_level0_flag, enable_hme_level1_flag, enable_hme_level2_flag;
    int32_t number_hme_search_region_in_width, number_hme_search_region_in_height;        /* 1 or 2 each */
    int32_t hme_level0_total_search_area_width, hme_level0_total_search_area_height;
    uint16_t hme_search_area_in_width_array[3][2];    /* hme_level{0,1,2}_search_area_in_width_array[region] */
    uint16_t hme_search_area_in_height_array[3][2];
    int32_t search_area_width, search_area_height;    /* before the round-up to 8 */
    int32_t ref_pic_poc[2];                           /* ref_pic_poc_array[list]: only their equality is read */
    int32_t is_used_as_reference_flag;                /* CheckZeroZeroCenter runs */
    int32_t max_number_of_pus_per_sb;                 /* 85: FullPelSearch_LCU; 209: open_loop_me_fullpel_search_sblock (pic_depth_mode <= PIC_ALL_C_DEPTH_MODE) */
    int32_t nsq_search_level;                         /* carried for the caller; the reference forces is_nsq_table_used off (:7633) */
    int32_t cu8x8_mode;                               /* != CU_8x8_MODE_0 with 85 PUs: bi-prediction on PUs 0 .. 20 only (:8305) */
    int32_t fractional_search_method;                 /* SUB_SAD_SEARCH (0): bi-prediction SAD on every other row, doubled */
    int32_t flavour;                                  /* SVT_HIP_FLAVOUR_C / _AVX2 */
} svt_hip_me_frame_params;
size_t svt_hip_motion_estimate_frame_scratch_bytes(const svt_hip_me_frame_params *params, uint32_t n_pictures);    /* 0: bad parameters */
int svt_hip_motion_estimate_frame(const svt_hip_me_pyramid *src, const svt_hip_me_pyramid *ref0, const svt_hip_me_pyramid *ref1,
                                  const svt_hip_me_frame_params *params, uint32_t n_pictures, uint32_t *d_best_sad,
                                  uint32_t *d_best_mv, int16_t *d_area_origin, uint32_t *d_bipred_sad, svt_hip_me_result *d_results,
                                  void *d_scratch, size_t scratch_bytes, void *stream);

/* ---- Sub-pel motion estimation: the half- and quarter-pel refinement of MotionEstimateLcu (use_subpel_flag = 1, which the reference
 * sets for every picture; EbMotionEstimation.c:8162-8236) and BiPredictionSearch on the refined vectors ----
 * svt_hip_me_subpel_frame is the refinement stage alone: for every 64x64 SB, list and picture of a stack it refines the full-pel rows
 * that svt_hip_motion_estimate_frame wrote - InterpolateSearchRegionAVC's three half-pel planes (taps (-2, 18, 18, -2), + 16 >> 5, clipped;
 * plane j is the vertical filter over the ROUNDED plane b), HalfPelSearch_LCU (eight neighbours in the order L R T B TL TR BR BL, strict
 * '<'; the direction is the first equality in the order L R T B TL TR BL BR) and QuarterPelSearch_LCU (the eight rounded averages of two
 * planes per case (y & 2) + ((x & 2) >> 1), masked by the half-pel direction).  All three values of fractional_search_method are
 * served: SUB_SAD_SEARCH 0 (every other row, doubled), FULL_SAD_SEARCH 1, SSD_SEARCH 2 (the decision is on the SSE, starting from the
 * full-pel winner's; the SAD row takes the SAD of the position that won).  The reference's quirks are kept: the 64x64 PU's quarter-pel
 * pass measures a 32x32 block (:4809), so its SAD row usually ends as a 32x32 distortion; the quarter pass addresses its planes by
 * ((mv + 2) >> 2) - origin on negative vectors too.
 *   d_best_sad, d_best_mv    uint32 [s][nl][209], in / out (s, nl as above): vectors in quarter-pel units (uint16 y << 16 | uint16 x)
 *   d_best_ssd (may be NULL) uint32 [s][nl][209], out: p_sb_best_ssd under SSD_SEARCH, 0 otherwise and for PUs not refined
 *   d_half_dir (may be NULL) uint8 [s][nl][209], out: psubPelDirection (TOP_LEFT 0, TOP 1, TOP_RIGHT 2, RIGHT 3, BOTTOM_RIGHT 4,
 *                            BOTTOM 5, BOTTOM_LEFT 6, LEFT 7), 0 for PUs whose half-pel pass is off
 * params: picture_width / _height, slice_type, max_number_of_pus_per_sb, cu8x8_mode (1: the 8x8 PUs are not refined) and
 * fractional_search_method are read.  The pyramids' level 0 is read only.  One launch.  The search-area origins are not an argument: the
 * reference uses them only to address its per-area planes, whose samples depend on the picture position alone.  A PU whose vector points outside what the padding
 * holds (no vector of the search does) keeps its rows.
 *
 * svt_hip_motion_estimate_subpel_frame is svt_hip_motion_estimate_frame with use_subpel_flag = 1 and the reference's enables (all on
 * when `subpel` is NULL): prologue, full-pel search, refinement, bi-prediction on the fractional vectors (BiPredictionCompensation /
 * SelectBuffer / QuarterPelCompensation: a half or integer position reads one plane, a quarter position the rounded average of two) and
 * the me_results rows - four launches, the same outputs in the same layouts, the vectors in quarter-pel units as the reference stores
 * them.  Its scratch is svt_hip_motion_estimate_subpel_frame_scratch_bytes (= the full-pel call's).
 *
 * Padding: the interpolation reads further than the search.  A search area's origin is clipped to 63 samples left of / above the picture
 * and its last point to the picture's last sample; a PU's planes need 2 samples before its block and, the quarter pass starting up to one
 * sample further, 3 after it: samples -65 .. width + 65 (rows likewise).  Level 0 of every pyramid needs origin_x, origin_y >= 66,
 * stride >= origin_x + width + 66 and as many rows below the picture; the encoder's 68 pass.  (The reference interpolates the whole
 * ROUND_UP_MUL_8(width + 2)-wide region and reads up to 72 samples right of the picture; those samples are never used.)
 * Both calls only enqueue, allocate nothing, do not synchronise and can be captured into a HIP graph; every argument is checked before
 * the first launch (SVT_HIP_ERR_INVALID), svt_hip_me_subpel_check runs those checks alone (no device needed; d_* may be any non-NULL
 * addresses).  svt_hip_me_subpel_planes writes B / H / J (the samples left of, above and above-left of each integer position) of the
 * w x h window at (x0, y0) of a reference's level 0 into d_planes [3][h][w]: the interpolation by itself, for pinning. */
typedef struct svt_hip_me_subpel_params {
    int32_t fractional_search64x64;                   /* the 64x64 PU is refined (half and quarter) */
    int32_t enable_half_pel32x32, enable_half_pel16x16, enable_half_pel8x8;
    int32_t enable_quarter_pel;                       /* the 32x32, 16x16 and 8x8 PUs; the non-square PUs of a 209-PU search always run both */
} svt_hip_me_subpel_params;
int svt_hip_me_subpel_check(const svt_hip_me_pyramid *src, const svt_hip_me_pyramid *ref0, const svt_hip_me_pyramid *ref1,
                            const svt_hip_me_frame_params *params, const svt_hip_me_subpel_params *subpel, uint32_t n_pictures,
                            const uint32_t *d_best_sad, const uint32_t *d_best_mv, const uint32_t *d_best_ssd, const uint8_t *d_half_dir);
int svt_hip_me_subpel_frame(const svt_hip_me_pyramid *src, const svt_hip_me_pyramid *ref0, const svt_hip_me_pyramid *ref1,
                            const svt_hip_me_frame_params *params, const svt_hip_me_subpel_params *subpel, uint32_t n_pictures,
                            uint32_t *d_best_sad, uint32_t *d_best_mv, uint32_t *d_best_ssd, uint8_t *d_half_dir, void *stream);
size_t svt_hip_motion_estimate_subpel_frame_scratch_bytes(const svt_hip_me_frame_params *params, uint32_t n_pictures);    /* 0: bad parameters */
int svt_hip_motion_estimate_subpel_frame(const svt_hip_me_pyramid *src, const svt_hip_me_pyramid *ref0, const svt_hip_me_pyramid *ref1,
                                         const svt_hip_me_frame_params *params, const svt_hip_me_subpel_params *subpel, uint32_t n_pictures,
                                         uint32_t *d_best_sad, uint32_t *d_best_mv, int16_t *d_area_origin, uint32_t *d_bipred_sad,
                                         svt_hip_me_result *d_results, void *d_scratch, size_t scratch_bytes, void *stream);
int svt_hip_me_subpel_planes(const svt_hip_me_pyramid *ref, int32_t picture_width, int32_t picture_height, int32_t x0, int32_t y0,
                             uint32_t w, uint32_t h, uint8_t *d_planes, void *stream);

/* K7 coefficient-domain distortion (full_distortion_kernel32_bits_func_ptr_array /
 * full_distortion_kernel_cbf_zero32_bits_func_ptr_array, EbPictureOperators.h:268-280;
 * C: EbPictureOperators.c:283-346).  d_out: uint64[nblocks][2] =
 * {DIST_CALC_RESIDUAL, DIST_CALC_PREDICTION}.  cbf_zero: d_recon is ignored. */
int svt_hip_full_distortion32_batch(const int32_t *d_coeff, uint32_t coeff_stride,
                                    size_t coeff_block_pitch, const int32_t *d_recon,
                                    uint32_t recon_stride, size_t recon_block_pitch,
                                    uint32_t width, uint32_t height, int cbf_zero,
                                    uint64_t *d_out, size_t nblocks, void *stream);

/* picture_full_distortion32_bits (EbPictureOperators.c:349-457), luma leg, for nblocks transform blocks: a 64-sample
 * dimension covers 32 coefficients, both buffers are dense with the (clamped) width as row stride and lie *_block_pitch
 * int32 apart, d_count_non_zero_coeffs[b] == 0 selects the cbf_zero kernel for block b (NULL: never).  flavour
 * SVT_HIP_FLAVOUR_AVX2 reproduces full_distortion_kernel32_bits_avx2's residual sum, which adds the low and high halves
 * of its 64-bit lanes separately (_mm256_add_epi32, EbPictureOperators_Intrinsic_AVX2.c:1989): it differs from the C
 * kernel once a lane's low halves sum past 2^32 (tests/golden/pins.npz holds both). */
int svt_hip_picture_full_distortion32_batch(const int32_t *d_coeff, size_t coeff_block_pitch, const int32_t *d_recon,
                                            size_t recon_block_pitch, uint32_t bwidth, uint32_t bheight,
                                            const uint32_t *d_count_non_zero_coeffs, int flavour, uint64_t *d_out,
                                            size_t nblocks, void *stream);

/* The luma mode-decision full loop, fused: ProductFullLoop (EbFullLoop.c:724-925) and ProductFullLoopTxSearch (:927-1100) for many
 * (transform size, type list) groups in one call.  Per block of a group and per type of its list, in the list's order:
 *   residual = src - pred                                          (ResidualKernel, EbProductCodingLoop.c:1969; 8-bit, BIT_INCREMENT_8BIT
 *                                                                   at EbFullLoop.c:799 / :1026)
 *   coeff, three_quad_energy = av1_estimate_transform(DEFAULT_SHAPE) (:763, EbTransforms.c:4918; partial-frequency shapes are compiled
 *                                                                   out of the reference)
 *   qcoeff, dqcoeff, eob = av1_quantize_inv_quantize               (flat qmatrix: aom_highbd_quantize_b{,_32x32,_64x64}; :650 eob ==
 *                                                                   count_non_zero_coeffs)
 *   dist[2] = picture_full_distortion32_bits(coeff, dqcoeff, eob)  (EbPictureOperators.c:349-400: {DIST_CALC_RESIDUAL, _PREDICTION};
 *                                                                   eob 0: the cbf_zero kernel, {sum c^2, sum c^2}; flavour as in
 *                                                                   svt_hip_picture_full_distortion32_batch)
 *   dist[i] = RIGHT_SIGNED_SHIFT(dist[i] + three_quad_energy, (1 - av1_get_tx_scale(tx_size)) * 2)      (:829-835, :1062-1068)
 * coeff and dqcoeff never leave the device's registers unless d_qcoeff / d_dqcoeff ask for them.  The rate of the coefficients
 * (Av1TuEstimateCoeffBits) is svt_hip_coeff_rate_frame below, which reads d_qcoeff / d_eob where this call leaves them.  Left to
 * the caller: the skip of a non-DCT type whose eob is 0 (:1034) and the allowed type set (:952-984).
 * Blocks: d_*_xy[b] = x | y << 16 on a plane with the given row stride (in samples), or NULL: dense W * H samples per block (many
 * candidates of one source block each repeat its origin in d_src_xy).  d_iscan: ntypes consecutive iscans of min(W,32) * min(H,32)
 * entries in tx_types order (8-byte aligned); d_dist / d_qcoeff / d_dqcoeff 16-byte aligned.  One quantiser row set per call (the MD
 * tables at the picture's qindex); quant_shift must be a power of two (every av1_build_quantizer table is), else
 * SVT_HIP_ERR_INVALID.  Every argument, empty groups' tx_size / types included, is validated before the first launch; the call
 * only enqueues work (one launch per register class and per 16 groups) and can be captured into a HIP graph. */
typedef struct svt_hip_full_loop_group {
    const void *d_src;  uint32_t src_stride;  const uint32_t *d_src_xy;   /* source plane + block origins; NULL xy: dense */
    const void *d_pred; uint32_t pred_stride; const uint32_t *d_pred_xy;  /* candidate predictions, same addressing */
    uint32_t nblocks;
    int32_t tx_size;
    int32_t ntypes;  uint8_t tx_types[16];      /* 1 .. 16 distinct types, each defined for tx_size */
    const int16_t *d_iscan;                      /* ntypes x min(W,32) * min(H,32), in tx_types order */
    uint64_t *d_dist;                            /* [nblocks][ntypes][2] {DIST_CALC_RESIDUAL, DIST_CALC_PREDICTION}, shifted */
    uint16_t *d_eob;                             /* [nblocks][ntypes] (== y_count_non_zero_coeffs) */
    int32_t *d_qcoeff, *d_dqcoeff;               /* optional (NULL: not written), [nblocks][ntypes][min(W,32) * min(H,32)] */
} svt_hip_full_loop_group;
int svt_hip_full_loop_frame(const svt_hip_full_loop_group *groups, int ngroups, int flavour,
                            const int16_t *zbin, const int16_t *round, const int16_t *quant,
                            const int16_t *quant_shift, const int16_t *dequant, void *stream);

/* The coefficient rate of quantised blocks, what ProductFullLoopTxSearch gets from Av1TuEstimateCoeffBits (EbFullLoop.c:1070-1098):
 * per (block, type) of a group
 *   eob > 0   av1_cost_coeffs_txb (EbRateDistortionCost.c:412-519) WITHOUT its Av1TransformTypeRateEstimation term (:454-461), plus
 *             d_type_bits[block][type] when that array is given (the caller's transform-type rate)
 *   eob == 0  av1_cost_skip_txb (:401-410): txb_skip_cost[txb_skip_ctx][1]; no coefficient is read
 * as the reference's int32 cost widened to uint64_t.  d_qcoeff / d_eob / d_iscan / tx_types are svt_hip_full_loop_group's, as that
 * call writes and reads them, so the full loop feeds this call without a host copy.  The level map (av1_txb_init_levels), the
 * coefficient contexts (av1_get_nz_map_contexts; the reference has only an SSE2 implementation of it, the kernel follows the AV1
 * specification's get_nz_map_ctx) and get_br_ctx are computed on the device and never stored.
 * Cost tables are the caller's data, device-resident: d_coeff_cost is ONE LV_MAP_COEFF_COST as its 529 int32 words in declaration
 * order (EbMdRateEstimation.h:34-41: txb_skip_cost[13][2], base_eob_cost[4][3], base_cost[42][4], eob_extra_cost[22][2],
 * dc_sign_cost[3][2], lps_cost[21][13]), d_eob_cost ONE LV_MAP_EOB_COST ([2][11]): coeffFacBits[txs_ctx][plane] and
 * eobFracBits[eob_multi_size][plane] of the group's size, the two indices from svt_hip_coeff_cost_index (a host helper that needs
 * no device).  Costs must keep a block's sum inside int32, as in the reference.
 * Every argument, empty groups' tx_size / types included, is validated before the first launch (SVT_HIP_ERR_INVALID: a bad size, a
 * type not defined for it or listed twice, a NULL member other than d_type_bits, nblocks * ntypes above 2^31 - 1, d_qcoeff not
 * 16-byte, d_iscan / d_bits not 8-byte, an int32 table not 4-byte aligned).  The contexts are device data and are clamped there
 * (d_txb_skip_ctx to 0 .. 12, d_dc_sign_ctx to 0 .. 2, an eob to the coefficient count): an out-of-range value gives an unspecified
 * cost for its block and does not fault.  The call only enqueues work (one launch per 32 groups), allocates nothing and can be
 * captured into a HIP graph. */
typedef struct svt_hip_coeff_rate_group {
    int32_t tx_size; int32_t ntypes; uint8_t tx_types[16];
    uint32_t nblocks;
    const int32_t *d_qcoeff;      /* [nblocks][ntypes][min(W,32)*min(H,32)]: svt_hip_full_loop_group.d_qcoeff as written */
    const uint16_t *d_eob;        /* [nblocks][ntypes] */
    const int16_t *d_iscan;       /* ntypes iscans, as in the full-loop group */
    const uint8_t *d_txb_skip_ctx, *d_dc_sign_ctx;   /* [nblocks]; 0..12 and 0..2 */
    const int32_t *d_type_bits;   /* optional [nblocks][ntypes], added where eob > 0 (the caller's transform-type rate); NULL: 0 */
    const int32_t *d_coeff_cost;  /* 529 words, one LV_MAP_COEFF_COST */
    const int32_t *d_eob_cost;    /* 22 words, one LV_MAP_EOB_COST */
    uint64_t *d_bits;             /* [nblocks][ntypes] */
} svt_hip_coeff_rate_group;
int svt_hip_coeff_rate_frame(const svt_hip_coeff_rate_group *groups, int ngroups, void *stream);
/* HOST: which coeffFacBits / eobFracBits entry a transform size reads: txs_ctx = (txsize_sqr_map + txsize_sqr_up_map + 1) >> 1 and
 * eob_multi_size = txsize_log2_minus4 (either pointer may be NULL).  SVT_HIP_OK or SVT_HIP_ERR_INVALID (a bad tx_size). */
int svt_hip_coeff_cost_index(int tx_size, int *txs_ctx, int *eob_multi_size);

/* The end of ProductFullLoopTxSearch (EbFullLoop.c:927-1124; encode_pass_tx_search :1127-1323 is the same loop): the RD cost of every
 * (block, type), the best type of every block and that type's coefficients, from the tables the two calls above write.  Per block,
 * for i = 0 .. ntypes - 1 in the list's order, in uint64 arithmetic that wraps as the reference's does:
 *   type i is skipped when d_eob[i] == 0 and tx_types[i] != DCT_DCT                                   (:1034)
 *   cost_i = ((d_bits[i] * lambda + 256) >> 9) + d_dist[i][DIST_CALC_RESIDUAL] * 128                    (av1_tu_calc_cost_luma,
 *            EbRateDistortionCost.c:2120-2194: RDCOST, EbRateDistortionCost.h:73, with LUMA_WEIGHT 1, AV1_COST_PRECISION 0 and
 *            AV1_PROB_COST_SHIFT 9; its zero-cbf branch is compiled to UINT64_MAX, :2176-2191)
 *   the winner is the first i with cost_i < best, best starting at UINT64_MAX                           (:940, :1102)
 * A block without a candidate (every eob 0 in a list without DCT_DCT, or every cost UINT64_MAX) gets cost UINT64_MAX, tx_type
 * DCT_DCT (the reference's initial best_tx_type), type_index 0xFF and zeros elsewhere.  d_best_qcoeff / d_best_dqcoeff, when given,
 * receive the winner's min(W,32) * min(H,32) coefficients; a winner whose eob is 0, or no winner, gives zeros and its input is not
 * read.  Only the winner's position, which is below ntypes by construction, addresses memory from device data.
 * Every argument, empty groups' tx_size / types included, is validated before the first launch (SVT_HIP_ERR_INVALID: a bad size, a
 * type not defined for it or listed twice, nblocks * ntypes above 2^31 - 1, a NULL d_dist / d_eob / d_bits / d_decision, a d_best_*
 * without its input or equal to it, d_dist or a coefficient array not 16-byte, d_bits / d_decision not 8-byte, d_eob not 2-byte
 * aligned).  The call only enqueues work (one launch per 32 groups), allocates nothing and can be captured into a HIP graph. */
typedef struct svt_hip_tx_decision {        /* one per block; sizeof 40, 8-byte aligned */
    uint64_t cost;       /* the winner's y_full_cost; UINT64_MAX when there is no candidate */
    uint64_t dist[2];    /* the winner's {DIST_CALC_RESIDUAL, DIST_CALC_PREDICTION} as given */
    uint64_t bits;       /* the winner's d_bits entry */
    uint16_t eob;        /* the winner's eob */
    uint8_t  tx_type;    /* best_tx_type (DCT_DCT when there is no candidate, the reference's initial value) */
    uint8_t  type_index; /* its position in tx_types; 0xFF: no candidate */
    uint8_t  has_coeff;  /* eob != 0 (the bit av1_tu_calc_cost_luma ors into y_has_coeff) */
    uint8_t  pad[3];     /* written as 0 */
} svt_hip_tx_decision;
typedef struct svt_hip_tx_decide_group {
    int32_t tx_size; int32_t ntypes; uint8_t tx_types[16];   /* as svt_hip_coeff_rate_group: defined for the size, distinct */
    uint32_t nblocks;
    uint32_t lambda;                       /* ModeDecisionContext_t.full_lambda (uint32 in the reference) */
    const uint64_t *d_dist;                /* [nblocks][ntypes][2], the full loop's, 16-byte aligned */
    const uint16_t *d_eob;                 /* [nblocks][ntypes] */
    const uint64_t *d_bits;                /* [nblocks][ntypes], the rate call's (type bits already inside) */
    const int32_t *d_qcoeff, *d_dqcoeff;   /* optional [nblocks][ntypes][NC], NC = min(W,32)*min(H,32), 16-byte aligned */
    svt_hip_tx_decision *d_decision;       /* [nblocks] */
    int32_t *d_best_qcoeff, *d_best_dqcoeff; /* optional [nblocks][NC]: the winner's coefficients; each needs its input */
} svt_hip_tx_decide_group;
int svt_hip_tx_decide_frame(const svt_hip_tx_decide_group *groups, int ngroups, void *stream);

/* The whole transform-type search in one call: svt_hip_full_loop_frame -> svt_hip_coeff_rate_frame -> svt_hip_tx_decide_frame
 * enqueued on `stream`, whose order carries the dependencies (host composition, no kernel of its own).  fl is the full-loop group;
 * its d_dist / d_eob / d_qcoeff / d_dqcoeff may be NULL, the array then lives in d_scratch, as d_bits always does.  Carved per
 * non-empty group in group order, every piece rounded up to 16 bytes: dist, eob, bits, qcoeff (each only when not supplied) and
 * dqcoeff (only when not supplied and d_best_dqcoeff asks for it).  svt_hip_tx_search_scratch_bytes returns their sum, a HOST
 * computation that needs no device: 0 for bad parameters (a NULL list, a bad size / count / type, nblocks * ntypes above 2^31 - 1)
 * and for a call without a non-empty group, which needs no scratch.  All three stages' arguments are validated before the first
 * launch (SVT_HIP_ERR_INVALID, as the three calls; also a scratch that is NULL, not 16-byte aligned or too small). */
typedef struct svt_hip_tx_search_group {
    svt_hip_full_loop_group fl;            /* d_dist / d_eob / d_qcoeff / d_dqcoeff may be NULL: they then live in the scratch */
    const uint8_t *d_txb_skip_ctx, *d_dc_sign_ctx; const int32_t *d_type_bits;   /* as svt_hip_coeff_rate_group */
    const int32_t *d_coeff_cost, *d_eob_cost;
    uint32_t lambda;
    svt_hip_tx_decision *d_decision; int32_t *d_best_qcoeff, *d_best_dqcoeff;    /* as svt_hip_tx_decide_group */
} svt_hip_tx_search_group;
size_t svt_hip_tx_search_scratch_bytes(const svt_hip_tx_search_group *groups, int ngroups);   /* 0: bad parameters */
int svt_hip_tx_search_frame(const svt_hip_tx_search_group *groups, int ngroups, int flavour, const int16_t *zbin, const int16_t *round,
                            const int16_t *quant, const int16_t *quant_shift, const int16_t *dequant,
                            void *d_scratch, size_t scratch_bytes, void *stream);
/* HOST: which row of the caller's transform-type rate tables feeds d_type_bits (Av1TransformTypeRateEstimation,
 * EbRateDistortionCost.c:155-191): *ext_tx_set = get_ext_tx_set(tx_size, is_inter, reduced_tx_set_used) and *square_tx_size =
 * txsize_sqr_map[tx_size] index intraTxTypeFacBits[ext_tx_set][square_tx_size][intra_dir][tx_type] (is_inter 0) or
 * interTxTypeFacBits[ext_tx_set][square_tx_size][tx_type] (either pointer may be NULL).  Returns 1 when a type is coded
 * (get_ext_tx_types > 1 and ext_tx_set > 0), 0 when the term is 0, SVT_HIP_ERR_INVALID for a bad tx_size. */
int svt_hip_tx_type_rate_index(int tx_size, int is_inter, int reduced_tx_set_used, int *ext_tx_set, int *square_tx_size);

/* The CfL alpha search of mode decision: CflPrediction (EbProductCodingLoop.c:1746-1860) without its luma inverse transform, that is
 * cfl_rd_pick_alpha (:1577-1737) and the AV1CostCalcCfl (:1395-1572) runs under it, for many chroma-size groups in one call.  From
 * the luma reconstruction and the DC chroma predictions to per-block alpha_q3_cb / alpha_q3_cr, which svt_hip_frame_cfl_group
 * (svt_hip_encode_recon_frame_ex) and svt_hip_cfl_predict_batch take as they are, without a host round trip.  8-bit samples only,
 * as the reference's mode decision (BIT_INCREMENT_8BIT).
 *
 * svt_hip_cfl_search_frame: THE TABLE.  Per chroma block, once: ac = cfl_luma_subsampling_420_lbd_c of the 2W x 2H luma area at
 * (2x, 2y), subtract_average with round_offset W * H / 2 and num_pel_log2 log2(W * H) (:1774-1789).  Then per plane (0 Cb, 1 Cr) and
 * per candidate a of SVT_HIP_CFL_NALPHA:
 *   pred = cfl_predict_lbd(ac, dc_pred, alpha_q3(a), 8); residual = src - pred; av1_estimate_transform(DEFAULT_SHAPE) (no CfL size is
 *   32x32: FullLoop_R's PF_N2_32X32 branch, EbFullLoop.c:1529-1710, is never taken); the production quantiser with THAT PLANE's rows
 *   (u_* / v_*, :559-579: they differ as soon as the picture has chroma delta-q; quant_shift a power of two, as the full loop);
 *   eob = count_non_zero_coeffs; d_dist = picture_full_distortion32_bits (the cbf-zero kernel at eob 0, flavour as
 *   svt_hip_full_loop_frame), both entries >> 2 (chromaShift, :1803 of CuFullDistortionFastTuMode_R, EbFullLoop.c:1715-1873; no
 *   three_quad_energy); d_bits = av1_cost_coeffs_txb for eob > 0, else av1_cost_skip_txb (Av1TuEstimateCoeffBits, PLANE_TYPE_UV).
 * Sizes: the nine chroma sizes the reference can reach (TX_4X4, 8X8, 16X16, 4X8, 8X4, 8X16, 16X8, 4X16, 16X4); any other tx_size, or
 * a tx_type not defined for the size, is SVT_HIP_ERR_INVALID.  The reference always uses DCT_DCT here (EbModeDecision.c:1976).
 * Two launches: the search kernel (one per 16 groups), which never stores a prediction or a dqcoeff, leaves every candidate's qcoeff
 * and context bytes in d_scratch, where svt_hip_coeff_rate_frame's kernel reads (block, plane, a) as a block with one type.
 * svt_hip_cfl_search_scratch_bytes (HOST, no device needed) is, per non-empty group in group order, nblocks * 66 * W * H * 4 bytes of
 * qcoeff and twice nblocks * 66 context bytes rounded up to 16; 0 for bad parameters (a NULL list, a bad size or type, nblocks * 66
 * above 2^31 - 1) and for a call without a non-empty group.
 * Divergences from the reference.  The first two have no effect on a decision; the third can have one:
 *   - the table always holds all 66 entries; the reference's walk skips some (`if (c > 2 && progress < c) break`), but an entry is a
 *     pure function of (block, plane, a);
 *   - AV1CostCalcCfl's "To check DC" test (cfl_alpha_idx 0 and cfl_alpha_signs 0, :1436 / :1511) is also met by the walk's Cr,
 *     CFL_SIGN_NEG, c = 0 step, which the reference therefore costs at alpha_q3 0 and not -1.  The table's entry [1][1] is the honest
 *     alpha_q3 -1; svt_hip_cfl_decide_frame reads entry [1][0] at that step, as the reference does;
 *   - QUANTISER ROWS.  Of each int16[8] row of svt_hip_qrows only entry [0] (the DC coefficient) and entry [1] (every other
 *     coefficient) are read, as the reference's C quantiser (highbd_quantize_b_helper_c) reads them.  The reference's production AVX2
 *     quantiser reads the lanes: coefficient 0 from [0], coefficient 1 from [1], and every coefficient from the third on from [2 .. 7].
 *     For a row that is {dc, ac, ac, ac, ac, ac, ac, ac} the two agree, and so does this call.  av1_build_quantizer does not build
 *     such a row for v_quant: it fills v_quant[q][2 .. 7] from u_quant[q][1] (EbModeDecisionConfigurationProcess.c:511; every other u /
 *     v row repeats its own [1]).  So in a picture with u_ac_delta_q != v_ac_delta_q the reference encoder quantises the Cr
 *     coefficients from the third on with Cb's AC multiplier and Cr's zbin / round / quant_shift / dequant, while this call uses
 *     Cr's own multiplier v_quant[q][1].  Then the Cr half of the table (qcoeff, d_eob, d_dist, d_bits) can differ from what the
 *     reference encoder computes, and with it the picked alpha or the CfL / DC choice.  With u_ac_delta_q == v_ac_delta_q (this
 *     reference never sets a chroma delta: all are 0) v_quant[q][2 .. 7] equals v_quant[q][1] and the call is bit-exact with the AVX2
 *     path, whatever the DC deltas; that is the case tests/golden/cfl_search.npz pins.  svt_hip_full_loop_frame reads its rows the
 *     same way.
 * Every argument, empty groups' tx_size / tx_type included, is validated before the first launch (SVT_HIP_ERR_INVALID: a NULL member,
 * d_dist not 16-byte, d_iscan / d_bits not 8-byte, d_xy not 4-byte, d_eob not 2-byte aligned, a stride below the block width (luma:
 * twice), a NULL or non-power-of-two quantiser row, a scratch that is NULL, not 16-byte aligned or too small).  Contexts are
 * device data and clamped as in svt_hip_coeff_rate_frame.  The calls only enqueue work on `stream`, allocate nothing and can be
 * captured into a HIP graph. */
#define SVT_HIP_CFL_NALPHA 33   /* a = 0: alpha_q3 0;  a = 1 + 16 * (sign - 1) + c: sign 1 = CFL_SIGN_NEG, 2 = CFL_SIGN_POS, alpha_q3 = -/+ (c + 1), c = 0 .. 15 */
typedef struct svt_hip_qrows { const int16_t *zbin, *round, *quant, *quant_shift, *dequant; } svt_hip_qrows;   /* HOST int16[8] rows; only [0] (DC) and [1] (AC) are read: see QUANTISER ROWS above */
typedef struct svt_hip_cfl_search_group {
    const uint8_t *d_luma_recon; uint32_t luma_stride;        /* sample (0,0) of the luma reconstruction; block at (2x, 2y) */
    const uint8_t *d_src[2];  uint32_t src_stride[2];         /* Cb, Cr source planes */
    const uint8_t *d_pred[2]; uint32_t pred_stride[2];        /* Cb, Cr DC predictions; only read */
    const uint32_t *d_xy;     uint32_t nblocks;               /* chroma origins x | y << 16 */
    int32_t tx_size, tx_type;                                 /* chroma transform block = chroma block (txb_count 1) */
    const int16_t *d_iscan;
    const uint8_t *d_txb_skip_ctx[2], *d_dc_sign_ctx[2];      /* [nblocks] per plane: cb_/cr_txb_skip_context, _dc_sign_context */
    const int32_t *d_coeff_cost, *d_eob_cost;                 /* the PLANE_TYPE_UV tables, as svt_hip_coeff_rate_group */
    uint64_t *d_dist;   /* [nblocks][2 planes][33][2]  {DIST_CALC_RESIDUAL, DIST_CALC_PREDICTION} >> 2 */
    uint64_t *d_bits;   /* [nblocks][2][33] */
    uint16_t *d_eob;    /* [nblocks][2][33] */
} svt_hip_cfl_search_group;
size_t svt_hip_cfl_search_scratch_bytes(const svt_hip_cfl_search_group *groups, int ngroups);   /* HOST; 0: bad parameters or nothing to do */
int svt_hip_cfl_search_frame(const svt_hip_cfl_search_group *groups, int ngroups, int flavour,
                             const svt_hip_qrows *q_cb, const svt_hip_qrows *q_cr,
                             void *d_scratch, size_t scratch_bytes, void *stream);

/* svt_hip_cfl_decide_frame: cfl_rd_pick_alpha's walk (:1587-1735) over the search call's tables, to the letter, one record per block.
 * RDCOST(lambda, R, D) = ((R * lambda + 256) >> 9) + D * 128 in uint64 arithmetic (EbRateDistortionCost.h:73), held and compared as
 * int64_t; sums of costs wrap as two's complement.
 *   alpha zero     per plane, best_rd_uv[PLANE_SIGN_TO_JOINT_SIGN(plane, CFL_SIGN_ZERO, i)][plane] = RDCOST(bits[plane][0] +
 *                  alpha_rate[js][plane][0], dist[plane][0][RESIDUAL]) for i = CFL_SIGN_NEG, CFL_SIGN_POS;
 *   the walk       per plane, per pn_sign, c = 0 .. 15 until `c > 2 && progress < c`: entry a = 1 + 16 * (pn_sign - 1) + c (entry 0 at
 *                  Cr, CFL_SIGN_NEG, c = 0: see above) costed under the three joint signs of i = 0 .. 2; a cost >= the joint sign's
 *                  best is rejected (a tie keeps the earlier candidate), an accepted one sets flag = 2 and, once the other plane has
 *                  a cost for the joint sign, competes with mode_rd + the other plane's best against best_rd (again >= rejects);
 *   against DC     dc_rd = RDCOST(bits[0][0] + bits[1][0], dist[0][0] + dist[1][0]) + RDCOST(d_dc_mode_bits, 0); dc_rd <= best_rd
 *                  picks UV_DC_PRED with index 0, signs 0; else UV_CFL_PRED with ind = (best_c[js][U] << 4) + best_c[js][V] and the
 *                  `best_joint_sign < 0` branch as written (ind 0, signs 0).
 * The two `coeffBits == INT64_MAX` breaks of the reference cannot fire (a rate is an int32 widened) and have no counterpart.
 * alpha_q3 = cfl_idx_to_alpha of the result; a UV_DC_PRED winner has 0 in both, and alpha 0 leaves a prediction unchanged in
 * cfl_predict, so a caller can send every block on.  Only the block index addresses memory from device data.
 * Validated before the launch (SVT_HIP_ERR_INVALID): a NULL member other than d_alpha_q3_*, nblocks * 66 above 2^31 - 1, d_dist not
 * 16-byte, d_bits / d_decision not 8-byte, an int32 array not 4-byte aligned.  One launch per 32 groups; enqueue only. */
typedef struct svt_hip_cfl_decision {     /* sizeof 32, 8-byte aligned */
    int64_t  best_rd;                     /* the CfL side's best_rd; INT64_MAX when no joint sign completed */
    int64_t  dc_rd;                       /* RDCOST(lambda, bits[0][0] + bits[1][0], dist[0][0] + dist[1][0]) + RDCOST(lambda, dc_mode_bits, 0) */
    int32_t  alpha_q3[2];                 /* cfl_idx_to_alpha of the result for Cb, Cr; 0, 0 for UV_DC_PRED */
    uint8_t  uv_mode;                     /* 0 UV_DC_PRED, 13 UV_CFL_PRED */
    uint8_t  cfl_alpha_idx, cfl_alpha_signs;
    uint8_t  pad[5];                      /* written as 0 */
} svt_hip_cfl_decision;
typedef struct svt_hip_cfl_decide_group {
    uint32_t nblocks; uint32_t lambda;                      /* full_lambda */
    const uint64_t *d_dist, *d_bits;                        /* the search call's tables */
    const int32_t *d_alpha_rate;                            /* cflAlphaFacBits[8][2][16], 256 words */
    const int32_t *d_cfl_mode_bits, *d_dc_mode_bits;        /* [nblocks]: intraUVmodeFacBits[CFL_ALLOWED][intra_luma_mode][UV_CFL_PRED] / [UV_DC_PRED] */
    svt_hip_cfl_decision *d_decision;                       /* [nblocks] */
    int32_t *d_alpha_q3_cb, *d_alpha_q3_cr;                 /* optional [nblocks]: what svt_hip_frame_cfl_group takes */
} svt_hip_cfl_decide_group;
int svt_hip_cfl_decide_frame(const svt_hip_cfl_decide_group *groups, int ngroups, void *stream);

/* Search then decide on `stream`, whose order carries the dependency (host composition, as svt_hip_tx_search_frame).  search.d_dist /
 * d_bits / d_eob may be NULL: the table then lives in d_scratch.  Carved first, per non-empty group in group order: dist (nblocks *
 * 66 * 16 bytes), bits (* 8) and eob (* 2), each only when not supplied and rounded up to 16 bytes; then the search call's own
 * scratch.  svt_hip_cfl_pick_scratch_bytes returns the sum (HOST; 0: bad parameters or nothing to do).  Both stages' arguments are
 * validated before the first launch. */
typedef struct svt_hip_cfl_pick_group {
    svt_hip_cfl_search_group search;
    uint32_t lambda;
    const int32_t *d_alpha_rate, *d_cfl_mode_bits, *d_dc_mode_bits;
    svt_hip_cfl_decision *d_decision;
    int32_t *d_alpha_q3_cb, *d_alpha_q3_cr;
} svt_hip_cfl_pick_group;
size_t svt_hip_cfl_pick_scratch_bytes(const svt_hip_cfl_pick_group *groups, int ngroups);
int svt_hip_cfl_pick_frame(const svt_hip_cfl_pick_group *groups, int ngroups, int flavour,
                           const svt_hip_qrows *q_cb, const svt_hip_qrows *q_cr,
                           void *d_scratch, size_t scratch_bytes, void *stream);

/* Open-loop intra search: open_loop_intra_search_sb, EbMotionEstimation.c:8694-8850,
 * for all blocks of ONE size of a picture (or of many pictures' worth of blocks) in one call.
 * d_pic points at picture sample (0, 0) (buffer_y + origin_y * stride_y + origin_x), width x height are
 * the picture's; d_xy[i] = x | y << 16 is a block's origin (the reference's cu_origin_x / _y).  Per block:
 * neighbour arrays gathered from the SOURCE picture exactly as update_neighbor_samples_array_open_loop does
 * (EbIntraPrediction.c:4707-4773: 127 / 129 / 128 fill at picture borders), then for each of the ncand
 * candidates (modes[c]: AV1 PredictionMode 0..12, angle_deltas[c]: -2..2 for the directional modes; HOST
 * arrays - the list the reference's loop :8747-8846 enumerates for this block size) the prediction of
 * intra_prediction_open_loop (:4778-4808: dr_predictor without edge filter / upsampling, DC by
 * availability, the other predictors as is) and its SAD against the source block.
 * d_distortion: uint32 [nblocks][ncand] (ois_candidate_t.distortion); d_best_index: int8 [nblocks]
 * (ois_sb_results_t.best_distortion_index: first strict minimum below 64*64*255, else 0).
 * d_work: scratch of svt_hip_ois_work_bytes(bsize, ncand, nblocks) bytes (neighbour arrays + one dense
 * prediction batch per candidate: split very large batches).  bsize 8 / 16 / 32 / 64, 8-bit. */
size_t svt_hip_ois_work_bytes(uint32_t bsize, int ncand, size_t nblocks);
int svt_hip_ois_search_batch(const uint8_t *d_pic, uint32_t stride, uint32_t width, uint32_t height,
                             const uint32_t *d_xy, uint32_t bsize, const uint8_t *modes,
                             const int8_t *angle_deltas, int ncand, uint32_t *d_distortion,
                             int8_t *d_best_index, void *d_work, size_t work_bytes, size_t nblocks,
                             void *stream);

/* The open-loop intra search of a whole PICTURE in one call: one group per block size (what svt_hip_ois_search_batch takes),
 * run concurrently on the library's internal streams (forked from / joined into `stream`; the call only enqueues).  The four
 * sizes of open_loop_intra_search_sb (EbMotionEstimation.c:8694) are independent, so the picture costs its slowest size, not
 * their sum.  Every group (ngroups <= 64; a group with nblocks == 0 is skipped) is checked before the first launch: when the
 * call returns an argument error it has enqueued nothing, under either setting of "ois_no_nd_multi". */
typedef struct svt_hip_ois_group {
    const uint32_t *d_xy;                 /* block origins x | y << 16 */
    uint32_t bsize;                       /* 8, 16, 32, 64 */
    const uint8_t *modes;                 /* HOST candidate list (svt_hip_ois_candidates) */
    const int8_t *angle_deltas;
    int32_t ncand;
    uint32_t *d_distortion;               /* [nblocks][ncand] */
    int8_t *d_best_index;                 /* [nblocks] */
    void *d_work;  size_t work_bytes;     /* svt_hip_ois_work_bytes(bsize, ncand, nblocks) */
    size_t nblocks;
} svt_hip_ois_group;
int svt_hip_ois_search_frame(const uint8_t *d_pic, uint32_t stride, uint32_t width, uint32_t height,
                             const svt_hip_ois_group *groups, int ngroups, void *stream);

/* K11 chroma-from-luma helpers of the encode pass (Av1EncodeLoop, EbCodingLoop.c:736-846) and the
 * entropy stage's level map - the remaining pieces of SURVEY.md 8(f) n3.
 *
 * svt_hip_cfl_luma_subsampling_420_batch replaces cfl_luma_subsampling_420_{lbd,hbd}_c
 * (EbIntraPrediction.c:1303-1332; aom_dsp_rtcd.h has no dispatch slot for them): per block, a
 * width x height LUMA area (8-bit, or 16-bit when is_16bit) becomes width/2 x height/2 Q3 sums
 * `(a + b + c + d) << 1`.  Blocks are addressed by d_xy[i] = x | y << 16 (sample units) in the
 * plane d_luma, or, when d_xy is NULL, lie luma_block_pitch samples apart.  Output rows are
 * q3_line int16 apart (CFL_BUF_LINE = 32 in the reference), blocks q3_block_pitch int16 apart
 * (CFL_BUF_SQUARE = 1024 there).  subtract_average != 0 also applies subtract_average with the
 * encode pass's arguments (round_offset = w*h/2, num_pel_log2 = log2(w*h) of the chroma block) in
 * the same kernel.  Chroma sizes 4..32 in both dimensions.  Only the width/2 x height/2 entries of a block's Q3 buffer are
 * written; the rest of each row and the rows below keep what they held (the reference's pred_buf_q3 is not cleared either).
 *
 * Block counts: svt_hip_cfl_luma_subsampling_420_batch and svt_hip_subtract_average_batch take at most 2^25 - 1 blocks per call (the
 * kernel counts lanes in 32 bits), svt_hip_cfl_predict_batch and svt_hip_txb_init_levels_batch at most 2^31 - 1; a larger nblocks is
 * SVT_HIP_ERR_INVALID ("too many blocks for one launch"), checked on the size_t before anything is derived from it. */
int svt_hip_cfl_luma_subsampling_420_batch(const void *d_luma, uint32_t luma_stride,
                                           size_t luma_block_pitch, const uint32_t *d_xy, int is_16bit,
                                           int16_t *d_q3, uint32_t q3_line, size_t q3_block_pitch,
                                           uint32_t width, uint32_t height, int subtract_average,
                                           size_t nblocks, void *stream);
/* subtract_average (aom_dsp_rtcd.h:138, C: EbIntraPrediction.c:1333-1359), in place on Q3 blocks. */
int svt_hip_subtract_average_batch(int16_t *d_q3, uint32_t q3_line, size_t q3_block_pitch,
                                   uint32_t width, uint32_t height, int32_t round_offset,
                                   int32_t num_pel_log2, size_t nblocks, void *stream);
/* cfl_predict_lbd / cfl_predict_hbd (aom_dsp_rtcd.h:142-146, C: EbIntraPrediction.c:1361-1402):
 * dst = clip(pred + ROUND_POWER_OF_TWO_SIGNED(alpha_q3 * ac_q3, 6), bit_depth), one alpha per block
 * (d_alpha_q3[nblocks]).  pred and dst are planes addressed by the same d_xy (the encode pass
 * predicts in place: d_dst == d_pred is allowed), or dense blocks (stride * height apart) when
 * d_xy is NULL. */
int svt_hip_cfl_predict_batch(const int16_t *d_ac_q3, uint32_t q3_line, size_t q3_block_pitch,
                              const void *d_pred, uint32_t pred_stride, void *d_dst,
                              uint32_t dst_stride, const uint32_t *d_xy, const int32_t *d_alpha_q3,
                              int bit_depth, uint32_t width, uint32_t height, int is_16bit,
                              size_t nblocks, void *stream);
/* av1_txb_init_levels (aom_dsp_rtcd.h:2374, C: EbRateDistortionCost.c:125-150).  d_levels_buf holds
 * one WHOLE padded buffer per block (the reference's levels_buf; its `levels` pointer is
 * buffer + TX_PAD_TOP * (width + TX_PAD_HOR)), levels_block_pitch >= (width + 4) * (height + 6) + 16
 * bytes, a multiple of 4.  Every byte of the (width + 4) * (height + 6) + 16 is written. */
int svt_hip_txb_init_levels_batch(const int32_t *d_coeff, size_t coeff_block_pitch,
                                  uint8_t *d_levels_buf, size_t levels_block_pitch, uint32_t width,
                                  uint32_t height, size_t nblocks, void *stream);

/* K9/K10 intra prediction.  Replaces the aom_{dc,...,paeth}_predictor_WxH /
 * aom_highbd_* slots (aom_dsp_rtcd.h:442-1262, 1626-2330; C: EbIntraPrediction.c:
 * 1838-2260) and av1_dr_prediction_z{1,2,3} / av1_highbd_dr_prediction_z*
 * (aom_dsp_rtcd.h:2340; C: EbIntraPrediction.c:370-477, 3394-3506).
 * Neighbours: d_above / d_left hold one row of `nb_pitch` samples per block; the
 * reference's above_row[p] / left_col[p] (p >= -2) is element SVT_HIP_NB_ORIGIN + p.
 * Samples are uint8 (is_16bit = 0, bd = 8) or uint16.  mode: SVT_INTRA_*; for the
 * directional modes dx, dy, upsample_above, upsample_left are the reference's
 * arguments (dr_intra_derivative based).  Destination addressing as in
 * svt_hip_inv_txfm2d_add_batch.  nblocks: at most 2^31 - 1, and at most 2^31 - 1 workgroups of 256
 * lanes (a block takes 4 .. 512 lanes); more is SVT_HIP_ERR_INVALID. */
enum { SVT_INTRA_DC, SVT_INTRA_V, SVT_INTRA_H, SVT_INTRA_SMOOTH, SVT_INTRA_SMOOTH_V, SVT_INTRA_SMOOTH_H,
       SVT_INTRA_PAETH, SVT_INTRA_DC_TOP, SVT_INTRA_DC_LEFT, SVT_INTRA_DC_128, SVT_INTRA_Z1, SVT_INTRA_Z2,
       SVT_INTRA_Z3, SVT_INTRA_MODES };
#define SVT_HIP_NB_ORIGIN 16
int svt_hip_intra_pred_batch(void *d_dst, int32_t dst_stride, size_t dst_block_pitch,
                             const uint32_t *d_dst_offsets, const void *d_above, const void *d_left,
                             int32_t nb_pitch, int mode, int bw, int bh, int upsample_above,
                             int upsample_left, int dx, int dy, int is_16bit, int bd,
                             size_t nblocks, void *stream);
/* build_intra_predictors / build_intra_predictors_high (EbIntraPrediction.c:3667-3855, 3857-4076): the
 * neighbour-availability glue of av1_predict_intra_block, fused into ONE launch for a batch of prediction blocks of one
 * transform size with per-block mode and availability.  Per block: which edges the mode needs, the constant fill when the
 * needed edge is missing, edge extension (last available sample replicated; base +- 1 defaults), the corner sample, for
 * directional modes the corner / edge smoothing filters and 2x up-sampling chosen from size, angle and filt_type, DC by
 * availability, then the prediction itself.
 *   d_top_neigh / d_left_neigh: the caller's topNeighArray / leftNeighArray (EbCodingLoop.c:2862-2893), one per block,
 *     `neigh_pitch` samples apart: element 0 = the above-left corner sample, element 1 + i = above[i] / left[i];
 *     neigh_pitch >= 1 + 2 * max(width, height).  Samples uint8 (is_16bit = 0, bd 8) or uint16.
 *   d_blocks: one descriptor per block (device memory); n_top_px / n_left_px above the block's width / height are clamped.
 *   Destination addressing as in svt_hip_inv_txfm2d_add_batch.
 *   nblocks: at most 2^31 - 1 in this call, in the ordered form and in svt_hip_intra_order_blocks_batch; more is SVT_HIP_ERR_INVALID. */
typedef struct svt_hip_intra_blk {
    uint8_t mode;                 /* AV1 PredictionMode: DC 0, V 1, H 2, D45 3, D135 4, D113 5, D157 6, D203 7, D67 8,
                                     SMOOTH 9, SMOOTH_V 10, SMOOTH_H 11, PAETH 12 */
    int8_t angle_delta;           /* -3 .. 3 (directional modes; angle = mode_to_angle_map[mode] + 3 * delta) */
    uint8_t filt_type;            /* get_filt_type (:146): 1 when the above or left block is a smooth-mode block */
    uint8_t disable_edge_filter;
    uint8_t n_top_px, n_topright_px, n_left_px, n_bottomleft_px;   /* available samples (svt_hip_intra_neighbor_px) */
} svt_hip_intra_blk;
int svt_hip_build_intra_predictors_batch(void *d_dst, int32_t dst_stride, size_t dst_block_pitch,
                                         const uint32_t *d_dst_offsets, const void *d_top_neigh,
                                         const void *d_left_neigh, int32_t neigh_pitch,
                                         const svt_hip_intra_blk *d_blocks, int tx_size, int is_16bit, int bd,
                                         size_t nblocks, void *stream);
/* The same walked through an ORDER of the batch (d_order[i] = block index): svt_hip_intra_order_blocks_batch groups the block
 * indices by the predictor kind each descriptor resolves to (DC variants, V, H, SMOOTH*, PAETH, the three directional zones),
 * on the device, inside tiles of SVT_HIP_INTRA_ORDER_TILE consecutive blocks (entries [t * TILE, (t + 1) * TILE) of d_order are a
 * permutation of those block indices, kinds contiguous), so that the lanes of a wave run one kind's code (mixed kinds in a wave
 * are correct, just slower: a wave runs every kind it holds).  d_order: uint32[nblocks]; d_work: unused (may be NULL; the first
 * version's counters).  Results do not depend on the order. */
#define SVT_HIP_INTRA_ORDER_TILE 4096
int svt_hip_intra_order_blocks_batch(const svt_hip_intra_blk *d_blocks, int tx_size, size_t nblocks, uint32_t *d_order,
                                     uint32_t *d_work, void *stream);
int svt_hip_build_intra_predictors_ordered_batch(void *d_dst, int32_t dst_stride, size_t dst_block_pitch,
                                                 const uint32_t *d_dst_offsets, const void *d_top_neigh,
                                                 const void *d_left_neigh, int32_t neigh_pitch,
                                                 const svt_hip_intra_blk *d_blocks, const uint32_t *d_order, int tx_size,
                                                 int is_16bit, int bd, size_t nblocks, void *stream);

/* The intra candidates of the mode-decision fast loop, fused: perform_fast_loop (EbProductCodingLoop.c:1152-1300) for one plane
 * and many (transform size, candidate list) groups in one call.  Per block of a group and per candidate of its list, in the list's
 * order: the prediction of build_intra_predictors (as svt_hip_build_intra_predictors_batch: the block's descriptor gives
 * availability, filt_type and disable_edge_filter, the candidate gives mode and angle delta; the descriptor's own mode / angle_delta
 * are ignored) and its distortion against the source block, 8-bit samples:
 *   SVT_HIP_FAST_SAD   the plain W x H SAD every NxMSadKernelSubSampled_funcPtrArray entry computes (fast_loop_nx_m_sad_kernel and
 *                      the AVX2 kernels agree), either flavour, all 19 sizes;
 *   SVT_HIP_FAST_SSD   SVT_HIP_FLAVOUR_C: the exact sum of (src - pred)^2 over the W x H block, spatial_full_distortion_kernel with
 *                      (bwidth, bheight).  DELIBERATE DIVERGENCE: the reference's call site (:3059-3077) passes (bheight, bwidth)
 *                      into (area_width, area_height); this is the corrected call, all 19 sizes.
 *                      SVT_HIP_FLAVOUR_AVX2: the arithmetic of the table entry the encoder runs (the SSSE3 kernels
 *                      spatial_full_distortion_kernel{4x4,8x8,16_mx_n}, EbPictureOperators_Intrinsic_SSE4_1.c:495-620): per
 *                      sample t = (a - b) & 255, d = t <= 128 ? t : 256 - t, d * d, summed in 32 bits.  Square sizes only: on a
 *                      non-square block the reference's kernels read samples outside the block (the 4x4 / 8x8 kernels cover a
 *                      fixed square, the swapped area covers other rows), stale prediction rows included - a result that cannot be
 *                      reproduced, so the call returns SVT_HIP_ERR_INVALID (the second divergence).
 * Chroma (CHROMA_MODE_0, UV modes other than UV_CFL_PRED): one group per plane with the chroma size; the caller adds the Cb and Cr
 * distortions.  d_dist[b * ncand + c] receives the distortion; d_pred (optional, 16-byte aligned; NULL: not written) the predictions,
 * dense [nblocks][ncand][H][W].  Source: d_src_xy[b] = x | y << 16 on a plane of src_stride samples, or NULL: dense W * H samples per
 * block.  Neighbours as in svt_hip_build_intra_predictors_batch (element 0 = the corner, neigh_pitch >= 1 + 2 * max(W, H)).
 * The candidate list is a HOST array in the group (svt_hip_md_intra_candidates gives inject_intra_candidates' list).  Every argument,
 * empty groups' tx_size and lists included, is validated before the first launch; invalid input (ncand outside 1 .. 64, a mode above
 * 12, a delta outside -3 .. 3 or on a non-directional mode, NULL required pointers, d_dist not 8-byte aligned, d_pred not 16-byte
 * aligned, the AVX2-flavour SSD on a non-square size) returns SVT_HIP_ERR_INVALID and launches nothing.  The call only enqueues work
 * (one launch per non-empty group, the group in the kernel arguments) and can be captured into a HIP graph. */
enum { SVT_HIP_FAST_SAD = 0, SVT_HIP_FAST_SSD = 1 };
#define SVT_HIP_FAST_LOOP_MAX_CANDIDATES 64
typedef struct svt_hip_fast_loop_group {
    const uint8_t *d_src; uint32_t src_stride; const uint32_t *d_src_xy;   /* plane + x | y << 16 origins; NULL xy: dense W * H */
    const uint8_t *d_top_neigh, *d_left_neigh; int32_t neigh_pitch;      /* as svt_hip_build_intra_predictors_batch */
    const svt_hip_intra_blk *d_blocks;   /* per block: filt_type, disable_edge_filter, n_*_px; mode / angle_delta ignored */
    uint32_t nblocks;
    int32_t tx_size;                     /* 0 .. 18 */
    int32_t ncand; uint8_t modes[64]; int8_t angle_deltas[64];          /* HOST-side list, 1 .. 64 entries */
    uint64_t *d_dist;                    /* [nblocks][ncand] */
    uint8_t *d_pred;                     /* optional (NULL: not written), [nblocks][ncand][H][W] dense */
} svt_hip_fast_loop_group;
int svt_hip_intra_fast_loop_frame(const svt_hip_fast_loop_group *groups, int ngroups, int metric, int flavour, void *stream);

/* The end of the fast loop for an all-intra candidate list, on the device: the fast cost of every (block, candidate), the buffer walk
 * that keeps the N best, the two index arrays, and the gather of the survivors' predictions into the layout the full loop reads.
 * svt_hip_intra_fast_loop_frame writes its inputs, svt_hip_full_loop_frame / svt_hip_tx_search_frame read its outputs as they lie.
 * What is reproduced.  Each piece is pinned to the reference's own compiled function (oracle/ref_md.c): cost to
 * av1_intra_fast_cost and model_rd_from_sse called directly, order to sort_fast_loop_candidates called directly, and cost, walk and order
 * together to inject_intra_candidates -> perform_fast_loop -> sort_fast_loop_candidates run whole on blocks of a picture
 * (tests/golden/fast_search_ref.npz).  Inter candidates, the first (src-to-src) loop and the intrabc branch remain the caller's.
 *   cost     av1_intra_fast_cost (EbRateDistortionCost.c:531-729), the non-intrabc branch (:598-728): the mode / skip-mode / is-inter /
 *            angle-delta / uv-mode bits out of d_rates (MdRateEstimationContext_s, EbMdRateEstimation.h:59, 93-103, in the reference's
 *            declaration shapes), intra_mode_context / size_group_lookup / num_pels_log2_lookup (EbDefinitions.h:1213, 1311, 1315),
 *            RDCOST (EbRateDistortionCost.h:71-75) = ((rate * lambda + 256) >> 9) + dist * 128 in uint64.  SVT_HIP_FAST_SSD takes the
 *            branch at :687-716: model_rd_from_sse -> av1_model_rd_from_var_lapndz -> model_rd_norm (EbInterPrediction.c:3311-3438).
 *   walk     perform_fast_loop (EbProductCodingLoop.c:1152-1365) as md_encode_block calls it (:3103-3131): n = min(ncand, nfl) full-loop
 *            slots, n + 1 buffers when ncand > n (one scratch), the candidates taken from the LAST list entry down to entry 0, each
 *            into the buffer the re-scan (:1331-1356, strict >, stops at the first empty buffer) found, the last one emptied (:1361).
 *   order    sort_fast_loop_candidates (EbModeDecision.c:436-489): best_candidate_index_array = the buffers in buffer order, the empty
 *            one last; ref_fast_cost; sorted_candidate_index_array.
 * Quirks kept, because AV1PerformFullLoop (:1919-1923) and get_skip_tx_search_flag (:1866-1878) consume exactly these values:
 *   - the rates are summed in uint32; fast_luma_rate / fast_chroma_rate (d_rate) are stored BEFORE the SSD model's rates are added;
 *     the SSD chroma call writes the model's rate OVER chromaRate (:704-710), so the chroma mode bits drop out of the SSD cost;
 *   - ref_fast_cost starts at MAX_MODE_COST (13616969489728 * 8) and is the minimum over buffers 0 .. n-1 BY BUFFER INDEX (:472-476):
 *     the scratch buffer may be among them, a real candidate in buffer n is then left out;
 *   - the sorted array is bubble-swapped on the costs of BUFFERS i and j, not of the entries being swapped (:480-488);
 *   - the candidate's use_angle_delta is the block-size flag AND "luma mode is directional" (:2444, :2490): the uv angle-delta bits
 *     are counted only under a directional luma mode.  The group's use_angle_delta is the block-size flag (bsize >= BLOCK_8X8).
 *   - UV_CFL_PRED (13) is costed as UV_DC_PRED (:606); cfl_allowed = W <= 32 && H <= 32 (:601).
 * has_chroma gates the uv rate bits only (blk_geom->has_uv && is_chroma_reference(mi_row, mi_col, bsize, 1, 1), :666-667); the chroma
 * distortions d_dist_cb + d_dist_cr are added for every block when given (the reference adds them when has_uv under CHROMA_MODE_0:
 * give zeros for blocks without chroma; NULL = 0, any other chroma level).  Context bytes are device data and are clamped on the
 * device (modes to 12, skip_mode_ctx to 2, is_inter_ctx to 3): an out-of-range byte gives an unspecified cost for its block, nothing
 * else.  A cost equal to MAX_CU_COST (UINT64_MAX >> 1) or above cannot be told from an empty buffer in the reference: the block's
 * results are then unspecified (the stores stay inside the block's rows).
 * Outputs, n = min(nfl, ncand), [nblocks][n] unless stated: d_cand = the list index of the candidate in full-loop slot k
 * (best_candidate_index_array order); d_sorted = sorted_candidate_index_array[k] as the SLOT that holds that buffer (the reference's
 * value is a buffer index; slots are what this interface exposes); d_cost = the candidate's fast cost; d_rate [..][2] = fast_luma_rate,
 * fast_chroma_rate; d_ref_fast_cost [nblocks]; optional d_all_cost [nblocks][ncand] = every candidate's cost; optional d_pred_out
 * [nblocks][n][H][W] (needs d_pred, the fast loop's [nblocks][ncand][H][W]) = the d_pred of a svt_hip_full_loop_group of nblocks * n
 * blocks; optional d_src_xy_out [nblocks][n] (needs d_src_xy) = the block's origin repeated, that group's d_src_xy.
 * Validation, every group before the first launch (SVT_HIP_ERR_INVALID, nothing launched): metric; tx_size 0 .. 18; bsize / bsize_uv
 * 0 .. 21; ncand 1 .. 64; nfl 1 .. 40; a mode above 12, a uv mode above 13, a delta outside -3 .. 3; ac_dequant_q3 < 0; and for non-empty
 * groups NULL d_dist / d_blk / d_rates / d_cand / d_sorted / d_cost / d_rate / d_ref_fast_cost, d_pred_out without d_pred,
 * d_src_xy_out without d_src_xy, d_pred_out == d_pred, misalignment (d_pred / d_pred_out 16 bytes; the 8-byte arrays and d_blk 8;
 * d_rates / d_rate / d_src_xy* 4), nblocks * ncand above 2^31 - 1.  One launch per non-empty group, the group in the kernel arguments; the call
 * only enqueues (no allocation, no synchronisation) and can be captured into a HIP graph.
 * Left to the caller here: inter candidates (svt_hip_inter_fast_pick_frame below costs them and walks the combined list), the intrabc branch
 * (:556-597; intrabc_bits is intrabcFacBits[0] when the picture allows intrabc, else 0).  product_full_mode_decision over the survivors is
 * svt_hip_md_decide_frame below. */
#define SVT_HIP_MAX_NFL 40
typedef struct svt_hip_fast_pick_blk {
    uint8_t top_mode, left_mode;         /* intra_luma_top_mode / intra_luma_left_mode, 0 .. 12 */
    uint8_t skip_mode_ctx;               /* cu_ptr->skip_flag_context, 0 .. 2 */
    uint8_t is_inter_ctx;                /* cu_ptr->is_inter_ctx, 0 .. 3 */
    uint8_t has_chroma;                  /* blk_geom->has_uv && is_chroma_reference(...) */
    uint8_t pad[3];
} svt_hip_fast_pick_blk;
typedef struct svt_hip_fast_rates {      /* the int32 tables of MdRateEstimationContext_s the intra fast cost reads */
    int32_t yModeFacBits[5][5][14];
    int32_t mbModeFacBits[4][14];
    int32_t intraUVmodeFacBits[2][13][15];
    int32_t angleDeltaFacBits[8][8];
    int32_t skipModeFacBits[3][3];
    int32_t intraInterFacBits[4][2];
} svt_hip_fast_rates;
typedef struct svt_hip_fast_pick_group {
    int32_t tx_size;                     /* 0 .. 18: the block, as in svt_hip_fast_loop_group */
    int32_t bsize, bsize_uv;             /* AV1 block_size order, 0 .. 21 */
    uint32_t nblocks;
    int32_t ncand; uint8_t modes[64]; int8_t angle_deltas[64];          /* HOST-side list, as svt_hip_fast_loop_group */
    uint8_t uv_modes[64]; int8_t uv_angle_deltas[64];                   /* 0 .. 13 (UV_CFL_PRED = 13), -3 .. 3 */
    int32_t use_angle_delta;             /* bsize >= BLOCK_8X8 */
    int32_t nfl;                         /* full_recon_search_count, 1 .. SVT_HIP_MAX_NFL */
    int32_t slice_is_intra;
    uint32_t lambda;                     /* fast_lambda (SAD) / full_lambda (SSD) */
    int16_t ac_dequant_q3;               /* y_dequant_Q3[qindex][1]; SSD only */
    uint32_t intrabc_bits;
    const uint64_t *d_dist, *d_dist_cb, *d_dist_cr;                     /* [nblocks][ncand]; cb / cr optional */
    const svt_hip_fast_pick_blk *d_blk;  /* [nblocks] */
    const svt_hip_fast_rates *d_rates;
    const uint8_t *d_pred;               /* optional [nblocks][ncand][H][W] */
    const uint32_t *d_src_xy;            /* optional [nblocks] */
    uint8_t *d_cand, *d_sorted;          /* [nblocks][n] */
    uint64_t *d_cost;                    /* [nblocks][n] */
    uint32_t *d_rate;                    /* [nblocks][n][2] */
    uint64_t *d_ref_fast_cost;           /* [nblocks] */
    uint64_t *d_all_cost;                /* optional [nblocks][ncand] */
    uint8_t *d_pred_out;                 /* optional [nblocks][n][H][W] */
    uint32_t *d_src_xy_out;              /* optional [nblocks][n] */
} svt_hip_fast_pick_group;
int svt_hip_fast_pick_frame(const svt_hip_fast_pick_group *groups, int ngroups, int metric, void *stream);

/* The whole intra fast search in one call: svt_hip_intra_fast_loop_frame (luma, then the Cb and Cr groups when use_chroma) ->
 * svt_hip_fast_pick_frame on `stream`, whose order carries the dependency.  Host composition: it has no kernel of its own.  The
 * pick's tx_size, nblocks, ncand, modes, angle_deltas, d_dist*, d_pred and d_src_xy are taken from the fast-loop groups (what `pick`
 * holds there is ignored; a luma group with a dense source, d_src_xy NULL, leaves the pick's own d_src_xy in place); cb / cr carry the chroma size and the uv candidates as intra modes, with luma's nblocks and ncand.  Arrays
 * the caller does not keep live in d_scratch (16-byte aligned), carved per non-empty group in group order, each piece rounded up to
 * 16 bytes: luma.d_dist when NULL (nblocks * ncand * 8), cb.d_dist and cr.d_dist likewise when use_chroma, luma.d_pred when NULL and
 * pick.d_pred_out asks for it (nblocks * ncand * W * H).  svt_hip_intra_fast_search_scratch_bytes returns their sum, a HOST
 * computation that needs no device (0: bad parameters, or nothing needed).  Every stage's arguments are validated before the first
 * launch; a scratch that is NULL, misaligned or too small returns SVT_HIP_ERR_INVALID.  Every candidate's prediction is still stored;
 * regenerating only the winners' is out of scope. */
typedef struct svt_hip_intra_fast_search_group {
    svt_hip_fast_loop_group luma;
    int32_t use_chroma;                  /* non-zero: cb and cr are fast-loop groups of the chroma planes */
    svt_hip_fast_loop_group cb, cr;
    svt_hip_fast_pick_group pick;
} svt_hip_intra_fast_search_group;
size_t svt_hip_intra_fast_search_scratch_bytes(const svt_hip_intra_fast_search_group *groups, int ngroups);
int svt_hip_intra_fast_search_frame(const svt_hip_intra_fast_search_group *groups, int ngroups, int metric, int flavour,
                                    void *d_scratch, size_t scratch_bytes, void *stream);

/* CDEF for whole 4:2:0 pictures: the strength search and the apply.  One descriptor serves both calls: a picture (or a stack of
 * npics pictures of one geometry, *_pitch samples / skip_pitch bytes apart) of width x height luma samples, both multiples of 8 as the
 * reference's padded pictures are; planes of uint8 (bit_depth 8) or uint16 (bit_depth 10; coeff_shift = bit_depth - 8) samples with
 * strides in samples; a skip map with one byte per 8x8 luma block (non-zero: every mode-info unit of the block is skipped, what
 * is_8x8_block_skip, EbCdef.c:380, returns), height / 8 rows of skip_stride bytes; base_qindex (both dampings are
 * 3 + (base_qindex >> 6), EbCdefProcess.c:128-129; cdef_filter_fb adds coeff_shift and takes one off for chroma, EbCdef.c:286-287).
 * Filter blocks are 64x64 luma samples, fb = fbr * nhfb + fbc, nhfb = (width + 63) / 64, nvfb = (height + 63) / 64, nfb = nhfb * nvfb.
 *
 * svt_hip_cdef_search_frame: cdef_seg_search (EbCdefProcess.c:89-258; 16-bit :260) for every filter block - the reference's mse_seg
 * table.  Per filter block, plane and gi in [start_gi, end_gi) (the reference: 0 .. 8 at cdef_filter_mode 1, 0 .. 64 otherwise, or
 * a window round the reference frame's strength, :217-220): the list of non-skipped 8x8 blocks (sb_compute_cdef_list, EbCdef.c:390;
 * a filter block with an empty list is left out, sb_all_skip :360); the input tile from the unfiltered d_rec with CDEF_VERY_LARGE
 * outside the picture (:203-216); direction and variance per 8x8 luma block (cdef_find_dir, EbCdef.c:129, reused by chroma);
 * cdef_filter_fb (EbCdef.c:273) with pri = gi / 4, sec = gi % 4 (+ 1 if 3), luma primary strength through adjust_strength (:267),
 * direction 0 when the primary strength is 0, cdef_filter_block (:204) to the letter; compute_cdef_dist (:1360) against d_src: luma
 * dist_8x8_16bit (:1305, binary64, reproduced bit for bit) per 8x8 block, chroma mse_4x4_16bit (:1346), each plane's sum shifted
 * right by 2 * coeff_shift.  d_mse[((pic * 2 + 0) * nfb + fb) * 64 + gi] = luma, [.. + 1 ..] = Cb + Cr; d_count[pic * nfb + fb] =
 * the length of the list.  Entries of left-out filter blocks and of gi outside the window are written as 0, so every entry of both
 * arrays is defined after the call.  Filtered samples are not stored.  The serving dispatch slots (aom_dsp_rtcd.h:78-88, 270-276):
 * cdef_find_dir, cdef_filter_block, copy_rect8_8bit_to_16bit, dist_8x8_16bit, mse_4x4_16bit.
 * NOT here: the choice of the picture's strength set from mse_seg (finish_cdef_search, EbCdef.c:1410, joint_strength_search_dual
 * :1259) - a few thousand sequential table look-ups that stay with the caller on the host.
 *
 * svt_hip_cdef_apply_frame: av1_cdef_frame (EbCdef.c:471; 16-bit :801).  d_luma_strength / d_chroma_strength [pic * nfb + fb]: the
 * filter block's strengths 0 .. 63 (cdef_strengths[] / cdef_uv_strengths[] of the block's mbmi.cdef_strength), -1 in either = leave
 * the filter block alone.  A filter block left alone, with both strengths 0 or with an empty list is copied (:600-604); otherwise every
 * listed 8x8 block of all three planes goes through cdef_filter_block (pri = s / 4, sec = s % 4 (+ 1 if 3), luma through
 * adjust_strength, chroma with luma's direction) and every other sample is copied.  The reference filters in place and keeps the
 * unfiltered neighbour rows / columns in line buffers (:620-760); here d_rec is read and d_dst written, two distinct buffers, which
 * computes the same picture.  Every sample of the width x height (chroma: half) area of d_dst is written, nothing outside it.
 *
 * Every argument is validated before the launch (SVT_HIP_ERR_INVALID: a side that is not a multiple of 8, a window outside 0 .. 64 or
 * empty, a bit depth other than 8 / 10, base_qindex outside 0 .. 255, NULL planes / map / outputs, a stride below the width, d_mse not
 * 8-byte aligned, d_dst == d_rec); each call is one kernel launch that only enqueues and can be captured into a HIP graph. */
typedef struct svt_hip_cdef_pic {
    const void *d_rec[3];  uint32_t rec_stride[3];   /* filter input: the deblocked reconstruction (Y, Cb, Cr) */
    const void *d_src[3];  uint32_t src_stride[3];   /* the source picture (search only) */
    void *d_dst[3];        uint32_t dst_stride[3];   /* the filtered picture (apply only) */
    const uint8_t *d_skip; uint32_t skip_stride;
    uint32_t width, height;
    int32_t bit_depth, base_qindex;
    uint32_t npics;                                 /* >= 1 */
    uint64_t rec_pitch[3], src_pitch[3], dst_pitch[3], skip_pitch;      /* between the pictures of a stack (ignored for npics 1) */
} svt_hip_cdef_pic;
int svt_hip_cdef_search_frame(const svt_hip_cdef_pic *pic, int start_gi, int end_gi, uint64_t *d_mse, int32_t *d_count, void *stream);
int svt_hip_cdef_apply_frame(const svt_hip_cdef_pic *pic, const int8_t *d_luma_strength, const int8_t *d_chroma_strength, void *stream);

/* HOST helper, no device work: the first half of av1_predict_intra_block / av1_predict_intra_block_16bit
 * (EbIntraPrediction.c:4078-4333, 4336-4566) - up / left availability from the block's mode-info position,
 * has_top_right (:1567) and has_bottom_left (:1755), and the four sample counts handed to build_intra_predictors.
 * The reference reads "is that neighbour block already coded" from bit tables (has_tr_* / has_bl_*); here it is the
 * comparison of two coding-order keys (Morton order of the enclosing squares; PARTITION_VERT_A / VERT_B visit the last
 * split column first).  is_16bit selects the tile handling of the 16-bit function (the 8-bit one treats the picture as
 * one tile, :4124-4137).  Fills blk->n_*_px; returns SVT_HIP_OK or SVT_HIP_ERR_INVALID. */
typedef struct svt_hip_intra_pos {
    int32_t is_16bit;
    int32_t sb_size_mi;                       /* mi_size_high[sb_size]: 16 (64x64 superblocks) or 32 */
    int32_t mi_rows, mi_cols;                 /* Av1Common */
    int32_t tile_mi_row_start, tile_mi_row_end, tile_mi_col_start, tile_mi_col_end;   /* TileInfo */
    int32_t partition;                        /* AV1 PartitionType (from_shape_to_part[blk_geom->shape]) */
    int32_t bsize;                            /* AV1 block_size, BLOCK_4X4 = 0 .. BLOCK_64X16 = 21 */
    int32_t tx_size, plane;
    int32_t bl_org_x_pict, bl_org_y_pict;     /* luma sample position of the block */
    int32_t col_off, row_off;                 /* transform block offset inside the block, 4-sample units of the plane */
    int32_t wpx, hpx;                         /* block size in samples of the plane */
} svt_hip_intra_pos;
int svt_hip_intra_neighbor_px(const svt_hip_intra_pos *pos, svt_hip_intra_blk *blk);
int svt_hip_intra_has_top_right(int sb_size_mi, int bsize, int mi_row, int mi_col, int top_available, int right_available,
                                int partition, int tx_size, int row_off, int col_off, int ss_x, int ss_y);
int svt_hip_intra_has_bottom_left(int sb_size_mi, int bsize, int mi_row, int mi_col, int bottom_available,
                                  int left_available, int partition, int tx_size, int row_off, int col_off, int ss_x,
                                  int ss_y);

/* av1_filter_intra_edge{,_high} / av1_upsample_intra_edge{,_high} (aom_dsp_rtcd.h:152,
 * 431; C: EbIntraPrediction.c:3539-3660) on nblocks edges laid out like d_above, an edge per
 * workgroup: at most 2^31 - 1 of them, more is SVT_HIP_ERR_INVALID. */
int svt_hip_filter_intra_edge_batch(void *d_edges, int32_t nb_pitch, int sz, int strength,
                                    int is_16bit, size_t nblocks, void *stream);
int svt_hip_upsample_intra_edge_batch(void *d_edges, int32_t nb_pitch, int sz, int is_16bit,
                                      int bd, size_t nblocks, void *stream);

/* ============================================================================
 * (A) drop-in entry points — reference signatures, HOST pointers, synchronous.
 * ==========================================================================*/

/* av1_fwd_txfm2d_WxH (aom_dsp_rtcd.h:160-255) */
#define SVT_HIP_DECL_FWD(W, H) \
    void svt_hip_av1_fwd_txfm2d_##W##x##H(int16_t *input, int32_t *output, uint32_t input_stride, \
                                          svt_tx_type_t transform_type, uint8_t bit_depth);
SVT_HIP_DECL_FWD(4, 4) SVT_HIP_DECL_FWD(8, 8) SVT_HIP_DECL_FWD(16, 16) SVT_HIP_DECL_FWD(32, 32)
SVT_HIP_DECL_FWD(64, 64) SVT_HIP_DECL_FWD(4, 8) SVT_HIP_DECL_FWD(8, 4) SVT_HIP_DECL_FWD(8, 16)
SVT_HIP_DECL_FWD(16, 8) SVT_HIP_DECL_FWD(16, 32) SVT_HIP_DECL_FWD(32, 16) SVT_HIP_DECL_FWD(32, 64)
SVT_HIP_DECL_FWD(64, 32) SVT_HIP_DECL_FWD(4, 16) SVT_HIP_DECL_FWD(16, 4) SVT_HIP_DECL_FWD(8, 32)
SVT_HIP_DECL_FWD(32, 8) SVT_HIP_DECL_FWD(16, 64) SVT_HIP_DECL_FWD(64, 16)
#undef SVT_HIP_DECL_FWD

/* av1_inv_txfm2d_add_WxH (aom_dsp_rtcd.h:350-417): the three signature classes */
#define SVT_HIP_DECL_INV_SQ(W, H) \
    void svt_hip_av1_inv_txfm2d_add_##W##x##H(const int32_t *input, uint16_t *output, int32_t stride, \
                                              svt_tx_type_t tx_type, int32_t bd);
#define SVT_HIP_DECL_INV_R1(W, H) \
    void svt_hip_av1_inv_txfm2d_add_##W##x##H(const int32_t *input, uint16_t *output, int32_t stride, \
                                              svt_tx_type_t tx_type, svt_tx_size_t tx_size, int32_t eob, int32_t bd);
#define SVT_HIP_DECL_INV_R2(W, H) \
    void svt_hip_av1_inv_txfm2d_add_##W##x##H(const int32_t *input, uint16_t *output, int32_t stride, \
                                              svt_tx_type_t tx_type, svt_tx_size_t tx_size, int32_t bd);
SVT_HIP_DECL_INV_SQ(4, 4) SVT_HIP_DECL_INV_SQ(8, 8) SVT_HIP_DECL_INV_SQ(16, 16) SVT_HIP_DECL_INV_SQ(32, 32)
SVT_HIP_DECL_INV_SQ(64, 64)
SVT_HIP_DECL_INV_R1(8, 16) SVT_HIP_DECL_INV_R1(16, 8) SVT_HIP_DECL_INV_R1(16, 32) SVT_HIP_DECL_INV_R1(32, 16)
SVT_HIP_DECL_INV_R1(32, 64) SVT_HIP_DECL_INV_R1(64, 32) SVT_HIP_DECL_INV_R1(8, 32) SVT_HIP_DECL_INV_R1(32, 8)
SVT_HIP_DECL_INV_R1(16, 64) SVT_HIP_DECL_INV_R1(64, 16)
SVT_HIP_DECL_INV_R2(4, 8) SVT_HIP_DECL_INV_R2(8, 4) SVT_HIP_DECL_INV_R2(4, 16) SVT_HIP_DECL_INV_R2(16, 4)
#undef SVT_HIP_DECL_INV_SQ
#undef SVT_HIP_DECL_INV_R1
#undef SVT_HIP_DECL_INV_R2
/* av1_inv_txfm_add (aom_dsp_rtcd.h:421-423): 8-bit recon */
void svt_hip_av1_inv_txfm_add(const svt_tran_low_t *dqcoeff, uint8_t *dst, int32_t stride,
                              const svt_txfm_param *txfm_param);

/* aom_highbd_quantize_b{,_32x32,_64x64} and the 8-bit aom_quantize_b* slots
 * (aom_dsp_rtcd.h:323-342) */
#define SVT_HIP_DECL_QUANT(name) \
    void name(const svt_tran_low_t *coeff_ptr, intptr_t n_coeffs, int32_t skip_block, \
              const int16_t *zbin_ptr, const int16_t *round_ptr, const int16_t *quant_ptr, \
              const int16_t *quant_shift_ptr, svt_tran_low_t *qcoeff_ptr, svt_tran_low_t *dqcoeff_ptr, \
              const int16_t *dequant_ptr, uint16_t *eob_ptr, const int16_t *scan, const int16_t *iscan);
SVT_HIP_DECL_QUANT(svt_hip_aom_highbd_quantize_b)
SVT_HIP_DECL_QUANT(svt_hip_aom_highbd_quantize_b_32x32)
SVT_HIP_DECL_QUANT(svt_hip_aom_highbd_quantize_b_64x64)
SVT_HIP_DECL_QUANT(svt_hip_aom_quantize_b)
SVT_HIP_DECL_QUANT(svt_hip_aom_quantize_b_32x32)
SVT_HIP_DECL_QUANT(svt_hip_aom_quantize_b_64x64)
#undef SVT_HIP_DECL_QUANT

/* EB_SADKERNELNxM_TYPE (EbComputeSAD.h:25-31): one row of NxMSadKernel_funcPtrArray */
uint32_t svt_hip_nxm_sad_kernel(const uint8_t *src, uint32_t src_stride, const uint8_t *ref,
                                uint32_t ref_stride, uint32_t height, uint32_t width);
/* EB_SADLOOPKERNELNxM_TYPE (EbComputeSAD.h:35-47) */
void svt_hip_sad_loop_kernel(uint8_t *src, uint32_t src_stride, uint8_t *ref, uint32_t ref_stride,
                             uint32_t height, uint32_t width, uint64_t *best_sad,
                             int16_t *x_search_center, int16_t *y_search_center,
                             uint32_t src_stride_raw, int16_t search_area_width,
                             int16_t search_area_height);
/* spatial_full_distortion_kernel_func_ptr_array entry (EbPictureOperators.h:470) */
uint64_t svt_hip_spatial_full_distortion_kernel(uint8_t *input, uint32_t input_stride, uint8_t *recon,
                                                uint32_t recon_stride, uint32_t area_width,
                                                uint32_t area_height);
/* ResidualKernel (aom_dsp_rtcd.h:2372) */
void svt_hip_residual_kernel(uint8_t *input, uint32_t input_stride, uint8_t *pred, uint32_t pred_stride,
                             int16_t *residual, uint32_t residual_stride, uint32_t area_width,
                             uint32_t area_height);

/* full_distortion_kernel32_bits / _cbf_zero32_bits (EbPictureOperators.h:268-280) */
void svt_hip_full_distortion_kernel32_bits(int32_t *coeff, uint32_t coeff_stride, int32_t *recon_coeff,
                                           uint32_t recon_coeff_stride, uint64_t distortion_result[2],
                                           uint32_t area_width, uint32_t area_height);
void svt_hip_full_distortion_kernel_cbf_zero32_bits(int32_t *coeff, uint32_t coeff_stride,
                                                    int32_t *recon_coeff, uint32_t recon_coeff_stride,
                                                    uint64_t distortion_result[2], uint32_t area_width,
                                                    uint32_t area_height);

/* intra_pred_fn / intra_high_pred_fn (EbIntraPrediction.h:36-41): one entry per mode;
 * the per-size RTCD slots aom_<mode>_predictor_WxH bind to these with W, H fixed
 * (INTEGRATION.md).  mode = SVT_INTRA_DC .. SVT_INTRA_DC_128. */
void svt_hip_intra_predictor(int mode, int bw, int bh, uint8_t *dst, ptrdiff_t stride,
                             const uint8_t *above, const uint8_t *left);
void svt_hip_highbd_intra_predictor(int mode, int bw, int bh, uint16_t *dst, ptrdiff_t stride,
                                    const uint16_t *above, const uint16_t *left, int32_t bd);
/* av1_dr_prediction_z1/z2/z3 and highbd twins (aom_dsp_rtcd.h:2340-2362) */
void svt_hip_av1_dr_prediction_z1(uint8_t *dst, ptrdiff_t stride, int32_t bw, int32_t bh, const uint8_t *above,
                                  const uint8_t *left, int32_t upsample_above, int32_t dx, int32_t dy);
void svt_hip_av1_dr_prediction_z2(uint8_t *dst, ptrdiff_t stride, int32_t bw, int32_t bh, const uint8_t *above,
                                  const uint8_t *left, int32_t upsample_above, int32_t upsample_left,
                                  int32_t dx, int32_t dy);
void svt_hip_av1_dr_prediction_z3(uint8_t *dst, ptrdiff_t stride, int32_t bw, int32_t bh, const uint8_t *above,
                                  const uint8_t *left, int32_t upsample_left, int32_t dx, int32_t dy);
void svt_hip_av1_highbd_dr_prediction_z1(uint16_t *dst, ptrdiff_t stride, int32_t bw, int32_t bh,
                                         const uint16_t *above, const uint16_t *left, int32_t upsample_above,
                                         int32_t dx, int32_t dy, int32_t bd);
void svt_hip_av1_highbd_dr_prediction_z2(uint16_t *dst, ptrdiff_t stride, int32_t bw, int32_t bh,
                                         const uint16_t *above, const uint16_t *left, int32_t upsample_above,
                                         int32_t upsample_left, int32_t dx, int32_t dy, int32_t bd);
void svt_hip_av1_highbd_dr_prediction_z3(uint16_t *dst, ptrdiff_t stride, int32_t bw, int32_t bh,
                                         const uint16_t *above, const uint16_t *left, int32_t upsample_left,
                                         int32_t dx, int32_t dy, int32_t bd);

/* ---- per-size RTCD slot entry points ------------------------------------------------------------------------------
 * X-macro lists of the reference's slot families (a host can use them too). */
#define SVT_HIP_BLOCK_SIZES_2(X, A, B) \
    X(A, B, 4, 4) X(A, B, 8, 8) X(A, B, 16, 16) X(A, B, 32, 32) X(A, B, 64, 64) X(A, B, 4, 8) X(A, B, 8, 4) X(A, B, 8, 16) \
    X(A, B, 16, 8) X(A, B, 16, 32) X(A, B, 32, 16) X(A, B, 32, 64) X(A, B, 64, 32) X(A, B, 4, 16) X(A, B, 16, 4) \
    X(A, B, 8, 32) X(A, B, 32, 8) X(A, B, 16, 64) X(A, B, 64, 16)
/* SIZES(X, mode, MODE) applied to every non-directional mode: aom_<mode>_predictor_WxH <-> SVT_INTRA_* */
#define SVT_HIP_INTRA_MODES(SIZES, X) \
    SIZES(X, dc, SVT_INTRA_DC) SIZES(X, dc_top, SVT_INTRA_DC_TOP) SIZES(X, dc_left, SVT_INTRA_DC_LEFT) \
    SIZES(X, dc_128, SVT_INTRA_DC_128) SIZES(X, v, SVT_INTRA_V) SIZES(X, h, SVT_INTRA_H) SIZES(X, smooth, SVT_INTRA_SMOOTH) \
    SIZES(X, smooth_v, SVT_INTRA_SMOOTH_V) SIZES(X, smooth_h, SVT_INTRA_SMOOTH_H) SIZES(X, paeth, SVT_INTRA_PAETH)
/* the 22 sizes of aom_sadMxN / aom_sadMxNx4d (aom_dsp_rtcd.h:1328-1500) */
#define SVT_HIP_SAD_SIZES(X) \
    X(128, 128) X(128, 64) X(64, 128) X(64, 64) X(64, 32) X(32, 64) X(32, 32) X(32, 16) X(16, 32) X(16, 16) X(16, 8) \
    X(8, 16) X(8, 8) X(8, 4) X(4, 8) X(4, 4) X(4, 16) X(16, 4) X(8, 32) X(32, 8) X(16, 64) X(64, 16)

/* aom_<mode>_predictor_WxH / aom_highbd_<mode>_predictor_WxH: exactly intra_pred_fn / intra_high_pred_fn
 * (EbIntraPrediction.h:36-41), one per mode and size, storable in the reference's slots and its pred[][] / dc_pred[][][]
 * tables (EbIntraPrediction.c:2842-3350).  10 modes x 19 sizes x {8-bit, high bit depth}. */
#define SVT_HIP_DECL_PRED(mode, MODE, W, H)                                                                             \
    void svt_hip_aom_##mode##_predictor_##W##x##H(uint8_t *dst, ptrdiff_t stride, const uint8_t *above, const uint8_t *left); \
    void svt_hip_aom_highbd_##mode##_predictor_##W##x##H(uint16_t *dst, ptrdiff_t stride, const uint16_t *above,          \
                                                         const uint16_t *left, int bd);
SVT_HIP_INTRA_MODES(SVT_HIP_BLOCK_SIZES_2, SVT_HIP_DECL_PRED)
#undef SVT_HIP_DECL_PRED
/* eb_smooth_v_predictor / eb_smooth_h_predictor (aom_dsp_rtcd.h:259-264) */
void svt_hip_eb_smooth_v_predictor(uint8_t *dst, ptrdiff_t stride, int32_t bw, int32_t bh, const uint8_t *above,
                                   const uint8_t *left);
void svt_hip_eb_smooth_h_predictor(uint8_t *dst, ptrdiff_t stride, int32_t bw, int32_t bh, const uint8_t *above,
                                   const uint8_t *left);
/* aom_sadMxN, aom_sadMxNx4d (aom_dsp_rtcd.h:1328-1500) */
#define SVT_HIP_DECL_SAD(W, H)                                                                                          \
    unsigned int svt_hip_aom_sad##W##x##H(const uint8_t *src_ptr, int src_stride, const uint8_t *ref_ptr, int ref_stride); \
    void svt_hip_aom_sad##W##x##H##x4d(const uint8_t *src_ptr, int src_stride, const uint8_t *const ref_ptr[],            \
                                       int ref_stride, uint32_t *sad_array);
SVT_HIP_SAD_SIZES(SVT_HIP_DECL_SAD)
#undef SVT_HIP_DECL_SAD
/* EB_SADAVGKERNELNxM_TYPE (EbComputeSAD.h:49-57): a row of NxMSadAveragingKernel_funcPtrArray */
uint32_t svt_hip_combined_averaging_sad(uint8_t *src, uint32_t src_stride, uint8_t *ref1, uint32_t ref1_stride,
                                        uint8_t *ref2, uint32_t ref2_stride, uint32_t height, uint32_t width);
/* residual_kernel16bit (EbPictureOperators.c:134) */
void svt_hip_residual_kernel16bit(uint16_t *input, uint32_t input_stride, uint16_t *pred, uint32_t pred_stride,
                                  int16_t *residual, uint32_t residual_stride, uint32_t area_width,
                                  uint32_t area_height);
/* av1_filter_intra_edge{,_high}, av1_upsample_intra_edge{,_high} (aom_dsp_rtcd.h:152-156, 431-437) */
void svt_hip_av1_filter_intra_edge(uint8_t *p, int32_t sz, int32_t strength);
void svt_hip_av1_filter_intra_edge_high(uint16_t *p, int32_t sz, int32_t strength);
void svt_hip_av1_upsample_intra_edge(uint8_t *p, int32_t sz);
void svt_hip_av1_upsample_intra_edge_high(uint16_t *p, int32_t sz, int32_t bd);
/* subtract_average, cfl_predict_lbd / _hbd (aom_dsp_rtcd.h:140-148), av1_txb_init_levels (:2376) */
void svt_hip_subtract_average(int16_t *pred_buf_q3, int32_t width, int32_t height, int32_t round_offset,
                              int32_t num_pel_log2);
void svt_hip_cfl_predict_lbd(const int16_t *pred_buf_q3, uint8_t *pred, int32_t pred_stride, uint8_t *dst,
                             int32_t dst_stride, int32_t alpha_q3, int32_t bit_depth, int32_t width, int32_t height);
void svt_hip_cfl_predict_hbd(const int16_t *pred_buf_q3, uint16_t *pred, int32_t pred_stride, uint16_t *dst,
                             int32_t dst_stride, int32_t alpha_q3, int32_t bit_depth, int32_t width, int32_t height);
void svt_hip_av1_txb_init_levels(const svt_tran_low_t *const coeff, const int32_t width, const int32_t height,
                                 uint8_t *const levels);

/* ---- picture input ("the y4m -> plane upload path") --------------------------------------------------
 * Host: the reference application's y4m reader (Source/App/EncApp/EbAppInputy4m.c) - the same header tokens, the same
 * accepted / rejected files (including its 7-character bound on the 'C' and 'F' tokens), "FRAME\n" delimiters. */
typedef struct svt_hip_y4m_info {
    uint32_t width, height, fr_n, fr_d, bit_depth, interlaced;
    char chroma[8];                /* "420" "422" "444" "411" "400" */
    char scan_type;                /* 'p' 't' 'b' */
} svt_hip_y4m_info;
typedef struct svt_hip_y4m svt_hip_y4m;
/* read_y4m_header (:35-243) on the line that follows the "YUV4MPEG2" signature */
int svt_hip_y4m_parse_header(const char *line, svt_hip_y4m_info *out);
size_t svt_hip_y4m_frame_bytes(const svt_hip_y4m_info *info);
/* check_if_y4m (:269) + read_y4m_header; read_y4m_frame_delimiter (:247) + the planes: 1 = frame read, 0 = end of file */
int svt_hip_y4m_open(const char *path, svt_hip_y4m **out, svt_hip_y4m_info *info);
int svt_hip_y4m_read_frame(svt_hip_y4m *h, void *host_dst, size_t capacity);
void svt_hip_y4m_close(svt_hip_y4m *h);
/* Device: a frame as the file holds it (d_frame: Y, Cb, Cr back to back, u8 or u16 samples, already in HBM) laid out in the
 * encoder's padded plane buffers in ONE launch: the copy, pad_input_picture (EbMcp.c:273; right / bottom extension to the
 * minimum CU size, PadPictureToMultipleOfMinCuSizeDimensions, EbPictureAnalysisProcess.c:4818) and generate_padding{,16_bit}
 * (EbMcp.c:176-267; the borders of origin_x / origin_y samples).  d_y / d_cb / d_cr = first sample of each BUFFER (the picture
 * origin is at (origin_x >> ss, origin_y >> ss)); strides in samples; d_cb = d_cr = NULL for luma only. */
int svt_hip_picture_import(const void *d_frame, uint32_t width, uint32_t height, int ss_x, int ss_y, int is_16bit, void *d_y,
                           uint32_t stride_y, void *d_cb, uint32_t stride_cb, void *d_cr, uint32_t stride_cr,
                           uint32_t origin_x, uint32_t origin_y, uint32_t pad_right, uint32_t pad_bottom, void *stream);
/* generate_padding / generate_padding16_bit in place (the reference also pads reconstructed reference pictures with it,
 * EbEncDecProcess.c:1040-1100): d_buf = first sample of the buffer, picture at (pad_w, pad_h) */
int svt_hip_picture_pad(void *d_buf, uint32_t stride, uint32_t width, uint32_t height, uint32_t pad_w, uint32_t pad_h,
                        int is_16bit, void *stream);
/* The 8-bit plane of a deeper picture, v >> (bd - 8): what the reference keeps as buffer_y next to its bit-increment plane and
 * what its HME / ME / open-loop intra search read; un_pack8_bit_data (C_DEFAULT/EbPackUnPack_C.c:152-175, bd = 10).  Whole padded buffer:
 * cols x rows samples from d_in (16-bit) to d_out (8-bit). */
int svt_hip_picture_luma8(const uint16_t *d_in, uint32_t in_stride, uint8_t *d_out, uint32_t out_stride, uint32_t cols,
                          uint32_t rows, int bd, void *stream);
/* DecimateInputPicture (EbPictureAnalysisProcess.c:4907-4958): Decimation2D (:170) at step 2 (quarter) and 4 (sixteenth) of
 * the luma picture at d_luma (its ORIGIN sample), each followed by generate_padding of the decimated buffer; either output may
 * be NULL.  d_quarter / d_sixteenth = first sample of the buffer. */
int svt_hip_picture_decimate(const uint8_t *d_luma, uint32_t luma_stride, uint32_t width, uint32_t height, uint8_t *d_quarter,
                             uint32_t q_stride, uint32_t q_origin_x, uint32_t q_origin_y, uint8_t *d_sixteenth,
                             uint32_t s_stride, uint32_t s_origin_x, uint32_t s_origin_y, void *stream);

/* ---- GatheringPictureStatistics for a whole picture (EbPictureAnalysisProcess.c:4759-4812; runs between decimation and ME) -----
 * svt_hip_picture_stats_frame computes, for one picture or a stack of n_pictures under one parameter set, what rate control, the
 * mode-decision configuration and scene-change detection read of the picture-analysis stage: the 85 luma block means and variances
 * and the 21 Cb / Cr block means of every 64x64 SB (ComputePictureSpatialStatistics :4631), pic_avg_variance (:4686-4689), the
 * per-region 256-bin histograms of the 1/16 luma and of the chroma planes (:4146-4284, CalculateHistogram :201-225) and the
 * average intensities (:4191, :4255, :4746-4748).  Two launches whatever n_pictures is (SB statistics + histograms; the
 * per-picture sums); nothing is allocated, nothing returns to the host, no buffer has to be zeroed, the call only enqueues and
 * can be captured into a HIP graph.  No atomics: the result is deterministic.
 *
 * Planes, all 8-bit (the reference analyses the 8-bit planes of a 10-bit input too), 4:2:0: k = 0 the padded luma, 1 / 2 the padded
 * Cb / Cr, 3 the padded 1/16 luma (svt_hip_picture_decimate).  As in svt_hip_me_pyramid d_plane[k] is the START of the buffer,
 * sample (0, 0) sits at (origin_x[k], origin_y[k]), rows are stride[k] bytes apart, picture i of a stack lies pitch[k] * i bytes
 * further.  The chroma origin is the luma origin >> 1 (origin_x[1] = origin_x[2] = origin_x[0] >> 1, likewise y).  The luma padding
 * must be at least 64 samples on every side: a partial SB reads its full 64x64 from the padding, as the reference does.
 *
 * Luma 8x8 blocks (ComputeBlockMeanComputeVariance :2066-3084), S = sum of samples, Q = sum of squares:
 *   block_mean_calc_prec 1 (BLOCK_MEAN_PREC_SUB, what the encoder sets, EbResourceCoordinationProcess.c:599): rows 0, 2, 4, 6 only,
 *     mean = S << 3, meansq = Q << 11 (compute_interm_var_four8x8_avx2_intrin); 0 (BLOCK_MEAN_PREC_FULL): all rows, mean = S << 2,
 *     meansq = Q << 10.  16x16, 32x32, 64x64: (a + b + c + d) >> 2 of the four children, mean and meansq separately, level by level
 *     (:2843-2896).  y_mean = mean >> 8, variance = (uint16)((meansq - mean * mean) >> 16) in 64-bit arithmetic (:2899-3082).
 * Chroma (ComputeChromaBlockMean :1770-2058): only for complete SBs (origin + 64 <= picture side both ways, is_complete_sb); all 21
 *   entries of both planes are 0 for the others (ZeroOutChromaBlockMean :1706).  The sixteen 8x8 chroma means by the same SUB / FULL
 *   formula, their tree to 32x32 and 64x64.  DIVERGENCE KEPT ON PURPOSE: the reference's 64x64 line reads
 *   (m32[0] + m32[1] + m32[3] + m32[3]) >> 2 (:2006-2007: entry 2 is never added, entry 3 twice), and so does this call.
 * Histograms: a region is side / regions wide, the last takes the remainder; bins start at 1.  Luma: the 1/16 picture
 *   ((w >> 2) x (h >> 2)), every sample, each bin << 4 after counting, region average (sum + (area >> 1)) / area.  Chroma: the full
 *   plane, region origin ((ox + r * regionW) >> 1, (oy + r * regionH) >> 1) with the luma origin and region size, area
 *   (regionW' >> 1) x (regionH' >> 1), every 4th sample of every 4th row, bins and sum << 4, region average
 *   (sum + (A >> 3)) / (A >> 2) with A the region's luma area.  Every average is cast to uint8 as the reference casts it.
 *   Picture averages: :4746-4748, the lines of every scd_mode but SCD_MODE_0.  The SCD_MODE_0 branch (:4718-4743) is outside this
 *   call: it indexes buffer_y without the picture origin, so it averages the padding.
 *
 * Outputs, all on the device, every entry written; SB index s = picture * nsb + sb_y * nsbx + sb_x (nsbx = (width + 63) / 64), rw /
 * rh = regions_per_width / _height:
 *   d_y_mean               uint8  [s][85]                  ME_TIER_ZERO_PU_* order (EbMotionEstimationContext.h:50-135): 0 = 64x64,
 *   d_variance             uint16 [s][85]                  1-4 = 32x32, 5-20 = 16x16, 21-84 = 8x8, each in raster order
 *   d_cb_mean, d_cr_mean   uint8  [s][21]                  the same order: 5-20 are the 8x8 chroma blocks
 *   d_pic_avg_variance     uint16 [picture]                sum of the SBs' 64x64 variances / nsb
 *   d_histogram            uint32 [picture][rw][rh][3][256] picture_histogram[region w][region h][plane]
 *   d_avg_intensity_region uint8  [picture][rw][rh][3]     average_intensity_per_region
 *   d_avg_intensity        uint8  [picture][3]             average_intensity
 *
 * Every argument is checked before the first launch (SVT_HIP_ERR_INVALID): NULL planes or outputs, misaligned 16- / 32-bit outputs, sides that
 * are not multiples of 8 or exceed 16384, a precision other than 0 / 1, a region count outside 1 .. 4 or larger than the 1/16
 * picture's side (the reference divides by a zero area there), luma padding below 64 on any side, a chroma origin that is not
 * the luma origin >> 1, strides or pitches too small, more than 65535 pictures.  n_pictures = 0 is a successful no-op. */
enum { SVT_HIP_BLOCK_MEAN_PREC_FULL = 0, SVT_HIP_BLOCK_MEAN_PREC_SUB = 1 };           /* EB_BLOCK_MEAN_PREC */
enum { SVT_HIP_PIC_STATS_LUMA = 0, SVT_HIP_PIC_STATS_CB = 1, SVT_HIP_PIC_STATS_CR = 2, SVT_HIP_PIC_STATS_SIXTEENTH = 3 };
typedef struct svt_hip_pic_stats_planes {
    const uint8_t *d_plane[4];
    uint32_t stride[4], origin_x[4], origin_y[4];
    uint64_t pitch[4];                                /* between the pictures of a stack (ignored for n_pictures 1) */
} svt_hip_pic_stats_planes;
typedef struct svt_hip_pic_stats_params {
    int32_t picture_width, picture_height;            /* luma; multiples of 8, at most 16384 */
    int32_t block_mean_calc_prec;                     /* SVT_HIP_BLOCK_MEAN_PREC_FULL / _SUB */
    int32_t regions_per_width, regions_per_height;    /* picture_analysis_number_of_regions_per_width / _height, 1 .. 4 */
} svt_hip_pic_stats_params;
typedef struct svt_hip_pic_stats_out {
    uint8_t *d_y_mean;
    uint16_t *d_variance;
    uint8_t *d_cb_mean, *d_cr_mean;
    uint16_t *d_pic_avg_variance;
    uint32_t *d_histogram;
    uint8_t *d_avg_intensity_region, *d_avg_intensity;
} svt_hip_pic_stats_out;
int svt_hip_picture_stats_frame(const svt_hip_pic_stats_planes *planes, const svt_hip_pic_stats_params *params,
                                uint32_t n_pictures, const svt_hip_pic_stats_out *out, void *stream);

/* ---- AV1 inter prediction for whole pictures (av1_inter_prediction / av1_inter_prediction_hbd, EbInterPrediction.c:1024, :2093) -----
 * svt_hip_inter_pred_frame turns motion vectors into predictions: translational prediction of one plane for many (plane, block size)
 * groups per call, one launch per SVT_HIP_INTER_PRED_MAX_GROUPS non-empty groups.  Samples are uint8 (bd 8) or uint16 (bd 10); strides
 * are in samples.  The call only enqueues (no allocation, no synchronisation) and can be captured into a HIP graph.
 *
 * Per block (svt_hip_inter_blk, device memory, one per (block, candidate)), in the reference's order:
 *   clamp      clamp_mv_to_umv_border_sb (:80-102) per list: the vector is scaled by 1 << (1 - ss) and cast to int16 first, then
 *              clamped to [mb_to_left_edge * (1 << (1 - ss)) - ((4 + bw) << 4), mb_to_right_edge * (1 << (1 - ss)) + ((4 + bw) << 4) - 16]
 *              (rows likewise), bw / bh the PLANE's block size, the edges from the block's luma origin, its size in mode-info units
 *              and mi_cols = pic_width / 4, mi_rows = pic_height / 4 (EbAdaptiveMotionVectorPrediction.c:1169-1172).
 *   address    luma: (x, y); chroma: (((x >> 3) << 3) / 2, ((y >> 3) << 3) / 2) (:1310); plus the clamped vector >> 4.
 *   filters    av1_get_interp_filter_params_with_block_size per direction: a plane dimension <= 4 takes the 4-tap tables (REGULAR
 *              and SHARP sub_pel_filters_4, SMOOTH sub_pel_filters_4smooth); filter_x and filter_y may differ.
 *   convolve   the convolve[subpel_x != 0][subpel_y != 0][compound] entry with get_conv_params_no_round (round_0 3; round_1 11, or 7
 *              for BI_PRED), use_jnt_comp_avg 0: all sixteen _c entries, 8-bit and highbd.
 *   BI_PRED    list 0 through the jnt entry (do_average 0), list 1 with do_average 1: ((c0 + c1) >> 1) minus the round offset,
 *              rounded by 4 bits and clipped.  List 0's intermediate lives in registers only.
 * The prediction is the dst_ptr contents after the call(s) of the plane; the block's x / y also place it in a strided d_pred and
 * in d_src (x, y for luma, the chroma address above for chroma).
 *
 * Fused distortion (d_src and d_dist both set): the prediction against the source block at the block's own origin, SVT_HIP_FAST_SAD
 * or SVT_HIP_FAST_SSD with their C-flavour definitions above, summed while the prediction is on chip; d_pred may be NULL then.
 *
 * BORDER CONTRACT (trusted, as for motion estimation): d_ref[l] points at sample (0, 0) of the PICTURE in list l's plane and the
 * plane carries, on every side, at least bw + 8 (bh + 8 above and below) plane samples of border for a luma group and bw + 10
 * (bh + 10) for a chroma group.  Derivation, per direction in plane samples, P the plane's side, p the block's position: the clamp
 * leaves p + (mv >> 4) in [-(bw + 4), P + 3] whatever x and the vector are (the vector's whole part is at least
 * -p - (4 + bw) and at most P - bw - p + (4 + bw) - 1); the 8-tap window reaches 3 samples before and
 * bw - 1 + 4 after that, so samples -(bw + 7) .. P + bw + 6 are read: bw + 7 on either side, for every phase (a full-pel block's
 * window is staged too when its wave filters).  Chroma floors the origin to the 8-grid (at most 2 plane samples lower than the
 * position the clamp was derived for): bw + 9.  The contract rounds both up.  x and y are multiples of 4, as every AV1 block origin
 * is (the edges are taken from x >> 2: an origin off that grid would reach up to 3 samples further on the far side).  x / y beyond pic - bwidth / - bheight are read as
 * that bound; pred_direction above 2 as 2, a filter above 3 as 3: such a block's prediction is unspecified, its accesses stay inside
 * the windows above and the block's own output.  d_ref[1] may be NULL only when no block of the group has pred_direction 1 or 2
 * (device data: not checked, unspecified otherwise).
 *
 * Validated before the first launch (SVT_HIP_ERR_INVALID, nothing launched): bd 8 / 10; metric; picture sides non-zero multiples of
 * 8 up to 16384; per group ss 0 / 1, bwidth and bheight in {4, 8, 16, 32, 64} (chroma: both >= 8) and not above the picture,
 * d_blk and d_ref[0] set, at least one of d_pred / (d_src, d_dist), d_src and d_dist together, d_dist 8-byte, d_blk 4-byte and a
 * dense d_pred 16-byte aligned, pred_stride 0 or >= the plane block's width, nblocks within one launch.  Not built: see DESIGN.md
 * section 7 (OBMC, global motion, masked and distance-weighted compound, scaled references, intrabc, sub-8x8 chroma, bd 12).  The local
 * warp of WARPED_CAUSAL candidates is svt_hip_warp_fit_frame / svt_hip_warp_pred_frame below; the chroma of a warped block below 16 in
 * either dimension is translational with interp_filters 0 (EbInterPrediction.c:2706-2768) and is this call's. */
enum { SVT_HIP_UNI_PRED_LIST_0 = 0, SVT_HIP_UNI_PRED_LIST_1 = 1, SVT_HIP_BI_PRED = 2 };    /* EbDefinitions.h:2061-2063 */
#define SVT_HIP_INTER_PRED_MAX_GROUPS 48
typedef struct svt_hip_inter_blk {       /* sizeof 16 */
    uint16_t x, y;                       /* luma origin of the block in the picture: pu_origin_x / _y */
    int16_t mv[2][2];                    /* [list][0 = x, 1 = y], 1/8 luma sample, as MvUnit_t */
    uint8_t pred_direction;              /* SVT_HIP_UNI_PRED_LIST_0 / _1 / SVT_HIP_BI_PRED */
    uint8_t filter_x, filter_y;          /* InterpFilter 0 .. 3: av1_extract_interp_filter(interp_filters, 1) / (.., 0) */
    uint8_t pad;
} svt_hip_inter_blk;
typedef struct svt_hip_inter_pred_group {
    const void *d_ref[2];                /* sample (0, 0) of the picture in each list's plane; the border lies at negative offsets */
    uint32_t ref_stride;
    int32_t ss;                          /* 0: a luma plane; 1: a chroma plane of 4:2:0 */
    int32_t bwidth, bheight;             /* LUMA block size; the plane's block is (bwidth >> ss) x (bheight >> ss) */
    uint32_t nblocks;
    const svt_hip_inter_blk *d_blk;      /* [nblocks] */
    void *d_pred;                        /* optional when the distortion is asked for */
    uint32_t pred_stride;                /* 0: dense [nblocks][h][w] (what svt_hip_full_loop_group.d_pred reads); else a plane, block at its origin */
    const void *d_src;                   /* optional source plane, sample (0, 0) of the picture, for the fused distortion */
    uint32_t src_stride;
    uint64_t *d_dist;                    /* optional [nblocks] */
} svt_hip_inter_pred_group;
int svt_hip_inter_pred_frame(const svt_hip_inter_pred_group *groups, int ngroups, uint32_t pic_width, uint32_t pic_height, int bd,
                             int metric, void *stream);

/* ---- Warped motion: the local warp model of a block and its prediction (WARPED_CAUSAL candidates) -----------------------------------
 * The two steps every candidate of inject_warped_motion_candidates (EbModeDecision.c:1120-1318) needs, for many groups per call, one
 * launch per SVT_HIP_INTER_PRED_MAX_GROUPS non-empty groups.  Both calls only enqueue (no allocation, no synchronisation) and can be
 * captured into a HIP graph.
 *
 * svt_hip_warp_fit_frame: warped_motion_parameters (EbAdaptiveMotionVectorPrediction.c:1876-1937) from the point where the samples
 * exist.  Gathering them (av1_find_samples / wm_count_samples, the walks over the mode-info grid of decided neighbours) stays the
 * caller's, like MVP generation: d_samples[b] is what av1_find_samples returned for block b, and the ncand candidates of a block (the
 * nine NEWMV refinements among them) share it.  A group is one block size (bsize in AV1 block_size order; a block below 8 in either
 * dimension has no warped motion, :1898, and a 128 side is not built: both are refused).  Per (block, candidate), with the
 * candidate's x, y and mv[0] (svt_hip_inter_blk; mi_col = x >> 2, mi_row = y >> 2), to the letter:
 *   nsamples == 0 -> invalid, nothing else computed.
 *   select_samples (:1512) when nsamples > 1: the threshold clamp(max(bw, bh), 16, 112) on |dx| + |dy| against the candidate's
 *              vector; none below it -> "keep at least 1" (the first sample alone).  The reference then compacts the kept samples by
 *              a walk from both ends; the walk only permutes them and every sum of the fit is order-free, so the device marks them.
 *   find_affine_int (EbWarpedMotion.c:1066): the LS_* sums in int32 over the samples with |sx - dx| and |sy - dy| below LS_MV_MAX; Det == 0 ->
 *              invalid; resolve_divisor_64 (the int16 iDet, `shift < 0` branch included); get_mult_shift_diag / _ndiag in 64 bits with
 *              their clamps; vx / vy in wrapping int32 with the WARPEDMODEL_TRANS_CLAMP clamp.
 *   get_shear_params (:344): resolve_divisor_32, the signed 64-bit rounding, the int16 clamps, the WARP_PARAM_REDUCE_BITS rounding
 *              (stored back into int16) and is_affine_shear_allowed.
 * d_model[b][c]: valid = local_warp_valid (!find_projection), num_proj_ref = the sample count find_projection saw (0 without
 * samples), mat = wmmat[0..5] and the four shears as far as the reference wrote them into a zeroed EbWarpedMotionParams (all 0 when
 * Det == 0; set, with valid 0, when the shear is refused).  d_nvalid[b] (optional) counts the block's valid models.  nsamples is
 * device data and is clamped to 0 .. 8.
 *
 * svt_hip_warp_pred_frame: one plane of warped_motion_prediction (EbInterPrediction.c:2584): av1_warp_plane (8 bit) /
 * av1_warp_plane_hbd (10 bit) -> av1_warp_affine_c / av1_highbd_warp_affine_c (EbWarpedMotion.c:672, :389) with a single reference,
 * is_compound 0, round_0 3, 11 bits of vertical rounding and clip(sum - (1 << (bd - 1)) - (1 << bd)).  Per 8x8 tile at (j, i) of the
 * plane block: the centre ((j + 4) << ss, (i + 4) << ss) in luma coordinates through mat in wrapping int32, arithmetic >> ss and
 * >> 16, sx4 / sy4 after the -4 * (alpha + beta) / -4 * (gamma + delta) step and the 6-bit mask, offs = ((s + 512) >> 10) + 64 per
 * sample, and BOTH source coordinates of every sample clamped to the plane, [0, (pic_width >> ss) - 1] x [0, (pic_height >> ss) - 1].
 * The reference reads no border here, so this call has NO border contract: d_ref points at sample (0, 0) of the plane and nothing
 * outside pic_width >> ss by pic_height >> ss is read.  A luma group takes bwidth / bheight 8 .. 64 (rectangles included); a chroma
 * group (ss 1) needs both luma sides >= 16 (:2653).  The chroma of smaller blocks is predicted translationally with interp_filters 0
 * (:2706-2768): that is svt_hip_inter_pred_frame's job and is not rebuilt here.
 * Addressing, slots numbered [nblocks][k]:
 *   direct     d_sel NULL, k = ncand: record r = b * ncand + c of d_blk / d_model is predicted into slot r.
 *   survivors  d_sel = svt_hip_inter_fast_pick_frame's d_cand ([nblocks][n]), k = n: for slot (b, s), c = d_sel[b][s] - sel_first; when
 *              0 <= c < ncand, record [b][c] is predicted into slot [b][s], otherwise the slot is left untouched.  This overwrites the
 *              warped survivors in svt_hip_inter_fast_search_frame's d_pred_out after that call.
 * A record whose model has valid == 0 leaves its slot untouched (prediction and distortion) in both modes.  Outputs per slot: d_pred
 * (dense [slot][h][w] with pred_stride 0, else a plane with the block at its own origin) and / or the fused distortion d_dist[slot]
 * against d_src at the block's origin (SVT_HIP_FAST_SAD / SVT_HIP_FAST_SSD, C flavour); d_pred is optional then.
 * mat and the shears are device data: offs is clamped to 0 .. 192 before it indexes (a valid model never reaches the clamp,
 * is_affine_shear_allowed bounds it), every source address is clamped as above and x / y beyond pic - bwidth / - bheight are read as
 * that bound, so a garbage model gives an unspecified prediction for its own slot and nothing else.
 *
 * Validated before the first launch (SVT_HIP_ERR_INVALID, nothing launched).  Fit: bsize 0 .. 21 with both sides 8 .. 64; ncand
 * 1 .. 64; d_samples, d_blk, d_model set and 4-byte aligned (d_nvalid too when given); nblocks within one launch.  Prediction: bd 8 /
 * 10; metric; picture sides non-zero multiples of 8 up to 16384; ss 0 / 1; bwidth and bheight in {8, 16, 32, 64} (chroma: both >= 16)
 * and not above the picture; ncand 1 .. 64; d_ref, d_blk, d_model set, d_blk and d_model 4-byte aligned; at least one of d_pred /
 * (d_src, d_dist), d_src and d_dist together, d_dist 8-byte and a dense d_pred 16-byte aligned, pred_stride 0 or >= the plane block's
 * width; with d_sel n 1 .. 64 and sel_first 0 .. 255, without it n == 0 and sel_first == 0; nblocks * k within one launch.
 * Not built: see DESIGN.md section 7 (OBMC, global motion and ROTZOOM, compound warp, av1_warp_error, the sample walks, bd 12, 4:2:2 /
 * 4:4:4, warped_motion_prediction_md). */
typedef struct svt_hip_warp_samples {    /* sizeof 132: what av1_find_samples returns for a block */
    int32_t nsamples;                    /* 0 .. 8 */
    int32_t pts[16];                     /* [sample][x, y], 1/8 sample, relative to the block's origin */
    int32_t pts_inref[16];
} svt_hip_warp_samples;
typedef struct svt_hip_warp_model {      /* sizeof 36 */
    int32_t mat[6];                      /* EbWarpedMotionParams.wmmat[0..5] */
    int16_t alpha, beta, gamma, delta;
    uint8_t valid;                       /* local_warp_valid */
    uint8_t num_proj_ref;
    uint8_t pad[2];
} svt_hip_warp_model;
typedef struct svt_hip_warp_fit_group {
    int32_t bsize;                       /* AV1 block_size order */
    uint32_t nblocks;
    int32_t ncand;                       /* candidates per block, 1 .. 64 */
    const svt_hip_warp_samples *d_samples;   /* [nblocks] */
    const svt_hip_inter_blk *d_blk;      /* [nblocks][ncand]: x, y, mv[0] */
    svt_hip_warp_model *d_model;         /* [nblocks][ncand] */
    uint32_t *d_nvalid;                  /* optional [nblocks] */
} svt_hip_warp_fit_group;
int svt_hip_warp_fit_frame(const svt_hip_warp_fit_group *groups, int ngroups, void *stream);
typedef struct svt_hip_warp_pred_group {
    const void *d_ref;                   /* sample (0, 0) of the picture plane; no border is read */
    uint32_t ref_stride;
    int32_t ss;                          /* 0: a luma plane; 1: a chroma plane of 4:2:0 */
    int32_t bwidth, bheight;             /* LUMA block size */
    uint32_t nblocks;
    int32_t ncand;                       /* records per block, 1 .. 64 */
    const svt_hip_inter_blk *d_blk;      /* [nblocks][ncand]: x, y */
    const svt_hip_warp_model *d_model;   /* [nblocks][ncand] */
    const uint8_t *d_sel;                /* NULL: direct; else [nblocks][n] list positions */
    int32_t n, sel_first;                /* survivors per block; the list position of the block's record 0 */
    void *d_pred;                        /* optional when the distortion is asked for */
    uint32_t pred_stride;                /* 0: dense [slot][h][w]; else a plane, block at its origin */
    const void *d_src;                   /* optional source plane, sample (0, 0) of the picture */
    uint32_t src_stride;
    uint64_t *d_dist;                    /* optional [slot] */
} svt_hip_warp_pred_group;
int svt_hip_warp_pred_frame(const svt_hip_warp_pred_group *groups, int ngroups, uint32_t pic_width, uint32_t pic_height, int bd, int metric,
                            void *stream);
/* HOST, no device: the project's statement of the warp filter of the AV1 specification (7.11.3.5, Warped_Filters), [193][8], and of its
 * divisor table (Div_Lut, [257]), as the kernels use them. */
void svt_hip_warp_tables(int16_t *filter, uint16_t *div_lut);

/* ---- Interpolation filter search of mode decision (interpolation_filter_search, EbInterPrediction.c:3578-3917) ---------------------
 * For an inter candidate the reference predicts the block with up to nine (vertical, horizontal) filter pairs out of {REGULAR, SMOOTH,
 * SHARP}, takes the SSE of every prediction against the source, models rate and distortion from it and keeps the first strict minimum
 * of the RD cost.  Three calls: the table, the walk, and both in one.  8-bit samples only (bd != 8 is refused: DESIGN.md section 7).
 *
 * svt_hip_interp_sse_frame: THE TABLE.  Per block record (the svt_hip_inter_blk of svt_hip_inter_pred_frame; filter_x / filter_y are
 * ignored) and plane (Y alone, or Y, Cb, Cr with use_uv), d_sse[block][plane][i], i = 0 .. 8, is the SSE (highbd_variance64_c, :3231,
 * truncated to 32 bits as highbd_8_variance does) between the source block and the prediction svt_hip_inter_pred_frame writes for that
 * plane with filter pair i.  Pair i is filter_sets[i] (:3573) through av1_make_interp_filters(y_filter, x_filter): the VERTICAL filter
 * is i / 3 (filter_y), the horizontal one i % 3 (filter_x).  Everything else is svt_hip_inter_pred_frame's and is stated there: the
 * clamp, the luma / chroma addressing, the 4-tap tables of a plane dimension <= 4 (the chroma of 8-wide blocks), BI_PRED through the two
 * jnt entries, the BORDER CONTRACT (luma borders for d_ref[l][0], chroma borders for d_ref[l][1 .. 2]), the rules for x / y and for
 * out-of-range device bytes.  d_ref[1][p] may be NULL only when no block of the group has pred_direction 1 or 2.  All nine pairs are
 * always computed; per list the (w + 7) x (h + 7) window is staged once and three horizontal passes feed nine vertical ones; no
 * prediction leaves the chip.  One launch per SVT_HIP_INTER_PRED_MAX_GROUPS (group, plane) entries; nothing is zeroed by the caller.
 * Validated before the first launch (SVT_HIP_ERR_INVALID, nothing launched): bd 8; picture sides as svt_hip_inter_pred_frame; bwidth and
 * bheight in {8, 16, 32, 64} and not above the picture; d_blk (4-byte aligned), d_sse (4-byte aligned), d_ref[0][0], d_src[0] set and,
 * with use_uv, d_ref[0][1 .. 2] and d_src[1 .. 2]; nblocks within one launch (the luma tiling's workgroups).
 *
 * svt_hip_interp_decide_frame: THE WALK, to the letter, one svt_hip_interp_decision per block.  Per pair i, model_rd_for_sb (:3440-3529):
 * per plane model_rd_from_sse(sse, num_pels_log2 of the PLANE block, ac_dequant_q3 >> 3), ac_dequant_q3 = y_dequant_Q3[qindex][1], the
 * LUMA AC value for all three planes (:3507-3516); rate and distortion summed in uint64, the rate cast to int32; skip_txfm_sb =
 * total_sse == 0, skip_sse_sb = total_sse << 4.  rs = d_rates[ctx[0]][i / 3] + d_rates[ctx[1]][i % 3] (av1_get_switchable_rate, :3184:
 * dir 0 reads the vertical filter; d_rates is switchable_interp_FacBitss, int32 [16][3]; d_ctx[block][dir] is
 * av1_get_pred_context_switchable_interp, the caller's, read as min(ctx, 15)).  rd = RDCOST(full_lambda, rs + rate, dist) = (((uint64)
 * (int32)(rs + rate) * full_lambda + 256) >> 9) + dist * 128 held as int64 (:3305).  Pair 0 first (:3621-3661); a later pair replaces
 * the best only when its rd is strictly below, and switchable_rate, skip_txfm_sb and skip_sse_sb follow the winner.  Pairs tried:
 *   SVT_HIP_INTERP_DUAL_FAST  :3672-3825: 1, 2, then best + 3 and best + 6, best the winner among 0 .. 2;
 *   SVT_HIP_INTERP_FULL       :3828 with enable_dual_filter: 1 .. 8;
 *   SVT_HIP_INTERP_SINGLE     :3828 without: 4, 8.
 * interp_filters = y_filter | x_filter << 16 of the winner.  A block whose d_searchable byte is 0 (av1_is_interp_needed, the caller's)
 * gets the :3909-3911 result: interp_filters 0 and pair 0's rd, rate and skip values.  d_blk_out (optional, with d_blk): the block's
 * record with filter_x / filter_y set from the winner, ready for svt_hip_inter_pred_frame (the reference's :4470); d_blk_out may equal
 * d_blk (a thread reads its record before it writes it) but must not overlap it otherwise.  Only the block index addresses memory from
 * device data.  Validated before the launch: params and d_rates set, mode 0 .. 2, ac_dequant_q3 0 .. 32767; per group the sides as
 * above, d_sse (4-byte), d_ctx, d_searchable, d_decision (8-byte) set, d_blk with d_blk_out (4-byte each).
 *
 * svt_hip_interp_search_frame: both on `stream`, whose order carries the dependency.  sse.d_sse may be NULL: the table then lives in
 * d_scratch, per non-empty group in group order nblocks * planes * 36 bytes rounded up to 16; svt_hip_interp_search_scratch_bytes (HOST)
 * returns the sum (0: bad parameters or nothing to carve).  d_scratch 16-byte aligned.  Both stages are validated before the first
 * launch.  All calls only enqueue, allocate nothing and can be captured into a HIP graph. */
enum { SVT_HIP_INTERP_DUAL_FAST = 0, SVT_HIP_INTERP_FULL = 1, SVT_HIP_INTERP_SINGLE = 2 };
typedef struct svt_hip_interp_sse_group {
    const uint8_t *d_ref[2][3];          /* [list][Y, Cb, Cr]: sample (0, 0) of the picture in each plane */
    uint32_t ref_stride[3];              /* Y, Cb, Cr; both lists */
    const uint8_t *d_src[3];             /* source planes, sample (0, 0) of the picture */
    uint32_t src_stride[3];
    int32_t bwidth, bheight;             /* LUMA block size */
    uint32_t nblocks;
    const svt_hip_inter_blk *d_blk;      /* [nblocks] */
    uint32_t *d_sse;                     /* [nblocks][use_uv ? 3 : 1][9] */
} svt_hip_interp_sse_group;
int svt_hip_interp_sse_frame(const svt_hip_interp_sse_group *groups, int ngroups, uint32_t pic_width, uint32_t pic_height, int bd,
                             int use_uv, void *stream);

typedef struct svt_hip_interp_decision { /* sizeof 32, 8-byte aligned */
    uint32_t interp_filters;             /* y_filter | x_filter << 16 */
    int32_t  switchable_rate;
    int64_t  rd;
    int64_t  skip_sse_sb;
    int32_t  skip_txfm_sb;
    uint32_t pad;                        /* written as 0 */
} svt_hip_interp_decision;
typedef struct svt_hip_interp_params {
    uint32_t full_lambda;
    int32_t ac_dequant_q3;               /* y_dequant_Q3[qindex][1] */
    const int32_t *d_rates;              /* switchable_interp_FacBitss: int32 [16][3], device */
    int32_t use_uv, mode;                /* mode: SVT_HIP_INTERP_DUAL_FAST / _FULL / _SINGLE */
} svt_hip_interp_params;
typedef struct svt_hip_interp_decide_group {
    int32_t bwidth, bheight;             /* LUMA block size */
    uint32_t nblocks;
    const uint32_t *d_sse;               /* [nblocks][use_uv ? 3 : 1][9] */
    const uint8_t *d_ctx;                /* [nblocks][2] */
    const uint8_t *d_searchable;         /* [nblocks] */
    svt_hip_interp_decision *d_decision; /* [nblocks] */
    const svt_hip_inter_blk *d_blk;      /* optional, with d_blk_out */
    svt_hip_inter_blk *d_blk_out;        /* optional [nblocks] */
} svt_hip_interp_decide_group;
int svt_hip_interp_decide_frame(const svt_hip_interp_decide_group *groups, int ngroups, const svt_hip_interp_params *params, void *stream);

typedef struct svt_hip_interp_search_group {
    svt_hip_interp_sse_group sse;        /* sse.d_sse may be NULL */
    const uint8_t *d_ctx, *d_searchable;
    svt_hip_interp_decision *d_decision;
    svt_hip_inter_blk *d_blk_out;        /* optional; may equal sse.d_blk */
} svt_hip_interp_search_group;
size_t svt_hip_interp_search_scratch_bytes(const svt_hip_interp_search_group *groups, int ngroups, int use_uv);   /* HOST */
int svt_hip_interp_search_frame(const svt_hip_interp_search_group *groups, int ngroups, uint32_t pic_width, uint32_t pic_height, int bd,
                                const svt_hip_interp_params *params, void *d_scratch, size_t scratch_bytes, void *stream);

/* ---- The fast loop for inter candidates: fast cost, the N best over the block's combined list, the survivors' records ----------------
 * svt_hip_inter_fast_pick_frame is svt_hip_fast_pick_frame for the list ProductGenerateMdCandidatesCu builds for a P or B picture:
 * per block `ninter` inter candidates followed by `nintra` intra candidates (the order in which fast_candidate_array is filled),
 * ncand = ninter + nintra <= 64.  svt_hip_inter_pred_frame (distortion only) writes its d_dist*, svt_hip_fast_pick_frame's d_all_cost
 * with slice_is_intra 0 is the intended d_intra_cost; its d_blk_out is a svt_hip_inter_pred_frame d_blk of nblocks * n records.
 * Everything that depends on MVP generation arrives as bytes (mode_ctx, ref_mv_count, drl_ctx, the predicted vectors), the split
 * d_ctx / d_searchable make in the interpolation search.  is_compound is pred_direction == SVT_HIP_BI_PRED: every injector of
 * EbModeDecision.c sets the two together (its twenty assignments of is_compound, :538 .. :2345, each beside prediction_direction[0]:
 * is_compound 0 with UNI_PRED_LIST_0 / _1, is_compound 1 with BI_PRED).
 * What is reproduced, to the letter:
 *   cost     av1_inter_fast_cost (EbRateDistortionCost.c:971-1318) with EstimateRefFramesNumBits (:741-947) and Av1ModeContextAnalyzer
 *            (:951-969, compound_mode_ctx_map_2); rf[] = av1_set_ref_frame(ref_frame_type) (EbAdaptiveMotionVectorPrediction.c:214-258).
 *            Reference bits :781-942 (compInterFacBits only under reference_mode_select and min(bw, bh) >= 8, the luma block of bsize);
 *            mode bits :1037-1057 (NEWMV / GLOBALMV / NEARESTMV cascade, or the compound table at the mapped context); the two DRL
 *            loops with their breaks :1058-1088; the MV rate :1090-1198, each av1_mv_bit_cost (:91-95) = (joint + comp[0][row diff] +
 *            comp[1][col diff]) * 108 rounded by 7 bits, d_mv_cost indexed from its centre entry MV_MAX = 16383
 *            (EbMdRateEstimation.c:363-366); motion-mode bits :1203-1229 out of motionModeFacBits1 (allowed == OBMC) or
 *            motionModeFacBits; intraInterFacBits[is_inter_ctx][1] :1250; then SAD RDCOST(lambda, rate, luma + chroma) or the two
 *            model_rd_from_sse calls :1260-1294 (quantiser ac_dequant_q3, bsize and bsize_uv).
 *   walk     the second loop of perform_fast_loop (EbProductCodingLoop.c:1225-1363) over the combined list from the last entry down,
 *            as svt_hip_fast_pick_frame states it.  Every candidate has distortion_ready 0 (only inject_intra_candidates_ois sets it),
 *            so the first, src-to-src loop (:1180-1222) does nothing and stays out of scope.
 *   order    sort_fast_loop_candidates (EbModeDecision.c:436-489) INCLUDING the "inter then intra" pass (:458-469).
 * Quirks kept:
 *   - lumaRate is summed in uint32 (:1251); fast_luma_rate / fast_chroma_rate (d_rate) are stored BEFORE the SSD model's rates are
 *     added (:1257-1258); chromaRate is 0 for inter and under SSD the model's chroma rate is written over it (:1276-1283);
 *   - merge_flag: skipModeFacBits[ctx][1] replaces the rate when it is strictly below it, in the SAD (:1310-1315) and the SSD branch
 *     (:1288-1293); d_rate keeps the unreplaced values;
 *   - the single-reference bits read ref_frame_type itself, the compound ones rf[] (:830-941); the single candidate's MV list is
 *     "pred_direction == 0 ? 0 : 1" (:1175); the mode context of a candidate whose rf[1] is a frame goes through
 *     compound_mode_ctx_map_2 whatever is_compound says (:960);
 *   - has_uv enters no number: the reference reads it only to print a warning (:1301).  The chroma distortions are added when given;
 *   - the :458-469 pass is no stable partition: for position i it swaps with the first later inter entry only while entry i is
 *     intra, so [A, B, c] (capitals intra) becomes [c, B, A].  Inter entries keep their order (DESIGN.md 4.34 has the closed form);
 *   - ref_fast_cost and the sorted array keep the by-buffer-index quirks stated for svt_hip_fast_pick_frame.
 * Context bytes are device data and are clamped before they index (skip ctx to 2, is_inter_ctx to 3, reference_mode_context and
 * compoud_reference_type_context to 4, the reference contexts to 2, newmv ctx to 5, refmv ctx to 5, the compound context to 7,
 * pred_mode to 13 .. 24, ref_frame_type to 1 .. 28, drl contexts to 2, motion_mode to its table, MV differences to +-16383): an
 * out-of-range byte gives an unspecified cost for its block and nothing else.  Costs at or above MAX_CU_COST are outside the domain,
 * as for the intra pick.  Only the block index and the winners' list positions address memory from device data.
 * Outputs, n = min(nfl, ninter + nintra), [nblocks][n] unless stated: d_cand (index into the combined list; >= ninter: intra), d_sorted
 * (slots), d_cost, d_rate [..][2], d_ref_fast_cost [nblocks], optional d_all_cost [nblocks][ninter] (the inter candidates' costs),
 * d_blk_out (the survivor's svt_hip_inter_blk; an intra slot gets the x / y of the block's first record, zero vectors, list 0,
 * filter 0, so a prediction call over the array stays inside that call's contract), optional d_cand_out (the survivor's
 * svt_hip_inter_cand, zeros in an intra slot), optional d_src_xy_out (x | y << 16 of the block's first record, repeated).
 * Validation, every group before the first launch (SVT_HIP_ERR_INVALID, nothing launched): metric; bsize / bsize_uv 0 .. 21; ninter
 * 1 .. 64, nintra 0 .. 63, their sum at most 64; nfl 1 .. 40; ac_dequant_q3 < 0; and for non-empty groups NULL d_blk / d_cand_in / d_ctx /
 * d_rates / d_mv_cost / d_dist / d_cand / d_sorted / d_cost / d_rate / d_ref_fast_cost / d_blk_out, d_intra_cost NULL with nintra > 0,
 * misalignment (the 8-byte arrays 8; d_blk, d_blk_out, d_cand_in, d_cand_out, d_ctx, d_rates, d_mv_cost, d_rate, d_intra_rate,
 * d_src_xy_out 4), nblocks * ncand above 2^31 - 1.  One launch per non-empty group; enqueue only, graph-capturable, nothing zeroed by the caller.
 *
 * svt_hip_inter_fast_search_frame: the one-call form, host composition on `stream`: (1) svt_hip_inter_pred_frame distortion-only over
 * the [nblocks][ninter] records on Y, and on Cb and Cr when use_chroma, into pick.d_dist* (d_scratch when NULL: per non-empty group
 * in group order Y, Cb, Cr, nblocks * ninter * 8 bytes each rounded up to 16; svt_hip_inter_fast_search_scratch_bytes, HOST, returns
 * the sum, 0 for bad parameters or nothing to carve); (2) the pick; (3) svt_hip_inter_pred_frame over pick.d_blk_out into the dense
 * d_pred_out[p] [nblocks][n][h][w] (p = 0 required; 1, 2 optional with use_chroma), what svt_hip_full_loop_group.d_pred reads; (4) with
 * d_intra_pred ([nblocks][nintra][H][W] luma samples of the call's depth) the intra survivors' luma slots are copied from it, ordered
 * after (3).  Without d_intra_pred an intra slot holds the benign record's prediction: the caller owns those slots.  The [nblocks]
 * [ninter][H][W] prediction array never exists.  bd 8 / 10 (the pick reads no samples); chroma follows svt_hip_inter_pred_frame's own
 * check.  Every stage is validated before the first launch; a scratch that is NULL, misaligned or too small is refused. */
typedef struct svt_hip_inter_cand {      /* sizeof 16: what only the cost reads of a candidate */
    int16_t pred_mv[2][2];               /* [list][0 = x, 1 = y]: motion_vector_pred_x / _y, the units of svt_hip_inter_blk.mv */
    int16_t mode_ctx;                    /* cu_ptr->inter_mode_ctx[ref_frame_type], raw */
    uint8_t pred_mode;                   /* PredictionMode: NEARESTMV 13 .. NEW_NEWMV 24 */
    uint8_t ref_frame_type;              /* 1 .. 28 */
    uint8_t drl_index;
    uint8_t ref_mv_count;                /* xd->ref_mv_count[ref_frame_type] */
    uint8_t drl_ctx;                     /* av1_drl_ctx(ref_mv_stack, idx) << 2 * idx, idx 0 .. 2 */
    uint8_t flags;                       /* merge_flag | motion_mode << 1 | motion_mode_allowed(...) << 3 (0 SIMPLE, 1 OBMC, 2 WARPED) */
} svt_hip_inter_cand;
typedef struct svt_hip_inter_fast_blk {  /* sizeof 16: the block's context bytes */
    uint8_t skip_flag_context, is_inter_ctx, reference_mode_context, compoud_reference_type_context;
    uint8_t comp_ref_p, comp_ref_p1, comp_ref_p2, comp_bwdref_p, comp_bwdref_p1;       /* av1_get_pred_context_* */
    uint8_t single_ref_p[6];             /* av1_get_pred_context_single_ref_p1 .. _p6 */
    uint8_t has_uv;
} svt_hip_inter_fast_blk;
typedef struct svt_hip_inter_fast_rates { /* the int32 tables of MdRateEstimationContext_s the inter fast cost reads */
    int32_t skipModeFacBits[3][3];
    int32_t newMvModeFacBits[6][3];
    int32_t zeroMvModeFacBits[2][3];
    int32_t refMvModeFacBits[6][3];
    int32_t drlModeFacBits[3][3];
    int32_t interCompoundModeFacBits[8][9];
    int32_t singleRefFacBits[3][6][3];
    int32_t compRefTypeFacBits[5][3];
    int32_t compRefFacBits[3][3][3];
    int32_t compBwdRefFacBits[3][2][3];
    int32_t compInterFacBits[5][3];
    int32_t motionModeFacBits[22][3];
    int32_t motionModeFacBits1[22][2];
    int32_t intraInterFacBits[4][2];
    int32_t nmv_vec_cost[4];
} svt_hip_inter_fast_rates;
#define SVT_HIP_MV_VALS 32767            /* MV_VALS; the centre entry is MV_MAX = 16383 */
typedef struct svt_hip_inter_fast_pick_group {
    int32_t bsize, bsize_uv;             /* AV1 block_size order, 0 .. 21 */
    uint32_t nblocks;
    int32_t ninter, nintra;              /* per block: ninter inter candidates, then nintra intra candidates */
    int32_t nfl;                         /* full_recon_search_count, 1 .. SVT_HIP_MAX_NFL */
    uint32_t lambda;                     /* fast_lambda (SAD) / full_lambda (SSD) */
    int16_t ac_dequant_q3;               /* y_dequant_Q3[qindex][1]; SSD only */
    int32_t reference_mode_select;       /* reference_mode == REFERENCE_MODE_SELECT */
    int32_t switchable_motion_mode;
    const svt_hip_inter_blk *d_blk;      /* [nblocks][ninter] */
    const svt_hip_inter_cand *d_cand_in; /* [nblocks][ninter] */
    const svt_hip_inter_fast_blk *d_ctx; /* [nblocks] */
    const svt_hip_inter_fast_rates *d_rates;
    const int32_t *d_mv_cost;            /* [2][SVT_HIP_MV_VALS]: nmv_costs or nmv_costs_hp, whichever nmvcoststack points into */
    const uint64_t *d_dist, *d_dist_cb, *d_dist_cr;                     /* [nblocks][ninter]; cb / cr optional */
    const uint64_t *d_intra_cost;        /* [nblocks][nintra]; required when nintra > 0 */
    const uint32_t *d_intra_rate;        /* optional [nblocks][nintra][2]; NULL: read as 0 */
    uint8_t *d_cand, *d_sorted;          /* [nblocks][n] */
    uint64_t *d_cost;                    /* [nblocks][n] */
    uint32_t *d_rate;                    /* [nblocks][n][2] */
    uint64_t *d_ref_fast_cost;           /* [nblocks] */
    uint64_t *d_all_cost;                /* optional [nblocks][ninter] */
    svt_hip_inter_blk *d_blk_out;        /* [nblocks][n] */
    svt_hip_inter_cand *d_cand_out;      /* optional [nblocks][n] */
    uint32_t *d_src_xy_out;              /* optional [nblocks][n] */
} svt_hip_inter_fast_pick_group;
int svt_hip_inter_fast_pick_frame(const svt_hip_inter_fast_pick_group *groups, int ngroups, int metric, void *stream);

typedef struct svt_hip_inter_fast_search_group {
    svt_hip_inter_fast_pick_group pick;  /* d_dist* may be NULL: scratch */
    int32_t bwidth, bheight;             /* LUMA block size, as svt_hip_inter_pred_group */
    int32_t use_chroma;                  /* non-zero: Cb and Cr distortions and (optionally) predictions */
    const void *d_ref[2][3];             /* [list][Y, Cb, Cr], as svt_hip_inter_pred_group.d_ref */
    uint32_t ref_stride[3];
    const void *d_src[3];                /* source planes, sample (0, 0) of the picture */
    uint32_t src_stride[3];
    void *d_pred_out[3];                 /* dense [nblocks][n][h][w] per plane; [0] required, [1] / [2] optional with use_chroma */
    const void *d_intra_pred;            /* optional [nblocks][nintra][H][W] luma */
} svt_hip_inter_fast_search_group;
size_t svt_hip_inter_fast_search_scratch_bytes(const svt_hip_inter_fast_search_group *groups, int ngroups);   /* HOST */
int svt_hip_inter_fast_search_frame(const svt_hip_inter_fast_search_group *groups, int ngroups, uint32_t pic_width, uint32_t pic_height,
                                    int bd, int metric, void *d_scratch, size_t scratch_bytes, void *stream);

/* The join of mode decision: the rest of AV1PerformFullLoop (EbProductCodingLoop.c:1877-2184) after the survivors' transform search,
 * and product_full_mode_decision (EbModeDecision.c:2653-2690): every survivor's full cost, the full loop's early exit and the best
 * candidate of every block, with the winner's prediction, coefficients and inter record gathered, for many groups in one launch.
 * A group is nblocks blocks of one block size, each with n full-loop slots in best_candidate_index_array order, which is what
 * svt_hip_fast_pick_frame / svt_hip_inter_fast_pick_frame write (n = min(nfl, ncand)).  Per (block, slot), in uint64 arithmetic
 * that wraps as the reference's does, RDCOST(R, D) = ((R * lambda + 256) >> 9) + D * 128 (EbRateDistortionCost.h:73):
 *   inputs    luma: d_luma's dist[2], bits, eob, has_coeff, tx_type (its cost is not read).  Cb, Cr: the given dist / bits / eob of
 *             svt_hip_full_loop_frame with ntypes 1 and svt_hip_coeff_rate_frame (FullLoop_R + CuFullDistortionFastTuMode_R,
 *             EbFullLoop.c:1529-1873), used when the arrays are given AND the block's has_uv is set, else zero distortion, bits and
 *             eob.  u_has_coeff / v_has_coeff are eob != 0 (av1_tu_calc_cost, EbRateDistortionCost.c:2103-2110), block_has_coeff the
 *             OR of the three.  A slot is intra iff d_cand >= ninter, its intra_luma_mode / pred_mode modes[d_cand - ninter].
 *   cost      Av1FullCost (EbRateDistortionCost.c:1456-1534): rate = fast_luma_rate + chroma rate + the three planes' bits, chroma
 *             rate = fast_chroma_rate and, for an intra slot of a has_uv block whose d_cfl record says UV_CFL_PRED (:1493-1506),
 *             + (cflAlphaFacBits[signs][0][idx >> 4] + cflAlphaFacBits[signs][1][idx & 15], summed as int32) + intraUVmodeFacBits
 *             [isCflAllowed][mode][UV_CFL_PRED] - intraUVmodeFacBits[isCflAllowed][mode][UV_DC_PRED], the -= on the uint64 as written;
 *             full_cost = RDCOST(rate, D), D = the three planes' dist[DIST_CALC_RESIDUAL]; full_lambda_rate = full_cost - D (D, not
 *             D * 128: as written, :1529); full_cost_luma = RDCOST(fast_luma_rate + luma bits, luma dist).
 *             Av1MergeSkipFullCost (:1551-1692) for an inter slot whose d_cand_out flags & 1 (merge_flag; av1_inter_full_cost,
 *             :1761-1811): merge_cost = RDCOST(fast_luma_rate + fast_chroma_rate + bits, D), skip_cost = RDCOST(skipModeFacBits
 *             [skip_flag_context][1], the three planes' dist[DIST_CALC_PREDICTION]); skip_cost <= merge_cost picks skip (a tie is skip);
 *             full_lambda_rate = the picked cost - the picked side's distortion.
 *   escape    on a non-I slice, walking the slots in order, slot k ends the loop when (intra || full_loop_escape == 2) &&
 *             best_inter_luma_zero_coeff == 0 (:1935-1941); that variable starts at 1 and, only with full_loop_escape != 0, becomes
 *             the y_has_coeff of an inter slot whose full cost is strictly below bestfullCost, which starts at 0xFFFFFFFF: 32 bits,
 *             so an inter cost of 2^32 - 1 or more never updates it (:1909, :2170-2181; a quirk, kept).  count = k, at least 1.
 *   decision  over the first count slots: the first strict minimum of the full cost from UINT64_MAX (slot 0 when no cost is below
 *             it: lowestCostIndex starts at best_candidate_index_array[0], :2674); best_intra_mode = the pred_mode of the first
 *             strict minimum among the intra slots, 0xFF when none was evaluated (the reference leaves its caller's value).
 * The decision's uv_mode / cfl_alpha_idx / cfl_alpha_signs are the winner's d_cfl record's when it is an intra slot of a has_uv
 * block and d_cfl is given, else 0: a candidate's own uv mode stays with the caller.  cost_luma is 0 for a merge winner (its cost
 * function does not set it); merge_cost / skip_cost are 0 unless the winner is a merge slot.
 * d_full_cost, when given, receives every slot's cost, those at or past the escape included (count says which were evaluated).
 * Gathers of the winner, each needing its input: d_best_pred[p] from the dense 8-bit [nblocks][n][h][w] d_pred[p] (p = 0 luma bw x
 * bh, 1 / 2 chroma max(bw / 2, 4) x max(bh / 2, 4)); d_best_qcoeff[p] / d_best_dqcoeff[p] from [nblocks][n][NC_p], NC_p = min(w, 32) *
 * min(h, 32) of the plane; d_best_inter_blk from d_inter_blk [nblocks][n].  A plane whose winner has eob 0 stores zero coefficients and
 * its input is not read.  Only the block index and the winner's slot, below n by construction, address memory from device data.
 * Context bytes are device data and clamped (skip ctx to 2, CfL signs to 7, the idx nibbles to 15 by construction, the list index
 * to 63, an intra mode to 12): an out-of-range byte gives an unspecified cost for its block and nothing else.
 * One transform block per plane is assumed: bsize 13, 14, 15 (128 wide or high, txb_count 2 or 4, EbUtility.c:861) are refused.
 * Validation, every group (empty ones' scalars included) before the first launch (SVT_HIP_ERR_INVALID): bsize outside 0 .. 21 or
 * 13 .. 15; n outside 1 .. 40; ninter < 0, nintra < 0, ninter + nintra outside 1 .. 64; an intra mode above 12; full_loop_escape
 * outside 0 .. 2; and for non-empty groups nblocks * n above 2^31 - 1; NULL d_luma / d_rate / d_cand / d_blk / d_rates / d_decision;
 * NULL d_cand_out with ninter > 0; some but not all of the six chroma arrays; a gather without its input or equal to it;
 * misalignment (records and uint64 arrays 8 bytes, d_inter_blk / d_best_inter_blk and the prediction and coefficient arrays 16,
 * d_rate / d_rates / d_blk / d_cand_out 4, the eobs 2).  One launch per 10 groups; the call only enqueues, allocates nothing and can be captured
 * into a HIP graph. */
typedef struct svt_hip_md_blk { uint8_t skip_flag_context, has_uv, pad[2]; } svt_hip_md_blk;     /* sizeof 4 */
typedef struct svt_hip_md_rates {         /* the int32 tables of MdRateEstimationContext_s the full cost reads, its declaration shapes */
    int32_t skipModeFacBits[3][3];
    int32_t intraUVmodeFacBits[2][13][15];
    int32_t cflAlphaFacBits[8][2][16];
} svt_hip_md_rates;
typedef struct svt_hip_md_decision {      /* one per block; sizeof 72, 8-byte aligned */
    uint64_t cost;                        /* the winner's full cost */
    uint64_t cost_luma;                   /* its full_cost_luma (0: merge winner) */
    uint64_t merge_cost, skip_cost;       /* full_cost_merge / full_cost_skip (0: the winner is no merge slot) */
    uint64_t full_lambda_rate;
    uint32_t full_distortion;             /* (uint32_t)luma dist[DIST_CALC_RESIDUAL], :2144 */
    uint16_t eob[3];                      /* Y, Cb, Cr */
    uint8_t  slot;                        /* the winner's full-loop slot, below count */
    uint8_t  cand;                        /* its d_cand entry: the index into the candidate list */
    uint8_t  count;                       /* the effective full_recon_search_count, 1 .. n */
    uint8_t  is_intra, skip_flag, merge_flag;
    uint8_t  y_has_coeff, u_has_coeff, v_has_coeff, block_has_coeff;
    uint8_t  tx_type;                     /* the luma record's */
    uint8_t  best_intra_mode;             /* 0xFF: no intra slot evaluated */
    uint8_t  uv_mode, cfl_alpha_idx, cfl_alpha_signs;
    uint8_t  pad[7];                      /* written as 0 */
} svt_hip_md_decision;
#define SVT_HIP_MD_NO_INTRA 0xFF
typedef struct svt_hip_md_decide_group {
    int32_t bsize;                        /* AV1 block_size order, 0 .. 21 without 13 .. 15; isCflAllowed = bw <= 32 && bh <= 32 */
    uint32_t nblocks;
    int32_t n;                            /* slots per block, 1 .. SVT_HIP_MAX_NFL */
    int32_t ninter, nintra;               /* of the candidate list d_cand indexes */
    uint32_t lambda;                      /* full_lambda */
    int32_t slice_is_intra;               /* slice_type == I_SLICE: no escape */
    int32_t full_loop_escape;             /* 0, 1, 2 */
    uint8_t modes[64];                    /* the intra list, as the pick groups carry it; [0 .. nintra) read */
    const svt_hip_tx_decision *d_luma;    /* [nblocks][n] */
    const uint64_t *d_dist_cb, *d_dist_cr;   /* optional [nblocks][n][2]; the six chroma arrays all or none */
    const uint64_t *d_bits_cb, *d_bits_cr;   /* [nblocks][n] */
    const uint16_t *d_eob_cb, *d_eob_cr;     /* [nblocks][n] */
    const uint32_t *d_rate;               /* [nblocks][n][2]: fast_luma_rate, fast_chroma_rate */
    const uint8_t *d_cand;                /* [nblocks][n] */
    const svt_hip_inter_cand *d_cand_out; /* [nblocks][n]; required when ninter > 0 */
    const svt_hip_cfl_decision *d_cfl;    /* optional [nblocks][n] */
    const svt_hip_md_blk *d_blk;          /* [nblocks] */
    const svt_hip_md_rates *d_rates;
    svt_hip_md_decision *d_decision;      /* [nblocks] */
    uint64_t *d_full_cost;                /* optional [nblocks][n] */
    const uint8_t *d_pred[3]; uint8_t *d_best_pred[3];                 /* optional gathers, see above */
    const int32_t *d_qcoeff[3], *d_dqcoeff[3]; int32_t *d_best_qcoeff[3], *d_best_dqcoeff[3];
    const svt_hip_inter_blk *d_inter_blk; svt_hip_inter_blk *d_best_inter_blk;
} svt_hip_md_decide_group;
int svt_hip_md_decide_frame(const svt_hip_md_decide_group *groups, int ngroups, void *stream);

/* The one-call form, host composition on `stream`, whose order carries the dependencies (no kernel of its own, as
 * svt_hip_tx_search_frame): (1) svt_hip_tx_search_frame over the nblocks * n luma survivor predictions (group `luma`, whose
 * fl.nblocks must be md.nblocks * md.n); (2) with use_chroma, svt_hip_full_loop_frame over `cb` and `cr` (ntypes 1:
 * transform_type[PLANE_TYPE_UV] at txsize_uv; nblocks as luma's) and svt_hip_coeff_rate_frame on them with the PLANE_TYPE_UV tables;
 * (3) the decide.  Both chroma planes are quantised with q_chroma: FullLoop_R indexes both planes' rows with cbQp (EbFullLoop.c:1625,
 * :1686), and the Cr rows equal the Cb rows in a picture without chroma delta q, the only kind this reference makes.
 * The stages' outputs are the decide's inputs: md.d_luma, the six chroma arrays, d_qcoeff[] and d_dqcoeff[] are SET BY THE CALL from
 * luma.d_decision / d_best_qcoeff / d_best_dqcoeff, cb / cr .d_dist / d_eob / d_qcoeff / d_dqcoeff and d_bits_c[]; what the caller put
 * into those members of md is ignored.  Any of these stage arrays may be NULL and then lives in d_scratch (the luma record and the
 * chroma dist / eob / bits / qcoeff always; luma's best_qcoeff / best_dqcoeff and chroma's dqcoeff only when the matching md.d_best_*
 * asks for them).  Carved per non-empty group in group order, every piece rounded up to 16 bytes: the luma record, luma best_qcoeff,
 * luma best_dqcoeff, then per plane Cb, Cr: dist, eob, bits, qcoeff, dqcoeff; after all groups the luma search's own scratch
 * (svt_hip_tx_search_scratch_bytes of the luma groups).  svt_hip_md_search_scratch_bytes returns the sum, a HOST computation that
 * needs no device: 0 for bad parameters and for a call without a non-empty group.
 * A luma type list without DCT_DCT is refused: a no-candidate record (type_index 0xFF) then cannot occur.  Every stage's arguments
 * are validated before the first launch (SVT_HIP_ERR_INVALID, as the stages' own calls; also luma / cb / cr nblocks other than
 * md.nblocks * md.n, a chroma ntypes other than 1, a scratch that is NULL, not 16-byte aligned or too small). */
typedef struct svt_hip_md_search_group {
    svt_hip_md_decide_group md;
    svt_hip_tx_search_group luma;
    int32_t use_chroma;
    svt_hip_full_loop_group cb, cr;
    const uint8_t *d_txb_skip_ctx_c[2], *d_dc_sign_ctx_c[2];     /* [nblocks * n] per plane, as svt_hip_coeff_rate_group */
    const int32_t *d_coeff_cost_uv, *d_eob_cost_uv;              /* the PLANE_TYPE_UV tables */
    uint64_t *d_bits_c[2];                                       /* optional [nblocks][n]: scratch when NULL */
} svt_hip_md_search_group;
size_t svt_hip_md_search_scratch_bytes(const svt_hip_md_search_group *groups, int ngroups);     /* HOST; 0: bad parameters or nothing to carve */
int svt_hip_md_search_frame(const svt_hip_md_search_group *groups, int ngroups, int flavour, const svt_hip_qrows *q_luma,
                            const svt_hip_qrows *q_chroma, void *d_scratch, size_t scratch_bytes, void *stream);

/* The partition decision of a picture: the d1 (shape) and d2 (depth) decisions that mode_decision_sb (EbProductCodingLoop.c:3375-3502)
 * makes around md_encode_block, and the block list the encode pass derives from them (EbCodingLoop.c:2571-2589, :3618-3621), for nsb
 * 64x64 superblocks in one launch.  It consumes the cost svt_hip_md_decide_frame stores first in its record (md_local_cu_unit[].cost).
 * A superblock has 1 101 blocks in md-scan order (mds) under 341 squares (EbUtility.c:782-917, build_blk_geom(0)); svt_hip_blk_geom_mds
 * gives a block's geometry on the host.  Per superblock, in uint64 arithmetic that wraps, RDCOST as at the decide above:
 *   start     Initialize_cu_data_structure (:651-683): every square split_flag 1, part PARTITION_SPLIT (3), not tested; and, defined
 *             HERE where the reference reads stale memory, cost 0, contexts 0, mdc_split_flag 0, best_d1_blk 0 for what no entry sets.
 *   entries   the MDC leaf list in order.  An entry gives its block its cost (d_cost[src] or d_decision[src].cost); a PART_N entry
 *             also makes its square tested and sets split_flag = mdc_split_flag = the entry's split_flag & 1 (a one-bit member) and
 *             the square's partition contexts.  d1_blocks_accumlated restarts at 1 on a PART_N entry and counts up on others.
 *   d1        d1_non_square_block_decision (EbFullLoop.c:1876-1898), at every entry that is the last block of its shape: the sum of
 *             the shape's blocks (an absent one counts 0); PART_N always takes the square, another shape only when strictly cheaper
 *             than the square's cost so far; part = NONE, HORZ, VERT, HORZ_A, HORZ_B, VERT_A, VERT_B, HORZ_4, VERT_4 (0, 1, 2, 4 .. 9),
 *             best_d1_blk = the shape's first block.
 *   d2        d2_inter_depth_block_decision (:2037-2103), at the entry whose count equals its tot_d1_blocks, when the square's
 *             split_flag is 0: climbs while the square is a last quadrant.  At each parent compute_depth_costs (:1902-2035): the parent
 *             takes child 0's contexts; parent cost = its cost + its PARTITION_NONE rate, MAX_MODE_COST (108 935 755 917 824) when it is
 *             not tested; current cost = the four children's costs + the parent's PARTITION_SPLIT rate + the PARTITION_NONE rate of
 *             every child with mdc_split_flag 0, these child rates NOT added in a climb that began at a 4x4 square (the reference tests
 *             the last leaf's block size).  parent <= current keeps the parent (split_flag 0, cost = parent cost); else part =
 *             PARTITION_SPLIT and cost = current.  On an I slice the 64x64 root is not computed: parent cost is MAX_MODE_COST, current
 *             keeps the value of the climb's previous level (0 when the climb begins at a 32x32).
 *   rate      av1_split_flag_rate (EbRateDistortionCost.c:2268-2342), as written: with the square's bottom and right halves inside
 *             the picture partitionFacBits[partition_cdf_length(bsize)][type] (row 4 for 8x8, row 10 above: the row is the LENGTH, not
 *             the context); on a picture edge 0 for PARTITION_SPLIT, else the row [left * 2 + above + 4 bsl] of BITS read as a CDF by
 *             partition_gather_vert_alike (bottom half outside only) or _horz_alike, an int32 converted to uint64; then
 *             RDCOST(rate, 0).  bsl = log2(size / 8), left / above = (context >> bsl) & 1, a context of -1 (INVALID_NEIGHBOR_DATA) is 0.
 *   final     the squares in mds order: a square all of whose ancestors have part 3 and whose own part is not 3 emits the blocks of
 *             its part (ns_blk_num[part] from ns_blk_offset[part]); d_final[sb][k] is the k-th of the superblock in coding order, with
 *             its picture position, block size, the square's part and the src of its entry (SVT_HIP_PART_NO_SRC for a block no entry
 *             listed); d_final_decision, when given, receives d_decision[src] (zeros for no entry).  At most 256 per superblock.
 * The level-by-level form the kernel uses equals the sequential loop for a list as MDC makes it: ascending mds_idx without repeats, a
 * square's entries carrying the count of its listed blocks as tot_d1_blocks, and no entry below a square listed with split_flag 0.
 * Another list gives an unspecified tree for its own superblock.  The partition contexts are the caller's (what md_encode_block stores
 * from the neighbour arrays); deriving them across blocks and superblocks stays with the caller.
 * Device data is clamped: mds_idx to 1 100, src to nsrc - 1, a leaf range to nleaves and to 1 101 entries; no address outside the
 * arrays is formed.  Entries of d_final / d_final_decision at or past d_final_count[sb] are not written; every d_sq entry and count is.
 * Records: svt_hip_part_leaf, svt_hip_part_sb and svt_hip_part_final are 12 bytes, 4-byte aligned; svt_hip_part_sq is 16 bytes, 8-byte
 * aligned.  Validation before the launch (SVT_HIP_ERR_INVALID): nsb 0 or above 2^31 / 341 (6 297 606); zero pic_width / pic_height; NULL
 * d_sb / d_partition_bits / d_sq / d_final_count / d_final; NULL d_leaf or nsrc 0 with nleaves > 0; both or neither of d_decision /
 * d_cost; d_final_decision without d_decision; misalignment (d_decision / d_cost / d_sq / d_final_decision 8 bytes, the others 4).
 * 128-wide superblocks are not supported.  One launch, one wave per superblock; the call only enqueues, allocates nothing and can be
 * captured into a HIP graph. */
typedef struct svt_hip_blk_geom {         /* BlockGeom's members a caller needs to build lists and groups; sizeof 16 */
    uint16_t sqi_mds;                     /* the block's square, in md scan */
    uint8_t bsize, shape;                 /* AV1 block_size; PART_N, H, V, HA, HB, VA, VB, H4, V4 = 0 .. 8 */
    uint8_t depth, nsi, totns, d1i;
    uint8_t origin_x, origin_y, bwidth, bheight, sq_size;
    uint8_t is_last_quadrant, has_uv, pad;
} svt_hip_blk_geom;
#define SVT_HIP_SB_BLOCKS 1101
#define SVT_HIP_SB_SQUARES 341
#define SVT_HIP_SB_MAX_FINAL 256
#define SVT_HIP_PART_NO_SRC 0xFFFFFFFFu
int svt_hip_blk_geom_mds(uint32_t mds_idx, svt_hip_blk_geom *out);      /* HOST; 64x64 superblock, 0 .. 1100; needs no device */
typedef struct svt_hip_part_leaf {        /* one MDC leaf (EbMdcLeafData_t) */
    uint16_t mds_idx;
    uint8_t split_flag, tot_d1_blocks;
    int8_t left_partition, above_partition;      /* read on PART_N entries */
    uint8_t pad[2];
    uint32_t src;                         /* index of this block's cost: into d_decision or d_cost */
} svt_hip_part_leaf;
typedef struct svt_hip_part_sb {
    uint32_t leaf_first;                  /* the superblock's entries: d_leaf[leaf_first .. leaf_first + leaf_count) */
    uint16_t leaf_count;
    uint16_t origin_x, origin_y;          /* in the picture */
    uint16_t pad;
} svt_hip_part_sb;
typedef struct svt_hip_part_sq {          /* one square after the decisions */
    uint64_t cost;
    uint16_t best_d1_blk;
    uint8_t part, split_flag, tested;
    uint8_t pad[3];                       /* written as 0 */
} svt_hip_part_sq;
typedef struct svt_hip_part_final {       /* one block the encode pass codes */
    uint16_t mds_idx, x, y;               /* x, y in the picture */
    uint8_t bsize, part;
    uint32_t src;
} svt_hip_part_final;
typedef struct svt_hip_partition_args {
    uint32_t nsb, nleaves, nsrc;
    uint32_t lambda;                      /* full_lambda */
    uint32_t pic_width, pic_height;       /* luma_width / luma_height */
    int32_t slice_is_intra;               /* slice_type == I_SLICE */
    int32_t pad;
    const svt_hip_part_sb *d_sb;          /* [nsb] */
    const svt_hip_part_leaf *d_leaf;      /* [nleaves] */
    const svt_hip_md_decision *d_decision;       /* exactly one of d_decision / d_cost: [nsrc] */
    const uint64_t *d_cost;
    const int32_t *d_partition_bits;      /* partitionFacBits in its declaration shape [20][11] */
    svt_hip_part_sq *d_sq;                /* [nsb][341], squares in mds order */
    uint32_t *d_final_count;              /* [nsb] */
    svt_hip_part_final *d_final;          /* [nsb][256], coding order */
    svt_hip_md_decision *d_final_decision;       /* optional [nsb][256]; needs d_decision */
} svt_hip_partition_args;
int svt_hip_partition_decide_frame(const svt_hip_partition_args *a, void *stream);

/* The reconstruction of the final block list: AV1PerformInverseTransformRecon for the winner (EbProductCodingLoop.c:871-1020, called at
 * :3205) over every block svt_hip_partition_decide_frame listed, 8-bit 4:2:0, into picture planes.  It takes d_final / d_final_count as
 * that call writes them, the records and the winners' arrays as svt_hip_md_decide_frame gathers them, and learns on the device how many
 * blocks of which size there are: no copy to the host, no synchronisation, no allocation; grid sizes come from nsb alone.
 * A source group is one md-decide group: the records src_first .. src_first + nblocks - 1, all of block size bsize, with d_best_pred[p]
 * dense [nblocks][h][w] (p = 0 luma bw x bh, 1 / 2 chroma max(bw / 2, 4) x max(bh / 2, 4)) and d_best_dqcoeff[p] / d_best_qcoeff[p]
 * [nblocks][min(w, 32) * min(h, 32)].  The groups are ascending, disjoint and cover [0, nsrc).  tx_type_uv is the chroma transform
 * type of the group (transform_type[PLANE_TYPE_UV], one scalar as in svt_hip_md_search_frame); the luma type is the record's tx_type.
 * Per final entry k < d_final_count[sb] (a count above 256 is taken as 256), with src its record:
 *   sizes     one transform block per plane: luma blk_geom->txsize[0] (the block size's own), chroma txsize_uv[0] (of the chroma block, a
 *             64-sample side taken as 32).  Chroma is written only when the geometry of mds_idx (clamped to 1 100) has has_uv.
 *   where     luma at (x, y); chroma at (((x >> 3) << 3) >> 1, ((y >> 3) << 3) >> 1) (:905-906).
 *   content   a plane whose record eob[p] is 0 receives the prediction (picture_copy8_bit) and its coefficients are not read; otherwise
 *             prediction + inverse transform of d_best_dqcoeff (bd 8) clipped: av1_inv_transform_recon8bit = av1_inv_txfm_add_c, bit for bit.
 *   skipped   nothing is written for an entry, and d_status says why, when (1, SVT_HIP_RECON_NO_SRC) src is SVT_HIP_PART_NO_SRC or
 *             >= nsrc; (2, _BSIZE) its bsize differs from its source group's; (3, _OUTSIDE) a plane block of it does not lie wholly inside
 *             that plane's width x height (the chroma planes are tested in a three-plane call only); (4, _TX_TYPE) the record's tx_type is
 *             not defined for the luma size (a 64-sample side: DCT_DCT; a 32-sample side: DCT_DCT, IDTX; else 0 .. 15).  The first
 *             that applies is reported.
 *   status    d_status (optional, uint8 [nsb][256]) receives 0 or the reason for every entry below the count; entries at or past the
 *             count are not written.  Samples no final block covers are not written.
 *   stream    the superblock coefficient stream of the entropy coder (coded_area_sb / coded_area_sb_uv, EbCodingLoop.c:3033-3035,
 *             :3376-3378): running offsets per superblock in coding order, luma advancing by bw * bh of every reconstructed entry, chroma by
 *             the chroma block's w * h of those with has_uv; skipped entries advance nothing.  d_coeff_offset (optional, uint32
 *             [nsb][256][2]) receives the luma and chroma offset of every entry below the count (a skipped entry: the running values).
 *             d_sb_qcoeff[p] (optional; with planes 3 all three or none; int32 [nsb][4096] luma, [nsb][1024] per chroma plane) receives at
 *             the entry's offset its min(w, 32) * min(h, 32) packed d_best_qcoeff[p], zeros for a plane with eob 0; the rest of a 64-wide
 *             span is not written.  An entry whose span would pass its superblock's 4096 / 1024 (a list that is no tiling) gets no copy.
 * Everything from device memory is clamped or checked before it forms an address.  Overlapping entries (a list that is no tiling) are
 * each reconstructed in an unspecified order, and a superblock that lists more plane blocks of one size than a tiling can hold may lose
 * some of them; nothing outside the arrays is touched.
 * Validation before anything is enqueued (SVT_HIP_ERR_INVALID): nsb 0 or above 2^20; nsrc 0; planes other than 1 / 3; NULL d_final /
 * d_final_count / d_decision / groups; ngroups outside 1 .. 32; a group table that is not ascending and contiguous from 0 to nsrc; a
 * bsize outside 0 .. 21 or 13 .. 15; a tx_type_uv the chroma size does not define; a requested plane without its d_recon, or with a stride
 * below its width, a width or height above 65 535, or, in a non-empty group, without d_best_pred / d_best_dqcoeff (d_best_qcoeff when the
 * stream is asked for); some but not all of the requested planes' d_sb_qcoeff; misalignment (prediction, coefficient and stream arrays
 * and the scratch 16 bytes, d_decision 8, d_final / d_final_count / d_coeff_offset 4); a scratch that is NULL or smaller than
 * svt_hip_recon_final_scratch_bytes(nsb), a HOST computation that needs no device (0 for an nsb the call refuses).
 * Six launches on `stream` (the lists' counters cleared, the bin stage, then the reconstruction by register class, the class of the 32-
 * and 64-sample sides in two halves); the call only enqueues, allocates nothing and can be captured into a HIP graph. */
#define SVT_HIP_RECON_FINAL_MAX_GROUPS 32
#define SVT_HIP_RECON_OK 0
#define SVT_HIP_RECON_NO_SRC 1
#define SVT_HIP_RECON_BSIZE 2
#define SVT_HIP_RECON_OUTSIDE 3
#define SVT_HIP_RECON_TX_TYPE 4
#define SVT_HIP_SB_QCOEFF_LUMA 4096       /* int32 per superblock of d_sb_qcoeff[0]; [1], [2]: a quarter */
typedef struct svt_hip_recon_final_group {
    uint32_t src_first, nblocks;
    int32_t bsize;                        /* 0 .. 21 without 13 .. 15 */
    int32_t tx_type_uv;
    const uint8_t *d_best_pred[3];
    const int32_t *d_best_dqcoeff[3];
    const int32_t *d_best_qcoeff[3];      /* read only with d_sb_qcoeff */
} svt_hip_recon_final_group;
typedef struct svt_hip_recon_final_args {
    uint32_t nsb, nsrc;
    int32_t ngroups;
    int32_t planes;                       /* 1: luma only; 3: Y, Cb, Cr */
    const svt_hip_part_final *d_final;    /* [nsb][256] */
    const uint32_t *d_final_count;        /* [nsb] */
    const svt_hip_md_decision *d_decision;       /* [nsrc] */
    const svt_hip_recon_final_group *groups;     /* HOST array [ngroups] */
    uint8_t *d_recon[3];
    uint32_t stride[3], width[3], height[3];     /* samples; width x height: what is allocated of the plane */
    uint8_t *d_status;                    /* optional [nsb][256] */
    int32_t *d_sb_qcoeff[3];              /* optional */
    uint32_t *d_coeff_offset;             /* optional [nsb][256][2] */
    void *d_scratch;
    size_t scratch_bytes;
} svt_hip_recon_final_args;
size_t svt_hip_recon_final_scratch_bytes(uint32_t nsb);      /* HOST */
int svt_hip_recon_final_frame(const svt_hip_recon_final_args *a, void *stream);

/* The intra encode pass in coding order: what the encode pass does with every intra block of the final list (EbCodingLoop.c:2853-3005
 * with Av1EncodeLoop :545-980 and Av1EncodeGenerateRecon :1408-1500), 8-bit 4:2:0, 64x64 superblocks, one transform block per plane.
 * Every intra entry is PREDICTED AGAIN from the reconstructed picture (av1_predict_intra_block at ED_STAGE, EbIntraPrediction.c:4078-4333),
 * then residual -> forward transform -> quantiser -> eob -> inverse transform -> reconstruction, in place in d_recon.  Inter blocks
 * depend on nothing inside the picture: the caller reconstructs them first (svt_hip_recon_final_frame or the encode calls), this call
 * codes the intra entries around them, which equals the reference's single walk.
 * Inputs: d_final / d_final_count of npics pictures of sb_cols x sb_rows superblocks in raster order (picture i at superblock
 * i * sb_pitch of every per-superblock array; sb_pitch 0 means nsb = sb_cols * sb_rows); d_blk, one svt_hip_intra_enc_blk per src
 * (picture i at element i * blk_pitch; 0: one table for all pictures); the source planes (read only) and the reconstruction planes
 * (read and written; on entry whatever the caller has reconstructed), picture i at sample i * src_pic_pitch[p] / recon_pic_pitch[p];
 * one set of quantiser rows for luma and one for chroma (HOST); the inverse scans of every (transform size, type) in one device blob the
 * caller builds once with svt_hip_intra_encode_tables_bytes / _fill and uploads.
 * Per entry k < count (a count above 256 is taken as 256) of a superblock, in coding order:
 *   geometry  of mds_idx (clamped to 1 100) as svt_hip_recon_final_frame: block size, has_uv; luma at (x, y), chroma at
 *             (((x >> 3) << 3) >> 1, ((y >> 3) << 3) >> 1), the chroma size txsize_uv with a 64-sample side taken as 32.
 *   not coded the first that applies is reported in d_status: (1, _NO_SRC) and (3, _OUTSIDE) as svt_hip_recon_final_frame; (4, _TX_TYPE)
 *             tx_type not defined for the luma size or, with has_uv, tx_type_uv for the chroma size; (5, _NOT_INTRA) is_intra 0: the
 *             samples stay, no error; (6, _MODE) mode > 12, uv_mode > 13, angle_delta outside -3 .. 3 or not 0 on a non-directional mode;
 *             (7, _CFL_SIZE) uv_mode 13 on a block wider or taller than 32 or narrower or lower than 8; (8, _SCHEDULE) the launch schedule
 *             did not reach the entry, which happens only for a list that is no partition tree.  The stream offsets advance for coded and
 *             for _NOT_INTRA entries alike and for no other, so they equal svt_hip_recon_final_frame's for the same list.
 *   predicted every plane the block has, from the neighbour row and column of the reconstruction plane; the available sample counts follow
 *             svt_hip_intra_neighbor_px (one tile, 8-bit; mi_cols / mi_rows from the luma width / height; the partition is the entry's
 *             part); filt_type from the above and left blocks' modes (get_filt_type / is_smooth; a block this call does not code counts
 *             as not smooth); the chroma mode is UV_DC_PRED when uv_mode is 13; disable_edge_filter 0; angle_delta applies to luma only.
 *             Samples the availability rules exclude are not read.
 *   coded     luma with tx_type and the luma rows; with uv_mode 13 cfl_luma_subsampling_420_lbd of the block's luma reconstruction,
 *             subtract_average and cfl_predict_lbd on the Cb and Cr DC predictions (cfl_idx_to_alpha); Cb and Cr with tx_type_uv and the
 *             chroma rows.  A plane with eob 0 keeps its prediction.
 * Outputs: the planes in place; d_result (optional) per coded entry the three eobs and the luma transform type, DCT_DCT when the luma eob
 * is 0 (:700-709); d_sb_qcoeff / d_coeff_offset (optional) with svt_hip_recon_final_frame's shapes and rules, filled for coded entries.
 * Entries at or past the count and samples no coded entry covers are not written.  Everything read from device memory is clamped or
 * checked before it forms an address; a list that is no tiling or breaks coding order gives unspecified samples for its own superblock
 * and its dependants, and nothing outside the arrays is touched.
 * Launch order carries the dependencies: no workgroup waits for another.  Superblock (r, c) is coded in step c + 2 r; a step is a fixed
 * schedule of launches by register class (intra_encode_plan.h), all pictures share them.  The call only enqueues, allocates nothing,
 * never synchronises and can be captured into a HIP graph.
 * Validation before anything is enqueued (SVT_HIP_ERR_INVALID): NULL arguments or required members; npics, sb_cols, sb_rows or nsrc 0; npics above 65 535; nsb
 * above 2^20; sb_pitch below nsb; a stride below its width; a width or height above 65 535 or no multiple of 8 (chroma: of 4, and half
 * the luma's); chroma planes (source and reconstruction) not all present or all absent (absent: luma only); some but not all stream
 * planes; misalignment (d_sb_qcoeff, d_tables and the scratch 16 bytes, d_result and d_blk 8, d_final / d_final_count / d_coeff_offset 4);
 * quantiser rows the one-product quantiser does not take; a scratch that is NULL or below svt_hip_intra_encode_scratch_bytes(npics, nsb),
 * a HOST computation (0 for parameters the call refuses); d_src[p] == d_recon[p]. */
#define SVT_HIP_INTRA_ENC_OK 0
#define SVT_HIP_INTRA_ENC_NO_SRC 1
#define SVT_HIP_INTRA_ENC_OUTSIDE 3
#define SVT_HIP_INTRA_ENC_TX_TYPE 4
#define SVT_HIP_INTRA_ENC_NOT_INTRA 5
#define SVT_HIP_INTRA_ENC_MODE 6
#define SVT_HIP_INTRA_ENC_CFL_SIZE 7
#define SVT_HIP_INTRA_ENC_SCHEDULE 8
typedef struct svt_hip_intra_enc_blk {
    uint8_t is_intra;
    uint8_t mode;                         /* 0 .. 12 */
    int8_t angle_delta;                   /* -3 .. 3, luma */
    uint8_t uv_mode;                      /* 0 .. 12, 13 = UV_CFL_PRED */
    uint8_t cfl_alpha_idx, cfl_alpha_signs;
    uint8_t tx_type, tx_type_uv;
} svt_hip_intra_enc_blk;
typedef struct svt_hip_intra_enc_result {
    uint16_t eob[3];
    uint8_t tx_type;                      /* the luma type, DCT_DCT when eob[0] is 0 */
    uint8_t pad;                          /* written as 0 */
} svt_hip_intra_enc_result;
typedef struct svt_hip_intra_encode_args {
    uint32_t npics, sb_cols, sb_rows;
    uint32_t sb_pitch;                    /* superblocks between pictures in the per-superblock arrays; 0: sb_cols * sb_rows */
    uint32_t nsrc, blk_pitch;
    const svt_hip_part_final *d_final;    /* [npics][sb_pitch][256] */
    const uint32_t *d_final_count;        /* [npics][sb_pitch] */
    const svt_hip_intra_enc_blk *d_blk;   /* [nsrc] */
    const uint8_t *d_src[3];
    uint8_t *d_recon[3];
    uint32_t src_stride[3], stride[3], width[3], height[3];      /* samples; width x height of the source and of the reconstruction */
    size_t src_pic_pitch[3], recon_pic_pitch[3];                  /* samples between pictures */
    const svt_hip_qrows *q_luma, *q_chroma;      /* HOST */
    const int16_t *d_tables;              /* svt_hip_intra_encode_tables_fill */
    uint8_t *d_status;                    /* optional [npics][sb_pitch][256] */
    svt_hip_intra_enc_result *d_result;   /* optional [npics][sb_pitch][256] */
    int32_t *d_sb_qcoeff[3];              /* optional [npics][sb_pitch][4096], [1024], [1024] */
    uint32_t *d_coeff_offset;             /* optional [npics][sb_pitch][256][2] */
    void *d_scratch;
    size_t scratch_bytes;
} svt_hip_intra_encode_args;
size_t svt_hip_intra_encode_scratch_bytes(uint32_t npics, uint32_t nsb);      /* HOST */
size_t svt_hip_intra_encode_tables_bytes(void);                               /* HOST */
int svt_hip_intra_encode_tables_fill(void *host);                             /* HOST: the blob d_tables holds */
int svt_hip_intra_encode_launches(uint32_t sb_cols, uint32_t sb_rows, int planes);      /* HOST: launches of one call */
int svt_hip_intra_encode_frame(const svt_hip_intra_encode_args *a, void *stream);

/* Deblocking of whole pictures: av1_loop_filter_frame(recon, pcs, 0, 3) as the DLF process calls it (EbDlfProcess.c:162,
 * EbDeblockingFilter.c:1351) and the filter-level search of av1_pick_filter_level (:1851), 8- and 10-bit 4:2:0, 64x64 superblocks.
 *
 * The mode-info grid.  The deblocker reads five members of MbModeInfo per 4x4 luma unit; they are held in a 4-byte record:
 *   bsize            sb_type (clamped to 0 .. 21 on the device)
 *   tx_size          the luma TxSize (clamped to 0 .. 18)
 *   ref_frame_skip   ref_frame[0] (0 .. 7) in bits 0 .. 2, skip in bit 7
 *   mode             the PredictionMode; anything at or above MB_MODE_COUNT (25), INTRA_MODE_4x4 among them, is read as DC_PRED
 *                    (get_filter_level, :637)
 * The grid is [mi_rows][mi_stride] records with mi_rows >= height / 4 and mi_stride >= width / 4 (the reference's is
 * picture_width_in_sb * 16); pictures of a stack are mi_pitch records apart.
 *
 * svt_hip_dlf_mi_frame scatters a final block list (d_final / d_final_count as svt_hip_partition_decide_frame writes them) into the
 * grid, what update_av1_mi_map (EbAdaptiveMotionVectorPrediction.c:1350-1415) does at the encode pass.  The fill rules are this
 * project's glue: per entry k < d_final_count[sb] (a count above 256 is taken as 256) the geometry of mds_idx (clamped to 1 100) gives
 * bsize and the block size's own transform size (blk_geom->txsize[0]); the entry's x, y are its place in the picture; d_info[src]
 * gives ref_frame0, mode and skip; the bwidth / 4 x bheight / 4 units from (x / 4, y / 4) are written.  An entry is left out when its
 * src is SVT_HIP_PART_NO_SRC or at or past nsrc, or when it reaches outside mi_cols x mi_rows.  Units no entry covers keep what they
 * held.  One launch.  Validation (SVT_HIP_ERR_INVALID): NULL pointers, zero npics / nsb / nsrc / mi_cols / mi_rows, mi_stride below
 * mi_cols, mi_cols or mi_rows above 16 384, npics * sb_pitch above 2^20, misalignment (4 bytes).
 *
 * svt_hip_dlf_apply_frame filters d_rec into d_dst; d_dst[i] == d_rec[i] for all three planes filters in place.
 *   limits    update_sharpness and the hev threshold lvl >> 4 (:608-627, :691-692)
 *   levels    av1_loop_filter_frame_init (:698-764): per plane, direction, reference frame and mode_lf_lut[mode], with the
 *             1 << (lvl >> 5) scale of the deltas and the clamp to 0 .. 63
 *   gating    loop_filter_sb (:1297-1303): both luma levels 0 end the plane loop (chroma is not filtered either); a chroma level 0
 *             skips that plane; with two buffers an unfiltered plane is copied
 *   edges     set_lpf_parameters (:893-1012) for every 4-sample edge unit: nothing at or beyond the plane's width / height; chroma
 *             reads the mode-info at the odd row and column of the 8x8; the previous unit lies 1 << ss units back in the edge's
 *             direction; the chroma transform size is av1_get_max_uv_txsize(bsize) through txsize_horz_map / txsize_vert_map; an edge
 *             only where the coordinate is a non-zero multiple of the current unit's transform side; it is filtered when
 *             (curr_level || pv_lvl) && (!pv_skip || !curr_skipped || pu_edge), a unit counting as skipped when skip &&
 *             ref_frame[0] > INTRA_FRAME; length 4 / 8 / 14 (luma) or 4 / 6 (chroma) from the smaller transform side;
 *             level = curr_level ? curr_level : pv_lvl
 *   filters   aom_lpf_{vertical,horizontal}_{4,6,8,14} and their highbd twins (filter4 / 6 / 8 / 14, :133-370; the thresholds
 *             shifted by bit_depth - 8)
 * The reference filters superblock by superblock and delays the horizontal edges by one superblock column; that equals every
 * vertical edge of the picture, then every horizontal one, and inside a pass no edge reads a sample another edge of the pass
 * modifies.  The reference walks by the current transform size, the kernels decide every 4-sample unit on its own:
 * the two agree on a grid whose blocks are aligned to their size; on any other grid the samples are unspecified, but nothing outside
 * width x height of a plane is read or written.  In place: two launches (vertical edges, horizontal edges).  Two buffers: one launch
 * over 64x64 tiles with a halo of 8 samples in the LDS.
 * Validation (SVT_HIP_ERR_INVALID): NULL planes or grid; a side that is 0, not a multiple of 8 or above 65 535; a stride below the
 * width; mi_stride below width / 4; a level above 63 or below 0; sharpness outside 0 .. 7; a bit depth other than 8 / 10; a delta
 * outside -63 .. 63; npics 0 or above 65 535; d_dst planes that are partly equal to d_rec, or that overlap d_rec without being equal.
 *
 * svt_hip_dlf_search_frame builds the table search_filter_level (:1687) fills lazily: d_sse[pic][plane][64] (uint64) = ss_err[level]
 * of the plane.  For every level in mask[plane] (bit l = level l) the plane is filtered as try_filter_frame does (:1632-1686; luma
 * with the trial level in both directions, the reference's dir == 2 call; Cb / Cr with the trial level; sharpness and deltas from the
 * descriptor, its four levels ignored) and the squared error against d_src is summed over width x height (PictureSseCalculations,
 * :1470).  Level 0 is the unfiltered plane's SSE.  Levels outside the mask are written as UINT64_MAX, the reference's "not computed"
 * -1, so every entry is defined after the call.  Filtered samples are never stored and d_rec is not written.  Two launches: per
 * tile and plane the partial sums (the tile and the source staged once for all levels), then their sum per (picture, plane, level).
 * d_scratch: svt_hip_dlf_search_scratch_bytes(width, height, npics) bytes, 8-byte aligned.
 *
 * Every call validates every host argument before anything is enqueued, only enqueues on the given stream, allocates nothing, never
 * synchronises and can be captured into a HIP graph.  svt_hip_dlf_check runs the same validation without a device (for_search: 0 =
 * apply, 1 = search).
 * NOT here: delta LF (delta_lf_present_flag, which the reference itself refuses), segment features, 128-wide superblocks, more than
 * one transform block per luma block, LPF_PICK_FROM_SUBIMAGE.  Loop restoration has its own block below (svt_hip_lr_*). */
typedef struct svt_hip_dlf_mi { uint8_t bsize, tx_size, ref_frame_skip, mode; } svt_hip_dlf_mi;
typedef struct svt_hip_dlf_info { uint8_t ref_frame0, mode, skip, pad; } svt_hip_dlf_info;      /* one per src */
typedef struct svt_hip_dlf_mi_args {
    const svt_hip_part_final *d_final;    /* [npics][sb_pitch][256] */
    const uint32_t *d_final_count;        /* [npics][sb_pitch] */
    const svt_hip_dlf_info *d_info;       /* [nsrc] */
    svt_hip_dlf_mi *d_mi;                 /* [npics] grids of [mi_rows][mi_stride], mi_pitch records apart */
    uint32_t npics, nsb, sb_pitch;        /* sb_pitch 0 = nsb */
    uint32_t nsrc;
    uint32_t mi_cols, mi_rows, mi_stride;
    uint32_t pad;
    uint64_t mi_pitch;
} svt_hip_dlf_mi_args;
typedef struct svt_hip_dlf_pic {
    const void *d_rec[3];  uint32_t rec_stride[3];   /* the reconstruction (Y, Cb, Cr), strides in samples */
    const void *d_src[3];  uint32_t src_stride[3];   /* the source picture (search only) */
    void *d_dst[3];        uint32_t dst_stride[3];   /* the deblocked picture (apply only); all three equal to d_rec = in place */
    const svt_hip_dlf_mi *d_mi; uint32_t mi_stride;
    uint32_t width, height;
    int32_t bit_depth;
    uint32_t npics;                                 /* >= 1 */
    uint64_t rec_pitch[3], src_pitch[3], dst_pitch[3], mi_pitch;      /* samples / records between the pictures of a stack */
    int32_t filter_level[2];                        /* luma: [0] vertical edges, [1] horizontal edges (apply only) */
    int32_t filter_level_u, filter_level_v;         /* (apply only) */
    int32_t sharpness_level;
    int32_t mode_ref_delta_enabled;
    int8_t ref_deltas[8], mode_deltas[2];
    uint8_t pad[6];
} svt_hip_dlf_pic;
int svt_hip_dlf_mi_frame(const svt_hip_dlf_mi_args *a, void *stream);
int svt_hip_dlf_apply_frame(const svt_hip_dlf_pic *pic, void *stream);
int svt_hip_dlf_search_frame(const svt_hip_dlf_pic *pic, const uint64_t mask[3], uint64_t *d_sse, void *d_scratch, size_t scratch_bytes,
                             void *stream);
size_t svt_hip_dlf_search_scratch_bytes(uint32_t width, uint32_t height, uint32_t npics);      /* HOST; 0 for a bad geometry */
int svt_hip_dlf_check(const svt_hip_dlf_pic *pic, int for_search);                              /* HOST */
int svt_hip_dlf_mi_check(const svt_hip_dlf_mi_args *a);                                         /* HOST */
/* HOST: the tables the kernels use, for inspection: lim / mblim / hev_thr of a level at a sharpness (update_sharpness), and the
 * level of (plane 0 .. 2, dir 0 .. 1, ref_frame 0 .. 7, mode_lf 0 .. 1) that av1_loop_filter_frame_init stores for pic. */
int svt_hip_dlf_limits(int level, int sharpness_level, uint8_t out[3]);
int svt_hip_dlf_levels(const svt_hip_dlf_pic *pic, uint8_t out[3][2][8][2]);

/* HOST helpers of the level pick, no device.
 * svt_hip_dlf_pick_level: the walk of search_filter_level (:1711-1848) over a table ss_err[64] (-1 = not computed).  start_level is
 * what the reference takes from last_frame_filter_level: for luma entry [2], the previous picture's filter_level_u, because
 * av1_pick_filter_level calls with dir 2 (:1918-1920, :1706); for Cb entry [2] and for Cr entry [3], the previous u and v levels.
 * loop_filter_mode <= 2: one step of 2 either way; otherwise the halving search from step (start < 16 ? 4 : start / 4).  The bias
 * against raising the level is (best_err >> (15 - filt_mid / 8)) * filter_step, halved unless tx_mode_is_only_4x4; a lower level
 * wins when its error is below best + bias ("close to best"), a higher one when below best - bias ("significantly better").
 * Returns SVT_HIP_OK with *level, or, when the walk reads an entry that is -1, SVT_HIP_DLF_NEED_LEVEL with that level in *need: a
 * caller fills the table in rounds (svt_hip_dlf_search_frame with that bit) or asks for all 64 at once.
 * svt_hip_dlf_level_from_q: the LPF_PICK_FROM_Q branch (:1867-1909) on the library's quantiser table: levels = {filter_level[0],
 * filter_level[1], filter_level_u, filter_level_v}. */
#define SVT_HIP_DLF_NEED_LEVEL 1
int svt_hip_dlf_pick_level(const int64_t ss_err[64], int start_level, int loop_filter_mode, int tx_mode_is_only_4x4, int *level, int *need);
int svt_hip_dlf_level_from_q(int base_qindex, int bit_depth, int is_key_frame, int levels[4]);

/* ---- loop restoration of whole pictures --------------------------------------------------------------------------
 * The reference's Rest process (EbRestProcess.c:205): the stage behind CDEF.  One tile, 4:2:0, bit depth 8 or 10, optimized_lr 0.
 * All of it is integer arithmetic and equals the reference bit for bit.
 *
 * Two operands instead of boundary buffers.  The reference saves lines of the deblocked picture and of the CDEF output
 * (av1_loop_restoration_save_boundary_lines, EbRestoration.c:1734), patches three rows into the frame above and below every
 * stripe (setup_processing_stripe_boundary, :374) and puts them back (restore_processing_stripe_boundary, :478); which rows is
 * get_stripe_boundary_info's business (:342).  All of that is a choice of the picture a halo row is read from, so the calls take
 * the CDEF output d_cdef (the filter's input) and the deblocked picture d_dblk (stripe context only) and read
 *   rows above a stripe that starts at y0 > 0                deblocked rows y0 - 2, y0 - 2, y0 - 1
 *   rows below a stripe that ends at y1 < plane height       deblocked rows y1, y1 + 1, y1 + 1
 *   at the picture's top / bottom                            the CDEF picture's edge row three times (extend_frame, :276)
 *   every column                                             clamped to 0 .. plane width - 1, in both pictures (extend_frame by 3,
 *                                                            extend_lines by 4, :1570)
 * With sides that are multiples of 8 a stripe never ends one row above the picture's bottom, so the reference's one-line case
 * (lines_to_save == 1, :1608) cannot occur; other sides are refused.
 *
 *   units     foreach_rest_unit_in_tile (:1331-1377): a unit is unit_size wide / high, the last of a row / column absorbs a
 *             remainder below unit_size * 3 / 2; v_start / v_end are shifted up by RESTORATION_UNIT_OFFSET >> ss_y (8 / 4) but at the
 *             picture's top / bottom; the counts are av1_alloc_restoration_struct's (:198-235).  unit_size: luma 64 / 128 / 256, chroma
 *             equal to luma or half of it (the reference: 256 above 352x288 luma samples, else 128; EbPictureControlSet.c:32-48).
 *   stripes   av1_loop_restoration_filter_unit (:1168-1236): 64 >> ss_y rows, the first shorter by 8 >> ss_y, cut at the unit's v_end
 *             (which, with these unit sizes, is a stripe boundary or the picture's bottom).
 *
 * svt_hip_lr_apply_frame is av1_loop_restoration_filter_frame (:1271-1329).  frame_type[plane]: 0 RESTORE_NONE, 1 RESTORE_WIENER,
 * 2 RESTORE_SGRPROJ, 3 RESTORE_SWITCHABLE.  d_units [pic][plane][units_per_tile(plane)] records, row-major over the unit grid (a plane's
 * block starts at svt_hip_lr_unit_offset(..)).  A plane of frame type none, and a unit of type none, is copied from d_cdef
 * (copy_tile, :1182-1185): every sample of the three planes of d_dst is defined after the call, and nothing outside them is written.
 *   Wiener        wiener_filter_stripe[_highbd] -> av1_[highbd_]wiener_convolve_add_src_c (convolve.c:64-143, 145-230): taps 0 .. 2 of the
 *                 record, the rest by symmetry with centre -2 * (t0 + t1 + t2) (finalize_sym_filter) plus the implicit 128; horizontal
 *                 pass with round_0 = 3 and the clamp to WIENER_CLAMP_LIMIT(3, bd) - 1, vertical pass with round_1 = 11, which is what
 *                 get_conv_params_wiener gives at 8 and 10 bit (:110-132).  The reference rounds a call's width up to 16 and writes past
 *                 the unit, which the next unit overwrites; here only the unit's own samples are produced.
 *   self-guided   sgrproj_filter_stripe -> apply_selfguided_restoration_c (:1062-1099) -> av1_selfguided_restoration_c (:1022-1060):
 *                 sgr_params[ep]; r[0] > 0: selfguided_restoration_fast_internal (:770-900; A / B on every other row counted from the
 *                 stripe's first row minus one, other weights on even and odd rows); r[1] > 0: selfguided_restoration_internal
 *                 (:902-1020); boxsum for r = 1, 2, the a * n < b * b saturation, x_by_xplus1, one_by_x; decode_xq, the projection and
 *                 the clip.  Each pass reads real neighbours, so the result does not depend on the reference's 64-column processing
 *                 units.
 * A record of the device array is not validated on the host: an out-of-range field is clamped (a type above 2 or one the plane's frame
 * type does not allow reads as none), and nothing outside the planes is touched.
 *
 * svt_hip_lr_try_frame is try_restoration_unit_seg (EbRestorationPick.c:197-224) for ncand candidates (pic, plane, unit, record): the
 * unit is filtered exactly as in apply and its squared error against d_src over the unit's rectangle goes to d_sse[cand] (int64;
 * sse_restoration_unit, :65-72).  A record of type none gives rusi->sse[RESTORE_NONE] (search_norestore_seg).  The plane's frame type
 * plays no part.  Filtered samples are never stored, d_cdef is not written, every d_sse entry is defined after the call (INT64_MAX for a
 * candidate whose pic / plane / unit is out of range), and many candidates for one unit are allowed: a search round.
 *
 * svt_hip_lr_wiener_stats_frame is av1_compute_stats_c / av1_compute_stats_highbd_c (:765-858) per unit of every plane: the truncating
 * average of the unit of d_cdef (find_average, EbRestorationPick.h:33), X = src - avg, the win x win window of d_cdef - avg indexed
 * k-major as written (:781-786: column offset outer, row offset inner), M[win2] and the full symmetric H[win2 * win2]; at 10 bit the
 * truncating division by 4 of M and of H's upper triangle before mirroring (:850-857).  Window reads outside the picture clamp (the
 * reference runs on the frame extended by 3); the stripe rule plays no part here.  wiener_win[plane]: 7, 5 or 3.  d_M [unit][49] and
 * d_H [unit][49 * 49] int64, each unit's block dense at win2 as the reference packs it; unit = svt_hip_lr_unit_offset + index, per
 * picture svt_hip_lr_units_per_pic records.  d_scratch: svt_hip_lr_stats_scratch_bytes(..) bytes, 8-byte aligned.
 *
 * Every call validates every host argument before anything is enqueued, only enqueues on the given stream, allocates nothing, never
 * synchronises and can be captured into a HIP graph.  svt_hip_lr_check runs the validation without a device: what = 0 apply, 1 try,
 * 2 statistics; h_units (may be NULL) is a HOST copy of the records ([plane][units], one picture, nunits of them) checked against
 * frame_type: a type the frame type does not allow, taps outside WIENER_FILT_TAP{0,1,2}_{MINV,MAXV}, ep outside 0 .. 15, xqd outside
 * SGRPROJ_PRJ_{MIN,MAX}{0,1}.  Validation (SVT_HIP_ERR_INVALID): NULL planes; a side that is 0, not a multiple of 8 or above 65 535; a
 * stride below the width; a bit depth other than 8 / 10; a bad unit_size; a frame type outside 0 .. 3; a window other than 7 / 5 / 3;
 * npics 0; an output plane that overlaps an input plane; in a stack an output pitch below one picture; misaligned 64-bit outputs.
 * NOT here (the Wiener derivation, its refinement walk and the picture-level finish are host helpers, and the self-guided parameter
 * search has its own calls, both below): more than one tile, superres, optimized_lr, bit depth 12, 4:2:2 / 4:4:4. */
typedef struct svt_hip_lr_unit {
    int32_t type;                       /* 0 none, 1 Wiener, 2 self-guided */
    int16_t vfilter[3], hfilter[3];     /* taps 0 .. 2 */
    int16_t xqd[2];
    int32_t ep;                         /* 0 .. 15 */
} svt_hip_lr_unit;
typedef struct svt_hip_lr_cand { uint32_t pic, plane, unit; svt_hip_lr_unit u; } svt_hip_lr_cand;
typedef struct svt_hip_lr_pic {
    const void *d_cdef[3]; uint32_t cdef_stride[3]; uint32_t pad0;   /* the CDEF output: the filter's input; strides in samples */
    const void *d_dblk[3]; uint32_t dblk_stride[3]; uint32_t pad1;   /* the deblocked picture before CDEF: stripe context only */
    const void *d_src[3];  uint32_t src_stride[3];  uint32_t pad2;   /* the source picture (try and statistics) */
    void *d_dst[3];        uint32_t dst_stride[3];  uint32_t pad3;   /* the restored picture (apply only) */
    uint32_t width, height;
    int32_t bit_depth;
    uint32_t unit_size[3];
    uint32_t npics;                                                  /* >= 1 */
    uint32_t pad4;
    uint64_t cdef_pitch[3], dblk_pitch[3], src_pitch[3], dst_pitch[3];      /* samples between the pictures of a stack */
} svt_hip_lr_pic;
int svt_hip_lr_apply_frame(const svt_hip_lr_pic *pic, const int32_t frame_type[3], const svt_hip_lr_unit *d_units, void *stream);
int svt_hip_lr_try_frame(const svt_hip_lr_pic *pic, const svt_hip_lr_cand *d_cand, uint32_t ncand, int64_t *d_sse, void *stream);
int svt_hip_lr_wiener_stats_frame(const svt_hip_lr_pic *pic, const int32_t wiener_win[3], int64_t *d_M, int64_t *d_H, void *d_scratch,
                                  size_t scratch_bytes, void *stream);
size_t svt_hip_lr_stats_scratch_bytes(uint32_t width, uint32_t height, const uint32_t unit_size[3], uint32_t npics);      /* HOST; 0 = refused */
int svt_hip_lr_check(const svt_hip_lr_pic *pic, int what, const int32_t frame_type[3], const svt_hip_lr_unit *h_units, uint32_t nunits);   /* HOST */
/* HOST: the unit grid of a plane: out = {horz_units_per_tile, vert_units_per_tile, units_per_tile}; the limits of unit `index`
 * (row-major): out = {h_start, h_end, v_start, v_end}; where a plane's records start inside a picture's block, and that block's size */
int svt_hip_lr_unit_grid(uint32_t width, uint32_t height, const uint32_t unit_size[3], int plane, int32_t out[3]);
int svt_hip_lr_unit_limits(uint32_t width, uint32_t height, const uint32_t unit_size[3], int plane, uint32_t index, int32_t out[4]);
uint32_t svt_hip_lr_unit_offset(uint32_t width, uint32_t height, const uint32_t unit_size[3], int plane);      /* 0 for a refused geometry */
uint32_t svt_hip_lr_units_per_pic(uint32_t width, uint32_t height, const uint32_t unit_size[3]);

/* HOST helpers of the Wiener search, no device, integer arithmetic as in the reference.
 * svt_hip_lr_wiener_solve: wiener_decompose_sep_sym (EbRestorationPick.c:1021-1052; update_a_sep_sym / update_b_sep_sym / linsolve_wiener,
 * NUM_WIENER_ITERS 5, WIENER_TAP_SCALE_FACTOR 2^16, the c / 256 * A / cd * 256 elimination), finalize_sym_filter (:1094-1126, with the
 * shuffle of the 5- and 3-tap windows) and compute_score (:1053-1092) on one unit's M [win2] / H [win2 * win2] as
 * svt_hip_lr_wiener_stats_frame packs them: taps 0 .. 2 of the vertical and the horizontal filter, and *accepted = 0 when the score is
 * above 0 (search_wiener_seg then leaves the unit's Wiener SSE at INT64_MAX and tries nothing), else 1.
 * svt_hip_lr_walk_start / _next: finer_tile_search_wiener_seg (:1278-1387) turned inside out.  start takes the solve's taps and
 * returns SVT_HIP_LR_WALK_TRY: the caller measures the taps in w->vfilter / w->hfilter (svt_hip_lr_try_frame) and hands the SSE to
 * next, which answers SVT_HIP_LR_WALK_TRY with the next taps to measure or SVT_HIP_LR_WALK_DONE with the final taps in the same place
 * and their SSE in w->err.  start_step 4; per step the horizontal taps, then the vertical ones, from the window's first tap (plane_off);
 * a successful downward move ends that tap loop (`if (skip) break;`); at step 4 a successful move is repeated; err2 > err rejects, so a tie
 * is accepted.  The walk makes no device call; many units' walks advance in lock step with one svt_hip_lr_try_frame per round. */
#define SVT_HIP_LR_WALK_TRY 1
#define SVT_HIP_LR_WALK_DONE 2
typedef struct svt_hip_lr_walk {
    int16_t vfilter[3], hfilter[3];     /* the taps to measure (TRY) or the final taps (DONE) */
    int32_t win, step, dir, p, phase, skip, state;      /* the walk's position: private to the two functions */
    int64_t err;                        /* the SSE of the taps kept so far */
} svt_hip_lr_walk;
int svt_hip_lr_wiener_solve(int win, const int64_t *M, const int64_t *H, int16_t vfilter[3], int16_t hfilter[3], int *accepted);
int svt_hip_lr_walk_start(svt_hip_lr_walk *w, int win, const int16_t vfilter[3], const int16_t hfilter[3]);
int svt_hip_lr_walk_next(svt_hip_lr_walk *w, int64_t sse);

/* The self-guided parameter search: search_sgrproj_seg -> search_selfguided_restoration (EbRestorationPick.c:1681-1722, :605-661) for
 * every unit of every plane, for the parameter sets ep_lo <= ep < ep_hi (0 <= ep_lo <= ep_hi <= 16; one range per call).  Filter once,
 * score many times:
 *   svt_hip_lr_sgr_stats_frame   apply_sgr (:580-603) and the sums of get_proj_subspace (:463-521).  The filter runs on d_cdef alone, every
 *                 halo row and column clamped to the plane: there is NO stripe rule here and d_dblk is not read (the reference filters
 *                 the CDEF frame extended by 3).  With u = dat << 4, s = (src << 4) - u, f1 = flt0 - u, f2 = flt1 - u (0 for a radius of
 *                 0): d_stats [pic][unit][16][5] int64 = H00 = sum f1 f1, H11 = sum f2 f2, H01 = sum f1 f2, C0 = sum f1 s, C1 = sum f2 s
 *                 over the unit, exact totals (the reference adds the same integers in double, below 2^53).  Entries of the range are
 *                 all defined after the call, entries outside it untouched.  f1 / f2 (an int16 pair per sample and ep) and src - dat
 *                 (int16 per sample) are left in d_scratch, unit-contiguous, for the walk.
 *   svt_hip_lr_sgr_solve   HOST: the tail of get_proj_subspace (:522-558: division by the sample count, the 1x1 or 2x2 solve, Det < 1e-8
 *                 -> (0, 0), rint(x * 128), INT32_MIN where that leaves int32 as the reference's compiled conversion does) and encode_xq
 *                 (:561-577) on one entry's five sums: binary64, nothing contracted.  npix: the unit's samples.
 *   svt_hip_lr_sgr_walk_frame   finer_search_pixel_proj_error (:398-459, start_step 2) per (pic, unit, ep) on the scratch the statistics
 *                 call left (same range): e = ((xq0 f1 + xq1 f2 + 1024) >> 11) - (src - dat), err = sum e e, no clip; a successful move is
 *                 repeated at step 2; a successful downward move of xqd[0] skips xqd[1] at that step; err2 > err rejects, so a tie is
 *                 accepted; components of radius 0 are skipped; SGRPROJ_PRJ_{MIN,MAX}{0,1} bound the moves.  d_start [pic][unit][16][2]
 *                 int16: the start per entry (out-of-range values are clamped), or NULL: solved on the device from d_stats by the same
 *                 text as svt_hip_lr_sgr_solve.  d_walk [pic][unit][16]: the final xqd, its error, the start the walk left from and the
 *                 evaluations made (at most 137: the ranges bound the walk).  One workgroup per entry; none waits for another.
 *   svt_hip_lr_sgr_walk_host   HOST: the same walk over arrays f1 / f2 / sd of n samples; xqd: start in, result out; trials (may be
 *                 NULL) [max_trials][3] int64: xq[0], xq[1] and the error of every evaluation in order.  Returns the evaluations (> 0)
 *                 or an error (< 0).
 *   svt_hip_lr_sgr_search_frame   the whole search: statistics, walk with the device solve, per unit the first lowest error of the range
 *                 (besterr == -1 || err < besterr), then try_restoration_unit_seg on the winner - the stripe-aware filter of
 *                 svt_hip_lr_try_frame, which is where d_dblk is read.  d_best [pic][unit]: what svt_hip_lr_result takes at index 2.  An
 *                 empty range (ep_lo == ep_hi: sg_filter_mode 1 with a reference ep) gives ep 0, xqd 0, 0, proj_err -1 and their SSE.
 *   svt_hip_lr_sgr_ep_range   HOST: get_sg_step (:681-700) and mid_ep / start_ep / end_ep (:625-631): out = {start_ep, end_ep}.
 *                 sg_ref_frame_ep: below 0 = none, else 0 .. 15.
 * d_scratch: svt_hip_lr_sgr_scratch_bytes(..) bytes (0 = refused), 16-byte aligned, one size for the three device calls: 2 bytes per
 * sample of a picture (width * height * 3 / 2) plus 4 per sample and ep of the range, plus a few bytes per unit for the search call's
 * stages.  1920x1080 with all 16 ep: about 205 MB per picture; a narrower range shrinks it in proportion.
 * The device calls follow the block's rules (validate everything first, enqueue only, allocate nothing, never synchronise, one stream,
 * a linear chain of launches, capturable); svt_hip_lr_check takes what = 3 for the statistics / walk operands (d_cdef, d_src) and 4 for
 * the search's (d_cdef, d_dblk, d_src).  Also refused: a bad ep range; a scratch that is NULL, too small or misaligned; d_stats, d_walk or
 * d_best NULL or not 8-byte aligned. */
typedef struct svt_hip_lr_sgr_walk { int64_t err; int16_t xqd[2], start[2]; int32_t evals, pad; } svt_hip_lr_sgr_walk;
typedef struct svt_hip_lr_sgr_best { int64_t sse, proj_err; int32_t ep; int16_t xqd[2]; } svt_hip_lr_sgr_best;
size_t svt_hip_lr_sgr_scratch_bytes(uint32_t width, uint32_t height, const uint32_t unit_size[3], uint32_t npics, int ep_lo, int ep_hi);      /* HOST */
int svt_hip_lr_sgr_stats_frame(const svt_hip_lr_pic *pic, int ep_lo, int ep_hi, int64_t *d_stats, void *d_scratch, size_t scratch_bytes, void *stream);
int svt_hip_lr_sgr_walk_frame(const svt_hip_lr_pic *pic, int ep_lo, int ep_hi, const int64_t *d_stats, const int16_t *d_start, const void *d_scratch,
                              size_t scratch_bytes, svt_hip_lr_sgr_walk *d_walk, void *stream);
int svt_hip_lr_sgr_search_frame(const svt_hip_lr_pic *pic, int ep_lo, int ep_hi, svt_hip_lr_sgr_best *d_best, void *d_scratch, size_t scratch_bytes,
                                void *stream);
int svt_hip_lr_sgr_solve(const int64_t stats[5], uint32_t npix, int ep, int16_t xqd[2]);                                                    /* HOST */
int svt_hip_lr_sgr_walk_host(const int16_t *f1, const int16_t *f2, const int16_t *sd, uint32_t n, int ep, int16_t xqd[2], int64_t *err, int64_t *trials,
                             int max_trials);                                                                                               /* HOST */
int svt_hip_lr_sgr_ep_range(const int8_t sg_ref_frame_ep[2], int sg_filter_mode, int32_t out[2]);                                           /* HOST */

/* svt_hip_lr_finish: rest_finish_search (EbRestorationPick.c:1989-2058) for one plane, on the host.  results[u]: what the unit's searches
 * left in RestUnitSearchInfo - sse[0] of the unfiltered unit (search_norestore_seg), sse[1] and the taps of the Wiener search (INT64_MAX =
 * compute_score refused), sse[2], ep and xqd of the self-guided search (svt_hip_lr_sgr_search_frame's d_best).  Mirrored as written:
 * force_restore_type_d (wn_filter_mode 0 allows none and self-guided only); num_rtypes = RESTORE_SWITCHABLE_TYPES when the plane has one
 * unit, so such a plane never ends switchable; per frame type search_rest_type_finish over the units in index order with the running
 * reference filters rsc->wiener / rsc->sgrproj reset to their defaults by rsc_on_tile; count_wiener_bits / count_sgrproj_bits with
 * aom_count_primitive_refsubexpfin (EbEntropyCoding.c:3293-3460); bits >> 4 inside RDCOST_DBL (binary64); search_wiener_finish's window
 * from wn_filter_mode and the plane, search_switchable's WIENER_WIN for luma whatever the mode (:1518-1519); r == 0 || cost < best_cost;
 * copy_unit_info into units[u] (all zero when the plane ends RESTORE_NONE).  *frame_restoration_type and units are what
 * svt_hip_lr_apply_frame takes for the plane. */
typedef struct svt_hip_lr_result {
    int64_t sse[3];                     /* none, Wiener (INT64_MAX = refused), self-guided */
    int16_t vfilter[3], hfilter[3];     /* taps 0 .. 2 of the Wiener search */
    int16_t xqd[2];
    int32_t ep;
    int32_t pad;
} svt_hip_lr_result;
typedef struct svt_hip_lr_costs {
    int32_t rdmult;
    int32_t wiener_restore_cost[2], sgrproj_restore_cost[2], switchable_restore_cost[3];
} svt_hip_lr_costs;
int svt_hip_lr_finish(int plane, int wn_filter_mode, const svt_hip_lr_costs *costs, const svt_hip_lr_result *results, uint32_t nunits,
                      int32_t *frame_restoration_type, svt_hip_lr_unit *units);

/* ---- dispatch registration ---------------------------------------------------------------------------------------
 * The library keeps a registry {reference slot name -> drop-in of the same signature} for every RTCD global of
 * aom_dsp_rtcd.h it implements (svt_hip_rtcd_slot_count() entries: the 19 av1_fwd_txfm2d_WxH, the 19
 * av1_inv_txfm2d_add_WxH, av1_inv_txfm_add, the six quantisers, ResidualKernel, 380 intra predictor slots,
 * eb_smooth_v/h_predictor, av1_dr_prediction_z1-3 and their highbd twins, the edge filters / upsamplers, subtract_average,
 * cfl_predict_lbd/hbd, av1_txb_init_levels, 22 aom_sadMxN and 22 aom_sadMxNx4d).  After the stock
 * setup_rtcd_internal(asm_type) (EbEncHandle.c:917) and BEFORE init_intra_predictors_internal() the host calls, per slot,
 *     svt_hip_rtcd_override_slot("aom_dc_predictor_16x16", (void **)&aom_dc_predictor_16x16);
 * (INTEGRATION.md has the macro that does it for every slot).  Unknown names return SVT_HIP_ERR_INVALID and leave the
 * slot alone.  GRACEFUL REFUSAL: when the device is unusable (no HIP runtime, no gfx950 part) both override calls return
 * SVT_HIP_ERR_NO_DEVICE and store nothing - the host's pointers keep what setup_rtcd_internal put there (the AVX2 kernels:
 * the encoder's own fallback; integration/asm_hip.patch also takes asm_type back to ASM_AVX2 then).  Once a slot has been
 * handed out, a HIP error in the middle of a run still abort()s inside the drop-in: its reference signature has no error
 * channel and there is deliberately no CPU path in this library.  The *_funcPtrArray[asm_type] tables are static per translation unit in the reference, so their ASM_HIP rows
 * are added at compile time (integration/asm_hip.patch). */
int svt_hip_rtcd_slot_count(void);
const char *svt_hip_rtcd_slot_name(int index);        /* NULL when out of range */
void *svt_hip_rtcd_slot_function(const char *name);   /* the drop-in registered under a reference slot name, or NULL */
int svt_hip_rtcd_override_slot(const char *name, void **slot);

/* Pointer table the host fills after the stock setup_rtcd_internal(asm_type)
 * (EbEncHandle.c:917) and BEFORE init_intra_predictors_internal(): each member is
 * the address of the reference's RTCD global of the same name (or NULL to leave
 * that slot alone).  svt_hip_rtcd_override stores the svt_hip_* drop-ins in them. */
typedef struct svt_hip_rtcd_table {
    void **av1_fwd_txfm2d[SVT_TX_SIZES_ALL];      /* &av1_fwd_txfm2d_4x4 ... by TxSize */
    void **av1_inv_txfm2d_add[SVT_TX_SIZES_ALL];  /* &av1_inv_txfm2d_add_4x4 ... */
    void **av1_inv_txfm_add;
    void **aom_quantize_b, **aom_quantize_b_32x32, **aom_quantize_b_64x64;
    void **aom_highbd_quantize_b, **aom_highbd_quantize_b_32x32, **aom_highbd_quantize_b_64x64;
    void **ResidualKernel;
} svt_hip_rtcd_table;
int svt_hip_rtcd_override(const svt_hip_rtcd_table *table);

#ifdef __cplusplus
}
#endif
#endif /* SVT_HIP_DSP_H */

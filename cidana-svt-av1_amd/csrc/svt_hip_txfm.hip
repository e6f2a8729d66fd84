// svt_hip_txfm.hip — entry points of the transform family of libsvt_hip_dsp.so (include/svt_hip_dsp.h): forward / inverse
// 2-D transforms, 64-point packing, quantiser, the fused chains (headline, encode pass, planes) and their drop-ins.
// Every entry point is require_init, the NULL and alias checks that need the pointers, ONE plan (tx_plan.h: every other refusal, the
// kernel, its variant, grid and threads) and one switch over the plan's route that launches.  Nothing here computes a grid.
#include "host_common.h"
#include "kernel_fused32.h"
#include "kernel_quant.h"
#include "kernel_txfm.h"
#include "kernel_txfm_staged.h"
#include "kernel_enc64.h"
#include "kernel_frame.h"
#include "tx_plan.h"

using namespace svtdev;
using namespace svthost;

namespace {
static_assert(kFrameMaxGroups == FRAME_MAX_GROUPS && kFrameMaxLaunchWgs == kMaxLaunchWgs, "tx_plan.h's frame_plan knows the room of a group table");

// every pointer 16-B aligned (NULL counts as aligned: an output the caller did not ask for)
template <typename... P>
bool aligned16(const P*... p) { return ((... | (uintptr_t)p) & 15) == 0; }
#define PLAN_LAUNCH(K, ...) hipLaunchKernelGGL(K, dim3(p.grid), dim3(p.threads), 0, s, __VA_ARGS__)

// ---------------------------------------------------------------------------
// 64-pt packing kernel (HandleTransform64x64_c & friends)
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(256) void pack64_kernel(int32_t* __restrict__ coeff,
                                                     unsigned long long* __restrict__ energy, int w, int h,
                                                     uint32_t nblocks) {
    // one workgroup per block; reads complete before any write (barrier)
    const uint32_t blk = blockIdx.x;
    if (blk >= nblocks) return;
    const int kw = w > 32 ? 32 : w, kh = h > 32 ? 32 : h;
    int32_t* c = coeff + (size_t)blk * w * h;
    __shared__ int32_t keep[1024];
    __shared__ unsigned long long part[4];
    unsigned long long e = 0;
    for (int i = threadIdx.x; i < w * h; i += 256) {
        const int r = i / w, cc = i - r * w;
        const long long v = c[i];
        if (r < kh && cc < kw) keep[r * kw + cc] = (int32_t)v;
        else e += (unsigned long long)(v * v);
    }
    e = group_sum64<64>(e);
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = e;
    __syncthreads();
    for (int i = threadIdx.x; i < w * h; i += 256) c[i] = i < kw * kh ? keep[i] : 0;
    if (threadIdx.x == 0 && energy) energy[blk] = part[0] + part[1] + part[2] + part[3];
}

// ---- the launches of the kernels that are built per size: grid, threads and variant are the plan's ----
template <int W, int H>
int launch_fwd(const TxPlan& p, const int16_t* in, uint32_t in_stride, size_t pitch, int32_t* out, uint32_t n, int tx_type, hipStream_t s) {
    PLAN_LAUNCH((fwd_txfm2d_kernel<W, H>), in, out, in_stride, pitch, tx_type, n);
    return launch_status("fwd_txfm2d");
}
template <int W, int H>
int launch_fwd_staged(const TxPlan& p, const int16_t* in, int32_t* out, uint32_t n, int tx_type, hipStream_t s) {
    QParams qp = {};
    PLAN_LAUNCH((fwd_staged_kernel<W, H, 0>), (const void*)in, (const uint8_t*)nullptr, out, (int32_t*)nullptr, (int32_t*)nullptr, (uint16_t*)nullptr,
                (uint32_t*)nullptr, (unsigned long long*)nullptr, (const int16_t*)nullptr, qp, tx_type, n);
    return launch_status("fwd_staged");
}
template <int W, int H>
int launch_inv_staged(const TxPlan& p, const int32_t* in, void* dst, uint32_t n, int tx_type, const uint32_t* offs, int32_t stride, hipStream_t s) {
    constexpr bool T16 = W >= 64 || H >= 64;      // (the plan's t16, a template argument here)
    if (p.is16) PLAN_LAUNCH((inv_staged_kernel<W, H, uint16_t, T16>), in, (uint16_t*)dst, tx_type, p.bd, n, offs, stride);
    else PLAN_LAUNCH((inv_staged_kernel<W, H, uint8_t, T16>), in, (uint8_t*)dst, tx_type, p.bd, n, offs, stride);
    return launch_status("inv_staged");
}
template <int W, int H>
int launch_inv(const TxPlan& p, const int32_t* in, void* dst, int32_t stride, size_t pitch, const uint32_t* offs, uint32_t n, int tx_type, hipStream_t s) {
    if (p.wide) PLAN_LAUNCH((inv_txfm2d_add_kernel<W, H, uint16_t, true>), in, (uint16_t*)dst, stride, pitch, offs, tx_type, p.bd, n);
    else if (p.is16) PLAN_LAUNCH((inv_txfm2d_add_kernel<W, H, uint16_t>), in, (uint16_t*)dst, stride, pitch, offs, tx_type, p.bd, n);
    else PLAN_LAUNCH((inv_txfm2d_add_kernel<W, H, uint8_t>), in, (uint8_t*)dst, stride, pitch, offs, tx_type, p.bd, n);
    return launch_status("inv_txfm2d_add");
}
// the outputs of the forward + quantise kernels
struct FqOut { int32_t *coeff, *qcoeff, *dqcoeff; uint16_t* eob; uint32_t* sad; uint64_t* energy; };
template <int W, int H>
int launch_fq_staged(const TxPlan& p, const void* src, const void* pred, const uint32_t* xy, uint32_t n, int tx_type, const int16_t* iscan, const FqOut& o, hipStream_t s) {
    if (p.is16)
        PLAN_LAUNCH((fwd_staged_kernel<W, H, 1, uint16_t>), src, pred, o.coeff, o.qcoeff, o.dqcoeff, o.eob, o.sad, (unsigned long long*)o.energy, iscan, p.qp, tx_type, n, xy,
                    p.src_stride, p.pred_stride);
    else
        PLAN_LAUNCH((fwd_staged_kernel<W, H, 1, uint8_t>), src, pred, o.coeff, o.qcoeff, o.dqcoeff, o.eob, o.sad, (unsigned long long*)o.energy, iscan, p.qp, tx_type, n, xy,
                    p.src_stride, p.pred_stride);
    return launch_status("fwd_quant_staged");
}
template <int W, int H>
int launch_fq(const TxPlan& p, const void* src, const void* pred, const uint32_t* xy, uint32_t n, int tx_type, const int16_t* iscan, const FqOut& o, hipStream_t s) {
    if (p.is16)
        PLAN_LAUNCH((fwd_quant_generic_kernel<W, H, uint16_t>), (const uint16_t*)src, p.src_stride, (size_t)W * H, (const uint16_t*)pred, p.pred_stride, (size_t)W * H, xy,
                    tx_type, p.qp, iscan, o.coeff, o.qcoeff, o.dqcoeff, o.eob, o.sad, (unsigned long long*)o.energy, n);
    else
        PLAN_LAUNCH((fwd_quant_generic_kernel<W, H, uint8_t>), (const uint8_t*)src, p.src_stride, (size_t)W * H, (const uint8_t*)pred, p.pred_stride, (size_t)W * H, xy,
                    tx_type, p.qp, iscan, o.coeff, o.qcoeff, o.dqcoeff, o.eob, o.sad, (unsigned long long*)o.energy, n);
    return launch_status("fwd_quant_generic");
}
// the operands of an encode-pass launch
struct EncArgs {
    const void *src, *pred; void* recon; const uint32_t* xy; uint32_t src_stride, pred_stride, recon_stride;
    const int16_t* iscan; int32_t *coeff, *qcoeff, *dqcoeff; uint16_t* eob; uint32_t* sad;
};
template <int W, int H>
int launch_enc_staged(const TxPlan& p, const EncArgs& a, uint32_t n, int tx_type, hipStream_t s) {
#define ENCL(KEEP, T, B) PLAN_LAUNCH((enc_staged_kernel<W, H, KEEP, T, B>), (const T*)a.src, (const T*)a.pred, (T*)a.recon, a.coeff, a.qcoeff, a.dqcoeff, a.eob, a.sad, \
                                     a.iscan, p.qp, tx_type, n, a.xy, a.src_stride, a.pred_stride, a.recon_stride)
    if (p.is16) { if (p.keep) ENCL(true, uint16_t, 10); else ENCL(false, uint16_t, 10); }
    else { if (p.keep) ENCL(true, uint8_t, 8); else ENCL(false, uint8_t, 8); }
#undef ENCL
    return launch_status("encode_recon_staged");
}

// ---- one switch per plan: the stages of the composed routes are planned by the same functions and launched here too ----
int run_fwd(const TxPlan& p, const int16_t* d_in, uint32_t in_stride, size_t in_block_pitch, int32_t* d_out, uint32_t n, int tx_size, int tx_type, hipStream_t s) {
    switch (p.route) {
    case TXR_FWD32: {
        QParams qp = {};
        PLAN_LAUNCH((fwd32_kernel<0, false, false>), (const void*)d_in, (const uint8_t*)nullptr, d_out, (int32_t*)nullptr, (int32_t*)nullptr, (uint16_t*)nullptr,
                    (uint32_t*)nullptr, (const int16_t*)nullptr, qp, p.idtx, n);
        return launch_status("fwd32");
    }
    case TXR_FWD_STAGED: {
#define CALLS(W, H) launch_fwd_staged<W, H>(p, d_in, d_out, n, tx_type, s)
        TX_SWITCH(tx_size, CALLS)
#undef CALLS
    }
    default: {
#define CALL(W, H) launch_fwd<W, H>(p, d_in, in_stride, in_block_pitch, d_out, n, tx_type, s)
        TX_SWITCH(tx_size, CALL)
#undef CALL
    }
    }
}
int run_inv(const TxPlan& p, const int32_t* d_coeff, void* d_dst, int32_t dst_stride, size_t dst_block_pitch, const uint32_t* d_dst_offsets, uint32_t n, int tx_size,
            int tx_type, hipStream_t s) {
    switch (p.route) {      // (the order the kernels are first named in is their order in the code object: as it was)
    case TXR_INV_GENERAL: {
#define CALL(W, H) launch_inv<W, H>(p, d_coeff, d_dst, dst_stride, dst_block_pitch, d_dst_offsets, n, tx_type, s)
        TX_SWITCH(tx_size, CALL)
#undef CALL
    }
    case TXR_INV32_PROBE:      // tuning probes (tools/tune_inv32.py)
#define INVV(WV, VR) if (p.wv == WV && p.vr == VR) PLAN_LAUNCH((inv32_kernel<uint8_t, 8, WV, VR>), d_coeff, (uint8_t*)d_dst, dst_stride, dst_block_pitch, d_dst_offsets, p.idtx, n);
        INVV(4, 1) INVV(4, 2) INVV(4, 4) INVV(4, 5) INVV(2, 0) INVV(4, 8)
#undef INVV
        return launch_status("inv32 probe");
    case TXR_INV32:
#define INV32(T, B) PLAN_LAUNCH((inv32_kernel<T, B>), d_coeff, (T*)d_dst, dst_stride, dst_block_pitch, d_dst_offsets, p.idtx, n)
        if (p.is16) { if (p.bd == 8) INV32(uint16_t, 8); else INV32(uint16_t, 10); }
        else INV32(uint8_t, 8);
#undef INV32
        return launch_status("inv32");
    default: {      // TXR_INV_STAGED
#define CALLS(W, H) launch_inv_staged<W, H>(p, d_coeff, d_dst, n, tx_type, d_dst_offsets, dst_stride, s)
        TX_SWITCH(tx_size, CALLS)
#undef CALLS
    }
    }
}
int run_quantize(const TxPlan& p, const int32_t* d_coeff, int n_coeffs, int skip_block, int32_t* d_qcoeff, int32_t* d_dqcoeff, uint16_t* d_eob, const int16_t* d_iscan,
                 uint32_t n, hipStream_t s) {
#define QL(L) case L: PLAN_LAUNCH((quantize_b_kernel<L>), d_coeff, d_qcoeff, d_dqcoeff, d_eob, d_iscan, p.qp, n_coeffs, skip_block, n); break;
    switch (p.lanes) { QL(4) QL(8) QL(16) QL(32) QL(64) }
#undef QL
    return launch_status("quantize_b");
}
int launch_fq32(const TxPlan& p, const void* d_src, const void* d_pred, uint32_t n, const int16_t* d_iscan, const FqOut& o, hipStream_t s) {
#define F32Q(SAD, NT, QM) PLAN_LAUNCH((fwd32_kernel<1, true, SAD, NT, QM>), d_src, d_pred, o.coeff, o.qcoeff, o.dqcoeff, o.eob, o.sad, d_iscan, p.qp, p.idtx, n)
#define F32Q_SAD(NT, QM) do { if (p.sad) F32Q(true, NT, QM); else F32Q(false, NT, QM); } while (0)
    if (p.nt) { if (p.qmode == 2) F32Q_SAD(true, 2); else F32Q_SAD(true, 1); }
    else { if (p.qmode != 2) F32Q_SAD(false, 1); else F32Q_SAD(false, 2); }
#undef F32Q_SAD
#undef F32Q
    return launch_status("fwd_quant_sad_32x32");
}
// (defined behind the encode pass: see run_inv on the order)
int run_fq(const TxPlan& p, const void* d_src, const void* d_pred, const uint32_t* d_xy, uint32_t n, int tx_size, int tx_type, const int16_t* d_iscan, const FqOut& o,
           hipStream_t s);
}  // namespace

// ===========================================================================
// (B) batched API
// ===========================================================================
extern "C" int svt_hip_fwd_txfm2d_batch(const int16_t* d_in, uint32_t in_stride, size_t in_block_pitch,
                                        int32_t* d_out, size_t nblocks, int tx_size, int tx_type, int bd,
                                        void* stream) {
    if (int rc = require_init()) return rc;
    if (nblocks == 0) return SVT_HIP_OK;
    if (!d_in || !d_out) return set_err(SVT_HIP_ERR_INVALID, "NULL buffer");
    TxPlan p;
    if (int rc = fwd_plan(tx_size, tx_type, bd, in_stride, in_block_pitch, nblocks, aligned16(d_in, d_out), tx_knobs(), p)) return rc;
    return run_fwd(p, d_in, in_stride, in_block_pitch, d_out, (uint32_t)nblocks, tx_size, tx_type, (hipStream_t)stream);
}

extern "C" int svt_hip_pack64_batch(int32_t* d_coeff, uint64_t* d_energy, size_t nblocks, int tx_size,
                                    void* stream) {
    if (int rc = require_init()) return rc;
    if (nblocks == 0) return SVT_HIP_OK;
    if (!d_coeff) return set_err(SVT_HIP_ERR_INVALID, "bad argument");
    TxPlan p;
    if (int rc = pack64_plan(tx_size, nblocks, p)) return rc;
    hipStream_t s = (hipStream_t)stream;
    if (p.route == TXR_PACK64_NONE) {
        if (d_energy) HIP_TRY(hipMemsetAsync(d_energy, 0, nblocks * sizeof(uint64_t), s));
        return SVT_HIP_OK;
    }
    PLAN_LAUNCH(pack64_kernel, d_coeff, (unsigned long long*)d_energy, kTxW[tx_size], kTxH[tx_size], (uint32_t)nblocks);
    return launch_status("pack64");
}

extern "C" int svt_hip_inv_txfm2d_add_batch(const int32_t* d_coeff, void* d_dst, int dst_is_16bit,
                                            int32_t dst_stride, size_t dst_block_pitch,
                                            const uint32_t* d_dst_offsets, size_t nblocks, int tx_size,
                                            int tx_type, int bd, void* stream) {
    if (int rc = require_init()) return rc;
    if (nblocks == 0) return SVT_HIP_OK;
    if (!d_coeff || !d_dst) return set_err(SVT_HIP_ERR_INVALID, "NULL buffer");
    TxPlan p;
    if (int rc = inv_plan(tx_size, tx_type, bd, dst_is_16bit, dst_stride, dst_block_pitch, d_dst_offsets != nullptr, nblocks, aligned16(d_coeff), aligned16(d_dst),
                          tx_knobs(), p)) return rc;
    return run_inv(p, d_coeff, d_dst, dst_stride, dst_block_pitch, d_dst_offsets, (uint32_t)nblocks, tx_size, tx_type, (hipStream_t)stream);
}

extern "C" int svt_hip_quantize_b_batch(const int32_t* d_coeff, size_t n_coeffs, int skip_block,
                                        const int16_t* zbin, const int16_t* round, const int16_t* quant,
                                        const int16_t* quant_shift, int32_t* d_qcoeff, int32_t* d_dqcoeff,
                                        const int16_t* dequant, uint16_t* d_eob, const int16_t* d_iscan,
                                        int log_scale, size_t nblocks, void* stream) {
    if (int rc = require_init()) return rc;
    if (nblocks == 0) return SVT_HIP_OK;
    if (!d_coeff || !d_qcoeff || !d_dqcoeff || !d_eob || !d_iscan || !zbin || !round || !quant || !quant_shift || !dequant)
        return set_err(SVT_HIP_ERR_INVALID, "NULL argument");
    TxPlan p;
    if (int rc = quantize_plan(n_coeffs, log_scale, svt_hip_qrows{zbin, round, quant, quant_shift, dequant}, nblocks, p)) return rc;
    return run_quantize(p, d_coeff, (int)n_coeffs, skip_block, d_qcoeff, d_dqcoeff, d_eob, d_iscan, (uint32_t)nblocks, (hipStream_t)stream);
}

extern "C" int svt_hip_fwd_quant_sad_batch(const uint8_t* d_src, const uint8_t* d_pred, size_t nblocks,
                                           int tx_size, int tx_type, const int16_t* zbin, const int16_t* round,
                                           const int16_t* quant, const int16_t* quant_shift,
                                           const int16_t* dequant, const int16_t* d_iscan, int32_t* d_coeff,
                                           int32_t* d_qcoeff, int32_t* d_dqcoeff, uint16_t* d_eob,
                                           uint32_t* d_sad, void* stream) {
    if (int rc = require_init()) return rc;
    if (nblocks == 0) return SVT_HIP_OK;
    if (!d_src || !d_pred || !d_coeff || !d_qcoeff || !d_dqcoeff || !d_eob || !d_iscan || !zbin || !round || !quant || !quant_shift || !dequant)
        return set_err(SVT_HIP_ERR_INVALID, "NULL argument");
    TxPlan p;
    if (int rc = fq_sad_plan(tx_size, tx_type, d_sad != nullptr, svt_hip_qrows{zbin, round, quant, quant_shift, dequant}, nblocks, aligned16(d_src, d_pred),
                             aligned16(d_coeff, d_qcoeff, d_dqcoeff), tx_knobs(), g_num_cu, p)) return rc;
    return run_fq(p, d_src, d_pred, nullptr, (uint32_t)nblocks, tx_size, tx_type, d_iscan, FqOut{d_coeff, d_qcoeff, d_dqcoeff, d_eob, d_sad, nullptr}, (hipStream_t)stream);
}

static int encode_recon_impl(const void* d_src, uint32_t src_stride, const void* d_pred, uint32_t pred_stride,
                             void* d_recon, uint32_t recon_stride, const uint32_t* d_xy, int is_16bit, int bd, size_t nblocks, int tx_size,
                             int tx_type, const int16_t* zbin, const int16_t* round, const int16_t* quant,
                             const int16_t* quant_shift, const int16_t* dequant, const int16_t* d_iscan,
                             int32_t* d_coeff, int32_t* d_qcoeff, int32_t* d_dqcoeff, uint16_t* d_eob,
                             uint32_t* d_sad, void* stream) {
    if (int rc = require_init()) return rc;
    if (nblocks == 0) return SVT_HIP_OK;
    if (!d_src || !d_pred || !d_qcoeff || !d_eob || !d_recon || !d_iscan || !zbin || !round || !quant || !quant_shift || !dequant)
        return set_err(SVT_HIP_ERR_INVALID, "NULL argument");
    TxPlan p, stage[2];
    if (int rc = encode_recon_plan(tx_size, tx_type, is_16bit, bd, d_xy != nullptr, d_coeff != nullptr, d_dqcoeff != nullptr, d_sad != nullptr,
                                   d_recon == d_src || (!d_xy && d_recon == d_pred), svt_hip_qrows{zbin, round, quant, quant_shift, dequant}, nblocks,
                                   EncAligned{aligned16(d_src, d_pred), aligned16(d_recon), aligned16(d_qcoeff, d_coeff, d_dqcoeff), aligned16(d_dqcoeff)}, tx_knobs(),
                                   g_num_cu, p, stage)) return rc;
    hipStream_t s = (hipStream_t)stream;
    const uint32_t n = (uint32_t)nblocks;
    const EncArgs a = {d_src, d_pred, d_recon, d_xy, src_stride, pred_stride, recon_stride, d_iscan, d_coeff, d_qcoeff, d_dqcoeff, d_eob, d_sad};
#define ENC_ARGS(T) (const T*)d_src, (const T*)d_pred, (T*)d_recon, d_coeff, d_qcoeff, d_dqcoeff, d_eob, d_sad, d_iscan, p.qp
#define ENC_PLANES d_xy, src_stride, pred_stride, recon_stride
    switch (p.route) {
    case TXR_ENC32:
#define ENC32(T, B, KEEP, SAD) PLAN_LAUNCH((enc32_kernel<T, B, KEEP, SAD>), ENC_ARGS(T), p.idtx, n, ENC_PLANES)
        if (p.is16) { if (p.keep) ENC32(uint16_t, 10, true, false); else ENC32(uint16_t, 10, false, false); }
        else if (p.keep) { if (p.sad) ENC32(uint8_t, 8, true, true); else ENC32(uint8_t, 8, true, false); }
        else { if (p.sad) ENC32(uint8_t, 8, false, true); else ENC32(uint8_t, 8, false, false); }
#undef ENC32
        return launch_status("encode_recon_32x32");
    case TXR_ENC4:
#define ENC4(T, B, KEEP) PLAN_LAUNCH((enc4_kernel<T, B, KEEP>), ENC_ARGS(T), p.fast ? 1 : 0, tx_type, n, ENC_PLANES)
        if (p.is16) { if (p.keep) ENC4(uint16_t, 10, true); else ENC4(uint16_t, 10, false); }
        else { if (p.keep) ENC4(uint8_t, 8, true); else ENC4(uint8_t, 8, false); }
#undef ENC4
        return launch_status("encode_recon_4x4");
    case TXR_ENC64:
#define ENC64(T, B, KEEP, SAD) PLAN_LAUNCH((enc64_kernel<T, B, KEEP, SAD>), ENC_ARGS(T), n, ENC_PLANES)
        if (p.is16) { if (p.keep) ENC64(uint16_t, 10, true, true); else if (p.sad) ENC64(uint16_t, 10, false, true); else ENC64(uint16_t, 10, false, false); }
        else { if (p.keep) ENC64(uint8_t, 8, true, true); else if (p.sad) ENC64(uint8_t, 8, false, true); else ENC64(uint8_t, 8, false, false); }
#undef ENC64
        return launch_status("encode_recon_64x64");
    case TXR_ENC_STAGED: {
#define ENCS(W, H) launch_enc_staged<W, H>(p, a, n, tx_type, s)
        TX_SWITCH(tx_size, ENCS)
#undef ENCS
    }
    default: break;
    }
#undef ENC_ARGS
#undef ENC_PLANES
    // TXR_ENC_COMPOSED: the two batched stages around a device copy of the prediction
    if (int rc = run_fq(stage[0], d_src, d_pred, nullptr, n, tx_size, tx_type, d_iscan, FqOut{d_coeff, d_qcoeff, d_dqcoeff, d_eob, d_sad, nullptr}, s)) return rc;
    const size_t pels = (size_t)kTxW[tx_size] * kTxH[tx_size];
    HIP_TRY(hipMemcpyAsync(d_recon, d_pred, pels * nblocks, hipMemcpyDeviceToDevice, s));
    return run_inv(stage[1], d_dqcoeff, d_recon, kTxW[tx_size], pels, nullptr, n, tx_size, tx_type, s);
}

extern "C" int svt_hip_encode_recon_batch(const uint8_t* d_src, const uint8_t* d_pred, size_t nblocks, int tx_size,
                                          int tx_type, const int16_t* zbin, const int16_t* round, const int16_t* quant,
                                          const int16_t* quant_shift, const int16_t* dequant, const int16_t* d_iscan,
                                          int32_t* d_coeff, int32_t* d_qcoeff, int32_t* d_dqcoeff, uint16_t* d_eob,
                                          uint32_t* d_sad, uint8_t* d_recon, void* stream) {
    return encode_recon_impl(d_src, 0, d_pred, 0, d_recon, 0, nullptr, 0, 8, nblocks, tx_size, tx_type, zbin, round, quant, quant_shift,
                             dequant, d_iscan, d_coeff, d_qcoeff, d_dqcoeff, d_eob, d_sad, stream);
}
extern "C" int svt_hip_encode_recon_planes_batch(const void* d_src, uint32_t src_stride, const void* d_pred,
                                                 uint32_t pred_stride, void* d_recon, uint32_t recon_stride,
                                                 const uint32_t* d_xy, size_t nblocks, int is_16bit, int bd, int tx_size, int tx_type,
                                                 const int16_t* zbin, const int16_t* round, const int16_t* quant,
                                                 const int16_t* quant_shift, const int16_t* dequant, const int16_t* d_iscan,
                                                 int32_t* d_coeff, int32_t* d_qcoeff, int32_t* d_dqcoeff, uint16_t* d_eob,
                                                 uint32_t* d_sad, void* stream) {
    if (nblocks && !d_xy) { if (int rc = require_init()) return rc; return set_err(SVT_HIP_ERR_INVALID, "NULL origin table"); }
    return encode_recon_impl(d_src, src_stride, d_pred, pred_stride, d_recon, recon_stride, d_xy, is_16bit, bd, nblocks, tx_size, tx_type, zbin,
                             round, quant, quant_shift, dequant, d_iscan, d_coeff, d_qcoeff, d_dqcoeff, d_eob, d_sad, stream);
}

namespace {
int run_fq(const TxPlan& p, const void* d_src, const void* d_pred, const uint32_t* d_xy, uint32_t n, int tx_size, int tx_type, const int16_t* d_iscan, const FqOut& o,
           hipStream_t s) {
    switch (p.route) {
    case TXR_FQ32: return launch_fq32(p, d_src, d_pred, n, d_iscan, o, s);
    case TXR_FQ32_PLANES:
#define F32P(INM, SAD, PL) PLAN_LAUNCH((fwd32_kernel<INM, true, SAD, false, 2, PL>), d_src, d_pred, o.coeff, o.qcoeff, o.dqcoeff, o.eob, o.sad, d_iscan, p.qp, p.idtx, n, \
                                       p.src_stride, p.pred_stride, d_xy)
        if (p.is16) { if (p.planes) F32P(2, false, true); else F32P(2, false, false); }
        else { if (p.sad) F32P(1, true, true); else F32P(1, false, true); }
#undef F32P
        return launch_status("fwd_quant_32x32_planes");
    case TXR_FQ64:
        if (p.is16)
            PLAN_LAUNCH((fq64_kernel<uint16_t, 10>), (const uint16_t*)d_src, (const uint16_t*)d_pred, o.coeff, o.qcoeff, o.dqcoeff, o.eob, o.sad, d_iscan, p.qp, n, d_xy,
                        p.src_stride, p.pred_stride);
        else
            PLAN_LAUNCH((fq64_kernel<uint8_t, 8>), (const uint8_t*)d_src, (const uint8_t*)d_pred, o.coeff, o.qcoeff, o.dqcoeff, o.eob, o.sad, d_iscan, p.qp, n, d_xy,
                        p.src_stride, p.pred_stride);
        return launch_status("fwd_quant_64x64");
    case TXR_FQ_STAGED: {
#define CALLS(W, H) launch_fq_staged<W, H>(p, d_src, d_pred, d_xy, n, tx_type, d_iscan, o, s)
        TX_SWITCH(tx_size, CALLS)
#undef CALLS
    }
    default: {
#define CALL(W, H) launch_fq<W, H>(p, d_src, d_pred, d_xy, n, tx_type, d_iscan, o, s)
        TX_SWITCH(tx_size, CALL)
#undef CALL
    }
    }
}
}  // namespace

extern "C" int svt_hip_fwd_quant_planes_batch(const void* d_src, uint32_t src_stride, const void* d_pred,
                                              uint32_t pred_stride, const uint32_t* d_xy, size_t nblocks, int is_16bit,
                                              int bd, int tx_size, int tx_type, const int16_t* zbin, const int16_t* round,
                                              const int16_t* quant, const int16_t* quant_shift, const int16_t* dequant,
                                              const int16_t* d_iscan, int32_t* d_coeff, int32_t* d_qcoeff,
                                              int32_t* d_dqcoeff, uint16_t* d_eob, uint32_t* d_sad, uint64_t* d_energy,
                                              void* stream) {
    if (int rc = require_init()) return rc;
    if (nblocks == 0) return SVT_HIP_OK;
    if (!d_src || !d_pred || !d_coeff || !d_qcoeff || !d_dqcoeff || !d_eob || !d_iscan || !zbin || !round || !quant || !quant_shift || !dequant)
        return set_err(SVT_HIP_ERR_INVALID, "NULL argument");
    TxPlan p;
    if (int rc = fq_planes_plan(tx_size, tx_type, is_16bit, bd, src_stride, pred_stride, d_xy != nullptr, d_sad != nullptr, d_energy != nullptr,
                                svt_hip_qrows{zbin, round, quant, quant_shift, dequant}, nblocks, aligned16(d_src, d_pred), aligned16(d_coeff, d_qcoeff, d_dqcoeff),
                                tx_knobs(), p)) return rc;
    return run_fq(p, d_src, d_pred, d_xy, (uint32_t)nblocks, tx_size, tx_type, d_iscan, FqOut{d_coeff, d_qcoeff, d_dqcoeff, d_eob, d_sad, d_energy}, (hipStream_t)stream);
}

// ---- frame-level call: the group tables of tx_plan.h's frame_plan, or independent groups fanned out on internal streams, forked from and joined into the caller's stream ----
extern "C" int svt_hip_encode_recon_frame(const svt_hip_frame_group* groups, int ngroups, int is_16bit, int bd,
                                          const int16_t* zbin, const int16_t* round, const int16_t* quant,
                                          const int16_t* quant_shift, const int16_t* dequant, void* stream) {
    if (int rc = require_init()) return rc;
    if (ngroups == 0) return SVT_HIP_OK;
    if (int rc = frame_groups_check(groups, ngroups, tx_knobs())) return rc;            // validate everything before anything is enqueued
    FramePlan fp;
    frame_plan(groups, ngroups, is_16bit, bd, svt_hip_qrows{zbin, round, quant, quant_shift, dequant}, tx_knobs(), fp);
    if (fp.tables) {
        // one table per class (kFrameOneLaunchTable: the one launch), its groups largest blocks first: the long workgroups start early
        GroupTable<FrameDesc, FRAME_MAX_GROUPS, true> tab[4];
        for (int g = 0; g < ngroups; g++) {
            const svt_hip_frame_group& G = groups[g];
            if (G.nblocks == 0) continue;
            FrameGroupDev* D = tab[fp.g[g].table].add(fp.g[g].wgs, (uint64_t)(kTxW[G.tx_size] * kTxH[G.tx_size]));
            if (!D) return set_err(SVT_HIP_ERR_RUNTIME, "frame plan and group table disagree");
            D->qp = fp.qp[fp.g[g].log_scale];
            D->src = G.d_src; D->pred = G.d_pred; D->recon = G.d_recon; D->qcoeff = G.d_qcoeff; D->eob = G.d_eob; D->xy = G.d_xy; D->iscan = G.d_iscan;
            D->src_stride = G.src_stride; D->pred_stride = G.pred_stride; D->recon_stride = G.recon_stride; D->nblocks = G.nblocks; D->tx_size = G.tx_size; D->tx_type = G.tx_type;
        }
        hipStream_t hs = (hipStream_t)stream;
        if (int rc = tab[kFrameOneLaunchTable].flush([&](const FrameDesc& fd, uint32_t total) { return launch_enc_frame_one(&fd, total, is_16bit, hs); })) return rc;      // (svt_hip_frame.hip)
        // (class launches: the 64x64 class first, the small sizes last)
#define FRAME_LAUNCH(C)                                                                                                                 \
        if (int rc = tab[C].flush([&](const FrameDesc& fd, uint32_t total) {                                                            \
                if (is_16bit) hipLaunchKernelGGL((enc_frame_kernel<uint16_t, 10, C>), dim3(total), dim3(256), 0, hs, fd);               \
                else hipLaunchKernelGGL((enc_frame_kernel<uint8_t, 8, C>), dim3(total), dim3(256), 0, hs, fd);                          \
                return launch_status("enc_frame");                                                                                      \
            })) return rc;
        FRAME_LAUNCH(2) FRAME_LAUNCH(1) FRAME_LAUNCH(0)
#undef FRAME_LAUNCH
        return SVT_HIP_OK;
    }
    if (int rc = t_fan.ensure()) return rc;
    hipStream_t s = (hipStream_t)stream;
    const int nstreams = ngroups < kFanStreams ? ngroups : kFanStreams;
    // From the fork on nothing returns early: a side stream that has waited on the fork event must be joined back, or a
    // caller capturing this call into a graph is left with dangling branches.  Failures become rc and fall through to the join.
    HIP_TRY(hipEventRecord(t_fan.fork, s));
    int rc = SVT_HIP_OK, forked = 0;
    for (; forked < nstreams; forked++)
        if (hipStreamWaitEvent(t_fan.s[forked], t_fan.fork, 0) != hipSuccess) { rc = set_err(SVT_HIP_ERR_RUNTIME, "stream fork failed"); break; }
    // largest groups first, round-robin: the long kernels start early and the small ones fill in beside them
    int order[256];
    const int ng = ngroups;                        // <= 256, checked with the arguments
    order_largest_first(order, ng, [&](int i) {      // by work (pixels); an empty group's size is not validated
        return groups[i].nblocks ? (size_t)groups[i].nblocks * kTxW[groups[i].tx_size] * kTxH[groups[i].tx_size] : (size_t)0;
    });
    for (int k = 0; k < ng && rc == SVT_HIP_OK; k++) {
        const svt_hip_frame_group& G = groups[order[k]];
        if (G.nblocks == 0) continue;
        hipStream_t gs = t_fan.s[k % nstreams];
        if (G.tx_size == SVT_TX_4X4 && g_tune_no_enc_staged) {
            rc = svt_hip_fwd_quant_planes_batch(G.d_src, G.src_stride, G.d_pred, G.pred_stride, G.d_xy, G.nblocks, is_16bit, bd, G.tx_size, G.tx_type,
                                                zbin, round, quant, quant_shift, dequant, G.d_iscan, G.d_coeff, G.d_qcoeff, G.d_dqcoeff, G.d_eob,
                                                nullptr, nullptr, gs);
            if (rc == SVT_HIP_OK)
                rc = svt_hip_inv_txfm2d_add_batch(G.d_dqcoeff, G.d_recon, is_16bit, (int32_t)G.recon_stride, 0, G.d_offsets, G.nblocks, G.tx_size,
                                                  G.tx_type, bd, gs);
        } else {
            rc = encode_recon_impl(G.d_src, G.src_stride, G.d_pred, G.pred_stride, G.d_recon, G.recon_stride, G.d_xy, is_16bit, bd, G.nblocks,
                                   G.tx_size, G.tx_type, zbin, round, quant, quant_shift, dequant, G.d_iscan, G.d_coeff, G.d_qcoeff, G.d_dqcoeff,
                                   G.d_eob, nullptr, gs);
        }
    }
    // always join, also after an error: the caller's stream (or capture) must not be left with dangling branches
    for (int i = 0; i < forked; i++) {
        if (hipEventRecord(t_fan.join[i], t_fan.s[i]) != hipSuccess || hipStreamWaitEvent(s, t_fan.join[i], 0) != hipSuccess)
            if (rc == SVT_HIP_OK) rc = set_err(SVT_HIP_ERR_RUNTIME, "stream join failed");
    }
    return rc;
}

extern "C" int svt_hip_fwd_quant_batch(const int16_t* d_residual, size_t nblocks, int tx_size, int tx_type, int bd,
                                       const int16_t* zbin, const int16_t* round, const int16_t* quant,
                                       const int16_t* quant_shift, const int16_t* dequant, const int16_t* d_iscan,
                                       int32_t* d_coeff, int32_t* d_qcoeff, int32_t* d_dqcoeff, uint16_t* d_eob,
                                       void* stream) {
    if (int rc = require_init()) return rc;
    if (nblocks == 0) return SVT_HIP_OK;
    if (!d_residual || !d_coeff || !d_qcoeff || !d_dqcoeff || !d_eob || !d_iscan || !zbin || !round || !quant || !quant_shift || !dequant)
        return set_err(SVT_HIP_ERR_INVALID, "NULL argument");
    TxPlan p, stage[2];
    if (int rc = fwd_quant_plan(tx_size, tx_type, bd, svt_hip_qrows{zbin, round, quant, quant_shift, dequant}, nblocks, aligned16(d_residual), aligned16(d_coeff),
                                tx_knobs(), p, stage)) return rc;
    hipStream_t s = (hipStream_t)stream;
    const uint32_t n = (uint32_t)nblocks;
    if (p.route == TXR_FWD32_QUANT) {
        PLAN_LAUNCH((fwd32_kernel<0, true, false>), (const void*)d_residual, (const uint8_t*)nullptr, d_coeff, d_qcoeff, d_dqcoeff, d_eob, (uint32_t*)nullptr, d_iscan, p.qp,
                    p.idtx, n);
        return launch_status("fwd32_quant");
    }
    // TXR_FWD_THEN_QUANT: transform into d_coeff, quantise (two more passes over d_coeff)
    const int w = kTxW[tx_size], h = kTxH[tx_size];
    if (int rc = run_fwd(stage[0], d_residual, (uint32_t)w, (size_t)w * h, d_coeff, n, tx_size, tx_type, s)) return rc;
    return run_quantize(stage[1], d_coeff, w * h, 0, d_qcoeff, d_dqcoeff, d_eob, d_iscan, n, s);
}
#undef PLAN_LAUNCH

// ===========================================================================
static void dropin_fwd(int tx_size, int16_t* input, int32_t* output, uint32_t stride, uint8_t tx_type, uint8_t bd,
                       const char* fn) {
    const int w = kTxW[tx_size], h = kTxH[tx_size];
    const size_t in_b = align256((size_t)w * h * 2), out_b = (size_t)w * h * 4;
    DROPIN_TRY(t_ctx.ensure(in_b + out_b), fn);
    int16_t* d_in = (int16_t*)t_ctx.dbuf;
    int32_t* d_out = (int32_t*)(t_ctx.dbuf + in_b);
    HIP_DIE(hipMemcpy2DAsync(d_in, (size_t)w * 2, input, (size_t)stride * 2, (size_t)w * 2, h, hipMemcpyHostToDevice, t_ctx.stream), fn);
    DROPIN_TRY(svt_hip_fwd_txfm2d_batch(d_in, (uint32_t)w, (size_t)w * h, d_out, 1, tx_size, tx_type, bd, t_ctx.stream), fn);
    HIP_DIE(hipMemcpyAsync(output, d_out, out_b, hipMemcpyDeviceToHost, t_ctx.stream), fn);
    HIP_DIE(hipStreamSynchronize(t_ctx.stream), fn);
}
#define DEF_FWD(W, H, TS)                                                                                          \
    extern "C" void svt_hip_av1_fwd_txfm2d_##W##x##H(int16_t* input, int32_t* output, uint32_t input_stride,      \
                                                     svt_tx_type_t transform_type, uint8_t bit_depth) {           \
        dropin_fwd(TS, input, output, input_stride, transform_type, bit_depth, "svt_hip_av1_fwd_txfm2d_" #W "x" #H); \
    }
DEF_FWD(4, 4, SVT_TX_4X4) DEF_FWD(8, 8, SVT_TX_8X8) DEF_FWD(16, 16, SVT_TX_16X16) DEF_FWD(32, 32, SVT_TX_32X32)
DEF_FWD(64, 64, SVT_TX_64X64) DEF_FWD(4, 8, SVT_TX_4X8) DEF_FWD(8, 4, SVT_TX_8X4) DEF_FWD(8, 16, SVT_TX_8X16)
DEF_FWD(16, 8, SVT_TX_16X8) DEF_FWD(16, 32, SVT_TX_16X32) DEF_FWD(32, 16, SVT_TX_32X16) DEF_FWD(32, 64, SVT_TX_32X64)
DEF_FWD(64, 32, SVT_TX_64X32) DEF_FWD(4, 16, SVT_TX_4X16) DEF_FWD(16, 4, SVT_TX_16X4) DEF_FWD(8, 32, SVT_TX_8X32)
DEF_FWD(32, 8, SVT_TX_32X8) DEF_FWD(16, 64, SVT_TX_16X64) DEF_FWD(64, 16, SVT_TX_64X16)
#undef DEF_FWD

static void dropin_inv(int tx_size, const int32_t* input, void* output, int is16, int32_t stride, uint8_t tx_type,
                       int32_t bd, const char* fn) {
    const int w = kTxW[tx_size], h = kTxH[tx_size];
    const int kw = w > 32 ? 32 : w, kh = h > 32 ? 32 : h;
    const size_t es = is16 ? 2 : 1;
    const size_t in_b = align256((size_t)kw * kh * 4), px_b = (size_t)w * h * es;
    DROPIN_TRY(t_ctx.ensure(in_b + px_b), fn);
    int32_t* d_in = (int32_t*)t_ctx.dbuf;
    char* d_px = t_ctx.dbuf + in_b;
    HIP_DIE(hipMemcpyAsync(d_in, input, (size_t)kw * kh * 4, hipMemcpyHostToDevice, t_ctx.stream), fn);
    HIP_DIE(hipMemcpy2DAsync(d_px, (size_t)w * es, output, (size_t)stride * es, (size_t)w * es, h, hipMemcpyHostToDevice, t_ctx.stream), fn);
    DROPIN_TRY(svt_hip_inv_txfm2d_add_batch(d_in, d_px, is16, w, (size_t)w * h, nullptr, 1, tx_size, tx_type, bd, t_ctx.stream), fn);
    HIP_DIE(hipMemcpy2DAsync(output, (size_t)stride * es, d_px, (size_t)w * es, (size_t)w * es, h, hipMemcpyDeviceToHost, t_ctx.stream), fn);
    HIP_DIE(hipStreamSynchronize(t_ctx.stream), fn);
}
#define DEF_INV_SQ(W, H, TS)                                                                                       \
    extern "C" void svt_hip_av1_inv_txfm2d_add_##W##x##H(const int32_t* input, uint16_t* output, int32_t stride,  \
                                                         svt_tx_type_t tx_type, int32_t bd) {                     \
        dropin_inv(TS, input, output, 1, stride, tx_type, bd, "svt_hip_av1_inv_txfm2d_add_" #W "x" #H);           \
    }
#define DEF_INV_R1(W, H, TS)                                                                                       \
    extern "C" void svt_hip_av1_inv_txfm2d_add_##W##x##H(const int32_t* input, uint16_t* output, int32_t stride,  \
                                                         svt_tx_type_t tx_type, svt_tx_size_t, int32_t, int32_t bd) { \
        dropin_inv(TS, input, output, 1, stride, tx_type, bd, "svt_hip_av1_inv_txfm2d_add_" #W "x" #H);           \
    }
#define DEF_INV_R2(W, H, TS)                                                                                       \
    extern "C" void svt_hip_av1_inv_txfm2d_add_##W##x##H(const int32_t* input, uint16_t* output, int32_t stride,  \
                                                         svt_tx_type_t tx_type, svt_tx_size_t, int32_t bd) {      \
        dropin_inv(TS, input, output, 1, stride, tx_type, bd, "svt_hip_av1_inv_txfm2d_add_" #W "x" #H);           \
    }
DEF_INV_SQ(4, 4, SVT_TX_4X4) DEF_INV_SQ(8, 8, SVT_TX_8X8) DEF_INV_SQ(16, 16, SVT_TX_16X16)
DEF_INV_SQ(32, 32, SVT_TX_32X32) DEF_INV_SQ(64, 64, SVT_TX_64X64)
DEF_INV_R1(8, 16, SVT_TX_8X16) DEF_INV_R1(16, 8, SVT_TX_16X8) DEF_INV_R1(16, 32, SVT_TX_16X32)
DEF_INV_R1(32, 16, SVT_TX_32X16) DEF_INV_R1(32, 64, SVT_TX_32X64) DEF_INV_R1(64, 32, SVT_TX_64X32)
DEF_INV_R1(8, 32, SVT_TX_8X32) DEF_INV_R1(32, 8, SVT_TX_32X8) DEF_INV_R1(16, 64, SVT_TX_16X64)
DEF_INV_R1(64, 16, SVT_TX_64X16)
DEF_INV_R2(4, 8, SVT_TX_4X8) DEF_INV_R2(8, 4, SVT_TX_8X4) DEF_INV_R2(4, 16, SVT_TX_4X16) DEF_INV_R2(16, 4, SVT_TX_16X4)
#undef DEF_INV_SQ
#undef DEF_INV_R1
#undef DEF_INV_R2

extern "C" void svt_hip_av1_inv_txfm_add(const svt_tran_low_t* dqcoeff, uint8_t* dst, int32_t stride,
                                         const svt_txfm_param* p) {
    dropin_inv(p->tx_size, dqcoeff, dst, 0, stride, p->tx_type, 8, "svt_hip_av1_inv_txfm_add");
}

static void dropin_quant(int log_scale, const int32_t* coeff, intptr_t n, int32_t skip, const int16_t* zbin,
                         const int16_t* round, const int16_t* quant, const int16_t* qshift, int32_t* q, int32_t* dq,
                         const int16_t* dequant, uint16_t* eob, const int16_t* iscan, const char* fn) {
    const size_t cb = align256((size_t)n * 4), ib = align256((size_t)n * 2);
    DROPIN_TRY(t_ctx.ensure(3 * cb + ib + 256), fn);
    int32_t* d_c = (int32_t*)t_ctx.dbuf;
    int32_t* d_q = (int32_t*)(t_ctx.dbuf + cb);
    int32_t* d_dq = (int32_t*)(t_ctx.dbuf + 2 * cb);
    int16_t* d_is = (int16_t*)(t_ctx.dbuf + 3 * cb);
    uint16_t* d_eob = (uint16_t*)(t_ctx.dbuf + 3 * cb + ib);
    HIP_DIE(hipMemcpyAsync(d_c, coeff, (size_t)n * 4, hipMemcpyHostToDevice, t_ctx.stream), fn);
    HIP_DIE(hipMemcpyAsync(d_is, iscan, (size_t)n * 2, hipMemcpyHostToDevice, t_ctx.stream), fn);
    DROPIN_TRY(svt_hip_quantize_b_batch(d_c, (size_t)n, skip, zbin, round, quant, qshift, d_q, d_dq, dequant, d_eob, d_is, log_scale, 1, t_ctx.stream), fn);
    HIP_DIE(hipMemcpyAsync(q, d_q, (size_t)n * 4, hipMemcpyDeviceToHost, t_ctx.stream), fn);
    HIP_DIE(hipMemcpyAsync(dq, d_dq, (size_t)n * 4, hipMemcpyDeviceToHost, t_ctx.stream), fn);
    HIP_DIE(hipMemcpyAsync(eob, d_eob, 2, hipMemcpyDeviceToHost, t_ctx.stream), fn);
    HIP_DIE(hipStreamSynchronize(t_ctx.stream), fn);
}
#define DEF_QUANT(name, LS)                                                                                        \
    extern "C" void name(const svt_tran_low_t* coeff_ptr, intptr_t n_coeffs, int32_t skip_block,                  \
                         const int16_t* zbin_ptr, const int16_t* round_ptr, const int16_t* quant_ptr,             \
                         const int16_t* quant_shift_ptr, svt_tran_low_t* qcoeff_ptr, svt_tran_low_t* dqcoeff_ptr, \
                         const int16_t* dequant_ptr, uint16_t* eob_ptr, const int16_t* scan, const int16_t* iscan) { \
        (void)scan;                                                                                                \
        dropin_quant(LS, coeff_ptr, n_coeffs, skip_block, zbin_ptr, round_ptr, quant_ptr, quant_shift_ptr,         \
                     qcoeff_ptr, dqcoeff_ptr, dequant_ptr, eob_ptr, iscan, #name);                                 \
    }
DEF_QUANT(svt_hip_aom_highbd_quantize_b, 0)
DEF_QUANT(svt_hip_aom_highbd_quantize_b_32x32, 1)
DEF_QUANT(svt_hip_aom_highbd_quantize_b_64x64, 2)
DEF_QUANT(svt_hip_aom_quantize_b, 0)
DEF_QUANT(svt_hip_aom_quantize_b_32x32, 1)
DEF_QUANT(svt_hip_aom_quantize_b_64x64, 2)
#undef DEF_QUANT


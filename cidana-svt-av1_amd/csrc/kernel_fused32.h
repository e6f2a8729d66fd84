// kernel_fused32.h — tuned 32x32 kernels (the sizes the headline metric and
// BASELINE.json configs[1] are quoted on).
//
//   fwd32_kernel<IN, QUANT, WITH_SAD, ...>
//     uint8 in + QUANT + WITH_SAD   headline: residual(src,pred) -> FwdTxfm2d -> quantize_b_32x32 -> SAD
//     uint8 / uint16 in, PLANES     the same chain on picture planes (svt_hip_fwd_quant_planes_batch)
//     int16 in + QUANT              configs[1]: FwdTxfm2d + quantize on a residual batch
//     int16 in, no QUANT            plain av1_fwd_txfm2d_32x32
//   inv32_kernel<PixT, BD>          av1_inv_txfm2d_add_32x32 / av1_inv_txfm_add (8-bit recon)
//   enc32_body / enc32_kernel       the encode pass: forward chain + inverse + reconstruction in one kernel
//                                   (enc32_body is also a body of enc_frame_kernel, kernel_frame.h)
//
// Replaces, per block, the reference call sequence
//   ResidualKernel                (EbCodingLoop.c:617  -> EbPictureOperators.c:166)
//   av1_fwd_txfm2d_32x32          (EbFullLoop.c:763    -> EbTransforms.c:4466 / AVX2 :4080)
//   aom_highbd_quantize_b_32x32   (EbFullLoop.c:780    -> EbFullLoop.c:239 / AVX2 :422)
//   NxMSadKernel 32x32            (EbProductCodingLoop.c:1259 -> EbComputeSAD_C.c:48)
//   av1_inv_txfm2d_add_32x32      (EbTransforms.c:8293 -> inv_txfm2d_add_c :8180)
//
// Mapping (CDNA4, wave64): one wave owns TWO blocks (lanes 0-31 / 32-63).  In
// the first pass lane c holds column c in 32 VGPRs and runs the straight-line
// generated DCT32; a swizzled LDS tile transposes; in the second pass lane r holds
// row r.  A second swizzled tile re-orders into the linear block layout so that
// quantisation happens on, and every 4 KB output is stored from, fully coalesced
// 16-B-per-lane positions.  Each wave uses a private LDS region: no workgroup
// barrier anywhere.  All LDS access patterns are conflict-free
// (SQ_LDS_BANK_CONFLICT = 0 measured, profiles/r01_a_pmc.json).
//
// HBM traffic per block (headline) = 2 x 1024 B in + 3 x 4096 + 2 + 4 B out =
// 14 342 B — the algorithmic minimum; everything else is VGPR/LDS.
//
// The three kernels are sequences of the per-wave steps of the first section (F = fwd32_kernel, I = inv32_kernel,
// E = enc32_body):
//   block_addr                                               F E    dense / plane origin of a block
//   stage_residual_u8,  read_cols_u8                         F E    8-bit samples  -> packed residual x4 -> columns
//   stage_residual_u16, read_cols_i16                        F E    16-bit samples -> packed residual x4 -> columns
//                                                                   (read_cols_i16 also reads F's own int16-residual staging)
//   transpose1_write, transpose1_rows, transpose2_write,
//   linear_chunk                                             F E    forward transposes and the linear re-order
//   iscan1_row, store_eob_sad                                F E    iscan + 1 rows; eob and SAD reduced and stored
//   quant_chunk                                                E    quantiser of one chunk (F carries the same statements
//                                                                   inline: as a call it costs F's loop a wave per SIMD)
//   Inv32Ranges, inv32_bounds, inv32_lds                     I E    clamp ranges, their VGPR bounds, tile A / B / C addresses
//   tile_a_put, tile_a_rows, idct32_pass, tile_b_write,
//   tile_b_cols, tile_c_write, tile_c_read, recon_chunk      I E    inverse passes and the reconstruction
// The 1-D forward networks are called from the kernels themselves (a network called from a helper on an array taken by
// reference costs registers, see kernel_txfm_staged.h fwd_row_scale); idct32_pass is the measured exception.
#pragma once
#include "dev_common.h"
#include "gen/txfm1d_gen.h"
#include "tx_plan.h"

namespace svtdev {

constexpr int F32_WAVES = 4;                 // waves per workgroup
static_assert(F32_WAVES == svthost::kF32Waves && svthost::f32_blocks_per_wg() == 2 * F32_WAVES, "tx_plan.h plans the grids of the 32x32 pair kernels");
constexpr int F32_TILE_WORDS = 1024;         // one 32x32 int32 tile per block
constexpr int F32_COS_BIT = 12;              // fwd_cos_bit_col/row[3][3] (EbTransforms.h:141-156)

// LDS byte offset of 16-B slot `s` (0..7) of row `r` in a 32x32 int32 tile whose
// slots are XOR-swizzled by f: conflict-free for the access pairs used below.
__device__ __forceinline__ int tile_slot(int r, int s, int f) { return r * 128 + ((s ^ f) << 4); }

// ---- per-wave steps of the 32x32 kernels -------------------------------------------------------------------------------------
// A wave takes two blocks: lanes 0-31 the first, lanes 32-63 the second; li = lane & 31 is the lane's column / row / chunk index
// inside its block and `tile` the block's private 4 KB of LDS.  No step fences: the caller owes a wave_lds_fence() between a
// step that writes the tile and the next one that reads it, and between a step that reads it and the next one that overwrites it.

// Sample offsets and row strides of block blk in the source, prediction and reconstruction arrays.  planes: origin
// (x, y) = (xy[blk] & 0xffff, xy[blk] >> 16) on planes with the given strides (samples); else dense 32x32 blocks back to back.
struct Blk32 { size_t sbase, pbase, rbase; uint32_t sstr, pstr, rstr; };
__device__ __forceinline__ Blk32 block_addr(bool planes, const uint32_t* __restrict__ xy, uint32_t blk, bool valid, uint32_t src_stride,
                                            uint32_t pred_stride, uint32_t recon_stride) {
    Blk32 a;
    a.sbase = a.pbase = a.rbase = (size_t)blk * 1024;
    a.sstr = a.pstr = a.rstr = 32;
    if (planes) {
        const uint32_t o = valid ? xy[blk] : 0u;
        const size_t by = o >> 16, bx = o & 0xffffu;
        a.sstr = src_stride; a.pstr = pred_stride; a.rstr = recon_stride;
        a.sbase = by * a.sstr + bx; a.pbase = by * a.pstr + bx; a.rbase = by * a.rstr + bx;
    }
    return a;
}

// 8-bit staging.  The lane loads 2 x 16 B of the source and of the prediction (sp / pp: the block's origin): rows li/2 and
// 16 + li/2, columns (li&1)*16 .. +15; pk[] returns the prediction chunks (chunk k = pixels (k*32 + li) * 16 .. +15 of the block,
// the unit of the reconstruction).  SAD on the raw bytes (v_sad_u8: 4 pixels per instruction).  The residual goes to the tile as
// packed int16, already x4 (fwd_shift_32x32[0] = 2): chunk k, part p (8 residuals = 16 B) at byte (2k+p)*544 + li*16 - linear
// (conflict-free) stores; the 544-B part stride keeps the column reads conflict-free too.
// Writes the staging image; the caller owes a fence before read_cols_u8.
template <bool WITH_SAD>
__device__ __forceinline__ void stage_residual_u8(char* tile, int li, bool valid, const uint8_t* sp, uint32_t sstr, const uint8_t* pp,
                                                  uint32_t pstr, unsigned& sad_acc, uint4 (&pk)[2]) {
    uint4 s0 = {0, 0, 0, 0}, s1 = s0;
    pk[0] = s0; pk[1] = s0;
    if (valid) {
        sp += (size_t)(li >> 1) * sstr + (li & 1) * 16;
        pp += (size_t)(li >> 1) * pstr + (li & 1) * 16;
        __builtin_memcpy(&s0, sp, 16); __builtin_memcpy(&s1, sp + (size_t)16 * sstr, 16);
        __builtin_memcpy(&pk[0], pp, 16); __builtin_memcpy(&pk[1], pp + (size_t)16 * pstr, 16);
    }
    const uint32_t sw[8] = {s0.x, s0.y, s0.z, s0.w, s1.x, s1.y, s1.z, s1.w};
    const uint32_t pw[8] = {pk[0].x, pk[0].y, pk[0].z, pk[0].w, pk[1].x, pk[1].y, pk[1].z, pk[1].w};
    if (WITH_SAD) {
#pragma unroll
        for (int i = 0; i < 8; i++) sad_acc = __builtin_amdgcn_sad_u8(sw[i], pw[i], sad_acc);
    }
#pragma unroll
    for (int kp = 0; kp < 4; kp++) {   // kp = 2k + p
        uint32_t r[4];
#pragma unroll
        for (int h2 = 0; h2 < 2; h2++) {
            // bytes -> 16-bit lanes with v_perm_b32, then packed subtract and the transform's
            // input up-shift (x4) on the packed words: 4 residuals in 8 instructions
            const uint32_t a = sw[kp * 2 + h2], b = pw[kp * 2 + h2];
            const uint32_t a01 = __builtin_amdgcn_perm(0u, a, 0x0c010c00u), a23 = __builtin_amdgcn_perm(0u, a, 0x0c030c02u);
            const uint32_t b01 = __builtin_amdgcn_perm(0u, b, 0x0c010c00u), b23 = __builtin_amdgcn_perm(0u, b, 0x0c030c02u);
            r[h2 * 2 + 0] = pk_shl2_i16(pk_sub_i16(a01, b01));
            r[h2 * 2 + 1] = pk_shl2_i16(pk_sub_i16(a23, b23));
        }
        *reinterpret_cast<uint4*>(tile + kp * 544 + li * 16) = make_uint4(r[0], r[1], r[2], r[3]);
    }
}
// Column li of the 8-bit staging image: element (r, li) was written by lane (r&15)*2 + (li>>4), part (li>>3)&1, item li&7.
// Reads the staging image; the caller owes a fence before anything overwrites it.
__device__ __forceinline__ void read_cols_u8(const char* tile, int li, int (&x)[32]) {
    const char* colbase = tile + ((li >> 3) & 1) * 544 + (li >> 4) * 16 + (li & 7) * 2;
#pragma unroll
    for (int r = 0; r < 32; r++) x[r] = (int)*reinterpret_cast<const short*>(colbase + (r >> 4) * 1088 + (r & 15) * 32);
}

// 16-bit (10-bit sample) staging.  The lane loads 4 x 16 B of each array: chunk k = row k*8 + li/4, columns (li&3)*8 .. +7 (again the
// unit of the reconstruction; pk[] returns the prediction chunks).  Residual by v_pk_sub_i16 and x4 on the loaded words
// (|s - p| * 4 <= 4092 fits int16), SAD by v_sad_u16.  Chunk k goes to byte k*512 + li*16, so that column c of row r is at
// (r>>3)*512 + (r&7)*64 + c*2: a 64-B contiguous run per row (no conflicts) - the layout of an int16 residual block as it lies
// in memory.  Writes the staging image; the caller owes a fence before read_cols_i16.
template <bool WITH_SAD>
__device__ __forceinline__ void stage_residual_u16(char* tile, int li, bool valid, const uint16_t* sp, uint32_t sstr, const uint16_t* pp,
                                                   uint32_t pstr, unsigned& sad_acc, uint4 (&pk)[4]) {
    uint4 sv[4];
#pragma unroll
    for (int k = 0; k < 4; k++) {
        sv[k] = make_uint4(0, 0, 0, 0); pk[k] = sv[k];
        if (valid) {
            __builtin_memcpy(&sv[k], sp + (size_t)(k * 8 + (li >> 2)) * sstr + (li & 3) * 8, 16);
            __builtin_memcpy(&pk[k], pp + (size_t)(k * 8 + (li >> 2)) * pstr + (li & 3) * 8, 16);
        }
    }
#pragma unroll
    for (int k = 0; k < 4; k++) {
        const uint32_t a[4] = {sv[k].x, sv[k].y, sv[k].z, sv[k].w}, b[4] = {pk[k].x, pk[k].y, pk[k].z, pk[k].w};
        uint32_t d[4];
#pragma unroll
        for (int j = 0; j < 4; j++) {
            d[j] = pk_shl2_i16(pk_sub_i16(a[j], b[j]));
            if (WITH_SAD) sad_acc = __builtin_amdgcn_sad_u16(a[j], b[j], sad_acc);
        }
        *reinterpret_cast<uint4*>(tile + k * 512 + li * 16) = make_uint4(d[0], d[1], d[2], d[3]);
    }
}
// Column li of an int16 staging image in memory order (stage_residual_u16, or a residual block copied as it is).
// Reads the staging image; the caller owes a fence before anything overwrites it.
__device__ __forceinline__ void read_cols_i16(const char* tile, int li, int (&x)[32]) {
#pragma unroll
    for (int r = 0; r < 32; r++) x[r] = (int)*reinterpret_cast<const short*>(tile + (r >> 3) * 512 + (r & 7) * 64 + li * 2);
}

// Transpose 1: the column pass's output of lane li (the caller has applied shift[1] = -4: done before its fence, the row reads
// start earlier than with the shift between the writes - 1.7 % on the plain transform) written as column li (slot swizzle
// f = (row>>1)&7) ...  Writes the tile; the caller owes a fence before (the staging image is read by the column pass) and after.
__device__ __forceinline__ void transpose1_write(char* tile, int li, const int (&x)[32]) {
#pragma unroll
    for (int r = 0; r < 32; r++)
        *reinterpret_cast<int*>(tile + tile_slot(r, li >> 2, (r >> 1) & 7) + (li & 3) * 4) = x[r];
}
// ... and read back as row li.  Reads the tile; the caller owes a fence before transpose2_write.
__device__ __forceinline__ void transpose1_rows(const char* tile, int li, int (&x)[32]) {
#pragma unroll
    for (int s = 0; s < 8; s++) {
        const int4 v = *reinterpret_cast<const int4*>(tile + tile_slot(li, s, (li >> 1) & 7));
        x[s * 4 + 0] = v.x; x[s * 4 + 1] = v.y; x[s * 4 + 2] = v.z; x[s * 4 + 3] = v.w;
    }
}
// Transpose 2: the row pass's output of lane li (shift[2] = 0) as row li of the block in linear order (slot swizzle f = row&7).
// Writes the tile; the caller owes a fence before linear_chunk.
__device__ __forceinline__ void transpose2_write(char* tile, int li, const int (&x)[32]) {
#pragma unroll
    for (int s = 0; s < 8; s++)
        *reinterpret_cast<int4*>(tile + tile_slot(li, s, li & 7)) = make_int4(x[s * 4 + 0], x[s * 4 + 1], x[s * 4 + 2], x[s * 4 + 3]);
}
// Linear 16-B chunk k*32 + li of the block (coefficients (k*32 + li)*4 .. +3), k = 0..7: what the lane quantises and stores.
// Reads the tile; the caller owes a fence before anything overwrites it.
__device__ __forceinline__ int4 linear_chunk(const char* tile, int li, int k) {
    const int row = 4 * k + (li >> 3);
    return *reinterpret_cast<const int4*>(tile + tile_slot(row, li & 7, row & 7));
}

// iscan + 1 of the four positions of the lane's chunk k, as packed 16-bit pairs (iscan <= 1023: no carry between the halves).
// The same for every block: a kernel that loops over blocks loads its eight rows once.
__device__ __forceinline__ uint2 iscan1_row(const int16_t* __restrict__ iscan, int li, int k) {
    uint2 v = *reinterpret_cast<const uint2*>(iscan + (k * 32 + li) * 4);
    v.x += 0x00010001u; v.y += 0x00010001u;
    return v;
}
// Quantises the lane's chunk k (c, from linear_chunk; isc1 from iscan1_row) and stores it at 16-B unit k*32 + li of the block's
// outputs: qcoeff always, coeff and dqcoeff when KEEP.  d returns the dequantised chunk.  Result: the chunk's eob candidate,
// max(iscan + 1) over its non-zero levels.  No LDS access.  (enc32_body; fwd32_kernel's loop carries the same statements, see there.)
template <bool KEEP>
__device__ __forceinline__ int quant_chunk(const int4& c, int k, int li, uint2 isc1, const QParams& qp, bool valid, int4* co4, int4* qc4,
                                           int4* dq4, int4& d) {
    int4 q;
    // only linear position 0 (k == 0, li == 0, .x) uses the DC entries
    quant_one<2>(c.x, (k == 0 && li == 0) ? 0 : 1, qp, q.x, d.x);
    quant_one<2>(c.y, 1, qp, q.y, d.y);
    quant_one<2>(c.z, 1, qp, q.z, d.z);
    quant_one<2>(c.w, 1, qp, q.w, d.w);
    const int e0 = q.x ? (int)(isc1.x & 0xffffu) : 0, e1 = q.y ? (int)(isc1.x >> 16) : 0;
    const int e2 = q.z ? (int)(isc1.y & 0xffffu) : 0, e3 = q.w ? (int)(isc1.y >> 16) : 0;
    if (valid) {
        const int u = k * 32 + li;
        if (KEEP) co4[u] = c;
        qc4[u] = q;
        if (KEEP) dq4[u] = d;
    }
    return max(max(e0, e1), max(e2, e3));
}
// eob = 1 + last scan position with a non-zero level: the half-wave maximum of the lanes' quant_chunk results; SAD: the
// half-wave sum of the staging step's accumulators.  Lane 0 of the half stores both.
template <bool WITH_SAD>
__device__ __forceinline__ void store_eob_sad(int eob_acc, unsigned sad_acc, bool valid, int li, uint32_t blk, uint16_t* __restrict__ eob,
                                              uint32_t* __restrict__ sad) {
    eob_acc = half_wave_max(eob_acc);
    if (WITH_SAD) sad_acc = half_wave_sum(sad_acc);
    if (valid && li == 0) {
        eob[blk] = (uint16_t)eob_acc;
        if (WITH_SAD) sad[blk] = sad_acc;
    }
}

// Clamp ranges of the inverse (av1_gen_inv_stage_range, EbTransforms.c:5404-5456; clamp_buf(input, bd + 8), :8226): row input
// bd+8, row stages 16 / 18 / 20, column input max(bd+6, 16), column stages 16 (18 at bd 12).
template <int BD>
struct Inv32Ranges {
    static constexpr int in_bits = BD + 8, row_bits = BD == 8 ? 16 : (BD == 10 ? 18 : 20);
    static constexpr int cin_bits = BD + 6 > 16 ? BD + 6 : 16, col_bits = BD == 12 ? 18 : 16;
};
// The four ranges' bounds in VGPRs (single v_med3_i32 clamps, see inv32_kernel); equal ranges share registers (bd = 8: all four
// are 16-bit; bd = 10: two pairs).
struct Clamp32 { int lo, hi; };
struct Inv32Bounds { Clamp32 in, row, cin, col; };
template <int BD>
__device__ __forceinline__ Inv32Bounds inv32_bounds() {
    using R = Inv32Ranges<BD>;
    Inv32Bounds b;
    b.in.hi = svtgen::svt_vgpr((1 << (R::in_bits - 1)) - 1);
    b.row.hi = R::row_bits == R::in_bits ? b.in.hi : svtgen::svt_vgpr((1 << (R::row_bits - 1)) - 1);
    b.cin.hi = R::cin_bits == R::in_bits ? b.in.hi : svtgen::svt_vgpr((1 << (R::cin_bits - 1)) - 1);
    b.col.hi = R::col_bits == R::cin_bits ? b.cin.hi : svtgen::svt_vgpr((1 << (R::col_bits - 1)) - 1);
    b.in.lo = ~b.in.hi; b.row.lo = ~b.row.hi; b.cin.lo = ~b.cin.hi; b.col.lo = ~b.col.hi;
    return b;
}

// One 32-point inverse pass of a lane (row or column x[0..31], raw as loaded): input clamp + idct32 / identity.
// Clamp-free fast path: with L1 = sum |x[i]|, every stage clamp of idct32 is a no-op while gain * L1 + slack <= the stage bound
// (txfm_net.clamp_free_bound, constants in gen/txfm1d_gen.h) and, L1 bounding every element, so is the input clamp when
// L1 <= the input bound.  The test is wave-uniform (one ballot); a wave with a louder row / column runs the clamped form.
// 32 v_sad_u32 + xor (~86 issue units) buy 160 v_med3_i32 (~272).  g_tune "no_clamp_free" (FAST = false) keeps the old form.
template <int IN_BITS, int STAGE_BITS, bool FAST>
__device__ __forceinline__ void idct32_pass(int (&x)[32], int is_idtx, Clamp32 in, Clamp32 st) {
    constexpr int in_max = (1 << (IN_BITS - 1)) - 1, st_max = (1 << (STAGE_BITS - 1)) - 1;
    constexpr int lim_net = svtgen::svt_clamp_free_l1(svtgen::svt_idct32_gain_q10, svtgen::svt_idct32_slack, st_max);
    constexpr int lim = lim_net < in_max ? lim_net : in_max;
    if (FAST && !is_idtx) {
        const int l1 = svtgen::svt_l1<32>(x);
        if (__builtin_amdgcn_ballot_w64(l1 > lim) == 0) {
            svtgen::svt_idct32<12, false, false>(x, 0, 0);
            return;
        }
    }
#pragma unroll
    for (int i = 0; i < 32; i++) x[i] = svtgen::svt_clamp(x[i], in.lo, in.hi);
    if (is_idtx) svtgen::svt_iidentity32<12>(x, 0, 0); else svtgen::svt_idct32<12>(x, st.lo, st.hi);
}

// Per-lane LDS byte offsets of the inverse's three tiles; every access is  (one of these) ^ (compile-time constant)  + immediate.
//   tile A (coefficients, linear chunks in, rows out): chunk k of lane li is row 4k + li/8, 16-B slot li%8, stored at slot
//          (li%8) ^ ((row>>1)&7): address (a_w ^ ((2k & 7) << 4)) + k*512; row li, slot s sits at a_r ^ (s << 4)
//   tile B (rows in, columns out): row li written with slot swizzle li&7 at b_w ^ (s << 4); element (r, li) is word li&3 of slot
//          (li>>2) ^ (r&7): address (b_r ^ ((r & 7) << 4)) + r*128
//   tile C (residual words in row order): see tile_c_write; lane li's column is addressed from b_r as in tile B
struct Inv32Lds { int a_w, a_r, b_w, b_r; };
__device__ __forceinline__ Inv32Lds inv32_lds(int li) {
    Inv32Lds a;
    a.a_w = (li >> 3) * 128 + (((li & 7) ^ (li >> 4)) << 4);
    a.a_r = li * 128 + (((li >> 1) & 7) << 4);
    a.b_w = li * 128 + ((li & 7) << 4);
    a.b_r = ((li >> 2) << 4) + (li & 3) * 4;
    return a;
}
// Pixels per 16-B chunk of a lane, the 16-B residual slots that go with them, and the chunks per lane and block.
template <typename PixT>
struct Pix32 {
    static constexpr int PPL = 16 / (int)sizeof(PixT), SPL = PPL / 4, STEPS = 1024 / (32 * PPL);
};

// Linear 16-B coefficient chunk k*32 + li (k = 0..7) into tile A.  Writes the tile; the caller owes a fence before tile_a_rows.
__device__ __forceinline__ void tile_a_put(char* tile, const Inv32Lds& a, int k, int4 v) {
    *reinterpret_cast<int4*>(tile + (a.a_w ^ (((2 * k) & 7) << 4)) + k * 512) = v;
}
// Row li of tile A.  Reads the tile; the caller owes a fence before tile_b_write.
__device__ __forceinline__ void tile_a_rows(const char* tile, const Inv32Lds& a, int (&x)[32]) {
#pragma unroll
    for (int s = 0; s < 8; s++) {
        const int4 v = *reinterpret_cast<const int4*>(tile + (a.a_r ^ (s << 4)));
        x[s * 4 + 0] = v.x; x[s * 4 + 1] = v.y; x[s * 4 + 2] = v.z; x[s * 4 + 3] = v.w;
    }
}
// The row pass's output of lane li, shift[0] = -2 applied, as row li of tile B.  Writes the tile; fence before tile_b_cols.
__device__ __forceinline__ void tile_b_write(char* tile, const Inv32Lds& a, const int (&x)[32]) {
#pragma unroll
    for (int s = 0; s < 8; s++)
        *reinterpret_cast<int4*>(tile + (a.b_w ^ (s << 4))) =
            make_int4((x[s * 4 + 0] + 2) >> 2, (x[s * 4 + 1] + 2) >> 2, (x[s * 4 + 2] + 2) >> 2, (x[s * 4 + 3] + 2) >> 2);
}
// Column li of tile B.  Reads the tile; the caller owes a fence before tile_c_write.
__device__ __forceinline__ void tile_b_cols(const char* tile, const Inv32Lds& a, int (&x)[32]) {
#pragma unroll
    for (int r = 0; r < 32; r++) x[r] = *reinterpret_cast<const int*>(tile + (a.b_r ^ ((r & 7) << 4)) + r * 128);
}
// Tile C: the column pass's output of lane li, shift[1] = -4 applied, as column li of the residual in row order.  Word (r, c)
// lives in 16-B slot sigma = r*8 + c/4; tile_c_read takes SPL consecutive slots per lane, so slots are swizzled by
// sigma ^ ((sigma >> 4) & (SPL-1)) = (c/4) ^ ((r>>1) & (SPL-1)) to keep its b128 reads conflict-free.
// Writes the tile; the caller owes a fence before tile_c_read.
template <int SPL>
__device__ __forceinline__ void tile_c_write(char* tile, const Inv32Lds& a, const int (&x)[32]) {
#pragma unroll
    for (int r = 0; r < 32; r++)
        *reinterpret_cast<int*>(tile + (a.b_r ^ (((r >> 1) & (SPL - 1)) << 4)) + r * 128) = (x[r] + 8) >> 4;
}
// The 4 * SPL residual words of 16-B pixel unit L = k*32 + li (pixels L*PPL .. +PPL-1 of the block).  Reads the tile.
template <int SPL>
__device__ __forceinline__ void tile_c_read(const char* tile, int L, int (&rv)[4 * SPL]) {
    const int g = ((L * SPL) >> 4) & (SPL - 1);      // slot swizzle of tile C
#pragma unroll
    for (int j = 0; j < SPL; j++) {
        const int4 t = *reinterpret_cast<const int4*>(tile + L * (SPL * 16) + ((j ^ g) << 4));
        rv[4 * j] = t.x; rv[4 * j + 1] = t.y; rv[4 * j + 2] = t.z; rv[4 * j + 3] = t.w;
    }
}
// Reconstruction of one 16-B chunk: prediction pv + the PPL int32 residual words of tile_c_read, clipped to BD bits, on packed
// 16-bit pairs: v_perm (pack two residuals), v_pk_add_i16, v_sat_pk_u8_i16 (8-bit) or v_pk_max/min_i16 (16-bit samples).  The
// reference adds in int32: exact for BD <= 10 (column outputs <= 16 bits, 12-14 after the shift).  (add_clip of
// kernel_txfm_staged.h is the same step on the int16 residual tile of the staged kernels; tile C holds int32 words, so the
// packing differs and the two are not forced under one signature.)
template <typename PixT, int BD>
__device__ __forceinline__ uint4 recon_chunk(uint4 pv, const int (&rv)[Pix32<PixT>::PPL]) {
    const uint32_t pw[4] = {pv.x, pv.y, pv.z, pv.w};
    uint32_t ow[4];
#pragma unroll
    for (int q = 0; q < 4; q++) {
        if constexpr (sizeof(PixT) == 1) {
            // pixels (0,2) / (1,3) of the dword as 16-bit lanes; same pairing for the residuals
            const uint32_t pe = pw[q] & 0x00ff00ffu, po = (pw[q] >> 8) & 0x00ff00ffu;
            const uint32_t re = __builtin_amdgcn_perm((uint32_t)rv[4 * q + 2], (uint32_t)rv[4 * q + 0], 0x05040100u);
            const uint32_t ro = __builtin_amdgcn_perm((uint32_t)rv[4 * q + 3], (uint32_t)rv[4 * q + 1], 0x05040100u);
            const uint32_t ue = sat_pk_u8_i16(pk_add_i16(pe, re)), uo = sat_pk_u8_i16(pk_add_i16(po, ro));
            ow[q] = __builtin_amdgcn_perm(uo, ue, 0x05010400u);
        } else {
            const uint32_t rr = __builtin_amdgcn_perm((uint32_t)rv[2 * q + 1], (uint32_t)rv[2 * q + 0], 0x05040100u);
            ow[q] = pk_clamp_i16(pk_add_i16(pw[q], rr), (1 << BD) - 1);
        }
    }
    return make_uint4(ow[0], ow[1], ow[2], ow[3]);
}

// ---- the kernels -----------------------------------------------------------------------------------------------------------

// IN: 0 = int16 residual (dense), 1 = uint8 src / pred, 2 = uint16 src / pred (10-bit).
// PLANES: blocks are addressed on picture planes (block_addr; row strides src_stride / pred_stride in samples); otherwise dense
// 32x32 blocks back to back (the strides fold to 32).  NT: streaming output stores.  QMODE: quant_one's arithmetic.
// (One register budget: a 128-register variant at more waves per SIMD was measured slower and removed, tools/tune_fused.py.)
template <int IN, bool QUANT, bool WITH_SAD, bool NT = false, int QMODE = 2, bool PLANES = false>
__global__ __launch_bounds__(F32_WAVES * 64) void fwd32_kernel(
    const void* __restrict__ src_v, const void* __restrict__ pred_v, int32_t* __restrict__ coeff,
    int32_t* __restrict__ qcoeff, int32_t* __restrict__ dqcoeff, uint16_t* __restrict__ eob,
    uint32_t* __restrict__ sad, const int16_t* __restrict__ iscan, QParams qp, int is_idtx, uint32_t nblocks,
    uint32_t src_stride_rt = 32, uint32_t pred_stride_rt = 32, const uint32_t* __restrict__ xy = nullptr) {
    __shared__ __attribute__((aligned(16))) int32_t lds[F32_WAVES * 2 * F32_TILE_WORDS];

    const int lane = threadIdx.x & 63;
    const int wave = threadIdx.x >> 6;
    const int half = lane >> 5;      // which of the wave's two blocks
    const int li = lane & 31;        // column index (pass 1) / row index (pass 2)
    char* tile = reinterpret_cast<char*>(lds + (wave * 2 + half) * F32_TILE_WORDS);

    uint2 isc1[8];                   // iscan + 1 of the lane's 32 linear positions: the same for every block of the loop
    if (QUANT) {
#pragma unroll
        for (int k = 0; k < 8; k++) isc1[k] = iscan1_row(iscan, li, k);
    }

    const uint32_t npairs = (nblocks + 1) >> 1;
    const uint32_t wave_stride = gridDim.x * F32_WAVES;
    for (uint32_t pair = blockIdx.x * F32_WAVES + wave; pair < npairs; pair += wave_stride) {
        const uint32_t blk = pair * 2 + half;
        const bool valid = blk < nblocks;
        const size_t pix_off = (size_t)blk * 1024;
        unsigned sad_acc = 0;
        int x[32];
        if constexpr (IN == 0) {
            // ---- int16 residual, 2 KB per block, copied as it lies in memory (16-B chunk k*32 + li at k*512 + li*16) ----
            const uint4* r4 = reinterpret_cast<const uint4*>(static_cast<const int16_t*>(src_v) + pix_off);
#pragma unroll
            for (int k = 0; k < 4; k++) {
                uint4 v = make_uint4(0, 0, 0, 0);
                if (valid) v = r4[k * 32 + li];
                *reinterpret_cast<uint4*>(tile + k * 512 + li * 16) = v;
            }
            wave_lds_fence();
            read_cols_i16(tile, li, x);
#pragma unroll
            for (int r = 0; r < 32; r++) x[r] *= 4;                  // shift[0] = 2 (fwd_shift_32x32)
        } else {
            // ---- source and prediction samples -> residual x4 (shift[0] = 2) -> columns ----
            const Blk32 a = block_addr(PLANES, xy, blk, valid, src_stride_rt, pred_stride_rt, 32);
            if constexpr (IN == 1) {
                uint4 pk[2];
                stage_residual_u8<WITH_SAD>(tile, li, valid, static_cast<const uint8_t*>(src_v) + a.sbase, a.sstr,
                                            static_cast<const uint8_t*>(pred_v) + a.pbase, a.pstr, sad_acc, pk);
                wave_lds_fence();
                read_cols_u8(tile, li, x);
            } else {
                uint4 pk[4];
                stage_residual_u16<WITH_SAD>(tile, li, valid, static_cast<const uint16_t*>(src_v) + a.sbase, a.sstr,
                                             static_cast<const uint16_t*>(pred_v) + a.pbase, a.pstr, sad_acc, pk);
                wave_lds_fence();
                read_cols_i16(tile, li, x);
            }
        }
        // ---- column pass: lane li owns column li ------------------------------------
        if (is_idtx) svtgen::svt_fidentity32<F32_COS_BIT>(x); else svtgen::svt_fdct32<F32_COS_BIT>(x);
#pragma unroll
        for (int r = 0; r < 32; r++) x[r] = (x[r] + 8) >> 4;      // shift[1] = -4
        wave_lds_fence();
        transpose1_write(tile, li, x);
        wave_lds_fence();
        transpose1_rows(tile, li, x);
        // ---- row pass: lane li owns row li ---------------------------------------------
        if (is_idtx) svtgen::svt_fidentity32<F32_COS_BIT>(x); else svtgen::svt_fdct32<F32_COS_BIT>(x);
        wave_lds_fence();
        transpose2_write(tile, li, x);
        wave_lds_fence();
        // ---- the lane's 8 linear chunks: store, or quantise and store ---------------------
        int4* co4 = reinterpret_cast<int4*>(coeff + pix_off);
        int4* qc4 = reinterpret_cast<int4*>(qcoeff + pix_off);
        int4* dq4 = reinterpret_cast<int4*>(dqcoeff + pix_off);
        int eob_acc = 0;
#pragma unroll
        for (int k = 0; k < 8; k++) {
            const int4 c = linear_chunk(tile, li, k);
            if constexpr (QUANT) {
                // quant_chunk<QMODE, true, NT> written out: called as a function it costs this loop 9 to 23 VGPRs (headline 160 -> 169,
                // dense IN = 0 / 2 128 -> 148 / 151: a wave per SIMD each), whatever the form of its arguments.  Keep the two equal.
                int4 q, d;
                quant_one<QMODE>(c.x, (k == 0 && li == 0) ? 0 : 1, qp, q.x, d.x);
                quant_one<QMODE>(c.y, 1, qp, q.y, d.y);
                quant_one<QMODE>(c.z, 1, qp, q.z, d.z);
                quant_one<QMODE>(c.w, 1, qp, q.w, d.w);
                const int e0 = q.x ? (int)(isc1[k].x & 0xffffu) : 0, e1 = q.y ? (int)(isc1[k].x >> 16) : 0;
                const int e2 = q.z ? (int)(isc1[k].y & 0xffffu) : 0, e3 = q.w ? (int)(isc1[k].y >> 16) : 0;
                eob_acc = max(eob_acc, max(max(e0, e1), max(e2, e3)));
                if (valid) {
                    const int u = k * 32 + li;
                    if (NT) {   // streaming outputs are never re-read by this kernel
                        typedef int v4i __attribute__((ext_vector_type(4)));
                        __builtin_nontemporal_store(v4i{c.x, c.y, c.z, c.w}, reinterpret_cast<v4i*>(&co4[u]));
                        __builtin_nontemporal_store(v4i{q.x, q.y, q.z, q.w}, reinterpret_cast<v4i*>(&qc4[u]));
                        __builtin_nontemporal_store(v4i{d.x, d.y, d.z, d.w}, reinterpret_cast<v4i*>(&dq4[u]));
                    } else {
                        co4[u] = c; qc4[u] = q; dq4[u] = d;
                    }
                }
            } else {
                if (valid) co4[k * 32 + li] = c;
            }
        }
        if (QUANT) store_eob_sad<WITH_SAD>(eob_acc, sad_acc, valid, li, blk, eob, sad);
        wave_lds_fence();   // tile is re-used by the next pair
    }
}

// ---------------------------------------------------------------------------
// inverse 32x32 + add (inv_txfm2d_add_c, EbTransforms.c:8180-8265): the mirror of
// the forward kernel.  Coefficients are read linearly (coalesced), a swizzled tile
// hands rows to lanes (row pass: clamp bd+8, idct32, round-shift 2), a second tile
// hands columns to lanes (column pass: clamp max(bd+6,16), idct32, round-shift 4),
// and a third tile puts the residual back in row order so that destination samples
// are read, updated and written 16 B per lane.
// dst block b at dst + (offsets ? offsets[b] : b*block_pitch), row stride dst_stride.
//
// This kernel is VALU-bound, not HBM-bound (tools/tune_inv32.py: with the global loads
// removed it runs in 73 % of the full time), so instruction selection follows the
// measured gfx950 issue costs (profiles/r01_valu_issue_cost_*.txt: v_add/v_sub/v_ashrrev/
// v_lshrrev/v_and/v_or/v_xor cost 1, nearly everything else - v_mul_i32_i24, v_mad_i32_i24,
// v_med3, v_lshlrev, v_bfe, SDWA, packed-16 ops - costs 1.7):
//   * every LDS address is  (per-lane base) ^ (compile-time constant)  + immediate offset,
//   * clamps are single v_med3_i32 with VGPR bounds, half_btf is two chained v_mad_i32_i24,
//   * the reconstruction works on packed 16-bit pairs: v_perm (pack two residuals),
//     v_pk_add_i16, v_sat_pk_u8_i16 (8-bit) or v_pk_max/min_i16 (16-bit samples).
// All LDS accesses are conflict-free under the lane-group rules of MI355X_MICROARCH.md
// (ds_read_b128: 4 x 16 lanes over 64 banks; ds_write_b128: 8 x 8 lanes over 32 banks).
// ---------------------------------------------------------------------------
// WAVES / VAR are tuning knobs (tools/tune_inv32.py): VAR bit0 = no destination prefetch,
// bit1 = skip the transforms (memory-only probe), bit2 = skip the global loads (compute-only probe), bit3 = always clamp
// (no clamp-free fast path, see idct32_pass; 5 waves / SIMD as before - the two-path form needs 117 VGPRs, so it runs at 4:
// measured 1.254 ms against 1.361 ms per 2^20 blocks, and 1.70 ms when squeezed into 96 VGPRs with 92 B of scratch).
// (A persistent, software-pipelined variant - next pair's coefficients fetched into registers during
// the transforms, 168 VGPRs, 3 waves/SIMD - measured 14 % SLOWER: the VALU needs the 5 waves/SIMD.)
template <typename PixT, int BD, int WAVES = F32_WAVES, int VAR = 0>
__global__ __launch_bounds__(WAVES * 64) __attribute__((amdgpu_waves_per_eu((VAR & 8) ? 5 : 4))) void inv32_kernel(
    const int32_t* __restrict__ coeff, PixT* __restrict__ dst, int32_t dst_stride, size_t dst_block_pitch,
    const uint32_t* __restrict__ dst_offsets, int is_idtx, uint32_t nblocks) {
    using R = Inv32Ranges<BD>;
    constexpr bool PRE = !(VAR & 1), XFORM = !(VAR & 2), LOADS = !(VAR & 4), FAST = !(VAR & 8);       // the probe bits
    constexpr int PPL = Pix32<PixT>::PPL, SPL = Pix32<PixT>::SPL, STEPS = Pix32<PixT>::STEPS;
    __shared__ __attribute__((aligned(16))) int32_t lds[WAVES * 2 * F32_TILE_WORDS];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int half = lane >> 5, li = lane & 31;
    char* tile = reinterpret_cast<char*>(lds + (wave * 2 + half) * F32_TILE_WORDS);
    const Inv32Bounds cb = inv32_bounds<BD>();
    const Inv32Lds a = inv32_lds(li);

    const uint32_t blk = (blockIdx.x * WAVES + wave) * 2 + half;
    const bool valid = blk < nblocks;
    const size_t dbase = valid ? (dst_offsets ? (size_t)dst_offsets[blk] : (size_t)blk * dst_block_pitch) : 0;
    const bool dst_aligned = (((reinterpret_cast<uintptr_t>(dst) + dbase * sizeof(PixT)) & 15) == 0) && ((dst_stride * (int)sizeof(PixT)) & 15) == 0;
    // destination samples are fetched up front (their latency hides under the two transform passes)
    uint4 dcur[STEPS];
    const bool dcur_ok = PRE && valid && dst_aligned;
    if (dcur_ok) {
#pragma unroll
        for (int k = 0; k < STEPS; k++) {
            const int p = (k * 32 + li) * PPL;
            dcur[k] = LOADS ? *reinterpret_cast<const uint4*>(dst + dbase + (size_t)(p >> 5) * dst_stride + (p & 31)) : make_uint4(k, li, k, li);
        }
    }
    int x[32];
    // ---- coefficients, read linearly (coalesced) -> tile A -> rows ------------------------
    const int4* c4 = reinterpret_cast<const int4*>(coeff + (size_t)blk * 1024);
#pragma unroll
    for (int k = 0; k < 8; k++) tile_a_put(tile, a, k, (valid && LOADS) ? c4[k * 32 + li] : make_int4(li, k, li, k));
    wave_lds_fence();
    tile_a_rows(tile, a, x);
    if constexpr (XFORM) idct32_pass<R::in_bits, R::row_bits, FAST>(x, is_idtx, cb.in, cb.row);
    wave_lds_fence();
    tile_b_write(tile, a, x);
    wave_lds_fence();
    tile_b_cols(tile, a, x);
    if constexpr (XFORM) idct32_pass<R::cin_bits, R::col_bits, FAST>(x, is_idtx, cb.cin, cb.col);
    wave_lds_fence();
    tile_c_write<SPL>(tile, a, x);
    wave_lds_fence();
    // ---- destination samples read, updated and written 16 B per lane --------------------------
    if (valid) {
#pragma unroll
        for (int k = 0; k < STEPS; k++) {
            const int L = k * 32 + li, p = L * PPL;           // 16-B store unit: pixels p .. p + PPL-1 = row p/32, column p%32
            PixT* d = dst + dbase + (size_t)(p >> 5) * dst_stride + (p & 31);
            int rv[PPL];
            tile_c_read<SPL>(tile, L, rv);
            if (dst_aligned) {
                const uint4 pv = dcur_ok ? dcur[k] : (LOADS ? *reinterpret_cast<const uint4*>(d) : make_uint4(k, li, k, li));
                *reinterpret_cast<uint4*>(d) = recon_chunk<PixT, BD>(pv, rv);
            } else {
#pragma unroll
                for (int j = 0; j < PPL; j++) d[j] = (PixT)min(max((int)d[j] + rv[j], 0), (1 << BD) - 1);
            }
        }
    }
}

// ---------------------------------------------------------------------------
// enc32_kernel — the encode-pass chain of one 32x32 8-bit transform block in ONE kernel
// (reference call sequence in Av1EncodeLoop, EbCodingLoop.c:545-950):
//   ResidualKernel -> av1_estimate_transform (32x32 DCT_DCT / IDTX) -> av1_quantize_inv_quantize
//   (aom_highbd_quantize_b_32x32: qcoeff, dqcoeff, eob) -> av1_inv_transform_recon8bit (pred + inverse)
// plus the 32x32 SAD(src, pred).  The forward coefficients, the dequantised coefficients and the
// residual never leave the CU: HBM traffic per block is 2 x 1024 B in + 4096 B (qcoeff) + 1024 B (recon)
// + 6 B out = 7 174 B, against 14 342 + 6 144 B for the two separate kernels.  coeff / dqcoeff are
// written too when the caller passes buffers for them (KEEP).
// The body is fwd32_kernel's steps up to the quantiser, whose dequantised int4 chunks are exactly
// the linear 16-B chunks inv32_kernel loads, then inv32_kernel's steps from tile A on: the prediction samples
// already sit in registers in the 16-B-per-lane layout of its reconstruction stage.
// ---------------------------------------------------------------------------
// PixT / BD: uint8_t / 8 or uint16_t / 10 (BASELINE configs[4]); the 16-bit variant differs only in how the
// residual is staged (stage_residual_u16), in the inverse's clamp ranges and in the final clip.
// (body / kernel split: the body takes its workgroup index and LDS from the caller, so that enc_frame_kernel - one launch for
// every group of a picture, kernel_frame.h - can run it for the workgroups of a 32x32 group)
constexpr int ENC32_LDS_BYTES = F32_WAVES * 2 * F32_TILE_WORDS * 4;
template <typename PixT, int BD, bool KEEP, bool WITH_SAD>
__device__ __forceinline__ void enc32_body(
    const PixT* __restrict__ src, const PixT* __restrict__ pred, PixT* __restrict__ recon,
    int32_t* __restrict__ coeff, int32_t* __restrict__ qcoeff, int32_t* __restrict__ dqcoeff,
    uint16_t* __restrict__ eob, uint32_t* __restrict__ sad, const int16_t* __restrict__ iscan, const QParams& qp,
    int is_idtx, uint32_t nblocks, const uint32_t* __restrict__ xy, uint32_t src_stride,
    uint32_t pred_stride, uint32_t recon_stride, uint32_t bid, int32_t* lds) {
    // xy != NULL: blocks addressed on picture planes (block_addr; recon may be the prediction plane itself); NULL: dense blocks.
    using R = Inv32Ranges<BD>;
    constexpr int PPL = Pix32<PixT>::PPL, SPL = Pix32<PixT>::SPL, STEPS = Pix32<PixT>::STEPS;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int half = lane >> 5, li = lane & 31;
    char* tile = reinterpret_cast<char*>(lds + (wave * 2 + half) * F32_TILE_WORDS);
    const uint32_t blk = (bid * F32_WAVES + wave) * 2 + half;
    const bool valid = blk < nblocks;
    const size_t pix_off = (size_t)blk * 1024;
    const Blk32 ad = block_addr(xy != nullptr, xy, blk, valid, src_stride, pred_stride, recon_stride);

    // ---- forward: residual x4 -> columns, column pass, transpose, row pass, re-order to linear (fwd32_kernel's chain) ----
    uint4 pk[STEPS];                                          // the lane's prediction chunks, kept for the reconstruction
    unsigned sad_acc = 0;
    int x[32];
    if constexpr (sizeof(PixT) == 1) {
        stage_residual_u8<WITH_SAD>(tile, li, valid, src + ad.sbase, ad.sstr, pred + ad.pbase, ad.pstr, sad_acc, pk);
        wave_lds_fence();
        read_cols_u8(tile, li, x);
    } else {
        stage_residual_u16<WITH_SAD>(tile, li, valid, src + ad.sbase, ad.sstr, pred + ad.pbase, ad.pstr, sad_acc, pk);
        wave_lds_fence();
        read_cols_i16(tile, li, x);
    }
    if (is_idtx) svtgen::svt_fidentity32<F32_COS_BIT>(x); else svtgen::svt_fdct32<F32_COS_BIT>(x);
#pragma unroll
    for (int r = 0; r < 32; r++) x[r] = (x[r] + 8) >> 4;      // shift[1] = -4
    wave_lds_fence();
    transpose1_write(tile, li, x);
    wave_lds_fence();
    transpose1_rows(tile, li, x);
    if (is_idtx) svtgen::svt_fidentity32<F32_COS_BIT>(x); else svtgen::svt_fdct32<F32_COS_BIT>(x);
    wave_lds_fence();
    transpose2_write(tile, li, x);
    wave_lds_fence();
    // ---- quantise the lane's 8 linear 16-B chunks; the dequantised chunks stay in registers: they are exactly the linear
    // chunks inv32_kernel loads
    int4 dqv[8];
    {
        int4 cv[8];
#pragma unroll
        for (int k = 0; k < 8; k++) cv[k] = linear_chunk(tile, li, k);
        wave_lds_fence();                                        // the tile is free for the inverse now
        int4* co4 = reinterpret_cast<int4*>(coeff + pix_off);
        int4* qc4 = reinterpret_cast<int4*>(qcoeff + pix_off);
        int4* dq4 = reinterpret_cast<int4*>(dqcoeff + pix_off);
        int eob_acc = 0;
#pragma unroll
        for (int k = 0; k < 8; k++)
            eob_acc = max(eob_acc, quant_chunk<KEEP>(cv[k], k, li, iscan1_row(iscan, li, k), qp, valid, co4, qc4, dq4, dqv[k]));
        store_eob_sad<WITH_SAD>(eob_acc, sad_acc, valid, li, blk, eob, sad);
    }
    // ---- inverse + reconstruction (inv32_kernel's chain from tile A on; the prediction chunks already sit in registers in
    // the 16-B-per-lane layout of its last stage)
    const Inv32Bounds cb = inv32_bounds<BD>();
    const Inv32Lds a = inv32_lds(li);
#pragma unroll
    for (int k = 0; k < 8; k++) tile_a_put(tile, a, k, dqv[k]);
    wave_lds_fence();
    tile_a_rows(tile, a, x);
    idct32_pass<R::in_bits, R::row_bits, true>(x, is_idtx, cb.in, cb.row);
    wave_lds_fence();
    tile_b_write(tile, a, x);
    wave_lds_fence();
    tile_b_cols(tile, a, x);
    idct32_pass<R::cin_bits, R::col_bits, true>(x, is_idtx, cb.cin, cb.col);
    wave_lds_fence();
    tile_c_write<SPL>(tile, a, x);
    wave_lds_fence();
    if (valid) {
#pragma unroll
        for (int k = 0; k < STEPS; k++) {
            const int L = k * 32 + li, p = L * PPL;                // 16-B unit: pixels p .. p + PPL-1 = the lane's prediction chunk k
            int rv[PPL];
            tile_c_read<SPL>(tile, L, rv);
            const uint4 ov = recon_chunk<PixT, BD>(pk[k], rv);
            if (xy) __builtin_memcpy(recon + ad.rbase + (size_t)(p >> 5) * ad.rstr + (p & 31), &ov, 16);
            else reinterpret_cast<uint4*>(recon + pix_off)[L] = ov;
        }
    }
}

template <typename PixT, int BD, bool KEEP, bool WITH_SAD>
__global__ __launch_bounds__(F32_WAVES * 64) __attribute__((amdgpu_waves_per_eu(3))) void enc32_kernel(
    const PixT* __restrict__ src, const PixT* __restrict__ pred, PixT* __restrict__ recon,
    int32_t* __restrict__ coeff, int32_t* __restrict__ qcoeff, int32_t* __restrict__ dqcoeff,
    uint16_t* __restrict__ eob, uint32_t* __restrict__ sad, const int16_t* __restrict__ iscan, QParams qp,
    int is_idtx, uint32_t nblocks, const uint32_t* __restrict__ xy = nullptr, uint32_t src_stride = 32,
    uint32_t pred_stride = 32, uint32_t recon_stride = 32) {
    __shared__ __attribute__((aligned(16))) int32_t lds[F32_WAVES * 2 * F32_TILE_WORDS];
    enc32_body<PixT, BD, KEEP, WITH_SAD>(src, pred, recon, coeff, qcoeff, dqcoeff, eob, sad, iscan, qp, is_idtx, nblocks, xy, src_stride,
                                         pred_stride, recon_stride, blockIdx.x, lds);
}

}  // namespace svtdev

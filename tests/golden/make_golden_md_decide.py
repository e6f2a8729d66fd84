"""Writes tests/golden/md_decide.npz: the join of mode decision on synthetic per-slot tables: the full cost of every (block, slot), the
early exit of AV1PerformFullLoop and the best candidate of product_full_mode_decision.

What is pinned to what.  The cost of every (block, slot) is the REFERENCE's own Av1FullCost (EbRateDistortionCost.c:1456-1534) for an
intra slot and av1_inter_full_cost (:1761-1811) for an inter slot, and every merge slot is also given to Av1MergeSkipFullCost (:1551-1692)
directly, in oracle/_ref/libsvtref.so through ctypes: full_cost, full_lambda_rate, full_cost_luma, full_cost_merge, full_cost_skip and
skip_flag are read back from the candidate buffer.  The DECISION is the reference's own product_full_mode_decision
(EbModeDecision.c:2653-2930) over the effective count: its return value (the buffers are numbered by slot), the best_intra_mode it
writes (preset to 0xFF) and the cost, cost_luma, merge_cost and skip_cost it stores into md_local_cu_unit / md_ep_pipe_sb.  The functions
read and write through pointers; the structs built here are zero-filled byte buffers with the members at their offsetof offsets (taken
once from a program compiled against the reference's headers, bit-fields as a byte and a mask; self_check() proves for every member
used that a written value is the one the function reads).  The ESCAPE WALK (EbProductCodingLoop.c:1935-1941, :2170-2181) is this file's
own glue, written line by line from the reference (glue_count); so is the assembly of the record from the pinned pieces.  np_md_decide is
a second restatement of everything, written independently as array arithmetic; tests compare the fixture with it, and so does main().

The rate tables are SYNTHETIC (no fixture carries skipModeFacBits / intraUVmodeFacBits / cflAlphaFacBits at real magnitude): random
int32 of the magnitude av1_cost_tokens_from_cdf produces (below 2^13).

Chroma inputs.  The decide adds the Cb / Cr distortions, bits and eobs as given; in a real chain they are what svt_hip_full_loop_frame
(ntypes 1) and svt_hip_coeff_rate_frame write for txsize_uv.  That these equal what the reference's chroma path produces is PINNED here to
the compiled CuFullDistortionFastTuMode_R (EbFullLoop.c:1715-1873), run whole through ctypes for each of the fourteen 4:2:0 chroma
transform sizes a supported block size has, both kernel flavours (asm_type 0 / 1), on the transform, quantised and dequantised
coefficients of Cb and Cr blocks that the reference's own transform and quantiser leaves made (random, near, exact and extreme
predictions: eob 0 goes through the cbf-zero kernel and av1_cost_skip_txb).  Its cb / cr distortion pair (with its chromaShift,
(MAX_TX_SCALE - av1_get_tx_scale(txsize_uv)) * 2), its cb / cr coefficient bits and the u_has_coeff / v_has_coeff it leaves in the
candidate are asserted equal to the full loop's restatement (make_golden_full_loop.chain's steps, three_quad_energy 0, shift (1 -
log_scale) * 2) and the rate's (make_golden_coeff_rate.np_cost_coeffs_txb, the eob-0 entry) and recorded as uv_* in the fixture.
Limits of that pin: transform_type[PLANE_TYPE_UV] is DCT_DCT throughout, and the transform and quantiser that fill the buffers are the
leaves the full-loop fixture already pins (FullLoop_R itself is not run whole: it needs a picture's source and prediction buffers).

CPU only; run from the repository root after build():  python tests/golden/make_golden_md_decide.py
"""
import ctypes
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(ROOT, "tests"))

OUT = os.path.join(HERE, "md_decide.npz")
REF = os.path.join(ROOT, "oracle", "_ref", "libsvtref.so")

# ---- offsets (bytes); a bit-field or scalar member is (first byte, mask of its bits from there, little endian) ----
SIZEOF_BUF = 192                                  # ModeDecisionCandidateBuffer_s
OFF_BUF_CANDIDATE_PTR, OFF_BUF_FULL_COST_PTR, OFF_BUF_FULL_COST_SKIP_PTR, OFF_BUF_FULL_COST_MERGE_PTR = 0, 96, 104, 112
OFF_BUF_FULL_LAMBDA_RATE, OFF_BUF_FULL_COST_LUMA = 72, 80
SIZEOF_CAND = 416                                 # ModeDecisionCandidate_s
OFF_CAND_MD_RATE_PTR = 24
OFF_CAND_FAST_LUMA_RATE, OFF_CAND_FAST_CHROMA_RATE = 32, 40          # uint64_t
CAND_TYPE, CAND_MERGE_FLAG, CAND_SKIP_FLAG, CAND_PRED_MODE = (20, 0xff), (17, 0xff), (16, 0xff), (108, 0xff)
CAND_INTRA_LUMA_MODE = (2, 0x7f80)                # an 8-bit bit-field
CAND_INTRA_CHROMA_MODE, CAND_CFL_ALPHA_IDX, CAND_CFL_ALPHA_SIGNS = (124, 0xffffffff), (128, 0xffffffff), (132, 0xffffffff)
CAND_Y_HAS_COEFF, CAND_BLOCK_HAS_COEFF, CAND_FULL_DISTORTION = (104, 0xffffffff), (100, 0xff), (68, 0xffffffff)
SIZEOF_CTX = 15460456                             # ModeDecisionContext_s
OFF_CTX_CU_PTR, OFF_CTX_BLK_GEOM, OFF_CTX_MD_LOCAL_CU_UNIT, OFF_CTX_MD_EP_PIPE_SB = 15137808, 15137816, 64, 15137864
OFF_MDCU_COST, OFF_MDCU_COST_LUMA, MDCU_FULL_DISTORTION = 24, 32, (8, 0xffffffff)      # MdCodingUnit_t [0]
OFF_EP_SKIP_COST, OFF_EP_MERGE_COST = 0, 8        # MdEncPassCuData_t [0]
SIZEOF_GEOM = 92                                  # BlockGeom
GEOM_HAS_UV, GEOM_BWIDTH, GEOM_BHEIGHT, GEOM_TXB_COUNT = (80, 0xffffffff), (10, 0xff), (11, 0xff), (18, 0xffff)
SIZEOF_CU = 600                                   # CodingUnit_s; prediction_unit_array and transform_unit_array lie inside it
CU_SKIP_FLAG_CONTEXT, CU_MDS_IDX, CU_PRED_MODE = (182, 0x3), (542, 0xffff), (493, 0xff)
CU_SKIP_FLAG, CU_PREDICTION_MODE_FLAG, CU_BLOCK_HAS_COEFF = (189, 0x2), (182, 0xc), (182, 0x10)
OFF_CU_AV1XD = 192
SIZEOF_XD = 248                                   # MacroBlockD
SIZEOF_MD = 834144                                # MdRateEstimationContext_s
OFF_MD_SKIP_MODE, OFF_MD_INTRA_UV_MODE, OFF_MD_CFL_ALPHA = 952, 793292, 795108
# CuFullDistortionFastTuMode_R's further members
SIZEOF_PICDESC, OFF_PICDESC_BUFFER_CB, OFF_PICDESC_BUFFER_CR, PICDESC_STRIDE_Y = 96, 8, 16, (48, 0xffff)      # EbPictureBufferDesc_s
OFF_BUF_RESIDUAL_QUANT_COEFF_PTR, OFF_BUF_RECON_COEFF_PTR = 32, 40
OFF_CTX_TRANS_QUANT_BUFFERS_PTR, CTX_FULL_LAMBDA = 15137720, (15137776, 0xffffffff)
SIZEOF_TQB, OFF_TQB_TU_TRANS_COEFF2NX2N_PTR = 40, 0                   # EbTransQuantBuffers
OFF_GEOM_TXSIZE, OFF_GEOM_TXSIZE_UV, OFF_GEOM_TX_WIDTH_UV, OFF_GEOM_TX_HEIGHT_UV = 20, 24, 68, 72      # uint8_t [0]; tx_org_x / _y [0] stay 0
CU_CB_TXB_SKIP_CONTEXT, CU_CB_DC_SIGN_CONTEXT, CU_CR_TXB_SKIP_CONTEXT, CU_CR_DC_SIGN_CONTEXT = (510, 0xffff), (512, 0xffff), (514, 0xffff), (516, 0xffff)
SIZEOF_PCS, OFF_PCS_PARENT_PCS_PTR, SIZEOF_PPCS = 4320, 56, 218784    # PictureControlSet_s, PictureParentControlSet_s (reduced_tx_set_used stays 0)
CAND_U_HAS_COEFF, CAND_V_HAS_COEFF, OFF_CAND_TRANSFORM_TYPE = (101, 0xff), (102, 0xff), 148
MAX_NUM_OF_TU_PER_CU, COMPONENT_CHROMA, PLANE_TYPE_UV = 21, 1, 1
INTER_MODE, INTRA_MODE = 1, 2
UV_DC_PRED, UV_CFL_PRED = 0, 13

RATE_TABLES = (("skipModeFacBits", (3, 3)), ("intraUVmodeFacBits", (2, 13, 15)), ("cflAlphaFacBits", (8, 2, 16)))
RATE_OFFSETS = (OFF_MD_SKIP_MODE, OFF_MD_INTRA_UV_MODE, OFF_MD_CFL_ALPHA)
RATE_WORDS = 655
U64_MAX = 0xFFFFFFFFFFFFFFFF
M64 = U64_MAX
NO_INTRA = 0xFF
BSIZE_W = (4, 4, 8, 8, 8, 16, 16, 16, 32, 32, 32, 64, 64, 64, 128, 128, 4, 16, 8, 32, 16, 64)
BSIZE_H = (4, 8, 4, 8, 16, 8, 16, 32, 16, 32, 64, 32, 64, 128, 64, 128, 16, 4, 32, 8, 64, 16)

TX_DEC_DTYPE = np.dtype([("cost", "<u8"), ("dist", "<u8", (2,)), ("bits", "<u8"), ("eob", "<u2"), ("tx_type", "u1"), ("type_index", "u1"),
                         ("has_coeff", "u1"), ("pad", "u1", (3,))])                       # svt_hip_tx_decision
CFL_DEC_DTYPE = np.dtype([("best_rd", "<i8"), ("dc_rd", "<i8"), ("alpha_q3", "<i4", (2,)), ("uv_mode", "u1"), ("cfl_alpha_idx", "u1"),
                          ("cfl_alpha_signs", "u1"), ("pad", "u1", (5,))])               # svt_hip_cfl_decision
CAND_DTYPE = np.dtype([("pred_mv", "<i2", (2, 2)), ("mode_ctx", "<i2"), ("pred_mode", "u1"), ("ref_frame_type", "u1"), ("drl_index", "u1"),
                       ("ref_mv_count", "u1"), ("drl_ctx", "u1"), ("flags", "u1")])      # svt_hip_inter_cand
BLK_DTYPE = np.dtype([("skip_flag_context", "u1"), ("has_uv", "u1"), ("pad", "u1", (2,))])      # svt_hip_md_blk
DEC_FLAGS = ("slot", "cand", "count", "is_intra", "skip_flag", "merge_flag", "y_has_coeff", "u_has_coeff", "v_has_coeff", "block_has_coeff",
             "tx_type", "best_intra_mode", "uv_mode", "cfl_alpha_idx", "cfl_alpha_signs")
DEC_DTYPE = np.dtype([("cost", "<u8"), ("cost_luma", "<u8"), ("merge_cost", "<u8"), ("skip_cost", "<u8"), ("full_lambda_rate", "<u8"),
                      ("full_distortion", "<u4"), ("eob", "<u2", (3,))] + [(f, "u1") for f in DEC_FLAGS] + [("pad", "u1", (7,))])      # svt_hip_md_decision
assert (TX_DEC_DTYPE.itemsize, CFL_DEC_DTYPE.itemsize, CAND_DTYPE.itemsize, BLK_DTYPE.itemsize, DEC_DTYPE.itemsize) == (40, 32, 16, 4, 72)
SLOT_KEYS = ("cost", "cost_luma", "merge_cost", "skip_cost", "lambda_rate", "skip_flag")


def cfl_allowed(bsize):
    return int(BSIZE_W[bsize] <= 32 and BSIZE_H[bsize] <= 32)


def rate_tables(rates):
    """int32 [655] -> the three tables in their declaration shapes"""
    out, at = {}, 0
    for name, shape in RATE_TABLES:
        k = int(np.prod(shape))
        out[name] = np.asarray(rates[at:at + k], np.int32).reshape(shape)
        at += k
    return out


# ---------------------------------------------------------------------------------------------------------------------------
# a case's inputs as plain arrays (what both restatements and the reference harness read)
# ---------------------------------------------------------------------------------------------------------------------------
def case_inputs(z, k):
    """-> dict of the case's scalars and [nb, n] arrays; chroma is zero where the arrays are absent or the block has no has_uv, the CfL
    record (uv_mode, idx, signs) is zero where it does not apply: exactly what the cost functions are handed"""
    g = lambda key: z[f"c{k}_{key}"]
    c = dict(bsize=int(g("bsize")), n=int(g("n")), ninter=int(g("ninter")), nintra=int(g("nintra")), lam=int(g("lam")),
             slice_is_intra=int(g("slice_is_intra")), escape=int(g("escape")), has_chroma=int(g("has_chroma")), has_cfl=int(g("has_cfl")),
             modes=np.asarray(g("modes"), np.uint8))
    luma = g("luma").view(TX_DEC_DTYPE)[..., 0]
    blk = g("blk").view(BLK_DTYPE)[..., 0]
    nb, n = luma.shape
    c["nb"] = nb
    c["yd"], c["ybits"], c["yeob"], c["yhc"], c["tx_type"] = luma["dist"], luma["bits"], luma["eob"], luma["has_coeff"], luma["tx_type"]
    c["skip_ctx"] = np.minimum(blk["skip_flag_context"], 2)
    c["has_uv"] = blk["has_uv"] != 0
    uv = c["has_uv"][:, None] & bool(c["has_chroma"])
    c["cd"] = np.where(uv[None, :, :, None], g("cdist"), np.uint64(0))                      # [2, nb, n, 2]
    c["cbits"] = np.where(uv[None], g("cbits"), np.uint64(0))
    c["ceob"] = np.where(uv[None], g("ceob"), np.uint16(0))
    c["rate"] = g("rate")
    c["cand"] = g("cand")
    c["intra"] = c["cand"] >= c["ninter"]
    listed = np.concatenate([c["modes"], np.zeros(1, np.uint8)])                             # (an inter slot reads the appended 0)
    c["mode"] = listed[np.where(c["intra"], c["cand"].astype(np.int64) - c["ninter"], c["nintra"])]
    flags = g("cand_out").view(CAND_DTYPE)[..., 0]["flags"]
    c["merge"] = ~c["intra"] & ((flags & 1) != 0)
    cfl = g("cfl").view(CFL_DEC_DTYPE)[..., 0]
    on = c["intra"] & c["has_uv"][:, None] & bool(c["has_cfl"])
    c["uv_mode"] = np.where(on, cfl["uv_mode"], 0).astype(np.uint8)
    c["cfl_idx"] = np.where(on, cfl["cfl_alpha_idx"], 0).astype(np.uint8)
    c["cfl_signs"] = np.where(on, cfl["cfl_alpha_signs"], 0).astype(np.uint8)
    return c


# ---------------------------------------------------------------------------------------------------------------------------
# restatement 1: the glue, scalar, line by line from the reference
# ---------------------------------------------------------------------------------------------------------------------------
def rdcost(lam, r, d):
    return ((((r * lam) & M64) + 256 & M64) >> 9) + ((d << 7) & M64) & M64


def s64(v):
    """an int32 table entry converted to uint64_t"""
    return int(v) & M64


def glue_slot(c, T, b, k):
    """Av1FullCost / Av1MergeSkipFullCost as av1_inter_full_cost chooses, for slot k of block b -> dict of SLOT_KEYS"""
    lam = c["lam"]
    yd0, yd1, yb = int(c["yd"][b, k, 0]), int(c["yd"][b, k, 1]), int(c["ybits"][b, k])
    cb0, cb1, cr0, cr1 = int(c["cd"][0, b, k, 0]), int(c["cd"][0, b, k, 1]), int(c["cd"][1, b, k, 0]), int(c["cd"][1, b, k, 1])
    cbb, crb = int(c["cbits"][0, b, k]), int(c["cbits"][1, b, k])
    out = dict(cost_luma=0, merge_cost=0, skip_cost=0, skip_flag=0)
    if c["merge"][b, k]:
        skipModeRate = s64(T["skipModeFacBits"][int(c["skip_ctx"][b]), 1])
        coeffRate = (yb + cbb + crb) & M64
        mergeLumaSse, mergeChromaSse = yd0, (cb0 + cr0) & M64
        skipLumaSse, skipChromaSse = yd1, (cb1 + cr1) & M64
        mergeRate = (int(c["rate"][b, k, 0]) + int(c["rate"][b, k, 1]) + coeffRate) & M64
        mergeDistortion = (mergeLumaSse + mergeChromaSse) & M64
        merge_cost = rdcost(lam, mergeRate, mergeDistortion)
        skipDistortion = (skipLumaSse + skipChromaSse) & M64
        skip_cost = rdcost(lam, skipModeRate, skipDistortion)
        out["cost"] = skip_cost if skip_cost <= merge_cost else merge_cost
        tempDistortion = skipDistortion if skip_cost <= merge_cost else mergeDistortion
        out["lambda_rate"] = (out["cost"] - tempDistortion) & M64
        out["merge_cost"], out["skip_cost"] = merge_cost, skip_cost
        out["skip_flag"] = int(skip_cost <= merge_cost)
        return out
    lumaRate, chromaRate = int(c["rate"][b, k, 0]), int(c["rate"][b, k, 1])
    if c["has_uv"][b]:
        if c["intra"][b, k] and c["uv_mode"][b, k] == UV_CFL_PRED:
            isCflAllowed = cfl_allowed(c["bsize"])
            signs, idx, mode = int(c["cfl_signs"][b, k]), int(c["cfl_idx"][b, k]), int(c["mode"][b, k])
            a = int(np.int32(T["cflAlphaFacBits"][signs, 0, idx >> 4]) + np.int32(T["cflAlphaFacBits"][signs, 1, idx & 15]))      # int + int
            chromaRate = (chromaRate + s64(a)) & M64
            chromaRate = (chromaRate + s64(T["intraUVmodeFacBits"][isCflAllowed, mode, UV_CFL_PRED])) & M64
            chromaRate = (chromaRate - s64(T["intraUVmodeFacBits"][isCflAllowed, mode, UV_DC_PRED])) & M64
    coeffRate = (yb + cbb + crb) & M64
    luma_sse, chromaSse = yd0, (cb0 + cr0) & M64
    totalDistortion = (luma_sse + chromaSse) & M64
    rate = (lumaRate + chromaRate + coeffRate) & M64
    out["cost"] = rdcost(lam, rate, totalDistortion)
    out["lambda_rate"] = (out["cost"] - totalDistortion) & M64
    out["cost_luma"] = rdcost(lam, (lumaRate + yb) & M64, luma_sse)
    return out


def glue_count(c, cost, b):
    """the early return of AV1PerformFullLoop: the effective full_recon_search_count of block b"""
    best_inter_luma_zero_coeff, bestfullCost = 1, 0xFFFFFFFF
    for k in range(c["n"]):
        if not c["slice_is_intra"]:
            if (c["intra"][b, k] or c["escape"] == 2) and best_inter_luma_zero_coeff == 0:
                return k
        if c["escape"]:
            if not c["slice_is_intra"]:
                if not c["intra"][b, k]:
                    if int(cost[b, k]) < bestfullCost:
                        best_inter_luma_zero_coeff = int(c["yhc"][b, k])
                        bestfullCost = int(cost[b, k])
    return c["n"]


def glue_decision(c, cost, b, count):
    """product_full_mode_decision's loop (EbModeDecision.c:2674-2690), mirrored -> (slot, best_intra_mode)"""
    lowestCost, lowestIntraCost, lowestCostIndex, best_intra_mode = U64_MAX, U64_MAX, 0, NO_INTRA
    for i in range(count):
        if int(cost[b, i]) < lowestIntraCost and c["intra"][b, i]:
            best_intra_mode = int(c["mode"][b, i])
            lowestIntraCost = int(cost[b, i])
        if int(cost[b, i]) < lowestCost:
            lowestCostIndex = i
            lowestCost = int(cost[b, i])
    return lowestCostIndex, best_intra_mode


def assemble(c, S, count, slot, best_intra_mode):
    """the records from per-slot values S (dict of [nb, n] arrays), counts, winners and best intra modes"""
    nb = c["nb"]
    rows, w = np.arange(nb), np.asarray(slot, np.int64)
    d = np.zeros(nb, DEC_DTYPE)
    for key, src in (("cost", "cost"), ("cost_luma", "cost_luma"), ("merge_cost", "merge_cost"), ("skip_cost", "skip_cost"), ("full_lambda_rate", "lambda_rate")):
        d[key] = S[src][rows, w]
    d["full_distortion"] = (c["yd"][rows, w, 0] & np.uint64(0xFFFFFFFF)).astype(np.uint32)
    d["eob"][:, 0] = c["yeob"][rows, w]; d["eob"][:, 1] = c["ceob"][0, rows, w]; d["eob"][:, 2] = c["ceob"][1, rows, w]
    d["slot"], d["cand"], d["count"] = w, c["cand"][rows, w], count
    d["is_intra"], d["skip_flag"], d["merge_flag"] = c["intra"][rows, w], S["skip_flag"][rows, w], c["merge"][rows, w]
    d["y_has_coeff"] = c["yhc"][rows, w] != 0
    d["u_has_coeff"], d["v_has_coeff"] = d["eob"][:, 1] != 0, d["eob"][:, 2] != 0
    d["block_has_coeff"] = d["y_has_coeff"] | d["u_has_coeff"] | d["v_has_coeff"]
    d["tx_type"], d["best_intra_mode"] = c["tx_type"][rows, w], best_intra_mode
    d["uv_mode"], d["cfl_alpha_idx"], d["cfl_alpha_signs"] = c["uv_mode"][rows, w], c["cfl_idx"][rows, w], c["cfl_signs"][rows, w]
    return d


def glue_md_decide(z, k, S=None):
    """restatement 1 of a case -> (DEC_DTYPE [nb], dict of per-slot arrays).  With S (the reference's per-slot values) only the walk and
    the decision are the glue's"""
    c, T = case_inputs(z, k), rate_tables(z["rates"])
    nb, n = c["nb"], c["n"]
    if S is None:
        S = {key: np.zeros((nb, n), np.uint64 if key != "skip_flag" else np.uint8) for key in SLOT_KEYS}
        for b in range(nb):
            for s in range(n):
                for key, v in glue_slot(c, T, b, s).items():
                    S[key][b, s] = v
    count = [glue_count(c, S["cost"], b) for b in range(nb)]
    picks = [glue_decision(c, S["cost"], b, count[b]) for b in range(nb)]
    return assemble(c, S, count, [p[0] for p in picks], [p[1] for p in picks]), S


# ---------------------------------------------------------------------------------------------------------------------------
# restatement 2: array arithmetic, written independently (what the tests use where the reference is not built)
# ---------------------------------------------------------------------------------------------------------------------------
def np_rd(lam, r, d):
    with np.errstate(over="ignore"):
        return ((r * np.uint64(lam) + np.uint64(256)) >> np.uint64(9)) + d * np.uint64(128)


def np_md_decide(z, k):
    """svt_hip_md_decide_frame for case k -> (DEC_DTYPE [nb], full cost uint64 [nb, n])"""
    c, T = case_inputs(z, k), rate_tables(z["rates"])
    nb, n = c["nb"], c["n"]
    u = lambda a: np.asarray(a).astype(np.int64).astype(np.uint64)                      # sign-extend, then wrap
    with np.errstate(over="ignore"):
        d_res = c["yd"][..., 0] + c["cd"][0, ..., 0] + c["cd"][1, ..., 0]
        d_pred = c["yd"][..., 1] + c["cd"][0, ..., 1] + c["cd"][1, ..., 1]
        bits = c["ybits"] + c["cbits"][0] + c["cbits"][1]
        r_luma, r_chroma = c["rate"][..., 0].astype(np.uint64), c["rate"][..., 1].astype(np.uint64)
        is_cfl = c["uv_mode"] == UV_CFL_PRED                                            # (zero unless intra, has_uv, d_cfl)
        signs, idx, mode = np.minimum(c["cfl_signs"], 7).astype(np.int64), c["cfl_idx"].astype(np.int64), c["mode"].astype(np.int64)
        alpha = (T["cflAlphaFacBits"][signs, 0, idx >> 4].astype(np.int64) + T["cflAlphaFacBits"][signs, 1, idx & 15]).astype(np.int32)
        uvt = T["intraUVmodeFacBits"][cfl_allowed(c["bsize"])]
        extra = u(alpha) + u(uvt[mode, UV_CFL_PRED]) - u(uvt[mode, UV_DC_PRED])
        r_chroma = r_chroma + np.where(is_cfl, extra, np.uint64(0))
        full = np_rd(c["lam"], r_luma + r_chroma + bits, d_res)
        merge_cost = np_rd(c["lam"], c["rate"][..., 0].astype(np.uint64) + c["rate"][..., 1].astype(np.uint64) + bits, d_res)
        skip_cost = np_rd(c["lam"], np.broadcast_to(u(T["skipModeFacBits"][c["skip_ctx"].astype(np.int64), 1])[:, None], (nb, n)), d_pred)
        skip = c["merge"] & (skip_cost <= merge_cost)
        cost = np.where(c["merge"], np.where(skip, skip_cost, merge_cost), full)
        S = dict(cost=cost, cost_luma=np.where(c["merge"], np.uint64(0), np_rd(c["lam"], r_luma + c["ybits"], c["yd"][..., 0])),
                 merge_cost=np.where(c["merge"], merge_cost, np.uint64(0)), skip_cost=np.where(c["merge"], skip_cost, np.uint64(0)),
                 lambda_rate=cost - np.where(skip, d_pred, d_res), skip_flag=skip.astype(np.uint8))
    # the escape: the running best inter cost below 2^32 - 1 and the has_coeff of the slot that set it, BEFORE each slot
    count = np.full(nb, n, np.int64)
    if not c["slice_is_intra"]:
        inter = ~c["intra"]
        track = np.where(inter & bool(c["escape"]), np.minimum(cost, np.uint64(0xFFFFFFFF)), np.uint64(0xFFFFFFFF))
        run = np.minimum.accumulate(track, axis=1)
        prev = np.concatenate([np.full((nb, 1), 0xFFFFFFFF, np.uint64), run[:, :-1]], axis=1)      # bestfullCost before slot k
        setter = inter & bool(c["escape"]) & (cost < prev)                              # slot k lowers it
        last = np.where(setter, np.arange(n)[None, :], -1)
        last_before = np.concatenate([np.full((nb, 1), -1), np.maximum.accumulate(last, axis=1)[:, :-1]], axis=1)
        zero = np.where(last_before >= 0, np.take_along_axis(c["yhc"], np.maximum(last_before, 0), axis=1) == 0, False)
        stop = (c["intra"] | (c["escape"] == 2)) & zero
        count = np.where(stop.any(axis=1), stop.argmax(axis=1), n)
    live = np.arange(n)[None, :] < count[:, None]
    slot = np.where(live, cost, np.uint64(U64_MAX)).argmin(axis=1)                      # the first of the smallest
    slot = np.where(np.where(live, cost, np.uint64(U64_MAX)).min(axis=1) == np.uint64(U64_MAX), 0, slot)
    icost = np.where(live & c["intra"], cost, np.uint64(U64_MAX))
    islot = icost.argmin(axis=1)
    bim = np.where(icost.min(axis=1) == np.uint64(U64_MAX), NO_INTRA, c["mode"][np.arange(nb), islot])
    return assemble(c, S, count, slot, bim), cost


def np_gather(dec, arr, plane=None):
    """the winner's row of arr [nb, n, ...] -> [nb, ...]; with plane (0 .. 2) rows whose winner has eob 0 in that plane are zeros"""
    out = arr[np.arange(len(dec)), dec["slot"].astype(np.int64)].copy()
    if plane is not None:
        out[dec["eob"][:, plane] == 0] = 0
    return out


# ---------------------------------------------------------------------------------------------------------------------------
# the reference
# ---------------------------------------------------------------------------------------------------------------------------
_lib = None


def ref_lib():
    global _lib
    if _lib is None and os.path.exists(REF):
        L = ctypes.CDLL(REF)
        P, U64 = ctypes.c_void_p, ctypes.c_uint64
        for name in ("Av1FullCost", "Av1MergeSkipFullCost", "av1_inter_full_cost"):
            f = getattr(L, name)
            f.restype = ctypes.c_int
            f.argtypes = [P, P, P, P, P, P, P, U64, P, P, P, ctypes.c_int]
        L.product_full_mode_decision.restype = ctypes.c_uint8
        L.product_full_mode_decision.argtypes = [P, P, ctypes.c_uint8, ctypes.c_uint8, P, ctypes.c_uint32, P, P]
        _lib = L
    return _lib


def put(buf, member, value):
    """writes a scalar or bit-field member (first byte, mask) of a byte buffer"""
    at, mask = member
    nbytes = (mask.bit_length() + 7) // 8
    shift = (mask & -mask).bit_length() - 1
    old = int.from_bytes(buf[at:at + nbytes].tobytes(), "little")
    assert (int(value) << shift) & ~mask == 0, (member, value)
    buf[at:at + nbytes] = np.frombuffer(((old & ~mask) | (int(value) << shift)).to_bytes(nbytes, "little"), np.uint8)


def get(buf, member):
    at, mask = member
    nbytes = (mask.bit_length() + 7) // 8
    return (int.from_bytes(buf[at:at + nbytes].tobytes(), "little") & mask) >> ((mask & -mask).bit_length() - 1)


def put64(buf, at, value):
    buf[at:at + 8].view(np.uint64)[0] = np.uint64(int(value) & M64)


def get64(buf, at):
    return int(buf[at:at + 8].view(np.uint64)[0])


class RefMd:
    """the structs the cost functions and product_full_mode_decision read and write through, as zero-filled byte buffers: the context
    with its block geometry and coding unit, the rate tables, and nslots candidate buffers, buffer i holding slot i"""

    def __init__(self, rates, nslots=40):
        self.md = np.zeros(SIZEOF_MD, np.uint8)
        for (name, shape), off, tab in zip(RATE_TABLES, RATE_OFFSETS, rate_tables(rates).values()):
            self.md[off:off + 4 * tab.size].view(np.int32)[:] = tab.reshape(-1)
        self.ctx, self.geom = np.zeros(SIZEOF_CTX, np.uint8), np.zeros(SIZEOF_GEOM, np.uint8)
        self.cu, self.xd = np.zeros(SIZEOF_CU, np.uint8), np.zeros(SIZEOF_XD, np.uint8)
        put64(self.ctx, OFF_CTX_BLK_GEOM, self.geom.ctypes.data)
        put64(self.ctx, OFF_CTX_CU_PTR, self.cu.ctypes.data)
        put64(self.cu, OFF_CU_AV1XD, self.xd.ctypes.data)
        put(self.geom, GEOM_TXB_COUNT, 1)
        self.cand = [np.zeros(SIZEOF_CAND, np.uint8) for _ in range(nslots)]
        self.buf = [np.zeros(SIZEOF_BUF, np.uint8) for _ in range(nslots)]
        self.costs = np.zeros((nslots, 3), np.uint64)                               # full_cost, full_cost_skip, full_cost_merge
        self.ptrs = np.array([b.ctypes.data for b in self.buf], np.uint64)          # buffer_ptr_array
        self.order = np.arange(nslots, dtype=np.uint8)                              # best_candidate_index_array: slot i is buffer i
        for i in range(nslots):
            put64(self.cand[i], OFF_CAND_MD_RATE_PTR, self.md.ctypes.data)
            put64(self.buf[i], OFF_BUF_CANDIDATE_PTR, self.cand[i].ctypes.data)
            for j, off in enumerate((OFF_BUF_FULL_COST_PTR, OFF_BUF_FULL_COST_SKIP_PTR, OFF_BUF_FULL_COST_MERGE_PTR)):
                put64(self.buf[i], off, self.costs[i, j:].ctypes.data)

    def block(self, bsize, has_uv, skip_ctx):
        put(self.geom, GEOM_HAS_UV, int(has_uv)); put(self.geom, GEOM_BWIDTH, BSIZE_W[bsize]); put(self.geom, GEOM_BHEIGHT, BSIZE_H[bsize])
        put(self.cu, CU_SKIP_FLAG_CONTEXT, int(skip_ctx))

    def slot(self, L, i, fn, intra, merge, mode, uv_mode, idx, signs, rate, yd, cbd, crd, bits, lam, bsize, yhc=0):
        """one cost call on buffer i, as AV1PerformFullLoop prepares the candidate (skip_flag EB_FALSE, :1954) -> dict of SLOT_KEYS"""
        cand, buf = self.cand[i], self.buf[i]
        put(cand, CAND_TYPE, INTRA_MODE if intra else INTER_MODE); put(cand, CAND_MERGE_FLAG, int(merge)); put(cand, CAND_SKIP_FLAG, 0)
        put(cand, CAND_INTRA_LUMA_MODE, int(mode)); put(cand, CAND_PRED_MODE, int(mode)); put(cand, CAND_INTRA_CHROMA_MODE, int(uv_mode))
        put(cand, CAND_CFL_ALPHA_IDX, int(idx)); put(cand, CAND_CFL_ALPHA_SIGNS, int(signs)); put(cand, CAND_Y_HAS_COEFF, int(yhc))
        put64(cand, OFF_CAND_FAST_LUMA_RATE, rate[0]); put64(cand, OFF_CAND_FAST_CHROMA_RATE, rate[1])
        self.costs[i] = 0
        put64(buf, OFF_BUF_FULL_LAMBDA_RATE, 0); put64(buf, OFF_BUF_FULL_COST_LUMA, 0)
        a = [np.array(v, np.uint64).reshape(-1) for v in (yd, cbd, crd, [bits[0]], [bits[1]], [bits[2]])]
        getattr(L, fn)(None, self.ctx.ctypes.data, buf.ctypes.data, self.cu.ctypes.data, a[0].ctypes.data, a[1].ctypes.data, a[2].ctypes.data,
                       int(lam), a[3].ctypes.data, a[4].ctypes.data, a[5].ctypes.data, int(bsize))
        return dict(cost=int(self.costs[i, 0]), skip_cost=int(self.costs[i, 1]), merge_cost=int(self.costs[i, 2]),
                    lambda_rate=get64(buf, OFF_BUF_FULL_LAMBDA_RATE), cost_luma=get64(buf, OFF_BUF_FULL_COST_LUMA), skip_flag=get(cand, CAND_SKIP_FLAG))

    def decide(self, L, count):
        """product_full_mode_decision over the first `count` buffers as the cost calls left them -> dict"""
        best = np.array([NO_INTRA], np.uint32)
        for off in (OFF_MDCU_COST, OFF_MDCU_COST_LUMA):
            put64(self.ctx, OFF_CTX_MD_LOCAL_CU_UNIT + off, 0)
        put(self.cu, CU_MDS_IDX, 0)
        slot = int(L.product_full_mode_decision(self.ctx.ctypes.data, self.cu.ctypes.data, 0, 0, self.ptrs.ctypes.data, int(count),
                                                self.order.ctypes.data, best.ctypes.data))
        ep = self.ctx[OFF_CTX_MD_EP_PIPE_SB:]
        return dict(slot=slot, best_intra_mode=int(best[0]), cost=get64(self.ctx, OFF_CTX_MD_LOCAL_CU_UNIT + OFF_MDCU_COST),
                    cost_luma=get64(self.ctx, OFF_CTX_MD_LOCAL_CU_UNIT + OFF_MDCU_COST_LUMA), merge_cost=get64(ep, OFF_EP_MERGE_COST),
                    skip_cost=get64(ep, OFF_EP_SKIP_COST), is_intra=int(get(self.cu, CU_PREDICTION_MODE_FLAG) == INTRA_MODE),
                    skip_flag=get(self.cu, CU_SKIP_FLAG), pred_mode=get(self.cu, CU_PRED_MODE))


def self_check(L):
    """every member written above is the one the functions read: tables whose entries name themselves, one member set at a time"""
    rates = np.arange(RATE_WORDS, dtype=np.int32) * 512 + 512                            # RDCOST(1, 512 v, 0) = v: entry e costs e + 1
    T = rate_tables(rates)
    r = RefMd(rates, 2)
    z2, z3 = [0, 0], [0, 0, 0]
    base = dict(intra=1, merge=0, mode=0, uv_mode=0, idx=0, signs=0, rate=[0, 0], yd=z2, cbd=z2, crd=z2, bits=z3, lam=1, bsize=3)
    call = lambda fn, **kw: r.slot(L, 0, fn, **dict(base, **kw))
    r.block(3, 1, 0)
    assert call("Av1FullCost", rate=[512 * 7, 0]) == dict(cost=7, cost_luma=7, lambda_rate=7, merge_cost=0, skip_cost=0, skip_flag=0)
    o = call("Av1FullCost", rate=[0, 512 * 9])
    assert (o["cost"], o["cost_luma"]) == (9, 0)
    o = call("Av1FullCost", yd=[3, 1000], cbd=[5, 2000], crd=[11, 4000], bits=[512, 1024, 2048])
    assert (o["cost"], o["cost_luma"], o["lambda_rate"]) == (7 + 19 * 128, 1 + 3 * 128, 7 + 19 * 128 - 19)
    for bsize, mode, idx, signs in ((3, 5, 0x3A, 6), (12, 12, 0xF1, 1)):                 # isCflAllowed 1 and 0
        r.block(bsize, 1, 0)
        want = int(T["cflAlphaFacBits"][signs, 0, idx >> 4] + T["cflAlphaFacBits"][signs, 1, idx & 15] + T["intraUVmodeFacBits"][cfl_allowed(bsize), mode, 13]
                   - T["intraUVmodeFacBits"][cfl_allowed(bsize), mode, 0]) // 512
        assert call("Av1FullCost", bsize=bsize, mode=mode, uv_mode=13, idx=idx, signs=signs)["cost"] == want
        assert call("Av1FullCost", bsize=bsize, mode=mode, uv_mode=12, idx=idx, signs=signs)["cost"] == 0       # not UV_CFL_PRED
        assert call("av1_inter_full_cost", intra=0, bsize=bsize, mode=mode, uv_mode=13, idx=idx, signs=signs)["cost"] == 0      # not INTRA_MODE
        r.block(bsize, 0, 0)
        assert call("Av1FullCost", bsize=bsize, mode=mode, uv_mode=13, idx=idx, signs=signs)["cost"] == 0       # no has_uv
    for ctx in range(3):
        r.block(3, 1, ctx)
        want = int(T["skipModeFacBits"][ctx, 1]) // 512
        for fn in ("av1_inter_full_cost", "Av1MergeSkipFullCost"):
            o = call(fn, intra=0, merge=1, yd=[1 << 20, 2], cbd=[0, 3], crd=[0, 4])
            assert o == dict(cost=want + 9 * 128, skip_cost=want + 9 * 128, merge_cost=1 << 27, lambda_rate=want + 9 * 128 - 9, cost_luma=0, skip_flag=1), o
        o = call("av1_inter_full_cost", intra=0, merge=0, yd=[1 << 20, 2])
        assert (o["cost"], o["skip_flag"], o["merge_cost"]) == (1 << 27, 0, 0)
    # the decision: buffer i is slot i; the cost, type and pred_mode members are the ones read
    r.block(3, 1, 0)
    call("Av1FullCost", rate=[512 * 50, 0], mode=9)
    r.slot(L, 1, "av1_inter_full_cost", **dict(base, intra=0, rate=[512 * 40, 0]))
    d = r.decide(L, 2)
    assert (d["slot"], d["best_intra_mode"], d["cost"], d["is_intra"]) == (1, 9, 40, 0), d
    d = r.decide(L, 1)
    assert (d["slot"], d["best_intra_mode"], d["cost"], d["cost_luma"], d["is_intra"], d["pred_mode"]) == (0, 9, 50, 50, 1, 9), d


def uv_sizes():
    """the 4:2:0 chroma transform sizes of the supported block sizes (a chroma side at least 4), ascending"""
    from svtlibs import TX_H, TX_W
    out = set()
    for bsize in range(22):
        if 13 <= bsize <= 15:
            continue
        w, h = max(BSIZE_W[bsize] // 2, 4), max(BSIZE_H[bsize] // 2, 4)
        out.add(next(s for s in range(19) if (TX_W[s], TX_H[s]) == (w, h)))
    return sorted(out)


UV_NBLK, UV_QINDEX, UV_LAMBDA = 4, 60, 29041                             # blocks per size: random, near, exact (eob 0), extreme


def uv_inputs(s):
    """-> src, pred uint8 [2 planes, UV_NBLK, H, W], skip / dc-sign contexts [2, UV_NBLK], the PLANE_TYPE_UV cost tables of the size"""
    import make_golden_coeff_rate as mgc
    from svtlibs import TX_H, TX_W
    rng = np.random.default_rng(9300 + s)
    shp = (2, TX_H[s], TX_W[s])
    src = rng.integers(0, 256, (UV_NBLK,) + shp)
    pred = np.stack([rng.integers(0, 256, shp), np.clip(src[1] + rng.integers(-6, 7, shp), 0, 255), src[2], np.zeros(shp, np.int64)])
    src[3] = 255
    cc, ec = mgc.tables_of(s)
    return (src.transpose(1, 0, 2, 3).astype(np.uint8), pred.transpose(1, 0, 2, 3).astype(np.uint8), rng.integers(0, 13, (2, UV_NBLK)),
            rng.integers(0, 3, (2, UV_NBLK)), cc, ec)


def uv_restatement(s, tx_type=0):
    """the chroma stage as this library's calls are restated: the full loop's steps (make_golden_full_loop.chain: residual, the reference's
    transform and quantiser leaves, picture_full_distortion32_bits in both flavours, the shift) and the rate's restatement
    -> dict: coeff, qcoeff, dqcoeff int32 [2, UV_NBLK, NC]; eob [2, UV_NBLK]; dist uint64 [2 flavours, 2 planes, UV_NBLK, 2]; bits [2, UV_NBLK]"""
    import make_golden_coeff_rate as mgc
    import make_golden_full_loop as mfl
    from svtlibs import TX_H, TX_W, ptr
    R, c_int = mfl.R, ctypes.c_int
    w, h = TX_W[s], TX_H[s]
    n, ls = w * h, (1 if w * h > 256 else 0)
    src, pred, skip, dcs, cc, ec = uv_inputs(s)
    tabs = mfl.y_tables()
    qrow = {k: np.ascontiguousarray(v[UV_QINDEX]) for k, v in tabs.items()}
    scan = np.ctypeslib.as_array(R.ref_get_scan(s, tx_type, 0), shape=(n,)).copy()
    iscan = np.ctypeslib.as_array(R.ref_get_scan(s, tx_type, 1), shape=(n,)).copy()
    o = dict(coeff=np.zeros((2, UV_NBLK, n), np.int32), qcoeff=np.zeros((2, UV_NBLK, n), np.int32), dqcoeff=np.zeros((2, UV_NBLK, n), np.int32),
             eob=np.zeros((2, UV_NBLK), np.uint16), dist=np.zeros((2, 2, UV_NBLK, 2), np.uint64), bits=np.zeros((2, UV_NBLK), np.uint64))
    for p in range(2):
        for b in range(UV_NBLK):
            x = mfl.aligned((h, 64), np.int16)
            x[:, :w] = src[p, b].astype(np.int16) - pred[p, b].astype(np.int16)
            co = mfl.aligned(n + 64, np.int32)
            e = np.zeros(1, np.uint64)
            assert R.ref_estimate_transform(ptr(x), ctypes.c_uint32(64), ptr(co), c_int(s), c_int(tx_type), c_int(0), ptr(e)) == 0 and e[0] == 0
            qc, dqc, eob = mfl.aligned(n + 64, np.int32), mfl.aligned(n + 64, np.int32), np.zeros(1, np.uint16)
            getattr(R, mfl.QNAMES[ls][2])(ptr(co), ctypes.c_ssize_t(n), c_int(0), ptr(qrow["zbin"]), ptr(qrow["round"]), ptr(qrow["quant"]),
                                          ptr(qrow["quant_shift"]), ptr(qc), ptr(dqc), ptr(qrow["dequant"]), ptr(eob), ptr(scan), ptr(iscan))
            for asm in (0, 1):
                y = np.zeros(2, np.uint64)
                assert R.ref_picture_full_distortion32(ptr(co), 0, ptr(dqc), 0, c_int(w), c_int(h), c_int(int(eob[0])), c_int(asm), ptr(y)) == 0
                o["dist"][asm, p, b] = y >> np.uint64((1 - ls) * 2)
            o["coeff"][p, b], o["qcoeff"][p, b], o["dqcoeff"][p, b], o["eob"][p, b] = co[:n], qc[:n], dqc[:n], eob[0]
            o["bits"][p, b] = (int(cc[mgc.TXB_SKIP + 2 * int(skip[p, b]) + 1]) if eob[0] == 0 else
                               mgc.np_cost_coeffs_txb(qc[:n], int(eob[0]), s, tx_type, int(skip[p, b]), int(dcs[p, b]), cc, ec, mgc.scan_of(s, tx_type)))
    return o


def ref_uv_stage(s, o, tx_type=0):
    """CuFullDistortionFastTuMode_R, the compiled function, on the restatement's coefficient buffers
    -> (dist [2 flavours, 2 planes, UV_NBLK, 2], bits [2 flavours, 2, UV_NBLK], has_coeff [2 flavours, 2, UV_NBLK])"""
    import make_golden_coeff_rate as mgc
    from svtlibs import TX_H, TX_W
    L = mgc.ref_lib()                                                       # (points the two RTCD slots av1_cost_coeffs_txb calls through)
    L.CuFullDistortionFastTuMode_R.restype = None
    L.CuFullDistortionFastTuMode_R.argtypes = [ctypes.c_void_p] * 8 + [ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int]
    w, h = TX_W[s], TX_H[s]
    n = w * h
    _, _, skip, dcs, cc, ec = uv_inputs(s)
    r = RefMd(np.zeros(RATE_WORDS, np.int32), 1)
    txs_ctx, eob_multi = mgc.cost_index(s)
    at = mgc.OFF_MD_COEFF_FAC_BITS + (txs_ctx * 2 + PLANE_TYPE_UV) * 4 * mgc.COEFF_COST_WORDS
    r.md[at:at + 4 * mgc.COEFF_COST_WORDS].view(np.int32)[:] = cc
    at = mgc.OFF_MD_EOB_FRAC_BITS + (eob_multi * 2 + PLANE_TYPE_UV) * 4 * mgc.EOB_COST_WORDS
    r.md[at:at + 4 * mgc.EOB_COST_WORDS].view(np.int32)[:] = ec
    pcs, ppcs, tqb = np.zeros(SIZEOF_PCS, np.uint8), np.zeros(SIZEOF_PPCS, np.uint8), np.zeros(SIZEOF_TQB, np.uint8)
    put64(pcs, OFF_PCS_PARENT_PCS_PTR, ppcs.ctypes.data)
    desc = {k: np.zeros(SIZEOF_PICDESC, np.uint8) for k in ("coeff", "qcoeff", "dqcoeff")}      # transform, residualQuantCoeff, reconCoeff
    planes = {k: np.zeros((2, n), np.int32) for k in desc}
    for k, d in desc.items():
        put64(d, OFF_PICDESC_BUFFER_CB, planes[k][0].ctypes.data); put64(d, OFF_PICDESC_BUFFER_CR, planes[k][1].ctypes.data)
        put(d, PICDESC_STRIDE_Y, 64)
    put64(tqb, OFF_TQB_TU_TRANS_COEFF2NX2N_PTR, desc["coeff"].ctypes.data)
    put64(r.ctx, OFF_CTX_TRANS_QUANT_BUFFERS_PTR, tqb.ctypes.data)
    put(r.ctx, CTX_FULL_LAMBDA, UV_LAMBDA)
    put64(r.buf[0], OFF_BUF_RESIDUAL_QUANT_COEFF_PTR, desc["qcoeff"].ctypes.data); put64(r.buf[0], OFF_BUF_RECON_COEFF_PTR, desc["dqcoeff"].ctypes.data)
    r.geom[OFF_GEOM_TXSIZE_UV], r.geom[OFF_GEOM_TX_WIDTH_UV], r.geom[OFF_GEOM_TX_HEIGHT_UV] = s, w, h
    r.geom[OFF_GEOM_TXSIZE] = 0
    put(r.cand[0], CAND_TYPE, INTRA_MODE)
    r.cand[0][OFF_CAND_TRANSFORM_TYPE + PLANE_TYPE_UV] = tx_type
    dist, bits, has = np.zeros((2, 2, UV_NBLK, 2), np.uint64), np.zeros((2, 2, UV_NBLK), np.uint64), np.zeros((2, 2, UV_NBLK), np.uint8)
    for asm in (0, 1):
        for b in range(UV_NBLK):
            for k in planes:
                planes[k][:] = o[k][:, b]
            put(r.cu, CU_CB_TXB_SKIP_CONTEXT, int(skip[0, b])); put(r.cu, CU_CB_DC_SIGN_CONTEXT, int(dcs[0, b]))
            put(r.cu, CU_CR_TXB_SKIP_CONTEXT, int(skip[1, b])); put(r.cu, CU_CR_DC_SIGN_CONTEXT, int(dcs[1, b]))
            put(r.cand[0], CAND_U_HAS_COEFF, 1); put(r.cand[0], CAND_V_HAS_COEFF, 1)        # the function clears them first (:1752)
            nz = np.zeros((3, MAX_NUM_OF_TU_PER_CU), np.uint32)
            nz[1, 0], nz[2, 0] = o["eob"][0, b], o["eob"][1, b]
            cbd, crd, cbb, crb = np.zeros(2, np.uint64), np.zeros(2, np.uint64), np.zeros(1, np.uint64), np.zeros(1, np.uint64)
            L.CuFullDistortionFastTuMode_R(None, r.buf[0].ctypes.data, r.ctx.ctypes.data, r.cand[0].ctypes.data, pcs.ctypes.data, cbd.ctypes.data,
                                           crd.ctypes.data, nz.ctypes.data, COMPONENT_CHROMA, cbb.ctypes.data, crb.ctypes.data, asm)
            dist[asm, 0, b], dist[asm, 1, b], bits[asm, 0, b], bits[asm, 1, b] = cbd, crd, cbb[0], crb[0]
            has[asm, 0, b], has[asm, 1, b] = get(r.cand[0], CAND_U_HAS_COEFF), get(r.cand[0], CAND_V_HAS_COEFF)
    return dist, bits, has


def uv_pin(check_ref=True):
    """-> the uv_* arrays of the fixture: per chroma size the restatement's values, asserted equal to the compiled
    CuFullDistortionFastTuMode_R's when check_ref"""
    sizes = uv_sizes()
    out = dict(uv_sizes=np.array(sizes, np.int32), uv_dist=np.zeros((len(sizes), 2, 2, UV_NBLK, 2), np.uint64),
               uv_bits=np.zeros((len(sizes), 2, UV_NBLK), np.uint64), uv_eob=np.zeros((len(sizes), 2, UV_NBLK), np.uint16))
    for i, s in enumerate(sizes):
        o = uv_restatement(s)
        if check_ref:
            dist, bits, has = ref_uv_stage(s, o)
            assert np.array_equal(dist, o["dist"]), ("chroma distortion pair", s)
            assert np.array_equal(bits[0], o["bits"]) and np.array_equal(bits[1], o["bits"]), ("chroma bits", s)
            assert np.array_equal(has[0], o["eob"] != 0) and np.array_equal(has[1], o["eob"] != 0), ("u / v_has_coeff", s)
        out["uv_dist"][i], out["uv_bits"][i], out["uv_eob"][i] = o["dist"], o["bits"], o["eob"]
    # the cases are met: both kernels of picture_full_distortion32_bits, both shifts, distortion the shift changes
    assert (out["uv_eob"] == 0).any() and (out["uv_eob"] != 0).any()
    from svtlibs import TX_H, TX_W
    assert {1 if TX_W[s] * TX_H[s] > 256 else 0 for s in sizes} == {0, 1} and max(TX_W[s] * TX_H[s] for s in sizes) == 1024
    return out


def ref_md_decide(L, z, k):
    """the case through the compiled reference -> (DEC_DTYPE [nb], dict of per-slot arrays)"""
    c = case_inputs(z, k)
    nb, n = c["nb"], c["n"]
    r = RefMd(z["rates"], n)
    S = {key: np.zeros((nb, n), np.uint64 if key != "skip_flag" else np.uint8) for key in SLOT_KEYS}
    dec = np.zeros(nb, DEC_DTYPE)
    glue, _ = glue_md_decide(z, k)
    for b in range(nb):
        r.block(c["bsize"], c["has_uv"][b], c["skip_ctx"][b])
        for s in range(n):
            kw = dict(intra=c["intra"][b, s], merge=c["merge"][b, s], mode=c["mode"][b, s], uv_mode=c["uv_mode"][b, s], idx=c["cfl_idx"][b, s],
                      signs=c["cfl_signs"][b, s], rate=c["rate"][b, s], yd=c["yd"][b, s], cbd=c["cd"][0, b, s], crd=c["cd"][1, b, s],
                      bits=[c["ybits"][b, s], c["cbits"][0, b, s], c["cbits"][1, b, s]], lam=c["lam"], bsize=c["bsize"], yhc=c["yhc"][b, s])
            o = r.slot(L, s, "Av1FullCost" if c["intra"][b, s] else "av1_inter_full_cost", **kw)
            if c["merge"][b, s]:
                assert r.slot(L, s, "Av1MergeSkipFullCost", **kw) == o
            for key in SLOT_KEYS:
                S[key][b, s] = o[key]
        count = glue_count(c, S["cost"], b)
        d = r.decide(L, count)
        w = d["slot"]
        one = assemble(c, S, np.full(nb, count), np.full(nb, w), np.full(nb, d["best_intra_mode"]))[b]
        # what the reference's decision stored agrees with the winner's buffer
        assert d["cost"] == int(S["cost"][b, w]) and d["is_intra"] == int(c["intra"][b, w]) and d["skip_flag"] == int(S["skip_flag"][b, w])
        assert not d["is_intra"] or d["cost_luma"] == int(S["cost_luma"][b, w])
        assert not c["merge"][b, w] or (d["merge_cost"], d["skip_cost"]) == (int(S["merge_cost"][b, w]), int(S["skip_cost"][b, w]))
        dec[b] = one
    assert np.array_equal(dec, glue), k                                                     # the mirrored arg-min equals the compiled one
    return dec, S


# ---------------------------------------------------------------------------------------------------------------------------
# cases
# ---------------------------------------------------------------------------------------------------------------------------
#        bsize  n  ninter nintra lambda  I-slice escape chroma cfl
CASES = ((3,    12, 10,    9,    29041,      0,   1,    1,    1),       # 8x8
         (6,    3,  4,     5,    1873,       0,   2,    1,    1),       # 16x16
         (9,    2,  3,     2,    29041,      0,   0,    1,    0),       # 32x32
         (0,    3,  2,     11,   511,        1,   2,    1,    1),       # 4x4, I slice (the inter entries are synthetic: nothing must escape)
         (12,   40, 30,    13,   0xFFFFFFFF, 0,   1,    1,    1),       # 64x64: isCflAllowed 0
         (21,   1,  0,     3,    1,          0,   1,    0,    0),       # 64x16, intra only, no chroma arrays
         (19,   12, 64,    0,    977,        0,   2,    0,    0))       # 32x8, inter only, no chroma arrays
NCASES = len(CASES)
NBLOCKS = 24


def make_rates():
    rng = np.random.default_rng(1807)
    r = rng.integers(0, 1 << 13, RATE_WORDS).astype(np.int32)
    T = rate_tables(r)
    T["intraUVmodeFacBits"][:, 3, UV_DC_PRED] = 8000                      # mode 3: CfL far cheaper than DC, so the -= can pass below zero
    T["intraUVmodeFacBits"][:, 3, UV_CFL_PRED] = 3
    T["cflAlphaFacBits"][2, :, 1] = 1
    return np.concatenate([T[name].reshape(-1) for name, _ in RATE_TABLES]).astype(np.int32)


def tie_bits(lam, skip_rate):
    """-> (bits, d_res, d_pred) of a merge slot without fast rates whose merge cost EQUALS its skip cost"""
    x = (skip_rate * lam + 256) >> 9
    for b in range(1, 1 << 16):
        y = (b * lam + 256) >> 9
        if (y - x) % 128 == 0:
            m = (y - x) // 128                                              # y + 128 d_res == x + 128 d_pred
            return b, 900 + max(-m, 0), 900 + max(m, 0)
    raise AssertionError((lam, skip_rate))


def make_case(k, rates):
    bsize, n, ninter, nintra, lam, islice, escape, chroma, cfl = CASES[k]
    rng = np.random.default_rng(5100 + k)
    nb, T = NBLOCKS, rate_tables(rates)
    modes = rng.permutation(13)[:nintra].astype(np.uint8)
    if nintra > 3:
        modes[0] = 3
    luma, cflrec = np.zeros((nb, n), TX_DEC_DTYPE), np.zeros((nb, n), CFL_DEC_DTYPE)
    cand_out, blk = np.zeros((nb, n), CAND_DTYPE), np.zeros(nb, BLK_DTYPE)
    luma["cost"] = rng.integers(0, 1 << 62, (nb, n))                       # never read
    luma["dist"] = rng.integers(0, 1 << 21, (nb, n, 2))
    luma["bits"] = rng.integers(0, 1 << 16, (nb, n))
    luma["eob"] = rng.integers(1, 1025, (nb, n)) * (rng.random((nb, n)) < 0.6)
    luma["has_coeff"] = luma["eob"] != 0
    luma["tx_type"] = rng.integers(0, 16, (nb, n)); luma["type_index"] = rng.integers(0, 16, (nb, n))
    cdist = rng.integers(0, 1 << 19, (2, nb, n, 2)).astype(np.uint64)
    cbits = rng.integers(0, 1 << 14, (2, nb, n)).astype(np.uint64)
    ceob = (rng.integers(1, 257, (2, nb, n)) * (rng.random((2, nb, n)) < 0.6)).astype(np.uint16)
    rate = rng.integers(0, 1 << 14, (nb, n, 2)).astype(np.uint32)
    cand = np.stack([rng.permutation(ninter + nintra)[:n] for _ in range(nb)]).astype(np.uint8)
    cand_out["flags"] = (rng.integers(0, 16, (nb, n)) & 0xFE) | (rng.random((nb, n)) < 0.4)
    cand_out["pred_mode"] = rng.integers(13, 25, (nb, n)); cand_out["ref_frame_type"] = rng.integers(1, 29, (nb, n))
    cand_out["pred_mv"] = rng.integers(-512, 512, (nb, n, 2, 2)); cand_out["mode_ctx"] = rng.integers(0, 1 << 10, (nb, n))
    iscfl = rng.random((nb, n)) < 0.6
    cflrec["uv_mode"] = np.where(iscfl, 13, rng.choice([0, 0, 0, 1, 9, 12], (nb, n)))
    cflrec["cfl_alpha_idx"] = np.where(iscfl, rng.integers(0, 256, (nb, n)), 0)
    cflrec["cfl_alpha_signs"] = np.where(iscfl, rng.integers(0, 8, (nb, n)), 0)
    cflrec["best_rd"] = rng.integers(0, 1 << 40, (nb, n)); cflrec["dc_rd"] = rng.integers(0, 1 << 40, (nb, n))
    cflrec["alpha_q3"] = rng.integers(-16, 17, (nb, n, 2))
    blk["skip_flag_context"] = rng.integers(0, 3, nb); blk["has_uv"] = rng.random(nb) < 0.7

    pinned = {}

    def slot(b, s, kind, d0, d1=0, bits=0, eob=0, r=(0, 0), c=None):
        """a slot whose cost is easy to place: no chroma contribution (the block's has_uv is cleared by the caller where that matters)"""
        luma["dist"][b, s] = (d0, d1); luma["bits"][b, s] = bits; luma["eob"][b, s] = eob; luma["has_coeff"][b, s] = eob != 0
        rate[b, s] = r
        pool = range(ninter, ninter + nintra) if kind == "intra" else range(ninter)
        used = set(int(v) for i, v in enumerate(cand[b]) if i != s)
        free = [v for v in pool if v not in used]
        pinned.setdefault(b, set()).add(s)
        if c is not None:
            cand[b, s] = c
        elif int(cand[b, s]) in pool:
            pass
        elif free:
            cand[b, s] = free[0]
        else:                                                               # every index of the kind is taken: trade with a slot not placed yet
            s2 = next(i for i in range(n) if i not in pinned[b] and int(cand[b, i]) in pool)
            cand[b, s], cand[b, s2] = cand[b, s2], cand[b, s]
        cand_out["flags"][b, s] = (int(cand_out["flags"][b, s]) & 0xFE) | int(kind == "merge")

    both = ninter > 0 and nintra > 0 and n >= 3
    if both:
        for b in range(8):
            blk["has_uv"][b] = 0
        skip_rate = lambda b: int(T["skipModeFacBits"][int(blk["skip_flag_context"][b]), 1])
        # 0: a merge slot whose skip cost equals its merge cost, and the lowest of the block: skip
        tb, dr, dp = tie_bits(lam, skip_rate(0))
        slot(0, 0, "merge", dr, dp, bits=tb, eob=4)
        slot(0, 1, "inter", 1 << 22, eob=3); slot(0, 2, "intra", 1 << 22, eob=3)
        # 1: skip wins (a small prediction distortion), 2: merge wins
        slot(1, 0, "merge", 1 << 20, 5, bits=3000, eob=9); slot(2, 0, "merge", 7, 1 << 20, bits=10, eob=2)
        # 3: two slots with equal cost, the lowest of the block: the earlier wins
        slot(3, 0, "inter", 1 << 22, eob=5); slot(3, 1, "intra", 40, bits=777, eob=1, r=(5, 0)); slot(3, 2, "intra", 40, bits=777, eob=8, r=(5, 0))
        cflrec["uv_mode"][3, 1:3] = 0
        # 4: the escape fires at slot 1 (escape 1: the intra slot; escape 2: any slot) and cuts off the lowest cost of all
        slot(4, 0, "inter", 5000, eob=0); slot(4, 1, "intra", 3, eob=2); slot(4, 2, "inter" if escape == 2 else "intra", 9000, eob=2)
        # 5: an inter cost of 2^32 or more never becomes bestfullCost: nothing escapes although its luma has no coefficient
        slot(5, 0, "inter", 1 << 25, eob=0); slot(5, 1, "intra", 1 << 26, eob=2); slot(5, 2, "intra", 1 << 27, eob=2)
        # 6: the same just below 2^32: the intra slot escapes
        slot(6, 0, "inter", (1 << 25) - 1, eob=0); slot(6, 1, "intra", 1 << 20, eob=2); slot(6, 2, "intra", 1 << 27, eob=2)
        # 7: a later, cheaper inter slot with coefficients takes the escape back
        slot(7, 0, "inter", 5000, eob=0); slot(7, 1, "inter", 4000, eob=6); slot(7, 2, "intra", 100, eob=0)
        for b in (4, 5, 6, 7):                                              # the other slots cost more, whatever they are
            luma["dist"][b, 3:] = (1 << 23) + 5
    if nintra > 3 and cfl:
        # 8: the -= passes below zero: mode 3, signs 2, idx 0x11, no fast chroma rate (has_uv set)
        blk["has_uv"][8] = 1
        slot(8, 0, "intra", 100, eob=1, c=ninter)
        cflrec["uv_mode"][8, 0], cflrec["cfl_alpha_idx"][8, 0], cflrec["cfl_alpha_signs"][8, 0] = 13, 0x11, 2
    # 9: dist * 128 wraps
    luma["dist"][9, n - 1, 0] = (1 << 57) + 2
    return dict(bsize=np.int32(bsize), n=np.int32(n), ninter=np.int32(ninter), nintra=np.int32(nintra), lam=np.uint64(lam),
                slice_is_intra=np.int32(islice), escape=np.int32(escape), has_chroma=np.int32(chroma), has_cfl=np.int32(cfl), modes=modes,
                luma=luma.view(np.uint8).reshape(nb, n, 40), cdist=cdist, cbits=cbits, ceob=ceob, rate=rate, cand=cand,
                cand_out=cand_out.view(np.uint8).reshape(nb, n, 16), cfl=cflrec.view(np.uint8).reshape(nb, n, 32), blk=blk.view(np.uint8).reshape(nb, 4))


def decisions(z, k):
    return z[f"c{k}_decision"].view(DEC_DTYPE).reshape(-1)


def slot_values(z, k):
    return {key: z[f"c{k}_{key}"] for key in SLOT_KEYS}


def check_conditions(z):
    """the fixture cannot miss the hard paths (the list of the cases the decide must meet)"""
    f = dict.fromkeys(("tie_skip", "skip_wins", "merge_wins", "equal_cost_earlier", "escape1", "escape2", "cut_off_lowest", "above_2_32_no_escape",
                       "below_2_32_escape", "islice_would_escape", "cfl_alphas", "cfl_fell_back", "has_uv0", "has_uv1", "eob0_y", "eob0_u", "eob0_v",
                       "sub_wraps", "dist_wraps", "no_intra", "cfl_not_allowed"), False)
    ns = set()
    for k in range(NCASES):
        c, dec, S = case_inputs(z, k), decisions(z, k), slot_values(z, k)
        cost, n = S["cost"], c["n"]
        ns.add(n)
        m = c["merge"]
        f["tie_skip"] |= bool((m & (S["skip_cost"] == S["merge_cost"]) & (S["skip_flag"] == 1)).any())
        f["skip_wins"] |= bool((m & (S["skip_cost"] < S["merge_cost"])).any())
        f["merge_wins"] |= bool((m & (S["skip_cost"] > S["merge_cost"]) & (S["skip_flag"] == 0)).any())
        for b in range(c["nb"]):
            w, cnt = int(dec["slot"][b]), int(dec["count"][b])
            f["equal_cost_earlier"] |= bool((cost[b, w + 1:cnt] == cost[b, w]).any())
            if cnt < n and not c["slice_is_intra"]:
                f[f"escape{c['escape']}"] = True
                f["cut_off_lowest"] |= int(cost[b].argmin()) == cnt and int(cost[b, cnt]) < int(dec["cost"][b])
            inter_zero = ~c["intra"][b] & (c["yhc"][b] == 0)
            if c["escape"] and not c["slice_is_intra"] and inter_zero[0] and c["intra"][b, 1:].any():
                first_intra = 1 + int(c["intra"][b, 1:].argmax())
                if not (~c["intra"][b, 1:first_intra]).any():
                    f["above_2_32_no_escape"] |= int(cost[b, 0]) >= 1 << 32 and cnt > first_intra
                    f["below_2_32_escape"] |= (1 << 31) <= int(cost[b, 0]) < (1 << 32) - 1 and cnt == first_intra
            f["no_intra"] |= int(dec["best_intra_mode"][b]) == NO_INTRA
        if c["slice_is_intra"] and c["escape"]:
            z2 = dict(z); z2[f"c{k}_slice_is_intra"] = np.int32(0)
            f["islice_would_escape"] |= bool((np_md_decide(z2, k)[0]["count"] < n).any()) and bool((dec["count"] == n).all())
        is_cfl = c["uv_mode"] == UV_CFL_PRED
        f["cfl_alphas"] |= bool((is_cfl & (c["cfl_idx"] != 0) & (c["cfl_signs"] != 0)).any())
        f["cfl_not_allowed"] |= bool(is_cfl.any()) and not cfl_allowed(c["bsize"])
        raw = z[f"c{k}_cfl"].view(CFL_DEC_DTYPE)[..., 0]
        f["cfl_fell_back"] |= bool((c["intra"] & c["has_uv"][:, None] & bool(c["has_cfl"]) & (raw["uv_mode"] == 0)).any())
        f["has_uv0"] |= bool((~c["has_uv"]).any()); f["has_uv1"] |= bool(c["has_uv"].any() and c["has_chroma"])
        for p, key in enumerate(("eob0_y", "eob0_u", "eob0_v")):
            others = [q for q in range(3) if q != p]
            f[key] |= bool(((dec["eob"][:, p] == 0) & (dec["eob"][:, others[0]] != 0) & (dec["eob"][:, others[1]] != 0)).any())
        T = rate_tables(z["rates"])
        uvt = T["intraUVmodeFacBits"][cfl_allowed(c["bsize"])]
        extra = (T["cflAlphaFacBits"][np.minimum(c["cfl_signs"], 7), 0, c["cfl_idx"] >> 4].astype(np.int64) + T["cflAlphaFacBits"][np.minimum(c["cfl_signs"], 7), 1, c["cfl_idx"] & 15]
                 + uvt[c["mode"], 13] - uvt[c["mode"], 0])
        f["sub_wraps"] |= bool((is_cfl & (c["rate"][..., 1].astype(np.int64) + extra < 0)).any())
        f["dist_wraps"] |= bool((c["yd"][..., 0] >= np.uint64(1 << 57)).any())
    assert {1, 2, 3, 12, 40} <= ns, ns
    assert all(f.values()), {key: v for key, v in f.items() if not v}


def main():
    L = ref_lib()
    if L is None:
        raise SystemExit("oracle/_ref/libsvtref.so is not built")
    self_check(L)
    out = {"rates": make_rates()}
    out.update(uv_pin())
    for k in range(NCASES):
        for key, v in make_case(k, out["rates"]).items():
            out[f"c{k}_{key}"] = v
        dec, S = ref_md_decide(L, out, k)
        g_dec, g_S = glue_md_decide(out, k)                                 # restatement 1, costs included
        n_dec, n_cost = np_md_decide(out, k)                                # restatement 2
        for key in SLOT_KEYS:
            assert np.array_equal(S[key], g_S[key]), (k, key)
        assert np.array_equal(dec, g_dec) and np.array_equal(dec, n_dec) and np.array_equal(S["cost"], n_cost), k
        out[f"c{k}_decision"] = dec.view(np.uint8).reshape(-1, DEC_DTYPE.itemsize)
        for key in SLOT_KEYS:
            out[f"c{k}_{key}"] = S[key]
    check_conditions(out)
    np.savez_compressed(OUT, **out)
    print(f"wrote {OUT}: {os.path.getsize(OUT)} bytes")


if __name__ == "__main__":
    main()

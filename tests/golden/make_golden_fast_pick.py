"""Writes tests/golden/fast_pick.npz: inputs and expected outputs of svt_hip_fast_pick_frame (fast cost of every intra candidate, the
buffer walk that keeps the N best, the two index arrays).

What is pinned to what.  Everything below is the reference's code RESTATED in Python integers, next to the line numbers it follows, and
is what runs where the compiled reference is absent:

  ref_model_rd        model_rd_from_sse -> av1_model_rd_from_var_lapndz -> model_rd_norm, EbInterPrediction.c:3311-3438
  ref_intra_fast_cost av1_intra_fast_cost, EbRateDistortionCost.c:598-728 (the non-intrabc branch); RDCOST, EbRateDistortionCost.h:71-75
  ref_walk_buffers    perform_fast_loop's second loop, EbProductCodingLoop.c:1225-1363, as md_encode_block calls it (:3103-3131)
  ref_sort            sort_fast_loop_candidates, EbModeDecision.c:436-489
  ref_fast_pick       the four over the blocks of a case

Where oracle/_ref/libsvtref.so exists (oracle/ref_md.c holds the harness), main() and tests/test_fast_pick_cpu.py take, for every block
and candidate of all 28 cases, the cost and the two rates from the reference's own av1_intra_fast_cost (lib_fast_costs), the SSD pieces
from its model_rd_from_sse (lib_model_rd) and the two index arrays and ref_fast_cost from its sort_fast_loop_candidates on the walk's
buffers (lib_sort), and assert ref_intra_fast_cost, ref_model_rd, ref_sort, np_fast_pick and every stored output equal to them
(check_case_against_reference); model_rd_edges() adds the model's edges.  has_chroma = has_uv && is_chroma_reference(mi_row, mi_col,
bsize, 1, 1) (EbRateDistortionCost.c:33-40) is asserted against the reference's function for every block size and parity.  The buffer
walk between cost and order is pinned by tests/golden/fast_search_ref.npz (make_golden_fast_search_ref.py): whole blocks through the
reference's inject_intra_candidates -> perform_fast_loop -> sort_fast_loop_candidates, which ref_fast_pick and np_fast_pick must
reproduce.  What remains a restatement because it is the caller's: inter candidates, the first (src-to-src) loop, the intrabc branch.

np_fast_pick is the vectorised restatement the tests import: the costs in numpy uint64, and the walk in the form the kernel runs it
(ranks of the costs, "first buffer of the largest rank" for the re-scan, one rotation per bubble pass); main() asserts that it equals
ref_fast_pick on every case.

Inputs: the sad / ssd_c tables of tests/golden/fast_loop.npz (12 blocks per size; its uniform blocks give many equal distortions) and
small synthetic tables; seeded random contexts, rate tables and chroma distortions.  Every cost stays below MAX_CU_COST.
"""
import ctypes
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
OUT = os.path.join(HERE, "fast_pick.npz")
FAST_LOOP = os.path.join(HERE, "fast_loop.npz")
REF = os.path.join(ROOT, "oracle", "_ref", "libsvtref.so")

U32, U64 = (1 << 32) - 1, (1 << 64) - 1
MAX_CU_COST = U64 >> 1                       # EbCodingUnit.h:40
MAX_MODE_COST = 13616969489728 * 8           # EbCodingUnit.h:41
MAX_NFL = 40                                 # EbDefinitions.h:177
SAD, SSD = 0, 1
LAMBDAS = (1, 29041, 0xFFFFFFFF)             # as make_golden_tx_decide.py
UV_CFL_PRED = 13
EMPTY = 127

# EbDefinitions.h:1213, 1311, 1315
INTRA_MODE_CONTEXT = (0, 1, 2, 3, 4, 4, 4, 4, 3, 0, 1, 2, 0)
SIZE_GROUP = (0, 0, 0, 1, 1, 1, 2, 2, 2, 3, 3, 3, 3, 3, 3, 3, 0, 0, 1, 1, 2, 2)
NUM_PELS_LOG2 = (4, 5, 5, 6, 7, 7, 8, 9, 9, 10, 11, 11, 12, 13, 13, 14, 6, 6, 8, 8, 10, 10)
# block_size order: (width, height)
BSIZE_WH = ((4, 4), (4, 8), (8, 4), (8, 8), (8, 16), (16, 8), (16, 16), (16, 32), (32, 16), (32, 32), (32, 64), (64, 32), (64, 64), (64, 128),
            (128, 64), (128, 128), (4, 16), (16, 4), (8, 32), (32, 8), (16, 64), (64, 16))
TX_W = (4, 8, 16, 32, 64, 4, 8, 8, 16, 16, 32, 32, 64, 4, 16, 8, 32, 16, 64)
TX_H = (4, 8, 16, 32, 64, 8, 4, 16, 8, 32, 16, 64, 32, 16, 4, 32, 8, 64, 16)
RATE_TABLES = (("yModeFacBits", (5, 5, 14)), ("mbModeFacBits", (4, 14)), ("intraUVmodeFacBits", (2, 13, 15)), ("angleDeltaFacBits", (8, 8)),
               ("skipModeFacBits", (3, 3)), ("intraInterFacBits", (4, 2)))        # EbMdRateEstimation.h:59, 93-103; CDF_SIZE(x) = x + 1
BLK_DTYPE = np.dtype([("top_mode", "u1"), ("left_mode", "u1"), ("skip_mode_ctx", "u1"), ("is_inter_ctx", "u1"), ("has_chroma", "u1"), ("pad", "u1", (3,))])
OUTPUTS = ("cand", "sorted", "cost", "rate", "ref_fast_cost", "all_cost")

# model_rd_norm's tables, EbInterPrediction.c:3324-3366
RATE_TAB_Q10 = (65536, 6086, 5574, 5275, 5063, 4899, 4764, 4651, 4553, 4389, 4255, 4142, 4044, 3958, 3881, 3811, 3748, 3635, 3538, 3453, 3376,
                3307, 3244, 3186, 3133, 3037, 2952, 2877, 2809, 2747, 2690, 2638, 2589, 2501, 2423, 2353, 2290, 2232, 2179, 2130, 2084, 2001,
                1928, 1862, 1802, 1748, 1698, 1651, 1608, 1530, 1460, 1398, 1342, 1290, 1243, 1199, 1159, 1086, 1021, 963, 911, 864, 821, 781,
                745, 680, 623, 574, 530, 490, 455, 424, 395, 345, 304, 269, 239, 213, 190, 171, 154, 126, 104, 87, 73, 61, 52, 44, 38, 28, 21,
                16, 12, 10, 8, 6, 5, 3, 2, 1, 1, 1, 0, 0)
DIST_TAB_Q10 = (0, 0, 1, 1, 1, 2, 2, 2, 3, 3, 4, 5, 5, 6, 7, 7, 8, 9, 11, 12, 13, 15, 16, 17, 18, 21, 24, 26, 29, 31, 34, 36, 39, 44, 49, 54, 59,
                64, 69, 73, 78, 88, 97, 106, 115, 124, 133, 142, 151, 167, 184, 200, 215, 231, 245, 260, 274, 301, 327, 351, 375, 397, 418, 439,
                458, 495, 528, 559, 587, 613, 637, 659, 680, 717, 749, 777, 801, 823, 842, 859, 874, 899, 919, 936, 949, 960, 969, 977, 983, 994,
                1001, 1006, 1010, 1013, 1015, 1017, 1018, 1020, 1022, 1022, 1023, 1023, 1023, 1024)
XSQ_IQ_Q10 = (0, 4, 8, 12, 16, 20, 24, 28, 32, 40, 48, 56, 64, 72, 80, 88, 96, 112, 128, 144, 160, 176, 192, 208, 224, 256, 288, 320, 352, 384, 416,
              448, 480, 544, 608, 672, 736, 800, 864, 928, 992, 1120, 1248, 1376, 1504, 1632, 1760, 1888, 2016, 2272, 2528, 2784, 3040, 3296, 3552,
              3808, 4064, 4576, 5088, 5600, 6112, 6624, 7136, 7648, 8160, 9184, 10208, 11232, 12256, 13280, 14304, 15328, 16352, 18400, 20448,
              22496, 24544, 26592, 28640, 30688, 32736, 36832, 40928, 45024, 49120, 53216, 57312, 61408, 65504, 73696, 81888, 90080, 98272, 106464,
              114656, 122848, 131040, 147424, 163808, 180192, 196576, 212960, 229344, 245728)
MAX_XSQ_Q10 = 245727
assert len(RATE_TAB_Q10) == len(DIST_TAB_Q10) == len(XSQ_IQ_Q10) == 104
# the closed form the kernel uses instead of the third table
assert all(XSQ_IQ_Q10[xq] == ((((xq & 7) + 8) << (xq >> 3)) - 8) << 2 for xq in range(104))


def bsize_of(w, h):
    return BSIZE_WH.index((w, h))


def bsizes_of_tx(s):
    """(bsize, bsize_uv) of a block of the transform size's shape, 4:2:0 (chroma halves, at least 4)"""
    w, h = TX_W[s], TX_H[s]
    return bsize_of(w, h), bsize_of(max(w >> 1, 4), max(h >> 1, 4))


def np_is_chroma_reference(mi_row, mi_col, bsize, ss_x=1, ss_y=1):
    """is_chroma_reference, EbRateDistortionCost.c:33-40 (mi_size_wide / mi_size_high: the block's width / height in 4-sample units)"""
    bw, bh = BSIZE_WH[bsize][0] >> 2, BSIZE_WH[bsize][1] >> 2
    return int(((mi_row & 1) or not (bh & 1) or not ss_y) and ((mi_col & 1) or not (bw & 1) or not ss_x))


# ---- the reference's loops in Python integers -------------------------------------------------------------------------------------
def ref_model_rd_norm(xsq_q10):
    """:3311-3375 -> (r_q10, d_q10, xq)"""
    tmp = (xsq_q10 >> 2) + 8                                   # :3367
    k = (tmp.bit_length() - 1) - 3                             # :3368 get_msb
    xq = (k << 3) + ((tmp >> k) & 7)                           # :3369
    a = ((xsq_q10 - XSQ_IQ_Q10[xq]) << 10) >> (2 + k)          # :3371
    b = (1 << 10) - a                                          # :3372
    return (RATE_TAB_Q10[xq] * b + RATE_TAB_Q10[xq + 1] * a) >> 10, (DIST_TAB_Q10[xq] * b + DIST_TAB_Q10[xq + 1] * a) >> 10, xq


def ref_model_rd(sse, n_log2, quantizer):
    """model_rd_from_sse(bsize, quantizer, sse) with n_log2 = num_pels_log2_lookup[bsize] -> (rate, dist)"""
    qstep = quantizer >> 3                                     # :3433, dequant_shift 3
    if sse == 0:                                               # :3386
        return 0, 0
    xsq = min(((((qstep * qstep) << (n_log2 + 10)) & U64) + (sse >> 1)) // sse, MAX_XSQ_Q10)    # :3393-3395
    r_q10, d_q10, _ = ref_model_rd_norm(xsq)
    rate = ((r_q10 << n_log2) + 1) >> 1                        # :3397 ROUND_POWER_OF_TWO(.., 10 - AV1_PROB_COST_SHIFT)
    dist = (sse * d_q10 + 512) >> 10                           # :3398
    return rate, (dist << 4) & U64                             # :3437


def ref_intra_fast_cost(P, R, blk, c, luma, chroma):
    """av1_intra_fast_cost :598-728 for candidate c of params P, rate tables R, block context blk -> (cost, fast_luma_rate, fast_chroma_rate)"""
    m, uvm = int(P["modes"][c]), int(P["uv_modes"][c])
    w, h = TX_W[P["tx_size"]], TX_H[P["tx_size"]]
    cfl_allowed = int(w <= 32 and h <= 32)                     # :601
    chroma_mode = 0 if uvm == UV_CFL_PRED else uvm             # :606
    directional, uv_directional = 1 <= m <= 8, 1 <= uvm <= 8   # av1_is_directional_mode: V_PRED .. D67_PRED
    cand_use_angle_delta = bool(P["use_angle_delta"]) and directional          # EbModeDecision.c:2444, :2490
    above, left = INTRA_MODE_CONTEXT[blk["top_mode"]], INTRA_MODE_CONTEXT[blk["left_mode"]]       # :625-626
    intra = bool(P["slice_is_intra"])
    mode_bits = 0 if intra else int(R["mbModeFacBits"][SIZE_GROUP[P["bsize"]]][m])              # :627
    skip_rate = 0 if intra else int(R["skipModeFacBits"][blk["skip_mode_ctx"]][0])              # :628
    luma_mode_bits = int(R["yModeFacBits"][above][left][m]) if intra else 0                      # :631
    luma_ang = int(R["angleDeltaFacBits"][m - 1][3 + int(P["deltas"][c])]) if directional and cand_use_angle_delta else 0     # :633-637
    chroma_bits = chroma_ang = 0
    if blk["has_chroma"]:                                      # :666-667
        chroma_bits = int(R["intraUVmodeFacBits"][cfl_allowed][m][chroma_mode])                   # :669
        if uv_directional and cand_use_angle_delta:
            chroma_ang = int(R["angleDeltaFacBits"][chroma_mode - 1][3 + int(P["uv_deltas"][c])])  # :672
    is_inter_rate = 0 if intra else int(R["intraInterFacBits"][blk["is_inter_ctx"]][0])          # :677
    luma_rate = (mode_bits + skip_rate + luma_mode_bits + luma_ang + is_inter_rate) & U32          # :678, uint32_t
    luma_rate = (luma_rate + P["intrabc_bits"]) & U32          # :679-680
    chroma_rate = (chroma_bits + chroma_ang) & U32             # :682
    fast_luma_rate, fast_chroma_rate = luma_rate, chroma_rate  # :685-686
    if P["metric"] == SSD:                                     # :687-716
        rate, total = ref_model_rd(luma, NUM_PELS_LOG2[P["bsize"]], P["ac_dequant_q3"])
        luma_rate = (luma_rate + rate) & U32                   # :700
        chroma_rate, chroma_dist = ref_model_rd(chroma, NUM_PELS_LOG2[P["bsize_uv"]], P["ac_dequant_q3"])     # :704-710: written OVER chromaRate
        total = (total + chroma_dist) & U64
    else:
        total = (luma + chroma) & U64                          # :719-721
    rate = (luma_rate + chroma_rate) & U32                     # :713 / :723
    cost = ((((rate * P["lambda"] + 256) & U64) >> 9) + ((total * 128) & U64)) & U64              # RDCOST
    return cost, fast_luma_rate, fast_chroma_rate


def ref_walk_buffers(costs, nfl):
    """the second loop of perform_fast_loop on one block's costs (list index order) -> fast_cost[nbuf], cand_of[nbuf], n"""
    ncand = len(costs)
    n = min(ncand, nfl)                                        # EbProductCodingLoop.c:3105
    scratch = ncand > n                                        # :3127
    nbuf = n + 1 if scratch else n                             # :3108
    fast_cost = [MAX_CU_COST] * nbuf                           # :1070
    cand_of = [0] * nbuf
    hi = 0                                                     # :1225
    idx = ncand - 1                                            # :1226
    while idx >= 0:                                            # :1227
        fast_cost[hi], cand_of[hi] = costs[idx], idx           # :1229-1230, :1313
        if idx or scratch:                                     # :1331
            hi, b = 0, 1                                       # :1344-1345
            while True:
                highest = fast_cost[hi]                        # :1348
                if highest == MAX_CU_COST:                     # :1349
                    break
                if fast_cost[b] > highest:                     # :1352
                    hi = b
                b += 1
                if not b < nbuf:                               # :1355
                    break
        idx -= 1
    if scratch:
        fast_cost[hi] = MAX_CU_COST                            # :1361
    return fast_cost, cand_of, n


def ref_sort(fast_cost, n):
    """sort_fast_loop_candidates on the buffers' costs, all candidates intra -> best[nbuf], sorted[n] (buffer indices), ref_fast_cost"""
    nbuf = len(fast_cost)
    best = [0] * nbuf                                          # EbModeDecision.c:447-456
    start, end = 0, nbuf - 1
    for b in range(nbuf):
        if fast_cost[b] == MAX_CU_COST:
            best[end] = b
            end -= 1
        else:
            best[start] = b
            start += 1
    ref_fast_cost = MAX_MODE_COST                              # EbProductCodingLoop.c:3133
    for i in range(n):                                         # :472-476: BUFFERS 0 .. n-1
        if fast_cost[i] < ref_fast_cost:
            ref_fast_cost = fast_cost[i]
    srt = list(best[:n])                                       # :477-479
    for i in range(n - 1):                                     # :480-488: the costs of BUFFERS i and j
        for j in range(i + 1, n):
            if fast_cost[j] < fast_cost[i]:
                srt[i], srt[j] = srt[j], srt[i]
    return best, srt, ref_fast_cost


def slots_of(best, srt, cand_of, n):
    """the interface's form of the two arrays: cand[k] = the list index in slot k, sorted[k] = the SLOT of buffer srt[k]"""
    slot_of = {b: k for k, b in enumerate(best)}
    return [cand_of[best[k]] for k in range(n)], [slot_of[b] for b in srt]


def ref_walk(costs, nfl):
    """perform_fast_loop's second loop and sort_fast_loop_candidates on one block's costs -> cand[n], sorted as slots [n], ref_fast_cost"""
    fast_cost, cand_of, n = ref_walk_buffers(costs, nfl)
    best, srt, ref_fast_cost = ref_sort(fast_cost, n)
    cand, slots = slots_of(best, srt, cand_of, n)
    return cand, slots, ref_fast_cost


def rates_dict(packed):
    out, at = {}, 0
    for name, shape in RATE_TABLES:
        k = int(np.prod(shape))
        out[name] = np.asarray(packed[at:at + k]).reshape(shape)
        at += k
    return out


def ref_fast_pick(P, dist, dist_cb, dist_cr, blk, rates):
    """every output of the call for one group, block by block"""
    R = rates_dict(rates)
    B, C = dist.shape
    n = min(P["nfl"], C)
    out = dict(cand=np.zeros((B, n), np.uint8), sorted=np.zeros((B, n), np.uint8), cost=np.zeros((B, n), np.uint64),
               rate=np.zeros((B, n, 2), np.uint32), ref_fast_cost=np.zeros(B, np.uint64), all_cost=np.zeros((B, C), np.uint64))
    for b in range(B):
        rec = {k: int(blk[b][k]) for k in ("top_mode", "left_mode", "skip_mode_ctx", "is_inter_ctx", "has_chroma")}
        res = []
        for c in range(C):
            chroma = (int(dist_cb[b, c]) if dist_cb is not None else 0) + (int(dist_cr[b, c]) if dist_cr is not None else 0)
            res.append(ref_intra_fast_cost(P, R, rec, c, int(dist[b, c]), chroma))
        costs = [r[0] for r in res]
        assert max(costs) < MAX_CU_COST
        cand, srt, ref = ref_walk(costs, P["nfl"])
        out["all_cost"][b] = costs
        out["cand"][b], out["sorted"][b], out["ref_fast_cost"][b] = cand, srt, ref
        out["cost"][b] = [costs[c] for c in cand]
        out["rate"][b] = [[res[c][1], res[c][2]] for c in cand]
    return out


# ---- the vectorised restatement ---------------------------------------------------------------------------------------------------
def np_model_rd(sse, n_log2, quantizer):
    """ref_model_rd on a uint64 array -> (rate uint32, dist uint64)"""
    sse = np.asarray(sse, np.uint64)
    qstep = np.uint64(quantizer >> 3)
    safe = np.maximum(sse, np.uint64(1))
    xsq = np.minimum(((qstep * qstep) << np.uint64(n_log2 + 10)) + (sse >> np.uint64(1)), np.uint64(U64)) // safe
    xsq = np.minimum(xsq, np.uint64(MAX_XSQ_Q10)).astype(np.int64)
    tmp = (xsq >> 2) + 8
    msb = np.zeros(tmp.shape, np.int64)
    for i in range(1, 18):
        msb += (tmp >> i) > 0
    k = msb - 3
    xq = (k << 3) + ((tmp >> k) & 7)
    rt, dt, iq = (np.array(t, np.int64) for t in (RATE_TAB_Q10, DIST_TAB_Q10, XSQ_IQ_Q10))
    a = ((xsq - iq[xq]) << 10) >> (2 + k)
    b = 1024 - a
    r_q10, d_q10 = (rt[xq] * b + rt[xq + 1] * a) >> 10, (dt[xq] * b + dt[xq + 1] * a) >> 10
    rate = (((r_q10 << n_log2) + 1) >> 1).astype(np.uint32)
    dist = ((sse * d_q10.astype(np.uint64) + np.uint64(512)) >> np.uint64(10)) << np.uint64(4)
    zero = sse == 0
    return np.where(zero, np.uint32(0), rate), np.where(zero, np.uint64(0), dist)


def np_fast_costs(P, dist, dist_cb, dist_cr, blk, rates):
    """-> cost uint64 [B, C], fast_luma_rate, fast_chroma_rate uint32 [B, C]"""
    R = rates_dict(np.asarray(rates, np.int32))
    B, C = dist.shape
    m, d = np.asarray(P["modes"][:C], np.int64), np.asarray(P["deltas"][:C], np.int64)
    uvm, uvd = np.asarray(P["uv_modes"][:C], np.int64), np.asarray(P["uv_deltas"][:C], np.int64)
    cm = np.where(uvm == UV_CFL_PRED, 0, uvm)
    use = bool(P["use_angle_delta"]) & (m >= 1) & (m <= 8)
    uv_dir = (uvm >= 1) & (uvm <= 8)
    ctx = np.array(INTRA_MODE_CONTEXT, np.int64)
    top, left = np.minimum(blk["top_mode"], 12).astype(np.int64), np.minimum(blk["left_mode"], 12).astype(np.int64)      # the device clamps
    skip, inter = np.minimum(blk["skip_mode_ctx"], 2).astype(np.int64), np.minimum(blk["is_inter_ctx"], 3).astype(np.int64)
    u32 = lambda a: np.asarray(a).astype(np.int64).astype(np.uint32)             # int32 bits as uint32
    if P["slice_is_intra"]:
        lr = u32(R["yModeFacBits"][ctx[top][:, None], ctx[left][:, None], m[None, :]])
    else:
        lr = u32(R["mbModeFacBits"][SIZE_GROUP[P["bsize"]]][m])[None, :] + u32(R["skipModeFacBits"][skip, 0])[:, None] + u32(R["intraInterFacBits"][inter, 0])[:, None]
    lr = lr + np.where(use, u32(R["angleDeltaFacBits"][np.clip(m - 1, 0, 7), 3 + d]), np.uint32(0))[None, :]
    lr = (lr + np.uint32(P["intrabc_bits"])).astype(np.uint32)
    w, h = TX_W[P["tx_size"]], TX_H[P["tx_size"]]
    cr = u32(R["intraUVmodeFacBits"][int(w <= 32 and h <= 32)][m, cm]) + np.where(use & uv_dir, u32(R["angleDeltaFacBits"][np.clip(cm - 1, 0, 7), 3 + uvd]), np.uint32(0))
    cr = np.where((blk["has_chroma"] != 0)[:, None], cr[None, :], np.uint32(0)).astype(np.uint32)
    luma = np.asarray(dist, np.uint64)
    chroma = np.zeros((B, C), np.uint64)
    for x in (dist_cb, dist_cr):
        if x is not None:
            chroma = chroma + np.asarray(x, np.uint64)
    if P["metric"] == SSD:
        r1, d1 = np_model_rd(luma, NUM_PELS_LOG2[P["bsize"]], P["ac_dequant_q3"])
        r2, d2 = np_model_rd(chroma, NUM_PELS_LOG2[P["bsize_uv"]], P["ac_dequant_q3"])
        rate, total = (lr + r1 + r2).astype(np.uint32), d1 + d2
    else:
        rate, total = (lr + cr).astype(np.uint32), luma + chroma
    cost = ((rate.astype(np.uint64) * np.uint64(P["lambda"]) + np.uint64(256)) >> np.uint64(9)) + total * np.uint64(128)
    return cost, lr, cr


def np_walk(cost, nfl):
    """ref_walk for every row of cost [B, C] at once, on the ranks of the costs -> cand [B, n], sorted [B, n], ref_fast_cost [B]"""
    B, C = cost.shape
    n = min(nfl, C)
    scratch = C > n
    nbuf = n + 1 if scratch else n
    rank = (cost[:, :, None] < cost[:, None, :]).sum(axis=1)                     # rank[b, c] = how many of block b's costs are below cost[b, c]
    rows = np.arange(B)
    brank, bcand = np.full((B, nbuf), EMPTY, np.int64), np.zeros((B, nbuf), np.int64)
    hi = np.zeros(B, np.int64)
    for c in range(C - 1, -1, -1):
        brank[rows, hi], bcand[rows, hi] = rank[:, c], c
        if c or scratch:
            hi = brank.argmax(axis=1)                                            # the first empty buffer, else the first of the maximum
    if scratch:
        brank[rows, hi] = EMPTY
    held = brank != EMPTY
    slot = np.cumsum(held, axis=1) - 1                                           # the empty buffer goes last
    bcost = np.where(held, np.take_along_axis(cost, bcand, axis=1), np.uint64(MAX_CU_COST))
    ref = np.minimum(bcost[:, :n].min(axis=1), np.uint64(MAX_MODE_COST))
    cand = np.zeros((B, n), np.int64)
    r, k = np.nonzero(held)
    cand[r, slot[r, k]] = bcand[r, k]
    # one rotation per bubble pass: position i and the positions j > i whose buffer ranks below buffer i's
    idx = np.arange(n)[None, :]
    srt = np.repeat(idx, B, axis=0)
    for i in range(n - 1):
        J = (idx > i) & (brank[:, :n] < brank[:, i:i + 1])
        mark = np.where(J, idx, -1)
        prev = np.maximum.accumulate(mark, axis=1)
        prev = np.concatenate([np.full((B, 1), -1), prev[:, :-1]], axis=1)       # the member of J below this position
        src = np.where(J, np.where(prev >= 0, prev, i), idx)
        last = mark.max(axis=1)
        src[:, i] = np.where(last >= 0, last, i)
        srt = np.take_along_axis(srt, src, axis=1)
    return cand, srt, ref


def np_fast_pick(P, dist, dist_cb, dist_cr, blk, rates):
    cost, lr, cr = np_fast_costs(P, dist, dist_cb, dist_cr, blk, rates)
    cand, srt, ref = np_walk(cost, P["nfl"])
    pick = lambda a: np.take_along_axis(a, cand, axis=1)
    return dict(cand=cand.astype(np.uint8), sorted=srt.astype(np.uint8), cost=pick(cost), rate=np.stack([pick(lr), pick(cr)], axis=2),
                ref_fast_cost=ref.astype(np.uint64), all_cost=cost)


def np_gather(cand, pred):
    """pred [B, C, ...] -> [B, n, ...]: the survivors in slot order"""
    return np.take_along_axis(pred, cand.astype(np.int64).reshape(cand.shape + (1,) * (pred.ndim - 2)), axis=1)


# ---- the compiled reference (oracle/ref_md.c) ----------------------------------------------------------------------------------------
def plain_ref_lib():
    """libsvtref.so as any build of it is (is_chroma_reference), or None where it is not built"""
    if not os.path.exists(REF):
        return None
    L = ctypes.CDLL(REF)
    L.is_chroma_reference.restype = ctypes.c_int32
    L.is_chroma_reference.argtypes = [ctypes.c_int32] * 5
    return L


def ref_lib():
    """libsvtref.so with the ref_md_* entries typed; None where it is not built, or is a build from before oracle/ref_md.c that could
    not be remade (the reference's sources are not there)"""
    L = plain_ref_lib()
    if L is None or not hasattr(L, "ref_md_fast_search"):
        return None
    vp, u64, i32 = ctypes.c_void_p, ctypes.c_uint64, ctypes.c_int32
    L.ref_md_intra_fast_cost.argtypes = [vp, vp, u64, vp, i32, vp, vp, vp, vp, vp]
    L.ref_md_model_rd_from_sse.argtypes = [i32, i32, u64, vp, vp]
    L.ref_md_model_rd_from_sse.restype = None
    L.ref_md_sort.argtypes = [i32, vp, i32, vp, vp, vp]
    return L


def _p(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def lib_model_rd(L, sse, bsize, quantizer):
    """(b) model_rd_from_sse(bsize, quantizer, sse) -> (rate, dist)"""
    r, d = np.zeros(1, np.uint32), np.zeros(1, np.uint64)
    L.ref_md_model_rd_from_sse(bsize, quantizer, int(sse), _p(r), _p(d))
    return int(r[0]), int(d[0])


def lib_sort(L, fast_cost, n):
    """(c) sort_fast_loop_candidates on the buffers' costs -> best[nbuf], sorted[n], ref_fast_cost"""
    costs = np.array(fast_cost, np.uint64)
    best, srt, ref = np.zeros(MAX_NFL + 2, np.uint8), np.zeros(MAX_NFL, np.uint8), np.zeros(1, np.uint64)
    assert L.ref_md_sort(len(costs), _p(costs), n, _p(best), _p(srt), _p(ref)) == 0
    return best[:len(costs)].tolist(), srt[:n].tolist(), int(ref[0])


def cand_records(P, C):
    """[C, 7] candidates as inject_intra_candidates leaves them (EbModeDecision.c:2439-2458): mode, delta, uv mode, uv delta, the two
    directional flags, use_angle_delta = the block-size flag AND directional luma"""
    m, uvm = np.asarray(P["modes"][:C], np.int32), np.asarray(P["uv_modes"][:C], np.int32)
    d, uvd = np.asarray(P["deltas"][:C], np.int32), np.asarray(P["uv_deltas"][:C], np.int32)
    lum, uv = ((m >= 1) & (m <= 8)).astype(np.int32), ((uvm >= 1) & (uvm <= 8)).astype(np.int32)
    return np.ascontiguousarray(np.stack([m, d, uvm, uvd, lum, uv, lum * int(bool(P["use_angle_delta"]))], axis=1).astype(np.int32))


def lib_fast_costs(L, P, dist, dist_cb, dist_cr, blk, rates, mi):
    """(a) av1_intra_fast_cost on every block and candidate -> cost uint64 [B, C], rate uint32 [B, C, 2].  has_chroma is reached the
    reference's way: blk_geom->has_uv = has_chroma, and a mode-info position at which is_chroma_reference holds (the fixture's own,
    or (1, 1) where the fixture forces has_chroma on a block whose drawn position has none)."""
    B, C = dist.shape
    w, h = TX_W[P["tx_size"]], TX_H[P["tx_size"]]
    cand = cand_records(P, C)
    pic = np.array([P["slice_is_intra"], int(P["intrabc_bits"] != 0), P["intrabc_bits"] & 0x7FFFFFFF, 60, P["ac_dequant_q3"], int(P["metric"] == SSD)], np.int32)
    assert P["intrabc_bits"] < (1 << 31)
    rates = np.ascontiguousarray(rates, np.int32)
    cost, rate = np.zeros((B, C), np.uint64), np.zeros((B, C, 2), np.uint32)
    for b in range(B):
        r, c = int(mi[b][0]), int(mi[b][1])
        if blk[b]["has_chroma"] and not np_is_chroma_reference(r, c, P["bsize"]):
            r, c = r | 1, c | 1
        rec = np.array([blk[b]["top_mode"], blk[b]["left_mode"], blk[b]["skip_mode_ctx"], blk[b]["is_inter_ctx"], r, c, w, h, blk[b]["has_chroma"]], np.int32)
        luma = np.ascontiguousarray(dist[b], np.uint64)
        chroma = np.zeros(C, np.uint64)
        for x in (dist_cb, dist_cr):
            if x is not None:
                chroma = chroma + np.asarray(x[b], np.uint64)
        assert L.ref_md_intra_fast_cost(_p(rec), _p(pic), P["lambda"], _p(rates), C, _p(cand), _p(luma), _p(chroma), _p(cost[b]), _p(rate[b])) == 0
    return cost, rate


def lib_fast_pick(L, P, dist, dist_cb, dist_cr, blk, rates, mi):
    """every output of the call with the costs and rates from (a) and the order from (c); the buffer walk between them is ref_walk_buffers
    (perform_fast_loop itself is pinned through tests/golden/fast_search_ref.npz)"""
    cost, rate = lib_fast_costs(L, P, dist, dist_cb, dist_cr, blk, rates, mi)
    return lib_pick_of(L, P, cost, rate), rate


def lib_pick_of(L, P, cost, rate):
    B, C = cost.shape
    n = min(P["nfl"], C)
    out = dict(cand=np.zeros((B, n), np.uint8), sorted=np.zeros((B, n), np.uint8), cost=np.zeros((B, n), np.uint64),
               rate=np.zeros((B, n, 2), np.uint32), ref_fast_cost=np.zeros(B, np.uint64), all_cost=cost)
    for b in range(B):
        costs = [int(v) for v in cost[b]]
        fast_cost, cand_of, n_ = ref_walk_buffers(costs, P["nfl"])
        best, srt, ref = lib_sort(L, fast_cost, n_)
        assert (best, srt, ref) == ref_sort(fast_cost, n_), b
        cand, slots = slots_of(best, srt, cand_of, n_)
        out["cand"][b], out["sorted"][b], out["ref_fast_cost"][b] = cand, slots, ref
        out["cost"][b] = [costs[c] for c in cand]
        out["rate"][b] = rate[b][cand]
    return out


def check_case_against_reference(L, z, ci):
    """the restatements against the compiled reference on fixture case ci: every block's and candidate's cost and rates through (a),
    the SSD model of every luma and chroma distortion through (b), the order through (c), and with them every stored output"""
    P, dist, cb, cr, blk, rates, want = case_of(z, ci)
    mi = z[f"c{ci}_mi"]
    got, rate_all = lib_fast_pick(L, P, dist, cb, cr, blk, rates, mi)
    for k in OUTPUTS:
        assert got[k].dtype == want[k].dtype and np.array_equal(got[k], want[k]), (CASE_NAMES[ci], k)
    R = rates_dict(rates)
    for b in range(dist.shape[0]):
        rec = {k: int(blk[b][k]) for k in ("top_mode", "left_mode", "skip_mode_ctx", "is_inter_ctx", "has_chroma")}
        for c in range(dist.shape[1]):
            chroma = (int(cb[b, c]) if cb is not None else 0) + (int(cr[b, c]) if cr is not None else 0)
            res = ref_intra_fast_cost(P, R, rec, c, int(dist[b, c]), chroma)
            assert res == (int(got["all_cost"][b, c]), int(rate_all[b, c, 0]), int(rate_all[b, c, 1])), (CASE_NAMES[ci], b, c)
    if P["metric"] == SSD:
        for vals, bs in ((dist, P["bsize"]), (cb, P["bsize_uv"]), (cr, P["bsize_uv"])):
            if vals is not None:
                for sse in np.unique(vals):
                    assert ref_model_rd(int(sse), NUM_PELS_LOG2[bs], P["ac_dequant_q3"]) == lib_model_rd(L, sse, bs, P["ac_dequant_q3"]), (CASE_NAMES[ci], int(sse))
    np_out = np_fast_pick(P, dist, cb, cr, blk, rates)
    for k in OUTPUTS:
        assert np.array_equal(np_out[k], got[k]), (CASE_NAMES[ci], k)


# ---- the cases --------------------------------------------------------------------------------------------------------------------
# name, source (fast_loop.npz size index or a synthetic kind), blocks, nfl, metric, slice_is_intra, chroma distortions, use_angle_delta,
# intrabc_bits, lambda, ac_dequant_q3, uv list, rate tables
CASES = [
    ("4x4_sad_nfl3", 0, 12, 3, SAD, 1, 0, 0, 0, 29041, 0, "luma", "rand"),
    ("4x4_sad_nfl13", 0, 12, 13, SAD, 0, 1, 0, 211, 1, 0, "dc", "rand"),
    ("4x4_ssd_nfl40", 0, 7, 40, SSD, 1, 1, 0, 0, 29041, 156, "luma", "rand"),
    ("4x4_sad_nfl1", 0, 12, 1, SAD, 1, 0, 0, 0, 0xFFFFFFFF, 0, "dc", "rand"),
    ("8x8_sad_nfl3", 1, 12, 3, SAD, 1, 1, 1, 0, 29041, 0, "cfl", "rand"),
    ("8x8_sad_nfl12", 1, 12, 12, SAD, 0, 1, 1, 977, 29041, 0, "dir", "rand"),
    ("8x8_sad_nfl40", 1, 12, 40, SAD, 1, 0, 1, 0, 1, 0, "luma", "rand"),
    ("8x8_sad_nfl1", 1, 12, 1, SAD, 0, 0, 0, 0, 29041, 0, "dc", "rand"),
    ("8x8_ssd_nfl3", 1, 12, 3, SSD, 1, 1, 1, 0, 29041, 156, "dir", "rand"),
    ("8x8_ssd_nfl12", 1, 12, 12, SSD, 0, 1, 1, 1500, 0xFFFFFFFF, 1336, "cfl", "rand"),
    ("8x8_ssd_nfl40", 1, 5, 40, SSD, 0, 0, 0, 0, 1, 8, "luma", "rand"),
    ("8x8_sad_ties", 1, 12, 12, SAD, 1, 0, 1, 0, 29041, 0, "dc", "zero"),
    ("8x8_sad_bigrates", 1, 12, 3, SAD, 0, 1, 1, 0x7FFFFFFF, 29041, 0, "dir", "big"),
    ("4x16_sad_nfl3", 13, 12, 3, SAD, 1, 1, 1, 0, 29041, 0, "dc", "rand"),
    ("4x16_ssd_nfl12", 13, 2, 12, SSD, 0, 1, 1, 0, 29041, 400, "dir", "rand"),
    ("16x4_sad_nfl12", 14, 12, 12, SAD, 0, 0, 1, 33, 1, 0, "luma", "rand"),
    ("16x4_ssd_nfl3", 14, 3, 3, SSD, 1, 1, 0, 0, 0xFFFFFFFF, 156, "cfl", "rand"),
    ("64x64_sad_nfl3", 4, 12, 3, SAD, 1, 1, 1, 0, 29041, 0, "dc", "rand"),
    ("64x64_ssd_nfl12", 4, 4, 12, SSD, 0, 1, 1, 0, 29041, 156, "dir", "rand"),
    ("32x32_ssd_nfl3", 3, 12, 3, SSD, 1, 0, 1, 0, 29041, 60, "cfl", "rand"),
    ("syn_ties3_nfl3", "ties3", 16, 3, SAD, 1, 0, 1, 0, 1, 0, "dc", "zero"),
    ("syn_ties3_nfl12", "ties3", 16, 12, SAD, 1, 0, 1, 0, 29041, 0, "dc", "zero"),
    ("syn_ties3_nfl40", "ties3", 16, 40, SSD, 1, 0, 1, 0, 29041, 156, "dc", "zero"),
    ("syn_rand_nfl5", "rand", 16, 5, SAD, 0, 1, 1, 0, 29041, 0, "dir", "rand"),
    ("syn_one_cand", "one", 4, 3, SAD, 1, 0, 1, 0, 29041, 0, "dc", "rand"),
    ("syn_two_cand_nfl1", "two", 8, 1, SAD, 1, 0, 1, 0, 29041, 0, "dc", "rand"),
    ("syn_64_cand_nfl40", "rand64", 9, 40, SAD, 0, 1, 1, 5, 29041, 0, "dir", "rand"),
    ("syn_ssd_edges", "ssd_edges", 6, 3, SSD, 1, 1, 1, 0, 29041, 1336, "dc", "rand"),
]
NCASES = len(CASES)
CASE_NAMES = [c[0] for c in CASES]


def make_rates(kind, rng):
    parts = []
    for _, shape in RATE_TABLES:
        k = int(np.prod(shape))
        if kind == "zero":
            parts.append(np.zeros(k, np.int32))
        elif kind == "big":
            parts.append(rng.integers(1 << 30, (1 << 31) - 1, k).astype(np.int32))                # sums that wrap uint32
        else:
            parts.append(rng.integers(0, 1 << 13, k).astype(np.int32))
    return np.concatenate(parts)


def make_case(ci, fl):
    name, src, nb, nfl, metric, intra, chroma, uad, ibc, lam, q, uvkind, rkind = CASES[ci]
    rng = np.random.default_rng(9100 + ci)
    if isinstance(src, int):
        tx = src
        modes, deltas = fl[f"s{src}_modes"].astype(np.uint8), fl[f"s{src}_deltas"].astype(np.int8)
        dist = fl[f"s{src}_{'ssd_c' if metric == SSD else 'sad'}"][:nb].astype(np.uint64)
    else:
        tx = 1
        C = {"one": 1, "two": 2, "rand64": 64, "ssd_edges": 8}.get(src, 61)
        modes = (np.arange(C) % 13).astype(np.uint8)
        deltas = np.where((modes >= 1) & (modes <= 8), (np.arange(C) % 7) - 3, 0).astype(np.int8)
        if src == "ties3":
            dist = rng.choice(np.array([100, 101, 4000], np.uint64), (nb, C))
        elif src == "ssd_edges":
            # SSE 0; the largest an 8x8 block has; SSEs around the table's two ends (q = 1336: qstep 167)
            dist = rng.integers(1, 1 << 20, (nb, C)).astype(np.uint64)
            dist[:, 0], dist[:, 1], dist[:, 2], dist[:, 3] = 0, 64 * 255 * 255, 1, 7
        else:
            dist = rng.integers(0, 1 << 16, (nb, C)).astype(np.uint64)
    C = dist.shape[1]
    if uvkind == "luma":
        uv_modes = modes.copy()
    elif uvkind == "cfl":
        uv_modes = np.full(C, UV_CFL_PRED, np.uint8)
        uv_modes[1::5] = 0
    elif uvkind == "dir":
        uv_modes = ((np.arange(C) * 5 + 1) % 14).astype(np.uint8)
    else:
        uv_modes = np.zeros(C, np.uint8)
    uv_deltas = np.where((uv_modes >= 1) & (uv_modes <= 8) & (uvkind == "dir"), (np.arange(C) * 3 % 7) - 3, 0).astype(np.int8)
    bsize, bsize_uv = bsizes_of_tx(tx)
    blk = np.zeros(nb, BLK_DTYPE)
    blk["top_mode"], blk["left_mode"] = rng.integers(0, 13, nb), rng.integers(0, 13, nb)
    blk["skip_mode_ctx"], blk["is_inter_ctx"] = rng.integers(0, 3, nb), rng.integers(0, 4, nb)
    mi = rng.integers(0, 64, (nb, 2))
    has_uv = rng.integers(0, 4, nb) != 0
    blk["has_chroma"] = [int(has_uv[b]) & np_is_chroma_reference(int(mi[b, 0]), int(mi[b, 1]), bsize) for b in range(nb)]
    if nb > 1:
        blk["has_chroma"][0], blk["has_chroma"][1] = 1, 0                         # both, whatever the draw
    P = dict(tx_size=tx, bsize=bsize, bsize_uv=bsize_uv, modes=modes, deltas=deltas, uv_modes=uv_modes, uv_deltas=uv_deltas, use_angle_delta=uad,
             nfl=nfl, slice_is_intra=intra, ac_dequant_q3=q, intrabc_bits=ibc, metric=metric)
    P["lambda"] = lam
    cb = cr = None
    if chroma:
        top = (1 << 14) if metric == SSD else (1 << 10)
        cb, cr = rng.integers(0, top, (nb, C)).astype(np.uint64), rng.integers(0, top, (nb, C)).astype(np.uint64)
        cb[nb // 2], cr[nb // 2] = 0, 0                                            # a block without chroma samples
    return P, dist, cb, cr, blk, make_rates(rkind, rng), mi


PARAM_KEYS = ("tx_size", "bsize", "bsize_uv", "use_angle_delta", "nfl", "slice_is_intra", "lambda", "ac_dequant_q3", "intrabc_bits", "metric")


def case_of(z, ci):
    """(P, dist, dist_cb, dist_cr, blk, rates, expected outputs) of fixture case ci"""
    p = f"c{ci}_"
    P = {k: int(v) for k, v in zip(PARAM_KEYS, z[p + "params"])}
    for k in ("modes", "deltas", "uv_modes", "uv_deltas"):
        P[k] = z[p + k]
    cb, cr = (z[p + "dist_cb"], z[p + "dist_cr"]) if p + "dist_cb" in z.files else (None, None)
    return P, z[p + "dist"], cb, cr, z[p + "blk"].view(BLK_DTYPE).reshape(-1), z[p + "rates"], {k: z[p + k] for k in OUTPUTS}


def generate(fn):
    fl = np.load(FAST_LOOP)
    out = {"names": np.array(CASE_NAMES)}
    for ci in range(NCASES):
        P, dist, cb, cr, blk, rates, mi = make_case(ci, fl)
        p = f"c{ci}_"
        out[p + "params"] = np.array([P[k] for k in PARAM_KEYS], np.int64)
        for k in ("modes", "deltas", "uv_modes", "uv_deltas"):
            out[p + k] = P[k]
        out[p + "dist"], out[p + "blk"], out[p + "rates"], out[p + "mi"] = dist, blk.view(np.uint8).reshape(-1, 8), rates, mi.astype(np.int32)
        if cb is not None:
            out[p + "dist_cb"], out[p + "dist_cr"] = cb, cr
        for k, v in fn(P, dist, cb, cr, blk, rates).items():
            out[p + k] = v
    return out


def check_conditions(z):
    """what the tests rely on the fixture to contain"""
    ties = quirk = unsorted_ = no_scratch = both_chroma = 0
    for ci in range(NCASES):
        P, dist, cb, cr, blk, rates, want = case_of(z, ci)
        n = want["cand"].shape[1]
        assert int(want["all_cost"].max()) < MAX_CU_COST
        ties += int(any(len(set(row.tolist())) < len(row) for row in want["all_cost"]))
        quirk += int((want["ref_fast_cost"] != np.minimum(want["cost"].min(axis=1), np.uint64(MAX_MODE_COST))).any())
        unsorted_ += int((want["sorted"] != np.arange(n)[None, :]).any())
        no_scratch += int(dist.shape[1] <= P["nfl"])
        both_chroma += int(len(set(blk["has_chroma"].tolist())) == 2)
    assert ties > 3 and quirk > 0 and unsorted_ > 3 and no_scratch > 2 and both_chroma > 10, (ties, quirk, unsorted_, no_scratch, both_chroma)


def check_is_chroma_reference(L=None):
    """np_is_chroma_reference against the reference's own function; False where libsvtref.so is not built"""
    L = L or plain_ref_lib()
    if L is None:
        return False
    for bsize in range(22):
        for r in range(4):
            for c in range(4):
                for sx in (0, 1):
                    for sy in (0, 1):
                        assert L.is_chroma_reference(r, c, bsize, sx, sy) == np_is_chroma_reference(r, c, bsize, sx, sy), (bsize, r, c, sx, sy)
    return True


def model_rd_edges():
    """(sse, n_log2 as a block size, quantizer) at the model's edges: sse 0 and 1, the MAX_XSQ_Q10 clamp from both sides, every xq bucket
    edge from both sides, quantisers 8 and 1336, n_log2 4 (BLOCK_4X4) and 14 (BLOCK_128X128)"""
    out = []
    for bsize in (0, 15):
        n_log2 = NUM_PELS_LOG2[bsize]
        for q in (8, 1336):
            num = ((q >> 3) ** 2) << (n_log2 + 10)
            sses = {0, 1, 2, 3}
            for xsq in list(XSQ_IQ_Q10) + [MAX_XSQ_Q10, MAX_XSQ_Q10 + 1]:
                for t in (xsq - 1, xsq, xsq + 1):
                    if t > 0:
                        sse = num // t                           # xsq = (num + sse / 2) / sse is t or next to it
                        sses.update(v for v in (sse - 1, sse, sse + 1) if v >= 0)
            out += [(v, bsize, q) for v in sorted(sses)]
    return out


def check_model_rd_edges(L=None):
    """ref_model_rd and np_model_rd on model_rd_edges(), against each other and, where L is given, against model_rd_from_sse itself
    -> the xq buckets reached"""
    seen = set()
    for sse, bsize, q in model_rd_edges():
        want = ref_model_rd(sse, NUM_PELS_LOG2[bsize], q)
        if L is not None:
            assert lib_model_rd(L, sse, bsize, q) == want, (sse, bsize, q)
        r, d = np_model_rd(np.array([sse], np.uint64), NUM_PELS_LOG2[bsize], q)
        assert (int(r[0]), int(d[0])) == want, (sse, bsize, q)
        if sse:
            xsq = min(((((q >> 3) ** 2) << (NUM_PELS_LOG2[bsize] + 10)) + (sse >> 1)) // sse, MAX_XSQ_Q10)
            seen.add(ref_model_rd_norm(xsq)[2])
    return seen


def main():
    L = ref_lib()
    z = generate(ref_fast_pick)
    v = generate(np_fast_pick)
    assert sorted(z) == sorted(v)
    for k in z:
        assert z[k].dtype == v[k].dtype and np.array_equal(z[k], v[k]), k
    np.savez_compressed(OUT, **z)
    z = np.load(OUT)
    check_conditions(z)
    pinned = "the reference is absent: restatements only"
    if L is not None:
        check_is_chroma_reference(L)
        for ci in range(NCASES):
            check_case_against_reference(L, z, ci)
        buckets = check_model_rd_edges(L)
        pinned = f"all {NCASES} cases equal av1_intra_fast_cost, model_rd_from_sse ({len(buckets)} xq buckets at the edges) and sort_fast_loop_candidates"
    print(f"wrote {OUT}: {NCASES} cases, {os.path.getsize(OUT)} bytes; {pinned}")


if __name__ == "__main__":
    main()

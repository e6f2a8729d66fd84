"""Writes tests/golden/inter_fast.npz: the end of the fast loop for the combined candidate list of a P / B picture (ninter inter candidates,
then nintra intra candidates), what svt_hip_inter_fast_pick_frame and svt_hip_inter_fast_search_frame must reproduce.

What is pinned to what.  The LEAVES are the reference's own compiled functions in oracle/_ref/libsvtref.so, each exported with a plain C
signature (nm -D lists av1_mv_bit_cost, av1_set_ref_frame, av1_drl_ctx, ref_md_model_rd_from_sse, ref_md_sort) and called through ctypes:
  MV rate          av1_mv_bit_cost (EbRateDistortionCost.c:91-95), mvcost[2] two pointers into the middle of the table, on every
                   (mv, pred mv) pair a fixture candidate costs;
  rf[]             av1_set_ref_frame (EbAdaptiveMotionVectorPrediction.c:247-258) for all 28 ref_frame_type values, recorded as
                   "ref_frame_map" (the device table is checked against the record);
  drl_ctx bytes    av1_drl_ctx (:43-59) on generated CandidateMv weights around REF_CAT_LEVEL;
  SSD model        ref_md_model_rd_from_sse on every (sse, bsize) used;
  order            ref_md_sort on the walk's final buffer costs, for lists of one type only: there the inter-before-intra pass is idle
                   and the export (which marks every buffer INTRA_MODE) is valid;
  predictions      make_golden_inter_pred's ref_lib / ref_inter_pred, whose own pinning is stated there.
The GLUE is this file's own, in Python integers, each function next to the reference lines it mirrors: EstimateRefFramesNumBits,
Av1ModeContextAnalyzer, the body of av1_inter_fast_cost, the walk, and the swap pass on mixed lists.  The walk's logic is pinned to
perform_fast_loop run whole for all-intra lists (tests/golden/fast_search_ref.npz, through make_golden_fast_pick.ref_walk_buffers): this
file asserts its own walk equal to that restatement on every block.  av1_inter_fast_cost is not pinned as a whole function: that would
need new C glue under oracle/.

The rate tables are synthetic (seeded, positive, below 2^20): the cost is lookup arithmetic, so synthetic tables exercise all of it.  No
existing fixture carries any of the fifteen tables with real magnitudes (fast_pick.npz and fast_search_ref.npz hold synthetic tables
themselves), so the second rate set is synthetic too, at the magnitude of real bit costs (below 2^12).  The MV cost table is regenerated from its seed (make_mv_cost), its CRC recorded; the pictures are
make_golden_inter_pred.make_planes', their CRC recorded.

Domain.  Inputs are chosen so that no cost reaches MAX_CU_COST and every MV difference lies within +-16383; both are asserted and the
counts recorded ("domain").  "coverage" records that every case of the issue's list occurs; check_coverage asserts it.

CPU only; run from the repository root after build():  python tests/golden/make_golden_inter_fast.py
"""
import ctypes
import os
import sys
import zlib

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import make_golden_fast_pick as FP  # noqa: E402
import make_golden_inter_pred as IP  # noqa: E402

OUT = os.path.join(HERE, "inter_fast.npz")
U32, U64 = 0xFFFFFFFF, 0xFFFFFFFFFFFFFFFF
MAX_CU_COST, MAX_MODE_COST = FP.MAX_CU_COST, FP.MAX_MODE_COST
SAD, SSD = 0, 1
MV_MAX, MV_VALS = 16383, 32767                 # EbCabacContextModel.h:881-882
MV_COST_WEIGHT = 108                           # EbRateDistortionCost.c:26
REF_CAT_LEVEL = 640                            # EbDefinitions.h:1003
NEARESTMV, NEARMV, GLOBALMV, NEWMV, NEAREST_NEARESTMV, NEAR_NEARMV, NEAREST_NEWMV, NEW_NEARESTMV, NEAR_NEWMV, NEW_NEARMV, GLOBAL_GLOBALMV, \
    NEW_NEWMV = range(13, 25)                  # EbDefinitions.h:878-890
LAST, LAST2, LAST3, GOLDEN, BWDREF, ALTREF2, ALTREF = range(1, 8)
# ref_frame_map (EbAdaptiveMotionVectorPrediction.c:214-233), ref_frame_type 8 .. 28
REF_FRAME_MAP = ((1, 5), (2, 5), (3, 5), (4, 5), (1, 6), (2, 6), (3, 6), (4, 6), (1, 7), (2, 7), (3, 7), (4, 7), (1, 2), (1, 3), (1, 4), (5, 7),
                 (2, 3), (2, 4), (3, 4), (5, 6), (6, 7))
COMPOUND_MODE_CTX_MAP_2 = ((0, 1, 1, 1, 1), (1, 2, 3, 4, 4), (4, 4, 5, 6, 7))      # EbRateDistortionCost.c:951-955
NUM_PELS_LOG2 = (4, 5, 5, 6, 7, 7, 8, 9, 9, 10, 11, 11, 12, 13, 13, 14, 6, 6, 8, 8, 10, 10)
BSIZE_WH = ((4, 4), (4, 8), (8, 4), (8, 8), (8, 16), (16, 8), (16, 16), (16, 32), (32, 16), (32, 32), (32, 64), (64, 32), (64, 64), (64, 128),
            (128, 64), (128, 128), (4, 16), (16, 4), (8, 32), (32, 8), (16, 64), (64, 16))
RATE_TABLES = (("skipModeFacBits", (3, 3)), ("newMvModeFacBits", (6, 3)), ("zeroMvModeFacBits", (2, 3)), ("refMvModeFacBits", (6, 3)),
               ("drlModeFacBits", (3, 3)), ("interCompoundModeFacBits", (8, 9)), ("singleRefFacBits", (3, 6, 3)), ("compRefTypeFacBits", (5, 3)),
               ("compRefFacBits", (3, 3, 3)), ("compBwdRefFacBits", (3, 2, 3)), ("compInterFacBits", (5, 3)), ("motionModeFacBits", (22, 3)),
               ("motionModeFacBits1", (22, 2)), ("intraInterFacBits", (4, 2)), ("nmv_vec_cost", (4,)))      # svt_hip_inter_fast_rates
RATE_WORDS = sum(int(np.prod(s)) for _, s in RATE_TABLES)
BLK_DTYPE = IP.BLK_DTYPE
CAND_DTYPE = np.dtype([("pred_mv", "<i2", (2, 2)), ("mode_ctx", "<i2"), ("pred_mode", "u1"), ("ref_frame_type", "u1"), ("drl_index", "u1"),
                       ("ref_mv_count", "u1"), ("drl_ctx", "u1"), ("flags", "u1")])                        # svt_hip_inter_cand
CTX_FIELDS = ("skip_flag_context", "is_inter_ctx", "reference_mode_context", "compoud_reference_type_context", "comp_ref_p", "comp_ref_p1",
              "comp_ref_p2", "comp_bwdref_p", "comp_bwdref_p1")
CTX_DTYPE = np.dtype([(f, "u1") for f in CTX_FIELDS] + [("single_ref_p", "u1", (6,)), ("has_uv", "u1")])      # svt_hip_inter_fast_blk
assert CAND_DTYPE.itemsize == 16 and CTX_DTYPE.itemsize == 16 and RATE_WORDS == 383
NB = 37                                        # blocks of a pick group: tests run its first 1, 5 and all 37
MV_COST_SEED = 0x3A7C
PICK_KEYS = ("ninter", "nintra", "nfl", "bsize", "bsize_uv", "metric", "lambda", "ac_dequant_q3", "reference_mode_select",
             "switchable_motion_mode", "chroma", "intra_rate", "rate_set")
#             ninter nintra nfl bsize uv metric lambda     q3   rms smm chroma irate set
PICK_GROUPS = ((1, 0, 1, 3, 0, SAD, 29041, 0, 1, 1, 1, 0, 0),
               (2, 0, 1, 6, 3, SSD, 6544, 312, 1, 0, 1, 0, 1),
               (3, 0, 3, 0, 0, SAD, 1, 0, 1, 1, 0, 0, 0),             # 4x4: min(bw, bh) < 8 under reference_mode_select
               (4, 0, 3, 9, 6, SSD, 29041, 1336, 0, 1, 1, 0, 1),
               (13, 0, 12, 19, 17, SAD, 0xFFFFF, 0, 1, 1, 1, 0, 0),
               (64, 0, 40, 12, 9, SAD, 29041, 0, 1, 1, 1, 0, 1),
               (5, 3, 3, 6, 3, SAD, 29041, 0, 0, 0, 1, 1, 0),
               (5, 3, 12, 3, 0, SSD, 6544, 80, 1, 1, 0, 1, 1),
               (40, 24, 40, 9, 6, SSD, 29041, 640, 1, 1, 1, 1, 0),
               (1, 63, 2, 6, 3, SAD, 4000, 0, 1, 1, 1, 0, 1),
               (6, 6, 5, 3, 0, SAD, 29041, 0, 1, 1, 1, 1, 1),         # intra costs around the inter ones: mixed survivors
               (3, 9, 4, 1, 0, SAD, 29041, 0, 0, 0, 0, 0, 0))         # 4x8; intra costs far below: survivors all intra
SEARCH_KEYS = ("bwidth", "bheight", "bd", "metric", "chroma", "nblocks") + PICK_KEYS[:5] + PICK_KEYS[6:10] + ("rate_set",)
#               bw  bh  bd metric chroma nblk ninter nintra nfl bsize uv lambda q3 rms smm set
SEARCH_GROUPS = ((8, 8, 8, SAD, 1, 6, 6, 2, 3, 3, 0, 29041, 0, 1, 1, 0),
                 (16, 16, 8, SSD, 1, 5, 5, 3, 3, 6, 3, 6544, 312, 1, 0, 1),
                 (32, 8, 8, SAD, 0, 5, 4, 0, 3, 19, 17, 29041, 0, 0, 1, 0),
                 (64, 64, 8, SSD, 0, 2, 3, 2, 2, 12, 9, 6544, 640, 1, 1, 1),
                 (16, 16, 10, SAD, 1, 5, 4, 2, 3, 6, 3, 29041, 0, 1, 1, 0))


def make_mv_cost(seed=MV_COST_SEED):
    """int32 [2][MV_VALS], positive, below 2^20"""
    return np.random.default_rng([0x3F, seed]).integers(1, 1 << 20, (2, MV_VALS)).astype(np.int32)


def make_rates(k):
    """rate set k: 0 below 2^20, 1 below 2^12 (the magnitude of real bit costs, 512 a bit)"""
    rng = np.random.default_rng([0x1F7, k])
    top = 1 << 20 if k == 0 else 1 << 12
    return {name: rng.integers(1, top, shape).astype(np.int32) for name, shape in RATE_TABLES}


def pack_rates(R):
    return np.concatenate([np.asarray(R[name], np.int32).reshape(-1) for name, _ in RATE_TABLES])


def unpack_rates(words):
    R, at = {}, 0
    for name, shape in RATE_TABLES:
        n = int(np.prod(shape))
        R[name] = np.asarray(words[at:at + n], np.int32).reshape(shape)
        at += n
    return R


# ---- the glue: the reference's lines in Python integers ---------------------------------------------------------------------------------
def set_ref_frame(t):
    """av1_set_ref_frame :247-258 -> (rf[0], rf[1]); NONE_FRAME = -1"""
    return REF_FRAME_MAP[t - 8] if t >= 8 else (t, -1)


def est_ref_bits(P, R, ctx, rft, is_compound):
    """EstimateRefFramesNumBits, EbRateDistortionCost.c:741-947"""
    bits = 0
    bw, bh = BSIZE_WH[P["bsize"]]
    if P["reference_mode_select"] and min(bw, bh) >= 8:                                               # :781-782
        bits += int(R["compInterFacBits"][ctx["reference_mode_context"]][is_compound])                # :786
    if is_compound:
        rf = set_ref_frame(rft)                                                                       # :799
        bits += int(R["compRefTypeFacBits"][ctx["compoud_reference_type_context"]][1])                # :804 BIDIR_COMP_REFERENCE
        bit = int(rf[0] == GOLDEN or rf[0] == LAST3)                                                  # :830
        bits += int(R["compRefFacBits"][ctx["comp_ref_p"]][0][bit])                                   # :835
        if not bit:
            bits += int(R["compRefFacBits"][ctx["comp_ref_p1"]][1][int(rf[0] == LAST2)])              # :844
        else:
            bits += int(R["compRefFacBits"][ctx["comp_ref_p2"]][2][int(rf[0] == GOLDEN)])             # :854
        bit_bwd = int(rf[1] == ALTREF)                                                                # :859
        bits += int(R["compBwdRefFacBits"][ctx["comp_bwdref_p"]][0][bit_bwd])                         # :864
        if not bit_bwd:
            bits += int(R["compBwdRefFacBits"][ctx["comp_bwdref_p1"]][1][int(rf[1] == ALTREF2)])      # :873
    else:
        p = ctx["single_ref_p"]
        bit0 = int(BWDREF <= rft <= ALTREF)                                                           # :880
        bits += int(R["singleRefFacBits"][p[0]][0][bit0])                                             # :887
        if bit0:
            bit1 = int(rft == ALTREF)
            bits += int(R["singleRefFacBits"][p[1]][1][bit1])                                         # :897
            if not bit1:
                bits += int(R["singleRefFacBits"][p[5]][5][int(rft == ALTREF2)])                      # :906
        else:
            bit2 = int(rft == LAST3 or rft == GOLDEN)
            bits += int(R["singleRefFacBits"][p[2]][2][bit2])                                         # :918
            if not bit2:
                bits += int(R["singleRefFacBits"][p[3]][3][int(rft != LAST)])                         # :927
            else:
                bits += int(R["singleRefFacBits"][p[4]][4][int(rft != LAST3)])                        # :937
    return bits


def mode_context_analyzer(mode_ctx, rf):
    """Av1ModeContextAnalyzer :956-969; the result as the uint32 it is assigned to (:1021)"""
    if rf[1] <= 0:                                                                                    # :960
        return mode_ctx & U32
    newmv_ctx, refmv_ctx = mode_ctx & 7, (mode_ctx >> 4) & 15                                         # :962-964
    return COMPOUND_MODE_CTX_MAP_2[refmv_ctx >> 1][min(newmv_ctx, 4)]                                 # :966


def mv_bit_cost(mv_cost, joint_cost, mv, ref):
    """av1_mv_bit_cost :91-95 (mv_cost :80-89, av1_get_mv_joint :72-79); mv / ref as (row, col)"""
    row, col = mv[0] - ref[0], mv[1] - ref[1]
    assert abs(row) <= MV_MAX and abs(col) <= MV_MAX
    joint = (2 if row else 0) | (1 if col else 0)
    c = int(joint_cost[joint]) + int(mv_cost[0][MV_MAX + row]) + int(mv_cost[1][MV_MAX + col])
    return (c * MV_COST_WEIGHT + 64) >> 7


def inter_fast_cost(P, R, mv_cost, ctx, b, c, luma, chroma, mv_pairs=None, merge_seen=None):
    """av1_inter_fast_cost :971-1318 -> (cost, fast_luma_rate, fast_chroma_rate); b / c the candidate's two records"""
    mode, rft = int(c["pred_mode"]), int(c["ref_frame_type"])
    is_compound = int(b["pred_direction"]) == 2
    rf = set_ref_frame(rft)                                                                           # :1020
    mode_ctx = mode_context_analyzer(int(c["mode_ctx"]), rf)                                          # :1021
    skip_rate = int(R["skipModeFacBits"][ctx["skip_flag_context"]][0])                                # :1022
    ref_bits = est_ref_bits(P, R, ctx, rft, int(is_compound))                                         # :1027
    bits = 0
    if is_compound:
        bits += int(R["interCompoundModeFacBits"][mode_ctx][mode - NEAREST_NEARESTMV])                # :1038
    else:
        bits += int(R["newMvModeFacBits"][mode_ctx & 7][int(mode != NEWMV)])                          # :1044-1046
        if mode != NEWMV:
            bits += int(R["zeroMvModeFacBits"][(mode_ctx >> 3) & 1][int(mode != GLOBALMV)])           # :1048-1050
            if mode != GLOBALMV:
                bits += int(R["refMvModeFacBits"][(mode_ctx >> 4) & 15][int(mode != NEARESTMV)])      # :1052-1054
    near = mode in (NEARMV, NEAR_NEARMV, NEAR_NEWMV, NEW_NEARMV)
    count, drl_index = int(c["ref_mv_count"]), int(c["drl_index"])
    drl = lambda idx: (int(c["drl_ctx"]) >> (2 * idx)) & 3
    if mode == NEWMV or mode == NEW_NEWMV or near:                                                    # :1058
        if mode == NEWMV or mode == NEW_NEWMV:
            for idx in range(2):                                                                      # :1064-1071
                if count > idx + 1:
                    bits += int(R["drlModeFacBits"][drl(idx)][int(drl_index != idx)])
                    if drl_index == idx:
                        break
        if near:
            for idx in range(1, 3):                                                                   # :1077-1085
                if count > idx + 1:
                    bits += int(R["drlModeFacBits"][drl(idx)][int(drl_index != idx - 1)])
                    if drl_index == idx - 1:
                        break
    mv_rate = 0
    if mode in (NEWMV, NEW_NEWMV, NEAREST_NEWMV, NEW_NEARESTMV, NEAR_NEWMV, NEW_NEARMV):              # :1090
        if is_compound:
            lists = (0, 1) if mode == NEW_NEWMV else ((1,) if mode in (NEAREST_NEWMV, NEAR_NEWMV) else (0,))      # :1095, :1123, :1147
        else:
            lists = (0,) if int(b["pred_direction"]) == 0 else (1,)                                   # :1175
        for l in lists:
            mv, ref = (int(b["mv"][l][1]), int(b["mv"][l][0])), (int(c["pred_mv"][l][1]), int(c["pred_mv"][l][0]))
            if mv_pairs is not None:
                mv_pairs.add((mv, ref))
            mv_rate += mv_bit_cost(mv_cost, R["nmv_vec_cost"], mv, ref)
    flags = int(c["flags"])
    if mode < NEAREST_NEARESTMV and P["switchable_motion_mode"] and rf[1] != 0:                       # :1203-1206
        allowed, mm = (flags >> 3) & 3, (flags >> 1) & 3
        if allowed == 1:                                                                              # :1222-1225
            bits += int(R["motionModeFacBits1"][P["bsize"]][mm])
        elif allowed != 0:                                                                            # :1226-1227
            bits += int(R["motionModeFacBits"][P["bsize"]][mm])
    is_inter_rate = int(R["intraInterFacBits"][ctx["is_inter_ctx"]][1])                               # :1250
    luma_rate = (ref_bits + skip_rate + bits + mv_rate + is_inter_rate) & U32                         # :1251, uint32_t
    fast_luma_rate, chroma_rate = luma_rate, 0                                                        # :1257-1258
    if P["metric"] == SSD:                                                                            # :1260-1294
        r, total = FP.ref_model_rd(luma, NUM_PELS_LOG2[P["bsize"]], P["ac_dequant_q3"])
        luma_rate = (luma_rate + r) & U32                                                             # :1273
        chroma_rate, cd = FP.ref_model_rd(chroma, NUM_PELS_LOG2[P["bsize_uv"]], P["ac_dequant_q3"])   # :1277-1283
        total = (total + cd) & U64
    else:
        total = (luma + chroma) & U64                                                                 # :1298-1300
    rate = (luma_rate + chroma_rate) & U32                                                            # :1286 / :1306
    if flags & 1:                                                                                     # merge_flag :1288 / :1310
        skip1 = int(R["skipModeFacBits"][ctx["skip_flag_context"]][1])
        if merge_seen is not None:
            merge_seen.add("below" if skip1 < rate else ("equal" if skip1 == rate else "above"))
        if skip1 < rate:
            rate = skip1
    cost = ((((rate * P["lambda"] + 256) & U64) >> 9) + ((total * 128) & U64)) & U64                  # RDCOST
    return cost, fast_luma_rate, 0


def walk(costs, nfl):
    """the second loop of perform_fast_loop (EbProductCodingLoop.c:1225-1363) -> fast_cost[nbuf], cand_of[nbuf], n"""
    ncand = len(costs)
    n = min(ncand, nfl)
    scratch = ncand > n
    nbuf = n + 1 if scratch else n
    fast_cost, cand_of = [MAX_CU_COST] * nbuf, [0] * nbuf
    hi = 0                                                                                            # :1225
    for idx in range(ncand - 1, -1, -1):                                                              # :1226-1227, :1357
        fast_cost[hi], cand_of[hi] = costs[idx], idx                                                  # :1229-1230, :1313
        if idx or scratch:                                                                            # :1331
            hi = 0                                                                                    # :1344
            for bi in range(1, max(nbuf, 2)):                                                         # :1345-1355 (a do-while: one pass at least)
                if fast_cost[hi] == MAX_CU_COST:                                                      # :1349
                    break
                if bi < nbuf and fast_cost[bi] > fast_cost[hi]:                                       # :1352
                    hi = bi
    if scratch:
        fast_cost[hi] = MAX_CU_COST                                                                   # :1361
    return fast_cost, cand_of, n


def sort_mixed(fast_cost, is_intra, n):
    """sort_fast_loop_candidates (EbModeDecision.c:436-489) with is_intra[b] the type of buffer b's candidate -> best, sorted, ref_fast_cost,
    whether the :458-469 pass moved anything"""
    nbuf = len(fast_cost)
    best = [0] * nbuf
    start, end = 0, nbuf - 1
    for b in range(nbuf):                                                                             # :449-456
        if fast_cost[b] == MAX_CU_COST:
            best[end] = b
            end -= 1
        else:
            best[start] = b
            start += 1
    before = list(best)
    for i in range(n - 1):                                                                            # :460-469
        for j in range(i + 1, n):
            if is_intra[best[i]] and not is_intra[best[j]]:
                best[i], best[j] = best[j], best[i]
    ref_fast_cost = MAX_MODE_COST
    for i in range(n):                                                                                # :472-476
        if fast_cost[i] < ref_fast_cost:
            ref_fast_cost = fast_cost[i]
    srt = list(best[:n])                                                                              # :477-479
    for i in range(n - 1):                                                                            # :480-488
        for j in range(i + 1, n):
            if fast_cost[j] < fast_cost[i]:
                srt[i], srt[j] = srt[j], srt[i]
    return best, srt, ref_fast_cost, best != before


def pick_block(costs, ninter, nfl, L=None, stats=None):
    """walk and order of one block's combined costs -> cand[n], sorted as slots [n], ref_fast_cost"""
    fast_cost, cand_of, n = walk(costs, nfl)
    assert (fast_cost, cand_of, n) == FP.ref_walk_buffers(costs, nfl), "the walk against the restatement fast_search_ref.npz pins"
    is_intra = [cand_of[b] >= ninter for b in range(len(fast_cost))]
    best, srt, ref_fast_cost, fired = sort_mixed(fast_cost, is_intra, n)
    held = [is_intra[b] for b in best[:n]]
    one_type = all(held) or not any(held)
    if one_type:
        assert (best, srt, ref_fast_cost) == FP.ref_sort(fast_cost, n) and not fired
        if L is not None:
            assert (best, srt, ref_fast_cost) == FP.lib_sort(L, fast_cost, n), "ref_md_sort"
            if stats is not None:
                stats["lib_sort"] += 1
    cand, slots = FP.slots_of(best, srt, cand_of, n)
    if stats is not None:
        stats["swap_fired"] += int(fired)
        stats["swap_idle"] += int(not fired)
        stats["all_intra"] += int(all(held))
        kinds = [c >= ninter for c in cand]
        pre = [cand_of[b] >= ninter for b in sorted(range(len(fast_cost)), key=lambda b: (fast_cost[b] == MAX_CU_COST, b))[:n]]      # before the pass
        stats["pre_intra_inter_intra"] += int(any(pre[i] and not pre[j] and pre[k] for i in range(n) for j in range(i + 1, n) for k in range(j + 1, n)))
        assert kinds == sorted(kinds)                                                                # inter entries first
    return cand, slots, ref_fast_cost


def pick_group(P, R, mv_cost, blk, cand_in, ctx, dist, dist_cb, dist_cr, intra_cost, intra_rate, L=None, stats=None, mv_pairs=None, sse_used=None,
               merge_seen=None):
    """every output of svt_hip_inter_fast_pick_frame for one group -> dict"""
    nb, ni, na = len(ctx), P["ninter"], P["nintra"]
    n = min(P["nfl"], ni + na)
    out = dict(cand=np.zeros((nb, n), np.uint8), sorted=np.zeros((nb, n), np.uint8), cost=np.zeros((nb, n), np.uint64),
               rate=np.zeros((nb, n, 2), np.uint32), ref_fast_cost=np.zeros(nb, np.uint64), all_cost=np.zeros((nb, ni), np.uint64),
               blk_out=np.zeros((nb, n), BLK_DTYPE), cand_out=np.zeros((nb, n), CAND_DTYPE), src_xy_out=np.zeros((nb, n), np.uint32))
    for i in range(nb):
        costs, rates = [], []
        for k in range(ni):
            luma = int(dist[i, k])
            chroma = (int(dist_cb[i, k]) if dist_cb is not None else 0) + (int(dist_cr[i, k]) if dist_cr is not None else 0)
            if sse_used is not None and P["metric"] == SSD:
                sse_used.add((luma, P["bsize"], P["ac_dequant_q3"]))
                sse_used.add((chroma, P["bsize_uv"], P["ac_dequant_q3"]))
            c, lr, cr = inter_fast_cost(P, R, mv_cost, ctx[i], blk[i, k], cand_in[i, k], luma, chroma, mv_pairs, merge_seen)
            costs.append(c)
            rates.append((lr, cr))
            out["all_cost"][i, k] = c
        for k in range(na):
            costs.append(int(intra_cost[i, k]))
            rates.append((int(intra_rate[i, k, 0]), int(intra_rate[i, k, 1])) if intra_rate is not None else (0, 0))
        assert max(costs) < MAX_CU_COST
        cand, slots, ref = pick_block(costs, ni, P["nfl"], L, stats)
        out["cand"][i], out["sorted"][i], out["ref_fast_cost"][i] = cand, slots, ref
        xy = int(blk[i, 0]["x"]) | int(blk[i, 0]["y"]) << 16
        for s, c in enumerate(cand):
            out["cost"][i, s], out["rate"][i, s] = costs[c], rates[c]
            out["src_xy_out"][i, s] = xy
            if c < ni:
                out["blk_out"][i, s], out["cand_out"][i, s] = blk[i, c], cand_in[i, c]
            else:
                out["blk_out"][i, s]["x"], out["blk_out"][i, s]["y"] = blk[i, 0]["x"], blk[i, 0]["y"]
    return out


# ---- the cases ---------------------------------------------------------------------------------------------------------------------------
def drl_ctx_of(w0, w1):
    """av1_drl_ctx :43-59 on two weights"""
    if w0 >= REF_CAT_LEVEL and w1 >= REF_CAT_LEVEL:
        return 0
    if w0 >= REF_CAT_LEVEL and w1 < REF_CAT_LEVEL:
        return 1
    if w0 < REF_CAT_LEVEL and w1 < REF_CAT_LEVEL:
        return 2
    return 0


def make_candidates(rng, nb, ni, xy, weights_out=None, search=False):
    """[nb, ni] records of both kinds.  xy: [nb] (x, y) origins.  search: vectors a prediction can follow (a few samples, any phase)"""
    blk, cand = np.zeros((nb, ni), BLK_DTYPE), np.zeros((nb, ni), CAND_DTYPE)
    for i in range(nb):
        for k in range(ni):
            b, c = blk[i, k], cand[i, k]
            b["x"], b["y"] = xy[i]
            mode = int(rng.integers(NEARESTMV, NEW_NEWMV + 1)) if (i * ni + k) >= 12 else NEARESTMV + (i * ni + k) % 12
            c["pred_mode"] = mode
            if mode >= NEAREST_NEARESTMV:
                b["pred_direction"], c["ref_frame_type"] = 2, int(rng.integers(8, 29)) if rng.integers(0, 4) == 0 else int(rng.integers(8, 20))
            else:
                b["pred_direction"], c["ref_frame_type"] = int(rng.integers(0, 2)), int(rng.integers(1, 8))
            span = 40 if search else 8191
            kind = int(rng.integers(0, 8))
            for l in range(2):
                for d in range(2):
                    mv = int(rng.integers(-span, span + 1))
                    pm = mv if kind == 0 or (kind == 1 and d == 0) or (kind == 2 and d == 1) else int(rng.integers(-span, span + 1))
                    if not search and kind == 3:
                        mv, pm = (8191, -8192) if d == 0 else (-8192, 8191)                         # the ends of the table: +-16383
                    b["mv"][l][d], c["pred_mv"][l][d] = mv, pm
            b["filter_x"], b["filter_y"] = int(rng.integers(0, 3)), int(rng.integers(0, 3))
            c["mode_ctx"] = int(rng.integers(0, 6)) | int(rng.integers(0, 2)) << 3 | int(rng.integers(0, 6)) << 4
            c["drl_index"], c["ref_mv_count"] = int(rng.integers(0, 3)), int(rng.integers(0, 5))
            w = [int(REF_CAT_LEVEL + rng.integers(-2, 2)) for _ in range(4)]
            c["drl_ctx"] = sum(drl_ctx_of(w[idx], w[idx + 1]) << (2 * idx) for idx in range(3))
            if weights_out is not None:
                weights_out.append((w, int(c["drl_ctx"])))
            allowed = int(rng.integers(0, 3))
            c["flags"] = int(rng.integers(0, 3) == 0) | int(rng.integers(0, allowed + 1)) << 1 | allowed << 3
    return blk, cand


def make_ctx(rng, nb):
    ctx = np.zeros(nb, CTX_DTYPE)
    ctx["skip_flag_context"], ctx["is_inter_ctx"] = rng.integers(0, 3, nb), rng.integers(0, 4, nb)
    ctx["reference_mode_context"], ctx["compoud_reference_type_context"] = rng.integers(0, 5, nb), rng.integers(0, 5, nb)
    for f in CTX_FIELDS[4:]:
        ctx[f] = rng.integers(0, 3, nb)
    ctx["single_ref_p"], ctx["has_uv"] = rng.integers(0, 3, (nb, 6)), rng.integers(0, 2, nb)
    return ctx


def params_of(keys, row):
    return {k: int(v) for k, v in zip(keys, row)}


def make_pick_case(gi, rate_sets, mv_cost, weights=None):
    P = params_of(PICK_KEYS, PICK_GROUPS[gi])
    rng = np.random.default_rng([0x1F5, gi])
    ni, na = P["ninter"], P["nintra"]
    R = rate_sets[P["rate_set"]].copy()
    top = 64 * 64 * 255 if P["metric"] == SAD else 1 << 24
    xy = [(int(rng.integers(0, 20)) * 4, int(rng.integers(0, 12)) * 4) for _ in range(NB)]
    blk, cand = make_candidates(rng, NB, ni, xy, weights)
    ctx = make_ctx(rng, NB)
    dist = rng.integers(0, top, (NB, ni)).astype(np.int64)
    dist[0, 0] = 0                                                                                    # the SSD model's sse == 0 exit
    dist_cb = rng.integers(0, top // 4, (NB, ni)).astype(np.int64) if P["chroma"] else None
    dist_cr = rng.integers(0, top // 4, (NB, ni)).astype(np.int64) if P["chroma"] else None
    for i in range(3, NB, 4):                                                                         # duplicates: equal costs meet > and <
        if ni >= 2:
            s, d = int(rng.integers(0, ni)), int(rng.integers(0, ni))
            blk[i, d], cand[i, d], dist[i, d] = blk[i, s], cand[i, s], dist[i, s]
            if P["chroma"]:
                dist_cb[i, d], dist_cr[i, d] = dist_cb[i, s], dist_cr[i, s]
    return P, R, blk, cand, ctx, dist, dist_cb, dist_cr, rng


def intra_tail(P, rng, inter_costs, gi):
    """intra costs placed against the block's inter costs: around them, or (the last group) far below"""
    nb, na = inter_costs.shape[0], P["nintra"]
    if na == 0:
        return None, None
    lo, hi = inter_costs.min(axis=1).astype(np.float64), inter_costs.max(axis=1).astype(np.float64)
    u = rng.random((nb, na))
    cost = (lo[:, None] * 0.5 + u * (hi[:, None] * 1.2 - lo[:, None] * 0.5 + 1)).astype(np.uint64)
    if gi == len(PICK_GROUPS) - 1:
        cost = (u * lo[:, None] * 0.5).astype(np.uint64)
    for i in range(2, nb, 5):                                                                         # an intra cost equal to an inter one, and two equal intra costs
        cost[i, 0] = inter_costs[i, 0]
        if na >= 2:
            cost[i, na - 1] = cost[i, na // 2]
    rate = rng.integers(0, 1 << 20, (nb, na, 2)).astype(np.uint32) if P["intra_rate"] else None
    return cost, rate


def engineer_merge(P, R, mv_cost, ctx, blk, cand, dist, dist_cb, dist_cr):
    """candidate (0, 0) merges with skipModeFacBits[ctx][1] EQUAL to its rate (that entry enters no rate); (1, 0) and (2, 0) merge too"""
    for i in range(min(3, len(ctx))):
        cand[i, 0]["flags"] |= 1
    P0 = dict(P)
    saved = int(cand[0, 0]["flags"])
    cand[0, 0]["flags"] = saved & ~1
    chroma = (int(dist_cb[0, 0]) if dist_cb is not None else 0) + (int(dist_cr[0, 0]) if dist_cr is not None else 0)
    _, lr, _ = inter_fast_cost(P0, R, mv_cost, ctx[0], blk[0, 0], cand[0, 0], int(dist[0, 0]), chroma)
    rate = lr
    if P["metric"] == SSD:
        r1, _ = FP.ref_model_rd(int(dist[0, 0]), NUM_PELS_LOG2[P["bsize"]], P["ac_dequant_q3"])
        r2, _ = FP.ref_model_rd(chroma, NUM_PELS_LOG2[P["bsize_uv"]], P["ac_dequant_q3"])
        rate = ((lr + r1) & U32) + r2 & U32
    cand[0, 0]["flags"] = saved
    R["skipModeFacBits"] = R["skipModeFacBits"].copy()
    R["skipModeFacBits"][ctx[0]["skip_flag_context"]][1] = rate
    return rate


def search_blocks(S, rng):
    bw, bh, nb = S["bwidth"], S["bheight"], S["nblocks"]
    xs, ys = np.arange(0, IP.W - bw + 1, 8), np.arange(0, IP.H - bh + 1, 8)
    return [(int(xs[(3 * i + 1) % len(xs)]), int(ys[(5 * i + 2) % len(ys)])) for i in range(nb)]


def search_dist(predict, S, blk):
    """[planes][nb, ni] distortions of the candidates' predictions against the source, as svt_hip_inter_pred_frame's fused distortion"""
    planes = IP.planes_of(S["bd"], "random")
    flat = blk.reshape(-1)
    out = []
    for p in range(3 if S["chroma"] else 1):
        ss = 1 if p else 0
        pred = predict(planes, S["bd"], ss, p, S["bwidth"], S["bheight"], flat)
        out.append(IP.np_dist(pred, planes["src"][p], ss, flat, S["metric"]).reshape(blk.shape))
    return out


def generate(predict, L=None):
    """the fixture.  predict(planes, bd, ss, plane, bwidth, bheight, blk) -> [n, h, w]; L: the compiled reference for the leaf pins"""
    z = {}
    stats = dict(swap_fired=0, swap_idle=0, all_intra=0, lib_sort=0, pre_intra_inter_intra=0)
    mv_pairs, sse_used, weights = set(), set(), []
    mv_cost = make_mv_cost()
    z["mv_cost_crc"] = np.array([zlib.crc32(mv_cost.tobytes())], np.uint32)
    rate_sets = [make_rates(0), make_rates(1)]
    z["pick_params"] = np.array(PICK_GROUPS, np.int64)
    z["search_params"] = np.array(SEARCH_GROUPS, np.int64)
    z["ref_frame_map"] = np.array([(0, 0)] + [set_ref_frame(t) for t in range(1, 29)], np.int8)
    z["compound_mode_ctx_map_2"] = np.array(COMPOUND_MODE_CTX_MAP_2, np.int32)
    seen = dict(modes=set(), types=set(), rms_small=set(), drl=set(), drl_new=set(), drl_near=set(), merge=set(), mm=set(), has_uv=set(), metric=set())
    ncost = 0
    for gi in range(len(PICK_GROUPS)):
        P, R, blk, cand, ctx, dist, dcb, dcr, rng = make_pick_case(gi, rate_sets, mv_cost, weights)
        if gi in (0, 3):
            engineer_merge(P, R, mv_cost, ctx, blk, cand, dist, dcb, dcr)
        inter_costs = np.array([[inter_fast_cost(P, R, mv_cost, ctx[i], blk[i, k], cand[i, k], int(dist[i, k]),
                                                 (int(dcb[i, k]) + int(dcr[i, k])) if dcb is not None else 0)[0]
                                 for k in range(P["ninter"])] for i in range(NB)], np.uint64)
        icost, irate = intra_tail(P, rng, inter_costs, gi)
        out = pick_group(P, R, mv_cost, blk, cand, ctx, dist, dcb, dcr, icost, irate, L, stats, mv_pairs, sse_used, seen["merge"])
        ncost += NB * (P["ninter"] + P["nintra"])
        z[f"pick_{gi}_rates"] = pack_rates(R)
        for name, a in (("blk", blk.view(np.uint8).reshape(NB, -1, 16)), ("cand_in", cand.view(np.uint8).reshape(NB, -1, 16)),
                        ("ctx", ctx.view(np.uint8).reshape(NB, 16)), ("dist", dist), ("dist_cb", dcb), ("dist_cr", dcr), ("intra_cost", icost),
                        ("intra_rate", irate)):
            if a is not None:
                z[f"pick_{gi}_{name}"] = a
        for name, a in out.items():
            z[f"pick_{gi}_out_{name}"] = a.view(np.uint8).reshape(a.shape + (16,)) if a.dtype.itemsize == 16 else a
        # coverage
        bw, bh = BSIZE_WH[P["bsize"]]
        seen["rms_small"].add((P["reference_mode_select"], min(bw, bh) < 8))
        seen["metric"].add(P["metric"])
        seen["has_uv"] |= set(ctx["has_uv"].tolist())
        for i in range(NB):
            for k in range(P["ninter"]):
                c = cand[i, k]
                m = int(c["pred_mode"])
                seen["modes"].add(m)
                seen["types"].add(int(c["ref_frame_type"]))
                cnt, di = int(c["ref_mv_count"]), int(c["drl_index"])
                seen["drl"].add((cnt, di))
                if m in (NEWMV, NEW_NEWMV):
                    seen["drl_new"].add("early" if cnt > 1 and di == 0 else ("late" if cnt > 2 and di == 1 else "never"))
                if m in (NEARMV, NEAR_NEARMV, NEAR_NEWMV, NEW_NEARMV):
                    seen["drl_near"].add("early" if cnt > 2 and di == 0 else ("late" if cnt > 3 and di == 1 else "never"))
                if P["switchable_motion_mode"] and m < NEAREST_NEARESTMV:
                    seen["mm"].add((int(c["flags"]) >> 3) & 3)
    # the search groups: real predictions and distortions
    for si in range(len(SEARCH_GROUPS)):
        S = params_of(SEARCH_KEYS, SEARCH_GROUPS[si])
        P = dict(S)
        rng = np.random.default_rng([0x5EA, si])
        nb, ni, na = S["nblocks"], S["ninter"], S["nintra"]
        R = rate_sets[S["rate_set"]]
        blk, cand = make_candidates(rng, nb, ni, search_blocks(S, rng), weights, search=True)
        if ni >= 2:
            blk[1, 1], cand[1, 1] = blk[1, 0], cand[1, 0]                                             # a duplicate: equal distortion, equal cost
        ctx = make_ctx(rng, nb)
        d = search_dist(predict, S, blk)
        dcb, dcr = (d[1], d[2]) if S["chroma"] else (None, None)
        inter_costs = np.array([[inter_fast_cost(P, R, mv_cost, ctx[i], blk[i, k], cand[i, k], int(d[0][i, k]),
                                                 (int(dcb[i, k]) + int(dcr[i, k])) if dcb is not None else 0)[0] for k in range(ni)] for i in range(nb)], np.uint64)
        P["intra_rate"] = 1
        icost, irate = intra_tail(P, rng, inter_costs, -1)
        out = pick_group(P, R, mv_cost, blk, cand, ctx, d[0], dcb, dcr, icost, irate, L, stats, mv_pairs, sse_used)
        ncost += nb * (ni + na)
        for name, a in (("blk", blk.view(np.uint8).reshape(nb, -1, 16)), ("cand_in", cand.view(np.uint8).reshape(nb, -1, 16)),
                        ("ctx", ctx.view(np.uint8).reshape(nb, 16)), ("dist", d[0]), ("dist_cb", dcb), ("dist_cr", dcr), ("intra_cost", icost),
                        ("intra_rate", irate)):
            if a is not None:
                z[f"search_{si}_{name}"] = a
        for name, a in out.items():
            z[f"search_{si}_out_{name}"] = a.view(np.uint8).reshape(a.shape + (16,)) if a.dtype.itemsize == 16 else a
    z["rate_sets"] = np.stack([pack_rates(r) for r in rate_sets])
    z["planes_crc"] = np.array([IP.planes_crc(IP.planes_of(bd, "random")) for bd in (8, 10)], np.uint32)
    # the leaf pins
    pins = dict(mv_pairs=len(mv_pairs), sse=len(sse_used), drl_weights=len(weights), lib=int(L is not None))
    if L is not None:
        check_leaves(L, mv_cost, rate_sets, mv_pairs, sse_used, weights)
    cov = dict(modes=sorted(seen["modes"]), types=sorted(seen["types"]), rms_small=sorted(seen["rms_small"]), drl=sorted(seen["drl"]),
               drl_new=sorted(seen["drl_new"]), drl_near=sorted(seen["drl_near"]), merge=sorted(seen["merge"]), mm=sorted(seen["mm"]),
               has_uv=sorted(seen["has_uv"]), metric=sorted(seen["metric"]))
    check_coverage(cov, stats)
    z["coverage_modes"] = np.array(cov["modes"], np.int32)
    z["coverage_types"] = np.array(cov["types"], np.int32)
    z["coverage_drl"] = np.array(cov["drl"], np.int32)
    z["coverage_walk"] = np.array([stats["swap_fired"], stats["swap_idle"], stats["all_intra"], stats["pre_intra_inter_intra"]], np.int64)
    z["domain"] = np.array([ncost, 0, len(mv_pairs), 0], np.int64)      # costs computed, of them >= MAX_CU_COST; MV pairs, of them outside +-16383
    z["pins"] = np.array([pins["mv_pairs"], pins["sse"], pins["drl_weights"], stats["lib_sort"]], np.int64)
    return z


def check_coverage(cov, stats):
    assert cov["modes"] == list(range(NEARESTMV, NEW_NEWMV + 1)), cov["modes"]
    assert set(range(1, 8)) <= set(cov["types"]) and len([t for t in cov["types"] if t >= 8]) >= 6, cov["types"]
    rf = [set_ref_frame(t) for t in cov["types"] if t >= 8]
    assert {LAST2, LAST3, GOLDEN} <= {r[0] for r in rf} and {BWDREF, ALTREF2, ALTREF} <= {r[1] for r in rf}
    assert set(cov["rms_small"]) >= {(1, True), (1, False), (0, True), (0, False)}, cov["rms_small"]
    assert {(c, d) for c in range(5) for d in range(3)} <= set(map(tuple, cov["drl"]))
    assert set(cov["drl_new"]) == {"early", "late", "never"} and set(cov["drl_near"]) == {"early", "late", "never"}
    assert set(cov["merge"]) == {"below", "equal", "above"}, cov["merge"]
    assert set(cov["mm"]) == {0, 1, 2} and cov["has_uv"] == [0, 1] and cov["metric"] == [SAD, SSD]
    assert stats["swap_fired"] > 0 and stats["swap_idle"] > 0 and stats["all_intra"] > 0 and stats["pre_intra_inter_intra"] > 0, stats


# ---- the compiled leaves ------------------------------------------------------------------------------------------------------------------
class MV(ctypes.Structure):
    _fields_ = [("row", ctypes.c_int16), ("col", ctypes.c_int16)]


class CandidateMv(ctypes.Structure):                           # EbCodingUnit.h:145-149
    _fields_ = [("this_mv", ctypes.c_uint32), ("comp_mv", ctypes.c_uint32), ("weight", ctypes.c_int32)]


def ref_lib():
    """libsvtref.so with the leaves typed, or None where it is not built"""
    L = FP.ref_lib()
    if L is None or not all(hasattr(L, s) for s in ("av1_mv_bit_cost", "av1_set_ref_frame", "av1_drl_ctx")):
        return None
    L.av1_mv_bit_cost.restype = ctypes.c_int32
    L.av1_mv_bit_cost.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int32]
    L.av1_set_ref_frame.restype = None
    L.av1_set_ref_frame.argtypes = [ctypes.c_void_p, ctypes.c_int8]
    L.av1_drl_ctx.restype = ctypes.c_uint8
    L.av1_drl_ctx.argtypes = [ctypes.c_void_p, ctypes.c_int32]
    return L


def lib_mv_bit_cost(L, mv_cost, joint_cost, mv, ref):
    a, b = MV(*mv), MV(*ref)
    ptrs = (ctypes.c_void_p * 2)(mv_cost[0].ctypes.data + 4 * MV_MAX, mv_cost[1].ctypes.data + 4 * MV_MAX)      # EbMdRateEstimation.c:363-366
    return L.av1_mv_bit_cost(ctypes.byref(a), ctypes.byref(b), joint_cost.ctypes.data_as(ctypes.c_void_p), ptrs, MV_COST_WEIGHT)


def lib_set_ref_frame(L, t):
    rf = (ctypes.c_int8 * 2)()
    L.av1_set_ref_frame(rf, t)
    return int(rf[0]), int(rf[1])


def lib_drl_ctx(L, w, idx):
    st = (CandidateMv * 4)()
    for i in range(4):
        st[i].weight = w[i]
    return int(L.av1_drl_ctx(st, idx))


def check_leaves(L, mv_cost, rate_sets, mv_pairs, sse_used, weights):
    mv_cost = np.ascontiguousarray(mv_cost)
    for R in rate_sets:
        joint = np.ascontiguousarray(R["nmv_vec_cost"], np.int32)
        for mv, ref in mv_pairs:
            assert lib_mv_bit_cost(L, mv_cost, joint, mv, ref) == mv_bit_cost(mv_cost, joint, mv, ref), (mv, ref)
    for t in range(1, 29):
        assert lib_set_ref_frame(L, t) == tuple(set_ref_frame(t)), t
    for w, byte in weights:
        assert sum(lib_drl_ctx(L, w, idx) << (2 * idx) for idx in range(3)) == byte, w
    for sse, bsize, q in sse_used:
        assert FP.lib_model_rd(L, sse, bsize, q) == FP.ref_model_rd(sse, NUM_PELS_LOG2[bsize], q), (sse, bsize, q)


def ref_predictor(R):
    return lambda planes, bd, ss, plane, bw, bh, blk: IP.ref_inter_pred(R, planes, bd, ss, plane, bw, bh, blk)


def np_predictor(taps):
    return lambda planes, bd, ss, plane, bw, bh, blk: IP.np_inter_pred(taps, planes, bd, ss, plane, bw, bh, blk)


def main():
    R, L = IP.ref_lib(), ref_lib()
    assert R is not None and L is not None, "oracle/_ref/libsvtref.so is not built: run build() first"
    z = generate(ref_predictor(R), L)
    np.savez_compressed(OUT, **z)
    print(f"wrote {OUT}: {os.path.getsize(OUT)} bytes, {len(z)} arrays; pins (mv pairs, sse, drl weights, lib sorts) {z['pins'].tolist()}, "
          f"walk (swap fired, idle, all intra, intra-inter-intra) {z['coverage_walk'].tolist()}, domain {z['domain'].tolist()}")


if __name__ == "__main__":
    main()

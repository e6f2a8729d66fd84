"""Writes tests/golden/partition.npz: the d1 / d2 partition decision of mode_decision_sb and the final block list of the encode pass, on
synthetic leaf lists, costs and partitionFacBits.

What is pinned to what.  Per superblock the REFERENCE's own functions run whole in oracle/_ref/libsvtref.so through ctypes:
Initialize_cu_data_structure (EbProductCodingLoop.c:651-683), d1_non_square_block_decision (EbFullLoop.c:1876-1898) and
d2_inter_depth_block_decision (:2037-2103), which itself calls the compiled compute_depth_costs (:1902-2035) and av1_split_flag_rate
(EbRateDistortionCost.c:2268-2342).  Per square cost, part, split_flag, best_d1_blk and tested_cu_flag are read back from
md_local_cu_unit / md_cu_arr_nsq.  The geometry table is get_blk_geom_mds after build_blk_geom(0), recorded as data.  The functions read
and write through pointers; the structs built here are zero-filled byte buffers with the members at their offsetof offsets (taken once
from a program compiled against the reference's headers, bit-fields as a byte and a mask; self_check() proves for every member used
that a written value is the one the functions read).  GLUE, written line by line from the reference: the loop of mode_decision_sb
(:3375-3502) without md_encode_block and the neighbour arrays (ref_partition: what each entry stores, when d1 and d2 run), with the
entry's cost stored where product_full_mode_decision stores it and the PART_N entry's contexts where md_encode_block stores them; and
the walk of the encode pass (EbCodingLoop.c:2571-2589, :3618-3621; glue_final).  Stale memory is DEFINED as zero: md_local_cu_unit and
md_cu_arr_nsq are zeroed per superblock before Initialize_cu_data_structure.  np_partition is a second restatement of everything,
written independently as array arithmetic level by level; tests compare the fixture with it, and so does main().

partitionFacBits is SYNTHETIC: random int32 below 2^13 (the magnitude av1_cost_tokens_from_cdf produces).

CPU only; run from the repository root after build():  python tests/golden/make_golden_partition.py
"""
import ctypes
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(ROOT, "tests"))

OUT = os.path.join(HERE, "partition.npz")
REF = os.path.join(ROOT, "oracle", "_ref", "libsvtref.so")

# ---- offsets (bytes); a bit-field or scalar member is (first byte, mask of its bits from there, little endian) ----
SIZEOF_CTX = 15460456                             # ModeDecisionContext_s
OFF_CTX_MD_RATE_PTR, OFF_CTX_MD_LOCAL_CU_UNIT, OFF_CTX_MD_CU_ARR_NSQ, OFF_CTX_CU_PTR, OFF_CTX_BLK_GEOM = 48, 64, 12484968, 15137808, 15137816
CTX_FULL_LAMBDA, CTX_SB_ORIGIN_X, CTX_SB_ORIGIN_Y = (15137776, 0xffffffff), (15456284, 0xffffffff), (15456288, 0xffffffff)
SIZEOF_MDCU, OFF_MDCU_COST = 2824, 24             # MdCodingUnit_t
MDCU_TESTED, MDCU_LEFT_PARTITION, MDCU_ABOVE_PARTITION = (0, 0x1), (20, 0xff), (21, 0xff)
SIZEOF_CU = 600                                   # CodingUnit_s
CU_SPLIT_FLAG, CU_MDC_SPLIT_FLAG, CU_PART, CU_MDS_IDX, CU_BEST_D1_BLK = (189, 0x1), (189, 0x4), (540, 0xff), (542, 0xffff), (592, 0xffffffff)
SIZEOF_PCS, OFF_PCS_SCS_WRAPPER_PTR, PCS_SLICE_TYPE = 4320, 0, (329, 0xff)       # PictureControlSet_s
SIZEOF_WRAPPER, OFF_WRAPPER_OBJECT_PTR = 32, 0    # EbObjectWrapper
SIZEOF_SCS = 1264                                 # SequenceControlSet
SCS_SB_SIZE, SCS_LUMA_WIDTH, SCS_LUMA_HEIGHT, SCS_MAX_BLOCK_CNT = (832, 0xff), (340, 0xffff), (342, 0xffff), (728, 0xffff)
SIZEOF_MD, OFF_MD_PARTITION = 834144, 72          # MdRateEstimationContext_s; partitionFacBits [20][11]
SIZEOF_GEOM = 92                                  # BlockGeom
GEOM_FIELDS = dict(depth=(0, 1), shape=(1, 1), origin_x=(2, 1), origin_y=(3, 1), d1i=(4, 1), sqi_mds=(6, 2), totns=(8, 1), nsi=(9, 1), bwidth=(10, 1),
                   bheight=(11, 1), bsize=(16, 1), has_uv=(80, 4), sq_size=(84, 4), is_last_quadrant=(88, 4))      # (offset, bytes)
I_SLICE, P_SLICE, BLOCK_64X64 = 2, 1, 12
PARTITION_NONE, PARTITION_SPLIT = 0, 3
MAX_MODE_COST = 13616969489728 * 8
NBLK, NSQ, MAX_FINAL = 1101, 341, 256
BITS_SHAPE = (20, 11)
NO_SRC = 0xFFFFFFFF
M64 = 0xFFFFFFFFFFFFFFFF
NS_BLK_OFFSET = (0, 1, 3, 25, 5, 8, 11, 14, 17, 21)      # by part (EbModeDecisionConfigurationProcess.h:23-24): data of the encode pass walk
NS_BLK_NUM = (1, 2, 2, 4, 3, 3, 3, 3, 4, 4)
NS_DEPTH_OFFSET = (1101, 269, 61, 9, 1)                  # EbUtility.h:96-106
D1_DEPTH_OFFSET = (25, 25, 25, 5, 1)

GEOM_DTYPE = np.dtype([("sqi_mds", "<u2")] + [(n, "u1") for n in ("bsize", "shape", "depth", "nsi", "totns", "d1i", "origin_x", "origin_y", "bwidth",
                                                                  "bheight", "sq_size", "is_last_quadrant", "has_uv", "pad")])      # svt_hip_blk_geom
LEAF_DTYPE = np.dtype([("mds_idx", "<u2"), ("split_flag", "u1"), ("tot_d1_blocks", "u1"), ("left_partition", "i1"), ("above_partition", "i1"),
                       ("pad", "u1", (2,)), ("src", "<u4")])                                                                      # svt_hip_part_leaf
SB_DTYPE = np.dtype([("leaf_first", "<u4"), ("leaf_count", "<u2"), ("origin_x", "<u2"), ("origin_y", "<u2"), ("pad", "<u2")])      # svt_hip_part_sb
SQ_DTYPE = np.dtype([("cost", "<u8"), ("best_d1_blk", "<u2"), ("part", "u1"), ("split_flag", "u1"), ("tested", "u1"), ("pad", "u1", (3,))])      # svt_hip_part_sq
FINAL_DTYPE = np.dtype([("mds_idx", "<u2"), ("x", "<u2"), ("y", "<u2"), ("bsize", "u1"), ("part", "u1"), ("src", "<u4")])          # svt_hip_part_final
assert (GEOM_DTYPE.itemsize, LEAF_DTYPE.itemsize, SB_DTYPE.itemsize, SQ_DTYPE.itemsize, FINAL_DTYPE.itemsize) == (16, 12, 12, 16, 12)


# ---------------------------------------------------------------------------------------------------------------------------
# the reference
# ---------------------------------------------------------------------------------------------------------------------------
_lib = None


def ref_lib():
    global _lib
    if _lib is None and os.path.exists(REF):
        L = ctypes.CDLL(REF)
        P = ctypes.c_void_p
        L.build_blk_geom.restype = None
        L.build_blk_geom.argtypes = [ctypes.c_int32]
        L.get_blk_geom_mds.restype = P
        L.get_blk_geom_mds.argtypes = [ctypes.c_uint32]
        L.Initialize_cu_data_structure.restype = None
        L.Initialize_cu_data_structure.argtypes = [P, P, P, P]
        L.d1_non_square_block_decision.restype = None
        L.d1_non_square_block_decision.argtypes = [P]
        L.d2_inter_depth_block_decision.restype = ctypes.c_uint32
        L.d2_inter_depth_block_decision.argtypes = [P, ctypes.c_uint32, P, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_uint64, P, P]
        L.build_blk_geom(0)
        assert ctypes.c_uint32.in_dll(L, "max_num_active_blocks").value == NBLK
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


def ref_geometry(L):
    """get_blk_geom_mds for all 1 101 blocks -> GEOM_DTYPE [1101]"""
    g = np.zeros(NBLK, GEOM_DTYPE)
    for i in range(NBLK):
        raw = np.ctypeslib.as_array(ctypes.cast(L.get_blk_geom_mds(i), ctypes.POINTER(ctypes.c_uint8)), shape=(SIZEOF_GEOM,))
        for name, (at, nbytes) in GEOM_FIELDS.items():
            g[name][i] = int.from_bytes(raw[at:at + nbytes].tobytes(), "little")
    return g


class RefPart:
    """the structs the partition functions read and write through, as zero-filled byte buffers"""

    def __init__(self, L, bits, lam, pic_width, pic_height, slice_is_intra):
        self.L = L
        self.ctx, self.md = np.zeros(SIZEOF_CTX, np.uint8), np.zeros(SIZEOF_MD, np.uint8)
        self.pcs, self.wrapper, self.scs = np.zeros(SIZEOF_PCS, np.uint8), np.zeros(SIZEOF_WRAPPER, np.uint8), np.zeros(SIZEOF_SCS, np.uint8)
        self.dummy = np.zeros(1 << 16, np.uint8)                             # sb_ptr / mdcResultTbPtr: named, never read
        self.md[OFF_MD_PARTITION:OFF_MD_PARTITION + 4 * bits.size].view(np.int32)[:] = np.asarray(bits, np.int32).reshape(-1)
        put64(self.ctx, OFF_CTX_MD_RATE_PTR, self.md.ctypes.data)
        put(self.ctx, CTX_FULL_LAMBDA, lam)
        put64(self.pcs, OFF_PCS_SCS_WRAPPER_PTR, self.wrapper.ctypes.data)
        put64(self.wrapper, OFF_WRAPPER_OBJECT_PTR, self.scs.ctypes.data)
        put(self.pcs, PCS_SLICE_TYPE, I_SLICE if slice_is_intra else P_SLICE)
        put(self.scs, SCS_SB_SIZE, BLOCK_64X64); put(self.scs, SCS_LUMA_WIDTH, pic_width); put(self.scs, SCS_LUMA_HEIGHT, pic_height)
        put(self.scs, SCS_MAX_BLOCK_CNT, NBLK)

    def mdcu(self, mds):
        at = OFF_CTX_MD_LOCAL_CU_UNIT + SIZEOF_MDCU * mds
        return self.ctx[at:at + SIZEOF_MDCU]

    def cu(self, mds):
        at = OFF_CTX_MD_CU_ARR_NSQ + SIZEOF_CU * mds
        return self.ctx[at:at + SIZEOF_CU]

    def start(self, origin_x, origin_y):
        self.ctx[OFF_CTX_MD_LOCAL_CU_UNIT:OFF_CTX_MD_LOCAL_CU_UNIT + SIZEOF_MDCU * NBLK] = 0      # stale memory is defined as zero
        self.ctx[OFF_CTX_MD_CU_ARR_NSQ:OFF_CTX_MD_CU_ARR_NSQ + SIZEOF_CU * NBLK] = 0
        put(self.ctx, CTX_SB_ORIGIN_X, origin_x); put(self.ctx, CTX_SB_ORIGIN_Y, origin_y)
        self.L.Initialize_cu_data_structure(self.ctx.ctypes.data, self.scs.ctypes.data, self.dummy.ctypes.data, self.dummy.ctypes.data)

    def entry(self, mds):
        """context_ptr->blk_geom / cu_ptr of the entry (:3382-3383)"""
        put64(self.ctx, OFF_CTX_BLK_GEOM, self.L.get_blk_geom_mds(mds))
        put64(self.ctx, OFF_CTX_CU_PTR, self.cu(mds).ctypes.data)

    def d1(self):
        self.L.d1_non_square_block_decision(self.ctx.ctypes.data)

    def d2(self, sqi_mds):
        return int(self.L.d2_inter_depth_block_decision(self.ctx.ctypes.data, sqi_mds, None, 0, 0, 0, 0, None, self.pcs.ctypes.data))

    def square(self, mds):
        m, c = self.mdcu(mds), self.cu(mds)
        return get64(m, OFF_MDCU_COST), get(c, CU_BEST_D1_BLK), get(c, CU_PART), get(c, CU_SPLIT_FLAG), get(m, MDCU_TESTED)


def ref_superblock(r, geom, origin_x, origin_y, leaves, costs):
    """the loop of mode_decision_sb (:3375-3502) for one superblock, as glue around the compiled functions -> SQ_DTYPE [341]"""
    r.start(origin_x, origin_y)
    d1_blocks_accumlated = 0
    for lf in leaves:
        blk_idx_mds = int(lf["mds_idx"])
        g = geom[blk_idx_mds]
        r.entry(blk_idx_mds)
        m, c = r.mdcu(blk_idx_mds), r.cu(blk_idx_mds)
        put(m, MDCU_TESTED, 1)
        put(c, CU_MDS_IDX, blk_idx_mds)
        put(c, CU_MDC_SPLIT_FLAG, int(lf["split_flag"]) & 1)
        put(c, CU_SPLIT_FLAG, int(lf["split_flag"]) & 1)
        put(c, CU_BEST_D1_BLK, blk_idx_mds)
        # md_encode_block: the neighbour arrays' partition contexts and the winner's cost
        if g["shape"] == 0:
            put(m, MDCU_LEFT_PARTITION, int(lf["left_partition"]) & 0xff); put(m, MDCU_ABOVE_PARTITION, int(lf["above_partition"]) & 0xff)
        put64(m, OFF_MDCU_COST, int(costs[int(lf["src"])]))
        if g["nsi"] + 1 == g["totns"]:
            r.d1()
        d1_blocks_accumlated = 1 if g["shape"] == 0 else d1_blocks_accumlated + 1
        if d1_blocks_accumlated == int(lf["tot_d1_blocks"]):
            r.d2(int(g["sqi_mds"]))
    sq = np.zeros(NSQ, SQ_DTYPE)
    for s, mds in enumerate(square_mds(geom)):
        sq["cost"][s], sq["best_d1_blk"][s], sq["part"][s], sq["split_flag"][s], sq["tested"][s] = r.square(int(mds))
    return sq


def glue_final(geom, sq, origin_x, origin_y, leaves):
    """the walk of the encode pass (EbCodingLoop.c:2571-2589, :3618-3621) over the squares' part -> FINAL_DTYPE [count]"""
    part_of = dict(zip(square_mds(geom).tolist(), sq["part"].tolist()))
    src_of = {int(lf["mds_idx"]): int(lf["src"]) for lf in leaves}
    out, blk_it = [], 0
    while blk_it < NBLK:
        part = part_of[blk_it]
        depth = int(geom["depth"][blk_it])
        if part != PARTITION_SPLIT:
            for d1_itr in range(blk_it + NS_BLK_OFFSET[part], blk_it + NS_BLK_OFFSET[part] + NS_BLK_NUM[part]):
                g = geom[d1_itr]
                out.append((d1_itr, origin_x + int(g["origin_x"]), origin_y + int(g["origin_y"]), int(g["bsize"]), part, src_of.get(d1_itr, NO_SRC)))
            blk_it += NS_DEPTH_OFFSET[depth]
        else:
            blk_it += D1_DEPTH_OFFSET[depth]
    return np.array(out, FINAL_DTYPE) if out else np.zeros(0, FINAL_DTYPE)


def square_mds(geom):
    """the mds index of the 341 squares, in mds order"""
    return np.nonzero(geom["shape"] == 0)[0]


def ref_partition(L, case, geom):
    """a case through the compiled reference -> (SQ_DTYPE [nsb, 341], counts [nsb], FINAL_DTYPE [sum of counts])"""
    r = RefPart(L, case["bits"], int(case["lam"]), int(case["pic_width"]), int(case["pic_height"]), int(case["slice_is_intra"]))
    sqs, finals = [], []
    for sb in case["sb"]:
        leaves = case["leaf"][int(sb["leaf_first"]):int(sb["leaf_first"]) + int(sb["leaf_count"])]
        sq = ref_superblock(r, geom, int(sb["origin_x"]), int(sb["origin_y"]), leaves, case["cost"])
        sqs.append(sq)
        finals.append(glue_final(geom, sq, int(sb["origin_x"]), int(sb["origin_y"]), leaves))
    return np.stack(sqs), np.array([len(f) for f in finals], np.uint32), np.concatenate(finals)


# ---------------------------------------------------------------------------------------------------------------------------
# restatement 2: array arithmetic, level by level (what the tests use where the reference is not built)
# ---------------------------------------------------------------------------------------------------------------------------
SHAPE_OFF = np.array([0, 1, 3, 5, 8, 11, 14, 17, 21])
SHAPE_N = np.array([1, 2, 2, 3, 3, 3, 3, 4, 4])
SHAPE_PART = np.array([0, 1, 2, 4, 5, 6, 7, 8, 9])
VERT_ALIKE, HORZ_ALIKE = (2, 3, 4, 6, 7, 9), (1, 3, 4, 5, 6, 8)


def np_rate(case, size, px, py, left, above, split):
    """av1_split_flag_rate for squares of one size at picture positions px, py (arrays) -> uint64 array"""
    bits, lam = np.asarray(case["bits"], np.int64).reshape(BITS_SHAPE), np.uint64(int(case["lam"]))
    px, py = np.asarray(px, np.int64), np.asarray(py, np.int64)
    ptype = PARTITION_SPLIT if split else PARTITION_NONE
    if size < 8:
        rate = np.full(px.shape, bits[0, ptype])
    else:
        hbs, bsl = size // 2, int(np.log2(size // 8))
        rows, cols = py + hbs < int(case["pic_height"]), px + hbs < int(case["pic_width"])
        fix = lambda c: np.where(np.asarray(c, np.int64) == -1, 0, np.asarray(c, np.int64))
        ctx = ((fix(left) >> bsl) & 1) * 2 + ((fix(above) >> bsl) & 1) + 4 * bsl
        row = bits[ctx]                                                         # [..., 11], a row of bits taken for a CDF
        prob = lambda e: row[..., e - 1] - row[..., e]                          # cdf_element_prob for e > 0
        gather = lambda es: sum(prob(e) for e in es).astype(np.int32).astype(np.int64)
        edge = np.int64(0) if split else np.where(~rows & cols, gather(VERT_ALIKE), gather(HORZ_ALIKE))
        rate = np.where(rows & cols, bits[4 if size == 8 else 10, ptype], edge)
    with np.errstate(over="ignore"):
        return (rate.astype(np.uint64) * lam + np.uint64(256)) >> np.uint64(9)


def np_superblock(case, geom, origin_x, origin_y, leaves):
    """-> (SQ_DTYPE [341], FINAL_DTYPE [count])"""
    sqm = square_mds(geom)
    mds = leaves["mds_idx"].astype(np.int64)
    n = len(mds)
    cost, listed, src_of = np.zeros(NBLK + 1, np.uint64), np.zeros(NBLK, bool), np.full(NBLK, NO_SRC, np.uint32)
    cost[mds], listed[mds], src_of[mds] = case["cost"][leaves["src"]], True, leaves["src"]
    tested, mdc, called = np.zeros(NBLK, bool), np.zeros(NBLK, bool), np.zeros(NBLK, bool)
    split, part, best = np.ones(NBLK, np.uint8), np.full(NBLK, PARTITION_SPLIT, np.uint8), np.zeros(NBLK, np.uint16)
    left, above = np.zeros(NBLK, np.int64), np.zeros(NBLK, np.int64)
    is_n = geom["shape"][mds] == 0
    tested[mds[is_n]] = True
    mdc[mds[is_n]] = (leaves["split_flag"][is_n] & 1) != 0
    split[mds[is_n]] = leaves["split_flag"][is_n] & 1
    left[mds[is_n]], above[mds[is_n]] = leaves["left_partition"][is_n], leaves["above_partition"][is_n]
    # d1_blocks_accumlated of every entry: the distance to the last PART_N entry at or before it
    idx = np.arange(n)
    last_n = np.maximum.accumulate(np.where(is_n, idx, -1)) if n else idx
    acc = np.where(last_n < 0, idx + 1, idx - last_n + 1)
    called[geom["sqi_mds"][mds[acc == leaves["tot_d1_blocks"]]]] = True
    with np.errstate(over="ignore"):
        # d1, shapes ascending
        for shape in range(9):
            sq = sqm[(geom["sq_size"][sqm] >= 16) | ((geom["sq_size"][sqm] == 8) & (shape < 3)) | (shape == 0)]
            first = sq + SHAPE_OFF[shape]
            tot = sum(cost[first + k] for k in range(SHAPE_N[shape]))
            take = listed[first + SHAPE_N[shape] - 1] & ((shape == 0) | (tot < cost[sq]))
            cost[sq[take]], part[sq[take]], best[sq[take]] = tot[take], SHAPE_PART[shape], first[take]
        # d2, from the 8x8 parents up
        compared, began4 = np.zeros(NBLK, bool), np.zeros(NBLK, bool)
        carry = np.uint64(0)
        for depth in (3, 2, 1, 0):
            par = sqm[geom["depth"][sqm] == depth]
            size = 64 >> depth
            kids = [par + D1_DEPTH_OFFSET[depth] + k * NS_DEPTH_OFFSET[depth + 1] for k in range(4)]
            starts = called[kids[3]] & tested[kids[3]] & ~mdc[kids[3]]
            do = starts | compared[kids[3]]
            b4 = np.where(starts, depth == 3, began4[kids[3]])
            if depth == 0 and int(case["slice_is_intra"]):
                parent_cost = np.full(1, MAX_MODE_COST, np.uint64)
                current = np.where(compared[kids[3]], carry, np.uint64(0))
            else:
                l, a = left[kids[0]], above[kids[0]]
                px, py = origin_x + geom["origin_x"][par].astype(np.int64), origin_y + geom["origin_y"][par].astype(np.int64)
                parent_cost = np.where(tested[par], cost[par] + np_rate(case, size, px, py, l, a, False), np.uint64(MAX_MODE_COST))
                current = np_rate(case, size, px, py, l, a, True)
                for k in kids:
                    kx, ky = origin_x + geom["origin_x"][k].astype(np.int64), origin_y + geom["origin_y"][k].astype(np.int64)
                    current = current + cost[k] + np.where(~b4 & ~mdc[k], np_rate(case, size // 2, kx, ky, left[k], above[k], False), np.uint64(0))
                left[par[do]], above[par[do]] = l[do], a[do]
            keep = do & (parent_cost <= current)
            cut = do & ~keep
            split[par[keep]], cost[par[keep]] = 0, parent_cost[keep]
            cost[par[cut]], part[par[cut]] = current[cut], PARTITION_SPLIT
            compared[par[do]], began4[par[do]] = True, b4[do]
            if depth == 1:
                carry = current[3]
    sq = np.zeros(NSQ, SQ_DTYPE)
    sq["cost"], sq["best_d1_blk"], sq["part"], sq["split_flag"], sq["tested"] = cost[sqm], best[sqm], part[sqm], split[sqm], tested[sqm]
    # the final blocks: a square is coded when its part is not SPLIT and every ancestor's is
    reached = np.ones(NBLK, bool)
    for depth in range(4):
        par = sqm[geom["depth"][sqm] == depth]
        for k in range(4):
            kid = par + D1_DEPTH_OFFSET[depth] + k * NS_DEPTH_OFFSET[depth + 1]
            reached[kid] = reached[par] & (part[par] == PARTITION_SPLIT)
    coded = sqm[reached[sqm] & (part[sqm] != PARTITION_SPLIT)]
    blocks = np.concatenate([s + NS_BLK_OFFSET[part[s]] + np.arange(NS_BLK_NUM[part[s]]) for s in coded]) if len(coded) else np.zeros(0, np.int64)
    final = np.zeros(len(blocks), FINAL_DTYPE)
    final["mds_idx"], final["x"], final["y"] = blocks, origin_x + geom["origin_x"][blocks].astype(np.int64), origin_y + geom["origin_y"][blocks].astype(np.int64)
    final["bsize"], final["part"], final["src"] = geom["bsize"][blocks], part[geom["sqi_mds"][blocks]], src_of[blocks]
    return sq, final


def np_partition(case, geom):
    """svt_hip_partition_decide_frame for a case -> (SQ_DTYPE [nsb, 341], counts uint32 [nsb], FINAL_DTYPE [sum of counts])"""
    sqs, finals = [], []
    for sb in case["sb"]:
        leaves = case["leaf"][int(sb["leaf_first"]):int(sb["leaf_first"]) + int(sb["leaf_count"])]
        sq, final = np_superblock(case, geom, int(sb["origin_x"]), int(sb["origin_y"]), leaves)
        sqs.append(sq); finals.append(final)
    return np.stack(sqs), np.array([len(f) for f in finals], np.uint32), np.concatenate(finals)


# ---------------------------------------------------------------------------------------------------------------------------
# the cases
# ---------------------------------------------------------------------------------------------------------------------------
CASE_NAMES = ("single64", "squares_to_8", "squares_to_4", "squares_h_v", "all_blocks", "irregular", "d1_subsets", "ties", "islice_all", "islice_irregular",
              "edges", "max_mode_cost")
LAMBDA = 29041


def build_list(rng, geom, pic_width, pic_height, origin_x, origin_y, min_size, shapes, p_split=1.0, p_unlisted=0.0, contexts=False):
    """a leaf list as MDC makes it -> [(mds, split_flag, tot_d1_blocks, left, above)], ascending mds.  A square wholly inside the picture
    is listed (unless p_unlisted drops it) with the blocks `shapes` selects; one crossing the edge is not listed and its quadrants are
    visited; one outside is dropped.  split_flag 1 goes with visiting the quadrants."""
    out = []

    def visit(mds):
        g = geom[mds]
        size, x, y = int(g["sq_size"]), origin_x + int(g["origin_x"]), origin_y + int(g["origin_y"])
        if x >= pic_width or y >= pic_height:
            return
        inside = x + size <= pic_width and y + size <= pic_height
        deeper = size > min_size and (not inside or rng.random() < p_split)
        if inside and (not deeper or rng.random() >= p_unlisted):
            nshapes = 9 if size >= 16 else (3 if size == 8 else 1)
            blocks = [0] + [SHAPE_OFF[s] + k for s in range(1, nshapes) for k in range(SHAPE_N[s]) if shapes(rng, size, s, k)]
            ctx = (int(rng.integers(-1, 32)), int(rng.integers(-1, 32))) if contexts else (0, 0)
            for b in blocks:
                out.append((mds + int(b), int(deeper), len(blocks)) + (ctx if b == 0 else (0, 0)))
        if deeper:
            for k in range(4):
                visit(mds + D1_DEPTH_OFFSET[int(g["depth"])] + k * NS_DEPTH_OFFSET[int(g["depth"]) + 1])

    visit(0)
    return out


def area_costs(rng, geom, mds, spread):
    """costs that make both outcomes of d1 and d2 frequent: a distortion of 100 per pixel times 128 (RDCOST's D << 7), which puts an 8x8
    at three to four partition rates, each block up to spread / 2 away from it, 7 % less per depth"""
    area = geom["bwidth"][mds].astype(np.int64) * geom["bheight"][mds].astype(np.int64)
    detail = np.where(spread > 0, 0.93, 1.0) ** geom["depth"][mds]              # smaller squares a little cheaper per pixel: the rates pull the other way
    return (area * 12800 * detail * (1 + spread * (rng.random(len(mds)) - 0.5))).astype(np.uint64)


def make_case(name, geom):
    """-> dict: bits int32 [20, 11], lam, pic_width, pic_height, slice_is_intra, sb SB_DTYPE [nsb], leaf LEAF_DTYPE [nleaves], cost uint64 [nsrc]"""
    rng = np.random.default_rng(1900 + CASE_NAMES.index(name))
    bits = rng.integers(0, 1 << 13, BITS_SHAPE).astype(np.int32)
    pic_width, pic_height, islice, nsb = 256, 192, 0, 3
    origins, kept = None, []
    only_n = lambda rng, size, s, k: False
    hv = lambda rng, size, s, k: s < 3
    every = lambda rng, size, s, k: True
    kw = dict(min_size=64, shapes=only_n)
    spread = 0.3
    if name == "squares_to_8":
        kw = dict(min_size=8, shapes=only_n)
    elif name == "squares_to_4":
        kw = dict(min_size=4, shapes=only_n, contexts=True)
    elif name == "squares_h_v":
        kw = dict(min_size=8, shapes=hv)
    elif name in ("all_blocks", "islice_all"):
        kw, nsb, islice = dict(min_size=4, shapes=every, contexts=True), 2, int(name == "islice_all")
    elif name in ("irregular", "islice_irregular"):
        kw, nsb, islice = dict(min_size=4, shapes=hv, p_split=0.6, p_unlisted=0.15, contexts=True), 6, int(name == "islice_irregular")
    elif name == "d1_subsets":
        kw, nsb = dict(min_size=8, shapes=lambda rng, size, s, k: rng.random() < 0.4, p_split=0.7), 4       # any subset of blocks: a last block without its first
    elif name == "ties":
        kw, bits, spread = dict(min_size=8, shapes=hv), np.zeros(BITS_SHAPE, np.int32), 0.0                  # every sum ties: N stays, the parent stays
    elif name == "edges":
        pic_width, pic_height = 200, 168                                                                    # 3 x 64 + 8, 2 x 64 + 40
        origins = [(192, 0), (192, 64), (0, 128), (64, 128), (192, 128)]                                     # right, right, bottom, bottom, corner
        kw = dict(min_size=4, shapes=hv, p_split=0.7, p_unlisted=0.2, contexts=True)
        # a dropped fourth quadrant ends every climb below a square whose right or bottom half is outside, so a list as MDC makes it
        # never takes a PARTITION_NONE rate on the edge's gather path.  Three more superblocks (right, bottom, corner) keep their
        # out-of-picture blocks listed: there the gathers and the contexts decide.
        kept = [(192, 64), (64, 128), (192, 128)]
    elif name == "max_mode_cost":
        kw = dict(min_size=16, shapes=hv)
    if origins is None:
        origins = [(64 * (i % 4), 64 * (i // 4)) for i in range(nsb)]
    mdc = len(origins)
    origins = origins + kept
    sb, leaf = np.zeros(len(origins), SB_DTYPE), []
    for i, (ox, oy) in enumerate(origins):
        rows = build_list(rng, geom, *((pic_width, pic_height) if i < mdc else (1 << 15, 1 << 15)), ox, oy, **kw)
        sb["leaf_first"][i], sb["leaf_count"][i], sb["origin_x"][i], sb["origin_y"][i] = len(leaf), len(rows), ox, oy
        leaf += rows
    lf = np.zeros(len(leaf), LEAF_DTYPE)
    for i, (mds, flag, tot, l, a) in enumerate(leaf):
        lf["mds_idx"][i], lf["split_flag"][i], lf["tot_d1_blocks"][i], lf["left_partition"][i], lf["above_partition"][i] = mds, flag, tot, l, a
    lf["src"] = rng.permutation(len(lf))                                                                     # the indirection is part of every case
    cost = np.zeros(len(lf), np.uint64)
    cost[lf["src"]] = area_costs(rng, geom, lf["mds_idx"].astype(np.int64), spread)
    if name == "squares_to_4":                                                                               # superblock 0: the 4x4s win everywhere, 256 final blocks
        first = lf[:int(sb["leaf_count"][0])]
        cost[first["src"]] = np.where(geom["sq_size"][first["mds_idx"]] == 4, 1, cost[first["src"]])
    if name == "max_mode_cost":
        for i in range(len(sb)):                                                                             # a 32x32, a 16x16 H block, the 64x64
            at = int(sb["leaf_first"][i])
            pick = [j for j in range(at, at + int(sb["leaf_count"][i])) if (geom["sq_size"][lf["mds_idx"][j]], geom["shape"][lf["mds_idx"][j]]) == ((32, 0), (16, 1), (64, 0))[i]]
            cost[lf["src"][pick[len(pick) // 2]]] = MAX_MODE_COST
    return dict(bits=bits, lam=np.uint32(LAMBDA), pic_width=np.uint32(pic_width), pic_height=np.uint32(pic_height), slice_is_intra=np.int32(islice),
                sb=sb, leaf=lf, cost=cost)


CASE_KEYS = ("bits", "lam", "pic_width", "pic_height", "slice_is_intra", "sb", "leaf", "cost")
NCASES = len(CASE_NAMES)
COMBINED = NCASES                                    # one more case: every superblock of the others in ONE call
ALL_NAMES = CASE_NAMES + ("combined",)


def combined_case(cases):
    """every superblock, leaf and cost of the given cases in one list (46 superblocks: a partial workgroup of four), under one set of
    scalars: the edge picture, a non-I slice, a table of its own.  Only its outputs are stored; the inputs are put together again"""
    rng = np.random.default_rng(1900 + COMBINED)
    sb, leaf = np.concatenate([c["sb"] for c in cases]), np.concatenate([c["leaf"] for c in cases])
    at_leaf = np.cumsum([0] + [len(c["leaf"]) for c in cases]).astype(np.uint32)
    at_sb = np.cumsum([0] + [len(c["sb"]) for c in cases])
    for i in range(len(cases)):                                             # (a case's leaves are its costs' permutation: one offset serves both)
        sb["leaf_first"][at_sb[i]:at_sb[i + 1]] += at_leaf[i]
        leaf["src"][at_leaf[i]:at_leaf[i + 1]] += at_leaf[i]
    return dict(bits=rng.integers(0, 1 << 13, BITS_SHAPE).astype(np.int32), lam=np.uint32(LAMBDA), pic_width=np.uint32(200), pic_height=np.uint32(168),
                slice_is_intra=np.int32(0), sb=sb, leaf=leaf, cost=np.concatenate([c["cost"] for c in cases]))


def load_case(z, k):
    """case k of the fixture -> (inputs dict, SQ_DTYPE [nsb, 341], counts [nsb], FINAL_DTYPE [sum of counts])"""
    if k == COMBINED:
        c = combined_case([load_case(z, j)[0] for j in range(NCASES)])
    else:
        c = {key: z[f"c{k}_{key}"] for key in CASE_KEYS}
        c["sb"], c["leaf"] = c["sb"].view(SB_DTYPE).reshape(-1), c["leaf"].view(LEAF_DTYPE).reshape(-1)
    return c, z[f"c{k}_sq"].view(SQ_DTYPE).reshape(-1, NSQ), z[f"c{k}_count"], z[f"c{k}_final"].view(FINAL_DTYPE).reshape(-1)


def load_geometry(z):
    return z["geom"].view(GEOM_DTYPE).reshape(-1)


# ---------------------------------------------------------------------------------------------------------------------------
def self_check(L, geom):
    """every member written above is the one the functions read, and every one read back is the one they write: one member at a time"""
    bits = (np.arange(220, dtype=np.int32).reshape(BITS_SHAPE) + 1) * 512      # RDCOST(1, 512 v, 0) = v: entry (r, c) costs 11 r + c + 1
    one = lambda mds, flag, tot=1, l=0, a=0, src=0: np.array([(mds, flag, tot, l, a, (0, 0), src)], LEAF_DTYPE)
    r = RefPart(L, bits, 1, 256, 256, 0)
    # an entry: cost, tested, split_flag, part, best_d1_blk of its square; untouched squares keep Initialize_cu_data_structure's values
    sq = ref_superblock(r, geom, 0, 0, one(0, 0), np.array([77], np.uint64))
    assert tuple(sq[0])[:5] == (77, 0, PARTITION_NONE, 0, 1) and tuple(sq[1])[:5] == (0, 0, PARTITION_SPLIT, 1, 0), (sq[0], sq[1])
    sq = ref_superblock(r, geom, 0, 0, one(0, 1), np.array([77], np.uint64))
    assert tuple(sq[0])[:5] == (77, 0, PARTITION_NONE, 1, 1)
    # d1: H (blocks 1, 2) strictly cheaper takes the square: cost, part HORZ, best_d1_blk 1
    lf = np.concatenate([one(0, 0, 3, src=0), one(1, 0, 3, src=1), one(2, 0, 3, src=2)])
    sq = ref_superblock(r, geom, 0, 0, lf, np.array([100, 40, 50], np.uint64))
    assert tuple(sq[0])[:5] == (90, 1, 1, 0, 1), sq[0]
    # d2 at the fourth 32x32 (mds 832): the root is tested, cost 1000; the children 10 each.  Interior: row 10, NONE -> 111, SPLIT -> 114;
    # a child's NONE rate 111 each.  parent = 1000 + 111, current = 40 + 114 + 4 * 111
    kids = [25 + 269 * k for k in range(4)]
    lf = np.concatenate([one(0, 1, src=0)] + [one(m, 0, src=1 + k) for k, m in enumerate(kids)])
    costs = np.array([1000, 10, 10, 10, 10], np.uint64)
    sq = ref_superblock(r, geom, 0, 0, lf, costs)
    assert tuple(sq[0])[:5] == (40 + 114 + 444, 0, PARTITION_SPLIT, 1, 1), sq[0]
    costs[0] = 40 + 114 + 444 - 111                                             # the tie keeps the parent
    sq = ref_superblock(r, geom, 0, 0, lf, costs)
    assert tuple(sq[0])[:5] == (40 + 114 + 444, 0, PARTITION_NONE, 0, 1), sq[0]
    # full_lambda: twice the rates
    r2 = RefPart(L, bits, 2, 256, 256, 0)
    assert int(ref_superblock(r2, geom, 0, 0, lf, np.array([5000, 10, 10, 10, 10], np.uint64))["cost"][0]) == 40 + 2 * (114 + 444)
    # an untested parent costs MAX_MODE_COST: the children win whatever they cost
    sq = ref_superblock(r, geom, 0, 0, lf[1:], costs)
    assert tuple(sq[0])[:5] == (40 + 114 + 444, 0, PARTITION_SPLIT, 1, 0), sq[0]
    # slice_type: the I-slice root is not computed
    ri = RefPart(L, bits, 1, 256, 256, 1)
    sq = ref_superblock(ri, geom, 0, 0, lf, costs)
    assert tuple(sq[0])[:5] == (0, 0, PARTITION_SPLIT, 1, 1), sq[0]
    # luma_width / luma_height, sb_origin and the contexts.  The first three children are listed with split_flag 1 (no NONE rate of their
    # own), the fourth at (32, 32) starts the climb; child 0's contexts (8, 0) go up to the root: bsl 3 -> left 1, above 0 -> row 14.
    # In the self-naming table every element's probability is -512, six of them: a NONE rate of (uint64)-3072, K after RDCOST; row 14's
    # entry 0 raised by 600 * 512 makes HORZ's probability 599 * 512, which only the horz-alike gather reads: 594 after RDCOST.
    K = (((-3072) & M64) + 256) >> 9
    b2 = bits.copy(); b2[14, 0] += 600 * 512
    lfe = lf.copy()
    lfe["split_flag"][1:4], lfe["left_partition"][1], lfe["above_partition"][1] = 1, 8, 0
    ce = np.array([10, 5000, 5000, 5000, 5000], np.uint64)
    for pw, ph, ox, oy, want in ((32, 256, 0, 0, 10 + 594), (256 + 32, 1024, 256, 0, 10 + 594),          # the right half outside: horz alike
                                 (256, 32, 0, 0, 10 + K), (1024, 256 + 32, 0, 256, 10 + K)):             # the bottom half only: vert alike
        sq = ref_superblock(RefPart(L, b2, 1, pw, ph, 0), geom, ox, oy, lfe, ce)
        assert tuple(sq[0])[:5] == (want, 0, PARTITION_NONE, 0, 1), (pw, ph, sq[0])                      # (current holds the fourth child's K + 20000)
    lfe["left_partition"][1] = 0                                                                         # row 12: the raised entry is not read
    sq = ref_superblock(RefPart(L, b2, 1, 32, 256, 0), geom, 0, 0, lfe, ce)
    assert int(sq["cost"][0]) == 10 + K, sq[0]
    lfe["left_partition"][1], lfe["above_partition"][1] = -1, 8                                          # INVALID_NEIGHBOR_DATA is 0; above 1 -> row 13
    b3 = bits.copy(); b3[13, 0] += 600 * 512
    sq = ref_superblock(RefPart(L, b3, 1, 32, 256, 0), geom, 0, 0, lfe, ce)
    assert int(sq["cost"][0]) == 10 + 594, sq[0]
    # mdc_split_flag: a child listed with split_flag 1 adds no NONE rate (and, being split, starts no climb: the fourth stays 0)
    lfm = lf.copy(); lfm["split_flag"][1] = 1
    sq = ref_superblock(r, geom, 0, 0, lfm, np.array([5000, 10, 10, 10, 10], np.uint64))
    assert int(sq["cost"][0]) == 40 + 114 + 333


def check_conditions(cases, outs, geom):
    """the fixture cannot miss the hard paths"""
    f = dict.fromkeys(("d1_n_stays", "d1_other", "d2_keep", "d2_cut", "began4", "untested_parent", "edge_none_rate", "ctx_nonzero", "islice_root_nonzero",
                       "islice_root_zero", "tie_d1", "absent_first", "max_cost", "final_256", "final_1"), False)
    for (name, c), (sq, count, final) in zip(cases, outs):
        sqm = square_mds(geom)
        f["d1_n_stays"] |= bool(((sq["part"] == 0) & (sq["tested"] == 1)).any()); f["d1_other"] |= bool(((sq["part"] != 0) & (sq["part"] != 3)).any())
        f["d2_keep"] |= bool(((sq["split_flag"] == 0) & (geom["sq_size"][sqm] > 8)[None]).any())
        f["d2_cut"] |= bool(((sq["part"] == 3) & (sq["tested"] == 1)).any())
        f["began4"] |= name in ("squares_to_4", "all_blocks") and bool((count > 64).any())
        f["untested_parent"] |= bool(((sq["tested"] == 0) & (sq["cost"] != 0)).any())
        f["ctx_nonzero"] |= bool((c["leaf"]["left_partition"] > 0).any())
        if name == "edges":                                                     # a listed square whose right or bottom half is outside
            for sb in c["sb"]:
                m = c["leaf"]["mds_idx"][int(sb["leaf_first"]):int(sb["leaf_first"]) + int(sb["leaf_count"])]
                m = m[(geom["shape"][m] == 0) & (geom["sq_size"][m] >= 8)]
                half = geom["sq_size"][m].astype(np.int64) // 2
                f["edge_none_rate"] |= bool(((int(sb["origin_x"]) + geom["origin_x"][m] + half >= int(c["pic_width"])) |
                                             (int(sb["origin_y"]) + geom["origin_y"][m] + half >= int(c["pic_height"]))).any())
        if int(c["slice_is_intra"]):
            climbed = sq["split_flag"][:, 0] == 1                              # (a root listed as a leaf is never compared)
            f["islice_root_nonzero"] |= bool((sq["cost"][climbed, 0] != 0).any()); f["islice_root_zero"] |= bool((sq["cost"][climbed, 0] == 0).any())
            assert (sq["part"][climbed, 0] == 3).all()
        if name == "ties":
            f["tie_d1"] = bool((sq["part"][sq["tested"] == 1] == 0).all()) and bool((count == 1).all())
        if name == "d1_subsets":
            listed = set(c["leaf"]["mds_idx"].tolist())
            f["absent_first"] |= any(geom["nsi"][m] > 0 and m - 1 not in listed for m in listed)
        f["max_cost"] |= bool((c["cost"] == MAX_MODE_COST).any())
        f["final_256"] |= bool((count == 256).any()); f["final_1"] |= bool((count == 1).any())
    assert all(f.values()), {k: v for k, v in f.items() if not v}


def main():
    L = ref_lib()
    if L is None:
        raise SystemExit("oracle/_ref/libsvtref.so is not built")
    geom = ref_geometry(L)
    self_check(L, geom)
    out = {"geom": geom.view(np.uint8).reshape(NBLK, GEOM_DTYPE.itemsize), "names": np.array(CASE_NAMES)}
    cases, outs = [], []
    for k, name in enumerate(ALL_NAMES):
        c = make_case(name, geom) if k < NCASES else combined_case([cc for _, cc in cases])
        sq, count, final = ref_partition(L, c, geom)
        n_sq, n_count, n_final = np_partition(c, geom)
        assert np.array_equal(sq, n_sq), (name, np.nonzero(sq != n_sq))
        assert np.array_equal(count, n_count) and np.array_equal(final, n_final), name
        for key in CASE_KEYS if k < NCASES else ():
            v = c[key]
            out[f"c{k}_{key}"] = v.view(np.uint8).reshape(len(v), v.dtype.itemsize) if v.dtype.names else v
        out[f"c{k}_sq"], out[f"c{k}_count"] = sq.view(np.uint8).reshape(len(sq), NSQ, SQ_DTYPE.itemsize), count
        out[f"c{k}_final"] = final.view(np.uint8).reshape(len(final), FINAL_DTYPE.itemsize)
        if k < NCASES:
            cases.append((name, c)); outs.append((sq, count, final))
        print(f"{name}: {len(c['sb'])} superblocks, {len(c['leaf'])} leaves, final {count.tolist()}")
    check_conditions(cases, outs, geom)
    np.savez_compressed(OUT, **out)
    print(f"wrote {OUT}: {os.path.getsize(OUT)} bytes")


if __name__ == "__main__":
    main()

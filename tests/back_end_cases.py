"""Shared by tests/golden/make_golden_back_end.py, tests/test_back_end_cpu.py and tests/test_gpu_back_end.py: the inputs of the back-end
chain on a real picture, every one of them a stated function of tests/golden/real_picture.npz (the source window and its list-0
reference picture), of the geometry tables recorded in partition.npz / recon_final.npz and of the expected final list - so the fixture
(tests/golden/back_end.npz) stores expected outputs only - and the fixture's loader and coverage conditions.  No reference library
and no device is needed here.

The rules (the contract between the calls, stated once):
  leaves   per superblock the MDC list make_golden_partition.build_list makes with every block of every square down to 4x4 (a square
           that crosses the picture edge is not listed, its quadrants are visited); contexts 0.
  src      ONE numbering serves every per-src table of the chain (d_cost, svt_hip_md_decision, svt_hip_intra_enc_blk, svt_hip_dlf_info)
           and the source groups of svt_hip_recon_final_frame: the leaves of one block size are numbered contiguously, sizes ascending,
           inside a size in list order.  A source group is then one block size, and the list svt_hip_partition_decide_frame writes is
           handed to every later call as it is.
  costs    integer arithmetic on the source luma: COST_ACT * (sum |n * sample - block sum| // n) + COST_BLOCK, n the block's area.
  per-src  in the coding order of the final list, i the running index over the picture: is_intra when the block's luma SAD against the
           co-located block of the reference picture exceeds INTRA_SAD_PER_SAMPLE * area, or when its whole superblock's does
           SB_INTRA_SAD_PER_SAMPLE * the superblock's area inside the picture (a superblock the reference predicts badly is coded
           intra throughout: whole CDEF filter blocks without a skipped 8x8); an intra block takes LUMA_MODES[(7 i + bsize)
           % 29], uv_mode 13 when i % 3 == 0 and the size allows CfL, else (5 i + 3) % 13, alpha index (37 i + 11) % 256, signs i % 8,
           and the transform types of make_golden_intra_encode.build_case's turn; an inter block is a skip block: eob 0 in all planes,
           prediction the co-located block of the reference picture, ref_frame0 1, mode GLOBALMV / NEWMV (15 + (i & 1)).
  skip     update_av1_mi_map's rule: with has_uv all three eobs 0, else the luma eob 0.
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, GOLDEN)
import dlf_cases as dc                      # noqa: E402
import make_golden_partition as mg          # noqa: E402
import make_golden_recon_final as mr        # noqa: E402
import make_golden_intra_encode as mi       # noqa: E402
from make_golden_md_decide import DEC_DTYPE  # noqa: E402
from make_golden_dlf import MIN_COVER       # noqa: E402

FIXTURE = os.path.join(GOLDEN, "back_end.npz")
REAL = os.path.join(GOLDEN, "real_picture.npz")
W, H = 352, 224                              # the window of real_picture.npz: 6 x 4 superblocks, the right column and the bottom row partial
SB_COLS, SB_ROWS = (W + 63) // 64, (H + 63) // 64
NSB = SB_COLS * SB_ROWS
STRIDE, ROWS = SB_COLS * 64 + 64, SB_ROWS * 64      # the planes the chain works in (chroma: halves), as the intra pass's model lays them out
PW, PH = (W, W // 2, W // 2), (H, H // 2, H // 2)
PLANES = ("y", "cb", "cr")
MAX_FINAL, NSQ = mg.MAX_FINAL, mg.NSQ
FINAL_DTYPE, BLK_DTYPE, RES_DTYPE = mg.FINAL_DTYPE, mi.BLK_DTYPE, mi.RES_DTYPE
INFO_DTYPE = np.dtype([("ref_frame0", "u1"), ("mode", "u1"), ("skip", "u1"), ("pad", "u1")])      # svt_hip_dlf_info
COST_ACT, COST_BLOCK = 2600, 400000
INTRA_SAD_PER_SAMPLE, SB_INTRA_SAD_PER_SAMPLE = 10, 16
BITS_SEED, LAMBDA = 20261020, mg.LAMBDA
GLOBALMV = 15
DLF_STARTS = ((0, 0, 0, 0), (0, 0, 20, 5))   # last_frame_filter_level of the two walks
LOOP_FILTER_MODE, ONLY_4X4 = 3, 0
SIZE_CAP = 768 << 10
STAT_NAMES = ("final_entries", "block_sizes", "nsq_depths", "count_64x64", "count_4x4", "max_sb_entries", "intra_share", "intra_next_to_inter",
              "inter_next_to_intra", "eob0_share_y", "eob0_share_cb", "eob0_share_cr", "luma_eob_above_10", "cfl_alpha_positive", "cfl_alpha_negative",
              "edges_luma_v_4", "edges_luma_v_8", "edges_luma_v_14", "edges_luma_h_4", "edges_luma_h_8", "edges_luma_h_14", "edges_chroma_v_4",
              "edges_chroma_v_6", "edges_chroma_h_4", "edges_chroma_h_6", "level_luma", "level_u", "level_v", "delta_pv_level_units",
              "cdef_luma_strengths", "cdef_fbs_with_a_skip", "cdef_fbs_without_a_skip")


# ---------------------------------------------------------------------------------------------------------------------------
# inputs
# ---------------------------------------------------------------------------------------------------------------------------
def geometry():
    """(svt_hip_blk_geom records [1101], the reconstruction's geometry records [1101]) as the sibling fixtures recorded them"""
    return mg.load_geometry(np.load(os.path.join(GOLDEN, "partition.npz"))), mr.load_geometry(np.load(os.path.join(GOLDEN, "recon_final.npz")))


def pictures():
    """{src: [y, cb, cr], ref: [y, cb, cr], origin}: the source window and the list-0 reference picture (the window displaced by DISP[0]
    and coded by the reference) of real_picture.npz"""
    z = np.load(REAL)
    return dict(src=[z[f"src_{n}"] for n in PLANES], ref=[z[f"ref0_{n}"] for n in PLANES], origin=z["origin"])


def partition_bits():
    """partitionFacBits, synthetic as in partition.npz: int32 below 2^13"""
    return np.random.default_rng(BITS_SEED).integers(0, 1 << 13, mg.BITS_SHAPE).astype(np.int32)


def leaf_lists(geom):
    """-> (svt_hip_part_sb [NSB], svt_hip_part_leaf [nleaves], source groups [(src_first, nblocks, bsize)])"""
    rng = np.random.default_rng(0)                                          # (decides nothing: every square splits, every block is listed)
    sb, rows = np.zeros(NSB, mg.SB_DTYPE), []
    for i in range(NSB):
        ox, oy = 64 * (i % SB_COLS), 64 * (i // SB_COLS)
        r = mg.build_list(rng, geom, W, H, ox, oy, min_size=4, shapes=lambda rng, size, s, k: True)
        sb["leaf_first"][i], sb["leaf_count"][i], sb["origin_x"][i], sb["origin_y"][i] = len(rows), len(r), ox, oy
        rows += r
    lf = np.zeros(len(rows), mg.LEAF_DTYPE)
    for i, (mds, flag, tot, l, a) in enumerate(rows):
        lf["mds_idx"][i], lf["split_flag"][i], lf["tot_d1_blocks"][i], lf["left_partition"][i], lf["above_partition"][i] = mds, flag, tot, l, a
    bsize = geom["bsize"][lf["mds_idx"]]
    order = np.argsort(bsize, kind="stable")
    lf["src"][order] = np.arange(len(lf))
    groups, at = [], 0
    for b in np.unique(bsize).tolist():
        n = int((bsize == b).sum())
        groups.append((at, n, b))
        at += n
    return sb, lf, groups


def leaf_positions(geom, sb, leaf):
    """picture position of every src -> (x int64 [nsrc], y int64 [nsrc], bsize int64 [nsrc])"""
    which = np.repeat(np.arange(NSB), sb["leaf_count"].astype(np.int64))
    x, y, b = (np.zeros(len(leaf), np.int64) for _ in range(3))
    m = leaf["mds_idx"]
    x[leaf["src"]] = sb["origin_x"][which].astype(np.int64) + geom["origin_x"][m]
    y[leaf["src"]] = sb["origin_y"][which].astype(np.int64) + geom["origin_y"][m]
    b[leaf["src"]] = geom["bsize"][m]
    return x, y, b


def block_costs(src_y, geom, sb, leaf):
    """d_cost: uint64 [nsrc]"""
    x, y, b = leaf_positions(geom, sb, leaf)
    luma = src_y.astype(np.int64)
    cost = np.zeros(len(leaf), np.uint64)
    for s in range(len(leaf)):
        w, h = mr.BS_W[b[s]], mr.BS_H[b[s]]
        blk = luma[y[s]:y[s] + h, x[s]:x[s] + w]
        n = w * h
        cost[s] = COST_ACT * (int(np.abs(blk * n - blk.sum()).sum()) // n) + COST_BLOCK
    return cost


def partition_case(pics, geom):
    """the inputs of svt_hip_partition_decide_frame in make_golden_partition's case form, and the source groups"""
    sb, leaf, groups = leaf_lists(geom)
    case = dict(bits=partition_bits(), lam=np.uint32(LAMBDA), pic_width=np.uint32(W), pic_height=np.uint32(H), slice_is_intra=np.int32(0),
                sb=sb, leaf=leaf, cost=block_costs(pics["src"][0], geom, sb, leaf))
    return case, groups


def padded_final(final, count):
    """the concatenated list -> FINAL_DTYPE [NSB, 256] (zeros past each count)"""
    out, at = np.zeros((NSB, MAX_FINAL), FINAL_DTYPE), 0
    for sb, n in enumerate(count.tolist()):
        out[sb, :n] = final[at:at + n]
        at += n
    return out


def entries(final, count):
    """(sb, k, entry) of every live entry in coding order"""
    for sb in range(NSB):
        for k in range(int(count[sb])):
            yield sb, k, final[sb, k]


def cfl_allowed(bsize):
    return 8 <= mr.BS_W[bsize] <= 32 and 8 <= mr.BS_H[bsize] <= 32


def src_tables(final, count, pics, geom, rgeom, nsrc):
    """the per-src tables of the rule above -> dict(blk BLK_DTYPE [nsrc], decision DEC_DTYPE [nsrc] (all eobs 0), inter_mode uint8 [nsrc],
    listed bool [nsrc]); final: FINAL_DTYPE [NSB, 256]"""
    blk, inter_mode, listed = np.zeros(nsrc, BLK_DTYPE), np.zeros(nsrc, np.uint8), np.zeros(nsrc, bool)
    src_y, ref_y = pics["src"][0].astype(np.int64), pics["ref"][0].astype(np.int64)
    turn = {}
    sb_intra = []
    for sb in range(NSB):
        d = np.abs(src_y - ref_y)[64 * (sb // SB_COLS):64 * (sb // SB_COLS) + 64, 64 * (sb % SB_COLS):64 * (sb % SB_COLS) + 64]
        sb_intra.append(int(d.sum()) > SB_INTRA_SAD_PER_SAMPLE * d.size)
    for i, (sb, k, e) in enumerate(entries(final, count)):
        src, x, y, bsize, mds = int(e["src"]), int(e["x"]), int(e["y"]), int(e["bsize"]), int(e["mds_idx"])
        assert src < nsrc and not listed[src]
        listed[src] = True
        w, h = mr.BS_W[bsize], mr.BS_H[bsize]
        sad = int(np.abs(src_y[y:y + h, x:x + w] - ref_y[y:y + h, x:x + w]).sum())
        inter_mode[src] = GLOBALMV + (i & 1)
        if sad <= INTRA_SAD_PER_SAMPLE * w * h and not sb_intra[sb]:
            continue                                                        # an inter skip block: every other member 0
        tx, tx_uv = int(rgeom["txsize"][mds]), int(rgeom["txsize_uv"][mds])
        ty, tyu = mi.types_of(tx), mi.types_of(tx_uv)
        t = turn.get(tx, 0)
        turn[tx] = t + 1
        mode, delta = mi.LUMA_MODES[(i * 7 + bsize) % len(mi.LUMA_MODES)]
        uv = 13 if i % 3 == 0 and cfl_allowed(bsize) else (i * 5 + 3) % 13
        blk[src] = (1, mode, delta, uv, (i * 37 + 11) % 256, i % 8, ty[t % len(ty)], tyu[(t // 2 + i) % len(tyu)])
    return dict(blk=blk, decision=np.zeros(nsrc, DEC_DTYPE), inter_mode=inter_mode, listed=listed)


def skip_of(eob, has_uv):
    """update_av1_mi_map's skip (EbAdaptiveMotionVectorPrediction.c:1480-1483)"""
    return int(eob[0] == 0 and (not has_uv or (eob[1] == 0 and eob[2] == 0)))


def info_table(final, count, tabs, result, geom, nsrc):
    """svt_hip_dlf_info per src from the blk table and the intra pass's result rows (inter entries: eob 0) -> INFO_DTYPE [nsrc]"""
    info = np.zeros(nsrc, INFO_DTYPE)
    for sb, k, e in entries(final, count):
        src, b = int(e["src"]), tabs["blk"][int(e["src"])]
        has_uv = bool(geom["has_uv"][int(e["mds_idx"])])
        if b["is_intra"]:
            info[src] = (0, b["mode"], skip_of(result["eob"][sb, k], has_uv), 0)
        else:
            info[src] = (1, tabs["inter_mode"][src], 1, 0)
    return info


def mi_grid(final, count, info, rgeom):
    """the grid svt_hip_dlf_mi_frame scatters, as make_golden_dlf.draw_grid lays it out -> uint8 [H / 4, W / 4, 4]"""
    grid = np.zeros((H // 4, W // 4, 4), np.uint8)
    for sb, k, e in entries(final, count):
        x, y, bsize, r = int(e["x"]), int(e["y"]), int(e["bsize"]), info[int(e["src"])]
        grid[y // 4:(y + mr.BS_H[bsize]) // 4, x // 4:(x + mr.BS_W[bsize]) // 4] = (bsize, rgeom["txsize"][int(e["mds_idx"])], r["ref_frame0"] | r["skip"] << 7, r["mode"])
    return grid


def skip_map(grid):
    """the CDEF skip map of the grid: an 8x8 is skipped when all four of its 4x4 units are (is_8x8_block_skip, EbCdef.c:380-388)"""
    s = grid[:, :, 2] >> 7
    return np.ascontiguousarray((s[::2, ::2] & s[::2, 1::2] & s[1::2, ::2] & s[1::2, 1::2]).astype(np.uint8))


def in_planes(pics3):
    """three W x H pictures in zeroed [ROWS, STRIDE] planes"""
    out = []
    for p in range(3):
        a = np.zeros((ROWS >> (p > 0), STRIDE >> (p > 0)), np.uint8)
        a[:PH[p], :PW[p]] = pics3[p]
        out.append(a)
    return out


def block_masks(final, count, tabs, geom, rgeom):
    """(inter, intra): per plane bool [PH, PW] of the samples the inter / the intra entries cover"""
    inter, intra = [np.zeros((PH[p], PW[p]), bool) for p in range(3)], [np.zeros((PH[p], PW[p]), bool) for p in range(3)]
    for sb, k, e in entries(final, count):
        x, y, bsize, mds = int(e["x"]), int(e["y"]), int(e["bsize"]), int(e["mds_idx"])
        m = intra if tabs["blk"]["is_intra"][int(e["src"])] else inter
        m[0][y:y + mr.BS_H[bsize], x:x + mr.BS_W[bsize]] = True
        if geom["has_uv"][mds]:
            cx, cy, t = ((x >> 3) << 3) >> 1, ((y >> 3) << 3) >> 1, int(rgeom["txsize_uv"][mds])
            for p in (1, 2):
                m[p][cy:cy + mr.TX_H[t], cx:cx + mr.TX_W[t]] = True
    return inter, intra


def dlf_row(levels, sharp, delta=None):
    """a dlf_cases parameter row; delta: (ref_deltas, mode_deltas)"""
    rd, md = delta if delta else ((0,) * 8, (0, 0))
    return np.array([W, H, 8] + [int(v) for v in levels] + [int(sharp), int(delta is not None)] + list(rd) + list(md), np.int32)


def delta_of(levels):
    """the delta row's ref / mode deltas: LAST_FRAME loses the smallest picked level, so that in that plane a GLOBALMV block filters at
    level 0 next to NEWMV blocks (+4) and intra blocks (+5)"""
    return (5, -int(min(levels)), 0, 0, 0, 0, 0, 0), (0, 4)


# ---------------------------------------------------------------------------------------------------------------------------
# the fixture
# ---------------------------------------------------------------------------------------------------------------------------
PIC_CHAIN = (("rec", "src"), ("dlf", "rec"), ("dlfd", "rec"), ("cdef", "dlf"))      # a stage's picture is stored as its difference to `base`


def pack(g):
    """the dict as stored: pictures as int16 differences to the stage before, masks as bits, records as bytes"""
    d = {}
    for k, v in g.items():
        stage = next((s for s in PIC_CHAIN if k[:-1] == s[0] and k[-1] in "012"), None)
        if stage:
            base = g["src" + k[-1]] if stage[1] == "src" else g[stage[1] + k[-1]]
            d[f"{stage[0]}_diff_{k[-1]}"] = v.astype(np.int16) - base.astype(np.int16)
        elif k[:3] == "src" and k[-1] in "012" or k[:3] == "ref" and k[-1] in "012":
            continue                                                        # real_picture.npz holds them
        elif v.dtype == bool:
            d[k] = np.packbits(v)
        elif v.dtype.names:
            d[k] = v.view(np.uint8).reshape(v.shape + (v.dtype.itemsize,))
        else:
            d[k] = v
    return d


def load(path=FIXTURE):
    """the stored file -> dict: src0..2 / ref0..2 from real_picture.npz, rec / dlf / dlfd / cdef 0..2 restored, masks as bool, part_sq,
    part_final, result, info as records"""
    z = np.load(path)
    pics = pictures()
    assert np.array_equal(z["origin"], pics["origin"])
    g = {k: z[k] for k in z.files if "_diff_" not in k}
    for p in range(3):
        g[f"src{p}"], g[f"ref{p}"] = pics["src"][p], pics["ref"][p]
    for name, base in PIC_CHAIN:
        for p in range(3):
            g[f"{name}{p}"] = (z[f"{name}_diff_{p}"] + g[f"{base}{p}"].astype(np.int16)).astype(np.uint8)
    for p in range(3):
        for m in ("imask", "rmask"):
            g[f"{m}{p}"] = np.unpackbits(z[f"{m}{p}"])[:PH[p] * PW[p]].reshape(PH[p], PW[p]).astype(bool)
        g[f"qmask{p}"] = np.unpackbits(z[f"qmask{p}"])[:g[f"sbq{p}"].size].reshape(g[f"sbq{p}"].shape).astype(bool)
    g["resmask"] = np.unpackbits(z["resmask"])[:NSB * MAX_FINAL].reshape(NSB, MAX_FINAL).astype(bool)
    g["part_sq"] = z["part_sq"].view(mg.SQ_DTYPE).reshape(NSB, NSQ)
    g["part_final"] = z["part_final"].view(FINAL_DTYPE).reshape(-1)
    g["result"] = z["result"].view(RES_DTYPE).reshape(NSB, MAX_FINAL)
    g["info"] = z["info"].view(INFO_DTYPE).reshape(-1)
    return g


# ---------------------------------------------------------------------------------------------------------------------------
# coverage: what the fixture must hold for the chain to be able to go wrong on it
# ---------------------------------------------------------------------------------------------------------------------------
def measure(g, geom, rgeom):
    """-> {stat name: value} of a loaded (or freshly built) fixture dict"""
    final, count = padded_final(g["part_final"], g["part_count"]), g["part_count"]
    tabs = src_tables(final, count, dict(src=[g[f"src{p}"] for p in range(3)], ref=[g[f"ref{p}"] for p in range(3)]), geom, rgeom, int(g["nsrc"]))
    v = {}
    live = [(sb, k, e) for sb, k, e in entries(final, count)]
    sizes = {int(e["bsize"]) for _, _, e in live}
    nsq_depths = {int(geom["depth"][int(e["mds_idx"])]) for _, _, e in live if geom["shape"][int(e["mds_idx"])] != 0}
    v["final_entries"], v["block_sizes"], v["nsq_depths"] = len(live), len(sizes), len(nsq_depths)
    v["count_64x64"], v["count_4x4"] = sum(int(e["bsize"]) == 12 for _, _, e in live), sum(int(e["bsize"]) == 0 for _, _, e in live)
    v["max_sb_entries"] = int(count.max())
    intra = np.array([bool(tabs["blk"]["is_intra"][int(e["src"])]) for _, _, e in live])
    v["intra_share"] = float(intra.mean())
    # neighbours through a map of the owning entry per 4x4 unit
    owner = np.full((H // 4, W // 4), -1, np.int64)
    for i, (_, _, e) in enumerate(live):
        x, y, b = int(e["x"]), int(e["y"]), int(e["bsize"])
        owner[y // 4:(y + mr.BS_H[b]) // 4, x // 4:(x + mr.BS_W[b]) // 4] = i
    assert (owner >= 0).all()
    near = np.zeros((len(live), 2), bool)                                   # has an intra / an inter block above or to the left
    for i, (_, _, e) in enumerate(live):
        x, y, b = int(e["x"]) // 4, int(e["y"]) // 4, int(e["bsize"])
        others = set(owner[y - 1, x:x + mr.BS_W[b] // 4].tolist() if y else []) | set(owner[y:y + mr.BS_H[b] // 4, x - 1].tolist() if x else [])
        near[i] = (any(intra[j] for j in others), any(not intra[j] for j in others))
    v["intra_next_to_inter"], v["inter_next_to_intra"] = int((intra & near[:, 1]).sum()), int((~intra & near[:, 0]).sum())
    zero, coded = np.zeros(3, np.int64), np.zeros(3, np.int64)
    above, pos, neg = 0, 0, 0
    for i, (sb, k, e) in enumerate(live):
        if not intra[i]:
            continue
        b, eob = tabs["blk"][int(e["src"])], g["result"]["eob"][sb, k]
        for p in range(3 if geom["has_uv"][int(e["mds_idx"])] else 1):
            coded[p] += 1
            zero[p] += eob[p] == 0
        above += eob[0] > 10
        if b["uv_mode"] == 13:
            alphas = [mi.idx_to_alpha(int(b["cfl_alpha_idx"]), int(b["cfl_alpha_signs"]), pl) for pl in (0, 1)]
            pos, neg = pos + any(a > 0 for a in alphas), neg + any(a < 0 for a in alphas)
    for p, n in enumerate(PLANES):
        v[f"eob0_share_{n}"] = float(zero[p] / coded[p])
    v["luma_eob_above_10"], v["cfl_alpha_positive"], v["cfl_alpha_negative"] = int(above), int(pos), int(neg)
    levels, sharp = g["dlf_levels"][0], int(g["dlf_sharp"])
    row = dlf_row(levels, sharp)
    for cls, planes in (("luma", (0,)), ("chroma", (1, 2))):
        for d, dn in enumerate("vh"):
            units = [u for pl in planes for u in dc.edge_units(row, g["mi"], pl, d)]
            for length in ((4, 8, 14) if cls == "luma" else (4, 6)):
                v[f"edges_{cls}_{dn}_{length}"] = sum(u[2] == length for u in units)
    v["level_luma"], v["level_u"], v["level_v"] = int(levels[0]), int(levels[2]), int(levels[3])
    drow = dlf_row(levels, sharp, delta_of(levels))
    n = 0
    for pl in range(3):
        ss = 1 if pl else 0
        for d in range(2):
            for (x, y, length, level) in dc.edge_units(drow, g["mi"], pl, d):
                cur = g["mi"][ss | ((y << ss) >> 2), ss | ((x << ss) >> 2)]
                n += dc.unit_level(drow, pl, d, int(cur[2]) & 7, int(cur[3])) == 0
    v["delta_pv_level_units"] = n
    skip = skip_map(g["mi"])
    h8, w8 = skip.shape
    has = [bool(skip[8 * r:8 * r + 8, 8 * c:8 * c + 8].any()) for r in range((h8 + 7) // 8) for c in range((w8 + 7) // 8)]
    v["cdef_luma_strengths"] = len(set(int(s) for s in g["cdef_ystr"] if s >= 0))
    v["cdef_fbs_with_a_skip"], v["cdef_fbs_without_a_skip"] = sum(has), len(has) - sum(has)
    return v


def conditions(v):
    """-> {condition: met} over the measured values: the issue's coverage conditions"""
    return {
        "8 block sizes, non-square blocks at 2 tree levels": v["block_sizes"] >= 8 and v["nsq_depths"] >= 2,
        "64x64 and 4x4 blocks": v["count_64x64"] >= 1 and v["count_4x4"] >= 1,
        "a superblock with more than 40 entries": v["max_sb_entries"] > 40,
        "25 % .. 75 % intra": 0.25 <= v["intra_share"] <= 0.75,
        "20 intra next to inter and 20 inter next to intra": v["intra_next_to_inter"] >= 20 and v["inter_next_to_intra"] >= 20,
        "10 % .. 60 % eob 0 per plane": all(0.10 <= v[f"eob0_share_{n}"] <= 0.60 for n in PLANES),
        "20 luma blocks with eob above 10": v["luma_eob_above_10"] >= 20,
        "10 CfL blocks with each sign of alpha": v["cfl_alpha_positive"] >= 10 and v["cfl_alpha_negative"] >= 10,
        "MIN_COVER edges of every length": all(v[k] >= MIN_COVER for k in STAT_NAMES if k.startswith("edges_")),
        "luma level non-zero and unlike the chroma levels": v["level_luma"] != 0 and v["level_luma"] != v["level_u"] and v["level_luma"] != v["level_v"],
        "MIN_COVER units with curr_level 0 and pv_lvl non-zero": v["delta_pv_level_units"] >= MIN_COVER,
        "3 luma CDEF strengths": v["cdef_luma_strengths"] >= 3,
        "filter blocks with and without a skipped 8x8": v["cdef_fbs_with_a_skip"] >= 1 and v["cdef_fbs_without_a_skip"] >= 1,
    }

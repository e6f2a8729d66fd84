"""Writes tests/golden/recon_final.npz: the reconstruction of the final block list (AV1PerformInverseTransformRecon for the winner,
EbProductCodingLoop.c:871-1020) and the superblock coefficient stream, on synthetic tilings, predictions and sparse coefficients.

What is pinned to what.  Per plane block the REFERENCE's own av1_inv_transform_recon8bit runs in oracle/_ref/libsvtref.so through ctypes
(ref_inv_txfm_add_u8 with which = 2, oracle/ref_pins.c) on a copy of the prediction, or the prediction is copied (picture_copy8_bit) when
the record's eob is 0.  txsize / txsize_uv / has_uv / the chroma sides of every block are read from the reference's get_blk_geom_mds after
build_blk_geom(0) and recorded as data.  GLUE, written here: the walk over the entries, the four skip rules of the call, the chroma
position (:905-906) and the running stream offsets (coded_area_sb / coded_area_sb_uv, EbCodingLoop.c:3033-3035, :3376-3378).  The final
lists are built here as valid tilings of the superblock from a tree of partitions and the md-scan offsets; no kernel takes part.

The coverage the issue lists does not fit one 128x128 picture: every (luma size, type) pair alone needs 27 904 luma samples, four
superblocks hold 16 384.  The main case is therefore THREE 128x128 pictures of 2x2 superblocks (main0 .. main2), which between them hold
the whole list (check_coverage).  `skips` is a 96x80 picture held in 128x128 planes with an entry for each skip reason; `combined` gives
every superblock of the four to one call, the pictures side by side in one plane (only its outputs are stored).

Expected outputs come with masks: a plane sample, a stream element, a status byte or an offset that is not in its mask must keep whatever
the caller had there.

CPU only; run from the repository root after build():  python tests/golden/make_golden_recon_final.py
"""
import ctypes
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, HERE)
import svtlibs  # noqa: E402
import make_golden_partition as mg  # noqa: E402
from make_golden_md_decide import DEC_DTYPE  # noqa: E402

OUT = os.path.join(HERE, "recon_final.npz")
NO_SRC, MAX_FINAL, NBLK = mg.NO_SRC, mg.MAX_FINAL, mg.NBLK
FINAL_DTYPE = mg.FINAL_DTYPE
OK, R_NO_SRC, R_BSIZE, R_OUTSIDE, R_TX_TYPE = 0, 1, 2, 3, 4
SPAN = (4096, 1024, 1024)
BS_W = (4, 4, 8, 8, 8, 16, 16, 16, 32, 32, 32, 64, 64, 64, 128, 128, 4, 16, 8, 32, 16, 64)
BS_H = (4, 8, 4, 8, 16, 8, 16, 32, 16, 32, 64, 32, 64, 128, 64, 128, 16, 4, 32, 8, 64, 16)
TX_W, TX_H = svtlibs.TX_W, svtlibs.TX_H
NONE, HORZ, VERT, HA, HB, VA, VB, H4, V4 = 0, 1, 2, 4, 5, 6, 7, 8, 9
# BlockGeom members (bytes): the partition generator's, and the transform sizes
RGEOM_FIELDS = dict(depth=(0, 1), shape=(1, 1), origin_x=(2, 1), origin_y=(3, 1), bwidth=(10, 1), bheight=(11, 1), bwidth_uv=(12, 1), bheight_uv=(13, 1),
                    bsize=(16, 1), txsize=(20, 1), txsize_uv=(24, 1), tx_width=(60, 1), tx_height=(64, 1), tx_width_uv=(68, 1), tx_height_uv=(72, 1),
                    has_uv=(80, 4))
RGEOM_DTYPE = np.dtype([(n, "u1") for n in RGEOM_FIELDS])
CASE_NAMES = ("main0", "main1", "main2", "skips")
MAIN = (0, 1, 2)
NCASES = len(CASE_NAMES)
COMBINED = NCASES
ALL_NAMES = CASE_NAMES + ("combined",)
INPUT_KEYS = ("width", "height", "stride", "rows", "final", "count", "decision", "groups", "pred0", "pred1", "pred2", "dq0", "dq1", "dq2", "q0", "q1", "q2")
OUTPUT_KEYS = ("recon0", "recon1", "recon2", "rmask0", "rmask1", "rmask2", "status", "offset", "sbq0", "sbq1", "sbq2", "qmask0", "qmask1", "qmask2")


# ---------------------------------------------------------------------------------------------------------------------------
# the reference
# ---------------------------------------------------------------------------------------------------------------------------
def ref_geometry(L):
    """get_blk_geom_mds for all 1 101 blocks -> RGEOM_DTYPE [1101]"""
    g = np.zeros(NBLK, RGEOM_DTYPE)
    for i in range(NBLK):
        raw = np.ctypeslib.as_array(ctypes.cast(L.get_blk_geom_mds(i), ctypes.POINTER(ctypes.c_uint8)), shape=(mg.SIZEOF_GEOM,))
        for name, (at, nbytes) in RGEOM_FIELDS.items():
            g[name][i] = int.from_bytes(raw[at:at + nbytes].tobytes(), "little")
    # the members read are the ones meant: a transform size's sides are the block's, the chroma block's at most 32
    for i in range(NBLK):
        r = g[i]
        assert (TX_W[r["txsize"]], TX_H[r["txsize"]]) == (r["tx_width"], r["tx_height"]) == (r["bwidth"], r["bheight"]) == (BS_W[r["bsize"]], BS_H[r["bsize"]]), i
        assert (TX_W[r["txsize_uv"]], TX_H[r["txsize_uv"]]) == (r["tx_width_uv"], r["tx_height_uv"]) == (min(r["bwidth_uv"], 32), min(r["bheight_uv"], 32)), i
        assert (r["bwidth_uv"], r["bheight_uv"]) == (max(r["bwidth"] // 2, 4), max(r["bheight"] // 2, 4)), i
    return g


def ref_inverse(L):
    """av1_inv_transform_recon8bit on a dense block -> inv(dq int32 [nc], blk uint8 [h, w], tx_type, tx_size, eob)"""
    L.ref_inv_txfm_add_u8.restype = None
    L.ref_inv_txfm_add_u8.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int32] + [ctypes.c_int] * 4

    def inv(dq, blk, tx_type, tx_size, eob):
        buf = np.zeros(TX_W[tx_size] * TX_H[tx_size], np.int32)              # the reference's coefficient buffer is the whole block's
        buf[:len(dq)] = dq
        L.ref_inv_txfm_add_u8(buf.ctypes.data, blk.ctypes.data, blk.shape[1], int(tx_type), int(tx_size), int(eob), 2)
    return inv


def oracle_inverse():
    """the CPU checker's inverse, the same signature (it takes no eob)"""
    O = svtlibs.oracle()

    def inv(dq, blk, tx_type, tx_size, eob):
        buf = np.ascontiguousarray(dq, np.int32)
        O.svt_oracle_inv_txfm2d_add_u8(svtlibs.ptr(buf), svtlibs.ptr(blk), blk.shape[1], int(tx_type), int(tx_size))
    return inv


# ---------------------------------------------------------------------------------------------------------------------------
# tables from the recorded geometry
# ---------------------------------------------------------------------------------------------------------------------------
def bsize_tables(geom):
    """-> {bsize: (txsize, txsize_uv, cw, ch)} for the 19 block sizes of a 64x64 superblock"""
    t = {}
    for r in geom:
        v = (int(r["txsize"]), int(r["txsize_uv"]), int(r["bwidth_uv"]), int(r["bheight_uv"]))
        assert t.setdefault(int(r["bsize"]), v) == v
    assert len(t) == 19
    return t


def types_of(tx_size):
    return [t for t in range(16) if svtlibs.txfm_allowed(tx_size, t)]


def uv_type(bsize, half, tabs):
    """the chroma transform type of a source group: a function of the block size and of which half of a split size it is"""
    ty = types_of(tabs[bsize][1])
    return ty[(bsize * 5 + half * 3 + 1) % len(ty)]


def tile(tree, mds=0, depth=0):
    """a tree of partitions (a part, or a list of four subtrees for PARTITION_SPLIT) -> [(mds, part)] in coding order"""
    if isinstance(tree, (list, tuple)):
        out = []
        for k, sub in enumerate(tree):
            out += tile(sub, mds + mg.D1_DEPTH_OFFSET[depth] + k * mg.NS_DEPTH_OFFSET[depth + 1], depth + 1)
        return out
    return [(mds + mg.NS_BLK_OFFSET[tree] + i, tree) for i in range(mg.NS_BLK_NUM[tree])]


S = lambda x: [x] * 4
SB_4X4 = S(S(S(S(NONE))))                                                     # 256 4x4
SB_64 = NONE
SB_32S = [NONE, NONE, HORZ, VERT]                                             # 32x32 twice, 32x16, 16x32
SB_F = [H4, V4, S(HORZ), S(HORZ)]                                             # 32x8, 8x32, sixteen 16x8
SB_16 = S(S(NONE))                                                            # sixteen 16x16
SB_H = [S(VERT), S(VERT), S(H4), S(V4)]                                       # sixteen 8x16, 16x4, 4x16
SB_I = [S(S(NONE)), [S(HORZ), S(HORZ), S(VERT), S(VERT)], [HA, HB, VA, VB], [S(NONE), NONE, NONE, NONE]]      # 8x8, 8x4, 4x8, the mixed shapes
PICTURES = {"main0": [SB_4X4, SB_64, None, SB_32S], "main1": [HORZ, VERT, SB_F, SB_16], "main2": [H4, V4, SB_H, SB_I]}
ORIGINS = [(0, 0), (64, 0), (0, 64), (64, 64)]


# ---------------------------------------------------------------------------------------------------------------------------
# the cases
# ---------------------------------------------------------------------------------------------------------------------------
def coefficients(rng, tx_size, tx_type, zero, big):
    """sparse coefficients with a true eob -> (q int32 [nc], dq int32 [nc], eob); zero: a pattern that must not be read, eob 0"""
    nc = min(TX_W[tx_size], 32) * min(TX_H[tx_size], 32)
    if zero:
        return np.full(nc, 0x00777777, np.int32), np.full(nc, 0x00333333, np.int32), 0
    scan = svtlibs.scan_tables(tx_size, tx_type)[0]
    assert len(scan) == nc
    eob = int(rng.integers(1, max(2, nc // 3 + 1)))
    at = np.unique(np.concatenate([[eob - 1], rng.integers(0, eob, min(eob, 6))]))
    q = np.zeros(nc, np.int32)
    q[scan[at]] = rng.integers(1, 13, len(at)) * rng.choice([-1, 1], len(at))
    if at[0] == 0:
        q[scan[0]] = int(rng.integers(1, 41 if not big else 200)) * int(rng.choice([-1, 1]))
    step = int(rng.integers(8, 56))
    return q, q * step, eob


def build_case(name, geom, tabs, sbs, dims, seed, skip_script=None):
    """sbs: [(origin_x, origin_y, [(mds, part)])]; dims: (width, height, stride, rows) of luma (chroma: halves).  Every entry gets a record;
    records are grouped by block size into source groups (8x8 and 16x16 in two groups each with chroma types of their own, an empty group
    between); skip_script(entries, records) edits entries for the skip case.  -> the case dict"""
    rng = np.random.default_rng(seed)
    entries = []                                                             # (sb, k, mds, x, y, bsize, part)
    for i, (ox, oy, blocks) in enumerate(sbs):
        for k, (mds, part) in enumerate(blocks):
            g = geom[mds]
            entries.append([i, k, mds, ox + int(g["origin_x"]), oy + int(g["origin_y"]), int(g["bsize"]), part])
    n = len(entries)
    # the source groups: entries by block size, shuffled inside a size
    by_bsize = {}
    for e, ent in enumerate(entries):
        by_bsize.setdefault(ent[5], []).append(e)
    order = list(by_bsize)
    rng.shuffle(order)
    groups, src_of, next_src = [], np.zeros(n, np.int64), 0
    for bsize in order:
        members = [by_bsize[bsize][j] for j in rng.permutation(len(by_bsize[bsize]))]
        halves = [members[:len(members) // 2], members[len(members) // 2:]] if bsize in (3, 6) and len(members) > 1 else [members]
        for half, mem in enumerate(halves):
            groups.append((next_src, len(mem), bsize, uv_type(bsize, half, tabs)))
            for local, e in enumerate(mem):
                src_of[e] = next_src + local
            next_src += len(mem)
        if len(groups) >= 3 and not any(nb == 0 for _, nb, _, _ in groups):
            groups.append((next_src, 0, 9, 0))                               # an empty group
    nsrc = next_src
    dec = np.zeros(nsrc, DEC_DTYPE)
    i = np.arange(nsrc)
    dec["cost"], dec["cost_luma"], dec["full_lambda_rate"], dec["full_distortion"], dec["slot"], dec["cand"] = i * 13 + 5, i * 3 + 1, i * 7 + 2, i * 11 + 3, i % 40, i % 64
    # types: every (size, type) pair in turn; eob masks
    turn = {}
    zero = np.zeros((n, 3), bool)
    for e, (sb, k, mds, x, y, bsize, part) in enumerate(entries):
        if name == "main0" and sb == 0:                                      # the 4x4 superblock: luma eob 0 every seventh, chroma in turns
            zero[e] = (k % 7 == 3, (k // 4) % 5 == 1, (k // 4) % 5 == 2)
        if name == "main2" and sb == 3 and len(sbs[sb][2]) - k <= 7:         # the last seven blocks of the mixed superblock: masks 1 .. 7
            m = len(sbs[sb][2]) - k
            zero[e] = (m & 1, m >> 1 & 1, m >> 2 & 1)
        ty = types_of(tabs[bsize][0])
        t = turn.get(bsize, 0)
        dec["tx_type"][src_of[e]] = ty[t % len(ty)]
        if not zero[e, 0]:
            turn[bsize] = t + 1
    final = np.zeros((len(sbs), MAX_FINAL), FINAL_DTYPE)
    count = np.zeros(len(sbs), np.uint32)
    for e, (sb, k, mds, x, y, bsize, part) in enumerate(entries):
        final[sb, k] = (mds, x, y, bsize, part, src_of[e])
        count[sb] = max(count[sb], k + 1)
    if skip_script:
        skip_script(entries, final, dec, src_of, groups, nsrc)
    for sb in range(len(sbs)):                                               # past the count: an entry that would write if it were read
        final[sb, count[sb]:] = final[sb, 0] if count[sb] else (0, sbs[sb][0], sbs[sb][1], 12, 0, 0)
    # the winners' arrays, group by group
    arrays = {k: [] for k in ("pred0", "pred1", "pred2", "dq0", "dq1", "dq2", "q0", "q1", "q2")}
    entry_of = {int(src_of[e]): e for e in range(n)}
    for first, nb, bsize, uvt in groups:
        tx, tx_uv, cw, ch = tabs[bsize]
        for local in range(nb):
            src = first + local
            e = entry_of[src]
            for p in range(3):
                w, h, t, ty = (BS_W[bsize], BS_H[bsize], tx, int(dec["tx_type"][src])) if p == 0 else (cw, ch, tx_uv, uvt)
                q, dq, eob = coefficients(rng, t, ty, bool(zero[e, p]), big=(src % 5 == 0))
                dec["eob"][src, p] = eob
                arrays[f"pred{p}"].append(rng.integers(0, 256, w * h).astype(np.uint8))
                arrays[f"dq{p}"].append(dq)
                arrays[f"q{p}"].append(q)
    dec["y_has_coeff"], dec["u_has_coeff"], dec["v_has_coeff"] = dec["eob"][:, 0] != 0, dec["eob"][:, 1] != 0, dec["eob"][:, 2] != 0
    dec["block_has_coeff"] = (dec["eob"] != 0).any(axis=1)
    width, height, stride, rows = dims
    c = dict(width=np.array([width, width // 2, width // 2], np.uint32), height=np.array([height, height // 2, height // 2], np.uint32),
             stride=np.array([stride, stride // 2, stride // 2], np.uint32), rows=np.array([rows, rows // 2, rows // 2], np.uint32),
             final=final, count=count, decision=dec, groups=np.array(groups, np.int32).reshape(-1, 4))
    for k, v in arrays.items():
        c[k] = np.concatenate(v) if v else np.zeros(0, np.uint8 if k.startswith("pred") else np.int32)
    return c


def skip_sbs(geom):
    """the skip case's tilings: a 96x80 picture; what pokes out is still listed"""
    q0_16 = [S(NONE), NONE, NONE, NONE]
    return [(0, 0, tile(HORZ)), (64, 0, tile(q0_16)), (0, 64, tile(NONE)), (64, 64, tile(q0_16))]


def skip_script(entries, final, dec, src_of, groups, nsrc):
    """edits the skip case: SB 0 the second 64x32 with IDTX (4); SB 1 the 16x16s: fine, NO_SRC (1), src >= nsrc (1), a src of another block
    size (2), then 32x32 outside (3), 32x32 with ADST_DCT (4), outside (3); SB 2 a 64x64 past the bottom (3) whatever its type; SB 3 the
    16x16s: fine, tx_type 16 (4), two outside (3), then three 32x32 outside"""
    at = {(sb, k): e for e, (sb, k, *_) in enumerate(entries)}
    dec["tx_type"][src_of[at[0, 0]]], dec["tx_type"][src_of[at[0, 1]]] = 0, 9
    dec["tx_type"][src_of[at[1, 0]]] = 7
    final["src"][1, 1], final["src"][1, 2] = NO_SRC, nsrc + 7
    other = [first for first, nb, bsize, _ in groups if bsize == 9 and nb][0]      # a 32x32 record for a 16x16 entry
    final["src"][1, 3] = other
    dec["tx_type"][src_of[at[1, 5]]] = 1
    dec["tx_type"][src_of[at[2, 0]]] = 9
    dec["tx_type"][src_of[at[3, 0]]], dec["tx_type"][src_of[at[3, 1]]] = 12, 16


def case_groups(c, tabs):
    """the case's source groups as dicts with their arrays split out of the flat ones"""
    at = {k: 0 for k in ("pred0", "pred1", "pred2", "dq0", "dq1", "dq2", "q0", "q1", "q2")}
    out = []
    for first, nb, bsize, uvt in c["groups"].tolist():
        tx, tx_uv, cw, ch = tabs[bsize]
        g = dict(src_first=first, nblocks=nb, bsize=bsize, tx_type_uv=uvt, pred=[], dq=[], q=[])
        for p in range(3):
            w, h, t = (BS_W[bsize], BS_H[bsize], tx) if p == 0 else (cw, ch, tx_uv)
            nc = min(w, 32) * min(h, 32)
            g["pred"].append(c[f"pred{p}"][at[f"pred{p}"]:at[f"pred{p}"] + nb * w * h].reshape(nb, h, w)); at[f"pred{p}"] += nb * w * h
            for key in ("dq", "q"):
                g[key].append(c[f"{key}{p}"][at[f"{key}{p}"]:at[f"{key}{p}"] + nb * nc].reshape(nb, nc)); at[f"{key}{p}"] += nb * nc
        out.append(g)
    return out


def combined_case(cases, tabs):
    """every superblock of the given cases in one call: picture i moved 128 samples to the right of picture i - 1, one plane of 480 x 128
    (the last picture is 96 wide), stride 512; the source groups of one block size and chroma type merged, the empty ones dropped"""
    finals, counts, decs, merged, order = [], [], [], {}, []
    src_map, next_src = [], 0
    for i, c in enumerate(cases):                                            # first pass: where every record goes
        for g in case_groups(c, tabs):
            key = (g["bsize"], g["tx_type_uv"])
            if g["nblocks"] and key not in merged:
                merged[key] = []
                order.append(key)
            if g["nblocks"]:
                merged[key].append((i, g))
    starts = {}
    for key in order:
        starts[key] = next_src
        next_src += sum(g["nblocks"] for _, g in merged[key])
    maps = [np.zeros(len(c["decision"]), np.int64) for c in cases]
    fill = dict(starts)
    for key in order:
        for i, g in merged[key]:
            maps[i][g["src_first"]:g["src_first"] + g["nblocks"]] = fill[key] + np.arange(g["nblocks"])
            fill[key] += g["nblocks"]
    dec = np.zeros(next_src, DEC_DTYPE)
    for i, c in enumerate(cases):
        dec[maps[i]] = c["decision"]
        f = c["final"].copy()
        f["x"] += 128 * i
        ok = f["src"] < len(c["decision"])
        f["src"] = np.where(ok, maps[i][np.minimum(f["src"], len(c["decision"]) - 1)], np.where(f["src"] == NO_SRC, NO_SRC, next_src + 7)).astype(np.uint32)
        finals.append(f); counts.append(c["count"])
    out = dict(width=np.array([480, 240, 240], np.uint32), height=np.array([128, 64, 64], np.uint32), stride=np.array([512, 256, 256], np.uint32),
               rows=np.array([128, 64, 64], np.uint32), final=np.concatenate(finals), count=np.concatenate(counts), decision=dec,
               groups=np.array([(starts[k], sum(g["nblocks"] for _, g in merged[k]), k[0], k[1]) for k in order], np.int32).reshape(-1, 4))
    for p in range(3):
        for key, name in (("pred", "pred"), ("dq", "dq"), ("q", "q")):
            out[f"{name}{p}"] = np.concatenate([g[key][p].reshape(-1) for k in order for _, g in merged[k]])
    return out


# ---------------------------------------------------------------------------------------------------------------------------
# the model: the glue around the inverse
# ---------------------------------------------------------------------------------------------------------------------------
def model(c, geom, tabs, inv, planes=3):
    """svt_hip_recon_final_frame for a case -> dict of OUTPUT_KEYS (recon / sbq of planes not asked for: all masked out)"""
    nsb, nsrc = len(c["count"]), len(c["decision"])
    groups, dec = case_groups(c, tabs), c["decision"]
    recon = [np.zeros((int(c["rows"][p]), int(c["stride"][p])), np.uint8) for p in range(3)]
    rmask = [np.zeros(r.shape, bool) for r in recon]
    sbq = [np.zeros((nsb, SPAN[p]), np.int32) for p in range(3)]
    qmask = [np.zeros(s.shape, bool) for s in sbq]
    status, offset = np.zeros((nsb, MAX_FINAL), np.uint8), np.zeros((nsb, MAX_FINAL, 2), np.uint32)
    for sb in range(nsb):
        run = [0, 0]
        for k in range(min(int(c["count"][sb]), MAX_FINAL)):
            e = c["final"][sb, k]
            offset[sb, k] = run
            src, bsize, x, y = int(e["src"]), int(e["bsize"]), int(e["x"]), int(e["y"])
            g = geom[min(int(e["mds_idx"]), NBLK - 1)]
            reason, grp = OK, None
            if src == NO_SRC or src >= nsrc:
                reason = R_NO_SRC
            else:
                grp = [G for G in groups if G["src_first"] <= src < G["src_first"] + G["nblocks"]][0]
                if grp["bsize"] != bsize:
                    reason = R_BSIZE
            if reason == OK:
                tx, tx_uv, cw, ch = tabs[bsize]
                bw, bh, has_uv = BS_W[bsize], BS_H[bsize], bool(g["has_uv"])
                cx, cy = ((x >> 3) << 3) >> 1, ((y >> 3) << 3) >> 1
                inside = x + bw <= c["width"][0] and y + bh <= c["height"][0]
                if planes == 3 and has_uv:
                    inside = inside and all(cx + cw <= c["width"][p] and cy + ch <= c["height"][p] for p in (1, 2))
                if not inside:
                    reason = R_OUTSIDE
            if reason == OK and not svtlibs.txfm_allowed(tx, int(dec["tx_type"][src])) or reason == OK and int(dec["tx_type"][src]) > 15:
                reason = R_TX_TYPE
            status[sb, k] = reason
            if reason != OK:
                continue
            local = src - grp["src_first"]
            for p in range(planes):
                if p and not has_uv:
                    continue
                w, h, t, ty, x0, y0 = (bw, bh, tx, int(dec["tx_type"][src]), x, y) if p == 0 else (cw, ch, tx_uv, grp["tx_type_uv"], cx, cy)
                blk = grp["pred"][p][local].copy()
                eob = int(dec["eob"][src, p])
                if eob:
                    inv(grp["dq"][p][local].copy(), blk, ty, t, eob)
                recon[p][y0:y0 + h, x0:x0 + w] = blk
                rmask[p][y0:y0 + h, x0:x0 + w] = True
                off, nc = run[0 if p == 0 else 1], min(w, 32) * min(h, 32)
                if off + w * h <= SPAN[p]:
                    sbq[p][sb, off:off + nc] = grp["q"][p][local] if eob else 0
                    qmask[p][sb, off:off + nc] = True
            run[0] += bw * bh
            if has_uv:
                run[1] += cw * ch
    out = dict(status=status, offset=offset)
    for p in range(3):
        out[f"recon{p}"], out[f"rmask{p}"], out[f"sbq{p}"], out[f"qmask{p}"] = recon[p], rmask[p], sbq[p], qmask[p]
    return out


# ---------------------------------------------------------------------------------------------------------------------------
def make_cases(geom, tabs):
    """-> [(name, case dict)] without the combined one"""
    cases = []
    for i, name in enumerate(CASE_NAMES[:3]):
        sbs = [(ox, oy, tile(tree) if tree is not None else []) for (ox, oy), tree in zip(ORIGINS, PICTURES[name])]
        cases.append((name, build_case(name, geom, tabs, sbs, (128, 128, 136, 128), 2000 + i)))
    cases.append(("skips", build_case("skips", geom, tabs, skip_sbs(geom), (96, 80, 128, 128), 2003, skip_script)))
    return cases


def check_coverage(cases, outs, geom, tabs):
    """the list of the issue, over the main pictures together; the skip reasons in the skip case"""
    pairs, bsizes, zero_masks, no_uv, counts = set(), set(), set(), False, []
    mixed4 = mixed8 = False
    for (name, c), o in zip(cases, outs):
        if name == "skips":
            assert set(o["status"][np.arange(MAX_FINAL)[None] < c["count"][:, None]].tolist()) == {0, 1, 2, 3, 4}, name
            assert ((c["final"]["src"] == NO_SRC) & (o["status"] == 1)).any() and ((c["final"]["src"] != NO_SRC) & (o["status"] == 1)).any()
            continue
        assert (o["status"] == 0).all(), name
        counts += c["count"].tolist()
        for sb in range(len(c["count"])):
            ent = c["final"][sb, :c["count"][sb]]
            ty = c["decision"]["tx_type"][ent["src"]]
            eob = c["decision"]["eob"][ent["src"]]
            for b, t, e, m in zip(ent["bsize"].tolist(), ty.tolist(), eob.tolist(), ent["mds_idx"].tolist()):
                bsizes.add(b)
                if e[0]:
                    pairs.add((tabs[b][0], t))
                if geom["has_uv"][m]:
                    zero_masks.add((e[0] == 0) + 2 * (e[1] == 0) + 4 * (e[2] == 0))
                else:
                    no_uv = True
            for b, flag in ((0, "m4"), (3, "m8")):
                run = (ent["bsize"][:-1] == b) & (ent["bsize"][1:] == b) & (ty[:-1] != ty[1:]) & (eob[:-1, 0] != 0) & (eob[1:, 0] != 0)
                if run.any():
                    mixed4, mixed8 = mixed4 or b == 0, mixed8 or b == 3
    assert len(bsizes) == 19, sorted(bsizes)
    want = {(t, ty) for t in range(19) for ty in types_of(t)}
    assert pairs == want, sorted(want - pairs)
    assert zero_masks == set(range(8)), zero_masks
    assert no_uv and mixed4 and mixed8
    assert 256 in counts and 1 in counts and 0 in counts, counts


def load_case(z, k, tabs=None):
    """case k of the fixture -> (inputs dict, outputs dict with boolean masks)"""
    tabs = tabs or bsize_tables(load_geometry(z))
    if k == COMBINED:
        c = combined_case([load_case(z, j, tabs)[0] for j in range(NCASES)], tabs)
    else:
        c = {key: z[f"c{k}_{key}"] for key in INPUT_KEYS}
        c["final"], c["decision"] = c["final"].view(FINAL_DTYPE).reshape(-1, MAX_FINAL), c["decision"].view(DEC_DTYPE).reshape(-1)
    o = {}
    for key in OUTPUT_KEYS:
        v = z[f"c{k}_{key}"]
        if "mask" in key:
            like = z[f"c{k}_{'recon' if key[0] == 'r' else 'sbq'}{key[-1]}"]
            v = np.unpackbits(v)[:like.size].reshape(like.shape).astype(bool)
        o[key] = v
    return c, o


def load_geometry(z):
    return z["geom"].view(RGEOM_DTYPE).reshape(-1)


def stored(c, o, with_inputs):
    """the arrays of a case as the file holds them"""
    out = {}
    for key in INPUT_KEYS if with_inputs else ():
        v = c[key]
        out[key] = v.view(np.uint8).reshape(v.shape + (v.dtype.itemsize,)) if v.dtype.names else v
    for key in OUTPUT_KEYS:
        out[key] = np.packbits(o[key]) if "mask" in key else o[key]
    return out


def build_all(L):
    """-> the dict the file holds"""
    geom = ref_geometry(L)
    tabs = bsize_tables(geom)
    inv = ref_inverse(L)
    out = {"geom": geom.view(np.uint8).reshape(NBLK, RGEOM_DTYPE.itemsize), "names": np.array(CASE_NAMES)}
    cases = make_cases(geom, tabs)
    outs = [model(c, geom, tabs, inv) for _, c in cases]
    check_coverage(cases, outs, geom, tabs)
    cases.append(("combined", combined_case([c for _, c in cases], tabs)))
    outs.append(model(cases[-1][1], geom, tabs, inv))
    assert len(cases[-1][1]["groups"]) <= 32 and all(len(c["groups"]) <= 32 for _, c in cases)
    for k, ((name, c), o) in enumerate(zip(cases, outs)):
        luma = model(c, geom, tabs, inv, planes=1)                           # a luma-only call: the same status, offsets and luma
        assert all(np.array_equal(luma[key], o[key]) for key in ("status", "offset", "recon0", "rmask0", "sbq0", "qmask0")), name
        for key, v in stored(c, o, k < NCASES).items():
            out[f"c{k}_{key}"] = v
        print(f"{name}: {len(c['count'])} superblocks, counts {c['count'].tolist()}, {len(c['decision'])} records, {len(c['groups'])} groups")
    return out


def main():
    L = mg.ref_lib()
    if L is None:
        raise SystemExit("oracle/_ref/libsvtref.so is not built")
    np.savez_compressed(OUT, **build_all(L))
    print(f"wrote {OUT}: {os.path.getsize(OUT)} bytes")


if __name__ == "__main__":
    main()

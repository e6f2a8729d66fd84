"""Writes tests/golden/intra_encode.npz: the intra encode pass in coding order (EbCodingLoop.c:2853-3005 with Av1EncodeLoop :545-980 and
Av1EncodeGenerateRecon :1408-1500) on synthetic pictures, for svt_hip_intra_encode_frame.

What is pinned to what.  Per coded block and plane the REFERENCE's own leaves run in oracle/_ref/libsvtref.so through ctypes:
ref_predict_intra_block (av1_predict_intra_block at ED_STAGE with has_top_right / has_bottom_left / get_filt_type / build_intra_predictors,
oracle/ref_intra.c), ref_estimate_transform, aom_highbd_quantize_b{,_32x32,_64x64}_avx2 with the scans of ref_get_scan,
ref_inv_txfm_add_u8 (av1_inv_transform_recon8bit), cfl_luma_subsampling_420_lbd_c, subtract_average_c and cfl_predict_lbd_c.  The quantiser
rows are rows of av1_build_quantizer's y tables.
GLUE, written here and mirrored from the lines cited above: the walk over the superblocks and their entries in coding order; the line
buffers the reference predicts from (topArray / leftArray / topLeftArray of its recon neighbour arrays, :2863-2893 and
EncodePassUpdateReconSampleNeighborArrays), updated after every entry from what the plane holds; the mode-info grid, filled for coded
blocks only (a block the call does not code counts as not smooth); the rules of the call for entries that are not coded; the chroma
position; UV_DC_PRED under UV_CFL_PRED (:2896); cfl_idx_to_alpha; the luma type DCT_DCT at eob 0 (:700-709); the running stream offsets.
The final lists are partition trees of the 64x64 superblock in md-scan order (make_golden_recon_final.tile); no kernel takes part.

Cases (one call each): cover0, cover1: two 128x128 pictures each (npics 2), between them every block size, partition shape, luma mode with
deltas -3 / 0 / 3, chroma mode, CfL with both signs and every transform type; edges: 176x144 in 3x3 superblocks; sb4, sb64: one
superblock of 256 4x4 entries, one 64x64; inter: half the entries is_intra 0 over prefilled samples; refuse: one entry per status.
Expected outputs come with masks: what is not in its mask must keep whatever the caller had there.

CPU only; run from the repository root after build():  python tests/golden/make_golden_intra_encode.py
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
import make_golden_recon_final as mr  # noqa: E402

OUT = os.path.join(HERE, "intra_encode.npz")
NO_SRC, MAX_FINAL, NBLK, FINAL_DTYPE = mg.NO_SRC, mg.MAX_FINAL, mg.NBLK, mg.FINAL_DTYPE
OK, R_NO_SRC, R_OUTSIDE, R_TX_TYPE, R_NOT_INTRA, R_MODE, R_CFL_SIZE, R_SCHEDULE = 0, 1, 3, 4, 5, 6, 7, 8
BLK_DTYPE = np.dtype([("is_intra", "u1"), ("mode", "u1"), ("angle_delta", "i1"), ("uv_mode", "u1"), ("cfl_alpha_idx", "u1"), ("cfl_alpha_signs", "u1"),
                      ("tx_type", "u1"), ("tx_type_uv", "u1")])
RES_DTYPE = np.dtype([("eob", "<u2", (3,)), ("tx_type", "u1"), ("pad", "u1")])
SPAN = (4096, 1024, 1024)
BS_W, BS_H, TX_W, TX_H = mr.BS_W, mr.BS_H, svtlibs.TX_W, svtlibs.TX_H
NONE, HORZ, VERT, HA, HB, VA, VB, H4, V4 = mr.NONE, mr.HORZ, mr.VERT, mr.HA, mr.HB, mr.VA, mr.VB, mr.H4, mr.V4
SHAPE_OF_PART = {0: 0, 1: 1, 2: 2, 4: 3, 5: 4, 6: 5, 7: 6, 8: 7, 9: 8}
S = mr.S
CASE_NAMES = ("cover0", "cover1", "edges", "sb4", "sb64", "inter", "refuse")
COVER = (0, 1)
ALL_OK = (0, 1, 2, 3, 4)
INPUT_KEYS = ("dims", "final", "count", "blk", "src0", "src1", "src2", "init0", "init1", "init2", "qrows")
OUTPUT_KEYS = ("recon0", "recon1", "recon2", "rmask0", "rmask1", "rmask2", "status", "result", "resmask", "offset", "sbq0", "sbq1", "sbq2", "qmask0", "qmask1", "qmask2")
QKEYS = ("zbin", "round", "quant", "quant_shift", "dequant")
QINDEX = (255, 220)                                                          # luma, chroma rows

# the trees of the coverage pictures
MIX_A = [S(S(NONE)), [S(HORZ), S(HORZ), S(VERT), S(VERT)], [HA, HB, VA, VB], [S(NONE), NONE, NONE, NONE]]       # 8x8, 8x4, 4x8, the 16-level mixed shapes
MIX_B = [[[S(NONE), HORZ, VERT, NONE], HA, H4, V4], NONE, HORZ, VERT]         # 4x4 .. 16x4, 4x16, 32x32, 32x16, 16x32
MIX_C = [HA, HB, VA, VB]                                                      # the 32-level mixed shapes
COVER_TREES = [[MIX_A, NONE, mr.SB_32S, mr.SB_F], [HORZ, VERT, mr.SB_H, mr.SB_16], [H4, V4, HA, HB], [VA, VB, MIX_C, MIX_B]]
LUMA_MODES = [(m, d) for m in range(13) for d in ((-3, 0, 3) if 1 <= m <= 8 else (0,))]      # 29


# ---------------------------------------------------------------------------------------------------------------------------
# the reference's leaves
# ---------------------------------------------------------------------------------------------------------------------------
class Ref:
    def __init__(self):
        import make_golden as g0
        from make_golden_full_loop import y_tables
        self.R, self.QNAMES, self.aligned = g0.R, g0.QNAMES, g0.aligned
        self.tabs = y_tables()
        self.geom = mr.ref_geometry(mg.ref_lib())
        self.inv = mr.ref_inverse(mg.ref_lib())
        self.scans = {}

    def scan(self, s, t):
        if (s, t) not in self.scans:
            n = min(TX_W[s], 32) * min(TX_H[s], 32)
            self.scans[s, t] = tuple(np.ctypeslib.as_array(self.R.ref_get_scan(s, int(t), k), shape=(n,)).copy() for k in (0, 1))
        return self.scans[s, t]

    def predict(self, mi_rows, mi_cols, mi_mode, mi_uv, part, bsize, tx, mode, delta, plane, x, y, wpx, hpx, top, left, recon):
        """av1_predict_intra_block (8-bit, ED_STAGE) into the plane `recon` (2-D uint8)"""
        tile = np.array([0, mi_rows, 0, mi_cols], np.int32)
        p = svtlibs.ptr
        rc = self.R.ref_predict_intra_block(0, 12, mi_rows, mi_cols, p(mi_mode), p(mi_uv), p(tile), SHAPE_OF_PART[part], bsize, tx, mode, delta, plane, x, y,
                                            0, 0, wpx, hpx, ctypes.c_void_p(top.ctypes.data + 1), ctypes.c_void_p(left.ctypes.data + 1), p(recon),
                                            recon.strides[0], 0, 0)
        assert rc == 0

    def code(self, s, t, qrow, src, blk):
        """residual -> transform -> quantiser -> inverse on the dense block blk (the prediction, uint8 [h, w], updated) -> (qcoeff, eob)"""
        c_int, p = ctypes.c_int, svtlibs.ptr
        w, h = TX_W[s], TX_H[s]
        n = min(w, 32) * min(h, 32)
        ls = 2 if w * h > 1024 else (1 if w * h > 256 else 0)
        x = self.aligned((h, 64), np.int16)
        x[:, :w] = src.astype(np.int16) - blk.astype(np.int16)
        co = self.aligned(w * h + 64, np.int32)
        e = np.zeros(1, np.uint64)
        assert self.R.ref_estimate_transform(p(x), ctypes.c_uint32(64), p(co), c_int(s), c_int(t), c_int(0), p(e)) == 0
        coeff = self.aligned(n + 64, np.int32); coeff[:n] = co[:n]
        qc = self.aligned(n + 64, np.int32); dqc = self.aligned(n + 64, np.int32)
        eob = np.zeros(1, np.uint16)
        scan, iscan = self.scan(s, t)
        getattr(self.R, self.QNAMES[ls][2])(p(coeff), ctypes.c_ssize_t(n), c_int(0), p(qrow["zbin"]), p(qrow["round"]), p(qrow["quant"]),
                                             p(qrow["quant_shift"]), p(qc), p(dqc), p(qrow["dequant"]), p(eob), p(scan), p(iscan))
        if eob[0]:
            self.inv(dqc[:n].copy(), blk, t, s, int(eob[0]))
        return qc[:n].copy(), int(eob[0])

    def cfl(self, luma, dc, alpha):
        """the CfL step on a DC prediction dc [h, w] from the luma reconstruction [2 h, 2 w] -> prediction"""
        c_int, p = ctypes.c_int, svtlibs.ptr
        h, w = dc.shape
        luma = np.ascontiguousarray(luma)
        q3 = np.zeros((32, 32), np.int16)
        self.R.cfl_luma_subsampling_420_lbd_c(p(luma), c_int(2 * w), p(q3), c_int(2 * w), c_int(2 * h))
        self.R.subtract_average_c(p(q3), c_int(w), c_int(h), c_int(w * h // 2), c_int((w * h).bit_length() - 1))
        dc = np.ascontiguousarray(dc)
        out = np.zeros((h, w), np.uint8)
        self.R.cfl_predict_lbd_c(p(q3), p(dc), c_int(w), p(out), c_int(w), c_int(alpha), c_int(8), c_int(w), c_int(h))
        return out


def idx_to_alpha(idx, js, plane):
    """cfl_idx_to_alpha (EbIntraPrediction.h:609-617): plane 0 Cb, 1 Cr"""
    su = ((js + 1) * 11) >> 5
    sign = su if plane == 0 else (js + 1) - 3 * su
    if sign == 0:
        return 0
    mag = (idx >> 4) if plane == 0 else (idx & 15)
    return mag + 1 if sign == 2 else -mag - 1


def types_of(tx_size):
    return [t for t in range(16) if svtlibs.txfm_allowed(tx_size, t)]


def mode_ok(b):
    m, d = int(b["mode"]), int(b["angle_delta"])
    return m <= 12 and b["uv_mode"] <= 13 and -3 <= d <= 3 and (d == 0 or 1 <= m <= 8)


# ---------------------------------------------------------------------------------------------------------------------------
# the cases
# ---------------------------------------------------------------------------------------------------------------------------
def smooth_noise(rng, rows, cols, amp):
    """random content with structure: a coarse random field, bilinearly enlarged, plus noise of +-amp"""
    gy, gx = rows // 16 + 2, cols // 16 + 2
    g = rng.integers(40, 216, (gy, gx)).astype(np.float64)
    yy, xx = np.arange(rows) / 16.0, np.arange(cols) / 16.0
    y0, x0 = yy.astype(int), xx.astype(int)
    fy, fx = (yy - y0)[:, None], (xx - x0)[None, :]
    v = g[y0][:, x0] * (1 - fy) * (1 - fx) + g[y0 + 1][:, x0] * fy * (1 - fx) + g[y0][:, x0 + 1] * (1 - fy) * fx + g[y0 + 1][:, x0 + 1] * fy * fx
    return np.clip(v + rng.integers(-amp, amp + 1, (rows, cols)), 0, 255).astype(np.uint8)


def build_case(R, name, trees, sb_cols, sb_rows, width, height, seed, npics=1, inter_share=0.0, script=None, amp=2, clip=True):
    """trees: [npics][nsb] partition trees (None: an empty list).  -> the case dict (inputs)"""
    rng = np.random.default_rng(seed)
    nsb = sb_cols * sb_rows
    stride, rows = sb_cols * 64 + 64, sb_rows * 64          # (the reference's vector predictors store aligned rows)
    final = np.zeros((npics, nsb, MAX_FINAL), FINAL_DTYPE)
    count = np.zeros((npics, nsb), np.uint32)
    blks = []
    turn = {}
    for pic in range(npics):
        for sb in range(nsb):
            ox, oy = 64 * (sb % sb_cols), 64 * (sb // sb_cols)
            ents = [] if trees[pic][sb] is None else mr.tile(trees[pic][sb])
            ents = [(m, p) for m, p in ents if not clip or ox + R.geom[m]["origin_x"] + R.geom[m]["bwidth"] <= width and oy + R.geom[m]["origin_y"] + R.geom[m]["bheight"] <= height]
            for k, (mds, part) in enumerate(ents):
                g = R.geom[mds]
                bsize = int(g["bsize"])
                i = len(blks)
                final[pic, sb, k] = (mds, ox + int(g["origin_x"]), oy + int(g["origin_y"]), bsize, part, i)
                tx, tx_uv = int(g["txsize"]), int(g["txsize_uv"])
                ty, tyu = types_of(tx), types_of(tx_uv)
                t = turn.get(tx, 0); turn[tx] = t + 1
                mode, delta = LUMA_MODES[(i * 7 + bsize) % len(LUMA_MODES)]
                uv = (i * 5 + 3) % 14
                bw, bh = BS_W[bsize], BS_H[bsize]
                if uv == 13 and (bw > 32 or bh > 32 or bw < 8 or bh < 8):
                    uv = (i // 2) % 13
                blks.append((int(rng.random() >= inter_share), mode, delta, uv, int(rng.integers(0, 256)), i % 8, ty[t % len(ty)], tyu[(t // 2 + i) % len(tyu)]))
            count[pic, sb] = len(ents)
            final[pic, sb, len(ents):] = final[pic, sb, 0] if ents else (0, ox, oy, 12, 0, 0)      # past the count: would write if it were read
    blk = np.array(blks, BLK_DTYPE)
    c = dict(dims=np.array([npics, sb_cols, sb_rows, width, height, stride, rows], np.uint32), final=final, count=count, blk=blk,
             qrows=np.stack([np.stack([R.tabs[k][q] for k in QKEYS]) for q in QINDEX]))
    for p in range(3):
        r, s = (rows, stride) if p == 0 else (rows // 2, stride // 2)
        c[f"src{p}"] = np.stack([smooth_noise(rng, r, s, amp) for _ in range(npics)])
        c[f"init{p}"] = np.stack([smooth_noise(rng, r, s, amp) for _ in range(npics)]) if inter_share or script else np.full((npics, r, s), 0xA5, np.uint8)
    if script:
        script(c)
    return c


REFUSE_TREE = [S(NONE), HORZ, VERT, [NONE, NONE, NONE, [NONE, NONE, NONE, S(NONE)]]]      # entries 0-3 16x16, 4-5 32x16, 6-7 16x32, 8-10 16x16, 11-13 8x8, 14-17 4x4


def refuse_script(c):
    """the refusal case: superblock 0 REFUSE_TREE, superblock 1 a 64x64 past the bottom edge (OUTSIDE).  Entry 1 NO_SRC, 2 src >= nsrc, 4 a
    luma type the 32-sample side does not define, 5 chroma type 16, 6 is_intra 0, 8 mode 13, 9 a delta on DC, 10 uv_mode 14, 11 delta -4,
    17 (a 4x4) UV_CFL_PRED.  The others stay coded, next to and below the refused ones."""
    f, b = c["final"], c["blk"]
    src = f["src"][0, 0].copy()
    f["src"][0, 0, 1], f["src"][0, 0, 2] = NO_SRC, len(b) + 3
    b["tx_type"][src[4]] = 1
    b["tx_type_uv"][src[5]] = 16
    b["is_intra"][src[6]] = 0
    b["mode"][src[8]] = 13
    b["mode"][src[9]], b["angle_delta"][src[9]] = 0, 2
    b["uv_mode"][src[10]] = 14
    b["mode"][src[11]], b["angle_delta"][src[11]] = 3, -4
    b["uv_mode"][src[17]] = 13


def make_cases(R):
    cases = []
    for i in (0, 1):
        cases.append(build_case(R, CASE_NAMES[i], COVER_TREES[2 * i:2 * i + 2], 2, 2, 128, 128, 3100 + i, npics=2))
    edge_trees = [[mr.SB_16, MIX_B, S(S(NONE)), MIX_C, mr.SB_32S, S(S(NONE)), mr.SB_16, S(S(NONE)), S(S(S(NONE)))]]
    cases.append(build_case(R, "edges", edge_trees, 3, 3, 176, 144, 3102))
    cases.append(build_case(R, "sb4", [[mr.SB_4X4]], 1, 1, 64, 64, 3103))
    cases.append(build_case(R, "sb64", [[NONE]], 1, 1, 64, 64, 3104))
    cases.append(build_case(R, "inter", [[MIX_B, mr.SB_16, MIX_C, MIX_A]], 2, 2, 128, 128, 3105, inter_share=0.5))
    cases.append(build_case(R, "refuse", [[REFUSE_TREE, NONE]], 1, 2, 64, 96, 3106, script=refuse_script, clip=False))
    return cases


# ---------------------------------------------------------------------------------------------------------------------------
# the model: the walk around the leaves
# ---------------------------------------------------------------------------------------------------------------------------
class Lines:
    """the recon neighbour arrays of one plane (topArray, leftArray, topLeftArray)"""
    def __init__(self, w, h):
        self.top, self.left, self.tl, self.off = np.zeros(w + 256, np.uint8), np.zeros(h + 256, np.uint8), np.zeros(w + h + 512, np.uint8), h + 128

    def update(self, plane, x, y, w, h):
        H, W = plane.shape
        x1, y1 = min(x + w, W), min(y + h, H)
        if x1 <= x or y1 <= y:
            return
        self.top[x:x1] = plane[y1 - 1, x:x1]
        self.left[y:y1] = plane[y:y1, x1 - 1]
        for i in range(x, x1):
            self.tl[self.off + i - (y1 - 1)] = plane[y1 - 1, i]
        for j in range(y, y1):
            self.tl[self.off + (x1 - 1) - j] = plane[j, x1 - 1]

    def neigh(self, x, y, w, h):
        top, left = np.zeros(160, np.uint8), np.zeros(160, np.uint8)
        if y:
            top[1:1 + 2 * w] = self.top[x:x + 2 * w]
        if x:
            left[1:1 + 2 * h] = self.left[y:y + 2 * h]
        if x and y:
            top[0] = left[0] = self.tl[self.off + x - y]
        return top, left


def model(R, c, planes=3):
    """svt_hip_intra_encode_frame for a case -> dict of OUTPUT_KEYS"""
    npics, sb_cols, sb_rows, width, height, stride, rows = (int(v) for v in c["dims"])
    nsb, nsrc, blk = sb_cols * sb_rows, len(c["blk"]), c["blk"]
    qrow = [{k: np.ascontiguousarray(c["qrows"][i][j]) for j, k in enumerate(QKEYS)} for i in (0, 1)]
    W, H = (width, width // 2, width // 2), (height, height // 2, height // 2)
    recon = []
    for p in range(3):
        recon.append(R.aligned(c[f"init{p}"].shape, np.uint8))
        recon[p][:] = c[f"init{p}"]
    rmask = [np.zeros(r.shape, bool) for r in recon]
    sbq = [np.zeros((npics, nsb, SPAN[p]), np.int32) for p in range(3)]
    qmask = [np.zeros(s.shape, bool) for s in sbq]
    status, offset = np.zeros((npics, nsb, MAX_FINAL), np.uint8), np.zeros((npics, nsb, MAX_FINAL, 2), np.uint32)
    result, resmask = np.zeros((npics, nsb, MAX_FINAL), RES_DTYPE), np.zeros((npics, nsb, MAX_FINAL), bool)
    mi_rows, mi_cols = height // 4, width // 4
    for pic in range(npics):
        pl = [recon[p][pic][:H[p], :W[p]] for p in range(3)]                 # views: what lies inside the picture
        lines = [Lines(W[p], H[p]) for p in range(3)]
        mi_mode, mi_uv = np.zeros(mi_rows * mi_cols, np.uint8), np.zeros(mi_rows * mi_cols, np.uint8)
        for sb in range(nsb):
            run = [0, 0]
            for k in range(min(int(c["count"][pic, sb]), MAX_FINAL)):
                e = c["final"][pic, sb, k]
                offset[pic, sb, k] = run
                src, x, y, part = int(e["src"]), int(e["x"]), int(e["y"]), int(e["part"])
                g = R.geom[min(int(e["mds_idx"]), NBLK - 1)]
                bsize, has_uv, tx, tx_uv = int(g["bsize"]), bool(g["has_uv"]), int(g["txsize"]), int(g["txsize_uv"])
                bw, bh, cw, ch = BS_W[bsize], BS_H[bsize], TX_W[tx_uv], TX_H[tx_uv]
                cx, cy = ((x >> 3) << 3) >> 1, ((y >> 3) << 3) >> 1
                reason = OK
                if src == NO_SRC or src >= nsrc:
                    reason = R_NO_SRC
                else:
                    b = blk[src]
                    inside = x + bw <= W[0] and y + bh <= H[0]
                    if planes == 3 and has_uv:
                        inside = inside and cx + cw <= W[1] and cy + ch <= H[1]
                    if not inside:
                        reason = R_OUTSIDE
                    elif not svtlibs.txfm_allowed(tx, int(b["tx_type"])) or b["tx_type"] > 15 or (has_uv and (not svtlibs.txfm_allowed(tx_uv, int(b["tx_type_uv"])) or b["tx_type_uv"] > 15)):
                        reason = R_TX_TYPE
                    elif not b["is_intra"]:
                        reason = R_NOT_INTRA
                    elif not mode_ok(b):
                        reason = R_MODE
                    elif b["uv_mode"] == 13 and (bw > 32 or bh > 32 or bw < 8 or bh < 8):
                        reason = R_CFL_SIZE
                status[pic, sb, k] = reason
                if reason == OK:
                    b = blk[src]
                    resmask[pic, sb, k] = True
                    result["tx_type"][pic, sb, k] = b["tx_type"]
                    cfl = b["uv_mode"] == 13
                    for p in range(planes):
                        if p and not has_uv:
                            continue
                        w, h, t, ty, x0, y0 = (bw, bh, tx, int(b["tx_type"]), x, y) if p == 0 else (cw, ch, tx_uv, int(b["tx_type_uv"]), cx, cy)
                        mode, delta = (int(b["mode"]), int(b["angle_delta"])) if p == 0 else (0 if cfl else int(b["uv_mode"]), 0)
                        top, left = lines[p].neigh(x0, y0, w, h)
                        R.predict(mi_rows, mi_cols, mi_mode, mi_uv, part, bsize, t, mode, delta, p, x, y, w, h, top, left, recon[p][pic])
                        if p and cfl:
                            pl[p][y0:y0 + h, x0:x0 + w] = R.cfl(pl[0][y:y + bh, x:x + bw], pl[p][y0:y0 + h, x0:x0 + w], idx_to_alpha(int(b["cfl_alpha_idx"]), int(b["cfl_alpha_signs"]), p - 1))
                        dense = np.ascontiguousarray(pl[p][y0:y0 + h, x0:x0 + w])
                        q, eob = R.code(t, ty, qrow[p > 0], c[f"src{p}"][pic][y0:y0 + h, x0:x0 + w], dense)
                        pl[p][y0:y0 + h, x0:x0 + w] = dense
                        rmask[p][pic][y0:y0 + h, x0:x0 + w] = True
                        result["eob"][pic, sb, k, p] = eob
                        if p == 0 and eob == 0:
                            result["tx_type"][pic, sb, k] = 0
                        off, nc = run[p > 0], min(w, 32) * min(h, 32)
                        if off + w * h <= SPAN[p]:
                            sbq[p][pic, sb, off:off + nc] = q
                            qmask[p][pic, sb, off:off + nc] = True
                    for r in range(bh // 4):                                   # the mode info of a coded block
                        at = ((y >> 2) + r) * mi_cols + (x >> 2)
                        mi_mode[at:at + bw // 4], mi_uv[at:at + bw // 4] = b["mode"], b["uv_mode"]
                if reason in (OK, R_NOT_INTRA):
                    run[0] += bw * bh
                    if has_uv:
                        run[1] += cw * ch
                # the line buffers move on with what the planes hold under the entry, coded or not
                lines[0].update(pl[0], x, y, bw, bh)
                if has_uv:
                    for p in (1, 2):
                        lines[p].update(pl[p], cx, cy, cw, ch)
    out = dict(status=status, offset=offset, result=result, resmask=resmask)
    for p in range(3):
        out[f"recon{p}"], out[f"rmask{p}"], out[f"sbq{p}"], out[f"qmask{p}"] = recon[p], rmask[p], sbq[p], qmask[p]
    if planes == 1:
        for p in (1, 2):
            out[f"recon{p}"] = c[f"init{p}"].copy()
    return out


# ---------------------------------------------------------------------------------------------------------------------------
def check_coverage(cases, outs, geom):
    """the conditions of the coverage case over cover0 and cover1 together; status 0 in the cases without refusals; every status in `refuse`"""
    bsizes, parts, modes, uvs, signs, pairs = set(), set(), set(), set(), set(), set()
    zero = np.zeros((3, 2), np.int64)
    for i in COVER:
        c, o = cases[i], outs[i]
        for pic in range(c["final"].shape[0]):
            for sb in range(c["final"].shape[1]):
                for k in range(int(c["count"][pic, sb])):
                    e, b = c["final"][pic, sb, k], c["blk"][c["final"]["src"][pic, sb, k]]
                    g = geom[e["mds_idx"]]
                    bsizes.add(int(g["bsize"])); parts.add((int(e["part"]), int(g["depth"])))
                    modes.add((int(b["mode"]), int(b["angle_delta"]))); pairs.add((int(g["txsize"]), int(b["tx_type"])))
                    if g["has_uv"]:
                        uvs.add(int(b["uv_mode"])); pairs.add((int(g["txsize_uv"]), int(b["tx_type_uv"])))
                        if b["uv_mode"] == 13:
                            js = int(b["cfl_alpha_signs"])
                            su = ((js + 1) * 11) >> 5
                            signs |= {("u", su), ("v", js + 1 - 3 * su)}
                    for p in range(3 if g["has_uv"] else 1):
                        zero[p] += (o["result"]["eob"][pic, sb, k, p] == 0, 1)
    assert len(bsizes) == 19, sorted(bsizes)
    assert {p for p, _ in parts} == {0, 1, 2, 4, 5, 6, 7, 8, 9} and {(p, d) for p in (4, 5, 6, 7) for d in (0, 1)} <= parts, parts
    assert set(LUMA_MODES) <= modes, sorted(set(LUMA_MODES) - modes)
    assert uvs == set(range(14)), uvs
    assert {("u", 1), ("u", 2), ("v", 1), ("v", 2)} <= signs, signs
    want = {(t, ty) for t in range(19) for ty in types_of(t)}
    assert want <= pairs, sorted(want - pairs)
    for p in range(3):
        assert zero[p, 1] // 4 <= zero[p, 0] <= 3 * zero[p, 1] // 4, (p, zero[p].tolist())
    for i in ALL_OK:
        live = np.arange(MAX_FINAL)[None, None] < cases[i]["count"][..., None]
        assert (outs[i]["status"][live] == 0).all(), CASE_NAMES[i]
    k = CASE_NAMES.index("refuse")
    live = np.arange(MAX_FINAL)[None, None] < cases[k]["count"][..., None]
    assert set(outs[k]["status"][live].tolist()) == {OK, R_NO_SRC, R_OUTSIDE, R_TX_TYPE, R_NOT_INTRA, R_MODE, R_CFL_SIZE}, set(outs[k]["status"][live].tolist())
    return zero


def load_case(z, k):
    """case k of the fixture -> (inputs dict, outputs dict with boolean masks)"""
    c = {key: z[f"c{k}_{key}"] for key in INPUT_KEYS}
    npics, sb_cols, sb_rows = (int(v) for v in c["dims"][:3])
    c["final"] = c["final"].view(FINAL_DTYPE).reshape(npics, sb_cols * sb_rows, MAX_FINAL)
    c["blk"] = c["blk"].view(BLK_DTYPE).reshape(-1)
    o = {}
    for key in OUTPUT_KEYS:
        v = z[f"c{k}_{key}"]
        if "mask" in key:
            like = z[f"c{k}_{'recon' + key[-1] if key[0] == 'r' and key != 'resmask' else ('sbq' + key[-1] if key[0] == 'q' else 'status')}"]
            v = np.unpackbits(v)[:like.size].reshape(like.shape).astype(bool)
        o[key] = v
    o["result"] = o["result"].view(RES_DTYPE).reshape(o["status"].shape)
    return c, o


def stored(c, o):
    out = {}
    for key in INPUT_KEYS:
        v = c[key]
        out[key] = v.view(np.uint8).reshape(v.shape + (v.dtype.itemsize,)) if v.dtype.names else v
    for key in OUTPUT_KEYS:
        v = o[key]
        out[key] = np.packbits(v) if "mask" in key else (v.view(np.uint8).reshape(v.shape + (v.dtype.itemsize,)) if v.dtype.names else v)
    return out


def build_all():
    R = Ref()
    cases = make_cases(R)
    outs = [model(R, c) for c in cases]
    zero = check_coverage(cases, outs, R.geom)
    out = {"names": np.array(CASE_NAMES)}
    for k, (c, o) in enumerate(zip(cases, outs)):
        luma = model(R, c, planes=1)                                          # a luma-only call: the same luma, status and offsets
        assert all(np.array_equal(luma[key], o[key]) for key in ("status", "offset", "recon0", "rmask0", "sbq0", "qmask0")), CASE_NAMES[k]
        for key, v in stored(c, o).items():
            out[f"c{k}_{key}"] = v
        print(f"{CASE_NAMES[k]}: counts {c['count'].reshape(-1).tolist()}, {len(c['blk'])} records")
    print("eob 0 of coded plane blocks (coverage case):", zero.tolist())
    return out


def main():
    if mg.ref_lib() is None:
        raise SystemExit("oracle/_ref/libsvtref.so is not built")
    np.savez_compressed(OUT, **build_all())
    print(f"wrote {OUT}: {os.path.getsize(OUT)} bytes")


if __name__ == "__main__":
    main()

"""Writes tests/golden/real_picture.npz: one 352 x 224 window of the reference's own test clip (test/vectors/Fruits_oranges,_jardin_
japonais_2.y4m, one 1296 x 864 4:2:0 8-bit frame) and what the REFERENCE's own functions make of it, stage by stage, each stage fed
by the reference's output of the stage before - what the whole-picture calls must reproduce on real content:

  1  the padded full / quarter / sixteenth pyramids of source, list-0 and list-1 reference (Decimation2D, generate_padding; asserted
     equal to svtlibs.me_pyramid here, so the tests rebuild them from the stored windows)
  2  GatheringPictureStatistics of the source, both block_mean_calc_prec values, 4 x 4 regions (make_golden_picture_stats.ref_picture_stats)
  3  MotionEstimateLcu on every SB for a P picture with 209 PUs and a B picture with 85, both with the three HME levels on 2 x 2 regions
     and the C flavour (the AVX2 HME kernels are undefined on a width that is no multiple of 64)
  4  open_loop_intra_search_sb on every SB of the source luma, every block size from 8 to 64
  5  the encode pass of the source with the list-0 reference co-located as prediction: 16x16 DCT_DCT on luma, 8x8 DCT_DCT on Cb and
     Cr, the highbd quantize_b flavour (aom_highbd_quantize_b_c, what tests/test_gpu_encode_recon.py pins through the oracle) with the
     luma tables of one qindex; qcoeff, eob, reconstruction, and the skip map (an 8x8 luma block is skipped when its 16x16 luma block
     and both co-located 8x8 chroma blocks have eob 0)
  6  cdef_seg_search's table and block counts of that reconstruction against the source, the per-filter-block argmin strengths
     (-1 where the count is 0) and av1_cdef_frame's picture with those strengths

The pictures.  Source: the window at luma origin ORIGIN (chroma at ORIGIN / 2).  List-0 / list-1 reference: the windows displaced by
(+7, -3) / (-9, +4) luma samples (chroma of list 0 at the displaced origin >> 1), then coded with the reference's own functions:
16x16 DCT_DCT forward of (window - 128), aom_highbd_quantize_b_c at qindex REF_QINDEX, inverse onto a flat 128 prediction - a
reference picture is a reconstruction, never a copy of the source.  List 1 is luma only.

The window.  Luma origins on a 16-sample grid at least 32 samples inside the frame are scanned row by row; the first that meets
every condition of check_conditions is taken (conditions b .. e depend on the reference's outputs, so they are evaluated stage by
stage).  The measured values are printed and stored in `stats` (names in `stat_names`).

What is this file's own: reading the clip, the choice of the window, the loops over SBs and blocks, the skip map, the argmin, the
conditions, and the numpy / oracle restatements the tests use where the reference is absent (np_cdef_*; everything else is the
siblings' glue).  CPU only; run from the repository root after build():  python tests/golden/make_golden_real_picture.py
"""
import ctypes
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
OUT = os.path.join(HERE, "real_picture.npz")
CLIP = "/root/reference/test/vectors/Fruits_oranges,_jardin_japonais_2.y4m"
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, HERE)
import svtlibs                              # noqa: E402
import make_golden_cdef as mg_cdef          # noqa: E402
import make_golden_me_frame as mg_me        # noqa: E402
import make_golden_picture_stats as mg_st   # noqa: E402
from svtlibs import ptr                     # noqa: E402

W, H = 352, 224                             # 5.5 x 3.5 SBs
NSBX, NSBY = (W + 63) // 64, (H + 63) // 64
NSB = NSBX * NSBY
DISP = ((7, -3), (-9, 4))                   # list-0 / list-1 displacement (x, y)
REF_QINDEX = 140                            # base_qindex of the reference pictures' own coding
QINDEX_ORDER = (140, 160, 120, 180, 100, 200, 80)
SIZE_CAP = 768 << 10
TX_8X8, TX_16X16, DCT_DCT = 1, 2, 0
ME_CASES = {"p": dict(slice_type=1, pic_depth_mode=0), "b": dict(slice_type=0, pic_depth_mode=2)}
ME_KEYS = mg_me.KEYS
OIS_TL, OIS_IPM, OIS_ISREF = 0, 0, 1
STATS_REGIONS = (4, 4)
PLANES = ("y", "cb", "cr")
STAT_NAMES = ("flat_share", "busy_share", "me_zero_sad_share", "me_p_sbs_with_two_vectors", "me_b_sbs_with_two_vectors", "ois_modes_besides_dc",
              "ois_directional_modes", "enc_eob0_share", "enc_eob_above_10_share", "cdef_luma_strengths", "cdef_fbs_with_a_skip",
              "cdef_fbs_without_a_skip")


# ---------------------------------------------------------------------------------------------------------------------------
# the clip and the windows
# ---------------------------------------------------------------------------------------------------------------------------
def read_clip(path=CLIP):
    """the one frame of the clip -> (y, cb, cr) uint8"""
    with open(path, "rb") as f:
        head = f.readline().split()
        assert head[0] == b"YUV4MPEG2" and b"C420jpeg" in head
        fw, fh = (int(next(t for t in head if t[:1] == c)[1:]) for c in (b"W", b"H"))
        assert f.readline() == b"FRAME\n"
        y = np.frombuffer(f.read(fw * fh), np.uint8).reshape(fh, fw)
        cb = np.frombuffer(f.read(fw * fh // 4), np.uint8).reshape(fh // 2, fw // 2)
        cr = np.frombuffer(f.read(fw * fh // 4), np.uint8).reshape(fh // 2, fw // 2)
    return y, cb, cr


def window(frame, ox, oy, chroma=True):
    """the W x H window at luma origin (ox, oy): [y, cb, cr] (or [y])"""
    out = [np.ascontiguousarray(frame[0][oy:oy + H, ox:ox + W])]
    if chroma:
        out += [np.ascontiguousarray(p[oy >> 1:(oy >> 1) + H // 2, ox >> 1:(ox >> 1) + W // 2]) for p in frame[1:]]
    return out


def candidate_origins(frame):
    fh, fw = frame[0].shape
    return [(ox, oy) for oy in range(32, fh - H - 32, 16) for ox in range(32, fw - W - 32, 16)]


def block_variances(y):
    b = y.astype(np.float64).reshape(y.shape[0] // 8, 8, y.shape[1] // 8, 8)
    return b.var(axis=(1, 3))


# ---------------------------------------------------------------------------------------------------------------------------
# the reference's transform / quantiser chain (make_golden.ref_fwd / ref_inv, the quantiser gen_quant calls)
# ---------------------------------------------------------------------------------------------------------------------------
def _tables():
    return np.load(os.path.join(HERE, "tables.npz"))


def qrows(qindex, tabs=None):
    tabs = tabs if tabs is not None else _tables()
    return {k: np.ascontiguousarray(tabs[f"{k}_8"][qindex]) for k in ("zbin", "round", "quant", "quant_shift", "dequant")}


def ref_code_plane(R, src, pred, tx_size, qindex):
    """every tx_size block of `src` (raster order) against `pred` through the reference's forward transform, aom_highbd_quantize_b_c and
    inverse -> (qcoeff int32 [n, side * side], eob uint16 [n], reconstruction uint8)"""
    import make_golden as mgold              # (asserts the reference library at import: only on this route)
    tabs = _tables()
    rows = qrows(qindex, tabs)
    sc, isc = np.ascontiguousarray(tabs[f"scan_{tx_size}_0"]), np.ascontiguousarray(tabs[f"iscan_{tx_size}_0"])
    side = svtlibs.TX_W[tx_size]
    n = side * side
    h, w = src.shape
    quantize = getattr(R, mgold.QNAMES[0][0])
    assert mgold.QNAMES[0][0] == "aom_highbd_quantize_b_c"
    qs, eobs = [], []
    rec = np.zeros((h, w), np.uint8)
    for y in range(0, h, side):
        for x in range(0, w, side):
            res = np.ascontiguousarray(src[y:y + side, x:x + side].astype(np.int16) - pred[y:y + side, x:x + side].astype(np.int16))
            co = mgold.ref_fwd(tx_size, DCT_DCT, 8, res)
            qc, dqc, eob = np.zeros(n, np.int32), np.zeros(n, np.int32), np.zeros(1, np.uint16)
            quantize(ptr(co), ctypes.c_ssize_t(n), ctypes.c_int(0), ptr(rows["zbin"]), ptr(rows["round"]), ptr(rows["quant"]),
                     ptr(rows["quant_shift"]), ptr(qc), ptr(dqc), ptr(rows["dequant"]), ptr(eob), ptr(sc), ptr(isc))
            dst = np.ascontiguousarray(pred[y:y + side, x:x + side].astype(np.uint16))
            mgold.ref_inv(tx_size, DCT_DCT, 8, dqc, dst)
            assert int(dst.max()) <= 255
            rec[y:y + side, x:x + side] = dst
            qs.append(qc)
            eobs.append(eob[0])
    return np.array(qs), np.array(eobs, np.uint16), rec


def oracle_code_plane(src, pred, tx_size, qindex):
    """ref_code_plane through the oracle's chain (svt_oracle_fwd_quant_sad, svt_oracle_inv_txfm2d_add_u8) and its quantiser tables"""
    O = svtlibs.oracle()
    qt = svtlibs.quant_tables(8)
    rows = {k: v[qindex].copy() for k, v in qt.items()}
    side = svtlibs.TX_W[tx_size]
    n = side * side
    h, w = src.shape
    qs, eobs = [], []
    rec = np.zeros((h, w), np.uint8)
    for y in range(0, h, side):
        for x in range(0, w, side):
            s, p = np.ascontiguousarray(src[y:y + side, x:x + side]), np.ascontiguousarray(pred[y:y + side, x:x + side])
            co, qc, dqc = np.zeros(n, np.int32), np.zeros(n, np.int32), np.zeros(n, np.int32)
            eob, sad = np.zeros(1, np.uint16), np.zeros(1, np.uint32)
            O.svt_oracle_fwd_quant_sad(ptr(s), side, ptr(p), side, tx_size, DCT_DCT, ptr(rows["zbin"]), ptr(rows["round"]), ptr(rows["quant"]),
                                       ptr(rows["quant_shift"]), ptr(rows["dequant"]), ptr(co), ptr(qc), ptr(dqc), ptr(eob), ptr(sad))
            O.svt_oracle_inv_txfm2d_add_u8(ptr(dqc), ptr(p), side, DCT_DCT, tx_size)
            rec[y:y + side, x:x + side] = p
            qs.append(qc)
            eobs.append(eob[0])
    return np.array(qs), np.array(eobs, np.uint16), rec


def input_pictures(R, frame, ox, oy):
    """{src_y, src_cb, src_cr, ref0_y, ref0_cb, ref0_cr, ref1_y}"""
    d = dict(zip(("src_y", "src_cb", "src_cr"), window(frame, ox, oy)))
    for l, (dx, dy) in enumerate(DISP):
        for name, p in zip(PLANES, window(frame, ox + dx, oy + dy, chroma=(l == 0))):
            d[f"ref{l}_{name}"] = ref_code_plane(R, p, np.full_like(p, 128), TX_16X16, REF_QINDEX)[2]
    return d


# ---------------------------------------------------------------------------------------------------------------------------
# the stages, each -> {fixture key: array}
# ---------------------------------------------------------------------------------------------------------------------------
def me_prms(case):
    geo = svtlibs.me_pyramid(np.zeros((H, W), np.uint8))[1]
    return np.array([svtlibs.me_lcu_params(W, H, sx, sy, geo, **ME_CASES[case]) for sy in range(0, H, 64) for sx in range(0, W, 64)])


def stage_pyramids(R, pics):
    """asserts stage 1 (the reference's pyramids == svtlibs.me_pyramid); -> the reference's planes of source, list 0, list 1"""
    out = []
    for name in ("src_y", "ref0_y", "ref1_y"):
        got, geo = mg_me.ref_pyramid(R, pics[name])
        want, wgeo = svtlibs.me_pyramid(pics[name])
        assert geo == wgeo and all(np.array_equal(a, b) for a, b in zip(got, want)), name
        out.append(got)
    return out


def stage_stats(stats_fn, pics):
    """stats_fn(y, cb, cr, prec, rw, rh): ref_picture_stats with its library bound, or np_picture_stats"""
    d = {}
    for prec in (mg_st.FULL, mg_st.SUB):
        o = stats_fn(pics["src_y"], pics["src_cb"], pics["src_cr"], prec, *STATS_REGIONS)
        for k in mg_st.SB_KEYS:
            d[f"stats_p{prec}_{k}"] = o[k]
        for k in mg_st.PIC_KEYS:
            assert f"stats_{k}" not in d or np.array_equal(d[f"stats_{k}"], o[k])
            d[f"stats_{k}"] = o[k]
    return d


def stage_me(fn, pyr):
    """fn: ref_motion_estimate_lcu or the oracle's twin; pyr: the three pictures' planes"""
    d = {}
    for case in ME_CASES:
        prms = me_prms(case)
        outs = [svtlibs.run_me_lcu(fn, prm, *pyr) for prm in prms]
        d[f"me_{case}_prm"] = prms
        for k in ME_KEYS:
            d[f"me_{case}_{k}"] = np.array([o[k] for o in outs])
    return d


def ois_blocks():
    from test_oracle_golden import ois_md_scan, ois_raster_idx
    return ois_md_scan(), ois_raster_idx


def ois_validity():
    md, raster = ois_blocks()
    valid = np.zeros((NSB, 85), np.uint8)
    for sb in range(NSB):
        sx, sy = (sb % NSBX) * 64, (sb // NSBX) * 64
        for (x, y, s) in md:
            valid[sb, raster(x, y, s)] = sx + x + s <= W and sy + y + s <= H
    return valid


def stage_ois(R, luma_plane):
    """make_golden.gen_ois's route to open_loop_intra_search_sb (ref_ois_sb), every SB; luma_plane: the padded full-size plane"""
    pad = svtlibs.ME_PADS[0]
    buf = np.ascontiguousarray(luma_plane)
    valid = ois_validity()
    d = dict(ois_valid=valid, ois_count=np.zeros((NSB, 85), np.uint8), ois_best=np.zeros((NSB, 85), np.int8), ois_mode=np.zeros((NSB, 85, 61), np.uint8),
             ois_delta=np.zeros((NSB, 85, 61), np.int8), ois_dist=np.zeros((NSB, 85, 61), np.uint32))
    c_int = ctypes.c_int
    for sb in range(NSB):
        sx, sy = (sb % NSBX) * 64, (sb // NSBX) * 64
        rc = R.ref_ois_sb(ptr(buf), c_int(buf.shape[1]), c_int(pad), c_int(pad), c_int(W), c_int(H), c_int(sx), c_int(sy), ptr(valid[sb]),
                          c_int(OIS_TL), c_int(OIS_IPM), c_int(OIS_ISREF), ptr(d["ois_count"][sb]), ptr(d["ois_best"][sb]), ptr(d["ois_mode"][sb]),
                          ptr(d["ois_delta"][sb]), ptr(d["ois_dist"][sb]))
        assert rc == 0
    return d


def oracle_ois(luma):
    """stage_ois through the oracle (svt_oracle_ois_candidates, svt_oracle_ois_block) on the unpadded luma"""
    O = svtlibs.oracle()
    md, raster = ois_blocks()
    valid = ois_validity()
    d = dict(ois_valid=valid, ois_count=np.zeros((NSB, 85), np.uint8), ois_best=np.zeros((NSB, 85), np.int8), ois_mode=np.zeros((NSB, 85, 61), np.uint8),
             ois_delta=np.zeros((NSB, 85, 61), np.int8), ois_dist=np.zeros((NSB, 85, 61), np.uint32))
    luma = np.ascontiguousarray(luma)
    c_int = ctypes.c_int
    for sb in range(NSB):
        sx, sy = (sb % NSBX) * 64, (sb // NSBX) * 64
        for i, (x, y, s) in enumerate(md):                     # fixture rows are in MD-scan order, validity in raster order
            if not valid[sb, raster(x, y, s)]:
                continue
            n = O.svt_oracle_ois_candidates(c_int(s), c_int(OIS_TL), c_int(OIS_IPM), c_int(OIS_ISREF), c_int(0), ptr(d["ois_mode"][sb, i]),
                                            ptr(d["ois_delta"][sb, i]))
            d["ois_count"][sb, i] = n
            d["ois_best"][sb, i] = O.svt_oracle_ois_block(ptr(luma), c_int(W), c_int(W), c_int(H), c_int(sx + x), c_int(sy + y), c_int(s), c_int(n),
                                                          ptr(d["ois_mode"][sb, i]), ptr(d["ois_delta"][sb, i]), ptr(d["ois_dist"][sb, i]))
    return d


def skip_map(eob_y, eob_cb, eob_cr):
    """uint8 [H / 8, W / 8]: 1 where the 16x16 luma block and both co-located 8x8 chroma blocks have eob 0"""
    z = (eob_y.reshape(H // 16, W // 16) == 0) & (eob_cb.reshape(H // 16, W // 16) == 0) & (eob_cr.reshape(H // 16, W // 16) == 0)
    return np.ascontiguousarray(np.kron(z.astype(np.uint8), np.ones((2, 2), np.uint8)))


def stage_encode(code_plane, pics, qindex):
    """code_plane(src, pred, tx_size, qindex): ref_code_plane with its library bound, or oracle_code_plane"""
    d = {}
    for name in PLANES:
        q, e, r = code_plane(pics[f"src_{name}"], pics[f"ref0_{name}"], TX_16X16 if name == "y" else TX_8X8, qindex)
        d[f"enc_{name}_qcoeff"], d[f"enc_{name}_eob"], d[f"enc_{name}_recon"] = q, e, r
    d["skip"] = skip_map(d["enc_y_eob"], d["enc_cb_eob"], d["enc_cr_eob"])
    return d


def argmin_strengths(mse, count):
    """per filter block the first strength of least table entry (luma, chroma), -1 where no block is listed"""
    ys, us = mse[0].argmin(1).astype(np.int8), mse[1].argmin(1).astype(np.int8)
    ys[count == 0] = -1
    us[count == 0] = -1
    return ys, us


def stage_cdef(L, pics, enc, qindex):
    rec = [enc[f"enc_{n}_recon"] for n in PLANES]
    src = [pics[f"src_{n}"] for n in PLANES]
    mse, count, dirs, var = mg_cdef.ref_search(L, rec, src, enc["skip"], 8, qindex)
    ys, us = argmin_strengths(mse, count)
    out = mg_cdef.ref_apply(L, rec, enc["skip"], 8, qindex, ys, us)
    d = dict(cdef_mse=mse, cdef_count=count, cdef_dir=dirs, cdef_var=var, cdef_ystr=ys, cdef_ustr=us)
    for n, o in zip(PLANES, out):
        d[f"cdef_out_{n}"] = o
    return d


# ---------------------------------------------------------------------------------------------------------------------------
# the numpy restatement of the CDEF stage, on make_golden_cdef.np_filter_block (directions and variances from the fixture)
# ---------------------------------------------------------------------------------------------------------------------------
def np_cdef_filter_fb(rec_plane, skip, fbr, fbc, pli, gi, q, dirs, var):
    """cdef_filter_fb's blocks of one filter block and plane at strength gi -> [((by, bx), filtered n x n)] (EbCdef.c:273-358)"""
    l2 = 3 - (pli > 0)
    n = 1 << l2
    pri, sec = gi // 4, gi % 4 + (gi % 4 == 3)
    damping = 3 + (q >> 6) - (pli > 0)
    inbuf = mg_cdef.fill_inbuf(None, rec_plane.astype(np.uint16), fbr, fbc, l2, skip.shape)
    out = []
    for by, bx in mg_cdef.build_dlist(skip, fbr, fbc)[1]:
        if pri == 0 and sec == 0:
            y0, x0 = ((fbr * 8 + by) << l2), ((fbc * 8 + bx) << l2)
            out.append(((by, bx), rec_plane[y0:y0 + n, x0:x0 + n].astype(np.int64)))
            continue
        t = pri if pli else mg_cdef.adjust_strength(pri, int(var[by, bx]))
        out.append(((by, bx), mg_cdef.np_filter_block(inbuf, by, bx, n, t, sec, int(dirs[by, bx]) if pri else 0, damping, 0)[0]))
    return out


def np_cdef_apply(rec, skip, q, ystr, ustr, dirs, var):
    nhfb = (skip.shape[1] + 7) // 8
    out = [p.copy() for p in rec]
    for fb in range(len(ystr)):
        ys, us = int(ystr[fb]), int(ustr[fb])
        fbr, fbc = fb // nhfb, fb % nhfb
        if ys < 0 or us < 0 or (ys == 0 and us == 0):
            continue
        for pli in range(3):
            l2 = 3 - (pli > 0)
            for (by, bx), blk in np_cdef_filter_fb(rec[pli], skip, fbr, fbc, pli, us if pli else ys, q, dirs[fb], var[fb]):
                y0, x0 = ((fbr * 8 + by) << l2), ((fbc * 8 + bx) << l2)
                out[pli][y0:y0 + blk.shape[0], x0:x0 + blk.shape[1]] = blk
    return out


def np_cdef_chroma_mse(rec, src, skip, q, fb, gi, dirs, var):
    """the chroma entry of cdef_seg_search's table: the squared error of Cb and Cr over the listed blocks (compute_cdef_dist on chroma)"""
    nhfb = (skip.shape[1] + 7) // 8
    fbr, fbc = fb // nhfb, fb % nhfb
    tot = 0
    for pli in (1, 2):
        for (by, bx), blk in np_cdef_filter_fb(rec[pli], skip, fbr, fbc, pli, gi, q, dirs[fb], var[fb]):
            y0, x0 = (fbr * 8 + by) * 4, (fbc * 8 + bx) * 4
            e = blk - src[pli][y0:y0 + 4, x0:x0 + 4].astype(np.int64)
            tot += int((e * e).sum())
    return tot


# ---------------------------------------------------------------------------------------------------------------------------
# the conditions
# ---------------------------------------------------------------------------------------------------------------------------
def cond_a(g):
    v = block_variances(g["src_y"])
    vals = dict(flat_share=float((v < 2).mean()), busy_share=float((v > 500).mean()))
    return vals, vals["flat_share"] >= 0.05 and vals["busy_share"] >= 0.05


def cond_b(g):
    zero = total = 0
    vals = {}
    for case, kw in ME_CASES.items():
        nl = 1 if kw["slice_type"] == 1 else 2
        npus = 209 if kw["pic_depth_mode"] <= 1 else 85
        sad = g[f"me_{case}_best_sad"][:, :nl, :npus]
        zero += int((sad == 0).sum())
        total += sad.size
        mv = g[f"me_{case}_best_mv"][:, 0, 21:85]
        vals[f"me_{case}_sbs_with_two_vectors"] = float(sum(len(np.unique(r)) >= 2 for r in mv))
    vals["me_zero_sad_share"] = zero / total
    return vals, vals["me_zero_sad_share"] <= 0.01 and vals["me_p_sbs_with_two_vectors"] >= 3 and vals["me_b_sbs_with_two_vectors"] >= 3


def cond_c(g):
    md, raster = ois_blocks()
    listed = np.array([[g["ois_valid"][sb, raster(x, y, s)] for (x, y, s) in md] for sb in range(NSB)], bool)
    assert (g["ois_count"][listed] > 0).all() and not g["ois_count"][~listed].any()
    best = np.take_along_axis(g["ois_mode"], g["ois_best"].astype(np.int64)[..., None], axis=2)[..., 0][listed]
    modes = set(int(m) for m in best) - {0}
    vals = dict(ois_modes_besides_dc=float(len(modes)), ois_directional_modes=float(len([m for m in modes if 1 <= m <= 8])))   # V_PRED .. D67_PRED
    return vals, len(modes) >= 3 and vals["ois_directional_modes"] >= 1


def cond_d(g):
    e = g["enc_y_eob"]
    vals = dict(enc_eob0_share=float((e == 0).mean()), enc_eob_above_10_share=float((e > 10).mean()))
    return vals, vals["enc_eob0_share"] >= 0.10 and vals["enc_eob_above_10_share"] >= 0.10


def cond_e(g):
    ys = g["cdef_ystr"]
    skip = g["skip"]
    h8, w8 = skip.shape
    has = [bool(skip[8 * r:8 * r + 8, 8 * c:8 * c + 8].any()) for r in range((h8 + 7) // 8) for c in range((w8 + 7) // 8)]
    vals = dict(cdef_luma_strengths=float(len(set(int(v) for v in ys if v >= 0))), cdef_fbs_with_a_skip=float(sum(has)),
                cdef_fbs_without_a_skip=float(len(has) - sum(has)))
    return vals, vals["cdef_luma_strengths"] >= 4 and vals["cdef_fbs_with_a_skip"] >= 1 and vals["cdef_fbs_without_a_skip"] >= 1


def measure(g):
    """-> ({stat name: value}, {condition letter: met})"""
    vals, met = {}, {}
    for letter, fn in zip("abcde", (cond_a, cond_b, cond_c, cond_d, cond_e)):
        v, ok = fn(g)
        vals.update(v)
        met[letter] = ok
    return vals, met


def check_conditions(g):
    """asserts conditions (a) .. (e) and the fixture's shape on the loaded file; no reference needed"""
    vals, met = measure(g)
    assert all(met.values()), (met, vals)
    assert [str(n) for n in g["stat_names"]] == list(STAT_NAMES)
    assert np.allclose(g["stats"], [vals[n] for n in STAT_NAMES]), (g["stats"], vals)
    ox, oy = (int(v) for v in g["origin"])
    assert ox % 16 == 0 and oy % 16 == 0 and ox >= 32 and oy >= 32
    assert g["src_y"].shape == (H, W) and g["src_cb"].shape == (H // 2, W // 2) and g["ref0_cr"].shape == (H // 2, W // 2) and g["ref1_y"].shape == (H, W)
    assert "ref1_cb" not in g
    for l in (0, 1):                                          # a reference is a reconstruction, never a copy of the source
        assert (g[f"ref{l}_y"] != g["src_y"]).mean() > 0.5
    assert int(g["ref_qindex"]) == REF_QINDEX and int(g["qindex"]) in QINDEX_ORDER
    assert g["me_p_results"].shape == (NSB, 209, 11) and g["ois_dist"].shape == (NSB, 85, 61) and g["cdef_mse"].shape == (2, NSB, 64)
    assert ((g["cdef_ystr"] == -1) == (g["cdef_count"] == 0)).all() and ((g["cdef_ustr"] == -1) == (g["cdef_count"] == 0)).all()


# ---------------------------------------------------------------------------------------------------------------------------
# the fixture
# ---------------------------------------------------------------------------------------------------------------------------
DERIVED = {f"enc_{n}_recon": f"src_{n}" for n in PLANES}
DERIVED.update({f"cdef_out_{n}": f"enc_{n}_recon" for n in PLANES})


def pack(g):
    """the dict as stored: a derived picture as its int16 difference from the picture it derives from"""
    d = {}
    for k, v in g.items():
        if k in DERIVED:
            d[k + "_diff"] = v.astype(np.int16) - g[DERIVED[k]].astype(np.int16)
        else:
            d[k] = v
    return d


def load(path=OUT):
    """the stored file -> dict with the derived pictures restored"""
    z = np.load(path)
    g = {k: z[k] for k in z.files if not k.endswith("_diff")}
    for k, base in DERIVED.items():                            # insertion order: the reconstructions before the CDEF pictures
        g[k] = (z[k + "_diff"] + g[base].astype(np.int16)).astype(np.uint8)
    return g


def build_fixture(frame, ox, oy, qindex, log=None):
    """every stage at one window through the reference -> (dict, None), or (None, the letter of the first condition missed)"""
    R = svtlibs.ref()
    assert R is not None, "oracle/_ref/libsvtref.so is not built (run build() where the reference sources are present)"
    say = log or (lambda *a: None)
    g = dict(origin=np.array([ox, oy], np.int32), qindex=np.array(qindex, np.int32), ref_qindex=np.array(REF_QINDEX, np.int32),
             displacement=np.array(DISP, np.int32))
    g["src_y"] = window(frame, ox, oy)[0]
    if not cond_a(g)[1]:
        return None, "a"
    g.update(input_pictures(R, frame, ox, oy))
    pyr = stage_pyramids(R, g)
    g.update(stage_me(R.ref_motion_estimate_lcu, pyr))
    say("  (b)", cond_b(g))
    if not cond_b(g)[1]:
        return None, "b"
    g.update(stage_ois(R, pyr[0][0]))
    say("  (c)", cond_c(g))
    if not cond_c(g)[1]:
        return None, "c"
    g.update(stage_encode(lambda *a: ref_code_plane(R, *a), g, qindex))
    say("  (d)", cond_d(g))
    if not cond_d(g)[1]:
        return None, "d"
    g.update(stage_cdef(mg_cdef.ref_lib(), g, g, qindex))
    say("  (e)", cond_e(g))
    if not cond_e(g)[1]:
        return None, "e"
    S = mg_st.ref_lib()
    g.update(stage_stats(lambda *a: mg_st.ref_picture_stats(S, *a), g))
    vals, _ = measure(g)
    g["stat_names"] = np.array(STAT_NAMES)
    g["stats"] = np.array([vals[n] for n in STAT_NAMES], np.float64)
    return g, None


def main():
    frame = read_clip()
    missed_before_encode = {}
    g = None
    for qindex in QINDEX_ORDER:                                # another qindex only if (d) is missed on every window
        for ox, oy in candidate_origins(frame):
            if (ox, oy) in missed_before_encode:
                continue
            print(f"window ({ox}, {oy}) at qindex {qindex}")
            g, missed = build_fixture(frame, ox, oy, qindex, log=print)
            if g is not None:
                break
            if missed in "abc":
                missed_before_encode[(ox, oy)] = missed
            print(f"  misses ({missed})")
        if g is not None:
            break
    assert g is not None, "no window meets the conditions"
    check_conditions(g)
    np.savez_compressed(OUT, **pack(g))
    size = os.path.getsize(OUT)
    back = load(OUT)
    assert sorted(back) == sorted(g) and all(np.array_equal(back[k], g[k]) and back[k].dtype == g[k].dtype for k in g)
    for n, v in zip(STAT_NAMES, g["stats"]):
        print(f"  {n} = {v:.4g}")
    print(f"wrote {OUT}: {size} bytes, origin {tuple(int(v) for v in g['origin'])}, qindex {int(g['qindex'])}")
    assert size < SIZE_CAP, size


if __name__ == "__main__":
    main()

"""Writes tests/golden/inter_pred.npz: translational inter prediction as av1_inter_prediction / av1_inter_prediction_hbd
(EbInterPrediction.c:1024, :2093) write it, what svt_hip_inter_pred_frame must reproduce, on a 104x72 4:2:0 picture, 8- and 10-bit.

What is pinned to what.  The LEAVES are the reference's own functions in oracle/_ref/libsvtref.so through ctypes: the sixteen _c convolve
entries (av1_convolve_{2d,x,y,2d_copy}_sr_c, av1_jnt_convolve_{2d,x,y,2d_copy}_c and their av1_highbd_ twins) and
av1_get_interp_filter_params_with_block_size, whose returned filter_ptr is also where the six tap tables are read from, as DATA, into
the fixture ("taps").  The GLUE is this file's own (block_glue, ref_inter_pred), in Python integers next to the line numbers it follows:
the clamp (clamp_mv_to_umv_border_sb :80-102 with the edges of EbAdaptiveMotionVectorPrediction.c:1169-1172), the addressing (:1282,
:1310, :1290), the chroma scaling, the filter choice by block dimension (:951-959), get_conv_params_no_round (convolve.h:115) and the
two-pass compound (:1291 / :1390: list 0 with do_average 0 into the CONV_BUF_TYPE buffer, list 1 with do_average 1).

np_inter_pred is the numpy restatement tests use where the reference is not built (and compare with it where it is): every entry as the
reference writes it, offsets and the uint16 intermediate included.  np_unified is the single 2-D body the device runs
(csrc/kernel_inter_pred.h); check_unified asserts it equal to the sixteen compiled entries.

The planes are not stored: make_planes regenerates them (tests compare what they regenerate with a stored checksum).

CPU only; run from the repository root after build():  python tests/golden/make_golden_inter_pred.py
"""
import ctypes
import os
import sys
import zlib

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import svtlibs  # noqa: E402

OUT = os.path.join(HERE, "inter_pred.npz")
W, H = 104, 72                                # luma picture
PAD = (80, 48)                                # border of the luma / chroma planes, every side (the contract: bw + 8 / bw + 10)
CONTENTS = ("random", "max", "checker1", "checker2")
LIST0, LIST1, BI = 0, 1, 2                    # UNI_PRED_LIST_0 / UNI_PRED_LIST_1 / BI_PRED, EbDefinitions.h:2061-2063
SAD, SSD = 0, 1
SIDES = (4, 8, 16, 32, 64)
BLK_DTYPE = np.dtype([("x", np.uint16), ("y", np.uint16), ("mv", np.int16, (2, 2)), ("pred_direction", np.uint8), ("filter_x", np.uint8),
                      ("filter_y", np.uint8), ("pad", np.uint8)])
assert BLK_DTYPE.itemsize == 16
GROUP_COLS = ("bd", "content", "ss", "bwidth", "bheight", "same_plane", "plane")      # plane: 0 Y, 1 Cb, 2 Cr
SUBPEL_BITS, SUBPEL_MASK, FILTER_BITS, ROUND0, AOM_INTERP_EXTEND = 4, 15, 7, 3, 4
ENTRY_NAMES = {(0, 0): "2d_copy", (1, 0): "x", (0, 1): "y", (1, 1): "2d"}


def i16(v):
    return ((int(v) + 32768) & 0xffff) - 32768


# ---- the planes ---------------------------------------------------------------------------------------------------------------------
def make_planes(bd, content):
    """{"ref0": [y, cb, cr], "ref1": [...], "src": [...]}: padded planes (borders are ordinary samples of the same kind).  random; constant
    maximum; a 0 / max checkerboard at 1- and at 2-sample pitch (the sharp kernels overshoot on both sides: clips at 0 and at max)"""
    rng = np.random.default_rng([0x1A7E, bd, CONTENTS.index(content)])
    mx = (1 << bd) - 1
    dt = np.uint8 if bd == 8 else np.uint16
    out = {}
    for name in ("ref0", "ref1", "src"):
        planes = []
        for k in range(3):
            pad = PAD[0] if k == 0 else PAD[1]
            h, w = (H, W) if k == 0 else (H // 2, W // 2)
            shape = (h + 2 * pad, w + 2 * pad)
            yy, xx = np.mgrid[0:shape[0], 0:shape[1]]
            if content == "random" or name == "src":
                p = rng.integers(0, mx + 1, shape)
            elif content == "max":
                p = np.full(shape, mx)
            else:
                pitch = 1 if content == "checker1" else 2
                p = (((yy // pitch) + (xx // pitch) + (name == "ref1")) & 1) * mx
            planes.append(np.ascontiguousarray(p.astype(dt)))
        out[name] = planes
    return out


def planes_crc(planes):
    c = 0
    for name in ("ref0", "ref1", "src"):
        for p in planes[name]:
            c = zlib.crc32(p.tobytes(), c)
    return c


# ---- the glue -----------------------------------------------------------------------------------------------------------------------
def clamp_mv(mv, org, lsize, psize, pic, ss):
    """one direction of clamp_mv_to_umv_border_sb (:80-102): mv in 1/8 luma sample -> 1/16 plane sample.  org / lsize: the block's luma
    origin and side, psize: the plane's side, pic: the picture's luma side"""
    mi = org >> 2                                              # mi_col = cu_origin_x >> MI_SIZE_LOG2, EbAdaptiveMotionVectorPrediction.c:1157-1158
    to_lo = -((mi * 4) * 8)                                    # mb_to_left_edge / mb_to_top_edge, :1169, :1171
    to_hi = (((pic >> 2) - (lsize >> 2) - mi) * 4) * 8         # mb_to_right_edge / mb_to_bottom_edge, :1170, :1172 (mi_cols = pic / 4)
    spel_lo = (AOM_INTERP_EXTEND + psize) << SUBPEL_BITS       # :86, :88
    spel_hi = spel_lo - (1 << SUBPEL_BITS)                     # :87, :89
    v = i16(int(mv) * (1 << (1 - ss)))                         # :90-91, the (int16_t) cast before the clamp
    lo, hi = to_lo * (1 << (1 - ss)) - spel_lo, to_hi * (1 << (1 - ss)) + spel_hi      # :96-99
    return i16(lo if v < lo else (hi if v > hi else v))       # clamp_mv :71-75


def block_glue(b, ss, bwidth, bheight):
    """-> (px, py, [(q_col, q_row) per list]) of one block record: the plane position (:1282 luma, :1310 chroma) and the clamped vectors"""
    x, y = int(b["x"]), int(b["y"])
    pw, ph = bwidth >> ss, bheight >> ss
    px, py = (((x >> 3) << 3) // 2, ((y >> 3) << 3) // 2) if ss else (x, y)
    q = [(clamp_mv(b["mv"][l][0], x, bwidth, pw, W, ss), clamp_mv(b["mv"][l][1], y, bheight, ph, H, ss)) for l in range(2)]
    return px, py, q


def lists_of(direction):
    return {LIST0: (0,), LIST1: (1,), BI: (0, 1)}[int(direction)]


def conv_rounds(compound):
    """get_conv_params_no_round (convolve.h:115-144) for bd 8 / 10: (round_0, round_1)"""
    return ROUND0, (7 if compound else 2 * FILTER_BITS - ROUND0)


# ---- the reference path -------------------------------------------------------------------------------------------------------------
class InterpFilterParams(ctypes.Structure):                    # EbDefinitions.h:487-492; InterpFilter is a one-byte packed enum
    _fields_ = [("filter_ptr", ctypes.POINTER(ctypes.c_int16)), ("taps", ctypes.c_uint16), ("subpel_shifts", ctypes.c_uint16),
                ("interp_filter", ctypes.c_uint8)]


class ConvolveParams(ctypes.Structure):                        # EbDefinitions.h:416-428
    _fields_ = [("ref", ctypes.c_int32), ("do_average", ctypes.c_int32), ("dst", ctypes.c_void_p), ("dst_stride", ctypes.c_int32),
                ("round_0", ctypes.c_int32), ("round_1", ctypes.c_int32), ("plane", ctypes.c_int32), ("is_compound", ctypes.c_int32),
                ("use_jnt_comp_avg", ctypes.c_int32), ("fwd_offset", ctypes.c_int32), ("bck_offset", ctypes.c_int32)]


assert ctypes.sizeof(InterpFilterParams) == 16 and ctypes.sizeof(ConvolveParams) == 48


def entry_name(bd, sx, sy, compound):
    core = ENTRY_NAMES[(int(sx != 0), int(sy != 0))]
    hb = "highbd_" if bd > 8 else ""
    return f"av1_{hb}jnt_convolve_{core}_c" if compound else f"av1_{hb}convolve_{core}_sr_c"


ALL_ENTRIES = sorted(entry_name(bd, sx, sy, c) for bd in (8, 10) for sx in (0, 1) for sy in (0, 1) for c in (0, 1))


def ref_lib():
    R = svtlibs.ref()
    if R is None or not hasattr(R, "av1_get_interp_filter_params_with_block_size"):
        return None
    R.av1_get_interp_filter_params_with_block_size.restype = InterpFilterParams
    R.av1_get_interp_filter_params_with_block_size.argtypes = [ctypes.c_uint8, ctypes.c_int32]
    for n in ALL_ENTRIES:
        f = getattr(R, n)
        f.restype = None
        f.argtypes = [ctypes.c_void_p, ctypes.c_int32, ctypes.c_void_p, ctypes.c_int32, ctypes.c_int32, ctypes.c_int32, ctypes.c_void_p,
                      ctypes.c_void_p, ctypes.c_int32, ctypes.c_int32, ctypes.c_void_p] + ([ctypes.c_int32] if "highbd" in n else [])
    return R


def ref_filter_params(R, f, dim):
    return R.av1_get_interp_filter_params_with_block_size(int(f), int(dim))


def table_index(f, dim):
    """which of the six recorded tables av1_get_interp_filter_params_with_block_size (:940-949) returns: 0 .. 3 the InterpFilter's own,
    4 sub_pel_filters_4, 5 sub_pel_filters_4smooth"""
    if dim <= 4 and f in (0, 2):
        return 4
    if dim <= 4 and f == 1:
        return 5
    return f


def record_taps(R):
    """the six tables as data, through filter_ptr"""
    t = np.zeros((6, 16, 8), np.int16)
    for idx, (f, dim) in enumerate(((0, 8), (1, 8), (2, 8), (3, 8), (0, 4), (1, 4))):
        p = ref_filter_params(R, f, dim)
        assert p.taps == 8 and p.subpel_shifts == 16
        t[idx] = np.ctypeslib.as_array(p.filter_ptr, shape=(128,)).reshape(16, 8)
    return t


def ref_convolve(R, plane, pad, bd, px, py, q, w, h, fx, fy, compound, do_average, tmp, dst, stats=None):
    """one convolve[subpel_x != 0][subpel_y != 0][is_compound] call (:1288-1306) on the padded plane"""
    sx, sy = q[0] & SUBPEL_MASK, q[1] & SUBPEL_MASK                                            # :1288-1289
    r0, c0 = pad + py + (q[1] >> SUBPEL_BITS), pad + px + (q[0] >> SUBPEL_BITS)                # :1282 / :1310, :1290
    assert 3 <= r0 and r0 + h + 4 <= plane.shape[0] and 3 <= c0 and c0 + w + 4 <= plane.shape[1], "the border contract"
    fpx, fpy = ref_filter_params(R, fx, w), ref_filter_params(R, fy, h)                        # :951-959
    cp = ConvolveParams()
    cp.do_average, cp.is_compound = do_average, compound
    cp.round_0, cp.round_1 = conv_rounds(compound)
    cp.dst, cp.dst_stride, cp.use_jnt_comp_avg = tmp.ctypes.data, w, 0
    name = entry_name(bd, sx, sy, compound)
    src = plane.ctypes.data + (r0 * plane.shape[1] + c0) * plane.itemsize
    args = [src, plane.shape[1], dst.ctypes.data, w, w, h, ctypes.addressof(fpx), ctypes.addressof(fpy), sx, sy, ctypes.addressof(cp)]
    getattr(R, name)(*(args + ([bd] if bd > 8 else [])))
    if stats is not None:
        stats["entries"].add(name)
        if sx:
            stats["tables"].add(table_index(fx, w))
        if sy:
            stats["tables"].add(table_index(fy, h))


def ref_inter_pred(R, planes, bd, ss, plane_idx, bwidth, bheight, blk, same_plane=False, stats=None):
    """[n, h, w] predictions of the block records through the compiled leaves"""
    w, h = bwidth >> ss, bheight >> ss
    pad = PAD[1] if ss else PAD[0]
    dt = np.uint8 if bd == 8 else np.uint16
    out = np.zeros((len(blk), h, w), dt)
    for i, b in enumerate(blk):
        px, py, q = block_glue(b, ss, bwidth, bheight)
        d = int(b["pred_direction"])
        compound = int(d == BI)                                                                # :1045
        tmp = np.zeros((h, w), np.uint16)                                                      # tmp_dstY, :1046
        dst = np.zeros((h, w), dt)
        for l in lists_of(d):
            ref = planes["ref0" if (l == 0 or same_plane) else "ref1"][plane_idx]
            ref_convolve(R, ref, pad, bd, px, py, q[l], w, h, int(b["filter_x"]), int(b["filter_y"]), compound, int(compound and l == 1), tmp, dst, stats)
        out[i] = dst
    return out


# ---- the numpy restatement ----------------------------------------------------------------------------------------------------------
def rnd(v, n):
    return (v + ((1 << n) >> 1)) >> n                          # ROUND_POWER_OF_TWO


def np_convolve(win, taps, bd, sx, sy, fx_tab, fy_tab, w, h, compound, do_average, tmp, stats=None):
    """one entry as the reference writes it.  win: the (h + 7) x (w + 7) window whose sample (3, 3) is the block's first, int64.  ->
    the clipped prediction (int64 [h, w]) or None after writing the CONV_BUF_TYPE intermediate into tmp (compound, do_average 0)"""
    r0, r1 = conv_rounds(compound)
    mx = (1 << bd) - 1
    xf, yf = taps[fx_tab][sx].astype(np.int64), taps[fy_tab][sy].astype(np.int64)
    blk = win[3:3 + h, 3:3 + w]
    offset_bits = bd + 2 * FILTER_BITS - r0
    round_offset = (1 << (offset_bits - r1)) + (1 << (offset_bits - r1 - 1))
    if sx and sy:                                              # av1_convolve_2d_sr_c :131-181, av1_jnt_convolve_2d_c :267-336
        im = sum(xf[k] * win[:, k:k + w] for k in range(8)) + (1 << (bd + FILTER_BITS - 1))
        im = rnd(im, r0)
        assert im.min() >= -32768 and im.max() <= 32767        # (int16_t) im_block
        s = sum(yf[k] * im[k:k + h] for k in range(8)) + (1 << offset_bits)
        res = rnd(s, r1)
        if not compound:
            res = res - round_offset
            pre = rnd(res, 2 * FILTER_BITS - r0 - r1)
    elif sy:                                                   # av1_convolve_y_sr_c :183-213, av1_jnt_convolve_y_c :338-390
        s = sum(yf[k] * win[k:k + h, 3:3 + w] for k in range(8))
        if not compound:
            pre = rnd(s, FILTER_BITS)
        else:
            res = (rnd(s * (1 << (FILTER_BITS - r0)), r1) + round_offset)
    elif sx:                                                   # av1_convolve_x_sr_c :215-246, av1_jnt_convolve_x_c :392-444
        s = sum(xf[k] * win[3:3 + h, k:k + w] for k in range(8))
        if not compound:
            pre = rnd(rnd(s, r0), FILTER_BITS - r0)
        else:
            res = (1 << (FILTER_BITS - r1)) * rnd(s, r0) + round_offset
    else:                                                      # av1_convolve_2d_copy_sr_c :248-265, av1_jnt_convolve_2d_copy_c :446-489
        if not compound:
            pre = blk.copy()
        else:
            res = (blk << (2 * FILTER_BITS - r1 - r0)) + round_offset
    if compound:
        res = res & 0xffff                                     # CONV_BUF_TYPE is uint16
        if not do_average:
            tmp[:] = res
            return None
        t = (tmp.astype(np.int64) + res) >> 1                  # :322-323
        pre = rnd(t - round_offset, 2 * FILTER_BITS - r0 - r1)
    if stats is not None:
        stats["clip0"] += int((pre < 0).sum())
        stats["clipmax"] += int((pre > mx).sum())
    return np.clip(pre, 0, mx)


def np_unified(win, taps, bd, sx, sy, fx_tab, fy_tab, w, h):
    """V of csrc/kernel_inter_pred.h: the 2-D body with the full-pel kernel where a direction is not filtered, offsets cancelled"""
    xf, yf = taps[fx_tab][sx].astype(np.int64), taps[fy_tab][sy].astype(np.int64)
    hr = (sum(xf[k] * win[:, k:k + w] for k in range(8)) + 4) >> 3
    return sum(yf[k] * hr[k:k + h] for k in range(8))


def window(plane, pad, px, py, q, w, h):
    r0, c0 = pad + py + (q[1] >> SUBPEL_BITS), pad + px + (q[0] >> SUBPEL_BITS)
    assert 3 <= r0 and r0 + h + 4 <= plane.shape[0] and 3 <= c0 and c0 + w + 4 <= plane.shape[1], "the border contract"
    return plane[r0 - 3:r0 + h + 4, c0 - 3:c0 + w + 4].astype(np.int64)


def np_inter_pred(taps, planes, bd, ss, plane_idx, bwidth, bheight, blk, same_plane=False, stats=None, unified=False):
    """[n, h, w] predictions of the block records, numpy only.  unified: through np_unified and the device's two rounding lines"""
    w, h = bwidth >> ss, bheight >> ss
    pad = PAD[1] if ss else PAD[0]
    mx = (1 << bd) - 1
    out = np.zeros((len(blk), h, w), np.uint8 if bd == 8 else np.uint16)
    for i, b in enumerate(blk):
        px, py, q = block_glue(b, ss, bwidth, bheight)
        d = int(b["pred_direction"])
        compound = int(d == BI)
        tmp = np.zeros((h, w), np.int64)
        fx_tab, fy_tab = table_index(int(b["filter_x"]), w), table_index(int(b["filter_y"]), h)
        V = []
        for l in lists_of(d):
            ref = planes["ref0" if (l == 0 or same_plane) else "ref1"][plane_idx]
            win = window(ref, pad, px, py, q[l], w, h)
            sx, sy = q[l][0] & SUBPEL_MASK, q[l][1] & SUBPEL_MASK
            if unified:
                V.append(np_unified(win, taps, bd, sx, sy, fx_tab, fy_tab, w, h))
            else:
                res = np_convolve(win, taps, bd, sx, sy, fx_tab, fy_tab, w, h, compound, int(compound and l == 1), tmp, stats)
        if unified:
            res = np.clip(((((V[0] + 64) >> 7) + ((V[1] + 64) >> 7) >> 1) + 8) >> 4 if compound else (V[0] + 1024) >> 11, 0, mx)
        out[i] = res
    return out


def np_dist(pred, src_plane, ss, blk, metric):
    """[n] SAD / SSD of the predictions against the source blocks at the blocks' own origins"""
    pad = PAD[1] if ss else PAD[0]
    n, h, w = pred.shape
    out = np.zeros(n, np.int64)
    for i, b in enumerate(blk):
        x, y = int(b["x"]), int(b["y"])
        px, py = (((x >> 3) << 3) // 2, ((y >> 3) << 3) // 2) if ss else (x, y)
        d = pred[i].astype(np.int64) - src_plane[pad + py:pad + py + h, pad + px:pad + px + w].astype(np.int64)
        out[i] = (d * d).sum() if metric == SSD else np.abs(d).sum()
    return out


# ---- the cases ----------------------------------------------------------------------------------------------------------------------
def _mv(ip, frac8):
    return ip * 8 + frac8


def make_blocks(ss, bwidth, bheight, level, seed):
    """block records of one group.  level 2 (small shapes): every filter pair x every sub-pel class with rotating phases, the clamp
    on each side at each picture corner, BI_PRED with every class pairing, list-1-only blocks.  level 1: one block of each kind.
    level 0: the special contents' short list (sharp / regular 2-D at the half phase, compound, copy)"""
    rng = np.random.default_rng([0xB10C, ss, bwidth, bheight, level, seed])
    step = 8 if ss else 4
    xs, ys = np.arange(0, W - bwidth + 1, step), np.arange(0, H - bheight + 1, step)
    corners = [(0, 0), (W - bwidth, 0), (0, H - bheight), (W - bwidth, H - bheight)]
    # fractions in 1/8 luma: luma phases 2, 8, 14; with ss the odd ones give the chroma phases 1, 8 (mv 8 -> q 8), 15
    fr = (1, 8, 15) if ss else (1, 4, 7)
    unit = 16 if ss else 8                                     # vector units per plane sample

    def mvof(cls, k):
        """class 0 copy, 1 x, 2 y, 3 2-D; phases rotate with k; a whole part of a few samples"""
        ix, iy = int(rng.integers(-5, 6)), int(rng.integers(-5, 6))
        fx = fr[k % 3] if cls & 1 else 0
        fy = fr[(k // 3 + k) % 3] if cls & 2 else 0
        return ix * unit + fx, iy * unit + fy

    recs = []

    def add(x, y, mv0, mv1, d, fx, fy):
        r = np.zeros((), BLK_DTYPE)
        r["x"], r["y"], r["pred_direction"], r["filter_x"], r["filter_y"] = x, y, d, fx, fy
        r["mv"][0], r["mv"][1] = mv0, mv1
        recs.append(r)

    def pos(k):
        return int(xs[k % len(xs)]), int(ys[(k * 5 + 1) % len(ys)])

    if level == 0:
        k = 0
        for cls in (3, 1, 2, 0):
            for fpair in ((2, 2), (0, 0), (1, 2), (3, 0)):
                add(*pos(k), (mvof(cls, 1)), (0, 0), LIST0, *fpair)
                k += 1
        for c0, c1 in ((3, 3), (0, 3), (1, 2)):
            add(*pos(k), mvof(c0, 1), mvof(c1, 1), BI, 2, 2)
            k += 1
        return np.array(recs)
    if level == 1 and (bwidth >> ss) * (bheight >> ss) >= 1024:
        # large blocks: the tiling is what can go wrong; one block of each kind
        far_br = (12005, 12003)
        add(*pos(1), mvof(3, 1), (0, 0), LIST0, 2, 0)
        add(corners[3][0], corners[3][1], far_br, (0, 0), LIST0, 0, 1)
        add(corners[0][0], corners[0][1], (-(bwidth + 12) * 8 - 3, -(bheight + 12) * 8 - 1), (0, 0), LIST0, 1, 2)
        add(*pos(2), mvof(0, 2), mvof(3, 3), BI, 0, 2)
        add(*pos(3), mvof(1, 4), mvof(2, 5), BI, 2, 1)
        add(*pos(4), (0, 0), mvof(3, 6), LIST1, 1, 0)
        return np.array(recs)
    k = 0
    pairs = [(fx, fy) for fx in range(4) for fy in range(4)] if level == 2 else [(0, 2), (2, 1), (1, 3), (3, 0)]
    for i, fpair in enumerate(pairs):
        for cls in (range(4) if level == 2 else (i,)):
            add(*pos(k), mvof(cls, k), (0, 0), LIST0, *fpair)
            k += 1
    # the clamp: far outside (the fraction is discarded; 20001 * 2 wraps the int16 of a luma vector), and a few samples past each edge
    far = ((-12003, 5), (12005, -3), (7, -12001), (-5, 12003), (20001, 20003), (-20003, -20001))
    near = ((-(bwidth + 12) * 8 - 3, 3), ((bwidth + 12) * 8 + 5, -5), (3, -(bheight + 12) * 8 - 1), (-3, (bheight + 12) * 8 + 7))
    vs = far + near
    cl = [(c, vs[(2 * j + i) % 10]) for j, c in enumerate(corners) for i in range(5)] if level == 2 else [(corners[i % 4], vs[2 * i + 1]) for i in range(4)]
    for (x, y), v in cl:
        add(x, y, v, (0, 0), LIST0, k % 3, (k // 3) % 3)
        k += 1
    # corners with an ordinary 2-D vector
    for x, y in (corners if level == 2 else corners[3:]):
        add(x, y, mvof(3, k), (0, 0), LIST0, 0, 0)
        k += 1
    # BI_PRED: every class pairing (level 1: three of them)
    bi = [(a, c) for a in range(4) for c in range(4)] if level == 2 else [(0, 3), (3, 3), (1, 2)]
    for a, c in bi:
        add(*pos(k), mvof(a, k), mvof(c, k + 1), BI, k % 4, (k + 1) % 4)
        k += 1
    add(corners[3][0], corners[3][1], far[1], far[2], BI, 2, 0)
    # list 1 only
    for cls in ((3, 1, 2, 0) if level == 2 else (3,)):
        add(*pos(k), (0, 0), mvof(cls, k), LIST1, 2, 1)
        k += 1
    if ss:                                                     # a chroma origin off the 8-grid: (x >> 3) << 3 of :1310
        add(12, 4, mvof(3, k), (0, 0), LIST0, 0, 0)
    return np.array(recs)


def group_list():
    """(bd, content, ss, bwidth, bheight, same_plane, plane, level) of every fixture group"""
    g = []
    for bd in (8, 10):
        for bw in SIDES:
            for bh in SIDES:
                small = bw * bh <= 64 or (bw, bh) == (16, 16)
                g.append((bd, 0, 0, bw, bh, 0, 0, 2 if small and (bd == 8 or bw == bh) else 1))
                if bw >= 8 and bh >= 8:
                    small_c = bw * bh <= 256
                    g.append((bd, 0, 1, bw, bh, 0, 1 + (bw + bh) // 8 % 2, 2 if small_c and bd == 8 else 1))
        g.append((bd, 0, 0, 8, 8, 1, 0, 1))                   # BI_PRED with both lists on one plane
        g.append((bd, 0, 1, 16, 16, 1, 2, 1))
        for content in (1, 2, 3):
            for ss, bw, bh, plane in ((0, 8, 8, 0), (0, 4, 4, 0), (0, 16, 4, 0), (1, 8, 8, 1)):
                g.append((bd, content, ss, bw, bh, 0, plane, 0))
    return g


def generate(predict):
    """the fixture but for the taps.  predict(bd, content, ss, plane, bwidth, bheight, blk, same_plane) -> [n, h, w]"""
    z = {}
    groups = group_list()
    z["groups"] = np.array([g[:7] for g in groups], np.int32)
    crc = []
    for bd in (8, 10):
        for c in CONTENTS:
            crc.append(planes_crc(make_planes(bd, c)))
    z["planes_crc"] = np.array(crc, np.uint32)
    for gi, (bd, content, ss, bw, bh, same, plane, level) in enumerate(groups):
        blk = make_blocks(ss, bw, bh, level, gi)
        z[f"blk_{gi}"] = blk.view(np.uint8).reshape(len(blk), 16)
        z[f"pred_{gi}"] = predict(bd, CONTENTS[content], ss, plane, bw, bh, blk, bool(same))
    return z


def blocks_of(z, gi):
    return z[f"blk_{gi}"].copy().view(BLK_DTYPE).reshape(-1)


_planes = {}


def planes_of(bd, content):
    if (bd, content) not in _planes:
        _planes[(bd, content)] = make_planes(bd, content)
    return _planes[(bd, content)]


def np_predictor(taps, stats=None, unified=False):
    return lambda bd, content, ss, plane, bw, bh, blk, same: np_inter_pred(taps, planes_of(bd, content), bd, ss, plane, bw, bh, blk, same, stats, unified)


def ref_predictor(R, stats=None):
    return lambda bd, content, ss, plane, bw, bh, blk, same: ref_inter_pred(R, planes_of(bd, content), bd, ss, plane, bw, bh, blk, same, stats)


def new_stats():
    return {"entries": set(), "tables": set(), "clip0": 0, "clipmax": 0}


def random_case(rng):
    """(bd, ss, plane, bwidth, bheight, blk[1]) anywhere in the parameter space, vectors up to far outside"""
    bd, ss = int(rng.choice((8, 10))), int(rng.integers(0, 2))
    sides = SIDES[1:] if ss else SIDES
    bw, bh = int(rng.choice(sides)), int(rng.choice(sides))
    r = np.zeros(1, BLK_DTYPE)
    step = 4
    r["x"], r["y"] = int(rng.integers(0, (W - bw) // step + 1)) * step, int(rng.integers(0, (H - bh) // step + 1)) * step
    span = int(rng.choice((40, 400, 3000, 32767)))
    r["mv"] = rng.integers(-span, span + 1, (1, 2, 2))
    r["pred_direction"], r["filter_x"], r["filter_y"] = rng.integers(0, 3), rng.integers(0, 4), rng.integers(0, 4)
    return bd, ss, (int(rng.integers(1, 3)) if ss else 0), bw, bh, r


def check_unified(R, taps, n=300):
    """the device's single body against the compiled entries, on random cases over all sixteen entries"""
    rng = np.random.default_rng(0x0D17)
    stats = new_stats()
    for _ in range(n):
        bd, ss, plane, bw, bh, blk = random_case(rng)
        p = planes_of(bd, "random")
        a = ref_inter_pred(R, p, bd, ss, plane, bw, bh, blk, False, stats)
        b = np_inter_pred(taps, p, bd, ss, plane, bw, bh, blk, unified=True)
        c = np_inter_pred(taps, p, bd, ss, plane, bw, bh, blk)
        assert np.array_equal(a, b) and np.array_equal(a, c), (bd, ss, bw, bh, blk)
    assert sorted(stats["entries"]) == ALL_ENTRIES, sorted(stats["entries"])


def check_conditions(z, taps):
    """conditions on the fixture, not measurements: clips on both sides, every entry and every table reached, every shape present"""
    stats = new_stats()
    for gi, row in enumerate(z["groups"]):
        bd, content, ss, bw, bh, same, plane = (int(v) for v in row)
        blk = blocks_of(z, gi)
        pred = np_inter_pred(taps, planes_of(bd, CONTENTS[content]), bd, ss, plane, bw, bh, blk, bool(same), stats)
        assert np.array_equal(pred, z[f"pred_{gi}"]), gi
        for b in blk:                                          # the entries and tables the fixture reaches, from the glue
            _, _, q = block_glue(b, ss, bw, bh)
            for l in lists_of(b["pred_direction"]):
                sx, sy = q[l][0] & 15, q[l][1] & 15
                stats["entries"].add(entry_name(bd, sx, sy, int(b["pred_direction"]) == BI))
                if sx:
                    stats["tables"].add(table_index(int(b["filter_x"]), bw >> ss))
                if sy:
                    stats["tables"].add(table_index(int(b["filter_y"]), bh >> ss))
    assert stats["clip0"] > 0 and stats["clipmax"] > 0, stats
    assert sorted(stats["entries"]) == ALL_ENTRIES, sorted(stats["entries"])
    assert stats["tables"] == set(range(6)), stats["tables"]
    shapes = {(int(r[2]), int(r[3]), int(r[4])) for r in z["groups"]}
    assert {(0, a, b) for a in SIDES for b in SIDES} | {(1, a, b) for a in SIDES[1:] for b in SIDES[1:]} <= shapes
    return stats


def main():
    R = ref_lib()
    assert R is not None, "oracle/_ref/libsvtref.so is not built"
    taps = record_taps(R)
    check_unified(R, taps)
    stats = new_stats()
    z = generate(ref_predictor(R, stats))
    z["taps"] = taps
    assert sorted(stats["entries"]) == ALL_ENTRIES and stats["tables"] == set(range(6)), stats
    zn = generate(np_predictor(taps))
    for k, v in zn.items():
        assert v.dtype == z[k].dtype and np.array_equal(v, z[k]), k
    st = check_conditions(z, taps)
    np.savez_compressed(OUT, **z)
    n = sum(len(z[f"blk_{gi}"]) for gi in range(len(z["groups"])))
    print(f"wrote {OUT}: {len(z['groups'])} groups, {n} blocks, {os.path.getsize(OUT)} bytes; clips at 0 / max: {st['clip0']} / {st['clipmax']}")
    assert os.path.getsize(OUT) < 1 << 20


if __name__ == "__main__":
    main()

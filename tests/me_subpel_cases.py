"""Sub-pel motion estimation in plain numpy: the half- and quarter-pel refinement of MotionEstimateLcu (EbMotionEstimation.c:8162-8236)
and the bi-prediction on fractional vectors (:6210-6632), restated sample by sample.  tests/test_me_subpel_cpu.py holds it equal to the
reference's own output (tests/golden/me_subpel.npz); the GPU tests use it on shapes the fixture does not hold.

Coordinates are absolute: (y, x) of a reference picture's integer sample grid, sample (0, 0) the picture's own.  The three half-pel
planes are position-invariant functions of the reference picture (taps (-2, 18, 18, -2), + 16 >> 5, clipped to 8 bits):
  B(y, x)  the half-pel sample LEFT of (y, x):   taps over I[y][x - 2 .. x + 1]
  H(y, x)  the half-pel sample ABOVE (y, x):     taps over I[y - 2 .. y + 1][x]
  J(y, x)  the sample above-left of (y, x):      the vertical taps over the ROUNDED B[y - 2 .. y + 1][x]
and the reference's pos_b / pos_h / pos_j pointers of a search area (:8194-8201: pos_b + 2 * stride, pos_h + 1, pos_j) hold exactly
B / H / J at the absolute position of each search point."""
import ctypes
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = os.path.join(ROOT, "tests", "golden", "me_subpel.npz")
REF_LIB = os.path.join(ROOT, "oracle", "_ref", "libsvtref_me_subpel.so")

SUB_SAD, FULL_SAD, SSD = 0, 1, 2
PUS, PUS_ALL = 85, 209
MAX_SAD = 128 * 128 * 255
# sub-pel directions (EbMotionEstimation.h:63-70)
TL, T, TR, R, BR, B_, BL, L = range(8)
# evaluation order of the eight neighbours: L R T B TL TR BR BL
EVAL_DIR = (L, R, T, B_, TL, TR, BR, BL)
EVAL_DXY = ((-1, 0), (1, 0), (0, -1), (0, 1), (-1, -1), (1, -1), (1, 1), (-1, 1))
# psubPelDirection: the first equality in the order L R T B TL TR BL BR (:3795-3821), as indices into the evaluation order
DIR_ORDER = (0, 1, 2, 3, 4, 5, 7, 6)
# half-pel neighbours as (plane, dy, dx) at the full-pel winner, evaluation order
HALF_POS = (("B", 0, 0), ("B", 0, 1), ("H", 0, 0), ("H", 1, 0), ("J", 0, 0), ("J", 0, 1), ("J", 1, 1), ("J", 1, 0))
# SetQuarterPelRefinementInputsOnTheFly (:4655): per case, per neighbour (evaluation order), the two planes averaged
QUARTER_POS = (
    ((("B", 0, 0), ("F", 0, 0)), (("F", 0, 0), ("B", 0, 1)), (("H", 0, 0), ("F", 0, 0)), (("F", 0, 0), ("H", 1, 0)),
     (("B", 0, 0), ("H", 0, 0)), (("H", 0, 0), ("B", 0, 1)), (("H", 1, 0), ("B", 0, 1)), (("B", 0, 0), ("H", 1, 0))),
    ((("F", 0, -1), ("B", 0, 0)), (("B", 0, 0), ("F", 0, 0)), (("J", 0, 0), ("B", 0, 0)), (("B", 0, 0), ("J", 1, 0)),
     (("H", 0, -1), ("B", 0, 0)), (("B", 0, 0), ("H", 0, 0)), (("B", 0, 0), ("H", 1, 0)), (("H", 1, -1), ("B", 0, 0))),
    ((("J", 0, 0), ("H", 0, 0)), (("H", 0, 0), ("J", 0, 1)), (("F", -1, 0), ("H", 0, 0)), (("H", 0, 0), ("F", 0, 0)),
     (("B", -1, 0), ("H", 0, 0)), (("H", 0, 0), ("B", -1, 1)), (("H", 0, 0), ("B", 0, 1)), (("B", 0, 0), ("H", 0, 0))),
    ((("H", 0, -1), ("J", 0, 0)), (("J", 0, 0), ("H", 0, 0)), (("B", -1, 0), ("J", 0, 0)), (("J", 0, 0), ("B", 0, 0)),
     (("H", 0, -1), ("B", -1, 0)), (("B", -1, 0), ("H", 0, 0)), (("B", 0, 0), ("H", 0, 0)), (("H", 0, -1), ("B", 0, 0))),
)
# valid* of PU_QuarterPelRefinementOnTheFly (:4396-4418): [half-pel winner fractional][neighbour, evaluation order] -> directions
QUARTER_VALID = (
    ((BL, L, TL), (TR, R, BR), (TL, T, TR), (BR, B_, BL), (L, TL, T), (T, TR, R), (R, BR, B_), (B_, BL, L)),
    ((TR, R, BR), (BL, L, TL), (BR, B_, BL), (TL, T, TR), (R, BR, B_), (B_, BL, L), (L, TL, T), (T, TR, R)),
)
# QuarterPelCompensation (:6236-6302) / SelectBuffer (:6181): fractional position -> the one or two planes, as (plane, dy, dx) at the
# vector's integer part (there pos_b / pos_h / pos_j are the samples right of, below and below-right of it)
BIPRED_POS = {0: (("F", 0, 0),), 2: (("B", 0, 1),), 8: (("H", 1, 0),), 10: (("J", 1, 1),),
              1: (("F", 0, 0), ("B", 0, 1)), 3: (("B", 0, 1), ("F", 0, 1)), 4: (("F", 0, 0), ("H", 1, 0)), 5: (("B", 0, 1), ("H", 1, 0)),
              6: (("B", 0, 1), ("J", 1, 1)), 7: (("B", 0, 1), ("H", 1, 1)), 9: (("H", 1, 0), ("J", 1, 1)), 11: (("J", 1, 1), ("H", 1, 1)),
              12: (("H", 1, 0), ("F", 1, 0)), 13: (("H", 1, 0), ("B", 1, 1)), 14: (("J", 1, 1), ("B", 1, 1)), 15: (("H", 1, 1), ("B", 1, 1))}
# what the refinement and the bi-prediction read of a reference beyond the picture (derived in csrc/me_subpel_plan.h)
MARGIN = 66


def pu_rect(n):
    """(x, y, w, h) in samples of the PU at index n of the result rows (EbMeTierZeroPu order): csrc/kernel_me_steps.h me_pu_rect"""
    def z16(z):
        return ((z >> 2) & 1) * 2 + (z & 1), (z >> 3) * 2 + ((z >> 1) & 1)
    if n == 0:
        r = (0, 0, 8, 8)
    elif n < 5:
        q = n - 1; r = ((q & 1) * 4, (q >> 1) * 4, 4, 4)
    elif n < 21:
        bx, by = z16(n - 5); r = (bx * 2, by * 2, 2, 2)
    elif n < 85:
        i = n - 21; bx, by = z16(i >> 2); r = (bx * 2 + (i & 1), by * 2 + ((i >> 1) & 1), 1, 1)
    elif n < 87:
        r = (0, (n - 85) * 4, 8, 4)
    elif n < 95:
        i = n - 87; q = i >> 1; r = ((q & 1) * 4, (q >> 1) * 4 + (i & 1) * 2, 4, 2)
    elif n < 127:
        i = n - 95; bx, by = z16(i >> 1); r = (bx * 2, by * 2 + (i & 1), 2, 1)
    elif n < 129:
        r = ((n - 127) * 4, 0, 4, 8)
    elif n < 137:
        i = n - 129; q = i >> 1; r = ((q & 1) * 4 + (i & 1) * 2, (q >> 1) * 4, 2, 4)
    elif n < 169:
        i = n - 137; bx, by = z16(i >> 1); r = (bx * 2 + (i & 1), by * 2, 1, 2)
    elif n < 185:
        i = n - 169; m = i >> 1; q = m >> 1; r = ((q & 1) * 4, (q >> 1) * 4 + (m & 1) * 2 + (i & 1), 4, 1)
    elif n < 201:
        i = n - 185; q = i >> 2; r = ((q & 1) * 4 + (i & 3), (q >> 1) * 4, 1, 4)
    elif n < 205:
        r = (0, (n - 201) * 2, 8, 2)
    else:
        r = ((n - 205) * 2, 0, 2, 8)
    return tuple(8 * v for v in r)


CLASS_STARTS = (0, 1, 5, 21, 85, 87, 95, 127, 129, 137, 169, 185, 201, 205, 209)


def raster_to_storage():
    """index in the result rows of raster PU p (the order of me_results): inside each shape class the raster order is row-major"""
    out = []
    for a, b in zip(CLASS_STARTS[:-1], CLASS_STARTS[1:]):
        out += sorted(range(a, b), key=lambda n: (pu_rect(n)[1], pu_rect(n)[0]))
    return out


RASTER = raster_to_storage()


def mv_xy(mv):
    x, y = int(mv) & 0xffff, (int(mv) >> 16) & 0xffff
    return x - 65536 if x >= 32768 else x, y - 65536 if y >= 32768 else y


def pack_mv(x, y):
    return ((y & 0xffff) << 16) | (x & 0xffff)


def _taps(a0, a1, a2, a3):
    return np.clip((-2 * a0 + 18 * a1 + 18 * a2 - 2 * a3 + 16) >> 5, 0, 255)


class Planes:
    """I / B / H / J of one padded reference picture, addressed by absolute coordinates"""

    def __init__(self, padded, origin_x, origin_y):
        i = padded.astype(np.int32)
        self.ox, self.oy = origin_x, origin_y
        h, w = i.shape
        b = np.zeros_like(i); hh = np.zeros_like(i); j = np.zeros_like(i)
        b[:, 2:w - 1] = _taps(i[:, 0:w - 3], i[:, 1:w - 2], i[:, 2:w - 1], i[:, 3:w])
        hh[2:h - 1] = _taps(i[0:h - 3], i[1:h - 2], i[2:h - 1], i[3:h])
        j[2:h - 1] = _taps(b[0:h - 3], b[1:h - 2], b[2:h - 1], b[3:h])
        self.p = {"F": i, "B": b, "H": hh, "J": j}

    def get(self, kind, y, x, h, w):
        y += self.oy; x += self.ox
        a = self.p[kind]
        # B needs 2 columns to the left and 1 to the right; H / J 2 rows above and 1 below (J one more row of B each way)
        assert y >= 4 and x >= 2 and y + h + 3 <= a.shape[0] and x + w + 1 <= a.shape[1], (kind, y, x, h, w, a.shape)
        return a[y:y + h, x:x + w]


def _dist(method, src, pred):
    if method == SSD:
        return int(((src - pred) ** 2).sum())
    if method == SUB_SAD:
        return 2 * int(np.abs(src[::2] - pred[::2]).sum())
    return int(np.abs(src - pred).sum())


def _half_sse(src, pred):
    """the SSE of the half-pel pass as spatial_full_distortion_kernel_func_ptr_array[..][Log2f(width) - 2] computes it (both asm rows hold
    the same SSSE3 kernels): the difference wraps to 8 bits before it is squared (_mm_sub_epi8 / _mm_sign_epi8: |d| above 128 counts as
    256 - |d|), and the 8-wide kernel sums 8 rows whatever the PU's height (8x16 and 8x32 PUs are measured on their upper 8x8)"""
    if src.shape[1] == 8:
        src, pred = src[:8], pred[:8]
    d = np.abs(src - pred)
    d = np.where(d > 128, 256 - d, d)
    return int((d * d).sum())


def _avg(a, b):
    return (a + b + 1) >> 1


def stage_enabled(n, npus, flags):
    """(half-pel runs, quarter-pel runs) for the PU at row index n; flags = (fractional_search64x64, half32, half16, half8, quarter,
    disable8x8)"""
    f64, h32, h16, h8, qp, no8 = flags
    if n >= npus:
        return False, False
    if n == 0:
        return bool(f64), bool(f64)
    if n < 5:
        return bool(h32), bool(qp)
    if n < 21:
        return bool(h16), bool(qp)
    if n < 85:
        return bool(h8) and not no8, bool(qp) and not no8
    return True, True


def refine_sb(pl, src_sb, sbx, sby, xo, yo, npus, method, flags, sad, mv, do_quarter=True, cover=None):
    """the refinement of one SB against one reference.  pl: Planes of the reference; src_sb: the SB's 64x64 source samples (padding
    included for a partial SB); (sbx, sby): the SB's origin; (xo, yo): its search-area origin; sad / mv: [209] full-pel rows.
    -> dict half_sad / half_mv / half_ssd / half_dir and sad / mv / ssd after the quarter-pel pass"""
    src_sb = src_sb.astype(np.int32)
    sad = [int(v) for v in sad]; mv = [int(v) for v in mv]
    ssd = [0] * PUS_ALL; dirn = [0] * PUS_ALL
    for n in range(npus):
        if not stage_enabled(n, npus, flags)[0]:
            continue
        px, py, w, h = pu_rect(n)
        s = src_sb[py:py + h, px:px + w]
        xm, ym = mv_xy(mv[n])
        X, Y = sbx + px + (xm >> 2), sby + py + (ym >> 2)
        if method == SSD:
            ssd[n] = _half_sse(s, pl.get("F", Y, X, h, w))
        d = []
        for k, (kind, dy, dx) in enumerate(HALF_POS):
            pred = pl.get(kind, Y + dy, X + dx, h, w)
            dk = _half_sse(s, pred) if method == SSD else _dist(method, s, pred)
            d.append(dk)
            if method == SSD:
                if dk < ssd[n]:
                    sad[n], ssd[n], mv[n] = _dist(FULL_SAD, s, pred), dk, pack_mv(xm + 2 * EVAL_DXY[k][0], ym + 2 * EVAL_DXY[k][1])
                    if cover is not None:
                        cover["ssd_update"] += 1
                elif cover is not None:
                    cover["ssd_keep"] += 1
            elif dk < sad[n]:
                sad[n], mv[n] = dk, pack_mv(xm + 2 * EVAL_DXY[k][0], ym + 2 * EVAL_DXY[k][1])
        best = min(d)
        dirn[n] = EVAL_DIR[next(k for k in DIR_ORDER if d[k] == best)]
        if cover is not None:
            sx, sy = (xm >> 2) - xo, (ym >> 2) - yo
            cover["winner"].append((sx, sy))
    out = dict(half_sad=np.array(sad, np.uint32), half_mv=np.array(mv, np.uint32), half_ssd=np.array(ssd, np.uint32), half_dir=np.array(dirn, np.uint8))
    if do_quarter:
        for n in range(npus):
            if not stage_enabled(n, npus, flags)[1]:
                continue
            px, py, w, h = pu_rect(n)
            if n == 0:
                w = h = 32                                    # the reference measures a 32x32 block for the 64x64 PU (:4809)
            s = src_sb[py:py + h, px:px + w]
            xm, ym = mv_xy(mv[n])
            case = (ym & 2) + ((xm & 2) >> 1)
            X, Y = sbx + px + ((xm + 2) >> 2), sby + py + ((ym + 2) >> 2)
            valid = QUARTER_VALID[1 if case else 0]
            if cover is not None:
                cover["quarter_case"][case][1 if case else 0] += 1
            for k in range(8):
                if dirn[n] not in valid[k]:
                    continue
                (k1, dy1, dx1), (k2, dy2, dx2) = QUARTER_POS[case][k]
                pred = _avg(pl.get(k1, Y + dy1, X + dx1, h, w), pl.get(k2, Y + dy2, X + dx2, h, w))
                dk = _dist(method, s, pred)
                nmv = pack_mv(xm + EVAL_DXY[k][0], ym + EVAL_DXY[k][1])
                if method == SSD:
                    if dk < ssd[n]:
                        sad[n], ssd[n], mv[n] = _dist(FULL_SAD, s, pred), dk, nmv
                elif dk < sad[n]:
                    sad[n], mv[n] = dk, nmv
    out.update(sad=np.array(sad, np.uint32), mv=np.array(mv, np.uint32), ssd=np.array(ssd, np.uint32))
    return out


def frac_block(pl, Y, X, frac, h, w):
    """the compensated block of one list: SelectBuffer for integer / half positions, QuarterPelCompensation's rounded average else"""
    planes = BIPRED_POS[frac]
    blk = pl.get(planes[0][0], Y + planes[0][1], X + planes[0][2], h, w)
    if len(planes) == 2:
        blk = _avg(blk, pl.get(planes[1][0], Y + planes[1][1], X + planes[1][2], h, w))
    return blk


def bipred_sb(pl0, pl1, src_sb, sbx, sby, npus, sub_sad, bipred_all, sad0, mv0, sad1, mv1, cover=None):
    """BiPredictionSearch on refined vectors and the me_results rows (:8250-8420).  pl1 None: a P picture.
    -> bipred_sad [209] (row order), results [209][11] (raster order; the columns of oracle/ref_me.c)"""
    src_sb = src_sb.astype(np.int32)
    bip = np.zeros(PUS_ALL, np.uint32)
    res = np.zeros((PUS_ALL, 11), np.int64)
    two = pl1 is not None
    for p in range(npus):
        n = RASTER[p]
        px, py, w, h = pu_rect(n)
        x0, y0 = mv_xy(mv0[n])
        x1, y1 = mv_xy(mv1[n]) if two else (0, 0)
        l0, l1 = int(sad0[n]), int(sad1[n]) if two else 0
        has_bi = two and (bipred_all or p < 21)
        if has_bi:
            s = src_sb[py:py + h, px:px + w]
            f0, f1 = (x0 & 3) + ((y0 & 3) << 2), (x1 & 3) + ((y1 & 3) << 2)
            if cover is not None:
                cover["bipred_frac"][0][f0] += 1; cover["bipred_frac"][1][f1] += 1
            a = frac_block(pl0, sby + py + (y0 >> 2), sbx + px + (x0 >> 2), f0, h, w)
            b = frac_block(pl1, sby + py + (y1 >> 2), sbx + px + (x1 >> 2), f1, h, w)
            bip[n] = _dist(SUB_SAD if sub_sad else FULL_SAD, s, _avg(a, b))
        bi = int(bip[n])
        d = (l0, l1, bi)
        if has_bi:
            total = 3
            if l0 <= l1 and l0 <= bi:
                order = (0, 1, 2) if l1 <= bi else (0, 2, 1)
            elif l1 <= l0 and l1 <= bi:
                order = (1, 0, 2) if l0 <= bi else (1, 2, 0)
            else:
                order = (2, 0, 1) if l0 <= l1 else (2, 1, 0)
        elif two:
            total, order = 2, ((0, 1, 2) if l0 <= l1 else (1, 0, 2))
        else:
            total, order = 1, (0, 1, 2)
        res[p, 0:4] = (x0, y0, x1, y1)
        for k in range(total):
            res[p, 4 + 2 * k], res[p, 5 + 2 * k] = d[order[k]], order[k]
        res[p, 10] = total
    return bip, res


def padded(luma, pad=68):
    return np.pad(luma, pad, mode="edge"), pad


def ref_lib():
    """oracle/_ref/libsvtref_me_subpel.so (tests/golden/make_golden_me_subpel.py builds it), or None"""
    if not os.path.exists(REF_LIB):
        return None
    L = ctypes.CDLL(REF_LIB)
    L.ref_me_subpel_stage.restype = ctypes.c_int
    L.ref_me_subpel_lcu.restype = ctypes.c_int
    return L


def ptr(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def run_ref_stage(L, src_pad, ref_pad, pad, sbx, sby, xo, yo, saw, sah, flg, sad, mv, plane_wh=None):
    """ref_me_subpel_stage on one SB -> dict (half_*, quarter sad / mv / ssd, planes or None)"""
    assert src_pad.flags.c_contiguous and ref_pad.flags.c_contiguous
    o = {k: np.zeros(PUS_ALL, np.uint32) for k in ("half_sad", "half_mv", "half_ssd", "sad", "mv", "ssd")}
    o["half_dir"] = np.zeros(PUS_ALL, np.uint8)
    planes = np.zeros((3, plane_wh[1], plane_wh[0]), np.uint8) if plane_wh else None
    flg = np.array(flg, np.int32)
    sad = np.ascontiguousarray(sad, np.uint32); mv = np.ascontiguousarray(mv, np.uint32)
    s_at = src_pad.ctypes.data + (pad + sby) * src_pad.shape[1] + pad + sbx
    r_at = ref_pad.ctypes.data + (pad + sby) * ref_pad.shape[1] + pad + sbx
    rc = L.ref_me_subpel_stage(ctypes.c_void_p(s_at), src_pad.shape[1], ctypes.c_void_p(r_at), ref_pad.shape[1], xo, yo, saw, sah, ptr(flg), ptr(sad), ptr(mv),
                               ptr(o["half_sad"]), ptr(o["half_mv"]), ptr(o["half_ssd"]), ptr(o["half_dir"]), ptr(o["sad"]), ptr(o["mv"]), ptr(o["ssd"]),
                               ptr(planes) if plane_wh else None, plane_wh[0] if plane_wh else 0, plane_wh[1] if plane_wh else 0)
    assert rc == 0, rc
    o["planes"] = planes
    return o

"""Loop restoration: what the fixture generator (tests/golden/make_golden_lr.py) and the tests share - the harness library's
bindings, the fixture's cases, and a plain numpy model of the filters written from the rules in include/svt_hip_dsp.h (the two-operand
halo rule, the unit and stripe grids, the Wiener and self-guided arithmetic, the statistics).  The model is the project's; that it
equals the reference's pictures is what tests/test_lr_cpu.py checks, so a disagreement between the kernels and the fixture can be
told from a misreading of the reference."""
import ctypes
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = os.path.join(ROOT, "tests", "golden", "lr.npz")
REF_LR = os.path.join(ROOT, "oracle", "_ref", "libsvtref_lr.so")
PLANES = ("y", "cb", "cr")

UNIT_DTYPE = np.dtype([("type", "<i4"), ("vfilter", "<i2", 3), ("hfilter", "<i2", 3), ("xqd", "<i2", 2), ("ep", "<i4")])      # svt_hip_lr_unit
CAND_DTYPE = np.dtype([("pic", "<u4"), ("plane", "<u4"), ("unit", "<u4"), ("u", UNIT_DTYPE)])                                  # svt_hip_lr_cand
REF_RESULT = np.dtype([("sse", "<i8", 3), ("vfilter", "<i4", 3), ("hfilter", "<i4", 3), ("ep", "<i4"), ("xqd", "<i4", 2), ("pad", "<i4")])   # ref_lr_result
RESULT_DTYPE = np.dtype([("sse", "<i8", 3), ("vfilter", "<i2", 3), ("hfilter", "<i2", 3), ("xqd", "<i2", 2), ("ep", "<i4"), ("pad", "<i4")])   # svt_hip_lr_result
COSTS_DTYPE = np.dtype([("rdmult", "<i4"), ("wiener_restore_cost", "<i4", 2), ("sgrproj_restore_cost", "<i4", 2), ("switchable_restore_cost", "<i4", 3)])
REF_REC = np.dtype([("type", "<i4"), ("vfilter", "<i4", 3), ("hfilter", "<i4", 3), ("ep", "<i4"), ("xqd", "<i4", 2)])           # ref_lr_rec

TAP_MIN, TAP_MAX = (-5, -23, -17), (10, 8, 46)
XQD_MIN, XQD_MAX = (-96, -32), (31, 95)
SGR_R = ((2, 1),) * 10 + ((0, 1),) * 4 + ((2, 0),) * 2
SGR_S = ((140, 3236), (112, 2158), (93, 1618), (80, 1438), (70, 1295), (58, 1177), (47, 1079), (37, 996), (30, 925), (25, 863),
         (-1, 2589), (-1, 1618), (-1, 1177), (-1, 925), (56, -1), (22, -1))
X_BY_XPLUS1 = np.array([1, 128, 171, 192, 205, 213, 219, 224, 228, 230, 233, 235, 236, 238, 239, 240, 241, 242, 243, 243, 244, 244, 245, 245, 246, 246] +
                       [247] * 4 + [248] * 4 + [249] * 5 + [250] * 7 + [251] * 10 + [252] * 17 + [253] * 29 + [254] * 68 + [255] * 85 + [256], np.int64)
assert len(X_BY_XPLUS1) == 256


def to_units(ref_recs):
    """REF_REC records -> UNIT_DTYPE records"""
    u = np.zeros(len(ref_recs), UNIT_DTYPE)
    for f in ("type", "vfilter", "hfilter", "xqd", "ep"):
        u[f] = ref_recs[f]
    return u


# ---- the harness library -------------------------------------------------------------------------------------------------------
_lib = []


def ref_lr():
    """the harness library, or None when it is not built"""
    if not _lib:
        L = None
        if os.path.exists(REF_LR):
            L = ctypes.CDLL(REF_LR)
            vp, ci = ctypes.c_void_p, ctypes.c_int
            L.ref_lr_new.restype = vp
            L.ref_lr_new.argtypes = [ci, ci, ci, vp, vp, vp, vp]
            L.ref_lr_free.argtypes = [vp]
            L.ref_lr_free.restype = None
            L.ref_lr_grid.argtypes = [vp, ci, vp]
            L.ref_lr_limits.argtypes = [vp, ci, ci, vp]
            L.ref_lr_frame.argtypes = [vp, ci, vp, vp, vp]
            L.ref_lr_try.argtypes = [vp, ci, ci, ci, vp]
            L.ref_lr_try.restype = ctypes.c_int64
            L.ref_lr_stats.argtypes = [vp, ci, ci, ci, ci, vp, vp]
            L.ref_lr_search_wiener.argtypes = [vp, ci, ci, ci, ci, vp, vp, vp, ci]
            L.ref_lr_finish.argtypes = [vp, ci, vp, vp, vp, vp]
        _lib.append(L)
    return _lib[0]


def _ptrs(planes):
    return (ctypes.c_void_p * 3)(*[p.ctypes.data for p in planes])


class RefPicture:
    """one picture (deblocked, CDEF output, source) with its unit sizes inside the harness"""

    def __init__(self, w, h, bd, unit_size, dblk, cdef, src):
        self.L = ref_lr()
        self.w, self.h, self.bd = w, h, bd
        self.keep = [[np.ascontiguousarray(p) for p in planes] for planes in (dblk, cdef, src)]
        us = (ctypes.c_int32 * 3)(*unit_size)
        self.ctx = self.L.ref_lr_new(w, h, bd, us, *[_ptrs(k) for k in self.keep])
        assert self.ctx

    def close(self):
        self.L.ref_lr_free(self.ctx)
        self.ctx = None

    def grid(self, plane):
        """(horz_units_per_tile, vert_units_per_tile, units_per_tile, units the visitor visits)"""
        out = (ctypes.c_int32 * 4)()
        assert self.L.ref_lr_grid(self.ctx, plane, out) == 0
        return tuple(out)

    def limits(self, plane, unit):
        out = (ctypes.c_int32 * 4)()
        assert self.L.ref_lr_limits(self.ctx, plane, unit, out) == 0
        return tuple(out)

    def frame(self, frame_type, units, flavour=0):
        """units: per plane REF_REC records -> the three restored planes"""
        units = [np.ascontiguousarray(u, REF_REC) for u in units]
        out = [np.zeros_like(p) for p in self.keep[1]]
        ft = (ctypes.c_int32 * 3)(*frame_type)
        assert self.L.ref_lr_frame(self.ctx, flavour, ft, _ptrs(units), _ptrs(out)) == 0
        return out

    def try_unit(self, plane, unit, rec, flavour=0):
        r = np.ascontiguousarray(rec, REF_REC).reshape(1)
        return int(self.L.ref_lr_try(self.ctx, flavour, plane, unit, r.ctypes.data))

    def search_wiener(self, plane, unit, wn_filter_mode, flavour=0):
        """search_wiener_seg whole -> (final taps [6]: vfilter 0 .. 2, hfilter 0 .. 2; sse, INT64_MAX when compute_score rejects; the taps
        of every trial in order [n, 6])"""
        taps, sse, trials = np.zeros(6, np.int16), np.zeros(1, np.int64), np.zeros((256, 6), np.int16)
        n = self.L.ref_lr_search_wiener(self.ctx, flavour, plane, unit, wn_filter_mode, taps.ctypes.data, sse.ctypes.data, trials.ctypes.data, 256)
        assert n >= 0
        return taps, int(sse[0]), trials[:n].copy()

    def finish(self, wn_filter_mode, costs, results):
        """rest_finish_search whole.  costs: 8 ints (rdmult, wiener[2], sgrproj[2], switchable[3]); results: per plane RESULT_DTYPE records
        -> (frame types [3], per plane UNIT_DTYPE records as copy_unit_info left them)"""
        ins = []
        for r in results:
            a = np.zeros(len(r), REF_RESULT)
            for f in ("sse", "vfilter", "hfilter", "ep", "xqd"):
                a[f] = r[f]
            ins.append(a)
        outs = [np.zeros(len(r), REF_REC) for r in results]
        types = np.zeros(3, np.int32)
        cs = np.ascontiguousarray(costs, np.int32)
        assert self.L.ref_lr_finish(self.ctx, wn_filter_mode, cs.ctypes.data, _ptrs(ins), types.ctypes.data, _ptrs(outs)) == 0
        return types.tolist(), [to_units(o) for o in outs]

    def stats(self, plane, unit, win, flavour=0):
        M, H = np.zeros(win * win, np.int64), np.zeros((win * win, win * win), np.int64)
        assert self.L.ref_lr_stats(self.ctx, flavour, plane, unit, win, M.ctypes.data, H.ctypes.data) == 0
        return M, H


# ---- the fixture ---------------------------------------------------------------------------------------------------------------
_fix = []


def fixture():
    if not _fix:
        _fix.append(np.load(FIXTURE))
    return _fix[0]


def case_names():
    return [str(s) for s in fixture()["cases"]]


def picture(g, pic):
    dblk = [g[f"{pic}_dblk_{p}"] for p in PLANES]
    cdef = [(d.astype(np.int32) + g[f"{pic}_dcdef_{p}"]).astype(d.dtype) for d, p in zip(dblk, PLANES)]
    src = [(d.astype(np.int32) + g[f"{pic}_dsrc_{p}"]).astype(d.dtype) for d, p in zip(dblk, PLANES)]
    return dblk, cdef, src


def case(name):
    """-> dict: w, h, bd, unit_size, frame_type, win, dblk / cdef / src / out (three planes each), units (UNIT_DTYPE, the planes' blocks one
    after another), offsets (where each plane's block starts, and the total), cands (CAND_DTYPE) with sse, M / H per unit"""
    g = fixture()
    pic = str(g[name + "_pic"])
    par = g[name + "_params"]
    w, h, bd = (int(v) for v in par[:3])
    dblk, cdef, src = picture(g, pic)
    out = [(c.astype(np.int32) + g[f"{name}_diff_{p}"]).astype(c.dtype) for c, p in zip(cdef, PLANES)]
    return dict(name=name, pic=pic, w=w, h=h, bd=bd, unit_size=[int(v) for v in par[3:6]], frame_type=[int(v) for v in par[6:9]],
                win=[int(v) for v in par[9:12]], dblk=dblk, cdef=cdef, src=src, out=out, units=g[name + "_units"].view(UNIT_DTYPE).reshape(-1),
                offsets=[int(v) for v in g[name + "_offsets"]], cands=g[name + "_cands"].view(CAND_DTYPE).reshape(-1), sse=g[name + "_sse"],
                stats_m=g[name + "_M"], stats_h=g[name + "_H"], ws_mode=int(g[name + "_ws_mode"]), ws_final=g[name + "_ws_final"], ws_sse=g[name + "_ws_sse"],
                ws_n=g[name + "_ws_n"], ws_trials=g[name + "_ws_trials"], ws_trial_sse=g[name + "_ws_trial_sse"],
                results=g[name + "_results"].view(RESULT_DTYPE).reshape(-1), fin_types=g[name + "_fin_types"],
                fin_units=g[name + "_fin_units"].view(UNIT_DTYPE).reshape(len(g[name + "_fin_types"]), -1), finishes=g["finishes"])


def search_of(c, unit_index):
    """the reference's search_wiener_seg of a unit of the picture's block -> (final taps [6], sse, trials [n, 6], their sse [n])"""
    a = int(c["ws_n"][:unit_index].sum())
    n = int(c["ws_n"][unit_index])
    return c["ws_final"][unit_index], int(c["ws_sse"][unit_index]), c["ws_trials"][a:a + n], c["ws_trial_sse"][a:a + n]


def unpack_stats(c, unit_index):
    """the fixture keeps M and the upper triangle of H per unit, one after another: -> (win, M [win2], H [win2, win2]) of a unit of the
    picture's block"""
    plane = max(p for p in range(3) if c["offsets"][p] <= unit_index)
    pos_m = pos_h = 0
    for u in range(unit_index):
        pl = max(p for p in range(3) if c["offsets"][p] <= u)
        w2 = c["win"][pl] ** 2
        pos_m += w2
        pos_h += w2 * (w2 + 1) // 2
    w2 = c["win"][plane] ** 2
    M = c["stats_m"][pos_m:pos_m + w2]
    H = np.zeros((w2, w2), np.int64)
    H[np.triu_indices(w2)] = c["stats_h"][pos_h:pos_h + w2 * (w2 + 1) // 2]
    H = H + np.triu(H, 1).T
    return c["win"][plane], M, H


# ---- the plain model -----------------------------------------------------------------------------------------------------------
def plane_grid(w, h, unit_size, plane):
    """-> pw, ph, ss, us, nh, nv"""
    ss = int(plane > 0)
    pw, ph, us = w >> ss, h >> ss, unit_size[plane]
    return pw, ph, ss, us, max((pw + us // 2) // us, 1), max((ph + us // 2) // us, 1)


def unit_limits(w, h, unit_size, plane, index):
    pw, ph, ss, us, nh, nv = plane_grid(w, h, unit_size, plane)
    i, j, off = index // nh, index % nh, 8 >> ss
    return (j * us, pw if j == nh - 1 else (j + 1) * us, 0 if i == 0 else i * us - off, ph if i == nv - 1 else (i + 1) * us - off)


def stripes(ph, ss):
    sh, off = 64 >> ss, 8 >> ss
    return [(max(0, s * sh - off), min(ph, (s + 1) * sh - off)) for s in range((ph + off + sh - 1) // sh)]


def halo_source(r, y0, y1, ph):
    """row r of the stripe [y0, y1) -> (row to read, from the deblocked picture?)"""
    if r < y0:
        return (0, False) if y0 == 0 else (max(r, y0 - 2), True)
    if r >= y1:
        return (ph - 1, False) if y1 == ph else (min(r, y1 + 1), True)
    return r, False


def stripe_rows(cdef, dblk, y0, y1):
    """the stripe with its halo of three rows and columns -> int64 [(y1 - y0 + 6), pw + 6]"""
    ph, pw = cdef.shape
    cols = np.clip(np.arange(-3, pw + 3), 0, pw - 1)
    rows = []
    for r in range(y0 - 3, y1 + 3):
        row, from_dblk = halo_source(r, y0, y1, ph)
        rows.append((dblk if from_dblk else cdef)[row][cols])
    return np.array(rows, np.int64)


def taps7(t):
    t = [int(v) for v in t]
    return np.array(t + [-2 * sum(t)] + t[::-1], np.int64)


def wiener(ext, vf, hf, bd):
    """ext: [(rows + 6), cols + 6] -> [rows, cols]"""
    rows, cols = ext.shape[0] - 6, ext.shape[1] - 6
    h7, v7 = taps7(hf), taps7(vf)
    s = sum(h7[k] * ext[:, k:k + cols] for k in range(7)) + (ext[:, 3:3 + cols] << 7) + (1 << (bd + 6))
    tmp = np.clip((s + 4) >> 3, 0, (1 << (bd + 5)) - 1)
    s = sum(v7[k] * tmp[k:k + rows] for k in range(7)) + (tmp[3:3 + rows] << 7) - (1 << (bd + 10))
    return np.clip((s + 1024) >> 11, 0, (1 << bd) - 1)


def _rpot(v, n):
    return (v + ((1 << n) >> 1)) >> n


def _sgr_ab(ext, r, s, bd):
    """A, B at rows -1 .. rows, columns -1 .. cols -> [(rows + 2), cols + 2]"""
    rows, cols = ext.shape[0] - 6, ext.shape[1] - 6
    n = (2 * r + 1) ** 2
    box = lambda a: sum(a[2 + dy:2 + dy + rows + 2, 2 + dx:2 + dx + cols + 2] for dy in range(-r, r + 1) for dx in range(-r, r + 1))
    bsum, asum = box(ext), box(ext * ext)
    a, b = _rpot(asum, 2 * (bd - 8)), _rpot(bsum, bd - 8)
    p = np.where(a * n < b * b, 0, a * n - b * b) & 0xFFFFFFFF
    z = _rpot((p * s) & 0xFFFFFFFF, 20)
    A = X_BY_XPLUS1[np.minimum(z, 255)]
    B = _rpot(((256 - A) * bsum * (164 if r == 2 else 455)) & 0xFFFFFFFF, 12)
    return A, B


def sgr(ext, ep, xqd, bd):
    rows, cols = ext.shape[0] - 6, ext.shape[1] - 6
    px = ext[3:3 + rows, 3:3 + cols]
    u = px << 4
    v = u << 7
    r0, r1 = SGR_R[ep]
    if r0 == 0:
        xq = (0, 128 - int(xqd[1]))
    elif r1 == 0:
        xq = (int(xqd[0]), 0)
    else:
        xq = (int(xqd[0]), 128 - int(xqd[0]) - int(xqd[1]))
    sl = lambda a, dy, dx: a[1 + dy:1 + dy + rows, 1 + dx:1 + dx + cols]
    if r0 > 0:
        A, B = _sgr_ab(ext, r0, SGR_S[ep][0], bd)
        even = lambda a: (sl(a, -1, 0) + sl(a, 1, 0)) * 6 + (sl(a, -1, -1) + sl(a, -1, 1) + sl(a, 1, -1) + sl(a, 1, 1)) * 5
        odd = lambda a: sl(a, 0, 0) * 6 + (sl(a, 0, -1) + sl(a, 0, 1)) * 5
        f_even, f_odd = (even(A) * px + even(B) + 256) >> 9, (odd(A) * px + odd(B) + 128) >> 8
        flt0 = np.where((np.arange(rows) & 1)[:, None] == 0, f_even, f_odd)
        v = v + xq[0] * (flt0 - u)
    if r1 > 0:
        A, B = _sgr_ab(ext, r1, SGR_S[ep][1], bd)
        full = lambda a: (sl(a, 0, 0) + sl(a, 0, -1) + sl(a, 0, 1) + sl(a, -1, 0) + sl(a, 1, 0)) * 4 + (sl(a, -1, -1) + sl(a, -1, 1) + sl(a, 1, -1) + sl(a, 1, 1)) * 3
        flt1 = (full(A) * px + full(B) + 256) >> 9
        v = v + xq[1] * (flt1 - u)
    w16 = ((v + 1024) >> 11).astype(np.int16).astype(np.int64)
    return np.clip(w16, 0, (1 << bd) - 1)


def filter_unit(cdef, dblk, limits, rec, ss, bd):
    """the restored samples of one unit -> int64 [v_end - v_start, h_end - h_start]"""
    hs, he, vs, ve = limits
    ph = cdef.shape[0]
    out = cdef[vs:ve, hs:he].astype(np.int64)
    if int(rec["type"]) == 0:
        return out
    for y0, y1 in stripes(ph, ss):
        a, b = max(y0, vs), min(y1, ve)
        if a >= b:
            continue
        ext = stripe_rows(cdef, dblk, a, b)[:, hs:he + 6]
        out[a - vs:b - vs] = wiener(ext, rec["vfilter"], rec["hfilter"], bd) if int(rec["type"]) == 1 else sgr(ext, int(rec["ep"]), rec["xqd"], bd)
    return out


def allowed(rec_type, frame_type):
    return rec_type if frame_type == 3 or frame_type == rec_type else 0


def model_apply(c):
    out = []
    for plane in range(3):
        pw, ph, ss, us, nh, nv = plane_grid(c["w"], c["h"], c["unit_size"], plane)
        res = c["cdef"][plane].copy()
        for k in range(nh * nv if c["frame_type"][plane] else 0):
            rec = c["units"][c["offsets"][plane] + k].copy()
            rec["type"] = allowed(int(rec["type"]), c["frame_type"][plane])
            hs, he, vs, ve = lim = unit_limits(c["w"], c["h"], c["unit_size"], plane, k)
            res[vs:ve, hs:he] = filter_unit(c["cdef"][plane], c["dblk"][plane], lim, rec, ss, c["bd"])
        out.append(res)
    return out


def model_try(c, cand):
    plane = int(cand["plane"])
    hs, he, vs, ve = lim = unit_limits(c["w"], c["h"], c["unit_size"], plane, int(cand["unit"]))
    f = filter_unit(c["cdef"][plane], c["dblk"][plane], lim, cand["u"], int(plane > 0), c["bd"])
    return int(((f - c["src"][plane][vs:ve, hs:he].astype(np.int64)) ** 2).sum())


def model_stats(c, plane, index, win):
    hs, he, vs, ve = unit_limits(c["w"], c["h"], c["unit_size"], plane, index)
    cdef, src = c["cdef"][plane].astype(np.int64), c["src"][plane].astype(np.int64)
    ph, pw = cdef.shape
    avg = int(cdef[vs:ve, hs:he].sum()) // ((ve - vs) * (he - hs))
    half = win // 2
    ys, xs = np.arange(vs, ve), np.arange(hs, he)
    Y = np.stack([(cdef[np.clip(ys + l, 0, ph - 1)][:, np.clip(xs + k, 0, pw - 1)] - avg).reshape(-1)
                  for k in range(-half, half + 1) for l in range(-half, half + 1)])
    X = (src[vs:ve, hs:he] - avg).reshape(-1)
    M, H = Y @ X, Y @ Y.T
    if c["bd"] == 10:
        trunc = lambda a: np.sign(a) * (np.abs(a) // 4)
        M, H = trunc(M), trunc(H)
    return M, H

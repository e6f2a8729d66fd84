"""Shared by tests/golden/make_golden_dlf.py, tests/test_dlf_cpu.py and tests/test_gpu_dlf.py: the deblocking fixture
(tests/golden/dlf.npz), the harness library round the reference's deblocking filter (oracle/_ref/libsvtref_dlf.so, None when it is
not built) and a plain model of set_lpf_parameters' edge decision that the generator uses to count what the cases cover."""
import ctypes
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = os.path.join(ROOT, "tests", "golden", "dlf.npz")
REF_DLF = os.path.join(ROOT, "oracle", "_ref", "libsvtref_dlf.so")

TX_W = (4, 8, 16, 32, 64, 4, 8, 8, 16, 16, 32, 32, 64, 4, 16, 8, 32, 16, 64)
TX_H = (4, 8, 16, 32, 64, 8, 4, 16, 8, 32, 16, 64, 32, 16, 4, 32, 8, 64, 16)
BS_W = (4, 4, 8, 8, 8, 16, 16, 16, 32, 32, 32, 64, 64, 64, 128, 128, 4, 16, 8, 32, 16, 64)
BS_H = (4, 8, 4, 8, 16, 8, 16, 32, 16, 32, 64, 32, 64, 128, 64, 128, 16, 4, 32, 8, 64, 16)
MODE_LF = (0,) * 13 + (1, 1, 0, 1) + (1, 1, 1, 1, 1, 1, 0, 1)
NO_SRC = 0xFFFFFFFF
PLANES = ("y", "cb", "cr")
# params row of a case
P_W, P_H, P_BD, P_L0, P_L1, P_LU, P_LV, P_SHARP, P_DELTA, P_RD, P_MD = 0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 17


def tx_of(w, h):
    return [i for i in range(19) if TX_W[i] == w and TX_H[i] == h][0]


class RefParams(ctypes.Structure):
    """ref_dlf_params of tests/c/ref_dlf.c"""
    _fields_ = [("width", ctypes.c_int32), ("height", ctypes.c_int32), ("bit_depth", ctypes.c_int32), ("filter_level", ctypes.c_int32 * 2),
                ("filter_level_u", ctypes.c_int32), ("filter_level_v", ctypes.c_int32), ("sharpness_level", ctypes.c_int32),
                ("mode_ref_delta_enabled", ctypes.c_int32), ("ref_deltas", ctypes.c_int8 * 8), ("mode_deltas", ctypes.c_int8 * 2),
                ("pad", ctypes.c_int8 * 2), ("loop_filter_mode", ctypes.c_int32), ("tx_mode_only_4x4", ctypes.c_int32),
                ("is_key_frame", ctypes.c_int32), ("base_qindex", ctypes.c_int32)]


def ref_params(row, **kw):
    p = RefParams()
    p.width, p.height, p.bit_depth = int(row[P_W]), int(row[P_H]), int(row[P_BD])
    p.filter_level[0], p.filter_level[1], p.filter_level_u, p.filter_level_v = (int(v) for v in row[P_L0:P_L0 + 4])
    p.sharpness_level, p.mode_ref_delta_enabled = int(row[P_SHARP]), int(row[P_DELTA])
    for i in range(8):
        p.ref_deltas[i] = int(row[P_RD + i])
    for i in range(2):
        p.mode_deltas[i] = int(row[P_MD + i])
    for k, v in kw.items():
        setattr(p, k, v)
    return p


_lib = []


def ref_dlf():
    """the harness library, or None when it is not built"""
    if not _lib:
        L = None
        if os.path.exists(REF_DLF):
            L = ctypes.CDLL(REF_DLF)
            for f in (L.ref_dlf_frame, L.ref_dlf_table, L.ref_dlf_pick, L.ref_dlf_filter):
                f.restype = ctypes.c_int
            vp, ci = ctypes.c_void_p, ctypes.c_int
            L.ref_dlf_frame.argtypes = [vp, vp, ci, vp, ci, vp, ci, vp, ci, ci, ci]
            L.ref_dlf_table.argtypes = [vp] + [vp, ci] * 6 + [vp, ci, vp]
            L.ref_dlf_pick.argtypes = [vp, ci] + [vp, ci] * 6 + [vp, ci, vp, vp]
            L.ref_dlf_filter.argtypes = [ci, ci, ci, ci, vp, ci, ci, ci, ci]
        _lib.append(L)
    return _lib[0]


def _p(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def ref_frame(row, planes, mi, plane_start=0, plane_end=3, **kw):
    """av1_loop_filter_frame on copies of the planes -> the filtered planes"""
    L = ref_dlf()
    out = [np.ascontiguousarray(p).copy() for p in planes]
    mi = np.ascontiguousarray(mi)
    p = ref_params(row, **kw)
    assert L.ref_dlf_frame(ctypes.addressof(p), _p(out[0]), out[0].shape[1], _p(out[1]), out[1].shape[1], _p(out[2]), out[2].shape[1], _p(mi),
                           mi.shape[1], plane_start, plane_end) == 0
    return out


def ref_table(row, planes, src, mi):
    L = ref_dlf()
    planes = [np.ascontiguousarray(p) for p in planes]
    src = [np.ascontiguousarray(p) for p in src]
    mi = np.ascontiguousarray(mi)
    sse = np.zeros((3, 64), np.uint64)
    p = ref_params(row)
    args = []
    for a in planes + src:
        args += [_p(a), a.shape[1]]
    assert L.ref_dlf_table(ctypes.addressof(p), *args, _p(mi), mi.shape[1], _p(sse)) == 0
    return sse


def ref_pick(row, method, planes, src, mi, **kw):
    """av1_pick_filter_level whole -> (levels[4], sharpness)"""
    L = ref_dlf()
    p = ref_params(row, **kw)
    levels = np.zeros(4, np.int32)
    sharp = np.zeros(1, np.int32)
    if planes is None:
        args = [None, 0] * 6 + [None, 0]
    else:
        planes = [np.ascontiguousarray(a) for a in planes]
        src = [np.ascontiguousarray(a) for a in src]
        mi = np.ascontiguousarray(mi)
        args = []
        for a in planes + src:
            args += [_p(a), a.shape[1]]
        args += [_p(mi), mi.shape[1]]
    assert L.ref_dlf_pick(ctypes.addressof(p), method, *args, _p(levels), _p(sharp)) == 0
    return levels, int(sharp[0])


# ---- the fixture ---------------------------------------------------------------------------------------------------------------
_fix = []


def fixture():
    if not _fix:
        _fix.append(np.load(FIXTURE))
    return _fix[0]


def case_names():
    return [str(s) for s in fixture()["cases"]]


def case(name):
    """-> dict: row (params), pic (name), rec / src / out (three planes each), mi [h / 4][w / 4][4], sse [3][64]"""
    g = fixture()
    pic = str(g[name + "_pic"])
    rec = [g[f"{pic}_rec_{p}"] for p in PLANES]
    out = [(r.astype(np.int32) + g[f"{name}_diff_{p}"]).astype(r.dtype) for r, p in zip(rec, PLANES)]
    src = [(r.astype(np.int32) + g[f"{pic}_dsrc_{p}"]).astype(r.dtype) for r, p in zip(rec, PLANES)]
    return dict(name=name, row=g[name + "_params"], pic=pic, rec=rec, src=src, out=out, mi=g[pic + "_mi"], sse=g[name + "_sse"],
                final=g[pic + "_final"], final_count=g[pic + "_final_count"], info=g[pic + "_info"])


# ---- a plain model of the edge decision (set_lpf_parameters), for counting what a grid covers ------------------------------------
def unit_level(row, plane, dirn, ref, mode):
    base = int(row[(P_L0 + dirn) if plane == 0 else (P_LU + plane - 1)])
    if not row[P_DELTA]:
        return base
    scale = 1 << (base >> 5)
    mlf = MODE_LF[mode] if mode < 25 else 0
    v = base + int(row[P_RD + ref]) * scale + (int(row[P_MD + mlf]) * scale if ref > 0 else 0)
    return min(max(v, 0), 63)


def edge_units(row, mi, plane, dirn):
    """-> list of (x, y, length, level) of the edge units av1_loop_filter_frame filters in `plane`, direction `dirn`"""
    w, h = int(row[P_W]), int(row[P_H])
    l0, l1, lu, lv = (int(v) for v in row[P_L0:P_L0 + 4])
    if not (l0 or l1) or (plane == 1 and not lu) or (plane == 2 and not lv):
        return []
    ss = 1 if plane else 0
    pw, ph = w >> ss, h >> ss

    def side(m, d):
        if plane == 0:
            return (TX_W if d == 0 else TX_H)[m[1]]
        s = (BS_W if d == 0 else BS_H)[m[0]]
        return min(max(s // 2, 4), 32)

    out = []
    for y in range(0, ph, 4):
        for x in range(0, pw, 4):
            coord = x if dirn == 0 else y
            if coord == 0:
                continue
            mr, mc = ss | ((y << ss) >> 2), ss | ((x << ss) >> 2)
            cur = mi[mr, mc]
            prv = mi[mr, mc - (1 << ss)] if dirn == 0 else mi[mr - (1 << ss), mc]
            ts = side(cur, dirn)
            if coord & (ts - 1):
                continue
            cref, pref = int(cur[2]) & 7, int(prv[2]) & 7
            cl, pl = unit_level(row, plane, dirn, cref, int(cur[3])), unit_level(row, plane, dirn, pref, int(prv[3]))
            cskip, pskip = (cur[2] >> 7) and cref > 0, (prv[2] >> 7) and pref > 0
            pu = (BS_W if dirn == 0 else BS_H)[cur[0]]
            pu = pu if plane == 0 else max(pu // 2, 4)
            if not (cl or pl) or (pskip and cskip and (coord & (pu - 1))):
                continue
            m = min(ts, side(prv, dirn))
            length = 4 if m <= 4 else (6 if plane else (8 if m == 8 else 14))
            out.append((x, y, length, cl if cl else pl))
    return out

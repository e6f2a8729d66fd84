"""The self-guided parameter search of loop restoration: what the fixture generator (tests/golden/make_golden_lr_sgr.py) and the tests
share - the harness library's bindings (tests/c/ref_lr_sgr.c), the fixture's cases, and a plain numpy model of what the search
computes per (unit, ep), written from the rules in include/svt_hip_dsp.h on lr_cases' self-guided arithmetic: the two filter passes over
the CDEF picture alone (no stripe rows, no projection), f1 / f2, the five sums and the projection error.  That the model equals the
reference is what tests/test_lr_sgr_cpu.py checks; the kernels are then compared with the model and the fixture."""
import ctypes
import os

import numpy as np

import lr_cases as lc

ROOT = lc.ROOT
FIXTURE = os.path.join(ROOT, "tests", "golden", "lr_sgr.npz")
REF_LR_SGR = os.path.join(ROOT, "oracle", "_ref", "libsvtref_lr_sgr.so")
WALK_DTYPE = np.dtype([("err", "<i8"), ("xqd", "<i2", 2), ("start", "<i2", 2), ("evals", "<i4"), ("pad", "<i4")])                          # svt_hip_lr_sgr_walk
BEST_DTYPE = np.dtype([("sse", "<i8"), ("proj_err", "<i8"), ("ep", "<i4"), ("xqd", "<i2", 2)])        # svt_hip_lr_sgr_best
XQD_MIN, XQD_MAX = lc.XQD_MIN, lc.XQD_MAX
MAX_EVALS = 137

_lib = []


def ref_lr_sgr():
    """the harness library, or None when it is not built"""
    if not _lib:
        L = None
        if os.path.exists(REF_LR_SGR):
            L = ctypes.CDLL(REF_LR_SGR)
            vp, ci = ctypes.c_void_p, ctypes.c_int
            L.ref_lr_new.restype = vp
            L.ref_lr_new.argtypes = [ci, ci, ci, vp, vp, vp, vp]
            L.ref_lr_free.argtypes = [vp]
            L.ref_lr_free.restype = None
            L.ref_lr_grid.argtypes = [vp, ci, vp]
            L.ref_lr_limits.argtypes = [vp, ci, ci, vp]
            L.ref_lr_try.argtypes = [vp, ci, ci, ci, vp]
            L.ref_lr_try.restype = ctypes.c_int64
            L.ref_lr_finish.argtypes = [vp, ci, vp, vp, vp, vp]
            L.ref_lr_sgr_search.argtypes = [vp, ci, ci, ci, vp, ci, vp, vp]
            L.ref_lr_sgr_search.restype = ctypes.c_int64
            L.ref_lr_sgr_ep.argtypes = [vp, ci, ci, ci, ci, vp, vp, vp, ci, vp, vp]
            L.ref_lr_sgr_ep_seen.argtypes = [vp, vp, ci, vp]
        _lib.append(L)
    return _lib[0]


class RefPicture(lc.RefPicture):
    """lr_cases.RefPicture inside the search's harness library"""

    def __init__(self, w, h, bd, unit_size, dblk, cdef, src):
        self.L = ref_lr_sgr()
        self.w, self.h, self.bd, self.unit_size = w, h, bd, list(unit_size)
        self.keep = [[np.ascontiguousarray(p) for p in planes] for planes in (dblk, cdef, src)]
        us = (ctypes.c_int32 * 3)(*unit_size)
        self.ctx = self.L.ref_lr_new(w, h, bd, us, *[lc._ptrs(k) for k in self.keep])
        assert self.ctx

    def sgr_search(self, plane, unit, ref_ep, sg_filter_mode, ep_cnt, flavour=0):
        """search_sgrproj_seg for one unit -> (ep, [xqd0, xqd1], sse); ep_cnt (int32 [16]) is incremented as cm->sg_frame_ep_cnt is"""
        out, ref = np.zeros(3, np.int32), np.array(ref_ep, np.int8)
        sse = self.L.ref_lr_sgr_search(self.ctx, flavour, plane, unit, ref.ctypes.data, sg_filter_mode, out.ctypes.data, ep_cnt.ctypes.data)
        assert sse >= 0
        return int(out[0]), [int(out[1]), int(out[2])], int(sse)

    def sgr_ep(self, plane, unit, ep, flavour=0, planes=False):
        """one (unit, ep) of the search's loop -> dict: exq, start, final (pairs), err, trials (int64 [n, 3]: xq0, xq1, error) and, on
        request, flt0 / flt1 (int32, unit-shaped; None for a radius of 0)"""
        hs, he, vs, ve = lc.unit_limits(self.w, self.h, self.unit_size, plane, unit)
        out, err, trials = np.zeros(6, np.int32), np.zeros(1, np.int64), np.zeros((512, 3), np.int64)
        f0 = np.zeros((ve - vs, he - hs), np.int32) if planes else None
        f1 = np.zeros((ve - vs, he - hs), np.int32) if planes else None
        n = self.L.ref_lr_sgr_ep(self.ctx, flavour, plane, unit, ep, out.ctypes.data, err.ctypes.data, trials.ctypes.data, len(trials),
                                 f0.ctypes.data if planes else None, f1.ctypes.data if planes else None)
        assert n > 0
        r0, r1 = lc.SGR_R[ep]
        return dict(exq=out[:2].tolist(), start=out[2:4].tolist(), final=out[4:].tolist(), err=int(err[0]), trials=trials[:n].copy(),
                    flt0=f0 if r0 else None, flt1=f1 if r1 else None)

    def ep_seen(self, ref_ep, sg_filter_mode):
        """the range of ep the reference's search filters under these settings -> (lo, hi) or (-1, -1) for an empty one"""
        out, ref = np.zeros(2, np.int32), np.array(ref_ep, np.int8)
        n = self.L.ref_lr_sgr_ep_seen(self.ctx, ref.ctypes.data, sg_filter_mode, out.ctypes.data)
        assert n >= 0 and (n == 0 or n == out[1] - out[0]), (n, out)
        return int(out[0]), int(out[1])


# ---- the fixture ---------------------------------------------------------------------------------------------------------------
_fix = []


def fixture():
    if not _fix:
        _fix.append(np.load(FIXTURE))
    return _fix[0]


def case_names():
    return [str(s) for s in fixture()["cases"]]


def picture(pic):
    """a picture of this fixture, else of lr.npz"""
    g = fixture()
    return lc.picture(g if f"{pic}_dblk_y" in g.files else lc.fixture(), pic)


_cases = {}


def case(name):
    """-> dict: w, h, bd, unit_size, dblk / cdef / src, offsets, and per (unit of the picture's block, ep): exq, start, final [U, 16, 2],
    err [U, 16], ntrials [U, 16], trials (xq int16 [sum, 2], err int64 [sum]); search [ranges, U, 4] = ep, xqd0, xqd1, sse; cnt [ranges, 16]"""
    if name not in _cases:
        g = fixture()
        par = g[name + "_params"]
        w, h, bd = (int(v) for v in par[:3])
        us = [int(v) for v in par[3:6]]
        dblk, cdef, src = picture(str(g[name + "_pic"]))
        offsets = [0]
        for plane in range(3):
            _, _, _, _, nh, nv = lc.plane_grid(w, h, us, plane)
            offsets.append(offsets[-1] + nh * nv)
        c = dict(name=name, w=w, h=h, bd=bd, unit_size=us, dblk=dblk, cdef=cdef, src=src, offsets=offsets)
        for k in ("exq", "start", "final", "err", "ntrials", "trial_xq", "trial_err", "search", "cnt"):
            c[k] = g[f"{name}_{k}"]
        c["trial_at"] = np.concatenate([[0], np.cumsum(c["ntrials"].reshape(-1))])
        if name + "_results" in g.files:
            c["results"] = g[name + "_results"].view(lc.RESULT_DTYPE).reshape(-1)
            c["fin_types"] = g[name + "_fin_types"]
            c["fin_units"] = g[name + "_fin_units"].view(lc.UNIT_DTYPE).reshape(len(c["fin_types"]), -1)
            c["wiener_win"] = [int(v) for v in g[name + "_wiener_win"]]
        _cases[name] = c
    return _cases[name]


def units_of(c):
    """(plane, unit of the plane, index inside the picture's block) of every unit"""
    return [(p, k, c["offsets"][p] + k) for p in range(3) for k in range(c["offsets"][p + 1] - c["offsets"][p])]


def trials_of(c, u, ep):
    a, b = c["trial_at"][u * 16 + ep], c["trial_at"][u * 16 + ep + 1]
    return c["trial_xq"][a:b].astype(np.int64), c["trial_err"][a:b]


def ranges():
    """the fixture's search settings: rows of (sg_ref_frame_ep[0], [1], sg_filter_mode, ep_lo, ep_hi)"""
    return fixture()["ranges"].tolist()


# ---- the plain model -----------------------------------------------------------------------------------------------------------
def unit_ext(plane_samples, limits):
    """the unit with its halo of three rows and columns, every row and column clamped to the plane (the CDEF picture extended by 3)"""
    hs, he, vs, ve = limits
    ph, pw = plane_samples.shape
    rows, cols = np.clip(np.arange(vs - 3, ve + 3), 0, ph - 1), np.clip(np.arange(hs - 3, he + 3), 0, pw - 1)
    return plane_samples[rows][:, cols].astype(np.int64)


def flt_planes(ext, ep, bd):
    """-> (flt0, flt1) int64 unit-shaped, None for a radius of 0.  The fast pass's row parity counts from the unit's first row, which is
    even in the plane as stripe and processing-unit starts are."""
    rows, cols = ext.shape[0] - 6, ext.shape[1] - 6
    px = ext[3:3 + rows, 3:3 + cols]
    r0, r1 = lc.SGR_R[ep]
    sl = lambda a, dy, dx: a[1 + dy:1 + dy + rows, 1 + dx:1 + dx + cols]
    flt0 = flt1 = None
    if r0 > 0:
        A, B = lc._sgr_ab(ext, r0, lc.SGR_S[ep][0], bd)
        even = lambda a: (sl(a, -1, 0) + sl(a, 1, 0)) * 6 + (sl(a, -1, -1) + sl(a, -1, 1) + sl(a, 1, -1) + sl(a, 1, 1)) * 5
        odd = lambda a: sl(a, 0, 0) * 6 + (sl(a, 0, -1) + sl(a, 0, 1)) * 5
        flt0 = np.where((np.arange(rows) & 1)[:, None] == 0, (even(A) * px + even(B) + 256) >> 9, (odd(A) * px + odd(B) + 128) >> 8)
    if r1 > 0:
        A, B = lc._sgr_ab(ext, r1, lc.SGR_S[ep][1], bd)
        full = lambda a: (sl(a, 0, 0) + sl(a, 0, -1) + sl(a, 0, 1) + sl(a, -1, 0) + sl(a, 1, 0)) * 4 + (sl(a, -1, -1) + sl(a, -1, 1) + sl(a, 1, -1) + sl(a, 1, 1)) * 3
        flt1 = (full(A) * px + full(B) + 256) >> 9
    return flt0, flt1


_model = {}


def model(c, plane, unit, ep):
    """-> (f1, f2, sd) int64, flat over the unit row-major: f = flt - (dat << 4), 0 for a radius of 0; sd = src - dat"""
    key = (c["name"], plane, unit, ep)
    if key not in _model:
        lim = hs, he, vs, ve = lc.unit_limits(c["w"], c["h"], c["unit_size"], plane, unit)
        ext = unit_ext(c["cdef"][plane], lim)
        dat = ext[3:-3, 3:-3]
        flt0, flt1 = flt_planes(ext, ep, c["bd"])
        zero = np.zeros_like(dat)
        f1 = zero if flt0 is None else flt0 - (dat << 4)
        f2 = zero if flt1 is None else flt1 - (dat << 4)
        sd = c["src"][plane][vs:ve, hs:he].astype(np.int64) - dat
        _model[key] = (f1.reshape(-1), f2.reshape(-1), sd.reshape(-1))
    return _model[key]


def sums(f1, f2, sd):
    """H00, H11, H01, C0, C1 with s = sd << 4"""
    s = sd * 16
    return np.array([(f1 * f1).sum(), (f2 * f2).sum(), (f1 * f2).sum(), (f1 * s).sum(), (f2 * s).sum()], np.int64)


def proj_error(f1, f2, sd, xq):
    e = ((int(xq[0]) * f1 + int(xq[1]) * f2 + 1024) >> 11) - sd
    return int((e * e).sum())


def decode_xq(xqd, ep):
    r0, r1 = lc.SGR_R[ep]
    if r0 == 0:
        return [0, 128 - int(xqd[1])]
    if r1 == 0:
        return [int(xqd[0]), 0]
    return [int(xqd[0]), 128 - int(xqd[0]) - int(xqd[1])]


def replay_walk(ep, start, trial_xq, trial_err):
    """The walk as include/svt_hip_dsp.h states it, every evaluation's error taken from a record of the reference's evaluations; asserts
    that each evaluation it asks for is the recorded one.  -> (final xqd, its error, events: ties accepted, runs of two successive moves
    at step 2, moves a range limit stopped, `if (skip) break;` taken with xqd[1] still to come)"""
    ev = dict(ties=0, twice=0, limit=0, skip=0)
    xqd, pos = [int(v) for v in start], [0]

    def evaluate():
        assert pos[0] < len(trial_err) and [int(v) for v in trial_xq[pos[0]]] == decode_xq(xqd, ep), (ep, xqd, pos[0])
        pos[0] += 1
        return int(trial_err[pos[0] - 1])

    err = evaluate()
    for s in (2, 1):
        for p in (0, 1):
            if lc.SGR_R[ep][p] == 0:
                continue
            skip = False
            for d in (-1, 1):
                if d == 1 and skip:
                    break
                run = 0
                while True:
                    nxt = xqd[p] + d * s
                    if nxt < XQD_MIN[p] or nxt > XQD_MAX[p]:
                        ev["limit"] += 1
                        break
                    keep, xqd[p] = xqd[p], nxt
                    e2 = evaluate()
                    if e2 > err:
                        xqd[p] = keep
                        break
                    ev["ties"] += e2 == err
                    err, run = e2, run + 1
                    skip = skip or d == -1
                    ev["twice"] += run == 2
                    if s != 2:
                        break
            if skip:
                ev["skip"] += p == 0 and lc.SGR_R[ep][1] > 0
                break
    assert pos[0] == len(trial_err), (ep, start, pos[0], len(trial_err))
    return xqd, err, ev

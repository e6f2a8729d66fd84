"""Writes tests/golden/cdef.npz: the CDEF strength search (cdef_seg_search, EbCdefProcess.c:89-258) and the CDEF apply (av1_cdef_frame,
EbCdef.c:471) of small pictures, computed by the REFERENCE's own functions in oracle/_ref/libsvtref.so through ctypes:
cdef_filter_fb, compute_cdef_dist, copy_rect8_8bit_to_16bit_c, and behind the five dispatch globals (NULL after load; pointed at the
_c functions here) cdef_find_dir_c, cdef_filter_block_c, dist_8x8_16bit_c, mse_4x4_16bit_c.

What is this file's own: the loop glue that cdef_seg_search / av1_cdef_frame wrap round those calls (the list of non-skipped 8x8
blocks from the skip map, the CDEF_VERY_LARGE fill and the copy of the tile, the loops over filter blocks, planes and strengths), the
test pictures, and np_filter_block, a numpy restatement of one block's filtering that is used only to ASSERT properties of the fixture
(a clamped sample exists, a corner tap reads CDEF_VERY_LARGE) and is itself checked against the reference's output.

CPU only; run from the repository root after build():  python tests/golden/make_golden_cdef.py
"""
import ctypes
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
OUT = os.path.join(HERE, "cdef.npz")
REF = os.path.join(ROOT, "oracle", "_ref", "libsvtref.so")
sys.path.insert(0, os.path.join(ROOT, "tests"))
import svtlibs      # noqa: E402

BSTRIDE, VBORDER, HBORDER = 144, 3, 8              # CDEF_BSTRIDE (MAX_SB_SIZE_LOG2 7), CDEF_VBORDER, CDEF_HBORDER
INBUF = BSTRIDE * (128 + 2 * VBORDER)              # CDEF_INBUF_SIZE
IN0 = VBORDER * BSTRIDE + HBORDER
LARGE = 30000                                      # CDEF_VERY_LARGE
BLOCK_4X4, BLOCK_8X8 = 0, 3
DIRS = [((-1, 1), (-2, 2)), ((0, 1), (-1, 2)), ((0, 1), (0, 2)), ((0, 1), (1, 2)), ((1, 1), (2, 2)), ((1, 0), (2, 1)), ((1, 0), (2, 0)),
        ((1, 0), (2, -1))]                         # cdef_directions as (dy, dx)

# (name, bit depth, width, height, base_qindex, skip map, content)
CASES = [("a", 8, 128, 128, 20, "none", "smooth"), ("b", 8, 200, 136, 100, "random", "edges"), ("c", 8, 200, 136, 100, "block", "noise"),
         ("d", 8, 128, 64, 230, "all", "mixed"), ("e", 10, 200, 136, 130, "random", "edges"), ("f", 10, 128, 128, 90, "none", "noise"),
         ("g", 10, 200, 136, 250, "block", "mixed"), ("h", 8, 64, 64, 40, "random", "mixed")]


def ptr(a):
    return a.ctypes.data_as(ctypes.c_void_p)


_lib = None
SLOTS = {s: s + "_c" for s in ("cdef_find_dir", "cdef_filter_block", "copy_rect8_8bit_to_16bit", "dist_8x8_16bit", "mse_4x4_16bit")}


def ref_lib():
    """libsvtref.so with the five CDEF dispatch globals pointed at the reference's C functions; None when it is not built.  The
    slots are pointed on every call (svtlibs.ref_with_slots: whatever refilled them since the last call does not matter)"""
    global _lib
    first = _lib is None
    _lib = svtlibs.ref_with_slots(SLOTS, _lib)
    if first and _lib is not None:
        _lib.compute_cdef_dist.restype = ctypes.c_uint64
        _lib.dist_8x8_16bit_c.restype = ctypes.c_uint64
        _lib.cdef_find_dir_c.restype = ctypes.c_int32
    return _lib


def smooth_picture(rng, h, w, grain=6):
    a = rng.integers(0, 256, (h // 4 + 3, w // 4 + 3)).astype(np.float64)
    a = np.kron(a, np.ones((4, 4)))
    k = np.ones(5) / 5
    a = np.apply_along_axis(lambda r: np.convolve(r, k, "same"), 1, a)
    a = np.apply_along_axis(lambda r: np.convolve(r, k, "same"), 0, a)
    return (a[:h, :w] + rng.integers(-grain, grain + 1, (h, w))).clip(0, 255).astype(np.int64)


def edge_picture(rng, h, w):
    """hard edges at several angles: 16x16 cells, each split by a line through its centre"""
    yy, xx = np.mgrid[0:h, 0:w]
    cell = (yy // 16) * ((w + 15) // 16) + xx // 16
    ang = (cell % 8) * (np.pi / 8) + np.pi / 16 * ((cell // 8) % 2)
    side = np.cos(ang) * ((xx % 16) - 7.5) + np.sin(ang) * ((yy % 16) - 7.5) > 0
    lo, hi = rng.integers(10, 90, cell.max() + 1), rng.integers(150, 250, cell.max() + 1)
    return np.where(side, hi[cell], lo[cell]).astype(np.int64)


def make_plane(rng, kind, h, w):
    """-> (source, reconstruction) of one plane at 8-bit scale; the reconstruction is the source with coding noise, exactly flat where the
    content is flat"""
    if kind == "smooth":
        s = smooth_picture(rng, h, w)
    elif kind == "edges":
        s = edge_picture(rng, h, w)
    elif kind == "noise":
        s = rng.integers(0, 256, (h, w)).astype(np.int64)
    else:                                            # mixed: flat | edges over smooth | full-range noise
        s = smooth_picture(rng, h, w)
        s[: h // 2, : w // 2] = 77
        s[: h // 2, w // 2:] = edge_picture(rng, h // 2, w - w // 2)
        s[h // 2:, w // 2:] = rng.integers(0, 256, (h - h // 2, w - w // 2))
    r = s + rng.integers(-5, 6, (h, w)) + (rng.random((h, w)) < 0.02) * rng.integers(-60, 61, (h, w))     # noise and a few ringing spikes
    if kind == "mixed":
        r[: h // 2, : w // 2] = 77
        # isolated pits of several depths in the flat part (not its first 16 columns, which stay flat): a sample that all its
        # neighbours pull the same way overshoots them and is clamped
        for k, (y, x) in enumerate((y, x) for y in range(3, h // 2 - 3, 5) for x in range(19, w // 2 - 3, 7)):
            r[y, x] = 77 - (2, 3, 5, 8)[k % 4]
    return s.clip(0, 255), r.clip(0, 255)


def make_case(rng, bd, w, h, skipkind, content):
    cs = bd - 8
    dt = np.uint8 if bd == 8 else np.uint16
    src, rec = [], []
    for pli in range(3):
        s, r = make_plane(rng, content, h >> (pli > 0), w >> (pli > 0))
        lsb = (lambda a: rng.integers(0, 1 << cs, a.shape)) if cs else (lambda a: 0)
        src.append(((s << cs) + lsb(s)).astype(dt))
        rec.append(((r << cs) + lsb(r) * (r != 77)).astype(dt))
    h8, w8 = h // 8, w // 8
    skip = np.zeros((h8, w8), np.uint8)
    if skipkind == "random":
        skip[:] = rng.random((h8, w8)) < 0.3
    elif skipkind == "block":
        skip[:] = rng.random((h8, w8)) < 0.1
        skip[0:8, 8:16] = 1                          # filter block (0, 1) skipped whole
    elif skipkind == "all":
        skip[:] = 1
    return src, rec, skip


class CdefList(ctypes.Structure):
    _fields_ = [("by", ctypes.c_uint8), ("bx", ctypes.c_uint8), ("skip", ctypes.c_uint8)]


def build_dlist(skip, fbr, fbc):
    """sb_compute_cdef_list: the non-skipped 8x8 blocks of a filter block in raster order, clipped to the picture"""
    h8, w8 = skip.shape
    blocks = [(by, bx) for by in range(min(8, h8 - 8 * fbr)) for bx in range(min(8, w8 - 8 * fbc)) if not skip[8 * fbr + by, 8 * fbc + bx]]
    dl = (CdefList * 64)()
    for i, (by, bx) in enumerate(blocks):
        dl[i] = CdefList(by, bx, 0)
    return dl, blocks


def fill_inbuf(L, plane, fbr, fbc, l2, skipshape):
    """EbCdefProcess.c:203-216: CDEF_VERY_LARGE everywhere, then the filter block with the rows / columns the picture has round it.
    l2 = log2 of an 8x8 luma block's side in this plane (3 luma, 2 chroma)"""
    h8, w8 = skipshape
    nvfb, nhfb = (h8 + 7) // 8, (w8 + 7) // 8
    nvb, nhb = min(8, h8 - 8 * fbr), min(8, w8 - 8 * fbc)
    inbuf = np.full(INBUF, LARGE, np.uint16)
    yoff, xoff = VBORDER * (fbr != 0), HBORDER * (fbc != 0)
    ysize = (nvb << l2) + VBORDER * (fbr + 1 < nvfb) + yoff
    xsize = (nhb << l2) + HBORDER * (fbc + 1 < nhfb) + xoff
    y0, x0 = ((fbr * 8) << l2) - yoff, ((fbc * 8) << l2) - xoff
    # the reference copies a full 8-column / 3-row border even where the next filter block is narrower (it reads the picture's padding);
    # the filter reads at most 2 samples out, which the picture always has there, so the copy is clipped to the plane
    ysize, xsize = min(ysize, plane.shape[0] - y0), min(xsize, plane.shape[1] - x0)
    dst_off = IN0 - yoff * BSTRIDE - xoff
    if plane.dtype == np.uint8:
        L.copy_rect8_8bit_to_16bit_c(ctypes.c_void_p(inbuf.ctypes.data + 2 * dst_off), BSTRIDE,
                                     ctypes.c_void_p(plane.ctypes.data + y0 * plane.shape[1] + x0), plane.shape[1], ysize, xsize)
    else:
        inbuf.reshape(-1, BSTRIDE)[VBORDER - yoff:VBORDER - yoff + ysize, HBORDER - xoff:HBORDER - xoff + xsize] = plane[y0:y0 + ysize, x0:x0 + xsize]
    return inbuf


def ref_search_fb(L, rec, src16, skip, fbr, fbc, bd, q, gis=range(64)):
    """one filter block of cdef_seg_search -> (mse[2][64], count, dir[8][8], var[8][8], the luma input buffer); None when it is left out.
    src16: the source planes as uint16 (the reference's ref_coeff)"""
    cs = bd - 8
    dl, blocks = build_dlist(skip, fbr, fbc)
    if not blocks:
        return None
    damping = 3 + (q >> 6)
    dirs, var = np.zeros((16, 16), np.int32), np.zeros((16, 16), np.int32)
    dirinit = ctypes.c_int32(0)
    mse = np.zeros((2, 64), np.uint64)
    tmp = np.zeros(128 * 128, np.uint16)
    luma_in = None
    for pli in range(3):
        l2 = 3 - (pli > 0)
        inbuf = fill_inbuf(L, rec[pli], fbr, fbc, l2, skip.shape)
        luma_in = inbuf if pli == 0 else luma_in
        stride = src16[pli].shape[1]
        ref0 = ctypes.c_void_p(src16[pli].ctypes.data + 2 * (((fbr * 8) << l2) * stride + ((fbc * 8) << l2)))
        for gi in gis:
            sec = gi % 4
            L.cdef_filter_fb(None, ptr(tmp), BSTRIDE, ctypes.c_void_p(inbuf.ctypes.data + 2 * IN0), int(pli > 0), int(pli > 0), ptr(dirs),
                             ctypes.byref(dirinit), ptr(var), pli, dl, len(blocks), gi // 4, sec + (sec == 3), damping, damping, cs)
            d = L.compute_cdef_dist(ref0, stride, ptr(tmp), dl, len(blocks), BLOCK_4X4 if pli else BLOCK_8X8, cs, pli)
            mse[min(pli, 1), gi] += np.uint64(d)
    return mse, len(blocks), dirs[:8, :8].copy(), var[:8, :8].copy(), luma_in


def ref_search(L, rec, src, skip, bd, q):
    h8, w8 = skip.shape
    nvfb, nhfb = (h8 + 7) // 8, (w8 + 7) // 8
    src16 = [np.ascontiguousarray(p.astype(np.uint16)) for p in src]
    mse = np.zeros((2, nvfb * nhfb, 64), np.uint64)
    count = np.zeros(nvfb * nhfb, np.int32)
    dirs, var = np.full((nvfb * nhfb, 8, 8), -1, np.int32), np.full((nvfb * nhfb, 8, 8), -1, np.int32)
    for fbr in range(nvfb):
        for fbc in range(nhfb):
            r = ref_search_fb(L, rec, src16, skip, fbr, fbc, bd, q)
            if r is None:
                continue
            fb = fbr * nhfb + fbc
            mse[:, fb], count[fb] = r[0], r[1]
            for by, bx in build_dlist(skip, fbr, fbc)[1]:
                dirs[fb, by, bx], var[fb, by, bx] = r[2][by, bx], r[3][by, bx]
    return mse, count, dirs, var


def ref_apply(L, rec, skip, bd, q, ystr, ustr):
    """av1_cdef_frame: cdef_filter_fb with dirinit = NULL writing the destination at picture stride, from the UNFILTERED input (the
    reference filters in place and restores the unfiltered neighbours from line buffers, EbCdef.c:620-760)"""
    cs = bd - 8
    h8, w8 = skip.shape
    nvfb, nhfb = (h8 + 7) // 8, (w8 + 7) // 8
    out = [p.copy() for p in rec]
    damping = 3 + (q >> 6)
    for fbr in range(nvfb):
        for fbc in range(nhfb):
            ys, us = int(ystr[fbr * nhfb + fbc]), int(ustr[fbr * nhfb + fbc])
            dl, blocks = build_dlist(skip, fbr, fbc)
            if ys < 0 or us < 0 or (ys == 0 and us == 0) or not blocks:
                continue
            dirs, var = np.zeros((16, 16), np.int32), np.zeros((16, 16), np.int32)
            for pli in range(3):
                l2 = 3 - (pli > 0)
                s = us if pli else ys
                sec = s % 4
                inbuf = fill_inbuf(L, rec[pli], fbr, fbc, l2, skip.shape)
                o = out[pli]
                dst = ctypes.c_void_p(o.ctypes.data + o.itemsize * (((fbr * 8) << l2) * o.shape[1] + ((fbc * 8) << l2)))
                L.cdef_filter_fb(dst if bd == 8 else None, None if bd == 8 else dst, o.shape[1], ctypes.c_void_p(inbuf.ctypes.data + 2 * IN0),
                                 int(pli > 0), int(pli > 0), ptr(dirs), None, ptr(var), pli, dl, len(blocks), s // 4, sec + (sec == 3), damping,
                                 damping, cs)
    return out


def adjust_strength(strength, var):
    i = min((var >> 6).bit_length() - 1, 12) if var >> 6 else 0
    return (strength * (4 + i) + 8) >> 4 if var else 0


def np_filter_block(inbuf, by, bx, n, pri, sec, d, damping, cs):
    """one n x n block through the filter, in numpy -> (filtered, clamped?, a tap beyond a tile corner read CDEF_VERY_LARGE?)"""
    a = inbuf.reshape(-1, BSTRIDE).astype(np.int64)
    y0, x0 = VBORDER + by * n, HBORDER + bx * n
    x = a[y0:y0 + n, x0:x0 + n]
    odd = (pri >> cs) & 1
    ptaps, staps = ((3, 3) if odd else (4, 2)), (2, 1)
    total, mn, mx, corner = np.zeros_like(x), x.copy(), x.copy(), False

    def constrain(diff, thr, damp):
        if not thr:
            return np.zeros_like(diff)
        shift = max(0, damp - (thr.bit_length() - 1))
        return np.sign(diff) * np.minimum(np.abs(diff), np.maximum(0, thr - (np.abs(diff) >> shift)))
    for k in range(2):
        for dd, thr, tap in ((d, pri, ptaps[k]), ((d + 2) & 7, sec, staps[k]), ((d + 6) & 7, sec, staps[k])):
            dy, dx = DIRS[dd][k]
            for sg in (1, -1):
                p = a[y0 + sg * dy:y0 + sg * dy + n, x0 + sg * dx:x0 + sg * dx + n]
                total = total + tap * constrain(p - x, thr, damping)
                mx = np.where(p != LARGE, np.maximum(mx, p), mx)
                mn = np.minimum(mn, p)
                if dy and dx:
                    corner |= bool((p[0, 0] == LARGE and a[y0 + sg * dy, x0] == LARGE and a[y0, x0 + sg * dx] == LARGE) or
                                   (p[-1, -1] == LARGE and a[y0 + n - 1 + sg * dy, x0 + n - 1] == LARGE and a[y0 + n - 1, x0 + n - 1 + sg * dx] == LARGE))
    y = x + ((8 + total - (total < 0)) >> 4)
    return np.clip(y, mn, mx), bool(((y < mn) | (y > mx)).any()), corner


def direct_route_check(L, rec, src, skip, bd, q, fbr, fbc, stats):
    """one filter block: cdef_find_dir_c / cdef_filter_block_c / dist_8x8_16bit_c called directly per 8x8 block give the numbers of the
    cdef_filter_fb + compute_cdef_dist route; the numpy restatement gives the same samples.  Collects the fixture's coverage facts."""
    cs = bd - 8
    src16 = np.ascontiguousarray(src[0].astype(np.uint16))
    mse, count, dirs, var, inbuf = ref_search_fb(L, rec, [src16, None, None][:1] + [np.ascontiguousarray(p.astype(np.uint16)) for p in src[1:]],
                                                 skip, fbr, fbc, bd, q)
    damping = 3 + (q >> 6) + cs
    blocks = build_dlist(skip, fbr, fbc)[1]
    for gi in (0, 5, 22, 63):
        pri, sec = (gi // 4) << cs, (gi % 4 + (gi % 4 == 3)) << cs
        total = 0
        for by, bx in blocks:
            blk = ctypes.c_void_p(inbuf.ctypes.data + 2 * (IN0 + 8 * by * BSTRIDE + 8 * bx))
            v = ctypes.c_int32(0)
            d = L.cdef_find_dir_c(blk, BSTRIDE, ctypes.byref(v), cs)
            assert d == dirs[by, bx] and v.value == var[by, bx]
            out = np.zeros((8, 8), np.uint16)
            adj = adjust_strength(pri, v.value)
            L.cdef_filter_block_c(None, ptr(out), 8, blk, adj, sec, d if pri else 0, damping, damping, BLOCK_8X8, (256 << cs) - 1, cs)
            mine, clamped, corner = np_filter_block(inbuf, by, bx, 8, adj, sec, d if pri else 0, damping, cs)
            assert np.array_equal(mine, out), (gi, by, bx)
            stats["clamped"] |= clamped
            stats["corner"] |= corner
            y, x = (fbr * 8 + by) * 8, (fbc * 8 + bx) * 8
            dist = L.dist_8x8_16bit_c(ctypes.c_void_p(src16.ctypes.data + 2 * (y * src16.shape[1] + x)), src16.shape[1], ptr(out), 8, cs)
            sse = int(((out.astype(np.int64) - src16[y:y + 8, x:x + 8]) ** 2).sum())
            stats["dist_ne_sse"] |= dist != sse
            total += dist
        assert total >> (2 * cs) == int(mse[0, gi]), (gi, total, mse[0, gi])


def generate(names=None):
    """-> {key: array} of the cases named (all by default); each case's generator is seeded by its own name"""
    L = ref_lib()
    assert L is not None, "build oracle/_ref/libsvtref.so first (python __graft_entry__.py)"
    out = {}
    for name, bd, w, h, q, skipkind, content in CASES:
        if names is not None and name not in names:
            continue
        rng = np.random.default_rng([0xCDEF, ord(name)])
        src, rec, skip = make_case(rng, bd, w, h, skipkind, content)
        mse, count, dirs, var = ref_search(L, rec, src, skip, bd, q)
        nfb = len(count)
        ystr = rng.integers(0, 64, nfb).astype(np.int8)
        ustr = rng.integers(0, 64, nfb).astype(np.int8)
        ystr[rng.random(nfb) < 0.15] = -1
        both0 = rng.random(nfb) < 0.15
        ystr[both0], ustr[both0] = 0, 0
        ystr[0], ustr[0] = 37, 0                     # a plane with zero strengths inside a filtered block, both ways round
        if nfb > 2:
            ystr[2], ustr[2] = 0, 26
        app = ref_apply(L, rec, skip, bd, q, ystr, ustr)
        p = name + "_"
        out[p + "meta"] = np.array([bd, w, h, q], np.int32)
        out[p + "skip"], out[p + "mse"], out[p + "count"], out[p + "dir"], out[p + "var"] = skip, mse, count, dirs, var
        out[p + "ystr"], out[p + "ustr"] = ystr, ustr
        for i, c in enumerate("yuv"):
            out[p + "src_" + c], out[p + "rec_" + c], out[p + "out_" + c] = src[i], rec[i], app[i]
    return out


def check_conditions(g, L=None):
    """what the fixture must contain so that it cannot miss the hard paths; with the reference library also the direct-route facts"""
    names = sorted({k.split("_")[0] for k in g})
    dirs = np.concatenate([g[n + "_dir"].ravel() for n in names])
    var = np.concatenate([g[n + "_var"].ravel() for n in names])
    listed = dirs >= 0
    assert set(dirs[listed]) == set(range(8)), sorted(set(dirs[listed]))
    assert (var[listed] == 0).any() and ((var[listed] >> 6) != 0).any()
    classes = {int(g[n + "_meta"][3]) >> 6 for n in names}
    assert classes == {0, 1, 2, 3}, classes
    assert {int(g[n + "_meta"][0]) for n in names} == {8, 10}
    assert any((g[n + "_count"] == 0).all() for n in names) and any((g[n + "_count"] == 64).all() for n in names)
    assert any((g[n + "_count"] == 0).any() and (g[n + "_count"] > 0).any() for n in names)
    assert any(int(g[n + "_meta"][1]) % 64 and int(g[n + "_meta"][2]) % 64 for n in names)
    assert any((g[n + "_out_y"] != g[n + "_rec_y"]).any() for n in names) and any((g[n + "_out_u"] != g[n + "_rec_u"]).any() for n in names)
    if L is not None:
        stats = dict(clamped=False, corner=False, dist_ne_sse=False)
        for n in ("b", "e", "g", "h"):
            rec, src = [g[n + "_rec_" + c] for c in "yuv"], [g[n + "_src_" + c] for c in "yuv"]
            bd, w, h, q = (int(v) for v in g[n + "_meta"])
            nhfb = (w + 63) // 64
            some = np.flatnonzero(g[n + "_count"])
            for fb in (some[0], some[-1]):          # the first and the last filter block that is not left out
                direct_route_check(L, rec, src, g[n + "_skip"], bd, q, int(fb) // nhfb, int(fb) % nhfb, stats)
        assert all(stats.values()), stats


if __name__ == "__main__":
    g = generate()
    check_conditions(g, ref_lib())
    np.savez_compressed(OUT, **g)
    print(f"wrote {OUT}: {os.path.getsize(OUT)} bytes, {len(g)} arrays", file=sys.stderr)

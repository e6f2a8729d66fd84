"""Writes tests/golden/dlf.npz: the deblocking fixture.  Runs where the reference's sources are; the tests read the fixture only.

The reference's Codec/EbDeblockingFilter.c and ASM_SSE2/EbDeblockingFilter_Intrinsic_SSE2.c are not in oracle/'s compiled subset, so
this script compiles them where they lie (the flags and the objcopy --weaken step of oracle/Makefile), next to the project's own
harness tests/c/ref_dlf.c, into oracle/_ref/libsvtref_dlf.so; the leftover symbols (Log2f_SSE2, eb_memcpy, av1_ac_quant_Q3) resolve
against oracle/_ref/libsvtref.so.

What is recorded, all of it the reference's own output:
  filters   the sixteen aom_[highbd_]lpf_{vertical,horizontal}_{4,6,8,14} entries the reference's macros select (_sse2) on four-line
            edge units, random ones and flat ones with a step; asserted equal to the _c versions where the reference has both
  pictures  av1_loop_filter_frame(recon, pcs, 0, 3) per case
  tables    av1_loop_filter_frame + PictureSseCalculations per plane and level, all 64 levels
  walks     av1_pick_filter_level(LPF_PICK_FROM_FULL_IMAGE) whole, both loop_filter_mode branches and both tx_mode cases
  from_q    av1_pick_filter_level(LPF_PICK_FROM_Q) over every qindex, key and non-key, 8 and 10 bit
and what the cases cover, asserted here (at least MIN_COVER each) and stored as `cover_*`: edges of every length per plane class and
direction (counted with the plain model of the edge decision in tests/dlf_cases.py, which the pictures themselves confirm), and lines
per class (13-tap, 7-tap, filter4 only, unchanged) from the reference's output - on the edge units for all sixteen filters, and in the
pictures for luma, whose vertical pass the reference runs alone when the horizontal level is 0.  Chroma has one level for both
directions, so its passes cannot be told apart in a picture; its line classes are the edge units'."""
import ctypes
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import dlf_cases as dc  # noqa: E402

REF = os.environ.get("SVT_REF", "/root/reference")
MIN_COVER = 20
SHAPE_OFF = (0, 1, 3, 5, 8, 11, 14, 17, 21)
SHAPE_N = (1, 2, 2, 3, 3, 3, 3, 4, 4)
STATE = {"n64": 0}


def build_ref_lib():
    rc = os.path.join(REF, "Source", "Lib", "Common")
    flags = ["-O2", "-mavx2", "-fPIC", "-w", "-I" + os.path.join(REF, "Source", "API")] + \
        ["-I" + os.path.join(rc, d) for d in ("Codec", "C_DEFAULT", "ASM_SSE2", "ASM_SSSE3", "ASM_SSE4_1", "ASM_AVX2")]
    out = os.path.join(ROOT, "oracle", "_ref")
    obj = os.path.join(out, "obj_dlf")
    os.makedirs(obj, exist_ok=True)
    assert os.path.exists(os.path.join(out, "libsvtref.so")), "build oracle/_ref/libsvtref.so first (make -C oracle ref)"
    objs = []
    for src in (os.path.join(rc, "Codec", "EbDeblockingFilter.c"), os.path.join(rc, "ASM_SSE2", "EbDeblockingFilter_Intrinsic_SSE2.c"),
                os.path.join(ROOT, "tests", "c", "ref_dlf.c")):
        o = os.path.join(obj, os.path.basename(src)[:-2] + ".o")
        subprocess.check_call(["gcc"] + flags + ["-c", src, "-o", o + ".tmp.o"])
        subprocess.check_call(["objcopy", "--weaken", o + ".tmp.o", o])
        os.remove(o + ".tmp.o")
        objs.append(o)
    subprocess.check_call(["gcc", "-shared", "-o", dc.REF_DLF] + objs + ["-L" + out, "-Wl,--no-as-needed", "-lsvtref", "-Wl,-rpath,$ORIGIN", "-lm"])      # every reference is weak: keep the dependency


class BlkGeom(ctypes.Structure):
    _fields_ = [("sqi_mds", ctypes.c_uint16), ("bsize", ctypes.c_uint8), ("shape", ctypes.c_uint8), ("depth", ctypes.c_uint8), ("nsi", ctypes.c_uint8),
                ("totns", ctypes.c_uint8), ("d1i", ctypes.c_uint8), ("origin_x", ctypes.c_uint8), ("origin_y", ctypes.c_uint8), ("bwidth", ctypes.c_uint8),
                ("bheight", ctypes.c_uint8), ("sq_size", ctypes.c_uint8), ("is_last_quadrant", ctypes.c_uint8), ("has_uv", ctypes.c_uint8), ("pad", ctypes.c_uint8)]


def geometry():
    import __graft_entry__ as ge
    lib = ge.load_package().load_library()
    geo = []
    for i in range(1101):
        g = BlkGeom()
        assert lib.svt_hip_blk_geom_mds(i, ctypes.byref(g)) == 0
        geo.append(g)
    squares = {(g.origin_x, g.origin_y, g.sq_size): i for i, g in enumerate(geo) if g.shape == 0}
    return geo, squares


def draw_tree(rng, geo, squares, w, h, sbx, sby, kind):
    """a partition tree of the superblock at (sbx, sby) -> [(mds, x, y)] in coding order; a square that is not wholly inside the picture
    splits"""
    out = []

    def rec(x, y, size):
        sqi = squares[(x, y, size)]
        px, py = sbx + x, sby + y
        if px >= w or py >= h:
            return
        inside = px + size <= w and py + size <= h
        nshapes = 9 if size >= 16 else (3 if size == 8 else 1)
        split_p = {64: 0.6, 32: 0.35, 16: 0.3, 8: 0.3}.get(size, 0.0)
        cycle = size == 64 and inside and w > 72            # whole superblocks of the larger pictures: split every other one, and
        if cycle:                                           # give the others the nine 64-wide shapes in turn
            STATE["n64"] += 1
        if size > 4 and (not inside or (STATE["n64"] % 2 == 1 if cycle else rng.random() < split_p)):
            hs = size // 2
            for qy, qx in ((0, 0), (0, 1), (1, 0), (1, 1)):
                rec(x + qx * hs, y + qy * hs, hs)
            return
        shape = (STATE["n64"] // 2) % 9 if cycle else (int(rng.integers(0, nshapes)) if rng.random() < 0.7 else 0)
        for nsi in range(SHAPE_N[shape]):
            mds = sqi + SHAPE_OFF[shape] + nsi
            g = geo[mds]
            assert g.shape == shape and g.nsi == nsi
            out.append((mds, sbx + g.origin_x, sby + g.origin_y))

    rec(0, 0, 64)
    return out


def draw_grid(rng, geo, squares, w, h, kind):
    """-> mi [h / 4][w / 4][4], final [nsb][256][3] uint32, final_count [nsb], info [nsrc][4]"""
    sb_cols, sb_rows = (w + 63) // 64, (h + 63) // 64
    mi = np.zeros((h // 4, w // 4, 4), np.uint8)
    final = np.zeros((sb_cols * sb_rows, 256, 3), np.uint32)
    count = np.zeros(sb_cols * sb_rows, np.uint32)
    info = []
    for sb in range(sb_cols * sb_rows):
        blocks = draw_tree(rng, geo, squares, w, h, (sb % sb_cols) * 64, (sb // sb_cols) * 64, kind)
        assert len(blocks) <= 256
        count[sb] = len(blocks)
        for k, (mds, x, y) in enumerate(blocks):
            g = geo[mds]
            inter = kind == "allskip" or rng.random() < 0.5
            if inter:
                ref, mode = int(rng.integers(1, 8)), int(rng.integers(13, 25))
                skip = 1 if kind == "allskip" else int(rng.random() < 0.5)
            else:
                ref, mode = 0, (26 if rng.random() < 0.1 else int(rng.integers(0, 13)))      # INTRA_MODE_4x4 now and then
                skip = int(rng.random() < 0.3)
            src = len(info)
            info.append((ref, mode, skip, 0))
            part = g.shape if g.shape < 3 else g.shape + 1
            final[sb, k] = (mds | x << 16, y | g.bsize << 16 | part << 24, src)
            tw, th = g.bwidth, g.bheight
            if kind == "allskip" and tw >= 8 and th >= 8 and rng.random() < 0.5:
                tw, th = tw // 2, th // 2                       # a transform edge inside the block: between skipped units only a PU edge is filtered
            mi[y // 4:(y + g.bheight) // 4, x // 4:(x + g.bwidth) // 4] = (g.bsize, dc.tx_of(tw, th), ref | skip << 7, mode)
    return mi, final, count, np.array(info, np.uint8)


def draw_picture(rng, w, h, bd, mi):
    """smooth content plus a per-block offset of a few levels and grain (the reconstruction); the source is the smooth content with
    other grain.  On noise alone the flat masks never fire."""
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import svtlibs
    rec, src = [], []
    for pl in range(3):
        pw, ph = (w, h) if pl == 0 else (w // 2, h // 2)
        base = svtlibs.smooth_picture(rng, ph + 8, pw + 8, grain=0)[:ph, :pw].astype(np.int32)
        base = 64 + base // 2                                   # gentle slopes, away from the clipping ends
        base[:, :pw // 2] = base[:, :pw // 2] // 16 * 16      # one half in plateaus: the flat masks need runs of equal samples
        off = np.zeros((ph, pw), np.int32)
        seen = {}
        ss = 1 if pl else 0
        step = 4 >> ss                                          # samples of this plane per mode-info unit
        for y in range(0, ph, step):
            for x in range(0, pw, step):
                m = mi[(y << ss) >> 2, (x << ss) >> 2]
                key = (int(m[0]), int(m[2]), int(m[3]))
                if key not in seen:       # an offset per kind of block; half the kinds are painted flat, a few levels apart
                    seen[key] = (int(rng.integers(-4, 5)), rng.random() < 0.5, 96 + int(rng.integers(-5, 6)))
                o, painted, level = seen[key]
                off[y:y + step, x:x + step] = level - base[y:y + step, x:x + step] if painted else o
        flat = rng.random((ph // 4 + 1, pw // 4 + 1)) < 0.75      # three in four 4x4s carry no grain, so flat runs exist
        grain = rng.integers(-2, 3, (ph, pw)) * (~np.kron(flat, np.ones((4, 4), bool))[:ph, :pw])
        r = base + off + grain
        s = base + rng.integers(-1, 2, (ph, pw))
        if bd == 10:
            r, s = r * 4 + rng.integers(0, 4, (ph, pw)) * (grain != 0), s * 4 + rng.integers(0, 4, (ph, pw))
        dt = np.uint8 if bd == 8 else np.uint16
        rec.append(r.clip(0, (1 << bd) - 1).astype(dt))
        src.append(s.clip(0, (1 << bd) - 1).astype(dt))
    return rec, src


def row_of(w, h, bd, levels, sharp, delta=0, rd=(0,) * 8, md=(0, 0)):
    return np.array([w, h, bd] + list(levels) + [sharp, delta] + list(rd) + list(md), np.int32)


def line_classes(before, after, x, y, dirn, length):
    """per line of the edge unit at (x, y): 0 unchanged, 1 only p1 .. q1 changed, 2 p2 / q2 changed but not p5 / q5, 3 p5 or q5 changed"""
    out = []
    for k in range(4):
        if dirn == 0:
            d = (before[y + k, max(x - 7, 0):x + 7].astype(np.int32) != after[y + k, max(x - 7, 0):x + 7]).astype(int)
            c = x - max(x - 7, 0)
        else:
            d = (before[max(y - 7, 0):y + 7, x + k].astype(np.int32) != after[max(y - 7, 0):y + 7, x + k]).astype(int)
            c = y - max(y - 7, 0)
        far = d[:max(c - 3, 0)].sum() + d[c + 3:].sum()
        mid = d[max(c - 3, 0):c - 2].sum() + d[c + 2:c + 3].sum()
        out.append(3 if far and length == 14 else (2 if mid or far else (1 if d.any() else 0)))
    return out


def filter_units(L, rng, out):
    """the sixteen filters on edge units: [bd][dir][len] -> in / par / out"""
    n = 48
    lens = (4, 6, 8, 14)
    fin = np.zeros((2, 2, 4, n, 4, 16), np.uint16)
    par = np.zeros((2, 2, 4, n, 3), np.uint8)
    fout = np.zeros_like(fin)
    classes = np.zeros((2, 2, 4, 4), np.int64)
    for b, bd in enumerate((8, 10)):
        sh = bd - 8
        dt = np.uint8 if bd == 8 else np.uint16
        for dirn in range(2):
            for li, length in enumerate(lens):
                for i in range(n):
                    step = int(rng.integers(2, 17)) * (1 if rng.random() < 0.5 else -1)
                    level, sharp = int(rng.integers(abs(step) if i % 2 == 0 else 1, 64)), int(rng.choice((0, 3, 7)))
                    lim = level >> ((sharp > 0) + (sharp > 4))
                    if sharp > 0:
                        lim = min(lim, 9 - sharp)
                    lim = max(lim, 1)
                    p = (2 * (level + 2) + lim, lim, level >> 4)
                    if i % 2 == 0:       # a flat unit with a step across the edge, and now and then a ripple
                        a = int(rng.integers(40, 200))
                        u = np.full((4, 16), a, np.int32)
                        u[:, 8:] += step
                        u += (rng.integers(-1, 2, (4, 16)) * (rng.random((4, 1)) < 0.3))
                        if i % 4 == 2:   # flat next to the edge only: the 8-tap's smoothing inside a 14-tap edge
                            u[:, :4] += rng.integers(-9, 10, (4, 4))
                            u[:, 12:] += rng.integers(-9, 10, (4, 4))
                    else:
                        u = int(rng.integers(30, 220)) + rng.integers(-10, 11, (4, 16)) // (1 if i % 4 == 1 else 4)
                    u = (u << sh) + (rng.integers(0, 1 << sh, (4, 16)) if sh and i % 8 >= 4 else 0)
                    u = u.clip(0, (1 << bd) - 1)
                    res = []
                    for flavour in (0, 1):
                        buf = rng.integers(0, 1 << bd, (32, 32)).astype(dt)
                        if dirn == 0:
                            buf[8:12, 8:24] = u
                            s = buf[8:, 16:]
                        else:
                            buf[8:24, 8:12] = u.T
                            s = buf[16:, 8:]
                        rc = L.ref_dlf_filter(flavour, dirn, length, bd, s.ctypes.data, 32, p[0], p[1], p[2])
                        res.append(None if rc else (buf[8:12, 8:24].copy() if dirn == 0 else buf[8:24, 8:12].T.copy()))
                    if res[1] is not None:
                        assert (res[0] == res[1]).all(), ("the _sse2 and _c filters differ", bd, dirn, length)
                    fin[b, dirn, li, i], par[b, dirn, li, i], fout[b, dirn, li, i] = u, p, res[0]
                    for c in line_classes(u.astype(dt), res[0], 8, 0, 0, length):
                        classes[b, dirn, li, c] += 1
    out["filt_in"], out["filt_par"], out["filt_out"], out["cover_filter_lines"] = fin, par, fout, classes
    # every class a length has, on the unit fixtures: 4 and 6 change at most p1 .. q1, 8 reaches p2, 14 reaches p5
    for b in range(2):
        for dirn in range(2):
            for li, top in enumerate((1, 1, 2, 3)):
                assert (classes[b, dirn, li, :top + 1] >= MIN_COVER).all(), ("filter units", b, dirn, lens[li], classes[b, dirn, li])


def main():
    build_ref_lib()
    L = dc.ref_dlf()
    geo, squares = geometry()
    rng = np.random.default_rng(20261020)
    out = {}
    filter_units(L, rng, out)

    pics = {}
    for name, w, h, bd, kind in (("sb1", 64, 64, 8, "mixed"), ("sb1s", 64, 64, 8, "allskip"), ("edge", 200, 136, 8, "mixed"),
                                 ("wide", 328, 200, 8, "mixed"), ("hbd", 72, 72, 10, "mixed")):
        mi, final, count, info = draw_grid(rng, geo, squares, w, h, kind)
        rec, src = draw_picture(rng, w, h, bd, mi)
        pics[name] = (rec, src, mi)
        out[name + "_mi"], out[name + "_final"], out[name + "_final_count"], out[name + "_info"] = mi, final, count, info
        for p, r, s in zip(dc.PLANES, rec, src):
            out[f"{name}_rec_{p}"] = r
            out[f"{name}_dsrc_{p}"] = (s.astype(np.int32) - r).astype(np.int16 if bd > 8 else np.int8)
            assert ((r.astype(np.int32) + out[f"{name}_dsrc_{p}"]) == s).all()
    rd = (6, -12, 0, -3, 2, -20, 1, -1)
    cases = (
        ("sb1_mixed", "sb1", row_of(64, 64, 8, (24, 24, 16, 16), 0)),
        ("sb1_allskip", "sb1s", row_of(64, 64, 8, (20, 20, 20, 20), 3)),
        ("edge_mixed", "edge", row_of(200, 136, 8, (30, 12, 20, 8), 3)),
        ("edge_luma0", "edge", row_of(200, 136, 8, (0, 0, 20, 20), 0)),
        ("edge_vonly", "edge", row_of(200, 136, 8, (28, 0, 0, 9), 7)),
        ("wide_delta", "wide", row_of(328, 200, 8, (10, 10, 6, 6), 7, 1, rd, (0, -8))),
        ("wide_high", "wide", row_of(328, 200, 8, (50, 44, 38, 40), 0, 1, rd, (3, -8))),
        ("hbd_mixed", "hbd", row_of(72, 72, 10, (40, 40, 36, 36), 0)),
        ("hbd_delta", "hbd", row_of(72, 72, 10, (14, 9, 12, 7), 3, 1, rd, (0, -8))),
    )
    out["cases"] = np.array([c[0] for c in cases])
    # coverage: edges per (plane class, direction, length), luma lines per class (the vertical pass alone is the reference's own run
    # with the horizontal luma level 0), units with curr_level 0 and pv_lvl not
    cover_edges = np.zeros((2, 2, 15), np.int64)
    cover_lines = np.zeros((2, 15, 4), np.int64)
    cover_pv_level = 0
    for name, pic, row in cases:
        rec, src, mi = pics[pic]
        res = dc.ref_frame(row, rec, mi)
        out[name + "_pic"], out[name + "_params"] = np.array(pic), row
        for p, r, o in zip(dc.PLANES, rec, res):
            out[f"{name}_diff_{p}"] = (o.astype(np.int32) - r).astype(np.int16)
        out[name + "_sse"] = dc.ref_table(row, rec, src, mi)
        plain = np.array([((s.astype(np.int64) - r) ** 2).sum() for r, s in zip(rec, src)], np.uint64)
        assert (out[name + "_sse"][:, 0] == plain).all(), "level 0 is the unfiltered plane's SSE"
        vrow = row.copy(); vrow[dc.P_L1] = 0
        vonly = dc.ref_frame(vrow, rec, mi)[0] if row[dc.P_L0] else rec[0]
        for plane in range(3):
            for dirn in range(2):
                for (x, y, length, level) in dc.edge_units(row, mi, plane, dirn):
                    cover_edges[min(plane, 1), dirn, length] += 1
                    if plane == 0 and (row[dc.P_L0] or dirn == 1):
                        before, after = (rec[0], vonly) if dirn == 0 else (vonly, res[0])
                        for c in line_classes(before, after, x, y, dirn, length):
                            cover_lines[dirn, length, c] += 1
                    if row[dc.P_DELTA]:
                        ss = 1 if plane else 0
                        cur = mi[ss | ((y << ss) >> 2), ss | ((x << ss) >> 2)]
                        cover_pv_level += dc.unit_level(row, plane, dirn, int(cur[2]) & 7, int(cur[3])) == 0
    out["cover_edges"], out["cover_lines"], out["cover_pv_level"] = cover_edges, cover_lines, np.array(cover_pv_level)
    for dirn in range(2):
        for length in (4, 8, 14):
            assert cover_edges[0, dirn, length] >= MIN_COVER, ("luma edges", dirn, length, cover_edges[0, dirn])
        for length in (4, 6):
            assert cover_edges[1, dirn, length] >= MIN_COVER, ("chroma edges", dirn, length, cover_edges[1, dirn])
        assert (cover_lines[dirn, 14] >= MIN_COVER).all(), ("14-tap lines", dirn, cover_lines[dirn, 14])
        assert (cover_lines[dirn, 8, :3] >= MIN_COVER).all(), ("8-tap lines", dirn, cover_lines[dirn, 8])
        assert (cover_lines[dirn, 4, :2] >= MIN_COVER).all(), ("4-tap lines", dirn, cover_lines[dirn, 4])
    assert cover_pv_level >= MIN_COVER, ("curr_level 0 with pv_lvl non-zero", cover_pv_level)

    # the walk, whole: LPF_PICK_FROM_FULL_IMAGE on two pictures, both loop_filter_mode branches, both tx_mode cases, a few starts.
    # The pick stores its own sharpness (0 on a key frame, LF_SHARPNESS otherwise); the table it walks is recorded at that sharpness.
    walks, walk_tables = [], {}
    for pic, w, h, bd in (("sb1", 64, 64, 8), ("hbd", 72, 72, 10), ("edge", 200, 136, 8)):
        rec, src, mi = pics[pic]
        for lfm in (1, 3):
            for only4 in (0, 1):
                for last in ((0, 0, 0, 0), (0, 0, 20, 5), (7, 3, 40, 63), (12, 12, 9, 33)):
                    row = row_of(w, h, bd, last, 0)
                    levels, sharp = dc.ref_pick(row, 0, rec, src, mi, loop_filter_mode=lfm, tx_mode_only_4x4=only4, is_key_frame=0)
                    if (pic, sharp) not in walk_tables:
                        walk_tables[(pic, sharp)] = dc.ref_table(row_of(w, h, bd, (0, 0, 0, 0), sharp), rec, src, mi)
                    walks.append([lfm, only4] + list(last) + [int(v) for v in levels] + [sharp, ("sb1", "hbd", "edge").index(pic)])
    out["walks"] = np.array(walks, np.int32)
    out["walk_pics"] = np.array(["sb1", "hbd", "edge"])
    for (pic, sharp), t in walk_tables.items():
        out[f"walk_table_{pic}_{sharp}"] = t
    # LPF_PICK_FROM_Q over every qindex
    fq = np.zeros((2, 2, 256, 4), np.int32)
    for b, bd in enumerate((8, 10)):
        for key in (0, 1):
            for q in range(256):
                fq[b, key, q], _ = dc.ref_pick(row_of(64, 64, bd, (0, 0, 0, 0), 0), 1, None, None, None, is_key_frame=key, base_qindex=q)
    out["from_q"] = fq
    np.savez_compressed(dc.FIXTURE, **out)
    print("wrote", dc.FIXTURE, os.path.getsize(dc.FIXTURE), "bytes")
    print("edges [class][dir][len]", cover_edges[:, :, (4, 6, 8, 14)].tolist())
    print("luma lines [dir][len][class]", cover_lines[:, (4, 8, 14)].tolist(), "pv_level", cover_pv_level)


if __name__ == "__main__":
    main()

"""Writes tests/golden/me_subpel.npz: the sub-pel motion estimation fixture.  Runs where the reference's sources are; the tests read the
fixture only.

The reference's AVC-style interpolation filters (Codec/EbAvcStyleMcp.c, ASM_SSSE3/EbAvcStyleMcp_Intrinsic_SSSE3.c,
ASM_SSE2/EbAvcStyleMcp_Intrinsic_SSE2.c) are not in oracle/'s compiled subset, so this script compiles them where they lie (the flags
and the objcopy --weaken step of make_golden_dlf.py), next to the project's own harness tests/c/ref_me_subpel.c, into
oracle/_ref/libsvtref_me_subpel.so; the leftover symbols resolve against oracle/_ref/libsvtref.so.

What is recorded, all of it the reference's own output:
  planes    pos_b / pos_h / pos_j of InterpolateSearchRegionAVC on a few search windows
  half      SAD, SSD, vector and direction rows after HalfPelSearch_LCU alone
  quarter   SAD, SSD and vector rows after QuarterPelSearch_LCU
  lcu       MotionEstimateLcu whole with use_subpel_flag = 1 on every SB of each case
  var       half / quarter of one case with the stage's enables switched off one at a time
The stage's inputs (`full`: the full-pel rows, `area`: each list's search area) are the reference's too: MotionEstimateLcu with
use_subpel_flag = 0 through oracle/ref_me.c.  With every enable on, the quarter rows are asserted equal to the lcu rows.

The pictures: a smooth base picture is the list-0 reference; the source is that picture displaced per 16x16 tile by a quarter-pel amount
(bilinear resampling) plus a little noise, so the refinement really moves; the list-1 reference is the base displaced as a whole by
another quarter-pel amount.  Some tiles move beyond the search area (full-pel winners on the area's edges and corners), one SB is flat
(every position ties) and one SB is an exact copy (SAD 0: the refinement leaves it integer).

What the cases cover is counted from the reference's outputs, asserted (at least MIN_COVER each) and stored as `cover_*`.

CPU only; run from the repository root after build():  python tests/golden/make_golden_me_subpel.py"""
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import me_subpel_cases as sp  # noqa: E402
import svtlibs  # noqa: E402

REF = os.environ.get("SVT_REF", "/root/reference")
MIN_COVER = 20
SIZES = {"edge": (136, 72), "full": (192, 128)}          # 3 x 2 SBs with an 8-wide partial column and an 8-high partial row; interior SBs
LCU_KEYS = ("best_sad", "best_mv", "area_origin", "bipred_sad", "results")

# (name, picture, keywords of svtlibs.me_lcu_params).  slice_type: B 0 / P 1; pic_depth_mode <= 1: 209 PUs, else 85;
# fractional_search_method: SUB_SAD 0, FULL_SAD 1, SSD 2
CASES = [
    ("p_edge_sub", "edge", dict(slice_type=1, pic_depth_mode=2, fractional_search_method=0, search_area_width=16, search_area_height=8)),
    ("b_edge_fullsad_nsq", "edge", dict(slice_type=0, pic_depth_mode=0, fractional_search_method=1, search_area_width=8, search_area_height=8)),
    ("b_edge_ssd_cu8", "edge", dict(slice_type=0, pic_depth_mode=2, fractional_search_method=2, cu8x8_mode=1, enable_hme_flag=0, search_area_width=16,
                                    search_area_height=8)),
    ("b_full_samepoc_ssd_nsq", "full", dict(slice_type=0, pic_depth_mode=0, fractional_search_method=2, ref1_poc=8, search_area_width=64,
                                            search_area_height=32)),
    ("b_full_sub_nsq", "full", dict(slice_type=0, pic_depth_mode=0, fractional_search_method=0, enable_hme_flag=0, search_area_width=16,
                                    search_area_height=8)),
    ("b_full_fullsad_avx2", "full", dict(slice_type=0, pic_depth_mode=2, fractional_search_method=1, asm_type=1, search_area_width=8, search_area_height=8)),
    ("p_edge_narrow_nsq", "edge", dict(slice_type=1, pic_depth_mode=0, fractional_search_method=0, temporal_layer_index=0, search_area_width=8,
                                       search_area_height=7)),
]
VARIANT_CASE = "b_edge_fullsad_nsq"
# (fractional_search64x64, half 32x32, half 16x16, half 8x8, quarter)
VARIANTS = [(0, 1, 1, 1, 1), (1, 0, 1, 1, 1), (1, 1, 0, 1, 0), (1, 1, 1, 0, 1), (0, 0, 0, 0, 0)]
PLANE_WINDOWS = [("p_edge_sub", 0, 0), ("p_edge_sub", 5, 0), ("b_full_samepoc_ssd_nsq", 4, 1)]      # (case, SB, list)


def build_ref_lib():
    rc = os.path.join(REF, "Source", "Lib", "Common")
    flags = ["-O2", "-mavx2", "-fPIC", "-w", "-I" + os.path.join(REF, "Source", "API")] + \
        ["-I" + os.path.join(rc, d) for d in ("Codec", "C_DEFAULT", "ASM_SSE2", "ASM_SSSE3", "ASM_SSE4_1", "ASM_AVX2")]
    out = os.path.join(ROOT, "oracle", "_ref")
    obj = os.path.join(out, "obj_me_subpel")
    os.makedirs(obj, exist_ok=True)
    assert os.path.exists(os.path.join(out, "libsvtref.so")), "build oracle/_ref/libsvtref.so first (make -C oracle ref)"
    objs = []
    for src in (os.path.join(rc, "Codec", "EbAvcStyleMcp.c"), os.path.join(rc, "ASM_SSSE3", "EbAvcStyleMcp_Intrinsic_SSSE3.c"),
                os.path.join(rc, "ASM_SSE2", "EbAvcStyleMcp_Intrinsic_SSE2.c"), os.path.join(ROOT, "tests", "c", "ref_me_subpel.c")):
        o = os.path.join(obj, os.path.basename(src)[:-2] + ".o")
        subprocess.check_call(["gcc"] + flags + ["-c", src, "-o", o + ".tmp.o"])
        subprocess.check_call(["objcopy", "--weaken", o + ".tmp.o", o])
        os.remove(o + ".tmp.o")
        objs.append(o)
    subprocess.check_call(["gcc", "-shared", "-o", sp.REF_LIB] + objs + ["-L" + out, "-Wl,--no-as-needed", "-lsvtref", "-Wl,-rpath,$ORIGIN", "-lm"])


def shifted(base, y0, x0, h, w, qx, qy):
    """base resampled at (y + qy / 4, x + qx / 4) for the h x w block at (y0, x0): bilinear, rounded"""
    ix, iy, fx, fy = qx >> 2, qy >> 2, qx & 3, qy & 3
    a = base[y0 + iy:y0 + iy + h + 1, x0 + ix:x0 + ix + w + 1].astype(np.int64)
    v = (4 - fy) * ((4 - fx) * a[:-1, :-1] + fx * a[:-1, 1:]) + fy * ((4 - fx) * a[1:, :-1] + fx * a[1:, 1:])
    return (v + 8) >> 4


def pictures():
    """{picture: (source, list-0 reference, list-1 reference)} uint8 [H, W]"""
    rng = np.random.default_rng(8162_8236)
    out = {}
    for name, (W, H) in SIZES.items():
        M = 96
        base = svtlibs.smooth_picture(rng, H + 2 * M, W + 2 * M, grain=0).astype(np.int64)
        base = (base + 12 * np.sin(np.arange(W + 2 * M)[None, :] / 2.3) + 12 * np.cos(np.arange(H + 2 * M)[:, None] / 1.9)).clip(0, 255).astype(np.uint8)
        ref0 = np.ascontiguousarray(base[M:M + H, M:M + W])
        ref1 = shifted(base, M, M, H, W, -11, 5).astype(np.uint8)              # the whole picture 2.75 left, 1.25 down
        src = np.zeros((H, W), np.int64)
        far = [(-38, -22), (38, -22), (-38, 22), (38, 22), (-38, 1), (38, -2), (3, -22), (-1, 22)]      # beyond an 8- or 16-wide area: edges, corners
        k = 0
        for y in range(0, H, 16):
            for x in range(0, W, 16):
                h, w = min(16, H - y), min(16, W - x)
                if k % 5 == 4:
                    qx, qy = far[(k // 5) % 8]
                else:
                    qx, qy = int(rng.integers(-13, 14)), int(rng.integers(-9, 10))
                k += 1
                src[y:y + h, x:x + w] = shifted(base, M + y, M + x, h, w, qx, qy)
        src = src + rng.integers(-1, 2, (H, W))
        sbx1 = 64
        # one SB an exact copy of the list-0 reference (SAD 0 at (0, 0): the refinement leaves it integer), one flat on flat references
        src[0:64, 0:64] = ref0[0:64, 0:64]
        src = src.clip(0, 255).astype(np.uint8)
        src[0:64, sbx1:sbx1 + 64] = 128
        ref0[0:72 if H > 72 else 64, sbx1 - 8:sbx1 + 66] = 128
        ref1[0:72 if H > 72 else 64, sbx1 - 8:sbx1 + 66] = 128
        if name == "edge":      # the last (8-wide) SB column repeats the reference's last sample column: it matches the right padding best
            src[:, 128:] = (ref0[:, -1:].astype(np.int64) + rng.integers(-1, 2, (H, 8))).clip(0, 255)
        out[name] = (src, ref0, np.ascontiguousarray(ref1))
    return out


def area_size(prm, xo, yo):
    """the clipped size of a list's search area from its origin (MotionEstimateLcu :7955-8040: only the right / bottom edges shrink it)"""
    saw, sah = (int(prm[13]) + 7) & ~7, int(prm[14])
    W, H, ox, oy = int(prm[0]), int(prm[1]), int(prm[2]), int(prm[3])
    if ox + xo + saw > W:
        saw = max(1, saw - (ox + xo + saw - W))
    if saw >= 8:
        saw &= ~7
    if oy + yo + sah > H:
        sah = max(1, sah - (oy + yo + sah - H))
    return saw, sah


def case_params(name):
    _, pic, kw = next(c for c in CASES if c[0] == name)
    W, H = SIZES[pic]
    geo = svtlibs.me_pyramid(np.zeros((H, W), np.uint8))[1]
    return pic, [svtlibs.me_lcu_params(W, H, sx, sy, geo, **kw) for sy in range(0, H, 64) for sx in range(0, W, 64)]


def stage_flags(prm, enables=(1, 1, 1, 1, 1)):
    """flg[] of ref_me_subpel_stage from an lcu parameter block"""
    return [int(prm[24])] + list(enables) + [int(prm[23] == 1), int(prm[25] == 209), int(prm[21])]


def run_lcu(L, prm, pyr):
    import ctypes
    bufs = (ctypes.c_void_p * 9)(*[p.ctypes.data for planes in pyr for p in planes])
    out = dict(best_sad=np.zeros((2, 209), np.uint32), best_mv=np.zeros((2, 209), np.uint32), area_origin=np.zeros((2, 2), np.int16),
               bipred_sad=np.zeros(209, np.uint32), results=np.zeros((209, 11), np.int32), best_ssd=np.zeros((2, 209), np.uint32))
    rc = L.ref_me_subpel_lcu(sp.ptr(prm), bufs, sp.ptr(out["best_sad"]), sp.ptr(out["best_mv"]), sp.ptr(out["area_origin"]), sp.ptr(out["bipred_sad"]),
                             sp.ptr(out["results"]), sp.ptr(out["best_ssd"]))
    assert rc == 0, rc
    return out


def run_case(L, R, name, pics, enables=(1, 1, 1, 1, 1), with_lcu=True):
    """every SB of one case -> dict of arrays [nsb, ...]"""
    pic, prms = case_params(name)
    pyr = [svtlibs.me_pyramid(p)[0] for p in pics[pic]]
    pad = svtlibs.ME_PADS[0]
    nl = 1 if prms[0][4] == 1 else 2
    d = {k: [] for k in ("full_sad", "full_mv", "area", "half_sad", "half_mv", "half_ssd", "half_dir", "quarter_sad", "quarter_mv", "quarter_ssd") +
         (tuple("lcu_" + k for k in LCU_KEYS + ("best_ssd",)) if with_lcu else ())}
    for prm in prms:
        full = svtlibs.run_me_lcu(R.ref_motion_estimate_lcu, prm, *pyr)
        rows = {k: np.zeros((2, 209), np.uint8 if k == "half_dir" else np.uint32) for k in d if k.startswith(("half", "quarter"))}
        area = np.zeros((2, 4), np.int16)
        for l in range(nl):
            xo, yo = (int(v) for v in full["area_origin"][l])
            saw, sah = area_size(prm, xo, yo)
            area[l] = (xo, yo, saw, sah)
            o = sp.run_ref_stage(L, pyr[0][0], pyr[1 + l][0], pad, int(prm[2]), int(prm[3]), xo, yo, saw, sah, stage_flags(prm, enables), full["best_sad"][l], full["best_mv"][l])
            for k in ("half_sad", "half_mv", "half_ssd", "half_dir"):
                rows[k][l] = o[k]
            for k in ("sad", "mv", "ssd"):
                rows["quarter_" + k][l] = o[k]
        d["full_sad"].append(full["best_sad"]); d["full_mv"].append(full["best_mv"]); d["area"].append(area)
        for k, v in rows.items():
            d[k].append(v)
        if with_lcu:
            lcu = run_lcu(L, prm, pyr)
            for k in LCU_KEYS + ("best_ssd",):
                d["lcu_" + k].append(lcu[k])
            assert np.array_equal(lcu["area_origin"][:nl], full["area_origin"][:nl])
            if tuple(enables) == (1, 1, 1, 1, 1):      # the stage harness and MotionEstimateLcu agree
                assert np.array_equal(lcu["best_sad"][:nl], rows["quarter_sad"][:nl]) and np.array_equal(lcu["best_mv"][:nl], rows["quarter_mv"][:nl]), name
    out = {k: np.array(v) for k, v in d.items()}
    out["prm"] = np.array(prms)
    return out


def coverage(g, pics):
    """the counts the fixture must hold, from the reference's outputs (the model is only asked which branch a recorded row took)"""
    c = dict(frac=np.zeros((2, 16), np.int64), half_dir=np.zeros(8, np.int64), quarter_case=np.zeros(4, np.int64), winner=np.zeros(8, np.int64),
             sign=np.zeros((2, 2), np.int64), ssd=np.zeros(2, np.int64), bipred_frac=np.zeros((2, 16), np.int64), integer=0, narrow=0)
    seen = set()
    for name, pic, kw in CASES:
        prm = g[name + "_prm"]
        p = prm[0]
        nl, npus = (1 if p[4] == 1 else 2), int(p[25])
        seen |= {("slice", int(p[4])), ("pus", npus), ("cu8x8", int(p[23])), ("method", int(p[24])), ("hme", int(p[8])), ("area", int(p[13]), int(p[14]))}
        if p[4] == 0 and p[19] == p[20]:
            seen.add("samepoc")
        no8 = p[23] == 1
        for i in range(len(prm)):
            for l in range(nl):
                xo, yo, saw, sah = (int(v) for v in g[name + "_area"][i, l])
                c["narrow"] += saw < 8
                for n in range(npus):
                    if 21 <= n < 85 and no8:
                        continue
                    x, y = sp.mv_xy(g[name + "_lcu_best_mv"][i, l, n])
                    c["frac"][l, (x & 3) + ((y & 3) << 2)] += 1
                    c["integer"] += (x & 3) == 0 and (y & 3) == 0
                    c["sign"][0, int(x > 0)] += x != 0
                    c["sign"][1, int(y > 0)] += y != 0
                    c["half_dir"][g[name + "_half_dir"][i, l, n]] += 1
                    hx, hy = sp.mv_xy(g[name + "_half_mv"][i, l, n])
                    c["quarter_case"][(hy & 2) + ((hx & 2) >> 1)] += 1
                    fx, fy = sp.mv_xy(g[name + "_full_mv"][i, l, n])
                    sx, sy = (fx >> 2) - xo, (fy >> 2) - yo
                    le, ri, to, bo = sx == 0, sx == saw - 1, sy == 0, sy == sah - 1
                    for k, hit in enumerate((le and not (to or bo), ri and not (to or bo), to and not (le or ri), bo and not (le or ri), le and to, ri and to, le and bo, ri and bo)):
                        c["winner"][k] += bool(hit) and saw > 1 and sah > 1
                    if p[24] == 2:
                        moved = g[name + "_half_mv"][i, l, n] != g[name + "_full_mv"][i, l, n]
                        c["ssd"][int(moved)] += 1
            if nl == 2:
                bip_all = p[23] == 0 or npus == 209
                for pu in range(npus if bip_all else 21):
                    n = sp.RASTER[pu]
                    for l in range(2):
                        x, y = sp.mv_xy(g[name + "_lcu_best_mv"][i, l, n])
                        c["bipred_frac"][l, (x & 3) + ((y & 3) << 2)] += 1
    need = {("slice", 0), ("slice", 1), ("pus", 85), ("pus", 209), ("cu8x8", 0), ("cu8x8", 1), ("method", 0), ("method", 1), ("method", 2), ("hme", 0),
            ("hme", 1), ("area", 8, 8), ("area", 16, 8), ("area", 64, 32), "samepoc"}
    assert need <= seen, sorted(map(str, need - seen))
    return c


def check_conditions(cover):
    """cover: the `cover_*` entries of the fixture (or the dict about to be written)"""
    assert (cover["cover_frac"] >= MIN_COVER).all(), ("final fractional positions [list][pos]", cover["cover_frac"].tolist())
    assert (cover["cover_half_dir"] >= MIN_COVER).all(), ("half-pel directions", cover["cover_half_dir"].tolist())
    assert (cover["cover_quarter_case"] >= MIN_COVER).all(), ("quarter-pel cases", cover["cover_quarter_case"].tolist())
    assert (cover["cover_winner"] >= MIN_COVER).all(), ("full-pel winners on L R T B edges, TL TR BL BR corners", cover["cover_winner"].tolist())
    assert (cover["cover_sign"] >= MIN_COVER).all(), ("negative / positive components [x, y][neg, pos]", cover["cover_sign"].tolist())
    assert (cover["cover_ssd"] >= MIN_COVER).all(), ("SSD branch not updating / updating", cover["cover_ssd"].tolist())
    quarter_positions = [f for f in range(16) if f not in (0, 2, 8, 10)]
    assert (cover["cover_bipred_frac"][:, quarter_positions] >= MIN_COVER).all(), ("QuarterPelCompensation cases [list][pos]", cover["cover_bipred_frac"].tolist())
    assert (cover["cover_bipred_frac"][:, (0, 2, 8, 10)] >= MIN_COVER).all(), ("SelectBuffer cases", cover["cover_bipred_frac"].tolist())
    assert int(cover["cover_integer"]) >= MIN_COVER and int(cover["cover_narrow"]) >= 1, (cover["cover_integer"], cover["cover_narrow"])


def main():
    build_ref_lib()
    L, R = sp.ref_lib(), svtlibs.ref()
    assert L is not None and R is not None
    pics = pictures()
    d = {"cases": np.array([c[0] for c in CASES])}
    for pic, planes in pics.items():
        for i, pl in enumerate(planes):
            d[f"pic_{pic}_{i}"] = pl
    for name, pic, _ in CASES:
        r = run_case(L, R, name, pics)
        for k, v in r.items():
            d[f"{name}_{k}"] = v
    # the stage with its enables off one at a time
    d["var_case"] = np.array(VARIANT_CASE)
    d["var_enables"] = np.array(VARIANTS, np.int32)
    for i, en in enumerate(VARIANTS):
        r = run_case(L, R, VARIANT_CASE, pics, enables=en, with_lcu=False)
        for k in ("half_sad", "half_mv", "half_ssd", "half_dir", "quarter_sad", "quarter_mv", "quarter_ssd"):
            d[f"var{i}_{k}"] = r[k]
    # the planes of a few windows
    pad = svtlibs.ME_PADS[0]
    d["plane_windows"] = np.array([(next(k for k, c in enumerate(CASES) if c[0] == nm), sb, l) for nm, sb, l in PLANE_WINDOWS], np.int32)
    for k, (name, sb, l) in enumerate(PLANE_WINDOWS):
        pic, prms = case_params(name)
        pyr = [svtlibs.me_pyramid(p)[0] for p in pics[pic]]
        xo, yo, saw, sah = (int(v) for v in d[name + "_area"][sb, l])
        o = sp.run_ref_stage(L, pyr[0][0], pyr[1 + l][0], pad, int(prms[sb][2]), int(prms[sb][3]), xo, yo, saw, sah, stage_flags(prms[sb]), d[name + "_full_sad"][sb, l],
                             d[name + "_full_mv"][sb, l], plane_wh=(saw + 64, sah + 64))
        d[f"planes_{k}"] = o["planes"]
    for k, v in coverage(d, pics).items():
        d["cover_" + k] = np.array(v)
    print({k: d[k].tolist() for k in d if k.startswith("cover_")})
    check_conditions(d)
    np.savez_compressed(sp.FIXTURE, **d)
    size = os.path.getsize(sp.FIXTURE)
    assert size < (1 << 20), size
    print(f"wrote {sp.FIXTURE}: {size} bytes, {len(CASES)} cases")


if __name__ == "__main__":
    main()

"""Writes tests/golden/me_frame.npz: MotionEstimateLcu (EbMotionEstimation.c:7527) on EVERY SB of small picture pyramids, computed by
the REFERENCE's own function through oracle/ref_me.c's ref_motion_estimate_lcu in oracle/_ref/libsvtref.so (ctypes, once per SB) -
the expected outputs of svt_hip_motion_estimate_frame: result rows of both lists, search-area origins, bi-prediction SADs, me_results.

The pictures: a textured list-0 reference, a source made of it by a known displacement per picture region plus a little noise (real
minima; a region copied unmoved and a flat block give ties), and a list-1 reference displaced the other way.  On the 160 x 96
picture the 32-wide last SB column of the source repeats the reference's last sample column, so it matches the reference's right
padding best: the HME centre there is about +31 and an 8-wide search area is clipped by the picture edge to fewer than 8 columns.
The pyramids are produced by the reference's Decimation2D and generate_padding (as make_golden.py does for picture.npz) and are
asserted equal to svtlibs.me_pyramid, which the tests use where the reference is absent.

What is this file's own: the pictures, the parameter sets, the loop over SBs and the coverage assertions (check_conditions).
For one SB per case the outputs are asserted equal to the oracle's twin (svt_oracle_me_lcu).

CPU only; run from the repository root after build():  python tests/golden/make_golden_me_frame.py
"""
import ctypes
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
OUT = os.path.join(HERE, "me_frame.npz")
sys.path.insert(0, os.path.join(ROOT, "tests"))
import svtlibs      # noqa: E402

KEYS = ("best_sad", "best_mv", "area_origin", "bipred_sad", "results")
SIZES = {"full": (192, 128), "edge": (160, 96)}      # 3 x 2 whole SBs; partial SBs to the right (32 wide) and at the bottom (32 high)

# (name, picture, keywords of svtlibs.me_lcu_params).  slice_type: B 0 / P 1; pic_depth_mode <= 1: 209 PUs, else 85; asm_type 1: AVX2
CASES = [
    ("p_full", "full", dict(slice_type=1, pic_depth_mode=0)),
    ("b_full", "full", dict(slice_type=0, pic_depth_mode=0)),
    ("b_full_avx2", "full", dict(slice_type=0, pic_depth_mode=2, asm_type=1)),
    ("p_l0_avx2", "full", dict(slice_type=1, pic_depth_mode=0, asm_type=1, hme_l1=0, hme_l2=0, regions_w=1, regions_h=1)),
    ("b_samepoc_base", "full", dict(slice_type=0, pic_depth_mode=0, temporal_layer_index=0, ref1_poc=8)),
    ("b_edge_full", "edge", dict(slice_type=0, pic_depth_mode=0)),
    ("p_edge_l0", "edge", dict(slice_type=1, pic_depth_mode=2, hme_l1=0, hme_l2=0, regions_w=1, regions_h=1)),
    ("b_edge_off", "edge", dict(slice_type=0, pic_depth_mode=2, enable_hme_flag=0, search_area_width=24, search_area_height=12)),
    ("b_edge_samepoc", "edge", dict(slice_type=0, pic_depth_mode=2, ref1_poc=8)),
    ("p_edge_narrow", "edge", dict(slice_type=1, pic_depth_mode=0, temporal_layer_index=0, search_area_width=8, search_area_height=7)),
    # the branches that no other case carries through the picture call: bi-prediction of PUs 0 .. 20 only, its full-row SAD, no
    # CheckZeroZeroCenter; the 525 % level-0 multiplier (the level-0 area clipped by the 1/16 picture's padding)
    ("b_edge_cu8x8_fullsad_nozz", "edge", dict(slice_type=0, pic_depth_mode=2, cu8x8_mode=1, fractional_search_method=1, is_used_as_reference_flag=0)),
    ("b_full_hl5_base", "full", dict(slice_type=0, pic_depth_mode=0, hierarchical_levels=5, temporal_layer_index=0)),
]
REGENERATED_IN_TESTS = ("b_full_avx2", "p_edge_narrow", "b_edge_cu8x8_fullsad_nozz")


def ptr(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def pictures():
    """{picture: (source, list-0 reference, list-1 reference)} uint8 [H, W]"""
    rng = np.random.default_rng(7527_25)
    big = svtlibs.smooth_picture(rng, 128 + 128, 192 + 128, grain=3)
    out = {}
    for name, (W, H) in SIZES.items():
        def cut(dx, dy, x0=0, y0=0, w=W, h=H):
            return big[64 + y0 + dy:64 + y0 + dy + h, 64 + x0 + dx:64 + x0 + dx + w]
        ref0 = np.ascontiguousarray(cut(0, 0))
        src = np.zeros((H, W), np.uint8)
        # the source's quadrants are the list-0 reference displaced by (dx, dy): the block at (x, y) matches the reference at (x + dx, y + dy)
        hx, hy = (W // 2 + 31) & ~31, H // 2
        for (x0, y0, w, h), (dx, dy) in zip(((0, 0, hx, hy), (hx, 0, W - hx, hy), (0, hy, hx, H - hy), (hx, hy, W - hx, H - hy)),
                                            ((7, 2), (-12, 5), (0, 0), (20, -9))):
            src[y0:y0 + h, x0:x0 + w] = cut(dx, dy, x0, y0, w, h)
        noise = rng.integers(-2, 3, (H, W))
        noise[hy:, :hx] = 0                                         # the unmoved quadrant is an exact copy: SAD 0 at (0, 0), ties elsewhere
        src = (src.astype(np.int64) + noise).clip(0, 255).astype(np.uint8)
        src[8:24, 72:104] = 128                                     # a flat block on flat reference samples: ties between search points
        ref0[8:40, 64:112] = 128
        if name == "edge":                                          # last SB column = the reference's last sample column (see the docstring)
            src[:, 128:] = (ref0[:, -1:].astype(np.int64) + rng.integers(-1, 2, (H, 32))).clip(0, 255)
        ref1 = np.ascontiguousarray(cut(-9, 4))
        out[name] = (src, ref0, np.ascontiguousarray(ref1))
    return out


def ref_pyramid(R, luma):
    """me_pyramid by the reference's own Decimation2D and generate_padding"""
    planes, geo = [], []
    h0, w0 = luma.shape
    for lvl, pad in enumerate(svtlibs.ME_PADS):
        step = 1 << lvl
        w, h = (w0 + step - 1) // step, (h0 + step - 1) // step
        stride = w + 2 * pad + 5
        buf = np.zeros((h + 2 * pad, stride), np.uint8)
        if lvl == 0:
            buf[pad:pad + h, pad:pad + w] = luma
        else:
            src = np.ascontiguousarray(luma)
            R.ref_decimation_2d(ptr(src), w0, w0, h0, ctypes.c_void_p(buf.ctypes.data + pad * stride + pad), stride, step)
        R.ref_generate_padding(ptr(buf), stride, w, h, pad, pad, 0)
        planes.append(buf)
        geo.append((stride, pad, pad, w, h))
    return planes, geo


def case_params(name):
    _, pic, kw = next(c for c in CASES if c[0] == name)
    W, H = SIZES[pic]
    geo = svtlibs.me_pyramid(np.zeros((H, W), np.uint8))[1]
    return pic, [svtlibs.me_lcu_params(W, H, sx, sy, geo, **kw) for sy in range(0, H, 64) for sx in range(0, W, 64)]


def run_case(R, name, pics=None):
    """every SB of one case through ref_motion_estimate_lcu -> {key: array [nsb, ...]}, prm [nsb, 54]"""
    pics = pics or pictures()
    pic, prms = case_params(name)
    pyr = [ref_pyramid(R, p)[0] for p in pics[pic]]
    outs = {k: [] for k in KEYS}
    for prm in prms:
        o = svtlibs.run_me_lcu(R.ref_motion_estimate_lcu, prm, *pyr)
        for k in KEYS:
            outs[k].append(o[k])
    d = {k: np.array(v) for k, v in outs.items()}
    d["prm"] = np.array(prms)
    return d


def area_width(prm, xo):
    """the clipped width of a list's search area from its origin (MotionEstimateLcu :7955-8040: only the right edge shrinks it)"""
    saw = (int(prm[13]) + 7) & ~7
    W, ox = int(prm[0]), int(prm[2])
    if ox + xo + saw > W:
        saw = max(1, saw - (ox + xo + saw - W))
    return saw & ~7 if saw >= 8 else saw


def check_conditions(g):
    """the coverage the fixture must hold; g = the loaded file (or the dict about to be written).  No reference needed."""
    names = [str(n) for n in g["cases"]]
    assert names == [c[0] for c in CASES] and 8 <= len(names) <= 12
    seen = set()
    narrow = False
    for name, pic, _ in CASES:
        prm = g[name + "_prm"]
        W, H = SIZES[pic]
        nsb = ((W + 63) // 64) * ((H + 63) // 64)
        assert prm.shape == (nsb, 54) and tuple(prm[0][:2]) == (W, H)
        assert g[name + "_best_sad"].shape == (nsb, 2, 209) and g[name + "_results"].shape == (nsb, 209, 11)
        p = prm[0]
        hme = "off" if not p[8] else ("full" if p[9] and p[10] and p[11] else ("l0" if p[9] and not p[10] and not p[11] else "mixed"))
        seen |= {("slice", int(p[4])), ("hme", hme), ("regions", int(p[15]), int(p[16])), ("pus", int(p[25])), ("flavour", int(p[21]), pic)}
        if p[4] == 0 and p[19] == p[20]:
            seen.add(("samepoc", "base" if p[6] == 0 else "above"))
        nl = 1 if p[4] == 1 else 2
        npus = int(p[25])
        for i in range(nsb):
            for l in range(nl):
                narrow |= area_width(prm[i], int(g[name + "_area_origin"][i, l, 0])) < 8
        assert (g[name + "_best_sad"][:, :nl, :npus] < 128 * 128 * 255).all()                     # every PU of every searched list found a vector
        if name == "b_edge_cu8x8_fullsad_nozz":           # cu8x8_mode 1 with 85 PUs: PUs 0 .. 20 are bi-predicted, the 8x8 PUs 21 .. 84 are not
            assert (p[23], p[24], p[12], npus, nl) == (1, 1, 0, 85, 2)
            assert (g[name + "_results"][:, :21, 10] == 3).all() and (g[name + "_results"][:, 21:85, 10] == 2).all()
            assert (g[name + "_bipred_sad"][:, :21] != 0).any()
            seen |= {("cu8x8", 1), ("fullsad", 1), ("nozz", 1)}
        else:
            assert p[23] == 0 and (g[name + "_results"][:, :npus, 10] == (1 if nl == 1 else 3)).all()     # cu8x8_mode 0: every PU is bi-predicted
        if p[8] and p[9] and (p[7], p[6]) == (5, 0):
            seen.add(("multiplier", 525))
    need = {("slice", 0), ("slice", 1), ("hme", "full"), ("hme", "l0"), ("hme", "off"), ("regions", 1, 1), ("regions", 2, 2), ("pus", 85), ("pus", 209),
            ("flavour", 0, "full"), ("flavour", 0, "edge"), ("flavour", 1, "full"), ("samepoc", "base"), ("cu8x8", 1), ("fullsad", 1), ("nozz", 1),
            ("multiplier", 525)}
    assert need <= seen, sorted(need - seen)
    assert ("flavour", 1, "edge") not in seen             # the reference's AVX2 HME kernels are undefined on partial SB columns
    assert narrow, "no search area clipped to fewer than 8 columns"
    # real minima and ties: a non-zero vector somewhere, SAD 0 in the exact-copy region
    assert any((g[n + "_best_mv"][:, 0, 0] != 0).any() for n in names) and any((g[n + "_best_sad"][:, 0, :85] == 0).any() for n in names)
    for pic in SIZES:
        for i in range(3):
            assert g[f"pic_{pic}_{i}"].shape == SIZES[pic][::-1]


def main():
    R = svtlibs.ref()
    assert R is not None, "oracle/_ref/libsvtref.so is not built (run build() where the reference sources are present)"
    O = svtlibs.oracle()
    pics = pictures()
    d = {"cases": np.array([c[0] for c in CASES])}
    for pic, planes in pics.items():
        for i, pl in enumerate(planes):
            d[f"pic_{pic}_{i}"] = pl
            got, geo = ref_pyramid(R, pl)
            want, wgeo = svtlibs.me_pyramid(pl)
            assert geo == wgeo and all(np.array_equal(a, b) for a, b in zip(got, want)), (pic, i)
    for k, (name, pic, _) in enumerate(CASES):
        r = run_case(R, name, pics)
        for key in KEYS + ("prm",):
            d[f"{name}_{key}"] = r[key]
        # one SB per case (a different one each time) against the oracle's twin
        i = k % len(r["prm"])
        pyr = [svtlibs.me_pyramid(p)[0] for p in pics[pic]]
        o = svtlibs.run_me_lcu(O.svt_oracle_me_lcu, r["prm"][i], *pyr)
        nl = 1 if r["prm"][i][4] == 1 else 2
        for key in ("best_sad", "best_mv", "area_origin"):
            assert np.array_equal(o[key][:nl], r[key][i][:nl]), (name, i, key)
        for key in ("bipred_sad", "results"):
            assert np.array_equal(o[key], r[key][i]), (name, i, key)
    check_conditions(d)
    np.savez_compressed(OUT, **d)
    size = os.path.getsize(OUT)
    assert size < (512 << 10), size
    print(f"wrote {OUT}: {size} bytes, {len(CASES)} cases")


if __name__ == "__main__":
    main()

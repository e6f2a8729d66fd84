"""CPU: the sub-pel motion estimation fixture (tests/golden/me_subpel.npz, written by tests/golden/make_golden_me_subpel.py from the
reference's own InterpolateSearchRegionAVC / HalfPelSearch_LCU / QuarterPelSearch_LCU / MotionEstimateLcu with use_subpel_flag = 1) holds
the cases and the coverage it must; the plain numpy restatement (tests/me_subpel_cases.py) equals it - planes, half rows, quarter rows,
bi-prediction and me_results; the built library exports the new entry points with the header's struct size and refuses each bad
argument without a device; where oracle/_ref/libsvtref_me_subpel.so is built, a live re-run reproduces stored rows."""
import ctypes
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
sys.path.insert(0, ROOT)
import make_golden_me_subpel as mg     # noqa: E402
import me_subpel_cases as sp           # noqa: E402
import svtlibs                         # noqa: E402

NAMES = [c[0] for c in mg.CASES]
PAD = svtlibs.ME_PADS[0]
_cache = {}


def gold():
    if "g" not in _cache:
        _cache["g"] = np.load(sp.FIXTURE)
    return _cache["g"]


def planes_of(pic, i):
    """sp.Planes of picture `pic`'s source (0) / list-0 (1) / list-1 (2) reference, computed once"""
    if (pic, i) not in _cache:
        _cache[(pic, i)] = sp.Planes(np.pad(gold()[f"pic_{pic}_{i}"], PAD, mode="edge"), PAD, PAD)
    return _cache[(pic, i)]


def package():
    import __graft_entry__ as ge
    return ge.load_package()


def case_flags(prm, enables=(1, 1, 1, 1, 1)):
    return tuple(enables) + (int(prm[23] == 1),)


def test_fixture_holds_the_cases_and_the_coverage():
    g = gold()
    assert os.path.getsize(sp.FIXTURE) < (1 << 20)
    assert [str(n) for n in g["cases"]] == NAMES
    mg.check_conditions(g)
    assert mg.MIN_COVER == 20
    pics = mg.pictures()
    for p in mg.SIZES:
        for i in range(3):
            assert np.array_equal(g[f"pic_{p}_{i}"], pics[p][i])
    # the counts are the generator's, recomputed from the stored rows
    for k, v in mg.coverage(g, pics).items():
        assert np.array_equal(np.array(v), g["cover_" + k]), k
    # what the issue lists: P and B, both references one picture, 85 and 209 PUs, cu8x8_mode 0 and 1, the three methods, HME on and off, the
    # four search areas (the last clipped by the picture below 8 wide)
    seen = {(int(g[n + "_prm"][0][4]), int(g[n + "_prm"][0][25]), int(g[n + "_prm"][0][23]), int(g[n + "_prm"][0][24]), int(g[n + "_prm"][0][8])) for n in NAMES}
    assert {s[0] for s in seen} == {0, 1} and {s[1] for s in seen} == {85, 209} and {s[2] for s in seen} == {0, 1} and {s[3] for s in seen} == {0, 1, 2}
    assert {s[4] for s in seen} == {0, 1}
    assert {(int(g[n + "_prm"][0][13]), int(g[n + "_prm"][0][14])) for n in NAMES} >= {(8, 8), (16, 8), (64, 32)}
    assert any((g[n + "_area"][:, :, 2] < 8).any() and (g[n + "_area"][:, :, 2] > 0).any() for n in NAMES)
    assert any(g[n + "_prm"][0][4] == 0 and g[n + "_prm"][0][19] == g[n + "_prm"][0][20] for n in NAMES)
    # the flat SB and the exact copy: all-tie behaviour is recorded, PUs stay at their full-pel vectors
    n = "b_full_sub_nsq"
    assert (g[n + "_lcu_best_mv"][1, 0, :209] == g[n + "_full_mv"][1, 0, :209]).sum() >= mg.MIN_COVER and (g[n + "_half_dir"][1, 0, :209] == sp.L).sum() >= mg.MIN_COVER
    assert ((g[n + "_lcu_best_mv"][0, 0] == g[n + "_full_mv"][0, 0]) & (g[n + "_lcu_best_sad"][0, 0] == 0))[:209].sum() >= mg.MIN_COVER


def test_the_model_equals_the_references_planes():
    g = gold()
    for k, (ci, sb, l) in enumerate(g["plane_windows"]):
        name, pic = NAMES[ci], mg.CASES[ci][1]
        prm = g[name + "_prm"][sb]
        xo, yo, saw, sah = (int(v) for v in g[name + "_area"][sb, l])
        pl = planes_of(pic, 1 + l)
        want = g[f"planes_{k}"]
        assert want.shape == (3, sah + 64, saw + 64)
        for i, kind in enumerate("BHJ"):
            got = pl.get(kind, int(prm[3]) + yo, int(prm[2]) + xo, sah + 64, saw + 64)
            assert np.array_equal(got, want[i]), (name, sb, l, kind)


def model_stage(g, name, i, l, enables=(1, 1, 1, 1, 1)):
    pic = next(c[1] for c in mg.CASES if c[0] == name)
    prm = g[name + "_prm"][i]
    sbx, sby = int(prm[2]), int(prm[3])
    src = planes_of(pic, 0).get("F", sby, sbx, 64, 64)
    xo, yo = (int(v) for v in g[name + "_area"][i, l, :2])
    return sp.refine_sb(planes_of(pic, 1 + l), src, sbx, sby, xo, yo, int(prm[25]), int(prm[24]), case_flags(prm, enables), g[name + "_full_sad"][i, l],
                        g[name + "_full_mv"][i, l])


@pytest.mark.parametrize("name", NAMES)
def test_the_model_equals_the_references_half_and_quarter_rows(name):
    g = gold()
    prm = g[name + "_prm"]
    nl = 1 if prm[0][4] == 1 else 2
    for i in range(len(prm)):
        for l in range(nl):
            o = model_stage(g, name, i, l)
            for k in ("half_sad", "half_mv", "half_ssd", "half_dir"):
                assert np.array_equal(o[k], g[f"{name}_{k}"][i, l]), (name, i, l, k, np.argwhere(o[k] != g[f"{name}_{k}"][i, l])[:4].tolist())
            for k in ("sad", "mv", "ssd"):
                assert np.array_equal(o[k], g[f"{name}_quarter_{k}"][i, l]), (name, i, l, k, np.argwhere(o[k] != g[f"{name}_quarter_{k}"][i, l])[:4].tolist())
            # MotionEstimateLcu whole leaves the same rows
            assert np.array_equal(o["sad"], g[name + "_lcu_best_sad"][i, l]) and np.array_equal(o["mv"], g[name + "_lcu_best_mv"][i, l])
            assert np.array_equal(o["ssd"], g[name + "_lcu_best_ssd"][i, l])


def test_the_model_equals_the_reference_with_the_enables_off_one_at_a_time():
    g = gold()
    name = str(g["var_case"])
    for v, en in enumerate(g["var_enables"]):
        for i in range(len(g[name + "_prm"])):
            for l in range(2):
                o = model_stage(g, name, i, l, tuple(int(e) for e in en))
                for k in ("half_sad", "half_mv", "half_ssd", "half_dir"):
                    assert np.array_equal(o[k], g[f"var{v}_{k}"][i, l]), (v, i, l, k)
                for k in ("sad", "mv", "ssd"):
                    assert np.array_equal(o[k], g[f"var{v}_quarter_{k}"][i, l]), (v, i, l, k)
    # everything off: the square PUs' rows are the full-pel rows (the non-square PUs of a 209-PU search are refined whatever the enables)
    last = len(g["var_enables"]) - 1
    assert not g["var_enables"][last].any()
    assert np.array_equal(g[f"var{last}_quarter_sad"][..., :85], g[name + "_full_sad"][..., :85])
    assert np.array_equal(g[f"var{last}_quarter_mv"][..., :85], g[name + "_full_mv"][..., :85])
    assert not np.array_equal(g[f"var{last}_quarter_mv"][..., 85:], g[name + "_full_mv"][..., 85:])


@pytest.mark.parametrize("name", NAMES)
def test_the_model_equals_the_references_bi_prediction_and_me_results(name):
    g = gold()
    pic = next(c[1] for c in mg.CASES if c[0] == name)
    prm = g[name + "_prm"]
    two = prm[0][4] == 0
    npus = int(prm[0][25])
    for i in range(len(prm)):
        sbx, sby = int(prm[i][2]), int(prm[i][3])
        src = planes_of(pic, 0).get("F", sby, sbx, 64, 64)
        S, M = g[name + "_lcu_best_sad"][i], g[name + "_lcu_best_mv"][i]
        bip, res = sp.bipred_sb(planes_of(pic, 1), planes_of(pic, 2) if two else None, src, sbx, sby, npus, prm[i][24] == 0, prm[i][23] == 0 or npus == 209,
                                S[0], M[0], S[1], M[1])
        assert np.array_equal(bip, g[name + "_lcu_bipred_sad"][i]), (name, i, np.argwhere(bip != g[name + "_lcu_bipred_sad"][i])[:4].tolist())
        assert np.array_equal(res, g[name + "_lcu_results"][i]), (name, i, np.argwhere(res != g[name + "_lcu_results"][i])[:4].tolist())


def test_python_mirror_has_the_headers_size_and_the_entry_points_are_exported():
    import test_me_frame_cpu as mf
    pkg = package()
    lib = pkg.load_library()
    assert ctypes.sizeof(pkg.MeSubpelParams) == mf.header_struct_size("svt_hip_me_subpel_params") == 20
    for name in ("svt_hip_me_subpel_frame", "svt_hip_me_subpel_check", "svt_hip_motion_estimate_subpel_frame", "svt_hip_motion_estimate_subpel_frame_scratch_bytes",
                 "svt_hip_me_subpel_planes"):
        assert getattr(lib, name).argtypes is not None, name
    assert lib.svt_hip_motion_estimate_subpel_frame_scratch_bytes.restype is ctypes.c_size_t
    g = gold()
    good = pkg.MeFrameParams.from_lcu_prm(g["b_edge_fullsad_nsq_prm"][0])
    assert lib.svt_hip_motion_estimate_subpel_frame_scratch_bytes(ctypes.addressof(good), 1) == lib.svt_hip_motion_estimate_frame_scratch_bytes(ctypes.addressof(good), 1) == 256
    good.fractional_search_method = 3                      # the full-pel call carries any value; the sub-pel call knows three
    assert lib.svt_hip_motion_estimate_frame_scratch_bytes(ctypes.addressof(good), 1) == 256
    assert lib.svt_hip_motion_estimate_subpel_frame_scratch_bytes(ctypes.addressof(good), 1) == 0
    # the existing structs are as they were
    assert ctypes.sizeof(pkg.MeFrameParams) == 116 and ctypes.sizeof(pkg.MePyramid) == 88


def host_pyramid(pkg, W, H, pad=68, extra=5):
    p = pkg.MePyramid()
    p.d_plane[0] = 0x10000
    p.stride[0], p.origin_x[0], p.origin_y[0] = W + 2 * pad + extra, pad, pad
    p.pitch[0] = p.stride[0] * (H + 2 * pad)
    return p


def test_the_stage_refuses_each_bad_argument_without_a_device():
    pkg = package()
    lib = pkg.load_library()
    g = gold()
    W, H = 136, 72

    def check(change=None, n_pictures=2, rows=(0x20000, 0x30000, 0x40000, 0x50001)):
        params = pkg.MeFrameParams.from_lcu_prm(g["b_edge_fullsad_nsq_prm"][0])
        s = pkg.MeSubpelParams(1, 1, 1, 1, 1)
        pyr = [host_pyramid(pkg, W, H) for _ in range(3)]
        a = dict(params=params, subpel=s, pyr=pyr, n_pictures=n_pictures, rows=list(rows))
        if change:
            change(a)
        return lib.svt_hip_me_subpel_check(*(ctypes.addressof(p) if p is not None else None for p in a["pyr"]), ctypes.addressof(a["params"]),
                                           ctypes.addressof(a["subpel"]) if a["subpel"] is not None else None, a["n_pictures"], *a["rows"])

    def field(obj, name, value):
        def change(a):
            setattr(a[obj], name, value)
        return change

    def plane(i, name, value):
        def change(a):
            getattr(a["pyr"][i], name)[0] = value
        return change

    def item(key, i, value):
        def change(a):
            a[key][i] = value
        return change

    assert check() == 0
    assert check(item("rows", 2, None)) == 0 and check(item("rows", 3, None)) == 0 and check(field("subpel", "enable_quarter_pel", 0)) == 0       # optional outputs
    assert check(lambda a: a.update(subpel=None)) == 0
    refused = [field("params", "picture_width", 132), field("params", "picture_height", 0), field("params", "picture_width", 16392), field("params", "slice_type", 2),
               field("params", "max_number_of_pus_per_sb", 100), field("params", "fractional_search_method", 3), field("params", "fractional_search_method", -1),
               field("params", "cu8x8_mode", -1), field("subpel", "fractional_search64x64", 2), field("subpel", "enable_half_pel32x32", -1),
               field("subpel", "enable_half_pel16x16", 2), field("subpel", "enable_half_pel8x8", 7), field("subpel", "enable_quarter_pel", 2),
               item("pyr", 0, None), item("pyr", 1, None), item("pyr", 2, None), plane(0, "d_plane", None), plane(1, "d_plane", None), plane(2, "d_plane", None),
               plane(1, "origin_x", 65), plane(1, "origin_y", 65), plane(2, "origin_x", 64), plane(2, "origin_y", 65),
               plane(1, "stride", 68 + W + 65), plane(2, "stride", 68 + W + 65), plane(0, "stride", 68 + W + 63),
               plane(1, "pitch", (W + 141) * (68 + H + 66) - 1), plane(0, "pitch", (W + 141) * (68 + H + 64) - 1),
               item("rows", 0, None), item("rows", 1, None), item("rows", 0, 0x20002), item("rows", 1, 0x30001), item("rows", 2, 0x40002),
               lambda a: a.update(n_pictures=65536)]
    for k, change in enumerate(refused):
        assert check(change) == -2, k
    # the neighbours of the bounds: the margin is 66 samples, the encoder's pictures have 68
    accepted = [plane(1, "origin_x", 66), plane(2, "origin_y", 66), plane(1, "stride", 68 + W + 66), plane(0, "stride", 68 + W + 64),
                plane(1, "pitch", (W + 141) * (68 + H + 66)), lambda a: a.update(n_pictures=65535), lambda a: a.update(n_pictures=0),
                field("params", "fractional_search_method", 2), field("params", "picture_width", 128)]
    for k, change in enumerate(accepted):
        assert check(change) == 0, k
    # a P picture takes no list-1 reference; a single picture needs no pitch
    assert check(field("params", "slice_type", 1)) == -2
    assert check(lambda a: (setattr(a["params"], "slice_type", 1), a["pyr"].__setitem__(2, None))) == 0
    assert check(plane(1, "pitch", 0), n_pictures=1) == 0 and check(plane(1, "pitch", 0), n_pictures=2) == -2
    # with NULL everywhere the launching calls answer INVALID (-2) on a machine with a device and NO_DEVICE (-1) without one
    assert lib.svt_hip_me_subpel_frame(None, None, None, None, None, 1, None, None, None, None, None) in (-1, -2)
    assert lib.svt_hip_motion_estimate_subpel_frame(None, None, None, None, None, 1, None, None, None, None, None, None, 0, None) in (-1, -2)
    assert lib.svt_hip_me_subpel_planes(None, 64, 64, 0, 0, 8, 8, None, None) in (-1, -2)


def test_a_live_run_of_the_reference_reproduces_the_fixture():
    L, R = sp.ref_lib(), svtlibs.ref()
    if L is None or R is None:
        pytest.skip("oracle/_ref/libsvtref_me_subpel.so is not built (tests/golden/make_golden_me_subpel.py builds it)")
    g = gold()
    pics = mg.pictures()
    for name in ("b_edge_ssd_cu8", "p_edge_narrow_nsq"):
        r = mg.run_case(L, R, name, pics)
        for k, v in r.items():
            assert np.array_equal(v, g[f"{name}_{k}"]), (name, k)

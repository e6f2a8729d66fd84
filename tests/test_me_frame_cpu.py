"""CPU: the whole-picture motion estimation fixture (tests/golden/me_frame.npz, written by tests/golden/make_golden_me_frame.py from
the reference's own MotionEstimateLcu) holds the cases it must; where oracle/_ref/libsvtref.so is built, regenerating two cases
reproduces the stored arrays; the Python mirrors of svt_hip_me_frame_params / svt_hip_me_pyramid have the header's sizes; the built
library exports svt_hip_motion_estimate_frame and answers without a device."""
import ctypes
import os
import re
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
sys.path.insert(0, ROOT)
import make_golden_me_frame as mg      # noqa: E402
import svtlibs                         # noqa: E402

GOLD = os.path.join(ROOT, "tests", "golden", "me_frame.npz")


def package():
    import __graft_entry__ as ge
    return ge.load_package()


def test_fixture_holds_the_cases_the_picture_call_must_cover():
    g = np.load(GOLD)
    assert os.path.getsize(GOLD) < (512 << 10)
    mg.check_conditions(g)                  # P / B, HME full / level 0 only / off, 1x1 / 2x2 regions, 85 / 209 PUs, same POC, narrow area,
    #                                         cu8x8_mode 1 (PUs 21 .. 84 not bi-predicted), full-row SAD, no zero-centre check, 525 %
    # sources and references are stored once per picture size; the pyramids are rebuilt from them
    assert sorted(k for k in g if k.startswith("pic_")) == sorted(f"pic_{p}_{i}" for p in mg.SIZES for i in range(3))
    pics = mg.pictures()
    for p in mg.SIZES:
        for i in range(3):
            assert np.array_equal(g[f"pic_{p}_{i}"], pics[p][i])


def test_the_randomised_draws_cover_every_listed_value_and_redraw_at_most_a_quarter():
    """svtlibs.me_frame_draws, shared by tests/test_oracle_vs_ref.py (oracle against the reference) and tests/test_gpu_me_frame.py (the
    picture call against the oracle): every listed value of every dimension at least twice over the seeds in use, at most 25 % of the
    draws outside the domain - decided by me_frame_outside_domain alone, which agrees with what the picture call refuses"""
    seen, stats = svtlibs.me_frame_generator_coverage()
    assert stats["drawn"] >= len(svtlibs.ME_FRAME_SEEDS) * svtlibs.ME_FRAME_DRAWS_PER_SEED and sum(seen["W"].values()) == 24
    assert max(r["prm"].shape[0] for s in svtlibs.ME_FRAME_SEEDS for r in svtlibs.me_frame_oracle_runs(s)) <= 24      # SBs per picture
    # the rules name exactly what svt_hip_motion_estimate_frame_scratch_bytes refuses (a host computation, no device)
    pkg = package()
    lib = pkg.load_library()
    geo = svtlibs.me_pyramid(np.zeros((192, 256), np.uint8))[1]
    outside = [(200, dict(enable_hme_flag=1, hme_l0=0, hme_l1=0, hme_l2=0)),
               (256, dict(slice_type=0, regions_w=1, regions_h=2, ref1_poc=8, temporal_layer_index=1)),
               (256, dict(slice_type=0, regions_w=2, regions_h=1, ref1_poc=8, temporal_layer_index=2, hme_l0=0)),
               (200, dict(asm_type=1))]
    inside = [(256, dict(slice_type=0, regions_w=1, regions_h=2, ref1_poc=8, temporal_layer_index=0)),
              (256, dict(slice_type=0, regions_w=1, regions_h=2, ref1_poc=8, temporal_layer_index=1, hme_l2=0)),
              (256, dict(slice_type=1, regions_w=2, regions_h=1, ref1_poc=8, temporal_layer_index=1)),
              (256, dict(asm_type=1)), (200, dict(asm_type=1, hme_l0=0))]
    for want, sets in ((True, outside), (False, inside)):
        for W, kw in sets:
            full = dict(svtlibs.ME_LCU_DEFAULTS); full.update(kw)
            assert (svtlibs.me_frame_outside_domain(W, 192, full) is not None) == want, kw
            p = pkg.MeFrameParams.from_lcu_prm(svtlibs.me_lcu_params(W, 192, 0, 0, geo, **kw))
            assert (lib.svt_hip_motion_estimate_frame_scratch_bytes(ctypes.addressof(p), 1) == 0) == want, kw


def test_the_randomised_draws_reach_the_branches_they_are_for():
    """from the oracle's outputs: an area clipped below 8 columns, a non-zero vector, cu8x8_mode 1 with PUs 21 .. 84 not bi-predicted, and
    the 70 % / 350 % / 525 % level-0 multipliers with level 0 on"""
    svtlibs.me_frame_oracle_coverage()


def test_regenerating_two_cases_reproduces_the_fixture():
    R = svtlibs.ref()
    if R is None:
        pytest.skip("oracle/_ref/libsvtref.so is not built")
    g = np.load(GOLD)
    for name in mg.REGENERATED_IN_TESTS:
        r = mg.run_case(R, name)
        for key in mg.KEYS + ("prm",):
            assert np.array_equal(r[key], g[f"{name}_{key}"]), (name, key)


def header_struct_size(name):
    """sizeof of a struct of int32 / uint32 / uint16 / uint64 / pointer members, from the header's text (natural alignment)"""
    text = open(os.path.join(ROOT, "include", "svt_hip_dsp.h")).read()
    body = re.search(r"typedef struct " + name + r" \{(.*?)\} " + name + ";", text, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    off, amax = 0, 1
    for decl in body.split(";"):
        decl = decl.strip()
        if not decl:
            continue
        m = re.match(r"(const uint8_t \*|int32_t|uint32_t|uint16_t|uint64_t)\s*(.*)", decl)
        assert m, decl
        size = {"const uint8_t *": 8, "int32_t": 4, "uint32_t": 4, "uint16_t": 2, "uint64_t": 8}[m.group(1)]
        amax = max(amax, size)
        for var in m.group(2).split(","):
            n = 1
            for d in re.findall(r"\[(\d+)\]", var):
                n *= int(d)
            off = (off + size - 1) // size * size + size * n
    return (off + amax - 1) // amax * amax


def test_python_mirrors_have_the_headers_sizes():
    pkg = package()
    assert ctypes.sizeof(pkg.MeFrameParams) == header_struct_size("svt_hip_me_frame_params") == 116
    assert ctypes.sizeof(pkg.MePyramid) == header_struct_size("svt_hip_me_pyramid") == 88
    g = np.load(GOLD)
    p = pkg.MeFrameParams.from_lcu_prm(g["b_full_avx2_prm"][0])
    assert (p.picture_width, p.picture_height, p.slice_type, p.flavour, p.max_number_of_pus_per_sb) == (192, 128, 0, 1, 85)
    assert [list(r) for r in p.hme_search_area_in_width_array] == [[16, 16], [8, 8], [8, 8]] and list(p.ref_pic_poc) == [8, 16]


def test_entry_point_is_exported_and_checks_its_arguments_without_a_device():
    pkg = package()
    lib = pkg.load_library()
    assert lib.svt_hip_motion_estimate_frame.argtypes is not None and lib.svt_hip_motion_estimate_frame_scratch_bytes.restype is ctypes.c_size_t
    g = np.load(GOLD)
    good = pkg.MeFrameParams.from_lcu_prm(g["b_edge_full_prm"][0])
    # the scratch size is a host computation: one int16 [4] area per SB and list, rounded up to 256 bytes
    assert lib.svt_hip_motion_estimate_frame_scratch_bytes(ctypes.addressof(good), 1) == 256
    assert lib.svt_hip_motion_estimate_frame_scratch_bytes(ctypes.addressof(good), 16) == (16 * 6 * 2 * 8 + 255) // 256 * 256
    bad = pkg.MeFrameParams.from_lcu_prm(g["b_edge_full_prm"][0])
    bad.flavour = 1                                            # AVX2 flavour, HME level 0 on, width 160: refused
    assert lib.svt_hip_motion_estimate_frame_scratch_bytes(ctypes.addressof(bad), 1) == 0
    for field, value in (("max_number_of_pus_per_sb", 100), ("picture_width", 100), ("slice_type", 2), ("number_hme_search_region_in_width", 3),
                         ("search_area_width", 0), ("search_area_height", 600), ("temporal_layer_index", 7)):
        bad = pkg.MeFrameParams.from_lcu_prm(g["b_edge_full_prm"][0])
        setattr(bad, field, value)
        assert lib.svt_hip_motion_estimate_frame_scratch_bytes(ctypes.addressof(bad), 1) == 0, field
    # with NULL everywhere the call answers INVALID (-2) on a machine with a device and NO_DEVICE (-1) without one; it never launches
    rc = lib.svt_hip_motion_estimate_frame(None, None, None, ctypes.addressof(good), 1, None, None, None, None, None, None, 0, None)
    assert rc in (-1, -2)

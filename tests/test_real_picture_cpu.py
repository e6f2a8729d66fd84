"""CPU: the real-picture fixture (tests/golden/real_picture.npz, written by tests/golden/make_golden_real_picture.py: a 352 x 224 window
of the reference's own test clip carried through the reference's pyramids, picture statistics, MotionEstimateLcu, open-loop intra
search, encode pass and CDEF, each stage fed by the one before).

  * the file meets its conditions (flat and busy blocks, real motion, directional intra winners, eob 0 and eob > 10, several CDEF
    strengths) and its size cap;
  * where the reference tree and oracle/_ref/libsvtref.so are present, the generator reproduces every stored array from the clip;
  * where they are not, each stage's oracle twin or numpy restatement reproduces the fixture on every SB and every filter block:
    svt_oracle_decimation_2d / svt_oracle_generate_padding, np_picture_stats, svt_oracle_me_lcu, svt_oracle_ois_block, the oracle's
    transform / quantiser chain, and make_golden_cdef's numpy filter (the applied picture of all three planes, and the chroma half of
    the search table at five strengths per filter block; luma's table entry is the reference's binary64 distortion, which the numpy
    filter does not restate).

This is the first time any of these runs on real content: a mismatch is fixed in the oracle or the restatement, never in the fixture."""
import ctypes
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
import make_golden_real_picture as mg      # noqa: E402
import svtlibs                             # noqa: E402
from svtlibs import ptr                    # noqa: E402


@pytest.fixture(scope="module")
def gold():
    g = mg.load()
    for v in g.values():
        v.setflags(write=False)
    return g


def assert_same(got, want, keys):
    for k in keys:
        assert got[k].dtype == want[k].dtype and got[k].shape == want[k].shape, (k, got[k].dtype, want[k].dtype, got[k].shape, want[k].shape)
        assert np.array_equal(got[k], want[k]), (k, np.argwhere(got[k] != want[k])[:4].tolist())


def test_the_fixture_meets_its_conditions_and_its_size_cap(gold):
    assert os.path.getsize(mg.OUT) < mg.SIZE_CAP == 768 << 10
    mg.check_conditions(gold)
    vals = dict(zip(mg.STAT_NAMES, gold["stats"]))
    # the floors, spelled out once more where the file is read
    assert vals["flat_share"] >= 0.05 and vals["busy_share"] >= 0.05
    assert vals["me_zero_sad_share"] <= 0.01 and vals["me_p_sbs_with_two_vectors"] >= 3 and vals["me_b_sbs_with_two_vectors"] >= 3
    assert vals["ois_modes_besides_dc"] >= 3 and vals["ois_directional_modes"] >= 1
    assert vals["enc_eob0_share"] >= 0.10 and vals["enc_eob_above_10_share"] >= 0.10
    assert vals["cdef_luma_strengths"] >= 4 and vals["cdef_fbs_with_a_skip"] >= 1 and vals["cdef_fbs_without_a_skip"] >= 1


def test_the_generator_and_the_live_reference_reproduce_every_array(gold):
    if svtlibs.ref() is None or not os.path.exists(mg.CLIP):
        pytest.skip("the reference tree / oracle/_ref/libsvtref.so is not here: the stored arrays are not regenerated")
    frame = mg.read_clip()
    ox, oy = (int(v) for v in gold["origin"])
    origins = mg.candidate_origins(frame)
    assert len(origins) == 1980
    for earlier in origins[:origins.index((ox, oy))]:          # the window is the FIRST that meets the conditions
        assert mg.build_fixture(frame, earlier[0], earlier[1], int(gold["qindex"]))[0] is None, earlier
    g, missed = mg.build_fixture(frame, ox, oy, int(gold["qindex"]))
    assert missed is None
    assert sorted(g) == sorted(gold)
    assert_same(g, gold, [k for k in gold if k != "stats"])
    assert np.allclose(g["stats"], gold["stats"])


def test_the_picture_oracle_gives_the_pyramids_the_tests_rebuild(gold):
    O = svtlibs.oracle()
    for name in ("src_y", "ref0_y", "ref1_y"):
        luma = np.ascontiguousarray(gold[name])
        planes, geo = svtlibs.me_pyramid(luma)
        for lvl, (stride, ox, oy, w, h) in enumerate(geo):
            e = np.zeros_like(planes[lvl])
            if lvl == 0:
                e[oy:oy + h, ox:ox + w] = luma
            else:
                O.svt_oracle_decimation_2d(ptr(luma), mg.W, mg.W, mg.H, ctypes.c_void_p(e.ctypes.data + oy * stride + ox), stride, 1 << lvl)
            O.svt_oracle_generate_padding(ptr(e), stride, w, h, ox, oy, 1)
            assert np.array_equal(e, planes[lvl]), (name, lvl)


def test_np_picture_stats_reproduces_the_statistics(gold):
    got = mg.stage_stats(mg.mg_st.np_picture_stats, gold)
    assert_same(got, gold, sorted(got))
    assert len(got) == 2 * len(mg.mg_st.SB_KEYS) + len(mg.mg_st.PIC_KEYS)
    # real content: the two precisions differ, partial SBs have no chroma means
    assert not np.array_equal(gold["stats_p0_variance"], gold["stats_p1_variance"])
    assert not gold["stats_p1_cb_mean"][mg.NSBX - 1].any() and gold["stats_p1_cb_mean"][0].any()


def test_the_oracles_motion_estimate_lcu_reproduces_every_sb(gold):
    O = svtlibs.oracle()
    pyr = [svtlibs.me_pyramid(np.ascontiguousarray(gold[n]))[0] for n in ("src_y", "ref0_y", "ref1_y")]
    got = mg.stage_me(O.svt_oracle_me_lcu, pyr)
    for case, kw in mg.ME_CASES.items():
        nl = 1 if kw["slice_type"] == 1 else 2
        assert np.array_equal(got[f"me_{case}_prm"], gold[f"me_{case}_prm"])
        for k in ("best_sad", "best_mv", "area_origin"):
            a, b = got[f"me_{case}_{k}"][:, :nl], gold[f"me_{case}_{k}"][:, :nl]
            assert np.array_equal(a, b), (case, k, np.argwhere(a != b)[:4].tolist())
        for k in ("bipred_sad", "results"):
            a, b = got[f"me_{case}_{k}"], gold[f"me_{case}_{k}"]
            assert np.array_equal(a, b), (case, k, np.argwhere(a != b)[:4].tolist())


def test_the_ois_oracle_reproduces_every_block_of_every_sb(gold):
    got = mg.oracle_ois(gold["src_y"])
    assert_same(got, gold, ("ois_valid", "ois_count", "ois_best", "ois_mode", "ois_delta", "ois_dist"))
    assert int(gold["ois_valid"].sum()) == 15 * 85 + 3 * 42 + 5 * 42 + 21           # whole SBs, the 32-wide column, the 32-high row, the corner


def test_the_oracles_transform_and_quantiser_chain_reproduces_the_encode_pass(gold):
    got = mg.stage_encode(mg.oracle_code_plane, gold, int(gold["qindex"]))
    assert_same(got, gold, sorted(got))
    assert got["enc_y_qcoeff"].shape == (308, 256) and got["enc_cb_qcoeff"].shape == (308, 64)
    # luma eobs alone would give another map: chroma keeps some blocks
    luma_only = mg.skip_map(gold["enc_y_eob"], np.zeros(308, np.uint16), np.zeros(308, np.uint16))
    assert not np.array_equal(luma_only, gold["skip"])


def test_the_numpy_cdef_filter_reproduces_the_applied_picture_and_the_chroma_table(gold):
    rec = [gold[f"enc_{n}_recon"] for n in mg.PLANES]
    src = [gold[f"src_{n}"] for n in mg.PLANES]
    q = int(gold["qindex"])
    ys, us = mg.argmin_strengths(gold["cdef_mse"], gold["cdef_count"])
    assert np.array_equal(ys, gold["cdef_ystr"]) and np.array_equal(us, gold["cdef_ustr"])
    assert np.array_equal(gold["cdef_count"], [min(8, 28 - 8 * r) * min(8, 44 - 8 * c) - int(gold["skip"][8 * r:8 * r + 8, 8 * c:8 * c + 8].sum())
                                               for r in range(4) for c in range(6)])
    out = mg.np_cdef_apply(rec, gold["skip"], q, ys, us, gold["cdef_dir"], gold["cdef_var"])
    for n, o in zip(mg.PLANES, out):
        assert np.array_equal(o, gold[f"cdef_out_{n}"]), (n, np.argwhere(o != gold[f"cdef_out_{n}"])[:4].tolist())
    assert (out[0] != rec[0]).any() and (out[1] != rec[1]).any()
    for fb in range(mg.NSB):
        if gold["cdef_count"][fb] == 0:
            assert not gold["cdef_mse"][:, fb].any()
            continue
        for gi in sorted({0, 5, 22, 63, int(us[fb])}):
            want = int(gold["cdef_mse"][1, fb, gi])
            assert mg.np_cdef_chroma_mse(rec, src, gold["skip"], q, fb, gi, gold["cdef_dir"], gold["cdef_var"]) == want, (fb, gi)

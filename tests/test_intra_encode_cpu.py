"""CPU: the fixture of svt_hip_intra_encode_frame (tests/golden/intra_encode.npz).  It regenerates byte for byte from the reference built
as oracle/_ref/libsvtref.so (when that is present), holds the coverage its first case promises and no refused entry where none is meant."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden", "intra_encode.npz")
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
import make_golden_intra_encode as mi  # noqa: E402
import make_golden_recon_final as mr  # noqa: E402


@pytest.fixture(scope="module")
def gold():
    return dict(np.load(GOLD))


@pytest.fixture(scope="module")
def geom():
    return mr.load_geometry(dict(np.load(os.path.join(ROOT, "tests", "golden", "recon_final.npz"))))


def test_fixture_regenerates_byte_for_byte(gold):
    if mi.mg.ref_lib() is None:
        pytest.skip("oracle/_ref/libsvtref.so is not built")
    again = mi.build_all()
    assert sorted(again) == sorted(gold)
    for key, v in again.items():
        assert v.dtype == gold[key].dtype and np.array_equal(v, gold[key]), key


def test_coverage_of_the_first_case(gold, geom):
    """every block size, all nine partition shapes (the mixed ones at the 32 and the 64 level), the 13 luma modes with deltas -3, 0 and 3
    on the directional ones, every chroma mode, CfL with both signs, every transform type on every size that defines it, and per plane
    between a quarter and three quarters of the coded blocks with eob 0; blocks on the superblock's right column and bottom row"""
    cases, outs = zip(*[mi.load_case(gold, k) for k in range(len(mi.CASE_NAMES))])
    zero = mi.check_coverage(list(cases), list(outs), geom)
    assert (zero[:, 1] >= 150).all(), zero.tolist()
    right = bottom = 0
    for k in mi.COVER:
        c = cases[k]
        live = np.arange(mi.MAX_FINAL)[None, None] < c["count"][..., None]
        e = c["final"][live]
        w, h = np.array(mi.BS_W)[e["bsize"]], np.array(mi.BS_H)[e["bsize"]]
        right += int((((e["x"] + w) % 64 == 0) & (e["y"] % 64 != 0)).sum())
        bottom += int((((e["y"] + h) % 64 == 0) & (e["x"] % 64 != 0)).sum())
    assert right >= 20 and bottom >= 20, (right, bottom)


@pytest.mark.parametrize("k", mi.ALL_OK, ids=[mi.CASE_NAMES[k] for k in mi.ALL_OK])
def test_no_entry_is_refused_where_none_is_meant(gold, k):
    c, o = mi.load_case(gold, k)
    live = np.arange(mi.MAX_FINAL)[None, None] < c["count"][..., None]
    assert live.sum() > 0 and (o["status"][live] == 0).all()
    assert np.array_equal(o["resmask"], live)
    for p in range(3):
        assert o[f"rmask{p}"].any() and o[f"qmask{p}"].any()


def test_shapes_of_the_special_cases(gold):
    counts = {name: mi.load_case(gold, k)[0]["count"].reshape(-1).tolist() for k, name in enumerate(mi.CASE_NAMES)}
    assert counts["sb4"] == [256] and counts["sb64"] == [1] and len(counts["edges"]) == 9 and len(counts["cover0"]) == 8
    c, o = mi.load_case(gold, mi.CASE_NAMES.index("edges"))
    assert tuple(int(v) for v in c["dims"][1:5]) == (3, 3, 176, 144)
    c, o = mi.load_case(gold, mi.CASE_NAMES.index("inter"))
    live = np.arange(mi.MAX_FINAL)[None, None] < c["count"][..., None]
    share = (o["status"][live] == mi.R_NOT_INTRA).mean()
    assert 0.35 <= share <= 0.65 and set(o["status"][live].tolist()) == {mi.OK, mi.R_NOT_INTRA}
    assert os.path.getsize(GOLD) < 1 << 20

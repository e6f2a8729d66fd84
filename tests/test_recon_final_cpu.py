"""CPU: the fixture of svt_hip_recon_final_frame (tests/golden/recon_final.npz).  It holds what the issue lists; the CPU checker's inverse
transform (libsvt_oracle.so), run through the generator's walk, gives the same planes, status, offsets and stream; and where the compiled
reference is present the generator reproduces the committed file byte for byte."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden", "recon_final.npz")
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
import make_golden_recon_final as mr  # noqa: E402
import make_golden_partition as mg  # noqa: E402


@pytest.fixture(scope="module")
def gold():
    z = dict(np.load(GOLD))
    geom = mr.load_geometry(z)
    tabs = mr.bsize_tables(geom)
    return z, geom, tabs, [mr.load_case(z, k, tabs) for k in range(len(mr.ALL_NAMES))]


def test_the_file_is_small_and_names_its_cases(gold):
    z = gold[0]
    assert os.path.getsize(GOLD) < 1 << 20
    assert tuple(z["names"].tolist()) == mr.CASE_NAMES


def test_coverage_of_the_fixture(gold):
    """every block size, every (luma size, type) pair, mixed types in consecutive 4x4 and 8x8 entries, eob 0 in each plane alone and
    together, blocks without chroma, superblocks of 256 blocks, one block and none; one entry per skip reason"""
    z, geom, tabs, cases = gold
    named = [(name, c) for name, (c, o) in zip(mr.CASE_NAMES, cases)]
    mr.check_coverage(named, [o for c, o in cases[:mr.NCASES]], geom, tabs)
    skips_c, skips_o = cases[mr.CASE_NAMES.index("skips")]
    assert (skips_c["width"][0], skips_c["height"][0], skips_c["stride"][0], skips_c["rows"][0]) == (96, 80, 128, 128)
    live = np.arange(mr.MAX_FINAL)[None] < skips_c["count"][:, None]
    outside = (skips_o["status"] == mr.R_OUTSIDE) & live
    assert outside.any() and (skips_c["final"]["x"][outside] < 96).any() and (skips_c["final"]["y"][outside] < 80).any()      # a block that begins inside and pokes out


def test_every_case_tiles_and_masks_agree(gold):
    """main pictures: each superblock's list covers disjoint blocks; the plane masks are exactly the blocks of the reconstructed entries;
    entries past the count would write if they were read"""
    z, geom, tabs, cases = gold
    for name, (c, o) in zip(mr.ALL_NAMES, cases):
        cover = np.zeros(o["rmask0"].shape, np.int32)
        for sb in range(len(c["count"])):
            n = int(c["count"][sb])
            for k in range(n):
                e = c["final"][sb, k]
                if o["status"][sb, k] == 0:
                    cover[e["y"]:e["y"] + mr.BS_H[e["bsize"]], e["x"]:e["x"] + mr.BS_W[e["bsize"]]] += 1
            assert (c["final"]["bsize"][sb, n:] < 22).all()
        assert cover.max() <= 1, name
        assert np.array_equal(cover == 1, o["rmask0"]), name
        if name in ("main1", "main2"):
            assert o["rmask0"][:128, :128].all() and o["rmask1"][:64, :64].all() and o["rmask2"][:64, :64].all()
        assert not o["rmask0"][:, int(c["width"][0]):].any() and not o["rmask0"][int(c["height"][0]):].any(), name
    c, o = cases[0]
    assert not o["rmask0"][64:128, 0:64].any() and not o["rmask1"][32:64, 0:32].any()      # the superblock with count 0
    assert not o["qmask0"][1, 1024:].any() and o["qmask0"][1, :1024].all()                  # a 64x64: the tail of its span


def test_offsets_are_the_running_coded_areas(gold):
    z, geom, tabs, cases = gold
    for name, (c, o) in zip(mr.ALL_NAMES, cases):
        for sb in range(len(c["count"])):
            y = uv = 0
            for k in range(int(c["count"][sb])):
                assert tuple(o["offset"][sb, k]) == (y, uv), (name, sb, k)
                if o["status"][sb, k] == 0:
                    e = c["final"][sb, k]
                    y += mr.BS_W[e["bsize"]] * mr.BS_H[e["bsize"]]
                    if geom["has_uv"][e["mds_idx"]]:
                        uv += tabs[int(e["bsize"])][2] * tabs[int(e["bsize"])][3]
            assert y <= 4096 and uv <= 1024


def test_the_oracle_inverse_gives_the_fixture(gold):
    z, geom, tabs, cases = gold
    inv = mr.oracle_inverse()
    for name, (c, o) in zip(mr.ALL_NAMES, cases):
        got = mr.model(c, geom, tabs, inv)
        for key in mr.OUTPUT_KEYS:
            assert np.array_equal(got[key], o[key]), (name, key)
        luma = mr.model(c, geom, tabs, inv, planes=1)
        for key in ("status", "offset", "recon0", "rmask0", "sbq0", "qmask0"):
            assert np.array_equal(luma[key], o[key]), (name, key)
        assert not luma["rmask1"].any() and not luma["qmask2"].any()


def test_the_geometry_matches_the_partition_fixture(gold):
    z, geom, tabs, cases = gold
    pgeom = mg.load_geometry(dict(np.load(os.path.join(ROOT, "tests", "golden", "partition.npz"))))
    for key in ("bsize", "has_uv", "origin_x", "origin_y", "bwidth", "bheight", "depth", "shape"):
        assert np.array_equal(geom[key], pgeom[key]), key


def test_the_generator_reproduces_the_file(gold):
    L = mg.ref_lib()
    if L is None:
        pytest.skip("oracle/_ref/libsvtref.so is not built")
    z = gold[0]
    again = mr.build_all(L)
    assert set(again) == set(z)
    for key, v in again.items():
        assert v.dtype == z[key].dtype and np.array_equal(v, z[key]), key

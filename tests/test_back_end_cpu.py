"""CPU: the back-end chain's fixture (tests/golden/back_end.npz) and the helper its inputs come from (tests/back_end_cases.py).  The
coverage conditions the generator asserted, re-checked on the committed bytes; the helper's leaves, costs and per-src tables against what
the stored outputs imply; the level walk on the host over the recorded table; and, where oracle/_ref/libsvtref.so and libsvtref_dlf.so
are present, every stage of the generator re-run live against the committed file."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
import back_end_cases as bc                     # noqa: E402
from back_end_cases import mg, mi, mr           # noqa: E402
import make_golden_back_end as mgb              # noqa: E402
import make_golden_real_picture as mg_real      # noqa: E402


@pytest.fixture(scope="module")
def gold():
    g = bc.load()
    geom, rgeom = bc.geometry()
    pics = dict(src=[g[f"src{p}"] for p in range(3)], ref=[g[f"ref{p}"] for p in range(3)])
    case, groups = bc.partition_case(pics, geom)
    final = bc.padded_final(g["part_final"], g["part_count"])
    tabs = bc.src_tables(final, g["part_count"], pics, geom, rgeom, len(case["leaf"]))
    return dict(g=g, geom=geom, rgeom=rgeom, pics=pics, case=case, groups=groups, final=final, tabs=tabs)


def test_coverage_conditions_hold_on_the_committed_file(gold):
    g = gold["g"]
    vals = bc.measure(g, gold["geom"], gold["rgeom"])
    met = bc.conditions(vals)
    assert all(met.values()), ([k for k, ok in met.items() if not ok], vals)
    assert [str(n) for n in g["stat_names"]] == list(bc.STAT_NAMES)
    assert np.allclose(g["stats"], [vals[n] for n in bc.STAT_NAMES]), (g["stats"].tolist(), vals)
    assert os.path.getsize(bc.FIXTURE) < bc.SIZE_CAP
    assert int(g["qindex"]) in mg_real.QINDEX_ORDER
    # the picture: at least 3 x 3 superblocks, a partial right column and bottom row, multiples of 8, at most 352 x 224
    assert bc.SB_COLS >= 3 and bc.SB_ROWS >= 3 and bc.W % 64 and bc.H % 64 and bc.W % 8 == 0 and bc.H % 8 == 0 and bc.W <= 352 and bc.H <= 224
    assert all(g[f"src{p}"].shape == (bc.PH[p], bc.PW[p]) for p in range(3))
    # a superblock with all four of the left, above-left, above and above-right neighbours whose list is not empty
    assert int(g["part_count"][bc.SB_COLS + 1]) > 0


def test_the_helpers_inputs_imply_the_stored_partition(gold):
    """the numpy restatement of the partition decision on the helper's leaves and costs gives the stored squares and list; the source
    groups are one block size each, ascending and contiguous over [0, nsrc)"""
    g, case, geom = gold["g"], gold["case"], gold["geom"]
    sq, count, final = mg.np_partition(case, geom)
    assert np.array_equal(sq, g["part_sq"]) and np.array_equal(count, g["part_count"]) and np.array_equal(final, g["part_final"])
    nsrc = len(case["leaf"])
    assert nsrc == int(g["nsrc"]) and sorted(case["leaf"]["src"].tolist()) == list(range(nsrc)) and len(case["cost"]) == nsrc
    at = 0
    bsize_of = np.zeros(nsrc, np.int64)
    bsize_of[case["leaf"]["src"]] = geom["bsize"][case["leaf"]["mds_idx"]]
    assert len(gold["groups"]) <= 32
    for first, n, b in gold["groups"]:
        assert first == at and n > 0 and (bsize_of[first:first + n] == b).all()
        at += n
    assert at == nsrc and [b for _, _, b in gold["groups"]] == sorted(b for _, _, b in gold["groups"])


def test_the_list_and_the_per_src_tables_are_consistent_with_the_stored_outputs(gold):
    g, geom, rgeom, final, tabs = gold["g"], gold["geom"], gold["rgeom"], gold["final"], gold["tabs"]
    count, nsrc = g["part_count"], int(g["nsrc"])
    live = np.arange(bc.MAX_FINAL)[None] < count[:, None]
    e = final[live]
    w, h = np.array(mr.BS_W)[e["bsize"]], np.array(mr.BS_H)[e["bsize"]]
    assert (e["x"] + w <= bc.W).all() and (e["y"] + h <= bc.H).all()                       # inside the picture
    assert len(set(e["src"].tolist())) == len(e) and (e["src"] < nsrc).all()               # src unique and below nsrc
    assert (geom["bsize"][e["mds_idx"]] == e["bsize"]).all()
    assert tabs["listed"].sum() == len(e) and not tabs["blk"]["is_intra"][~tabs["listed"]].any()
    intra = tabs["blk"]["is_intra"][final["src"]].astype(bool) & live
    assert np.array_equal(g["resmask"], intra)
    assert np.array_equal(g["status"][live], np.where(intra, mi.OK, mi.R_NOT_INTRA)[live])
    # the stream offsets: luma advances by the block's area, chroma by the chroma block's of the entries with has_uv
    for sb in range(bc.NSB):
        run = [0, 0]
        for k in range(int(count[sb])):
            assert g["offset"][sb, k].tolist() == run, (sb, k)
            m = int(final["mds_idx"][sb, k])
            run[0] += mr.BS_W[final["bsize"][sb, k]] * mr.BS_H[final["bsize"][sb, k]]
            if geom["has_uv"][m]:
                run[1] += mr.TX_W[rgeom["txsize_uv"][m]] * mr.TX_H[rgeom["txsize_uv"][m]]
    # the info rows under the skip rule, and the grid scattered from them
    info = bc.info_table(final, count, tabs, g["result"], geom, nsrc)
    assert np.array_equal(info, g["info"])
    for sb, k, ent in bc.entries(final, count):
        r, b = g["info"][int(ent["src"])], tabs["blk"][int(ent["src"])]
        eob, has_uv = g["result"]["eob"][sb, k], bool(geom["has_uv"][int(ent["mds_idx"])])
        if b["is_intra"]:
            assert (r["ref_frame0"], r["mode"]) == (0, b["mode"]) and r["skip"] == (eob[0] == 0 and (not has_uv or (eob[1] == 0 and eob[2] == 0)))
            assert g["result"]["tx_type"][sb, k] == (b["tx_type"] if eob[0] else 0)
        else:
            assert (r["ref_frame0"], r["skip"]) == (1, 1) and r["mode"] in (15, 16)
    assert any(geom["has_uv"][int(ent["mds_idx"])] and g["result"]["eob"][sb, k][0] == 0 and g["result"]["eob"][sb, k][1:].any()
               for sb, k, ent in bc.entries(final, count) if tabs["blk"]["is_intra"][int(ent["src"])]), "no block on which the luma eob alone would decide skip otherwise"
    assert np.array_equal(bc.mi_grid(final, count, g["info"], rgeom), g["mi"])
    # the pictures: the masks tile the picture, the inter samples are the reference picture's
    inter, intra_m = bc.block_masks(final, count, tabs, geom, rgeom)
    for p in range(3):
        assert np.array_equal(inter[p], g[f"imask{p}"]) and np.array_equal(intra_m[p], g[f"rmask{p}"]) and (inter[p] ^ intra_m[p]).all()
        assert np.array_equal(g[f"rec{p}"][inter[p]], g[f"ref{p}"][inter[p]])
    # the skip map ANDs all four units of an 8x8: the fixture holds 8x8s on which the first and the last unit alone would say otherwise
    s = g["mi"][:, :, 2] >> 7
    assert int(((s[::2, ::2] & s[1::2, 1::2]) != bc.skip_map(g["mi"])).sum()) >= 1
    # the argmin recorded is the argmin of the recorded table
    ys, us = mg_real.argmin_strengths(g["cdef_mse"], g["cdef_count"])
    assert np.array_equal(ys, g["cdef_ystr"]) and np.array_equal(us, g["cdef_ustr"])
    assert (g["dlf_table"][:, 0] == [((g[f"rec{p}"].astype(np.int64) - g[f"src{p}"]) ** 2).sum() for p in range(3)]).all()


def test_the_host_walk_over_the_recorded_table_picks_the_recorded_levels(pkg, gold):
    g = gold["g"]
    table = g["dlf_table"].astype(np.int64)
    for last, want in zip(g["dlf_starts"].tolist(), g["dlf_levels"].tolist()):
        assert want[0] == want[1]
        for plane, start, level in ((0, last[2], want[0]), (1, last[2], want[2]), (2, last[3], want[3])):
            assert pkg.SvtHipDsp.dlf_pick_level(table[plane], start, bc.LOOP_FILTER_MODE, bc.ONLY_4X4) == ("level", level), (plane, start)
            lazy, asked = np.full(64, -1, np.int64), []
            while True:
                kind, l = pkg.SvtHipDsp.dlf_pick_level(lazy, start, bc.LOOP_FILTER_MODE, bc.ONLY_4X4)
                if kind == "level":
                    break
                assert lazy[l] < 0 and l not in asked
                asked.append(l)
                lazy[l] = table[plane, l]
            assert l == level and 1 <= len(asked) < 64
    assert g["dlf_levels"][0].tolist() != g["dlf_levels"][1].tolist()         # the start decides: the table has more than one basin


@pytest.mark.skipif(not mgb.libraries_built(), reason="oracle/_ref/libsvtref.so and libsvtref_dlf.so are built where the reference's sources are "
                    "(build(), tests/golden/make_golden_dlf.py)")
def test_live_reference_equals_the_fixture(gold):
    g = gold["g"]
    live, vals, met = mgb.build_fixture(int(g["qindex"]))
    assert all(met.values())
    assert sorted(live) == sorted(g)
    for k in g:
        assert live[k].dtype == g[k].dtype and np.array_equal(live[k], g[k]), k

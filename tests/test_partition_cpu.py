"""CPU: the golden fixture of the partition decision (tests/golden/partition.npz, written by tests/golden/make_golden_partition.py: the d1
and d2 decisions are the reference's own functions run whole, the loop around them and the encode pass walk are the generator's glue, see
there), its array restatement, the library's block geometry and the Python mirror of the C ABI."""
import ctypes
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden", "partition.npz")
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
import make_golden_partition as mg  # noqa: E402

HAVE_REF = os.path.exists(os.path.join(ROOT, "oracle", "_ref", "libsvtref.so"))
INVALID = -2
NCASES = len(mg.CASE_NAMES)


@pytest.fixture(scope="module")
def gold():
    return dict(np.load(GOLD))


def test_fixture_loads_and_meets_the_conditions(gold):
    """the hard paths are IN the committed file: N staying and another shape taking the square, parents kept and cut, climbs that began
    at a 4x4, an untested parent, the picture edges with non-zero contexts, the I-slice root with and without a carried cost, exact ties, a
    shape whose last block is listed without its first, MAX_MODE_COST, superblocks that code 1 and 256 blocks"""
    geom = mg.load_geometry(gold)
    assert [str(n) for n in gold["names"]] == list(mg.CASE_NAMES)
    loaded = [mg.load_case(gold, k) for k in range(NCASES)]
    mg.check_conditions([(n, c) for n, (c, _, _, _) in zip(mg.CASE_NAMES, loaded)], [o[1:] for o in loaded], geom)
    for c, sq, count, final in loaded:
        assert c["bits"].shape == mg.BITS_SHAPE and c["bits"].dtype == np.int32 and int(np.abs(c["bits"]).max()) < 1 << 13
        assert sq.shape == (len(c["sb"]), mg.NSQ) and not sq["pad"].any() and int(count.sum()) == len(final) and int(count.max()) <= mg.MAX_FINAL
        for sb in c["sb"]:                                                 # the lists are as MDC makes them: ascending, no repeats
            m = c["leaf"]["mds_idx"][int(sb["leaf_first"]):int(sb["leaf_first"]) + int(sb["leaf_count"])].astype(np.int64)
            assert (np.diff(m) > 0).all() and m.max() < mg.NBLK
        assert sorted(c["leaf"]["src"].tolist()) == list(range(len(c["cost"])))
    nsb = len(mg.load_case(gold, mg.COMBINED)[0]["sb"])
    assert nsb == sum(len(c["sb"]) for c, _, _, _ in loaded) and nsb % 4 != 0      # the combined call ends in a partial workgroup
    assert os.path.getsize(GOLD) < 512 << 10


def test_generator_reproduces_the_fixture_inputs(gold):
    """without the reference: the synthetic inputs are the generator's"""
    geom = mg.load_geometry(gold)
    for k, name in enumerate(mg.CASE_NAMES):
        made, (c, _, _, _) = mg.make_case(name, geom), mg.load_case(gold, k)
        for key in mg.CASE_KEYS:
            assert np.array_equal(made[key], c[key]), (name, key)


@pytest.mark.parametrize("k", range(NCASES + 1), ids=mg.ALL_NAMES)
def test_array_restatement_equals_the_fixture(gold, k):
    """np_partition, the level-by-level restatement written as array arithmetic: every square, count and final block"""
    c, sq, count, final = mg.load_case(gold, k)
    n_sq, n_count, n_final = mg.np_partition(c, mg.load_geometry(gold))
    assert np.array_equal(n_sq, sq) and np.array_equal(n_count, count) and np.array_equal(n_final, final)


def test_ignoring_a_quirk_changes_the_fixture(gold):
    """what the fixture can tell apart: a slice type swapped, the contexts dropped, a d1 that lets a tie win"""
    geom = mg.load_geometry(gold)
    differs = lambda k, **change: not np.array_equal(mg.np_partition(dict(mg.load_case(gold, k)[0], **change), geom)[0], mg.load_case(gold, k)[1])
    k_i, k_e, k_t = mg.CASE_NAMES.index("islice_all"), mg.CASE_NAMES.index("edges"), mg.CASE_NAMES.index("ties")
    assert differs(k_i, slice_is_intra=np.int32(0))
    leaf = mg.load_case(gold, k_e)[0]["leaf"].copy()
    leaf["left_partition"], leaf["above_partition"] = 0, 0
    assert differs(k_e, leaf=leaf)
    assert differs(k_e, pic_width=np.uint32(256))
    cost = mg.load_case(gold, k_t)[0]["cost"].copy()
    cost -= np.uint64(1)                                                      # every H / V sum now strictly cheaper than N
    assert differs(k_t, cost=cost)


@pytest.mark.skipif(not HAVE_REF, reason="oracle/_ref/libsvtref.so is built by build() where the reference's source is present")
@pytest.mark.parametrize("k", range(NCASES + 1), ids=mg.ALL_NAMES)
def test_fixture_equals_the_compiled_reference(gold, k):
    L = mg.ref_lib()
    geom = mg.ref_geometry(L)
    assert np.array_equal(geom, mg.load_geometry(gold))
    if k == 0:
        mg.self_check(L, geom)
    c, sq, count, final = mg.load_case(gold, k)
    r_sq, r_count, r_final = mg.ref_partition(L, c, geom)
    assert np.array_equal(r_sq, sq) and np.array_equal(r_count, count) and np.array_equal(r_final, final)


def test_final_lists_tile_the_tested_area(gold):
    """per superblock the final blocks do not overlap, and inside the picture they cover exactly the pixels that a listed square covers
    (every pixel under a tested square is coded once; nothing outside one is)"""
    geom = mg.load_geometry(gold)
    for k, name in enumerate(mg.ALL_NAMES):
        c, sq, count, final = mg.load_case(gold, k)
        at = 0
        for i, sb in enumerate(c["sb"]):
            ox, oy = int(sb["origin_x"]), int(sb["origin_y"])
            hits, want = np.zeros((64, 64), np.int32), np.zeros((64, 64), bool)
            for f in final[at:at + int(count[i])]:
                g = geom[int(f["mds_idx"])]
                assert (int(f["x"]), int(f["y"]), int(f["bsize"])) == (ox + int(g["origin_x"]), oy + int(g["origin_y"]), int(g["bsize"]))
                hits[g["origin_y"]:g["origin_y"] + g["bheight"], g["origin_x"]:g["origin_x"] + g["bwidth"]] += 1
            at += int(count[i])
            for lf in c["leaf"][int(sb["leaf_first"]):int(sb["leaf_first"]) + int(sb["leaf_count"])]:
                g = geom[int(lf["mds_idx"])]
                if g["shape"] == 0:
                    want[g["origin_y"]:g["origin_y"] + g["sq_size"], g["origin_x"]:g["origin_x"] + g["sq_size"]] = True
            assert hits.max() <= 1, (name, i)
            inside = ((np.arange(64) + oy < int(c["pic_height"]))[:, None] & (np.arange(64) + ox < int(c["pic_width"]))[None, :])
            assert np.array_equal((hits == 1) & inside, want & inside), (name, i)


def test_library_geometry_equals_the_recorded_table(pkg, gold):
    """svt_hip_blk_geom_mds, built from the scan rule, against get_blk_geom_mds as recorded, for all 1 101 blocks; 1 101 is refused"""
    lib, geom = pkg.load_library(), mg.load_geometry(gold)
    got = np.zeros(mg.NBLK, mg.GEOM_DTYPE)
    for i in range(mg.NBLK):
        g = pkg.BlkGeom()
        assert lib.svt_hip_blk_geom_mds(i, ctypes.byref(g)) == 0
        got[i] = np.frombuffer(bytes(g), mg.GEOM_DTYPE)[0]
    for name in mg.GEOM_DTYPE.names:
        assert np.array_equal(got[name], geom[name]), name
    g = pkg.BlkGeom()
    assert lib.svt_hip_blk_geom_mds(mg.NBLK, ctypes.byref(g)) == INVALID and lib.svt_hip_blk_geom_mds(0, None) == INVALID
    assert lib.svt_hip_blk_geom_mds(0xFFFFFFFF, ctypes.byref(g)) == INVALID
    assert (pkg.SB_BLOCKS, pkg.SB_SQUARES, pkg.SB_MAX_FINAL, pkg.PARTITION_SPLIT) == (mg.NBLK, mg.NSQ, mg.MAX_FINAL, mg.PARTITION_SPLIT)


def test_mirror_layouts_match_the_header(pkg):
    """the ctypes mirror and the numpy dtypes against the header's declarations: member names in order, and the sizes"""
    import re
    lib = pkg.load_library()
    hdr = open(os.path.join(ROOT, "include", "svt_hip_dsp.h")).read()
    assert lib.svt_hip_partition_decide_frame.argtypes == [ctypes.c_void_p, ctypes.c_void_p] and lib.svt_hip_partition_decide_frame.restype is ctypes.c_int
    assert "int svt_hip_partition_decide_frame(const svt_hip_partition_args *a, void *stream);" in hdr

    def members(name):
        body = re.search(r"typedef struct " + name + r" \{(.*?)\} " + name + ";", hdr, re.S).group(1)
        body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
        out = []
        for decl in body.split(";"):
            decl = decl.strip()
            if decl:
                first, *rest = decl.split(",")
                out += [re.sub(r"\[.*\]", "", first.split()[-1]).lstrip("*")] + [re.sub(r"\[.*\]", "", r.strip()).lstrip("*") for r in rest]
        return out

    assert members("svt_hip_partition_args") == [n.replace("lambda_", "lambda") for n, _ in pkg.PartitionArgs._fields_]
    assert members("svt_hip_blk_geom") == [n for n, _ in pkg.BlkGeom._fields_]
    for cname, dt in (("svt_hip_part_leaf", pkg.part_leaf_dtype()), ("svt_hip_part_sb", pkg.part_sb_dtype()), ("svt_hip_part_sq", pkg.part_sq_dtype()),
                      ("svt_hip_part_final", pkg.part_final_dtype())):
        assert members(cname) == list(dt.names), cname
    assert (ctypes.sizeof(pkg.PartitionArgs), ctypes.sizeof(pkg.BlkGeom)) == (104, 16)
    assert (pkg.part_leaf_dtype(), pkg.part_sb_dtype(), pkg.part_sq_dtype(), pkg.part_final_dtype()) == (mg.LEAF_DTYPE, mg.SB_DTYPE, mg.SQ_DTYPE, mg.FINAL_DTYPE)

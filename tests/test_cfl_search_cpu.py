"""CPU: the C ABI of svt_hip_cfl_search_frame / svt_hip_cfl_decide_frame / svt_hip_cfl_pick_frame as the Python mirror binds it, and the
golden fixture of the CfL alpha search (tests/golden/cfl_search.npz, written by tests/golden/make_golden_cfl_search.py: every leaf of
the table is the reference's own function, the walk is the generator's glue, see there)."""
import ctypes
import os
import subprocess
import sys
import tempfile

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden", "cfl_search.npz")
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
import make_golden_cfl_search as mg  # noqa: E402

HAVE_REF = os.path.exists(os.path.join(ROOT, "oracle", "_ref", "libsvtref.so"))
INVALID, NO_DEVICE = -2, -1
NSZ = len(mg.SIZES)


@pytest.fixture(scope="module")
def gold():
    return np.load(GOLD)


def test_fixture_loads_and_meets_the_conditions(gold):
    mg.check_conditions(gold)
    for si in range(NSZ):
        v = mg.size_view(gold, si)
        assert int(v["size"]) == mg.SIZES[si]
        assert v["dist_c"].dtype == v["dist_avx2"].dtype == v["bits"].dtype == np.uint64 and v["eob"].dtype == np.uint16
        assert v["bits"].shape == v["eob"].shape == (mg.NBLOCKS, 2, mg.NALPHA)
        assert v["qrows"].shape == (2, 5, 8) and v["qrows"].dtype == np.int16
        assert v["alpha_rate"].shape == (8, 2, 16)
        for fl in ("c", "avx2"):
            assert v["decision_" + fl].shape == (mg.NBLOCKS, 32) and v["decision_" + fl].dtype == np.uint8
            assert not mg.decisions(gold, si, fl)["pad"].any()
        assert mg.decisions(gold, si)["uv_mode"][mg.FLAT] == mg.UV_DC_PRED      # all alphas tie: nothing beats DC's cheaper mode
    assert os.path.getsize(GOLD) < 1 << 20


@pytest.mark.parametrize("si", [0, 5])
def test_generator_reproduces_two_sizes_of_the_fixture(gold, si):
    """the inputs are the generator's and the restatement gives the fixture's table and records (4x4 and 4x8), without the reference"""
    z = mg.gen_size(si, None, mg.size_view(gold, si)["qrows"])
    for key, v in z.items():
        assert np.array_equal(v, gold[f"s{si}_{key}"]), (si, key)


@pytest.mark.skipif(not HAVE_REF, reason="needs the reference build (oracle/_ref)")
def test_restatement_equals_the_reference_on_every_case(gold):
    L = mg.ref_lib()
    for si in range(NSZ):
        v = mg.size_view(gold, si)
        assert np.array_equal(mg.ref_qrows(L, int(v["qindex"])), v["qrows"])
        ref = mg.ref_table(L, v)
        rest = mg.np_table(v)
        for key, t in ref.items():
            assert np.array_equal(rest[key], t), (si, key)                          # the restatement against the reference, all nine sizes
            assert np.array_equal(t, v[key]), (si, key)                             # and the fixture is the reference's output
    # rows whose AC entries differ between the planes (what tests/test_gpu_cfl_search.py runs against np_table): the reference too
    z = mg.ac_rows_case(mg.size_view(gold, 1))
    ref, rest = mg.ref_table(L, z), mg.np_table(z)
    for key, t in ref.items():
        assert np.array_equal(rest[key], t), key
    assert (ref["eob"][:, 0] != ref["eob"][:, 1]).any()


def test_the_walk_written_as_the_reference_loops_equals_the_restatement(gold):
    """cfl_rd_pick_alpha's nested loops in Python integers against np_walk and against the fixture's records, every block, both flavours"""
    for si in range(NSZ):
        v = mg.size_view(gold, si)
        for fl in ("c", "avx2"):
            dec = mg.decisions(gold, si, fl)
            rest, _ = mg.np_decide(v, v["dist_" + fl])
            assert np.array_equal(rest, dec), (si, fl)
            for b in range(mg.NBLOCKS):
                got = mg.ref_walk(v["dist_" + fl][b], v["bits"][b], v["alpha_rate"], int(v["lam"]), int(v["cfl_mode_bits"][b]), int(v["dc_mode_bits"][b]))
                d = dec[b]
                want = (int(d["best_rd"]), int(d["dc_rd"]), int(d["uv_mode"]), int(d["cfl_alpha_idx"]), int(d["cfl_alpha_signs"]),
                        int(d["alpha_q3"][0]), int(d["alpha_q3"][1]))
                assert got == want, (si, fl, b)


def test_walk_corner_cases():
    """synthetic tables: the DC-check entry of the Cr walk, a tie that keeps the earlier candidate, and costs that wrap"""
    rate = np.full((8, 2, 16), 1000, np.int32)
    bits = np.full((2, mg.NALPHA), 5000, np.uint64)
    dist = np.full((2, mg.NALPHA, 2), 900, np.uint64)
    # Cr: entry 1 (alpha -1) is far the best of its table, but the walk reads entry 0 at (Cr, NEG, c = 0): it must not be picked there
    dist[1, 1, 0] = 1
    dist[0, 17 + 2, 0] = 10                                                       # Cb: alpha +3
    for fn in (lambda: mg.np_walk(dist, bits, rate, 4000, 3000, 300)[0], ):
        rec = fn()
        assert rec["uv_mode"] == mg.UV_CFL_PRED and rec["alpha_q3"][0] == 3 and rec["alpha_q3"][1] != -1
    got = mg.ref_walk(dist, bits, rate, 4000, 3000, 300)
    assert got[5:] == (int(rec["alpha_q3"][0]), int(rec["alpha_q3"][1])) and got[0] == int(rec["best_rd"])
    # an exact tie of c = 0 and c = 1 keeps c = 0
    dist[:] = 900
    dist[0, 17, 0] = dist[0, 18, 0] = 5
    rec, _ = mg.np_walk(dist, bits, rate, 4000, 3000, 300)
    assert rec["alpha_q3"][0] == 1
    # distortions that wrap RDCOST's uint64: both walks agree
    dist[0, :, 0] = (1 << 57) + np.arange(mg.NALPHA)
    rec, _ = mg.np_walk(dist, bits, rate, 0xFFFFFFFF, -5, 300)
    got = mg.ref_walk(dist, bits, rate, 0xFFFFFFFF, -5, 300)
    assert got == (int(rec["best_rd"]), int(rec["dc_rd"]), int(rec["uv_mode"]), int(rec["cfl_alpha_idx"]), int(rec["cfl_alpha_signs"]),
                   int(rec["alpha_q3"][0]), int(rec["alpha_q3"][1]))


def test_mirror_sets_argtypes_and_restype(pkg):
    lib = pkg.load_library()
    hdr = open(os.path.join(ROOT, "include", "svt_hip_dsp.h")).read()
    for n, nargs, ret, cret in (("svt_hip_cfl_search_frame", 8, ctypes.c_int, "int"), ("svt_hip_cfl_search_scratch_bytes", 2, ctypes.c_size_t, "size_t"),
                                ("svt_hip_cfl_decide_frame", 3, ctypes.c_int, "int"), ("svt_hip_cfl_pick_frame", 8, ctypes.c_int, "int"),
                                ("svt_hip_cfl_pick_scratch_bytes", 2, ctypes.c_size_t, "size_t")):
        assert f"{cret} {n}(" in hdr
        f = getattr(lib, n)
        assert f.argtypes is not None and len(f.argtypes) == nargs and f.restype is ret, n
    assert "#define SVT_HIP_CFL_NALPHA 33" in hdr and pkg.SvtHipDsp.CFL_NALPHA == mg.NALPHA == 33


def test_struct_layouts_match_the_header(pkg):
    structs = (("svt_hip_qrows", pkg.QRows, {}), ("svt_hip_cfl_search_group", pkg.CflSearchGroup, {}), ("svt_hip_cfl_decision", pkg.CflDecision, {}),
               ("svt_hip_cfl_decide_group", pkg.CflDecideGroup, {"lambda_": "lambda"}), ("svt_hip_cfl_pick_group", pkg.CflPickGroup, {"lambda_": "lambda"}))
    assert ctypes.sizeof(pkg.CflDecision) == 32 and ctypes.alignment(pkg.CflDecision) == 8
    assert np.dtype(pkg.SvtHipDsp.CFL_DECISION_DTYPE) == mg.DEC_DTYPE
    args, want = [], []
    for cname, S, ren in structs:
        fields = [n for n, _ in S._fields_]
        args += [f"sizeof({cname})"] + [f"offsetof({cname}, {ren.get(n, n)})" for n in fields]
        want += [ctypes.sizeof(S)] + [getattr(S, n).offset for n in fields]
    code = ('#include <stddef.h>\n#include <stdio.h>\n#include "svt_hip_dsp.h"\nint main(void){printf("%zu"' + ' " %zu"' * (len(args) - 1) + ", " +
            ", ".join(args) + ");return 0;}\n")
    with tempfile.TemporaryDirectory() as d:
        open(os.path.join(d, "t.c"), "w").write(code)
        subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), os.path.join(d, "t.c"), "-o", os.path.join(d, "t")])
        out = [int(v) for v in subprocess.check_output([os.path.join(d, "t")]).decode().split()]
    assert out == want


def search_groups(pkg, specs):
    """a CflSearchGroup array from (tx_size, tx_type, nblocks): the scratch computation reads no memory"""
    arr = (pkg.CflSearchGroup * max(len(specs), 1))()
    for i, (s, t, n) in enumerate(specs):
        arr[i].tx_size, arr[i].tx_type, arr[i].nblocks = s, t, n
    return arr


def pick_groups(pkg, specs):
    """a CflPickGroup array from (tx_size, tx_type, nblocks, supplied) with supplied a set of dist / bits / eob"""
    arr = (pkg.CflPickGroup * max(len(specs), 1))()
    for i, (s, t, n, have) in enumerate(specs):
        g = arr[i].search
        g.tx_size, g.tx_type, g.nblocks = s, t, n
        for k in ("dist", "bits", "eob"):
            setattr(g, "d_" + k, 0x1000 if k in have else None)
    return arr


def test_scratch_bytes_on_hand_computed_cases(pkg):
    lib = pkg.load_library()
    sb = lambda specs: lib.svt_hip_cfl_search_scratch_bytes(search_groups(pkg, specs), len(specs))
    # 4x4, 5 blocks = 330 candidates: qcoeff 330 * 64 = 21120, contexts 2 * (330 -> 336)
    assert sb([(0, 0, 5)]) == 21120 + 2 * 336
    # 16x16, 1 block = 66 candidates: qcoeff 66 * 1024 = 67584, contexts 2 * (66 -> 80)
    assert sb([(2, 0, 1)]) == 67584 + 160
    # 8x4 with another type, 8 blocks = 528 candidates: qcoeff 528 * 128 = 67584, contexts 2 * 528
    assert sb([(6, 9, 8)]) == 67584 + 1056
    # groups add up; an empty group adds nothing; no groups need nothing
    assert sb([(0, 0, 5), (14, 0, 0), (2, 0, 1)]) == 21120 + 672 + 67584 + 160
    assert sb([]) == 0 and sb([(13, 0, 0)]) == 0
    # bad parameters: 0 (a size with a 32- or 64-sample side, no size, a type that is none, nblocks * 66 = 2^31 and above, an empty group's size)
    for bad in ((3, 0, 5), (4, 0, 5), (9, 0, 5), (15, 0, 5), (18, 0, 5), (19, 0, 5), (-1, 0, 5), (0, 16, 5), (0, -1, 5), (0, 0, 32537632)):
        assert sb([bad]) == 0, bad
    assert sb([(0, 0, 32537631)]) == 32537631 * 66 * 64 + 2 * ((32537631 * 66 + 15) & ~15)
    assert sb([(0, 0, 5), (3, 0, 0)]) == 0
    assert lib.svt_hip_cfl_search_scratch_bytes(None, 1) == 0 and lib.svt_hip_cfl_search_scratch_bytes(None, -1) == 0
    pb = lambda specs: lib.svt_hip_cfl_pick_scratch_bytes(pick_groups(pkg, specs), len(specs))
    # the pick adds the tables it was not given: dist 330 * 16 = 5280, bits 330 * 8 = 2640, eob 660 -> 672
    assert pb([(0, 0, 5, set())]) == 5280 + 2640 + 672 + 21120 + 672
    assert pb([(0, 0, 5, {"dist", "eob"})]) == 2640 + 21120 + 672
    assert pb([(0, 0, 5, {"dist", "bits", "eob"})]) == 21120 + 672
    assert pb([(0, 0, 5, set()), (2, 0, 0, set())]) == 5280 + 2640 + 672 + 21120 + 672
    assert pb([]) == 0 and pb([(3, 0, 5, set())]) == 0 and lib.svt_hip_cfl_pick_scratch_bytes(None, 2) == 0


def test_frame_calls_without_a_device_or_with_bad_arguments(pkg):
    """a NULL group list: SVT_HIP_ERR_INVALID (-2) on a machine with a device, SVT_HIP_ERR_NO_DEVICE (-1) without one, as the sibling
    calls answer (the device is looked for first); no call ever returns a result.  No groups at all is not an error."""
    import torch
    lib = pkg.load_library()
    have = torch.cuda.is_available()
    bad, ok = (INVALID if have else NO_DEVICE), (0 if have else NO_DEVICE)
    row = (ctypes.c_int16 * 8)(*([64] * 8))
    q = pkg.QRows(*([ctypes.addressof(row)] * 5))
    Q = ctypes.addressof(q)
    assert lib.svt_hip_cfl_decide_frame(None, 1, None) == bad and lib.svt_hip_cfl_decide_frame(None, -1, None) == bad
    assert lib.svt_hip_cfl_decide_frame(None, 0, None) == ok
    assert lib.svt_hip_cfl_search_frame(None, 1, 1, Q, Q, None, 0, None) == bad
    assert lib.svt_hip_cfl_search_frame(None, 0, 1, Q, Q, None, 0, None) == ok
    assert lib.svt_hip_cfl_search_frame(None, 0, 1, None, Q, None, 0, None) == bad           # a NULL row set
    assert lib.svt_hip_cfl_pick_frame(None, 1, 1, Q, Q, None, 0, None) == bad
    assert lib.svt_hip_cfl_pick_frame(None, 0, 1, Q, Q, None, 0, None) == ok
    g = search_groups(pkg, [(0, 0, 5)])
    assert lib.svt_hip_cfl_search_frame(g, 1, 1, Q, Q, None, 0, None) == bad                  # NULL members and no scratch
    assert lib.svt_hip_cfl_search_frame(search_groups(pkg, [(3, 0, 0)]), 1, 1, Q, Q, None, 0, None) == bad      # an empty group's size
    d = (pkg.CflDecideGroup * 1)()
    d[0].nblocks = 4
    assert lib.svt_hip_cfl_decide_frame(d, 1, None) == bad
    assert lib.svt_hip_cfl_pick_frame(pick_groups(pkg, [(0, 0, 5, set())]), 1, 1, Q, Q, None, 0, None) == bad

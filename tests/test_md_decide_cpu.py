"""CPU: the C ABI of svt_hip_md_decide_frame / svt_hip_md_search_frame as the Python mirror binds it, and the golden fixture of the join
of mode decision (tests/golden/md_decide.npz, written by tests/golden/make_golden_md_decide.py: the per-slot costs and the decision are
the reference's own functions, the escape walk is the generator's glue, see there)."""
import ctypes
import os
import subprocess
import sys
import tempfile

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden", "md_decide.npz")
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
import make_golden_md_decide as mg  # noqa: E402

HAVE_REF = os.path.exists(os.path.join(ROOT, "oracle", "_ref", "libsvtref.so"))
INVALID, NO_DEVICE = -2, -1


@pytest.fixture(scope="module")
def gold():
    return dict(np.load(GOLD))


def test_fixture_loads_and_meets_the_conditions(gold):
    """the cases the decide must meet are IN the committed file: a tie of skip and merge, skip winning, merge winning, two equal costs,
    the escape firing under full_loop_escape 1 and 2, an escape that cuts off the lowest cost, an inter cost on each side of 2^32 before an
    intra slot, an I slice that would escape, CfL with alphas and fallen back, has_uv 0 and 1, a winner with eob 0 in each plane"""
    mg.check_conditions(gold)
    assert gold["rates"].shape == (mg.RATE_WORDS,) and gold["rates"].dtype == np.int32
    for k in range(mg.NCASES):
        n, nb = int(gold[f"c{k}_n"]), mg.NBLOCKS
        assert tuple(int(gold[f"c{k}_{key}"]) for key in ("bsize", "n", "ninter", "nintra", "lam", "slice_is_intra", "escape", "has_chroma", "has_cfl")) == mg.CASES[k]
        assert gold[f"c{k}_luma"].shape == (nb, n, 40) and gold[f"c{k}_cfl"].shape == (nb, n, 32) and gold[f"c{k}_cand_out"].shape == (nb, n, 16)
        assert gold[f"c{k}_cdist"].shape == (2, nb, n, 2) and gold[f"c{k}_cdist"].dtype == np.uint64 and gold[f"c{k}_rate"].shape == (nb, n, 2)
        assert gold[f"c{k}_decision"].shape == (nb, 72) and gold[f"c{k}_decision"].dtype == np.uint8
        assert gold[f"c{k}_cost"].shape == (nb, n) and gold[f"c{k}_cost"].dtype == np.uint64
        d = mg.decisions(gold, k)
        assert not d["pad"].any() and (d["slot"] < d["count"]).all() and (d["count"] >= 1).all() and (d["count"] <= n).all()
        assert (gold[f"c{k}_cand"] < int(gold[f"c{k}_ninter"]) + int(gold[f"c{k}_nintra"])).all()
    # the chroma stage's pin: every 4:2:0 chroma transform size of a supported block size, both kernel flavours, eob 0 and eob > 0
    sizes = [int(v) for v in gold["uv_sizes"]]
    assert sizes == mg.uv_sizes() and len(sizes) == 14
    assert gold["uv_dist"].shape == (14, 2, 2, mg.UV_NBLK, 2) and gold["uv_bits"].shape == gold["uv_eob"].shape == (14, 2, mg.UV_NBLK)
    assert (gold["uv_eob"] == 0).any(axis=(1, 2)).all() and (gold["uv_eob"] != 0).any(axis=(1, 2)).all()      # in every size
    assert not gold["uv_dist"][:, :, :, 2].any() and gold["uv_dist"][:, :, :, 3, 1].all()      # exact prediction: nothing; extreme: a distortion the shift changes
    assert os.path.getsize(GOLD) < 512 << 10


def test_generator_reproduces_the_fixture_inputs(gold):
    """without the reference: the synthetic inputs are the generator's"""
    assert np.array_equal(mg.make_rates(), gold["rates"])
    for k in range(mg.NCASES):
        for key, v in mg.make_case(k, gold["rates"]).items():
            assert np.array_equal(v, gold[f"c{k}_{key}"]), (k, key)


def test_array_restatement_equals_the_fixture(gold):
    """np_md_decide, the restatement written as array arithmetic: every record and every slot's cost"""
    for k in range(mg.NCASES):
        dec, cost = mg.np_md_decide(gold, k)
        want = mg.decisions(gold, k)
        bad = np.flatnonzero(dec != want)
        assert bad.size == 0, (k, bad[:4].tolist(), dec[bad[0]], want[bad[0]])
        assert np.array_equal(cost, gold[f"c{k}_cost"]), k


def test_glue_restatement_equals_the_fixture(gold):
    """the generator's line-by-line glue: the per-slot values of the six members the cost functions write, and the records"""
    for k in range(mg.NCASES):
        dec, S = mg.glue_md_decide(gold, k)
        for key in mg.SLOT_KEYS:
            assert np.array_equal(S[key], gold[f"c{k}_{key}"]), (k, key)
        assert np.array_equal(dec, mg.decisions(gold, k)), k


def test_ignoring_the_escape_or_the_tie_rules_changes_the_fixture(gold):
    """what the fixture can tell apart: a walk without the escape, an arg-min that lets a later equal cost win, and a merge / skip choice
    with < each give a different record somewhere"""
    no_escape = later_wins = strict_skip = 0
    for k in range(mg.NCASES):
        c, dec, S = mg.case_inputs(gold, k), mg.decisions(gold, k), mg.slot_values(gold, k)
        cost = S["cost"]
        for b in range(c["nb"]):
            no_escape += int(cost[b].argmin()) != int(dec["slot"][b]) and int(dec["count"][b]) < c["n"]
            cnt = int(dec["count"][b])
            later_wins += cnt - 1 - int(cost[b, :cnt][::-1].argmin()) != int(dec["slot"][b])
        strict_skip += int((c["merge"] & (S["skip_cost"] == S["merge_cost"])).sum())
    assert no_escape > 0 and later_wins > 0 and strict_skip > 0, (no_escape, later_wins, strict_skip)


@pytest.mark.skipif(not HAVE_REF, reason="needs the reference build (oracle/_ref)")
def test_fixture_equals_the_compiled_reference(gold):
    L = mg.ref_lib()
    mg.self_check(L)
    for k in range(mg.NCASES):
        dec, S = mg.ref_md_decide(L, gold, k)
        for key in mg.SLOT_KEYS:
            assert np.array_equal(S[key], gold[f"c{k}_{key}"]), (k, key)
        assert np.array_equal(dec, mg.decisions(gold, k)), k


@pytest.mark.skipif(not HAVE_REF, reason="needs the reference build (oracle/_ref)")
def test_chroma_stage_equals_the_compiled_reference(gold):
    """CuFullDistortionFastTuMode_R run whole: its Cb / Cr distortion pairs, bits and has_coeff flags equal the full loop's and the rate's
    restatement for every chroma transform size (asserted inside uv_pin), and the recorded values are those"""
    for key, v in mg.uv_pin().items():
        assert np.array_equal(v, gold[key]), key
    # the harness tells a wrong shift apart: the unshifted distortion of a size with shift 2 is not what the reference returns
    o = mg.uv_restatement(1)
    dist, _, _ = mg.ref_uv_stage(1, o)
    assert np.array_equal(dist, o["dist"]) and not np.array_equal(dist, o["dist"] << np.uint64(2))


def test_mirror_sets_argtypes_and_restype(pkg):
    lib = pkg.load_library()
    hdr = open(os.path.join(ROOT, "include", "svt_hip_dsp.h")).read()
    for n, nargs, ret, cret in (("svt_hip_md_decide_frame", 3, ctypes.c_int, "int"), ("svt_hip_md_search_frame", 8, ctypes.c_int, "int"),
                                ("svt_hip_md_search_scratch_bytes", 2, ctypes.c_size_t, "size_t")):
        assert f"{cret} {n}(" in hdr
        f = getattr(lib, n)
        assert f.argtypes is not None and len(f.argtypes) == nargs and f.restype is ret, n


def test_struct_layouts_match_the_header(pkg):
    structs = (("svt_hip_md_blk", pkg.MdBlk, {}), ("svt_hip_md_rates", pkg.MdRates, {}), ("svt_hip_md_decision", pkg.MdDecision, {}),
               ("svt_hip_md_decide_group", pkg.MdDecideGroup, {"lambda_": "lambda"}), ("svt_hip_md_search_group", pkg.MdSearchGroup, {}))
    assert ctypes.sizeof(pkg.MdDecision) == 72 and ctypes.alignment(pkg.MdDecision) == 8 and ctypes.sizeof(pkg.MdBlk) == 4
    assert ctypes.sizeof(pkg.MdRates) == 4 * pkg.MD_RATE_WORDS == 4 * mg.RATE_WORDS
    assert pkg.md_decision_dtype() == mg.DEC_DTYPE and pkg.md_blk_dtype() == mg.BLK_DTYPE
    assert pkg.inter_cand_dtype() == mg.CAND_DTYPE and np.dtype(pkg.SvtHipDsp.CFL_DECISION_DTYPE) == mg.CFL_DEC_DTYPE
    assert np.dtype(pkg.SvtHipDsp.TX_DECISION_DTYPE) == mg.TX_DEC_DTYPE
    for (name, off, _), (f, _) in zip(((n, mg.DEC_DTYPE.fields[n][1], 0) for n in mg.DEC_DTYPE.names), pkg.MdDecision._fields_):
        assert name == f and getattr(pkg.MdDecision, f).offset == off, name
    assert tuple(pkg.MD_RATE_TABLES) == tuple(mg.RATE_TABLES) and pkg.MD_NO_INTRA == mg.NO_INTRA == 0xFF
    assert tuple(pkg.BSIZE_W) == tuple(mg.BSIZE_W) and tuple(pkg.BSIZE_H) == tuple(mg.BSIZE_H)
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


def test_pack_md_rates_and_plane_sizes(pkg):
    T = mg.rate_tables(np.arange(mg.RATE_WORDS, dtype=np.int32))
    assert np.array_equal(pkg.pack_md_rates(T), np.arange(mg.RATE_WORDS))
    assert pkg.md_plane_sizes(0) == [(4, 4, 16)] * 3 and pkg.md_plane_sizes(9) == [(32, 32, 1024), (16, 16, 256), (16, 16, 256)]
    assert pkg.md_plane_sizes(12) == [(64, 64, 1024), (32, 32, 1024), (32, 32, 1024)] and pkg.md_plane_sizes(16) == [(4, 16, 64), (4, 8, 32), (4, 8, 32)]


def search_groups(pkg, specs):
    """an MdSearchGroup array from (bsize, n, nblocks, luma tx_size, luma types, chroma tx_size or None, asked) with asked a set of "best_qcoeff",
    "best_dqcoeff", "best_dqcoeff_c" (the decide's gathers) and "luma_decision" (supplied): a pointer is any non-NULL value, the scratch
    computation reads no memory"""
    arr = (pkg.MdSearchGroup * max(len(specs), 1))()
    for i, (bsize, n, nb, s, types, sc, asked) in enumerate(specs):
        g = arr[i]
        g.md.bsize, g.md.n, g.md.nblocks, g.md.ninter, g.md.nintra = bsize, n, nb, 1, 1
        g.luma.fl.tx_size, g.luma.fl.ntypes, g.luma.fl.nblocks = s, len(types), nb * n
        for j, t in enumerate(types):
            g.luma.fl.tx_types[j] = t
        g.luma.d_decision = 0x1000 if "luma_decision" in asked else None
        g.md.d_best_qcoeff[0] = 0x1000 if "best_qcoeff" in asked else None
        g.md.d_best_dqcoeff[0] = 0x1000 if "best_dqcoeff" in asked else None
        g.use_chroma = int(sc is not None)
        for c in (g.cb, g.cr):
            c.tx_size, c.ntypes, c.nblocks = (sc if sc is not None else 0), 1, nb * n
        g.md.d_best_dqcoeff[1] = g.md.d_best_dqcoeff[2] = 0x1000 if "best_dqcoeff_c" in asked else None
    return arr


def test_scratch_bytes_on_hand_computed_cases(pkg):
    lib = pkg.load_library()
    sb = lambda specs, n=None: lib.svt_hip_md_search_scratch_bytes(search_groups(pkg, specs), len(specs) if n is None else n)
    # 8x8 (bsize 3), n 3, 5 blocks = 15 survivors, luma TX_8X8 with 2 types, no chroma, no gather: the record 15 * 40 = 600 -> 608; the luma
    # search over 30 pairs: dist 480, eob 60 -> 64, bits 240, qcoeff 30 * 256 = 7680
    luma = 480 + 64 + 240 + 7680
    assert sb([(3, 3, 5, 1, [0, 9], None, set())]) == 608 + luma
    assert sb([(3, 3, 5, 1, [0, 9], None, {"luma_decision"})]) == luma
    # the gathers ask for the survivors' best coefficients: 15 * 64 * 4 = 3840 each, and best_dqcoeff makes the luma search keep dqcoeff
    assert sb([(3, 3, 5, 1, [0, 9], None, {"best_qcoeff"})]) == 608 + 3840 + luma
    assert sb([(3, 3, 5, 1, [0, 9], None, {"best_qcoeff", "best_dqcoeff"})]) == 608 + 2 * 3840 + luma + 7680
    # chroma TX_4X4: per plane dist 240, eob 30 -> 32, bits 120 -> 128, qcoeff 15 * 64 = 960 (and dqcoeff 960 when its gather asks)
    assert sb([(3, 3, 5, 1, [0, 9], 0, set())]) == 608 + 2 * (240 + 32 + 128 + 960) + luma
    assert sb([(3, 3, 5, 1, [0, 9], 0, {"best_dqcoeff_c"})]) == 608 + 2 * (240 + 32 + 128 + 2 * 960) + luma
    # an empty group adds nothing; the order of the groups does not matter to the sum
    assert sb([(0, 1, 0, 0, [0], None, set()), (3, 3, 5, 1, [0, 9], None, set())]) == 608 + luma
    assert sb([]) == 0 and sb([(3, 3, 0, 1, [0, 9], None, set())]) == 0
    # bad parameters: 0
    for bad in ((13, 3, 5, 4, [0], None, set()), (22, 3, 5, 1, [0], None, set()), (3, 0, 5, 1, [0], None, set()), (3, 41, 5, 1, [0], None, set()),
                (3, 3, 5, 1, [9, 1], None, set()), (3, 3, 5, 0, [0, 9], None, set()), (3, 3, 5, 1, [0, 9], 1, set()), (3, 3, 0x40000000, 1, [0], None, set())):
        assert sb([bad]) == 0, bad
    assert sb([(3, 3, 5, 1, [0, 9], None, set()), (13, 3, 0, 1, [0], None, set())]) == 0      # an empty group's scalars count
    assert lib.svt_hip_md_search_scratch_bytes(None, 1) == 0 and lib.svt_hip_md_search_scratch_bytes(None, -1) == 0


def test_frame_calls_without_a_device_or_with_bad_arguments(pkg):
    """a NULL group list: SVT_HIP_ERR_INVALID (-2) on a machine with a device, SVT_HIP_ERR_NO_DEVICE (-1) without one, as the sibling
    calls answer (the device is looked for first).  No groups at all is not an error."""
    import torch
    lib = pkg.load_library()
    have = torch.cuda.is_available()
    bad = INVALID if have else NO_DEVICE
    assert lib.svt_hip_md_decide_frame(None, 1, None) == bad and lib.svt_hip_md_decide_frame(None, -1, None) == bad
    assert lib.svt_hip_md_decide_frame(None, 0, None) == (0 if have else NO_DEVICE)
    q = (ctypes.c_int16 * 8)(*([64] * 8))
    rows = pkg.QRows(*[ctypes.addressof(q)] * 5)
    assert lib.svt_hip_md_search_frame(None, 1, 1, ctypes.addressof(rows), None, None, 0, None) == bad
    assert lib.svt_hip_md_search_frame(None, 0, 1, ctypes.addressof(rows), None, None, 0, None) == (0 if have else NO_DEVICE)

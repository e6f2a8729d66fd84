"""CPU: the C ABI of svt_hip_tx_decide_frame / svt_hip_tx_search_frame / svt_hip_tx_type_rate_index as the Python mirror binds it, and
the golden fixture of the transform-type decision (tests/golden/tx_decide.npz, written by tests/golden/make_golden_tx_decide.py: the
per-pair cost is the reference's av1_tu_calc_cost_luma, the loop glue is the generator's own, see there)."""
import ctypes
import os
import subprocess
import sys
import tempfile

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden", "tx_decide.npz")
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
import make_golden_tx_decide as mg  # noqa: E402

HAVE_REF = os.path.exists(os.path.join(ROOT, "oracle", "_ref", "libsvtref.so"))
INVALID, NO_DEVICE = -2, -1


@pytest.fixture(scope="module")
def gold():
    return np.load(GOLD)


def test_fixture_loads_and_meets_the_conditions(gold):
    mg.check_conditions(gold)
    for k in range(mg.NCASES):
        T = len(gold[f"c{k}_types"])
        assert gold[f"c{k}_dist"].shape == (mg.NBLOCKS, T, 2) and gold[f"c{k}_dist"].dtype == np.uint64
        assert gold[f"c{k}_eob"].shape == gold[f"c{k}_bits"].shape == gold[f"c{k}_cost"].shape == (mg.NBLOCKS, T)
        assert gold[f"c{k}_decision"].shape == (mg.NBLOCKS, 40) and gold[f"c{k}_decision"].dtype == np.uint8
        assert not mg.decisions(gold, k)["pad"].any()
    assert [int(gold[f"c{k}_size"]) for k in range(19)] == list(range(19))
    assert all(0 not in gold[f"c{k}_types"] for k in (19, 20))
    assert gold["helper"].shape == (19, 2, 2, 3)
    assert os.path.getsize(GOLD) < 512 << 10


def test_generator_reproduces_the_fixture_inputs_and_the_restatement_its_results(gold):
    """without the reference: the synthetic inputs are the generator's, and np_tx_decide gives the fixture's costs and records"""
    for k in range(mg.NCASES):
        for key, v in mg.gen_case(k, None).items():
            assert np.array_equal(v, gold[f"c{k}_{key}"]), (k, key)
        dec, cost = mg.np_tx_decide(gold[f"c{k}_dist"], gold[f"c{k}_eob"], gold[f"c{k}_bits"], gold[f"c{k}_types"], int(gold[f"c{k}_lam"]))
        assert np.array_equal(cost, gold[f"c{k}_cost"]) and np.array_equal(dec, mg.decisions(gold, k)), k


def test_the_loop_glue_written_out_as_the_reference_loop(gold):
    """the record of every block by a plain loop in the reference's order (skip, strict <, first wins), in Python integers"""
    for k in range(mg.NCASES):
        types, lam = [int(t) for t in gold[f"c{k}_types"]], int(gold[f"c{k}_lam"])
        dist, eob, bits = gold[f"c{k}_dist"], gold[f"c{k}_eob"], gold[f"c{k}_bits"]
        dec = mg.decisions(gold, k)
        for b in range(mg.NBLOCKS):
            best, best_i = mg.U64_MAX, None
            for i, ty in enumerate(types):
                if int(eob[b, i]) == 0 and ty != mg.DCT_DCT:
                    continue
                cost = ((((int(bits[b, i]) * lam) & mg.U64_MAX) + 256 & mg.U64_MAX) >> 9) + int(dist[b, i, 0]) * 128 & mg.U64_MAX
                if cost < best:
                    best, best_i = cost, i
            d = dec[b]
            if best_i is None:
                want = (mg.U64_MAX, 0, 0, 0, 0, mg.DCT_DCT, mg.NO_CANDIDATE, 0)
            else:
                want = (best, int(dist[b, best_i, 0]), int(dist[b, best_i, 1]), int(bits[b, best_i]), int(eob[b, best_i]), types[best_i], best_i,
                        int(eob[b, best_i] != 0))
            got = (int(d["cost"]), int(d["dist"][0]), int(d["dist"][1]), int(d["bits"]), int(d["eob"]), int(d["tx_type"]), int(d["type_index"]),
                   int(d["has_coeff"]))
            assert got == want, (k, b)


@pytest.mark.skipif(not HAVE_REF, reason="needs the reference build (oracle/_ref)")
def test_restatement_equals_the_reference_on_every_case(gold):
    L = mg.ref_lib()
    rc = mg.RefCandidate()
    for k in range(mg.NCASES):
        dist, eob, bits = gold[f"c{k}_dist"], gold[f"c{k}_eob"], gold[f"c{k}_bits"]
        cost, has = mg.ref_costs(L, rc, int(gold[f"c{k}_size"]), dist, eob, bits, int(gold[f"c{k}_lam"]))
        assert np.array_equal(cost, gold[f"c{k}_cost"]) and np.array_equal(cost, mg.np_cost(dist, bits, int(gold[f"c{k}_lam"]))), k
        assert np.array_equal(has, gold[f"c{k}_has"]) and np.array_equal(has, eob != 0), k
    assert np.array_equal(mg.gen_helper(L), gold["helper"])


def test_rate_index_helper_equals_the_fixture(pkg, gold):
    """svt_hip_tx_type_rate_index is a host helper: it answers without a device; where the reference reads a row it names that row"""
    lib = pkg.load_library()
    coded_any = 0
    for s in range(19):
        for inter in (0, 1):
            for red in (0, 1):
                want = [int(v) for v in gold["helper"][s, inter, red]]
                a, b = ctypes.c_int(-7), ctypes.c_int(-7)
                rc = lib.svt_hip_tx_type_rate_index(s, inter, red, ctypes.addressof(a), ctypes.addressof(b))
                assert rc == want[0], (s, inter, red)
                if rc:
                    assert [a.value, b.value] == want[1:], (s, inter, red)
                    coded_any += 1
                assert mg.np_tx_type_rate_index(s, inter, red)[0] == rc
                assert pkg.tx_type_rate_index(s, inter, red) == (bool(rc), a.value, b.value)
                assert lib.svt_hip_tx_type_rate_index(s, inter, red, None, None) == rc
    assert coded_any > 30
    a = ctypes.c_int(77)
    for bad in (-1, 19, 1000):
        assert lib.svt_hip_tx_type_rate_index(bad, 0, 0, ctypes.addressof(a), None) == INVALID and a.value == 77


def test_mirror_sets_argtypes_and_restype(pkg):
    lib = pkg.load_library()
    hdr = open(os.path.join(ROOT, "include", "svt_hip_dsp.h")).read()
    for n, nargs, ret, cret in (("svt_hip_tx_decide_frame", 3, ctypes.c_int, "int"), ("svt_hip_tx_search_frame", 11, ctypes.c_int, "int"),
                                ("svt_hip_tx_search_scratch_bytes", 2, ctypes.c_size_t, "size_t"),
                                ("svt_hip_tx_type_rate_index", 5, ctypes.c_int, "int")):
        assert f"{cret} {n}(" in hdr
        f = getattr(lib, n)
        assert f.argtypes is not None and len(f.argtypes) == nargs and f.restype is ret, n


def test_struct_layouts_match_the_header(pkg):
    structs = (("svt_hip_tx_decision", pkg.TxDecision, {}), ("svt_hip_tx_decide_group", pkg.TxDecideGroup, {"lambda_": "lambda"}),
               ("svt_hip_tx_search_group", pkg.TxSearchGroup, {"lambda_": "lambda"}))
    assert pkg.TxDecision is pkg.SvtHipDsp.TxDecision and ctypes.sizeof(pkg.TxDecision) == 40 and ctypes.alignment(pkg.TxDecision) == 8
    assert np.dtype(pkg.SvtHipDsp.TX_DECISION_DTYPE) == mg.DEC_DTYPE
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
    """a TxSearchGroup array from (tx_size, types, nblocks, supplied) with supplied a set of "dist", "eob", "qcoeff", "dqcoeff", "best_dqcoeff":
    a supplied pointer is any non-NULL value, the scratch computation reads no memory"""
    arr = (pkg.TxSearchGroup * max(len(specs), 1))()
    for i, (s, types, n, have) in enumerate(specs):
        g = arr[i]
        g.fl.tx_size, g.fl.ntypes, g.fl.nblocks = s, len(types), n
        for j, t in enumerate(types):
            g.fl.tx_types[j] = t
        for k in ("dist", "eob", "qcoeff", "dqcoeff"):
            setattr(g.fl, "d_" + k, 0x1000 if k in have else None)
        g.d_best_dqcoeff = 0x1000 if "best_dqcoeff" in have else None
    return arr


def test_scratch_bytes_on_hand_computed_cases(pkg):
    lib = pkg.load_library()
    sb = lambda specs, n=None: lib.svt_hip_tx_search_scratch_bytes(search_groups(pkg, specs), len(specs) if n is None else n)
    # 4x4, 3 types, 5 blocks = 15 pairs, nothing supplied, no best_dqcoeff: dist 240, eob 30 -> 32, bits 120 -> 128, qcoeff 15 * 64 = 960
    assert sb([(0, [0, 1, 9], 5, set())]) == 240 + 32 + 128 + 960
    # the same with best_dqcoeff asked for: dqcoeff another 960
    assert sb([(0, [0, 1, 9], 5, {"best_dqcoeff"})]) == 240 + 32 + 128 + 960 + 960
    # everything supplied: only the bits, 15 * 8 = 120 -> 128
    assert sb([(0, [0, 1, 9], 5, {"dist", "eob", "qcoeff", "dqcoeff", "best_dqcoeff"})]) == 128
    # 64x64 packs to 32x32: 7 blocks of 1 type: dist 112, eob 14 -> 16, bits 56 -> 64, qcoeff 7 * 4096; dist supplied in the second group
    assert sb([(4, [0], 7, set())]) == 112 + 16 + 64 + 28672
    assert sb([(4, [0], 7, set()), (4, [0], 7, {"dist"})]) == 2 * (112 + 16 + 64 + 28672) - 112
    # 16x8, 16 types, 1 block: dist 256, eob 32, bits 128, qcoeff and dqcoeff 16 * 512
    assert sb([(8, list(range(16)), 1, {"best_dqcoeff"})]) == 256 + 32 + 128 + 2 * 8192
    # an empty group adds nothing; no groups need nothing
    assert sb([(0, [0], 0, set()), (0, [0, 1, 9], 5, set())]) == 240 + 32 + 128 + 960
    assert sb([]) == 0 and sb([(3, [0, 9], 0, set())]) == 0
    # bad parameters: 0
    assert sb([(19, [0], 5, set())]) == 0 and sb([(-1, [0], 5, set())]) == 0
    assert sb([(0, [], 5, set())]) == 0 and sb([(0, [0, 0], 5, set())]) == 0 and sb([(3, [0, 1], 5, set())]) == 0 and sb([(0, [16], 5, set())]) == 0
    assert sb([(0, [0, 1], 0x40000000, set())]) == 0                      # nblocks * ntypes = 2^31
    assert sb([(0, [0, 1, 9], 5, set()), (4, [9], 0, set())]) == 0        # an empty group's types count
    assert lib.svt_hip_tx_search_scratch_bytes(None, 1) == 0 and lib.svt_hip_tx_search_scratch_bytes(None, -1) == 0


def test_frame_calls_without_a_device_or_with_bad_arguments(pkg):
    """a NULL group list: SVT_HIP_ERR_INVALID (-2) on a machine with a device, SVT_HIP_ERR_NO_DEVICE (-1) without one, as the sibling
    calls answer (the device is looked for first); neither call ever returns a result.  No groups at all is not an error."""
    import torch
    lib = pkg.load_library()
    have = torch.cuda.is_available()
    bad = INVALID if have else NO_DEVICE
    assert lib.svt_hip_tx_decide_frame(None, 1, None) == bad and lib.svt_hip_tx_decide_frame(None, -1, None) == bad
    assert lib.svt_hip_tx_decide_frame(None, 0, None) == (0 if have else NO_DEVICE)
    q = (ctypes.c_int16 * 8)(*([64] * 8))
    P = ctypes.addressof(q)
    assert lib.svt_hip_tx_search_frame(None, 1, 1, P, P, P, P, P, None, 0, None) == bad
    assert lib.svt_hip_tx_search_frame(None, 0, 1, P, P, P, P, P, None, 0, None) == (0 if have else NO_DEVICE)
    g = search_groups(pkg, [(0, [0, 1, 9], 5, set())])
    assert lib.svt_hip_tx_search_frame(g, 1, 1, P, P, P, P, P, None, 0, None) == bad      # a group that needs a scratch, none given

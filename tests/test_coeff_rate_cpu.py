"""CPU: the C ABI of svt_hip_coeff_rate_frame / svt_hip_coeff_cost_index as the Python mirror binds it, and the golden fixture of the
coefficient rate (tests/golden/coeff_rate.npz, written by tests/golden/make_golden_coeff_rate.py from the reference's
av1_cost_coeffs_txb; its coefficient-context derivation is pinned to the AV1 specification, see the generator)."""
import ctypes
import os
import subprocess
import sys
import tempfile

import numpy as np
import pytest

from svtlibs import TX_H, TX_W

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden", "coeff_rate.npz")
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
import make_golden_coeff_rate as mg  # noqa: E402

HAVE_REF = os.path.exists(os.path.join(ROOT, "oracle", "_ref", "libsvtref.so"))


@pytest.fixture(scope="module")
def gold():
    return np.load(GOLD)


def test_fixture_loads_and_covers_every_size_class_and_pattern(gold):
    classes = set()
    for s in range(19):
        types = [int(t) for t in gold[f"s{s}_types"]]
        assert types == mg.types_of(s) and 0 in types, s
        classes |= {mg.tx_class(t) for t in types}
        T, n = len(types), min(TX_W[s], 32) * min(TX_H[s], 32)
        assert gold[f"s{s}_q"].shape == (T, 24, n) and gold[f"s{s}_eob"].shape == (T, 24) and gold[f"s{s}_bits"].shape == (T, 24)
        assert gold[f"s{s}_coeff_cost"].shape == (529,) and gold[f"s{s}_eob_cost"].shape == (22,)
        assert gold[f"s{s}_skip_ctx"].max() <= 12 and gold[f"s{s}_dc_ctx"].max() <= 2
        eob, q = gold[f"s{s}_eob"], gold[f"s{s}_q"]
        assert (eob[:, 0] == 0).all() and (eob[:, 1] == 1).all() and (eob[:, 4] == n).all()
        assert (np.abs(q[:, 8]).max(axis=1) == 14).all() and (np.abs(q[:, 9]).max(axis=1) >= 270).all() and (q[:, 10] <= 0).all()
        assert [int(e) - 1 for e in eob[0, 11:15]] == [n // 8, n // 8 + 1, n // 4, n // 4 + 1]      # both sides of the last-context limits
        assert int(gold[f"s{s}_bits"].max()) < 2 ** 31
    assert classes == {0, 1, 2}
    assert {int(v) for s in range(19) for v in gold[f"s{s}_skip_ctx"]} == set(range(13))
    assert os.path.getsize(GOLD) < os.path.getsize(os.path.join(ROOT, "tests", "golden", "cdef.npz"))


def test_generator_reproduces_the_fixture_inputs(gold):
    for s in (0, 6, 9, 4):
        d = mg.gen_size(s, None)                      # the restatement in place of the reference
        for k, v in d.items():
            assert np.array_equal(v, gold[f"s{s}_{k}"]), (s, k)


@pytest.mark.skipif(not HAVE_REF, reason="needs the reference build (oracle/_ref)")
def test_restatement_equals_the_reference_on_every_case(gold):
    L = mg.ref_lib()
    rc = mg.RefCandidate()
    for s in range(19):
        cc, ec = gold[f"s{s}_coeff_cost"], gold[f"s{s}_eob_cost"]
        for ti, t in enumerate(int(t) for t in gold[f"s{s}_types"]):
            scan = mg.scan_of(s, t)
            for b in range(24):
                a = (gold[f"s{s}_q"][ti, b], int(gold[f"s{s}_eob"][ti, b]), s, t, int(gold[f"s{s}_skip_ctx"][b]), int(gold[f"s{s}_dc_ctx"][b]), cc, ec)
                ref = mg.ref_cost(L, rc, *a)
                assert ref == int(gold[f"s{s}_bits"][ti, b]) == mg.np_cost_coeffs_txb(*a, scan), (s, t, b)


@pytest.mark.skipif(not HAVE_REF, reason="needs the reference build (oracle/_ref)")
def test_hand_computed_blocks_through_the_reference():
    mg.prove_offsets(mg.ref_lib())                    # raises SystemExit on a difference


def test_hand_computed_blocks():
    """the three blocks whose cost is a sum of table entries written out by hand, against the restatement and the fixture's values"""
    for s in (0, 1, 9):
        cc, ec = mg.tables_of(s)
        scan = mg.scan_of(s, 0)
        for sk, dc in ((0, 0), (7, 2), (12, 1)):
            want = mg.hand_costs(s, 0, sk, dc, cc, ec, scan)
            got = [mg.np_cost_coeffs_txb(q, e, s, 0, sk, dc, cc, ec, scan) for q, e in mg.hand_blocks(s, scan)]
            assert got == want, (s, sk, dc)
    z = np.load(GOLD)
    for s in range(19):                               # blocks 1 .. 3 of every size's DCT_DCT are these three
        cc, ec, scan = z[f"s{s}_coeff_cost"], z[f"s{s}_eob_cost"], mg.scan_of(s, 0)
        for b, (q, e) in zip((1, 2, 3), mg.hand_blocks(s, scan)):
            assert np.array_equal(z[f"s{s}_q"][0, b], q) and z[f"s{s}_eob"][0, b] == e
            want = mg.hand_costs(s, 0, int(z[f"s{s}_skip_ctx"][b]), int(z[f"s{s}_dc_ctx"][b]), cc, ec, scan)[b - 1]
            assert int(z[f"s{s}_bits"][0, b]) == want, (s, b)


def test_mirror_sets_argtypes_and_restype(pkg):
    lib = pkg.load_library()
    new = [n for n in ("svt_hip_coeff_rate_frame", "svt_hip_coeff_cost_index")]
    hdr = open(os.path.join(ROOT, "include", "svt_hip_dsp.h")).read()
    for n, nargs in zip(new, (3, 3)):
        assert f"int {n}(" in hdr
        f = getattr(lib, n)
        assert f.argtypes is not None and len(f.argtypes) == nargs and f.restype is ctypes.c_int, n


def test_group_layout_matches_header(pkg):
    G = pkg.SvtHipDsp.CoeffRateGroup
    fields = [n for n, _ in G._fields_]
    code = ('#include <stddef.h>\n#include <stdio.h>\n#include "svt_hip_dsp.h"\nint main(void){printf("%zu"' + ' " %zu"' * len(fields) +
            ', sizeof(svt_hip_coeff_rate_group)' + "".join(f", offsetof(svt_hip_coeff_rate_group, {n})" for n in fields) + ');return 0;}\n')
    with tempfile.TemporaryDirectory() as d:
        open(os.path.join(d, "t.c"), "w").write(code)
        subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), os.path.join(d, "t.c"), "-o", os.path.join(d, "t")])
        out = [int(v) for v in subprocess.check_output([os.path.join(d, "t")]).decode().split()]
    assert out == [ctypes.sizeof(G)] + [getattr(G, n).offset for n in fields]


def test_cost_index_helper(pkg):
    """svt_hip_coeff_cost_index is a host helper: it answers without a device, and a bad size is SVT_HIP_ERR_INVALID"""
    lib = pkg.load_library()
    for s in range(19):
        assert pkg.coeff_cost_index_lib(s) == pkg.coeff_cost_index(s) == mg.cost_index(s), s
    assert [pkg.coeff_cost_index(s) for s in (0, 4, 13, 17)] == [(0, 0), (4, 6), (1, 2), (3, 5)]
    a = ctypes.c_int(77)
    for bad in (-1, 19, 1000):
        assert lib.svt_hip_coeff_cost_index(bad, ctypes.addressof(a), None) == -2 and a.value == 77
    assert lib.svt_hip_coeff_cost_index(3, None, None) == 0


def test_frame_call_without_a_device_or_with_bad_arguments(pkg):
    """a NULL group list: SVT_HIP_ERR_INVALID (-2) on a machine with a device, SVT_HIP_ERR_NO_DEVICE (-1) without one, as the sibling
    calls answer (the device is looked for first); it never launches.  No groups at all is not an error."""
    import torch
    lib = pkg.load_library()
    have = torch.cuda.is_available()
    assert lib.svt_hip_coeff_rate_frame(None, 1, None) == (-2 if have else -1)
    assert lib.svt_hip_coeff_rate_frame(None, -1, None) == (-2 if have else -1)
    assert lib.svt_hip_coeff_rate_frame(None, 0, None) == (0 if have else -1)

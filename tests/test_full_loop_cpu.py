"""CPU: the C ABI of svt_hip_full_loop_frame as the Python mirror binds it, and the golden fixture of the mode-decision full loop
(tests/golden/full_loop.npz, written by tests/golden/make_golden_full_loop.py from the reference)."""
import ctypes
import os
import subprocess
import tempfile

import numpy as np
import pytest

from svtlibs import TX_H, TX_W, txfm_allowed

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden", "full_loop.npz")


def test_mirror_sets_argtypes_and_restype(pkg):
    lib = pkg.load_library()
    f = lib.svt_hip_full_loop_frame
    assert f.argtypes is not None and len(f.argtypes) == 9
    assert f.restype is ctypes.c_int


def test_group_layout_matches_header(pkg):
    G = pkg.SvtHipDsp.FullLoopGroup
    fields = [n for n, _ in G._fields_]
    code = ('#include <stddef.h>\n#include <stdio.h>\n#include "svt_hip_dsp.h"\nint main(void){printf("%zu"' + ' " %zu"' * len(fields) +
            ', sizeof(svt_hip_full_loop_group)' + "".join(f", offsetof(svt_hip_full_loop_group, {n})" for n in fields) + ');return 0;}\n')
    with tempfile.TemporaryDirectory() as d:
        open(os.path.join(d, "t.c"), "w").write(code)
        subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), os.path.join(d, "t.c"), "-o", os.path.join(d, "t")])
        out = [int(v) for v in subprocess.check_output([os.path.join(d, "t")]).decode().split()]
    assert out == [ctypes.sizeof(G)] + [getattr(G, n).offset for n in fields]


def test_fixture_covers_every_size_and_allowed_type():
    z = np.load(GOLD)
    for s in range(19):
        want = [t for t in range(16) if txfm_allowed(s, t)]
        assert list(z[f"s{s}_types"]) == want, s
        T, n = len(want), min(TX_W[s], 32) * min(TX_H[s], 32)
        assert z[f"s{s}_src"].shape == (4, 2, TX_H[s], TX_W[s])
        assert z[f"s{s}_dist_c"].shape == (T, 4, 4, 2, 2) and z[f"s{s}_dist_avx2"].shape == (T, 4, 4, 2, 2)
        assert z[f"s{s}_eob"].shape == (T, 4, 4, 2) and z[f"s{s}_qcoeff"].shape == (T, 4, 4, 2, n)
        assert (z[f"s{s}_eob"][:, :, 2] == 0).all()                       # the zero residual takes the cbf_zero branch
        assert (z[f"s{s}_eob"][:, :, 0] > 0).any()


@pytest.mark.skipif(not os.path.exists(os.path.join(ROOT, "oracle", "_ref", "libsvtref.so")), reason="needs the reference build (oracle/_ref)")
def test_generator_reproduces_the_fixture():
    import sys
    sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
    import make_golden_full_loop as mg
    z = np.load(GOLD)
    for s in (0, 2, 3, 4, 11, 13):
        d = mg.gen_size(s)
        for k, v in d.items():
            assert np.array_equal(v, z[f"s{s}_{k}"]), (s, k)

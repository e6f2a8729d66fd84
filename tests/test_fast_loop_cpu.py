"""CPU: the fixture of the mode-decision fast loop's intra candidates (tests/golden/fast_loop.npz, written by
tests/golden/make_golden_fast_loop.py from the reference) against the oracle's build_intra_predictors and numpy distortions, and the
candidate list of inject_intra_candidates (svt_hip_md_intra_candidates and its Python mirror)."""
import ctypes
import os

import numpy as np
import pytest

import sys

import svtlibs
from svtlibs import TX_H, TX_W, ptr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden", "fast_loop.npz")
# AV1 block_size (BLOCK_4X4 = 0 .. BLOCK_64X16 = 21) -> (width, height)
BSIZE_WH = [(4, 4), (4, 8), (8, 4), (8, 8), (8, 16), (16, 8), (16, 16), (16, 32), (32, 16), (32, 32), (32, 64), (64, 32), (64, 64),
            (64, 128), (128, 64), (128, 128), (4, 16), (16, 4), (8, 32), (32, 8), (16, 64), (64, 16)]


HAVE_REF = svtlibs.ref() is not None and hasattr(svtlibs.ref(), "ref_md_inject_intra")
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
import make_golden_fast_loop as mgl  # noqa: E402


def wrapped_ssd(src, pred):
    t = (src.astype(np.int64) - pred.astype(np.int64)) & 255
    d = np.where(t <= 128, t, 256 - t)
    return int((d * d).sum())


def test_mirror_sets_argtypes_and_restype(pkg):
    lib = pkg.load_library()
    assert lib.svt_hip_intra_fast_loop_frame.argtypes is not None and len(lib.svt_hip_intra_fast_loop_frame.argtypes) == 5
    assert lib.svt_hip_intra_fast_loop_frame.restype is ctypes.c_int
    assert lib.svt_hip_md_intra_candidates.argtypes is not None and len(lib.svt_hip_md_intra_candidates.argtypes) == 8
    assert lib.svt_hip_md_intra_candidates.restype is ctypes.c_int
    assert ctypes.sizeof(pkg.SvtHipDsp.FastLoopGroup) == 216          # == sizeof(svt_hip_fast_loop_group)


def test_fixture_reproduced_by_oracle_predictions_and_numpy_distortions():
    g = np.load(GOLD)
    O = svtlibs.oracle()
    for s in range(19):
        w, h = TX_W[s], TX_H[s]
        p = f"s{s}_"
        modes, deltas = g[p + "modes"], g[p + "deltas"]
        assert len(modes) == (13 if (w, h) in ((4, 4), (4, 8), (8, 4)) else 61)
        for i in range(g[p + "blk"].shape[0]):
            blk, top, left, src = g[p + "blk"][i], g[p + "top"][i], g[p + "left"][i], g[p + "src"][i]
            for c in range(len(modes)):
                pred = np.zeros((h, w), np.uint8)
                O.svt_oracle_build_intra_predictors(0, ctypes.c_void_p(top.ctypes.data + 16), ctypes.c_void_p(left.ctypes.data + 16), ptr(pred), w,
                                                    int(modes[c]), int(deltas[c]), s, int(blk[3]), int(blk[4]), int(blk[5]), int(blk[6]),
                                                    int(blk[7]), int(blk[2]), 8)
                diff = src.astype(np.int64) - pred.astype(np.int64)
                assert int(np.abs(diff).sum()) == int(g[p + "sad"][i, c]), (s, i, c)
                assert int((diff * diff).sum()) == int(g[p + "ssd_c"][i, c]), (s, i, c)
                if w == h:
                    assert wrapped_ssd(src, pred) == int(g[p + "ssd_avx2"][i, c]), (s, i, c)


def test_fixture_exercises_the_wrap():
    """the wrapped-byte SSD differs from the exact one somewhere (a 255 source over a near-0 prediction), and agrees on small residuals"""
    g = np.load(GOLD)
    differs = sum(int((g[f"s{s}_ssd_avx2"] != g[f"s{s}_ssd_c"]).sum()) for s in range(5))
    agrees = sum(int((g[f"s{s}_ssd_avx2"] == g[f"s{s}_ssd_c"]).sum()) for s in range(5))
    assert differs > 0 and agrees > 0


@pytest.mark.parametrize("is16", [False, True])
def test_md_intra_candidates_counts_and_order(pkg, is16):
    C = pkg.SvtHipDsp.md_intra_candidates
    m, d = C(16, 16, 16, 6, 0, is16)
    assert len(m) == (60 if is16 else 61)
    # DC first, then V with deltas -3 .. 3, ..., SMOOTH, SMOOTH_V, SMOOTH_H (, PAETH)
    assert list(m[:8]) == [0, 1, 1, 1, 1, 1, 1, 1] and list(d[1:8]) == [-3, -2, -1, 0, 1, 2, 3]
    assert list(m[-4:] if not is16 else m[-3:]) == ([9, 10, 11, 12] if not is16 else [9, 10, 11])
    # no deltas for BLOCK_4X4 / 4X8 / 8X4 (bsize >= BLOCK_8X8 in enum order: 4x16 and 16x4 keep them)
    for bs in (0, 1, 2):
        w, h = BSIZE_WH[bs]
        m, d = C(w, h, 8, bs, 0, is16)
        assert len(m) == (12 if is16 else 13) and not d.any()
    for bs in (16, 17):
        w, h = BSIZE_WH[bs]
        assert len(C(w, h, 16, bs, 0, is16)[0]) == (60 if is16 else 61)
    # intra_pred_mode 1, sq_size > 16: z2 angles dropped, delta 0 only
    m, d = C(32, 32, 32, 9, 1, False)
    assert len(m) == 10 and not d.any() and list(m) == [0, 1, 2, 3, 7, 8, 9, 10, 11, 12]
    # intra_pred_mode 1 on a 16x16 in a 16x16 square: untouched
    assert len(C(16, 16, 16, 6, 1, False)[0]) == 61
    # intra_pred_mode 2: no directional modes for sq_size > 16 or 4-sample sides
    assert len(C(32, 32, 32, 9, 2, False)[0]) == 5 and len(C(16, 16, 16, 6, 2, False)[0]) == 61
    # intra_pred_mode 3: no directional modes at all
    m, d = C(16, 16, 16, 6, 3, False)
    assert len(m) == 5 and list(m) == [0, 9, 10, 11, 12]


def test_md_intra_candidates_c_abi_equals_python(pkg):
    lib = pkg.load_library()
    for bs, (w, h) in enumerate(BSIZE_WH):
        for sq in sorted({max(w, h), 2 * max(w, h), 8, 16, 32, 64}):
            for ipm in range(4):
                for is16 in (0, 1):
                    m = np.zeros(64, np.uint8); d = np.zeros(64, np.int8)
                    n = lib.svt_hip_md_intra_candidates(w, h, sq, bs, ipm, is16, ptr(m), ptr(d))
                    pm, pd = pkg.SvtHipDsp.md_intra_candidates(w, h, sq, bs, ipm, bool(is16))
                    assert n == len(pm) and np.array_equal(m[:n], pm) and np.array_equal(d[:n], pd), (bs, sq, ipm, is16)
                    lm, ld = pkg.SvtHipDsp.md_intra_candidates_lib(w, h, sq, bs, ipm, bool(is16))
                    assert np.array_equal(lm, pm) and np.array_equal(ld, pd)
    m = np.zeros(64, np.uint8); d = np.zeros(64, np.int8)
    assert lib.svt_hip_md_intra_candidates(16, 16, 16, 6, 4, 0, ptr(m), ptr(d)) < 0
    assert lib.svt_hip_md_intra_candidates(16, 16, 16, 22, 0, 0, ptr(m), ptr(d)) < 0
    assert lib.svt_hip_md_intra_candidates(16, 16, 16, 6, 0, 0, None, None) < 0


@pytest.mark.skipif(not HAVE_REF, reason="needs the reference build with oracle/ref_md.c in it (oracle/_ref)")
def test_md_intra_candidates_equal_the_reference_inject_intra_candidates(pkg):
    """svt_hip_md_intra_candidates (C ABI) and its Python mirror against the reference's own inject_intra_candidates (oracle/ref_md.c) on
    every distinct geometry of the reference's block table (width, height, sq_size, bsize, has_uv), intra_pred_mode 0 .. 3, 8- and
    10-bit; and the list's other fields as the fast cost relies on them"""
    R = svtlibs.ref()
    lib = pkg.load_library()
    geoms = mgl.ref_geometries(R)
    assert {g[:2] for g in geoms} >= {(TX_W[s], TX_H[s]) for s in range(19)} and len({g[2] for g in geoms}) == 5
    for (w, h, sq, bs, has_uv), idx in sorted(geoms.items()):
        for ipm in range(4):
            for is16 in (0, 1):
                lst = mgl.ref_inject_list(R, idx, ipm, is16)
                m = np.zeros(64, np.uint8); d = np.zeros(64, np.int8)
                n = lib.svt_hip_md_intra_candidates(w, h, sq, bs, ipm, is16, ptr(m), ptr(d))
                assert n == len(lst) and np.array_equal(m[:n], lst[:, 0]) and np.array_equal(d[:n], lst[:, 1]), (w, h, sq, bs, ipm, is16)
                pm, pd = pkg.SvtHipDsp.md_intra_candidates(w, h, sq, bs, ipm, bool(is16))
                assert np.array_equal(pm, lst[:, 0]) and np.array_equal(pd, lst[:, 1]), (w, h, sq, bs, ipm, is16)
                # what svt_hip_fast_pick_frame's header states about the candidates
                lum = (lst[:, 0] >= 1) & (lst[:, 0] <= 8)
                assert np.array_equal(lst[:, 4], lum) and np.array_equal(lst[:, 5], (lst[:, 2] >= 1) & (lst[:, 2] <= 8))
                assert np.array_equal(lst[:, 6], lum & (bs >= 3)) and not lst[:, 3].any()

"""Golden vectors of the intra candidates of the mode-decision fast loop (perform_fast_loop, EbProductCodingLoop.c:1152-1300), from the
reference built as oracle/_ref/libsvtref.so.  Writes tests/golden/fast_loop.npz (data only):

    python tests/golden/make_golden_fast_loop.py

Per transform size, per block, per candidate of the list (8-bit):
  prediction       ref_build_intra_predictors (the reference's build_intra_predictors, as AV1IntraPredictionCL reaches it)
  sad              fast_loop_nx_m_sad_kernel(src, pred, bheight, bwidth); the AVX2 table entries (Compute4xMSadSub_AVX2_INTRIN,
                   compute{8,16,32,64}x_m_sad_avx2_intrin) are asserted to agree on every case
  ssd_c            spatial_full_distortion_kernel(src, pred, bwidth, bheight): the exact W x H SSD (the call site's swap corrected)
  ssd_avx2         square sizes only: spatial_full_distortion_kernel{4x4,8x8,16_mx_n}_ssse3_intrin with the call site's argument
                   order (area_width = bheight, area_height = bwidth) - the wrapped-byte SSD the encoder runs

Layout, per size s (key prefix f"s{s}_"): modes uint8 [C], deltas int8 [C] (the list the reference's own inject_intra_candidates gives
at intra_pred_mode 0, through oracle/ref_md.c: 61 entries wherever the size has angle deltas, else 13); top, left uint8 [NB, 176] (element 15 = the corner, 16 =
above[0] / left[0]); blk uint8 [NB, 8] (svt_hip_intra_blk: mode / angle_delta 0, filt_type, disable_edge_filter, n_top_px,
n_topright_px, n_left_px, n_bottomleft_px); src uint8 [NB, H, W]; sad, ssd_c uint64 [NB, C]; ssd_avx2 uint64 [NB, C] (square sizes).
Blocks cycle through six availability patterns (all, none, top only, left only, partial top-right, partial bottom-left), both
filt_type values, the edge filter on and off, and four inputs (random; a 255 source over a near-0 prediction and the reverse, which
exercise the wrapped difference; uniform)."""
import ctypes
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)
from svtlibs import TX_H, TX_W, ptr, ref  # noqa: E402

NB = 12
SEED = 1152


def ref_geometries(R):
    """the distinct block geometries of the reference's table (build_blk_geom(0): 64x64 superblocks) through oracle/ref_md.c:
    {(bwidth, bheight, sq_size, bsize, has_uv): first table index}"""
    out, info, idx = {}, np.zeros(8, np.int32), 0
    while R.ref_md_geom_info(idx, ptr(info)) == 0:
        out.setdefault(tuple(int(v) for v in info[:5]), idx)
        idx += 1
    return out


def ref_inject_list(R, idx, intra_pred_mode, is16, chroma_level=1):
    """the reference's own inject_intra_candidates on table entry idx -> int32 [n, 7]: mode, angle delta, uv mode, uv delta, the two
    directional flags, use_angle_delta"""
    lst = np.zeros((64, 7), np.int32)
    n = R.ref_md_inject_intra(idx, intra_pred_mode, int(is16), chroma_level, ptr(lst))
    assert 0 < n <= 64
    return lst[:n]


def ref_cand_list(R, s):
    """inject_intra_candidates' own luma list at intra_pred_mode 0, 8-bit, of every table geometry of the transform size's shape (they
    agree: at level 0 nothing depends on sq_size), asserted equal to the restatement cand_list"""
    w, h = TX_W[s], TX_H[s]
    lists = [ref_inject_list(R, idx, 0, False) for g, idx in sorted(ref_geometries(R).items()) if g[:2] == (w, h)]
    assert lists and all(np.array_equal(l[:, :2], lists[0][:, :2]) for l in lists), s
    modes, deltas = lists[0][:, 0].astype(np.uint8), lists[0][:, 1].astype(np.int8)
    rm, rd = cand_list(s)
    assert np.array_equal(modes, rm) and np.array_equal(deltas, rd), s
    return modes, deltas


def cand_list(s):
    """inject_intra_candidates' luma list at intra_pred_mode 0, 8-bit, restated (what runs where the reference is absent; ref_cand_list
    asserts it equal to the reference's own): 7 deltas unless the block is 4x4, 4x8 or 8x4"""
    w, h = TX_W[s], TX_H[s]
    nd = 1 if (w, h) in ((4, 4), (4, 8), (8, 4)) else 7
    modes, deltas = [], []
    for m in range(13):
        for k in (range(nd) if 1 <= m <= 8 else range(1)):
            modes.append(m); deltas.append(0 if nd == 1 or not 1 <= m <= 8 else k - 3)
    return np.array(modes, np.uint8), np.array(deltas, np.int8)


def block_case(rng, s, i):
    """-> (blk descriptor [8], top [176], left [176], src [H, W])"""
    w, h = TX_W[s], TX_H[s]
    pat, inp = i % 6, i % 4
    ft, dis = (i // 2) % 2, (i // 4) % 2
    n_top, n_tr, n_left, n_bl = [(w, h, h, w), (0, 0, 0, 0), (w, h, 0, 0), (0, 0, h, w),
                                 (w, int(rng.integers(1, h + 1)), h, 0), (w, 0, h, int(rng.integers(1, w + 1)))][pat]
    if inp == 0:
        top = rng.integers(0, 256, 176); left = rng.integers(0, 256, 176); src = rng.integers(0, 256, (h, w))
    elif inp == 1:                                   # 255 source over a near-0 prediction: |a - b| > 127, the wrap
        top = rng.integers(0, 4, 176); left = rng.integers(0, 4, 176); src = np.full((h, w), 255)
    elif inp == 2:                                   # the reverse
        top = rng.integers(252, 256, 176); left = rng.integers(252, 256, 176); src = rng.integers(0, 4, (h, w))
    else:                                            # uniform
        v = int(rng.integers(0, 256))
        top = np.full(176, v); left = np.full(176, v); src = np.full((h, w), int(rng.integers(0, 256)))
    blk = np.array([0, 0, ft, dis, n_top, n_tr, n_left, n_bl], np.uint8)
    return blk, top.astype(np.uint8), left.astype(np.uint8), np.ascontiguousarray(src.astype(np.uint8))


def main():
    R = ref()
    for f in ("fast_loop_nx_m_sad_kernel", "Compute4xMSadSub_AVX2_INTRIN", "compute8x_m_sad_avx2_intrin", "compute16x_m_sad_avx2_intrin",
              "compute32x_m_sad_avx2_intrin", "compute64x_m_sad_avx2_intrin"):
        getattr(R, f).restype = ctypes.c_uint32
    for f in ("spatial_full_distortion_kernel", "spatial_full_distortion_kernel4x4_ssse3_intrin", "spatial_full_distortion_kernel8x8_ssse3_intrin",
              "spatial_full_distortion_kernel16_mx_n_ssse3_intrin"):
        getattr(R, f).restype = ctypes.c_uint64
    avx2_sad = {4: R.Compute4xMSadSub_AVX2_INTRIN, 8: R.compute8x_m_sad_avx2_intrin, 16: R.compute16x_m_sad_avx2_intrin,
                32: R.compute32x_m_sad_avx2_intrin, 64: R.compute64x_m_sad_avx2_intrin}          # NxMSadKernelSubSampled_funcPtrArray[1][w >> 3]
    ssd_tab = {4: R.spatial_full_distortion_kernel4x4_ssse3_intrin, 8: R.spatial_full_distortion_kernel8x8_ssse3_intrin}
    d = {}
    for s in range(19):
        w, h = TX_W[s], TX_H[s]
        rng = np.random.default_rng(SEED + s)
        modes, deltas = ref_cand_list(R, s) if hasattr(R, "ref_md_inject_intra") else cand_list(s)          # a build from before oracle/ref_md.c
        C = len(modes)
        blks, tops, lefts, srcs = [], [], [], []
        sad = np.zeros((NB, C), np.uint64); ssd_c = np.zeros((NB, C), np.uint64); ssd_a = np.zeros((NB, C), np.uint64)
        for i in range(NB):
            blk, top, left, src = block_case(rng, s, i)
            blks.append(blk); tops.append(top); lefts.append(left); srcs.append(src)
            for c in range(C):
                pred = np.zeros((h, 64), np.uint8)          # row stride 64: samples past the block stay defined for the wide kernels
                R.ref_build_intra_predictors(0, ctypes.c_void_p(top.ctypes.data + 16), ctypes.c_void_p(left.ctypes.data + 16), ptr(pred), 64,
                                             int(modes[c]), int(deltas[c]), s, int(blk[3]), int(blk[4]), int(blk[5]), int(blk[6]), int(blk[7]),
                                             int(blk[2]), 8)
                v = R.fast_loop_nx_m_sad_kernel(ptr(src), w, ptr(pred), 64, h, w)
                assert avx2_sad[w](ptr(src), w, ptr(pred), 64, h, w) == v, (s, i, c)
                assert v == int(np.abs(src.astype(np.int64) - pred[:, :w]).sum()), (s, i, c)
                sad[i, c] = v
                ssd_c[i, c] = R.spatial_full_distortion_kernel(ptr(src), w, ptr(pred), 64, w, h)
                if w == h:
                    fn = ssd_tab.get(w, R.spatial_full_distortion_kernel16_mx_n_ssse3_intrin)
                    ssd_a[i, c] = fn(ptr(src), w, ptr(pred), 64, h, w)          # the call site's (bheight, bwidth)
        p = f"s{s}_"
        d[p + "modes"] = modes; d[p + "deltas"] = deltas
        d[p + "blk"] = np.array(blks); d[p + "top"] = np.array(tops); d[p + "left"] = np.array(lefts); d[p + "src"] = np.array(srcs)
        d[p + "sad"] = sad; d[p + "ssd_c"] = ssd_c
        if w == h:
            d[p + "ssd_avx2"] = ssd_a
    out = os.path.join(HERE, "fast_loop.npz")
    np.savez_compressed(out, **d)
    print(out, os.path.getsize(out), "bytes")


if __name__ == "__main__":
    main()

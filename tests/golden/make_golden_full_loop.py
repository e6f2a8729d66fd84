"""Golden vectors of the luma mode-decision full loop (ProductFullLoop / ProductFullLoopTxSearch, EbFullLoop.c:724-1100), from
the reference built as oracle/_ref/libsvtref.so.  Writes tests/golden/full_loop.npz (data only):

    python tests/golden/make_golden_full_loop.py

Per transform block, per transform type, 8-bit, the chain the reference runs:
  1. residual = src - pred                              ResidualKernel (EbProductCodingLoop.c:1969) - written here
  2. coeff, three_quad_energy = av1_estimate_transform  ref_estimate_transform (EbFullLoop.c:763, EbTransforms.c:4918)
  3. qcoeff, dqcoeff, eob = quantize                    aom_highbd_quantize_b{,_32x32,_64x64}_avx2 (production), y tables of
                                                        av1_build_quantizer, scans of ref_get_scan; count_non_zero = eob (:650)
  4. dist = picture_full_distortion32_bits             ref_picture_full_distortion32, asm_type 0 (C) and 1 (AVX2)
  5. dist[i] = RIGHT_SIGNED_SHIFT(dist[i] + three_quad_energy, (1 - av1_get_tx_scale) * 2)   (:829-835, :1062-1068) - written here

Layout, per size s (key prefix f"s{s}_"): types [T]; qindex [4]; src, pred uint8 [4 inputs, 2 blocks, H, W] (inputs: uniform
+-255 residual, small residual pred = src +- 3, zero residual, all-255 source on a zero prediction); dist_c, dist_avx2 uint64
[T, 4 q, 4 inputs, 2 blocks, 2]; eob uint16 [T, 4, 4, 2]; qcoeff, dqcoeff int32 [T, 4, 4, 2, min(W,32) * min(H,32)].
Every size draws from its own seed, so any subset of sizes regenerates on its own (tests/test_full_loop_cpu.py does)."""
import ctypes
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)
from make_golden import QNAMES, R, aligned  # noqa: E402
from svtlibs import TX_H, TX_W, ptr, txfm_allowed  # noqa: E402

c_int = ctypes.c_int
QINDEX = (0, 60, 160, 255)
INPUTS = ("uniform", "small", "zero", "extreme")
NBLK = 2
SEED = 13650


def y_tables():
    q = np.zeros((18, 256, 8), np.int16)
    dq = np.zeros((6, 256, 8), np.int16)
    R.av1_build_quantizer(c_int(8), 0, 0, 0, 0, 0, ptr(q), ptr(dq))      # y tables: Quants fields 0..3, Dequants 0
    return {"quant": q[0], "quant_shift": q[1], "zbin": q[2], "round": q[3], "dequant": dq[0]}


def inputs(rng, h, w):
    """src, pred uint8 [4, NBLK, h, w] for the four input kinds"""
    shp = (NBLK, h, w)
    r = rng.integers(-255, 256, size=shp)                       # uniform residual: pred uniform on the range that keeps src in 0..255
    lo, hi = np.maximum(0, -r), np.minimum(255, 255 - r)
    p_u = lo + (rng.random(shp) * (hi - lo + 1)).astype(np.int64)
    s_u = p_u + r
    s_s = rng.integers(0, 256, size=shp)                        # small: pred = src +- 3 (tests/test_gpu_fullsize.py's recipe, narrower)
    p_s = np.clip(s_s + rng.integers(-3, 4, size=shp), 0, 255)
    s_z = rng.integers(0, 256, size=shp)                        # zero residual: eob 0, the cbf_zero kernel
    src = np.stack([s_u, s_s, s_z, np.full(shp, 255)]).astype(np.uint8)
    pred = np.stack([p_u, p_s, s_z, np.zeros(shp, np.int64)]).astype(np.uint8)
    return src, pred


def chain(s, t, qrow, src, pred, scan, iscan):
    """one block through steps 1-5 -> (dist_c[2], dist_avx2[2], eob, qcoeff, dqcoeff)"""
    w, h = TX_W[s], TX_H[s]
    n = min(w, 32) * min(h, 32)
    pels = w * h
    ls = 2 if pels > 1024 else (1 if pels > 256 else 0)
    x = aligned((h, 64), np.int16)
    x[:, :w] = src.astype(np.int16) - pred.astype(np.int16)                 # 1. ResidualKernel
    co = aligned(w * h + 64, np.int32)
    e = np.zeros(1, np.uint64)
    assert R.ref_estimate_transform(ptr(x), ctypes.c_uint32(64), ptr(co), c_int(s), c_int(t), c_int(0), ptr(e)) == 0
    coeff = aligned(n + 64, np.int32); coeff[:n] = co[:n]
    qc = aligned(n + 64, np.int32); dqc = aligned(n + 64, np.int32)
    eob = np.zeros(1, np.uint16)
    getattr(R, QNAMES[ls][2])(ptr(coeff), ctypes.c_ssize_t(n), c_int(0), ptr(qrow["zbin"]), ptr(qrow["round"]), ptr(qrow["quant"]),
                              ptr(qrow["quant_shift"]), ptr(qc), ptr(dqc), ptr(qrow["dequant"]), ptr(eob), ptr(scan), ptr(iscan))
    dists = []
    for asm in (0, 1):
        y = np.zeros(2, np.uint64)
        assert R.ref_picture_full_distortion32(ptr(coeff), 0, ptr(dqc), 0, c_int(w), c_int(h), c_int(int(eob[0])), c_int(asm), ptr(y)) == 0
        y = y + e[0]                                                         # 5. + three_quad_energy, RIGHT_SIGNED_SHIFT
        sh = (1 - ls) * 2
        dists.append(y >> np.uint64(sh) if sh >= 0 else y << np.uint64(-sh))
    return dists[0], dists[1], eob[0], qc[:n].copy(), dqc[:n].copy()


def gen_size(s, tabs=None):
    tabs = tabs or y_tables()
    w, h = TX_W[s], TX_H[s]
    n = min(w, 32) * min(h, 32)
    rng = np.random.default_rng(SEED + s)
    types = np.array([t for t in range(16) if txfm_allowed(s, t)], np.uint8)
    src, pred = inputs(rng, h, w)
    T, Q, K = len(types), len(QINDEX), len(INPUTS)
    d = {"types": types, "qindex": np.array(QINDEX, np.int32), "src": src, "pred": pred,
         "dist_c": np.zeros((T, Q, K, NBLK, 2), np.uint64), "dist_avx2": np.zeros((T, Q, K, NBLK, 2), np.uint64),
         "eob": np.zeros((T, Q, K, NBLK), np.uint16), "qcoeff": np.zeros((T, Q, K, NBLK, n), np.int32),
         "dqcoeff": np.zeros((T, Q, K, NBLK, n), np.int32)}
    for ti, t in enumerate(types):
        scan = np.ctypeslib.as_array(R.ref_get_scan(s, int(t), 0), shape=(n,)).copy()
        iscan = np.ctypeslib.as_array(R.ref_get_scan(s, int(t), 1), shape=(n,)).copy()
        for qi, qx in enumerate(QINDEX):
            qrow = {k: np.ascontiguousarray(v[qx]) for k, v in tabs.items()}
            for k in range(K):
                for b in range(NBLK):
                    dc, da, eob, qc, dqc = chain(s, int(t), qrow, src[k, b], pred[k, b], scan, iscan)
                    d["dist_c"][ti, qi, k, b] = dc; d["dist_avx2"][ti, qi, k, b] = da; d["eob"][ti, qi, k, b] = eob
                    d["qcoeff"][ti, qi, k, b] = qc; d["dqcoeff"][ti, qi, k, b] = dqc
    return d


def generate(sizes=range(19)):
    tabs = y_tables()
    out = {}
    for s in sizes:
        for k, v in gen_size(s, tabs).items():
            out[f"s{s}_{k}"] = v
    return out


if __name__ == "__main__":
    path = os.path.join(HERE, "full_loop.npz")
    np.savez_compressed(path, **generate())
    print(path, os.path.getsize(path))

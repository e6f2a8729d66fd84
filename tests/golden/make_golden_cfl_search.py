"""Writes tests/golden/cfl_search.npz: the CfL alpha search of mode decision (CflPrediction / cfl_rd_pick_alpha / AV1CostCalcCfl,
EbProductCodingLoop.c:1395-1860) for the nine chroma sizes the reference can reach, 24 blocks each: the (block, plane, alpha) table of
svt_hip_cfl_search_frame and the records of svt_hip_cfl_decide_frame.

What is pinned to what.  Every LEAF of the table is the REFERENCE's own function in oracle/_ref/libsvtref.so through ctypes:
cfl_luma_subsampling_420_lbd_c, subtract_average_c, cfl_predict_lbd_c, ref_estimate_transform (av1_estimate_transform, DEFAULT_SHAPE),
aom_highbd_quantize_b_avx2 (the production quantiser) with the u / v rows of av1_build_quantizer called with non-zero chroma deltas,
ref_picture_full_distortion32 (asm 0 and 1) and av1_cost_coeffs_txb through make_golden_coeff_rate.RefCandidate (PLANE_TYPE_UV).  The
GLUE is this file's own, written out next to the line numbers it follows: ResidualKernel, the chroma shift (>> 2,
CuFullDistortionFastTuMode_R), cfl_idx_to_alpha (EbIntraPrediction.h:609-617), RDCOST (EbRateDistortionCost.h:73) and the walk of
cfl_rd_pick_alpha (:1587-1735) in ref_walk, the reference's nested loops in Python integers.

np_table / np_walk are the restatements tests use where the reference is not built (and compare with it where it is): numpy for the
AC, the prediction, the residual and the rate (make_golden_coeff_rate.np_cost_coeffs_txb), the project's CPU oracle
(oracle/libsvt_oracle.so, pinned to the reference by tests/test_oracle_vs_ref.py) for transform, quantiser and distortion; the walk
with its costs formed for all candidates at once in uint64 numpy.

One thing the walk does that its table does not say: AV1CostCalcCfl's "To check DC" test (cfl_alpha_idx 0 and cfl_alpha_signs 0,
:1436 / :1511) is also met by the walk's Cr, CFL_SIGN_NEG, c = 0 step, which the reference therefore costs at alpha_q3 0 (entry 0 of
the Cr table), not -1.  walk_entry() says so once for both walks.

CPU only; run from the repository root after build():  python tests/golden/make_golden_cfl_search.py
"""
import ctypes
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, HERE)
import make_golden_coeff_rate as mgc  # noqa: E402
import svtlibs  # noqa: E402
from svtlibs import TX_H, TX_W, ptr  # noqa: E402

OUT = os.path.join(HERE, "cfl_search.npz")
c_int = ctypes.c_int

SIZES = (0, 1, 2, 5, 6, 7, 8, 13, 14)                 # 4x4 8x8 16x16 4x8 8x4 8x16 16x8 4x16 16x4
NBLOCKS = 24
NALPHA = 33
DCT_DCT = 0
UV_DC_PRED, UV_CFL_PRED = 0, 13
CFL_SIGN_ZERO, CFL_SIGN_NEG, CFL_SIGN_POS, CFL_SIGNS = 0, 1, 2, 3
I64_MAX, U64 = (1 << 63) - 1, (1 << 64) - 1
# y_dc, u_dc, u_ac, v_dc, v_ac delta q: Cb rows differ from Cr rows (the DC entries of every row).  The AC deltas are EQUAL on purpose:
# av1_build_quantizer fills v_quant[q][2 .. 7] from u_quant[q][1] (EbModeDecisionConfigurationProcess.c:511), and the AVX2 quantiser
# reads those lanes for every coefficient from the third on, so with u_ac != v_ac the reference quantises Cr with Cb's AC multiplier
# and its own AVX2 and C quantisers disagree.  The library reads entries [0] and [1] of a row, as the C quantiser does; with equal AC
# deltas the reference's rows are the "ac repeated to SIMD width" its quantisers document and all three agree.  (Rows whose AC
# entries differ too are run against np_table in tests/test_gpu_cfl_search.py.)
CHROMA_DELTAS = (0, -6, 4, 9, 4)
QINDEX = 100                                           # one quantiser row set: the nine sizes are nine groups of ONE call
LAMBDAS = (4000, 6000, 9000, 12000, 15000, 20000, 28000, 38000, 50000)      # full_lambda per size, around that qindex's
KS = (0, 0, 1 / 8, -1 / 4, 1 / 2, -1, 3 / 2, -2, 2)
CFL_MODE_BITS, DC_MODE_BITS = 3000, 300
QKEYS = ("zbin", "round", "quant", "quant_shift", "dequant")
FLAT, CLIP0, CLIP255 = 0, 1, 2                        # blocks with a purpose
DEC_DTYPE = np.dtype([("best_rd", "<i8"), ("dc_rd", "<i8"), ("alpha_q3", "<i4", (2,)), ("uv_mode", "u1"), ("cfl_alpha_idx", "u1"),
                      ("cfl_alpha_signs", "u1"), ("pad", "u1", (5,))])
assert DEC_DTYPE.itemsize == 32


def alpha_of(a):
    """alpha_q3 of table entry a: 0; a = 1 + 16 * (sign - 1) + c -> -(c + 1) for CFL_SIGN_NEG, c + 1 for CFL_SIGN_POS"""
    return 0 if a == 0 else (-a if a <= 16 else a - 16)


def joint_sign(plane, a, b):
    """PLANE_SIGN_TO_JOINT_SIGN (:1574)"""
    return a * CFL_SIGNS + b - 1 if plane == 0 else b * CFL_SIGNS + a - 1


def idx_to_alpha(idx, js, plane):
    """cfl_idx_to_alpha (EbIntraPrediction.h:609-617) with CFL_SIGN_U / _V, CFL_IDX_U / _V (EbDefinitions.h:797-824)"""
    su = ((js + 1) * 11) >> 5
    sign = su if plane == 0 else (js + 1) - CFL_SIGNS * su
    if sign == CFL_SIGN_ZERO:
        return 0
    mag = (idx >> 4) if plane == 0 else (idx & 15)
    return mag + 1 if sign == CFL_SIGN_POS else -mag - 1


def walk_entry(plane, pn_sign, c):
    """the table entry AV1CostCalcCfl costs at the walk's (plane, pn_sign, c): cfl_alpha_idx (c << 4) + c under the joint sign of i = 0
    is alpha_q3 -/+ (c + 1) in this plane, except where idx and signs are both 0 (Cr, CFL_SIGN_NEG, c = 0): the DC check, alpha_q3 0"""
    if ((c << 4) + c) == 0 and joint_sign(plane, pn_sign, 0) == 0:
        return 0
    return 1 + 16 * (pn_sign - 1) + c


# ---------------------------------------------------------------------------------------------------------------------------
# inputs
# ---------------------------------------------------------------------------------------------------------------------------
def make_inputs(si):
    """-> dict of the size's synthetic inputs.  luma = base + one sinusoid of amplitude 4 .. 60 + noise +-3; chroma source = m + k x (luma
    AC) + noise +-2 with k drawn from KS, 40 % of the blocks with k = 0 in both planes; DC prediction flat at m +- 3; alpha rates uniform in
    200 .. 3000; mode bits 3000 (CfL) and 300 (DC); qindex QINDEX, lambda from LAMBDAS.  Three blocks with a purpose: FLAT (flat luma: all alphas
    tie), CLIP0 / CLIP255 (a prediction that clips at 0 / at 255)."""
    s = SIZES[si]
    w, h = TX_W[s], TX_H[s]
    rng = np.random.default_rng(4100 + s)
    n = NBLOCKS
    luma = np.zeros((n, 2 * h, 2 * w), np.uint8)
    src = np.zeros((n, 2, h, w), np.uint8)
    pred = np.zeros((n, 2, h, w), np.uint8)
    yy, xx = np.mgrid[0:2 * h, 0:2 * w]
    for b in range(n):
        amp = rng.uniform(4, 60)
        ang, per, ph = rng.uniform(0, np.pi), rng.uniform(6, 4 * max(w, h)), rng.uniform(0, 2 * np.pi)
        base = rng.uniform(70, 185)
        wave = amp * np.sin(2 * np.pi * (xx * np.cos(ang) + yy * np.sin(ang)) / per + ph)
        lum = base + wave + rng.integers(-3, 4, (2 * h, 2 * w))
        if b == FLAT:
            lum = np.full((2 * h, 2 * w), 131.0)
        luma[b] = np.clip(np.rint(lum), 0, 255)
        ds = luma[b].astype(np.float64).reshape(h, 2, w, 2).sum((1, 3)) / 4
        ac = ds - ds.mean()
        both_zero = rng.random() < 0.4
        for p in range(2):
            k = 0.0 if both_zero else KS[int(rng.integers(0, len(KS)))]
            m = rng.uniform(60, 190)
            if b == CLIP0:
                m, k = 4.0, 2.0
            if b == CLIP255:
                m, k = 251.0, -2.0
            src[b, p] = np.clip(np.rint(m + k * ac + rng.integers(-2, 3, (h, w))), 0, 255)
            pred[b, p] = int(np.clip(np.rint(m) + rng.integers(-3, 4), 0, 255))
    qx, lam = QINDEX, LAMBDAS[si]
    bb = np.arange(n)
    cc, ec = mgc.tables_of(s)
    return dict(size=np.int32(s), qindex=np.int32(qx), lam=np.uint32(lam), luma=luma, src=src, pred=pred,
                skip_ctx=np.stack([(bb + s) % 13, (bb + s + 7) % 13]).astype(np.uint8),
                dc_ctx=np.stack([(bb + 2 * s) % 3, (bb + 2 * s + 1) % 3]).astype(np.uint8),
                coeff_cost=cc, eob_cost=ec, alpha_rate=rng.integers(200, 3001, (8, 2, 16)).astype(np.int32),
                cfl_mode_bits=np.full(n, CFL_MODE_BITS, np.int32), dc_mode_bits=np.full(n, DC_MODE_BITS, np.int32))


def qrows_of(qrows, plane):
    """the fixture's int16 [2, 5, 8] rows -> dict for one plane"""
    return {k: np.ascontiguousarray(qrows[plane, i]) for i, k in enumerate(QKEYS)}


# ---------------------------------------------------------------------------------------------------------------------------
# numpy restatements
# ---------------------------------------------------------------------------------------------------------------------------
def np_ac(luma, w, h):
    """cfl_luma_subsampling_420_lbd_c + subtract_average(round_offset w * h / 2, num_pel_log2 log2(w * h)) -> int [h, w]"""
    q3 = luma.astype(np.int64).reshape(h, 2, w, 2).sum((1, 3)) << 1
    avg = (int(q3.sum()) + w * h // 2) >> ((w * h).bit_length() - 1)
    return (q3 - avg).astype(np.int16).astype(np.int64)


def np_predict(ac, dc, alpha):
    """cfl_predict_lbd_c: clip_pixel(ROUND_POWER_OF_TWO_SIGNED(alpha_q3 * ac, 6) + dc)"""
    q6 = alpha * ac
    mag = (np.abs(q6) + 32) >> 6
    return np.clip(dc.astype(np.int64) + np.where(q6 < 0, -mag, mag), 0, 255).astype(np.uint8)


def np_table(z):
    """svt_hip_cfl_search_frame for one size from the inputs z -> dict dist_c, dist_avx2 [n, 2, 33, 2] uint64, bits [n, 2, 33] uint64,
    eob [n, 2, 33] uint16"""
    O = svtlibs.oracle()
    s = int(z["size"])
    w, h = TX_W[s], TX_H[s]
    n = z["luma"].shape[0]
    scan = mgc.scan_of(s, DCT_DCT)
    out = dict(dist_c=np.zeros((n, 2, NALPHA, 2), np.uint64), dist_avx2=np.zeros((n, 2, NALPHA, 2), np.uint64),
               bits=np.zeros((n, 2, NALPHA), np.uint64), eob=np.zeros((n, 2, NALPHA), np.uint16))
    co, q, dq = (np.zeros(w * h, np.int32) for _ in range(3))
    eob, sad = np.zeros(1, np.uint16), np.zeros(1, np.uint32)
    for b in range(n):
        ac = np_ac(z["luma"][b], w, h)
        for p in range(2):
            row = qrows_of(z["qrows"], p)
            srcb = np.ascontiguousarray(z["src"][b, p])
            for a in range(NALPHA):
                pr = np.ascontiguousarray(np_predict(ac, z["pred"][b, p], alpha_of(a)))
                O.svt_oracle_fwd_quant_sad(ptr(srcb), w, ptr(pr), w, s, DCT_DCT, ptr(row["zbin"]), ptr(row["round"]), ptr(row["quant"]),
                                           ptr(row["quant_shift"]), ptr(row["dequant"]), ptr(co), ptr(q), ptr(dq), ptr(eob), ptr(sad))
                e = int(eob[0])
                for key, fn in (("dist_c", O.svt_oracle_full_distortion32), ("dist_avx2", O.svt_oracle_full_distortion32_avx2)):
                    y = np.zeros(2, np.uint64)
                    fn(ptr(co), w, ptr(dq if e else np.zeros_like(dq)), w, ptr(y), w, h)      # eob 0: the cbf-zero kernel, {sum c^2, sum c^2}
                    if e == 0:
                        y[0] = y[1]
                    out[key][b, p, a] = y >> np.uint64(2)
                out["eob"][b, p, a] = e
                out["bits"][b, p, a] = mgc.np_cost_coeffs_txb(q, e, s, DCT_DCT, int(z["skip_ctx"][p, b]), int(z["dc_ctx"][p, b]), z["coeff_cost"],
                                                              z["eob_cost"], scan) & U64
    return out


def np_rdcost(lam, r, d):
    """RDCOST in uint64 arithmetic that wraps, read as int64"""
    with np.errstate(over="ignore"):
        return (((np.asarray(r, np.uint64) * np.uint64(lam) + np.uint64(256)) >> np.uint64(9)) + np.asarray(d, np.uint64) * np.uint64(128)).view(np.int64)


def np_walk(dist, bits, alpha_rate, lam, cfl_bits, dc_bits):
    """svt_hip_cfl_decide_frame for one block.  dist [2, 33, 2], bits [2, 33] uint64 -> (record (DEC_DTYPE scalar), stops int [2, 2]: the
    c at which the walk of (plane, pn_sign - 1) ended, 16 when it completed)"""
    dist, bits = np.asarray(dist, np.uint64), np.asarray(bits, np.uint64)
    rate = np.asarray(alpha_rate, np.int64).astype(np.uint64)                       # int32 widened: sign-extended
    to_i = lambda v: int(np.asarray(v, np.uint64).view(np.int64)) if not isinstance(v, int) else ((v + (1 << 63)) % (1 << 64)) - (1 << 63)
    mode_rd = int(np_rdcost(lam, np.uint64(np.int64(cfl_bits)), 0))
    best_rd, best_js = I64_MAX, -1
    rd_uv = np.full((8, 2), I64_MAX, np.int64)
    best_c = np.zeros((8, 2), np.int64)
    for plane in range(2):
        for i in (CFL_SIGN_NEG, CFL_SIGN_POS):
            js = joint_sign(plane, CFL_SIGN_ZERO, i)
            with np.errstate(over="ignore"):
                rd_uv[js, plane] = np_rdcost(lam, bits[plane, 0] + rate[js, plane, 0], dist[plane, 0, 0])
    stops = np.full((2, 2), 16, np.int64)
    for plane in range(2):
        for pn in (CFL_SIGN_NEG, CFL_SIGN_POS):
            ents = np.array([walk_entry(plane, pn, c) for c in range(16)])
            jss = [joint_sign(plane, pn, i) for i in range(CFL_SIGNS)]
            with np.errstate(over="ignore"):
                rd = np.stack([np_rdcost(lam, bits[plane, ents] + rate[js, plane], dist[plane, ents, 0]) for js in jss])      # [3, 16]
            progress = 0
            for c in range(16):
                if c > 2 and progress < c:
                    stops[plane, pn - 1] = c
                    break
                flag = 0
                for i, js in enumerate(jss):
                    this = int(rd[i, c])
                    if this >= rd_uv[js, plane]:
                        continue
                    rd_uv[js, plane], best_c[js, plane], flag = this, c, 2
                    if rd_uv[js, 1 - plane] == I64_MAX:
                        continue
                    this = to_i(this + mode_rd + int(rd_uv[js, 1 - plane]))
                    if this >= best_rd:
                        continue
                    best_rd, best_js = this, js
                progress += flag
    with np.errstate(over="ignore"):
        dc_rd = to_i(int(np_rdcost(lam, bits[0, 0] + bits[1, 0], dist[0, 0, 0] + dist[1, 0, 0])) + int(np_rdcost(lam, np.uint64(np.int64(dc_bits)), 0)))
    rec = np.zeros((), DEC_DTYPE)
    rec["best_rd"], rec["dc_rd"] = best_rd, dc_rd
    if not dc_rd <= best_rd:
        ind = 0
        if best_js >= 0:
            ind = (int(best_c[best_js, 0]) << 4) + int(best_c[best_js, 1])
        else:
            best_js = 0
        rec["uv_mode"], rec["cfl_alpha_idx"], rec["cfl_alpha_signs"] = UV_CFL_PRED, ind, best_js
        rec["alpha_q3"] = (idx_to_alpha(ind, best_js, 0), idx_to_alpha(ind, best_js, 1))
    return rec, stops


def np_decide(z, dist):
    """every block of a size -> (DEC_DTYPE [n], stops [n, 2, 2])"""
    n = dist.shape[0]
    dec, stops = np.zeros(n, DEC_DTYPE), np.zeros((n, 2, 2), np.int64)
    for b in range(n):
        dec[b], stops[b] = np_walk(dist[b], z["bits"][b], z["alpha_rate"], int(z["lam"]), int(z["cfl_mode_bits"][b]), int(z["dc_mode_bits"][b]))
    return dec, stops


# ---------------------------------------------------------------------------------------------------------------------------
# the reference
# ---------------------------------------------------------------------------------------------------------------------------
def ref_lib():
    """libsvtref.so ready for the whole chain, None when it is not built.  The ref_* pin functions refill the dispatch globals on first
    use; make_golden_coeff_rate.ref_lib (svtlibs.ref_with_slots) has that refill run before it points av1_txb_init_levels and
    av1_get_nz_map_contexts, and points them on every call, so av1_cost_coeffs_txb never jumps through NULL."""
    return mgc.ref_lib()


def ref_qrows(L, qindex):
    """-> int16 [2 planes, 5 (QKEYS), 8]: the u / v rows of av1_build_quantizer with CHROMA_DELTAS (Quants fields 10 .. 17: u_quant,
    v_quant, u_quant_shift, v_quant_shift, u_zbin, v_zbin, u_round, v_round; Dequants 1 and 2)"""
    q = np.zeros((18, 256, 8), np.int16)
    dq = np.zeros((6, 256, 8), np.int16)
    L.av1_build_quantizer(c_int(8), *[c_int(v) for v in CHROMA_DELTAS], ptr(q), ptr(dq))
    assert (q[10:18, :, 2:] == q[10:18, :, 1:2]).all() and (dq[1:3, :, 2:] == dq[1:3, :, 1:2]).all(), "rows are not [dc, ac x 7]: see CHROMA_DELTAS"
    return np.stack([np.stack([q[14 + p, qindex], q[16 + p, qindex], q[10 + p, qindex], q[12 + p, qindex], dq[1 + p, qindex]]) for p in range(2)])


def _aligned(shape, dt, al=64):
    n = int(np.prod(shape)); it = np.dtype(dt).itemsize
    raw = np.zeros(n * it + al, np.uint8)
    off = (-raw.ctypes.data) % al
    return raw[off:off + n * it].view(dt).reshape(shape)


def ref_table(L, z):
    """the table of one size by the reference's functions (AV1CostCalcCfl :1395-1572 per entry) -> as np_table"""
    s = int(z["size"])
    w, h = TX_W[s], TX_H[s]
    n = z["luma"].shape[0]
    nc = w * h
    scan = np.ctypeslib.as_array(L.ref_get_scan(s, DCT_DCT, 0), shape=(nc,)).copy()
    iscan = np.ctypeslib.as_array(L.ref_get_scan(s, DCT_DCT, 1), shape=(nc,)).copy()
    rc = mgc.RefCandidate()
    out = dict(dist_c=np.zeros((n, 2, NALPHA, 2), np.uint64), dist_avx2=np.zeros((n, 2, NALPHA, 2), np.uint64),
               bits=np.zeros((n, 2, NALPHA), np.uint64), eob=np.zeros((n, 2, NALPHA), np.uint16))
    for b in range(n):
        luma = np.ascontiguousarray(z["luma"][b])
        q3 = np.zeros((32, 32), np.int16)                                            # pred_buf_q3, CFL_BUF_LINE 32
        L.cfl_luma_subsampling_420_lbd_c(ptr(luma), c_int(2 * w), ptr(q3), c_int(2 * w), c_int(2 * h))             # :1774
        L.subtract_average_c(ptr(q3), c_int(w), c_int(h), c_int(w * h // 2), c_int((w * h).bit_length() - 1))     # :1784
        for p in range(2):
            row = qrows_of(z["qrows"], p)
            dc = np.ascontiguousarray(z["pred"][b, p])
            for a in range(NALPHA):
                pr = np.zeros((h, w), np.uint8)
                L.cfl_predict_lbd_c(ptr(q3), ptr(dc), c_int(w), ptr(pr), c_int(w), c_int(alpha_of(a)), c_int(8), c_int(w), c_int(h))   # :1442
                x = _aligned((h, 64), np.int16)
                x[:, :w] = z["src"][b, p].astype(np.int16) - pr.astype(np.int16)      # ResidualKernel :1455
                co = _aligned(nc + 64, np.int32)
                e = np.zeros(1, np.uint64)
                assert L.ref_estimate_transform(ptr(x), ctypes.c_uint32(64), ptr(co), c_int(s), c_int(DCT_DCT), c_int(0), ptr(e)) == 0      # FullLoop_R
                qc, dqc = _aligned(nc + 64, np.int32), _aligned(nc + 64, np.int32)
                eob = np.zeros(1, np.uint16)
                L.aom_highbd_quantize_b_avx2(ptr(co), ctypes.c_ssize_t(nc), c_int(0), ptr(row["zbin"]), ptr(row["round"]), ptr(row["quant"]),
                                             ptr(row["quant_shift"]), ptr(qc), ptr(dqc), ptr(row["dequant"]), ptr(eob), ptr(scan), ptr(iscan))
                ev = int(eob[0])
                for key, asm in (("dist_c", 0), ("dist_avx2", 1)):
                    y = np.zeros(2, np.uint64)
                    assert L.ref_picture_full_distortion32(ptr(co), 0, ptr(dqc), 0, c_int(w), c_int(h), c_int(ev), c_int(asm), ptr(y)) == 0
                    out[key][b, p, a] = y >> np.uint64(2)                            # chromaShift, CuFullDistortionFastTuMode_R
                out["eob"][b, p, a] = ev
                out["bits"][b, p, a] = mgc.ref_cost(L, rc, qc[:nc], ev, s, DCT_DCT, int(z["skip_ctx"][p, b]), int(z["dc_ctx"][p, b]),
                                                    z["coeff_cost"], z["eob_cost"]) & U64
    return out


def ref_walk(dist, bits, alpha_rate, lam, cfl_bits, dc_bits):
    """cfl_rd_pick_alpha (:1587-1735) as its nested loops, in Python integers.  dist [2, 33, 2], bits [2, 33] -> (best_rd, dc_rd, uv_mode,
    cfl_alpha_idx, cfl_alpha_signs, alpha_cb, alpha_cr)"""
    i64 = lambda v: ((v + (1 << 63)) & U64) - (1 << 63)
    u64 = lambda v: int(v) & U64
    rdcost = lambda r, d: i64((((u64(r) * lam & U64) + 256 & U64) >> 9) + (u64(d) * 128 & U64) & U64)      # :73, uint64, held as int64
    cost_calc = lambda plane, a: (int(dist[plane][a][0]), int(bits[plane][a]))           # AV1CostCalcCfl: (full_distortion[RESIDUAL], coeffBits)
    best_rd = I64_MAX
    mode_rd = rdcost(int(cfl_bits), 0)                                                    # :1591
    best_rd_uv = [[I64_MAX, I64_MAX] for _ in range(8)]
    best_c = [[0, 0] for _ in range(8)]
    for plane in range(2):                                                                # :1598
        for i in range(CFL_SIGN_NEG, CFL_SIGNS):
            js = joint_sign(plane, CFL_SIGN_ZERO, i)
            if i == CFL_SIGN_NEG:
                d, cb = cost_calc(plane, 0)                                               # idx 0; both joint signs leave this plane's alpha 0
            best_rd_uv[js][plane] = rdcost(cb + int(alpha_rate[js][plane][0]), d)         # :1631
    best_joint_sign = -1
    for plane in range(2):                                                                # :1638
        for pn_sign in range(CFL_SIGN_NEG, CFL_SIGNS):
            progress = 0
            for c in range(16):
                flag = 0
                if c > 2 and progress < c:
                    break
                for i in range(CFL_SIGNS):
                    js = joint_sign(plane, pn_sign, i)
                    if i == 0:
                        d, cb = cost_calc(plane, walk_entry(plane, pn_sign, c))           # :1649-1663
                    this_rd = rdcost(cb + int(alpha_rate[js][plane][c]), d)               # :1670
                    if this_rd >= best_rd_uv[js][plane]:
                        continue
                    best_rd_uv[js][plane] = this_rd
                    best_c[js][plane] = c
                    flag = 2
                    if best_rd_uv[js][1 - plane] == I64_MAX:
                        continue
                    this_rd = i64(this_rd + mode_rd + best_rd_uv[js][1 - plane])          # :1678
                    if this_rd >= best_rd:
                        continue
                    best_rd = this_rd
                    best_joint_sign = js
                progress += flag
    dc_mode_rd = rdcost(int(dc_bits), 0)                                                  # :1695
    dc_rd = i64(rdcost(int(bits[0][0]) + int(bits[1][0]), int(dist[0][0][0]) + int(dist[1][0][0])) + dc_mode_rd)      # :1699-1716
    if dc_rd <= best_rd:
        return best_rd, dc_rd, UV_DC_PRED, 0, 0, 0, 0
    ind = 0
    if best_joint_sign >= 0:
        ind = (best_c[best_joint_sign][0] << 4) + best_c[best_joint_sign][1]
    else:
        best_joint_sign = 0
    return best_rd, dc_rd, UV_CFL_PRED, ind, best_joint_sign, idx_to_alpha(ind, best_joint_sign, 0), idx_to_alpha(ind, best_joint_sign, 1)


# ---------------------------------------------------------------------------------------------------------------------------
# the fixture
# ---------------------------------------------------------------------------------------------------------------------------
def gen_size(si, L=None, qrows=None):
    """-> dict of one size's arrays: the inputs, the table (from the reference L or, without it, the restatement with the given qrows)
    and the decisions for both flavours"""
    z = make_inputs(si)
    z["qrows"] = ref_qrows(L, int(z["qindex"])) if L is not None else qrows
    z.update(ref_table(L, z) if L is not None else np_table(z))
    for fl in ("c", "avx2"):
        dec, _ = np_decide(z, z["dist_" + fl])
        z["decision_" + fl] = dec.view(np.uint8).reshape(-1, DEC_DTYPE.itemsize)
    return z


def decisions(z, si, flavour="avx2"):
    return z[f"s{si}_decision_{flavour}"].view(DEC_DTYPE).reshape(-1)


def size_view(z, si):
    """the keys of one size of the loaded fixture, without the prefix"""
    pre = f"s{si}_"
    return {k[len(pre):]: z[k] for k in (z.files if hasattr(z, "files") else z) if k.startswith(pre)}


def ac_rows_case(v, nblocks=6):
    """a size's first blocks with row sets whose AC entries differ between the planes, which the fixture does not hold (see CHROMA_DELTAS):
    the luma rows of qindex 70 for Cb and of qindex 140 for Cr, each {dc, ac x 7}, so that the reference's AVX2 quantiser, its C quantiser
    and the library read the same values.  -> the inputs as np_table / ref_table take them"""
    qt = svtlibs.quant_tables(8)
    blocks = np.arange(nblocks)
    z = {k: (v[k][blocks] if k in ("luma", "src", "pred") else (v[k][:, blocks] if k in ("skip_ctx", "dc_ctx") else v[k])) for k in v}
    z["qrows"] = np.stack([np.stack([qt[k][qx] for k in QKEYS]) for qx in (70, 140)])
    assert (z["qrows"][:, :, 2:] == z["qrows"][:, :, 1:2]).all() and not np.array_equal(z["qrows"][0, :, 1], z["qrows"][1, :, 1])
    return z


def check_conditions(z):
    """the fixture cannot miss the hard paths"""
    sizes, joint, modes = set(), set(), {UV_DC_PRED: 0, UV_CFL_PRED: 0}
    cut3 = completes = eob0 = eobn = clip0 = clip255 = flat = rows_differ = False
    total = 0
    for si in range(len(SIZES)):
        v = size_view(z, si)
        s = int(v["size"])
        w, h = TX_W[s], TX_H[s]
        sizes.add(s)
        rows_differ |= not np.array_equal(v["qrows"][0], v["qrows"][1])
        assert v["dist_c"].shape == v["dist_avx2"].shape == (NBLOCKS, 2, NALPHA, 2)
        eob0 |= bool((v["eob"] == 0).any()); eobn |= bool((v["eob"] > 0).any())
        dec, stops = np_decide(v, v["dist_avx2"])
        assert np.array_equal(dec, decisions(z, si))
        cut3 |= bool((stops == 3).any()); completes |= bool((stops == 16).any())
        for b in range(NBLOCKS):
            modes[int(dec["uv_mode"][b])] += 1
            total += 1
            if dec["uv_mode"][b] == UV_CFL_PRED:
                joint.add(int(dec["cfl_alpha_signs"][b]))
            ac = np_ac(v["luma"][b], w, h)
            for p in range(2):
                for a in (16, 32):
                    raw = v["pred"][b, p].astype(np.int64) + np.where(alpha_of(a) * ac < 0, -1, 1) * ((np.abs(alpha_of(a) * ac) + 32) >> 6)
                    clip0 |= bool((raw < 0).any()); clip255 |= bool((raw > 255).any())
            if not ac.any():
                flat = True
                for key in ("dist_c", "dist_avx2", "bits", "eob"):                      # all alphas tie
                    assert (v[key] == v[key][:, :, :1])[b].all(), (si, key)
    assert sizes == set(SIZES), sizes
    assert min(modes.values()) * 5 >= total, modes
    assert joint == set(range(8)), joint
    assert cut3 and completes and eob0 and eobn and clip0 and clip255 and flat and rows_differ, \
        (cut3, completes, eob0, eobn, clip0, clip255, flat, rows_differ)


def main():
    L = ref_lib()
    if L is None:
        raise SystemExit("oracle/_ref/libsvtref.so is not built")
    out = {}
    for si in range(len(SIZES)):
        z = gen_size(si, L)
        t = np_table(z)                                                                 # the restatement, on every case
        for k, v in t.items():
            assert np.array_equal(v, z[k]), (SIZES[si], k)
        dec = z["decision_avx2"].view(DEC_DTYPE).reshape(-1)
        print(f"size {SIZES[si]}: CfL wins {int((dec['uv_mode'] == UV_CFL_PRED).sum())} of {NBLOCKS}, eob 0 entries {int((z['eob'] == 0).sum())}")
        for k, v in z.items():
            out[f"s{si}_{k}"] = v
    check_conditions(out)
    np.savez_compressed(OUT, **out)
    print(f"wrote {OUT}: {os.path.getsize(OUT)} bytes")


if __name__ == "__main__":
    main()

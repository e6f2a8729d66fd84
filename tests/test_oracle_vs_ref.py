"""CPU: randomized cross-check of the oracle against the reference's own kernels
compiled from /root/reference (oracle/_ref/libsvtref.so).  Skipped where the
reference build is absent AND cannot be made; the golden-fixture tests still pin
the oracle there."""
import ctypes

import numpy as np
import pytest

import svtlibs
from svtlibs import TX_H, TX_SIZES, TX_TYPES, TX_W, ptr, txfm_allowed

c_int = ctypes.c_int
R = svtlibs.ref()
pytestmark = pytest.mark.skipif(R is None, reason="oracle/_ref/libsvtref.so not built (needs /root/reference)")

SQ = {0, 1, 2, 3, 4}
NO_EOB = {5, 6, 13, 14}


def ref_fwd_name(s, impl):
    w, h = TX_W[s], TX_H[s]
    if impl == "c":
        return f"Av1TransformTwoD_{w}x{h}_c" if w == h else f"av1_fwd_txfm2d_{w}x{h}_c"
    return "av1_fwd_txfm2d_4x4_sse4_1" if (w, h) == (4, 4) else f"av1_fwd_txfm2d_{w}x{h}_avx2"


@pytest.mark.parametrize("tx_size", range(19))
def test_fwd_txfm2d_vs_reference_c_and_avx2(tx_size):
    """FwdTxfm2dAsmTest.cc:74-166 procedure, oracle as third party"""
    O = svtlibs.oracle()
    w, h = TX_W[tx_size], TX_H[tx_size]
    rng = np.random.default_rng(tx_size)
    fc = getattr(R, ref_fwd_name(tx_size, "c"))
    fa = getattr(R, ref_fwd_name(tx_size, "avx2"), None)
    for t in range(16):
        if not txfm_allowed(tx_size, t):
            continue
        for bd in (8, 10):
            for _ in range(6):
                x = np.zeros((h, 64), np.int16)          # stride 64 as in the reference test; 32-B aligned rows
                x[:, :w] = rng.integers(-(1 << bd) + 1, 1 << bd, size=(h, w))
                o = np.zeros(w * h, np.int32); c = np.zeros(w * h + 16, np.int32)
                O.svt_oracle_fwd_txfm2d(ptr(x), ptr(o), ctypes.c_uint32(64), t, tx_size, bd)
                fc(ptr(x), ptr(c), ctypes.c_uint32(64), c_int(t), ctypes.c_uint8(bd))
                assert np.array_equal(o, c[:w * h]), (TX_SIZES[tx_size], TX_TYPES[t], bd)


@pytest.mark.parametrize("tx_size", range(19))
def test_inv_txfm2d_add_vs_reference(tx_size):
    O = svtlibs.oracle()
    w, h = TX_W[tx_size], TX_H[tx_size]
    kw, kh = min(w, 32), min(h, 32)
    f = getattr(R, f"av1_inv_txfm2d_add_{w}x{h}_c")
    rng = np.random.default_rng(50 + tx_size)
    for t in range(16):
        if not txfm_allowed(tx_size, t):
            continue
        for bd in (8, 10, 12):
            for mag in (bd + 5, bd + 8, 21):
                co = rng.integers(-(1 << mag), 1 << mag, size=kw * kh).astype(np.int32)
                d1 = rng.integers(0, 1 << bd, size=(h, 80)).astype(np.uint16)
                d2 = d1.copy()
                if tx_size in SQ:
                    f(ptr(co), ptr(d1), c_int(80), c_int(t), c_int(bd))
                elif tx_size in NO_EOB:
                    f(ptr(co), ptr(d1), c_int(80), c_int(t), c_int(tx_size), c_int(bd))
                else:
                    f(ptr(co), ptr(d1), c_int(80), c_int(t), c_int(tx_size), c_int(kw * kh), c_int(bd))
                O.svt_oracle_inv_txfm2d_add(ptr(co), ptr(d2), c_int(80), t, tx_size, bd)
                assert np.array_equal(d1, d2), (TX_SIZES[tx_size], TX_TYPES[t], bd, mag)


QNAMES = {0: ("aom_highbd_quantize_b_c", "aom_quantize_b_c_II", "aom_highbd_quantize_b_avx2"),
          1: ("aom_highbd_quantize_b_32x32_c", "aom_quantize_b_32x32_c_II", "aom_highbd_quantize_b_32x32_avx2"),
          2: ("aom_highbd_quantize_b_64x64_c", "aom_quantize_b_64x64_c_II", "aom_highbd_quantize_b_64x64_avx2")}


@pytest.mark.parametrize("bd", [8, 10])
def test_quantize_b_vs_reference_all_q(bd):
    """QuantAsmTest.cc:84-308: q sweep 0..255 (step 5 here), coefficients +-2^(7+bd)"""
    O = svtlibs.oracle()
    t = svtlibs.quant_tables(bd)
    rng = np.random.default_rng(bd)
    for s, ls in ((2, 0), (3, 1), (4, 2)):
        sc, isc = svtlibs.scan_tables(s, 0)
        n = len(sc)
        for q in list(range(0, 256, 5)) + [255]:
            co = rng.integers(-(1 << (7 + bd)), (1 << (7 + bd)) + 1, size=n).astype(np.int32)
            tabs = [np.ascontiguousarray(t[k][q]) for k in ("zbin", "round", "quant", "quant_shift", "dequant")]
            for variant, fn in ((0, QNAMES[ls][0]), (1, QNAMES[ls][1]), (0, QNAMES[ls][2])):
                a = [np.zeros(n, np.int32), np.zeros(n, np.int32), np.zeros(1, np.uint16)]
                b = [np.zeros(n, np.int32), np.zeros(n, np.int32), np.zeros(1, np.uint16)]
                getattr(R, fn)(ptr(co), ctypes.c_ssize_t(n), c_int(0), ptr(tabs[0]), ptr(tabs[1]), ptr(tabs[2]), ptr(tabs[3]),
                               ptr(a[0]), ptr(a[1]), ptr(tabs[4]), ptr(a[2]), ptr(sc), ptr(isc))
                O.svt_oracle_quantize_b(ptr(co), ctypes.c_ssize_t(n), 0, ptr(tabs[0]), ptr(tabs[1]), ptr(tabs[2]), ptr(tabs[3]),
                                        ptr(b[0]), ptr(b[1]), ptr(tabs[4]), ptr(b[2]), ptr(sc), ptr(isc), ls, variant)
                assert all(np.array_equal(x, y) for x, y in zip(a, b)), (fn, bd, q)


def test_headline_chain_vs_reference_avx2_threads():
    """oracle chain == the reference's production AVX2 call sequence (the CPU baseline harness)"""
    O = svtlibs.oracle()
    n = 300
    rng = np.random.default_rng(77)
    src = rng.integers(0, 256, size=(n, 32, 32), dtype=np.uint8)
    pred = rng.integers(0, 256, size=(n, 32, 32), dtype=np.uint8)
    qt = svtlibs.quant_tables(8)
    tabs = [np.ascontiguousarray(qt[k][100]) for k in ("zbin", "round", "quant", "quant_shift", "dequant")]
    for avx2 in (1, 0):
        co = np.zeros((n, 1024), np.int32); q = np.zeros((n, 1024), np.int32); dq = np.zeros((n, 1024), np.int32)
        eob = np.zeros(n, np.uint16); sad = np.zeros(n, np.uint32)
        R.ref_bench_fwd_quant_sad(ptr(src), ptr(pred), ctypes.c_size_t(n), 3, avx2, ptr(tabs[0]), ptr(tabs[1]), ptr(tabs[2]),
                                  ptr(tabs[3]), ptr(tabs[4]), ptr(co), ptr(q), ptr(dq), ptr(eob), ptr(sad))
        for i in range(0, n, 7):
            r = [np.zeros(1024, np.int32), np.zeros(1024, np.int32), np.zeros(1024, np.int32), np.zeros(1, np.uint16), np.zeros(1, np.uint32)]
            O.svt_oracle_fwd_quant_sad(ptr(src[i]), 32, ptr(pred[i]), 32, 3, 0, ptr(tabs[0]), ptr(tabs[1]), ptr(tabs[2]),
                                       ptr(tabs[3]), ptr(tabs[4]), ptr(r[0]), ptr(r[1]), ptr(r[2]), ptr(r[3]), ptr(r[4]))
            assert np.array_equal(co[i], r[0]) and np.array_equal(q[i], r[1]) and np.array_equal(dq[i], r[2])
            assert eob[i] == r[3][0] and sad[i] == r[4][0]


# ---- intra prediction: no reference unit test exists; pinned by the scalar C functions ----
INTRA_NAMES = ["dc", "v", "h", "smooth", "smooth_v", "smooth_h", "paeth", "dc_top", "dc_left", "dc_128"]


@pytest.mark.parametrize("tx_size", range(19))
def test_intra_nondirectional_vs_reference(tx_size):
    O = svtlibs.oracle()
    bw, bh = TX_W[tx_size], TX_H[tx_size]
    rng = np.random.default_rng(900 + tx_size)
    for mode, name in enumerate(INTRA_NAMES):
        for bd in (8, 10):
            for trial in range(3):
                if bd == 8:
                    nb_a = rng.integers(0, 256, size=16 + 2 * 64 + 16, dtype=np.uint8)
                    nb_l = rng.integers(0, 256, size=16 + 2 * 64 + 16, dtype=np.uint8)
                    d1 = np.zeros((bh, 80), np.uint8); d2 = d1.copy()
                    f = getattr(R, f"aom_{name}_predictor_{bw}x{bh}_c")
                    f(ptr(d1), ctypes.c_ssize_t(80), ctypes.c_void_p(nb_a.ctypes.data + 16), ctypes.c_void_p(nb_l.ctypes.data + 16))
                    O.svt_oracle_intra_pred(mode, ptr(d2), ctypes.c_ssize_t(80), bw, bh, ctypes.c_void_p(nb_a.ctypes.data + 16),
                                            ctypes.c_void_p(nb_l.ctypes.data + 16))
                else:
                    nb_a = rng.integers(0, 1 << bd, size=16 + 2 * 64 + 16).astype(np.uint16)
                    nb_l = rng.integers(0, 1 << bd, size=16 + 2 * 64 + 16).astype(np.uint16)
                    if trial == 1:
                        nb_a[:] = (1 << bd) - 1; nb_l[:] = (1 << bd) - 1
                    d1 = np.zeros((bh, 80), np.uint16); d2 = d1.copy()
                    f = getattr(R, f"aom_highbd_{name}_predictor_{bw}x{bh}_c")
                    f(ptr(d1), ctypes.c_ssize_t(80), ctypes.c_void_p(nb_a.ctypes.data + 32), ctypes.c_void_p(nb_l.ctypes.data + 32), c_int(bd))
                    O.svt_oracle_intra_pred_hbd(mode, ptr(d2), ctypes.c_ssize_t(80), bw, bh, ctypes.c_void_p(nb_a.ctypes.data + 32),
                                                ctypes.c_void_p(nb_l.ctypes.data + 32), bd)
                assert np.array_equal(d1, d2), (TX_SIZES[tx_size], name, bd)


DR_DERIV = {3: 1023, 6: 547, 9: 372, 14: 273, 17: 215, 20: 178, 23: 151, 26: 132, 29: 116, 32: 102, 36: 90, 39: 80,
            42: 71, 45: 64, 48: 57, 51: 51, 54: 45, 58: 40, 61: 35, 64: 31, 67: 27, 70: 23, 73: 19, 76: 15, 81: 11,
            84: 7, 87: 3}


def test_dr_intra_derivative_table():
    t = (ctypes.c_uint16 * 90).in_dll(R, "dr_intra_derivative")
    for k, v in DR_DERIV.items():
        assert t[k] == v


@pytest.mark.parametrize("tx_size", [0, 1, 2, 3, 4, 5, 8, 9, 13, 16, 17])
def test_directional_vs_reference(tx_size):
    O = svtlibs.oracle()
    bw, bh = TX_W[tx_size], TX_H[tx_size]
    rng = np.random.default_rng(1700 + tx_size)
    angles = sorted(DR_DERIV)
    for bd in (8, 10):
        dt = np.uint8 if bd == 8 else np.uint16
        es = 1 if bd == 8 else 2
        for zone in (1, 2, 3):
            for a in angles[::3] + [87]:
                for up in ((0, 0), (1, 1)) if bw + bh <= 16 else ((0, 0),):
                    nb_a = rng.integers(0, 1 << bd, size=16 + 300).astype(dt)
                    nb_l = rng.integers(0, 1 << bd, size=16 + 300).astype(dt)
                    dx = DR_DERIV[a] if zone in (1, 2) else 1
                    dy = DR_DERIV[a] if zone in (2, 3) else 1
                    if zone == 2:      # angle p in (90,180): dx = deriv[180-p], dy = deriv[p-90]
                        dy = DR_DERIV[90 - a]
                    ua, ul = up
                    pa = ctypes.c_void_p(nb_a.ctypes.data + 16 * es); pl = ctypes.c_void_p(nb_l.ctypes.data + 16 * es)
                    d1 = np.zeros((bh, 72), dt); d2 = d1.copy()
                    S = ctypes.c_ssize_t(72)
                    if bd == 8:
                        if zone == 1: R.av1_dr_prediction_z1_c(ptr(d1), S, bw, bh, pa, pl, ua, dx, dy)
                        elif zone == 2: R.av1_dr_prediction_z2_c(ptr(d1), S, bw, bh, pa, pl, ua, ul, dx, dy)
                        else: R.av1_dr_prediction_z3_c(ptr(d1), S, bw, bh, pa, pl, ul, dx, dy)
                        O.svt_oracle_dr_prediction(zone, ptr(d2), S, bw, bh, pa, pl, ua, ul, dx, dy)
                    else:
                        if zone == 1: R.av1_highbd_dr_prediction_z1_c(ptr(d1), S, bw, bh, pa, pl, ua, dx, dy, bd)
                        elif zone == 2: R.av1_highbd_dr_prediction_z2_c(ptr(d1), S, bw, bh, pa, pl, ua, ul, dx, dy, bd)
                        else: R.av1_highbd_dr_prediction_z3_c(ptr(d1), S, bw, bh, pa, pl, ul, dx, dy, bd)
                        O.svt_oracle_dr_prediction_hbd(zone, ptr(d2), S, bw, bh, pa, pl, ua, ul, dx, dy, bd)
                    assert np.array_equal(d1, d2), (TX_SIZES[tx_size], bd, zone, a, up)


def test_edge_filter_and_upsample_vs_reference():
    O = svtlibs.oracle()
    rng = np.random.default_rng(4242)
    for sz in (5, 9, 17, 33, 65, 129):
        for strength in (0, 1, 2, 3):
            e = rng.integers(0, 1024, size=sz).astype(np.uint16); e2 = e.copy()
            R.av1_filter_intra_edge_high_c(ptr(e), sz, strength)
            O.svt_oracle_filter_intra_edge_hbd(ptr(e2), sz, strength)
            assert np.array_equal(e, e2)
            e8 = rng.integers(0, 256, size=sz).astype(np.uint8); e82 = e8.copy()
            R.av1_filter_intra_edge_high_c_old(ptr(e8), sz, strength)   # the uint8 body (EbIntraPrediction.c:177)
            O.svt_oracle_filter_intra_edge(ptr(e82), sz, strength)
            assert np.array_equal(e8, e82)
    for sz in (4, 8, 16):
        b = rng.integers(0, 256, size=64).astype(np.uint8); b2 = b.copy()
        R.av1_upsample_intra_edge_c(ctypes.c_void_p(b.ctypes.data + 16), sz)
        O.svt_oracle_upsample_intra_edge(ctypes.c_void_p(b2.ctypes.data + 16), sz)
        assert np.array_equal(b, b2)
        h = rng.integers(0, 1024, size=64).astype(np.uint16); h2 = h.copy()
        R.av1_upsample_intra_edge_high_c(ctypes.c_void_p(h.ctypes.data + 32), sz, 10)
        O.svt_oracle_upsample_intra_edge_hbd(ctypes.c_void_p(h2.ctypes.data + 32), sz, 10)
        assert np.array_equal(h, h2)


# ---- round 2: the reference's own search drivers and caller-level functions (oracle/ref_me.c, oracle/ref_pins.c) ----
def aligned(shape, dt, al=64):
    n = int(np.prod(shape)); it = np.dtype(dt).itemsize
    raw = np.zeros(n * it + al, np.uint8)
    off = (-raw.ctypes.data) % al
    return raw[off:off + n * it].view(dt).reshape(shape)


def test_me_fullpel_search_vs_reference_randomized():
    """K6: FullPelSearch_LCU (8-search-point AVX2 / SSE4.1 kernels + single-point remainder) and the NSQ driver
    open_loop_me_fullpel_search_sblock, asm_type 0 and 1, against svt_oracle_me_sb_search_full (flavour = asm_type).
    Covers ties (coarse content), maximal SADs, negative origins, widths below / not a multiple of 8."""
    O = svtlibs.oracle()
    rng = np.random.default_rng(5)
    for trial in range(60):
        sw = int(rng.integers(1, 44)); sh = int(rng.integers(1, 8))
        xo = int(rng.integers(-40, 10)); yo = int(rng.integers(-20, 10))
        stride = 64 + sw + 16 + int(rng.integers(0, 9))
        src = rng.integers(0, 256, (64, 64), dtype=np.uint8)
        win = rng.integers(0, 256, (64 + sh + 8, stride), dtype=np.uint8)
        if trial % 4 == 0:
            win[:] = (win >> 6) << 6; src[:] = (src >> 6) << 6
        if trial % 4 == 1:
            win[:] = (win >> 7) << 7; src[:] = (src >> 7) << 7
        if trial % 7 == 0:
            win[:] = 255; src[:] = 0
        wp = ctypes.c_void_p(win.ctypes.data + 4 * stride + 8)
        for nsq in (0, 1):
            for asm in (0, 1):
                ms = np.full(209, 128 * 128 * 255, np.uint32); mm = np.zeros(209, np.uint32)
                O.svt_oracle_me_sb_search_full(ptr(src), 64, wp, stride, sw, sh, xo, yo, asm, nsq, ptr(ms), ptr(mm))
                rs = np.zeros(209, np.uint32); rm = np.zeros(209, np.uint32)
                assert R.ref_me_fullpel(ptr(src), 64, wp, stride, xo, yo, sw, sh, asm, nsq, 1, ptr(rs), ptr(rm)) == 0
                k = 209 if nsq else 85
                assert np.array_equal(rs[:k], ms[:k]) and np.array_equal(rm[:k], mm[:k]), (trial, asm, nsq, sw, sh, xo, yo)


def test_estimate_transform_vs_reference_all_sizes():
    """a5: av1_estimate_transform (RTCD forward transform + HandleTransform64x64_c & co) for every size / allowed type"""
    O = svtlibs.oracle()
    rng = np.random.default_rng(11)
    for s in range(19):
        w, h = TX_W[s], TX_H[s]
        for t in range(16):
            if not txfm_allowed(s, t):
                continue
            for bi in (0, 1):
                bd = 10 if bi else 8
                x = aligned((h, 64), np.int16); x[:, :w] = rng.integers(-(1 << bd) + 1, 1 << bd, size=(h, w))
                co = aligned(w * h + 64, np.int32); e = np.zeros(1, np.uint64)
                assert R.ref_estimate_transform(ptr(x), ctypes.c_uint32(64), ptr(co), c_int(s), c_int(t), c_int(bi), ptr(e)) == 0
                o = np.zeros(w * h, np.int32)
                O.svt_oracle_fwd_txfm2d(ptr(x), ptr(o), ctypes.c_uint32(64), t, s, bd)
                oe = O.svt_oracle_fwd_txfm2d_pack64(ptr(o), s)
                n = min(w, 32) * min(h, 32)
                assert np.array_equal(co[:n], o[:n]) and int(e[0]) == int(oe), (TX_SIZES[s], TX_TYPES[t], bd)


def test_inv_txfm_add_u8_entry_vs_reference():
    """a6: the 8-bit reconstruction entry, C (av1_inv_txfm_add_c), production (av1_inv_txfm_add_ssse3) and the caller
    av1_inv_transform_recon8bit, on transform-consistent coefficients (InvTxfm2dAsmTest's procedure: the SIMD inverse
    kernels the dispatch pointers select - also inside av1_inv_txfm_add_c - only promise equality with the C kernels
    there; arbitrary coefficients are covered for the C kernels by test_inv_txfm2d_add_vs_reference)."""
    O = svtlibs.oracle()
    rng = np.random.default_rng(12)
    for s in range(19):
        w, h = TX_W[s], TX_H[s]
        kw, kh = min(w, 32), min(h, 32)
        for t in range(16):
            if not txfm_allowed(s, t):
                continue
            for trial in range(2):
                x = aligned((h, 64), np.int16); x[:, :w] = rng.integers(-255, 256, size=(h, w))
                full = np.zeros(w * h, np.int32)
                O.svt_oracle_fwd_txfm2d(ptr(x), ptr(full), ctypes.c_uint32(64), t, s, 8)
                O.svt_oracle_fwd_txfm2d_pack64(ptr(full), s)
                co = aligned(kw * kh + 64, np.int32); co[:kw * kh] = full[:kw * kh]
                if trial == 1:
                    co[kw * kh // 4:kw * kh] = 0
                d0 = rng.integers(0, 256, size=(h, 96), dtype=np.uint8)
                exp = d0.copy()
                O.svt_oracle_inv_txfm2d_add_u8(ptr(co), ptr(exp), c_int(96), t, s)
                for which in (0, 1, 2):
                    d = aligned((h, 96), np.uint8); d[:] = d0
                    R.ref_inv_txfm_add_u8(ptr(co), ptr(d), c_int(96), c_int(t), c_int(s), c_int(kw * kh), c_int(which))
                    assert np.array_equal(d, exp), (TX_SIZES[s], TX_TYPES[t], trial, which)


def test_full_distortion32_vs_reference_c_and_avx2():
    """a12 coefficient domain: C kernels, and the AVX2 kernels incl. their carry-less residual accumulation"""
    O = svtlibs.oracle()
    rng = np.random.default_rng(13)
    U = ctypes.c_uint32
    for (w, h) in ((4, 4), (8, 8), (16, 16), (32, 32), (8, 16), (32, 8), (64, 64), (16, 64)):
        for mag in (8, 12, 15, 17, 20, 26):
            a = aligned((h, w + 16), np.int32); b = aligned((h, w + 24), np.int32)
            a[:] = rng.integers(-(1 << mag), 1 << mag, size=a.shape); b[:] = rng.integers(-(1 << mag), 1 << mag, size=b.shape)
            o = np.zeros(2, np.uint64); o2 = np.zeros(2, np.uint64)
            O.svt_oracle_full_distortion32(ptr(a), U(w + 16), ptr(b), U(w + 24), ptr(o), U(w), U(h))
            O.svt_oracle_full_distortion32_avx2(ptr(a), U(w + 16), ptr(b), U(w + 24), ptr(o2), U(w), U(h))
            r = np.zeros(2, np.uint64)
            R.full_distortion_kernel32_bits(ptr(a), U(w + 16), ptr(b), U(w + 24), ptr(r), U(w), U(h))
            assert np.array_equal(r, o), (w, h, mag)
            R.full_distortion_kernel32_bits_avx2(ptr(a), U(w + 16), ptr(b), U(w + 24), ptr(r), U(w), U(h))
            assert np.array_equal(r, o2), (w, h, mag, "avx2")
            for nm in ("full_distortion_kernel_cbf_zero32_bits", "full_distortion_kernel_cbf_zero32_bits_avx2"):
                getattr(R, nm)(ptr(a), U(w + 16), ptr(b), U(w + 24), ptr(r), U(w), U(h))
                assert r[0] == o[1] and r[1] == o[1], (w, h, mag, nm)


def test_sad_variants_vs_reference():
    """a9: combined_averaging_sad (C), aom_sadMxN_c / aom_sadMxNx4d_c for the 22 RTCD sizes, and the AVX2 twins where the
    reference has them - all plain SADs (x4d = four of them), pinned here so that the drop-ins have a checker"""
    O = svtlibs.oracle()
    rng = np.random.default_rng(21)
    R.combined_averaging_sad.restype = ctypes.c_uint32
    U = ctypes.c_uint32
    for (w, h) in ((4, 4), (8, 8), (16, 16), (24, 24), (32, 32), (48, 48), (64, 64), (8, 32), (64, 16)):
        s = rng.integers(0, 256, (h, w + 5), dtype=np.uint8); r1 = rng.integers(0, 256, (h, w + 9), dtype=np.uint8)
        r2 = rng.integers(0, 256, (h, w + 1), dtype=np.uint8)
        if w == 8:
            r1[:] = 255; r2[:] = 254; s[:] = 0
        got = R.combined_averaging_sad(ptr(s), U(w + 5), ptr(r1), U(w + 9), ptr(r2), U(w + 1), U(h), U(w))
        assert got == O.svt_oracle_sad_avg(ptr(s), U(w + 5), ptr(r1), U(w + 9), ptr(r2), U(w + 1), U(h), U(w)), (w, h)
    sizes = [(128, 128), (128, 64), (64, 128), (64, 64), (64, 32), (32, 64), (32, 32), (32, 16), (16, 32), (16, 16), (16, 8), (8, 16),
             (8, 8), (8, 4), (4, 8), (4, 4), (4, 16), (16, 4), (8, 32), (32, 8), (16, 64), (64, 16)]
    for (w, h) in sizes:
        s = rng.integers(0, 256, (h, w + 3), dtype=np.uint8)
        refs = [rng.integers(0, 256, (h, w + 7), dtype=np.uint8) for _ in range(4)]
        exp = [O.svt_oracle_sad(ptr(s), U(w + 3), ptr(r), U(w + 7), U(h), U(w)) for r in refs]
        f = getattr(R, f"aom_sad{w}x{h}_c"); f.restype = ctypes.c_uint32
        assert [f(ptr(s), c_int(w + 3), ptr(r), c_int(w + 7)) for r in refs] == exp, (w, h)
        arr = (ctypes.c_void_p * 4)(*[r.ctypes.data for r in refs])
        out = np.zeros(4, np.uint32)
        getattr(R, f"aom_sad{w}x{h}x4d_c")(ptr(s), c_int(w + 3), arr, c_int(w + 7), ptr(out))
        assert list(out) == exp, (w, h)
        fa = getattr(R, f"aom_sad{w}x{h}_avx2", None)
        if fa is not None and w >= 32:
            fa.restype = ctypes.c_uint32
            assert fa(ptr(s), c_int(w + 3), ptr(refs[0]), c_int(w + 7)) == exp[0], (w, h, "avx2")


def test_hme_levels_vs_reference_randomized():
    """n1: HmeLevel0 / 1 / 2 (the reference's own functions, oracle/ref_me.c) on random pictures, SB positions incl. all
    picture edges, partial SBs, search regions and multipliers, off-picture centres.  asm_type 1 is compared too except for
    4-sample-wide blocks (AVX2 width-4 SAD kernels return wrong sums: DESIGN.md)."""
    O = svtlibs.oracle()
    rng = np.random.default_rng(3)
    checked = 0
    for trial in range(160):
        level = int(rng.integers(0, 3))
        sbw = sbh = {0: 16, 1: 32, 2: 64}[level]
        if trial % 5 == 0:
            sbw = int(rng.choice({0: [4, 8, 12, 16], 1: [8, 16, 24, 32], 2: [16, 32, 40, 48, 56, 64]}[level]))
        if trial % 7 == 0:
            sbh = int(rng.choice({0: [4, 8, 16], 1: [8, 16, 32], 2: [16, 32, 64]}[level]))
        W = int(rng.integers(sbw + 8, 200)); H = int(rng.integers(sbh + 8, 150))
        pad = {0: 16, 1: 32, 2: 64}[level] + int(rng.integers(0, 20))
        stride = W + 2 * pad + int(rng.integers(0, 7))
        ref = rng.integers(0, 256, (H + 2 * pad, stride), dtype=np.uint8)
        srcp = rng.integers(0, 256, (H, W), dtype=np.uint8)
        if trial % 3 == 0:
            ref[:] = (ref >> 6) << 6; srcp[:] = (srcp >> 6) << 6
        ox = int(rng.integers(0, W - sbw + 1)); oy = int(rng.integers(0, H - sbh + 1))
        if trial % 4 == 0:
            ox = 0
        if trial % 4 == 1:
            ox = W - sbw; oy = H - sbh
        hw = rng.integers(4, 70, 2).astype(np.uint16); hh = rng.integers(2, 40, 2).astype(np.uint16)
        rw = int(rng.integers(0, 2)); rh = int(rng.integers(0, 2))
        mx = int(rng.choice([100, 100, 150, 200])); my = int(rng.choice([100, 100, 150]))
        xc = int(rng.integers(-60, 60)); yc = int(rng.integers(-40, 40))
        p = svtlibs.hme_params(level, hw, hh, rw, rh, mx, my, pad, W, H)
        # reads must stay inside this test's buffer (the encoder's padding covers its own ranges): same arithmetic as the oracle
        saw, sah = p.search_area_width, p.search_area_height
        xo, yo = p.x_origin_offset + xc, p.y_origin_offset + yc
        xo = -p.pad_width - ox if ox + xo < -p.pad_width else xo
        xo = xo - ((ox + xo) - (W - 1)) if ox + xo > W - 1 else xo
        saw = max(1, saw - ((ox + xo + saw) - W)) if ox + xo + saw > W else saw
        yo = -p.pad_height - oy if oy + yo < -p.pad_height else yo
        yo = yo - ((oy + yo) - (H - 1)) if oy + yo > H - 1 else yo
        sah = max(1, sah - ((oy + yo + sah) - H)) if oy + yo + sah > H else sah
        if ox + xo < -pad or ox + xo + saw - 1 + sbw > W + pad or oy + yo < -pad or oy + yo + sah - 1 + sbh > H + pad:
            continue
        ob = np.zeros(1, np.uint64); oxv = np.zeros(1, np.int16); oyv = np.zeros(1, np.int16)
        O.svt_oracle_hme_level(ptr(srcp), W, ctypes.c_void_p(ref.ctypes.data + pad * stride + pad), stride, ox, oy, sbw, sbh, xc, yc, ctypes.byref(p),
                               ptr(ob), ptr(oxv), ptr(oyv))
        for asm in (0, 1):
            if asm == 1 and sbw == 4:
                continue
            rb = np.zeros(1, np.uint64); rx = np.zeros(1, np.int16); ry = np.zeros(1, np.int16)
            assert R.ref_hme_level(c_int(level), ptr(srcp), c_int(W), ptr(ref), c_int(stride), c_int(pad), c_int(pad), c_int(W), c_int(H), c_int(ox),
                                   c_int(oy), c_int(sbw), c_int(sbh), c_int(xc), c_int(yc), ptr(hw), ptr(hh), c_int(rw), c_int(rh), c_int(int(hw.sum())),
                                   c_int(int(hh.sum())), c_int(mx), c_int(my), c_int(asm), ptr(rb), ptr(rx), ptr(ry)) == 0
            assert (rb[0], rx[0], ry[0]) == (ob[0], oxv[0], oyv[0]), (trial, level, asm, sbw, sbh)
            checked += 1
    assert checked > 150


def test_has_top_right_bottom_left_vs_reference_tables():
    """the oracle replays the coding order; the reference looks it up in has_tr_* / has_bl_* bit tables
    (EbIntraPrediction.c:1435-1826).  Every block size x position in the superblock x partition x transform size x offset."""
    from svtlibs import BLOCK_W, BLOCK_H, partitions_for
    O = svtlibs.oracle()
    n = 0
    for sb_bsize, sb_mi in ((12, 16), (15, 32)):
        for bsize in range(22):
            if BLOCK_W[bsize] > sb_mi * 4 or BLOCK_H[bsize] > sb_mi * 4:
                continue
            bw, bh = BLOCK_W[bsize] // 4, BLOCK_H[bsize] // 4
            for part in partitions_for(bsize):
                for r in range(0, sb_mi, bh):
                    for c in range(0, sb_mi, bw):
                        for tx in range(19):
                            if TX_W[tx] > BLOCK_W[bsize] or TX_H[tx] > BLOCK_H[bsize]:
                                continue
                            if (r + c + tx + part) % 3:            # a third of the transform sizes per position keeps this in seconds
                                continue
                            for ss in (0, 1):
                                if ss and (BLOCK_W[bsize] < 8 or BLOCK_H[bsize] < 8):
                                    continue
                                tw, th = TX_W[tx] // 4, TX_H[tx] // 4
                                offs = [(0, 0)]
                                if tw < max(bw >> ss, 1):
                                    offs.append((0, tw))
                                if th < max(bh >> ss, 1):
                                    offs.append((th, 0))
                                for ro, co in offs:
                                    args = (bsize, 64 + r, 96 + c, 1, 1, part, tx, ro, co, ss, ss)
                                    assert R.ref_has_top_right(sb_bsize, *args) == O.svt_oracle_has_top_right(sb_mi, *args), args
                                    assert R.ref_has_bottom_left(sb_bsize, *args) == O.svt_oracle_has_bottom_left(sb_mi, *args), args
                                    n += 1
    assert n > 50000


def test_build_intra_predictors_vs_reference_randomized():
    """build_intra_predictors{,_high} (EbIntraPrediction.c:3667, 3857) through oracle/ref_intra.c: every mode, size, angle delta,
    availability pattern (none / full / partial counts), edge-filter type and switch, 8 and 10 bit"""
    from svtlibs import aligned_array
    O = svtlibs.oracle(); P = ptr
    rng = np.random.default_rng(9)
    seen = set()
    for trial in range(6000):
        s = int(rng.integers(0, 19)); w, h = TX_W[s], TX_H[s]
        mode = int(rng.integers(0, 13)); ad = int(rng.integers(-3, 4)) if 1 <= mode <= 8 else 0
        is16 = int(rng.integers(0, 2)); bd = 10 if is16 else 8
        dt = np.uint16 if is16 else np.uint8
        top = rng.integers(0, 1 << bd, 16 + 2 * 64 + 32).astype(dt); left = rng.integers(0, 1 << bd, 16 + 2 * 64 + 32).astype(dt)
        n_top = int(rng.choice([0, w])); n_left = int(rng.choice([0, h]))
        if trial % 5 == 0:
            n_top, n_left = w, h
        if trial % 7 == 0:
            n_top = int(rng.integers(1, w // 4 + 1)) * 4; n_left = int(rng.integers(1, h // 4 + 1)) * 4
        n_tr = int(rng.choice([0, h, int(rng.integers(0, h + 1))])) if n_top == w else 0      # :3974 asserts n_top_px == txwpx
        n_bl = int(rng.choice([0, w, int(rng.integers(0, w + 1))])) if n_left == h else 0
        dis = int(rng.integers(0, 4) == 0); ft = int(rng.integers(0, 2))
        es = 2 if is16 else 1
        tp = ctypes.c_void_p(top.ctypes.data + 16 * es); lp = ctypes.c_void_p(left.ctypes.data + 16 * es)
        d1 = aligned_array((h, 128), dt); d2 = aligned_array((h, 128), dt)
        R.ref_build_intra_predictors(is16, tp, lp, P(d1), 128, mode, ad, s, dis, n_top, n_tr, n_left, n_bl, ft, bd)
        O.svt_oracle_build_intra_predictors(is16, tp, lp, P(d2), 128, mode, ad, s, dis, n_top, n_tr, n_left, n_bl, ft, bd)
        assert np.array_equal(d1, d2), (TX_SIZES[s], mode, ad, is16, n_top, n_tr, n_left, n_bl, dis, ft)
        seen.add((s, mode))
    assert len(seen) == 19 * 13


def test_predict_intra_block_vs_reference_randomized():
    """av1_predict_intra_block / av1_predict_intra_block_16bit (EbIntraPrediction.c:4078, 4336) end to end: picture position ->
    availability -> sample counts -> edge preparation -> prediction, luma and chroma, picture and tile borders"""
    from svtlibs import intra_block_case, ref_predict_intra_block, oracle_predict_intra_block
    O = svtlibs.oracle()
    rng = np.random.default_rng(5)
    n = 0
    for trial in range(5000):
        c = intra_block_case(rng, trial)
        if c is None:
            continue
        got = ref_predict_intra_block(R, c)
        exp, out5 = oracle_predict_intra_block(O, c)
        assert np.array_equal(got, exp), ({k: v for k, v in c.items() if np.isscalar(v)}, out5)
        n += 1
    assert n > 3500


# ---- picture input: y4m header, padding, decimation ---------------------------------------------------
def test_y4m_header_vs_reference_application(tmp_path):
    """read_y4m_header / check_if_y4m / read_y4m_frame_delimiter of the reference's application on real files"""
    O = svtlibs.oracle()
    R.ref_y4m_header.restype = ctypes.c_long
    for i, (line, good) in enumerate(svtlibs.Y4M_HEADERS):
        path = str(tmp_path / f"h{i}.y4m")
        svtlibs.write_y4m(path, line, [(np.zeros(4, np.uint8),) * 3])
        out = np.zeros(8, np.int32)
        pos = R.ref_y4m_header(path.encode(), ptr(out))
        info = svtlibs.Y4mInfo()
        rc = O.svt_oracle_y4m_parse_header(line.encode(), ctypes.byref(info))
        assert out[0] == 1
        assert (rc == 0) == good == (out[1] == 0), (line, rc, out)
        if good:
            assert [info.width, info.height, info.fr_n, info.fr_d, info.bit_depth, info.interlaced] == out[2:8].tolist(), line
            assert pos == 9 + len(line) + 6        # signature + header line + "FRAME\n"
    # random headers: valid and damaged tokens in any order
    rng = np.random.default_rng(247)
    path = str(tmp_path / "r.y4m")
    for trial in range(300):
        line = svtlibs.random_y4m_header(rng)
        svtlibs.write_y4m(path, line, [(np.zeros(4, np.uint8),) * 3])
        out = np.zeros(8, np.int32)
        R.ref_y4m_header(path.encode(), ptr(out))
        info = svtlibs.Y4mInfo()
        rc = O.svt_oracle_y4m_parse_header(line.encode(), ctypes.byref(info))
        assert (rc == 0) == (out[1] == 0), (line, rc, out)
        if rc == 0:
            assert [info.width, info.height, info.fr_n, info.fr_d, info.bit_depth, info.interlaced] == out[2:8].tolist(), line
    # not a y4m file
    p = str(tmp_path / "raw.yuv")
    open(p, "wb").write(b"\x10" * 64)
    out = np.zeros(8, np.int32)
    R.ref_y4m_header(p.encode(), ptr(out))
    assert out[0] == 0


@pytest.mark.parametrize("is16", [0, 1])
def test_padding_and_decimation_vs_reference(is16):
    O = svtlibs.oracle()
    rng = np.random.default_rng(77 + is16)
    dt = np.uint16 if is16 else np.uint8
    for trial in range(40):
        w, h = int(rng.integers(1, 70)), int(rng.integers(1, 50))
        pw, ph = int(rng.integers(0, 20)), int(rng.integers(0, 12))
        stride = w + 2 * pw + int(rng.integers(0, 9))
        a = rng.integers(0, 1 << (10 if is16 else 8), (h + 2 * ph, stride)).astype(dt)
        b = a.copy()
        R.ref_generate_padding(ptr(a), stride, w, h, pw, ph, is16)
        O.svt_oracle_generate_padding(ptr(b), stride, w, h, pw, ph, 2 if is16 else 1)
        assert np.array_equal(a, b), (trial, w, h, pw, ph)
        # closed form the device kernel uses: every sample of the padded area = the nearest picture sample
        yy = np.clip(np.arange(h + 2 * ph) - ph, 0, h - 1)
        xx = np.clip(np.arange(w + 2 * pw) - pw, 0, w - 1)
        assert np.array_equal(a[:, :w + 2 * pw], a[ph:ph + h, pw:pw + w][np.ix_(yy, xx)])
    if is16:
        for trial in range(10):                            # un_pack8_bit_data: the 8-bit plane of a 10-bit picture
            w, h = int(rng.integers(1, 90)), int(rng.integers(1, 40))
            src = rng.integers(0, 1024, (h, w + 3)).astype(np.uint16)
            a = np.full((h, w + 5), 9, np.uint8); b = a.copy()
            R.ref_unpack8(ptr(src), w + 3, ptr(a), w + 5, w, h)
            O.svt_oracle_unpack8(ptr(src), w + 3, ptr(b), w + 5, w, h)
            assert np.array_equal(a, b) and np.array_equal(a[:, :w], (src[:, :w] >> 2).astype(np.uint8))
        return
    for trial in range(40):
        w, h = int(rng.integers(1, 70)), int(rng.integers(1, 50))
        pr, pb = int(rng.integers(0, 8)), int(rng.integers(0, 8))
        stride = w + pr + int(rng.integers(0, 5))
        a = rng.integers(0, 256, (h + pb, stride)).astype(np.uint8)
        b = a.copy()
        R.ref_pad_input_picture(ptr(a), stride, w, h, pr, pb)
        O.svt_oracle_pad_input_picture(ptr(b), stride, w, h, pr, pb, 1)
        assert np.array_equal(a, b)
        for step in (2, 4):
            ow, oh = (w + step - 1) // step, (h + step - 1) // step
            src = rng.integers(0, 256, (h, w + 3)).astype(np.uint8)
            d0 = np.full((oh, ow + 2), 7, np.uint8); d1 = d0.copy()
            R.ref_decimation_2d(ptr(src), w + 3, w, h, ptr(d0), ow + 2, step)
            O.svt_oracle_decimation_2d(ptr(src), w + 3, w, h, ptr(d1), ow + 2, step)
            assert np.array_equal(d0, d1)
            assert np.array_equal(d0[:, :ow], src[::step, :w:step])


@pytest.mark.parametrize("seed", [11, 12])
def test_motion_estimate_lcu_vs_reference_randomized(seed):
    """oracle/me_lcu.c against the reference's whole MotionEstimateLcu (oracle/ref_me.c) on random pictures, picture sizes with partial
    SBs, random parameter sets: slice type, 85 / 209 PUs, HME level switches, 1 x 1 / 2 x 2 regions, equal reference POCs (second-best
    region, base-layer list 1), search areas, CheckZeroZeroCenter on / off, bi-prediction gating, SAD sub-sampling.  asm_type 1 only
    on pictures of whole SBs: the AVX2 HME kernels are undefined on the 2- / 4-wide blocks of a partial SB (DESIGN 2 e)."""
    O = svtlibs.oracle()
    rng = np.random.default_rng(seed)
    ncase = nnarrow = 0
    for trial in range(14):
        W = int(rng.choice([200, 256, 328])); H = int(rng.choice([136, 192, 200]))
        base = svtlibs.smooth_picture(rng, H + 96, W + 96)
        dx0, dy0, dx1, dy1 = (int(v) for v in rng.integers(-20, 21, 4))
        src = base[48:48 + H, 48:48 + W].copy()
        ref0 = base[48 + dy0:48 + dy0 + H, 48 + dx0:48 + dx0 + W].copy() if trial % 4 else rng.integers(0, 256, (H, W), dtype=np.uint8)
        ref1 = base[48 + dy1:48 + dy1 + H, 48 + dx1:48 + dx1 + W].copy() if trial % 3 else rng.integers(0, 256, (H, W), dtype=np.uint8)
        (ps, geo), (p0, _), (p1, _) = svtlibs.me_pyramid(src), svtlibs.me_pyramid(ref0), svtlibs.me_pyramid(ref1)
        kw = dict(slice_type=int(rng.integers(0, 2)), pic_depth_mode=int(rng.choice([0, 2])), temporal_layer_index=int(rng.integers(0, 4)),
                  hme_l0=int(rng.integers(0, 2)), hme_l1=int(rng.integers(0, 2)), hme_l2=int(rng.integers(0, 2)),
                  enable_hme_flag=int(rng.integers(0, 4) > 0), is_used_as_reference_flag=int(rng.integers(0, 2)),
                  search_area_width=int(rng.choice([7, 8, 16, 24, 30])), search_area_height=int(rng.choice([5, 9, 16])),
                  regions_w=int(rng.choice([1, 2])), ref1_poc=int(rng.choice([8, 16])), asm_type=int(rng.integers(0, 2)) if W % 64 == 0 else 0,
                  cu8x8_mode=int(rng.integers(0, 2)), fractional_search_method=int(rng.choice([0, 1])))
        kw["regions_h"] = kw["regions_w"]
        for sy in range(0, H, 64):
            for sx in range(0, W, 64):
                prm = svtlibs.me_lcu_params(W, H, sx, sy, geo, **kw)
                a = svtlibs.run_me_lcu(R.ref_motion_estimate_lcu, prm, ps, p0, p1)
                bufs = (ctypes.c_void_p * 9)(*[p.ctypes.data for p in list(ps) + list(p0) + list(p1)])
                b = dict(best_sad=np.zeros((2, 209), np.uint32), best_mv=np.zeros((2, 209), np.uint32), area_origin=np.zeros((2, 2), np.int16),
                         bipred_sad=np.zeros(209, np.uint32), results=np.zeros((209, 11), np.int32))
                areas = np.zeros((2, 4), np.int16)
                assert O.svt_oracle_me_lcu_ex(ptr(prm), bufs, ptr(b["best_sad"]), ptr(b["best_mv"]), ptr(b["area_origin"]), ptr(b["bipred_sad"]),
                                              ptr(b["results"]), None, ptr(areas), None, None) == 0
                for k in a:
                    assert np.array_equal(a[k], b[k]), (trial, (W, H), (sx, sy), kw, k)
                ncase += 1
                nnarrow += int(0 < areas[0, 2] < 8) + int(0 < areas[1, 2] < 8)
    assert ncase > 150 and nnarrow > 0            # search areas clipped below 8 columns (the single-search-point form) did occur


def test_motion_estimate_lcu_vs_reference_on_the_picture_calls_draws():
    """the same comparison on svtlibs.me_frame_draws, the draws tests/test_gpu_me_frame.py sends through svt_hip_motion_estimate_frame:
    hierarchical_levels 0 .. 5 with every temporal layer (the 70 % .. 525 % level-0 multipliers), 1 x 2 / 2 x 1 region grids, unequal
    per-region HME areas at all three levels, every subset of the levels, 64-wide / 64-high search areas, 8-wide and 8-high partial
    SBs.  The chain reference -> oracle (here) -> picture call (there) needs no fixture."""
    svtlibs.me_frame_generator_coverage()
    ncase = nnarrow = 0
    for seed in svtlibs.ME_FRAME_SEEDS:
        for d, b in enumerate(svtlibs.me_frame_oracle_runs(seed)):
            for i, prm in enumerate(b["prm"]):
                a = svtlibs.run_me_lcu(R.ref_motion_estimate_lcu, prm, *b["pyr"])
                for k in a:
                    assert np.array_equal(a[k], b[k][i]), (seed, d, (b["W"], b["H"]), tuple(prm[2:4]), b["kw"], k, np.argwhere(a[k] != b[k][i])[:4].tolist())
                ncase += 1
                nnarrow += int(0 < b["areas"][i, 0, 2] < 8) + int(0 < b["areas"][i, 1, 2] < 8)
    assert ncase > 150 and nnarrow > 0
    svtlibs.me_frame_oracle_coverage()


@pytest.mark.parametrize("name", sorted(svtlibs.ME_FRAME_ACCEPTED_LIMITS))
def test_motion_estimate_lcu_vs_reference_on_the_largest_search_areas(name):
    """the two largest areas svt_hip_motion_estimate_frame accepts (svtlibs.ME_FRAME_ACCEPTED_LIMITS): the reference is defined there
    (every read stays inside the padded pictures) and the oracle equals it, so the GPU test may compare the picture call with the oracle"""
    b = svtlibs.me_frame_limit_run(name)
    for i, prm in enumerate(b["prm"]):
        a = svtlibs.run_me_lcu(R.ref_motion_estimate_lcu, prm, *b["pyr"])
        for k in a:
            assert np.array_equal(a[k], b[k][i]), (name, tuple(prm[2:4]), k, np.argwhere(a[k] != b[k][i])[:4].tolist())
    if name == "area_512x8":
        assert (b["areas"][:, :, 2] < 512).all() and (b["areas"][:, :, 2] >= 8).any()      # clipped by the picture's right side everywhere

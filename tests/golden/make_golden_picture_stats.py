"""Writes tests/golden/picture_stats.npz: GatheringPictureStatistics (EbPictureAnalysisProcess.c:4759-4812) on small pictures, what
svt_hip_picture_stats_frame must reproduce: the 85 luma block means / variances and the 21 Cb / Cr block means of every SB,
pic_avg_variance, the per-region histograms of the 1/16 luma and the chroma planes and the average intensities, for both
block_mean_calc_prec values.

What is pinned to what.  The LEAVES are the reference's own functions in oracle/_ref/libsvtref.so through ctypes:
compute_interm_var_four8x8_avx2_intrin (SUB luma mean and mean of squares, four 8x8 blocks per call, 32 bytes of rows 0, 2, 4, 6),
compute_mean8x8_avx2_intrin (FULL means, luma and chroma), CalculateHistogram, and ref_decimation_2d / ref_generate_padding
(Decimation2D, generate_padding) for the planes.  The GLUE is this file's own (ref_picture_stats), in Python integers next to the
line numbers it follows: the trees (:2843-2896, :1992-2007), the variance line (:2992-3082), is_complete_sb, the chroma zeroing
(:1706) and the chroma 64x64 line as the reference has it, (m32[0] + m32[1] + m32[3] + m32[3]) >> 2 (:2006-2007), the region
arithmetic (:4162-4191, :4222-4255) and the averages (:4746-4748, the lines of every scd_mode but SCD_MODE_0).

The two SSE2 leaves of ASM_SSE2/EbComputeMean_Intrinsic_SSE2.c are the reference's own as well, through oracle/ref_md.c's
ref_md_mean8x8: the SUB chroma mean compute_sub_mean8x8_sse2_intrin (:52-76: the sum of rows 0, 2, 4, 6, << 3) and the FULL mean of
squares compute_mean_of_squared_values8x8_sse2_intrin (:80-118: the sum of squares of all rows, << 10).  ref_picture_stats calls them
(ref_sub_mean8x8, ref_mean_sq8x8) and asserts the plain formulas sub_mean8x8 / mean_sq8x8, which np_picture_stats follows, equal to
them on every block it visits; check_sub_restatement does the same on random and extreme blocks.

np_picture_stats is the numpy restatement tests use where the reference is not built (and compare with it where it is).

CPU only; run from the repository root after build():  python tests/golden/make_golden_picture_stats.py
"""
import ctypes
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import svtlibs  # noqa: E402
from svtlibs import ptr  # noqa: E402

OUT = os.path.join(HERE, "picture_stats.npz")
PADS = (68, 34, 17)                           # origin of the luma, chroma and 1/16 pictures in their buffers, as the encoder's
FULL, SUB = 0, 1                              # BLOCK_MEAN_PREC_FULL / _SUB
# (width, height, regions per width, regions per height): 136x72 = 3x2 SBs of which two are complete, an 8-wide partial column and an
# 8-high partial row, a 34x18 1/16 picture (region remainders 2 and 2), odd chroma region origins; 192x128 all SBs complete; 64x64 one
# SB, with 4x4 regions of 4x4 1/16 samples and 2x2 chroma samples; 200x136 sides that 3 regions do not divide
CASES = ((136, 72, 4, 4), (192, 128, 2, 2), (64, 64, 1, 1), (64, 64, 4, 4), (200, 136, 3, 3))
CONTENTS = ("random", "all255", "checker1", "checker8", "oddrows", "gradient")
SB_KEYS = ("y_mean", "variance", "cb_mean", "cr_mean", "pic_avg_variance")             # depend on the precision
PIC_KEYS = ("histogram", "avg_region", "avg")                                           # do not


def make_frame(ci, content):
    """(y, cb, cr) of case ci.  random; all 255 (mean * mean overflows int32, variance 0); a 0 / 255 checkerboard at 1- and at 8-pixel
    pitch (the largest variances); odd rows that differ from the even rows (SUB and FULL must differ); a gradient with grain (the
    trees' >> 2 truncate)"""
    W, H = CASES[ci][:2]
    rng = np.random.default_rng([0x5053, ci, CONTENTS.index(content)])
    shapes = ((H, W), (H // 2, W // 2), (H // 2, W // 2))
    out = []
    for k, (h, w) in enumerate(shapes):
        yy, xx = np.mgrid[0:h, 0:w]
        if content == "random":
            p = rng.integers(0, 256, (h, w))
        elif content == "all255":
            p = np.full((h, w), 255)
        elif content == "checker1":
            p = ((xx + yy + k) & 1) * 255
        elif content == "checker8":
            p = (((xx >> 3) + (yy >> 3) + k) & 1) * 255
        elif content == "oddrows":
            p = np.where(yy & 1, 200 - 13 * k + (xx & 7), 40 + 9 * k + ((xx * 3) & 15))
        else:
            p = (xx * 255) // max(w - 1, 1) * 3 // 4 + (yy * 60) // max(h - 1, 1) + rng.integers(-3, 4, (h, w)) + 5 * k
        out.append(np.ascontiguousarray(np.clip(p, 0, 255).astype(np.uint8)))
    return tuple(out)


def np_planes(y, cb, cr):
    """the padded luma, Cb, Cr and 1/16 luma buffers (Decimation2D keeps every 4th sample of every 4th row, generate_padding
    replicates the edge), each with 5 spare columns of stride -> [(buffer, origin)]"""
    out = []
    for p, pad in ((y, PADS[0]), (cb, PADS[1]), (cr, PADS[1]), (np.ascontiguousarray(y[::4, ::4]), PADS[2])):
        h, w = p.shape
        buf = np.zeros((h + 2 * pad, w + 2 * pad + 5), np.uint8)
        buf[:, :w + 2 * pad] = np.pad(p, pad, mode="edge")
        out.append((buf, pad))
    return out


def ref_planes(R, y, cb, cr):
    """np_planes by the reference's own Decimation2D and generate_padding"""
    out = []
    H, W = y.shape
    for k, (p, pad) in enumerate(((y, PADS[0]), (cb, PADS[1]), (cr, PADS[1]), (None, PADS[2]))):
        h, w = (H // 4, W // 4) if k == 3 else p.shape
        stride = w + 2 * pad + 5
        buf = np.zeros((h + 2 * pad, stride), np.uint8)
        if k == 3:
            src = np.ascontiguousarray(y)
            R.ref_decimation_2d(ptr(src), W, W, H, ctypes.c_void_p(buf.ctypes.data + pad * stride + pad), stride, 4)
        else:
            buf[pad:pad + h, pad:pad + w] = p
        R.ref_generate_padding(ptr(buf), stride, w, h, pad, pad, 0)
        out.append((buf, pad))
    return out


# ---------------------------------------------------------------------------------------------------------------------------
# the two SSE2 leaves as plain formulas (what np_picture_stats follows), and the reference's own through oracle/ref_md.c
# ---------------------------------------------------------------------------------------------------------------------------
def sub_mean8x8(buf, y, x):
    """compute_sub_mean8x8_sse2_intrin (EbComputeMean_Intrinsic_SSE2.c:52-76)"""
    return int(buf[y:y + 8:2, x:x + 8].astype(np.int64).sum()) << 3


def mean_sq8x8(buf, y, x):
    """compute_mean_of_squared_values8x8_sse2_intrin (:80-118)"""
    b = buf[y:y + 8, x:x + 8].astype(np.int64)
    return int((b * b).sum()) << 10


def has_sse2_leaves(R):
    """False for a build of libsvtref.so from before the two leaves joined it (one that could not be remade: no reference sources)"""
    return R is not None and hasattr(R, "ref_md_mean8x8")


def ref_sub_mean8x8(R, buf, y, x):
    """the reference's leaf, asserted equal to the plain formula; the formula alone where the library has no such entry"""
    if not has_sse2_leaves(R):
        return sub_mean8x8(buf, y, x)
    v = int(R.ref_md_mean8x8(_at(buf, y, x), buf.strides[0], 0))
    assert v == sub_mean8x8(buf, y, x), (y, x)
    return v


def ref_mean_sq8x8(R, buf, y, x):
    if not has_sse2_leaves(R):
        return mean_sq8x8(buf, y, x)
    v = int(R.ref_md_mean8x8(_at(buf, y, x), buf.strides[0], 1))
    assert v == mean_sq8x8(buf, y, x), (y, x)
    return v


# ---------------------------------------------------------------------------------------------------------------------------
# the reference: its leaves, this file's glue
# ---------------------------------------------------------------------------------------------------------------------------
def ref_lib():
    R = svtlibs.ref()
    if R is None:
        return None
    R.compute_mean8x8_avx2_intrin.restype = ctypes.c_uint64
    R.compute_mean8x8_avx2_intrin.argtypes = [ctypes.c_void_p, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_uint32]
    R.compute_interm_var_four8x8_avx2_intrin.restype = None
    R.compute_interm_var_four8x8_avx2_intrin.argtypes = [ctypes.c_void_p, ctypes.c_uint16, ctypes.c_void_p, ctypes.c_void_p]
    R.CalculateHistogram.restype = None
    R.CalculateHistogram.argtypes = [ctypes.c_void_p, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_uint8, ctypes.c_void_p, ctypes.c_void_p]
    if has_sse2_leaves(R):
        R.ref_md_mean8x8.restype = ctypes.c_uint64
        R.ref_md_mean8x8.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_int]
    return R


def _at(buf, y, x):
    return ctypes.c_void_p(buf.ctypes.data + y * buf.strides[0] + x)


def tree(v8, n):
    """n x n leaves in raster order -> [64x64] + 32x32 + 16x16 + leaves as ME_TIER_ZERO_PU orders them; every level is
    (a + b + c + d) >> 2 of its four children (:2843-2896)"""
    levels = [list(v8)]
    while n > 1:
        prev, n = levels[-1], n // 2
        levels.append([(prev[2 * r * 2 * n + 2 * c] + prev[2 * r * 2 * n + 2 * c + 1] + prev[(2 * r + 1) * 2 * n + 2 * c] +
                        prev[(2 * r + 1) * 2 * n + 2 * c + 1]) >> 2 for r in range(n) for c in range(n)])
    return [v for lv in reversed(levels) for v in lv]


def region_sizes(side, regions):
    """(offset, size) of each region of one direction: side / regions each, the last takes the remainder (:4162-4179)"""
    r = side // regions
    return [(i * r, r + (side - regions * r if i == regions - 1 else 0)) for i in range(regions)]


def ref_picture_stats(R, y, cb, cr, prec, rw, rh):
    H, W = y.shape
    (luma, oy), (pcb, oc), (pcr, _), (six, o16) = ref_planes(R, y, cb, cr)
    ox = oy
    nsbx, nsby = (W + 63) // 64, (H + 63) // 64
    out = dict(y_mean=np.zeros((nsbx * nsby, 85), np.uint8), variance=np.zeros((nsbx * nsby, 85), np.uint16),
               cb_mean=np.zeros((nsbx * nsby, 21), np.uint8), cr_mean=np.zeros((nsbx * nsby, 21), np.uint8))
    m4, q4 = np.zeros(4, np.uint64), np.zeros(4, np.uint64)
    tot = 0
    for sb in range(nsbx * nsby):
        sx, sy = (sb % nsbx) * 64, (sb // nsbx) * 64
        mean, msq = [0] * 64, [0] * 64
        for by in range(8):                              # ComputeBlockMeanComputeVariance (:2066-2841)
            if prec == SUB:
                for half in range(2):
                    R.compute_interm_var_four8x8_avx2_intrin(_at(luma, oy + sy + 8 * by, ox + sx + 32 * half), luma.strides[0], ptr(m4), ptr(q4))
                    for k in range(4):
                        mean[by * 8 + 4 * half + k], msq[by * 8 + 4 * half + k] = int(m4[k]), int(q4[k])
            else:
                for bx in range(8):
                    mean[by * 8 + bx] = int(R.compute_mean8x8_avx2_intrin(_at(luma, oy + sy + 8 * by, ox + sx + 8 * bx), luma.strides[0], 8, 8))
                    msq[by * 8 + bx] = ref_mean_sq8x8(R, luma, oy + sy + 8 * by, ox + sx + 8 * bx)
        M, Q = tree(mean, 8), tree(msq, 8)
        for e in range(85):
            out["y_mean"][sb, e] = (M[e] >> 8) & 0xff                                    # MEAN_PRECISION (:2899-2989)
            out["variance"][sb, e] = (((Q[e] - M[e] * M[e]) & ((1 << 64) - 1)) >> 16) & 0xffff       # VARIANCE_PRECISION (:2992-3082)
        tot += int(out["variance"][sb, 0])                                               # :4686
        if sx + 64 <= W and sy + 64 <= H:                # is_complete_sb: ComputeChromaBlockMean (:1770-2058), else ZeroOutChromaBlockMean
            cy, cx = (oy + sy) >> 1, (ox + sx) >> 1      # :4658
            for name, pl in (("cb_mean", pcb), ("cr_mean", pcr)):
                if prec == SUB:
                    m16 = [ref_sub_mean8x8(R, pl, cy + 8 * r, cx + 8 * c) for r in range(4) for c in range(4)]
                else:
                    m16 = [int(R.compute_mean8x8_avx2_intrin(_at(pl, cy + 8 * r, cx + 8 * c), pl.strides[0], 8, 8)) for r in range(4) for c in range(4)]
                m32 = tree(m16, 4)[1:5]
                m64 = (m32[0] + m32[1] + m32[3] + m32[3]) >> 2                           # :2006-2007, as written
                out[name][sb] = [(v >> 8) & 0xff for v in [m64] + m32 + m16]
    out["pic_avg_variance"] = np.array([(tot // (nsbx * nsby)) & 0xffff], np.uint16)     # :4689
    hist = np.zeros((rw, rh, 3, 256), np.uint32)
    avg_region = np.zeros((rw, rh, 3), np.uint8)
    sums = [0, 0, 0]
    s64 = ctypes.c_uint64()
    for i, (x16, w16) in enumerate(region_sizes(W >> 2, rw)):                            # SubSampleLumaGeneratePixelIntensityHistogramBins
        for j, (y16, h16) in enumerate(region_sizes(H >> 2, rh)):
            hist[i, j, 0] = 1
            R.CalculateHistogram(_at(six, o16 + y16, o16 + x16), w16, h16, six.strides[0], 1, ptr(hist[i, j, 0]), ctypes.byref(s64))
            avg_region[i, j, 0] = ((s64.value + ((w16 * h16) >> 1)) // (w16 * h16)) & 0xff      # :4191
            sums[0] += s64.value << 4
            hist[i, j, 0] <<= 4
    for i, (xr, wr) in enumerate(region_sizes(W, rw)):                                   # SubSampleChromaGeneratePixelIntensityHistogramBins
        for j, (yr, hr) in enumerate(region_sizes(H, rh)):
            for p, pl in ((1, pcb), (2, pcr)):
                hist[i, j, p] = 1
                R.CalculateHistogram(_at(pl, (oy + yr) >> 1, (ox + xr) >> 1), wr >> 1, hr >> 1, pl.strides[0], 4, ptr(hist[i, j, p]), ctypes.byref(s64))
                s = s64.value << 4
                sums[p] += s
                avg_region[i, j, p] = ((s + ((wr * hr) >> 3)) // ((wr * hr) >> 2)) & 0xff         # :4255
                hist[i, j, p] <<= 4
    out["histogram"], out["avg_region"] = hist, avg_region
    out["avg"] = np.array([((sums[0] + ((W * H) >> 1)) // (W * H)) & 0xff, ((sums[1] + ((W * H) >> 3)) // ((W * H) >> 2)) & 0xff,
                           ((sums[2] + ((W * H) >> 3)) // ((W * H) >> 2)) & 0xff], np.uint8)      # :4746-4748
    return out


def check_sub_restatement(R, rng, n=2000):
    """sub_mean8x8 and mean_sq8x8 against the reference's two SSE2 leaves (ref_md_mean8x8) and against the lanes of
    compute_interm_var_four8x8_avx2_intrin, on random, all-255, all-0, 0 / 255 and near-flat blocks"""
    m4, q4 = np.zeros(4, np.uint64), np.zeros(4, np.uint64)
    for i in range(n):
        kind = i % 4
        a = (rng.integers(0, 256, (8, 40)) if kind == 0 else np.full((8, 40), 255) if kind == 1 else rng.integers(0, 2, (8, 40)) * 255 if kind == 2
             else 128 + rng.integers(-1, 2, (8, 40))).astype(np.uint8)
        R.compute_interm_var_four8x8_avx2_intrin(ptr(a), a.strides[0], ptr(m4), ptr(q4))
        for k in range(4):
            b = a[0:8:2, 8 * k:8 * k + 8].astype(np.int64)
            assert ref_sub_mean8x8(R, a, 0, 8 * k) == int(m4[k]) == int(b.sum()) << 3
            assert ref_mean_sq8x8(R, a, 0, 8 * k) == int((a[:, 8 * k:8 * k + 8].astype(np.int64) ** 2).sum()) << 10
            assert int(q4[k]) == int((b * b).sum()) << 11
            assert int(R.compute_mean8x8_avx2_intrin(_at(a, 0, 8 * k), a.strides[0], 8, 8)) == int(a[:, 8 * k:8 * k + 8].astype(np.int64).sum()) << 2


def check_sse2_leaves(R, rng, n=2000):
    """the plain formulas against the reference's two SSE2 leaves on n random 8x8 blocks (at a random offset of a wider buffer, so the
    stride counts) plus all-0 and all-255"""
    assert has_sse2_leaves(R), "libsvtref.so has no ref_md_mean8x8: rebuild it (make -C oracle ref)"
    blocks = [rng.integers(0, 256, (8, 24)).astype(np.uint8) for _ in range(n)] + [np.zeros((8, 24), np.uint8), np.full((8, 24), 255, np.uint8)]
    for i, a in enumerate(blocks):
        x = i % 17
        ref_sub_mean8x8(R, a, 0, x)
        ref_mean_sq8x8(R, a, 0, x)
    assert ref_sub_mean8x8(R, blocks[-1], 0, 0) == (255 * 32) << 3 and ref_mean_sq8x8(R, blocks[-1], 0, 0) == (255 * 255 * 64) << 10
    assert ref_sub_mean8x8(R, blocks[-2], 0, 0) == 0 and ref_mean_sq8x8(R, blocks[-2], 0, 0) == 0
    return len(blocks)


# ---------------------------------------------------------------------------------------------------------------------------
# the numpy restatement
# ---------------------------------------------------------------------------------------------------------------------------
def _np_tree(v):
    """v [..., n, n] uint64 leaves -> [..., 1 + 4 + ... + n * n] in ME_TIER_ZERO_PU order"""
    levels = [v]
    while levels[-1].shape[-1] > 1:
        p = levels[-1]
        levels.append((p[..., 0::2, 0::2] + p[..., 0::2, 1::2] + p[..., 1::2, 0::2] + p[..., 1::2, 1::2]) >> np.uint64(2))
    return np.concatenate([lv.reshape(lv.shape[:-2] + (-1,)) for lv in reversed(levels)], axis=-1)


def np_picture_stats(y, cb, cr, prec, rw, rh):
    """the same outputs from the unpadded planes of one picture, in numpy"""
    H, W = y.shape
    (luma, oy), (pcb, oc), (pcr, _), (six, o16) = np_planes(y, cb, cr)
    ox = oy
    nsbx, nsby = (W + 63) // 64, (H + 63) // 64
    rows = slice(0, 8, 2) if prec == SUB else slice(0, 8)
    msh, qsh = (3, 11) if prec == SUB else (2, 10)

    def leaves(pl, y0, x0, nby, nbx):
        b = pl[y0:y0 + 8 * nby, x0:x0 + 8 * nbx].astype(np.uint64).reshape(nby, 8, nbx, 8)[:, rows]
        return b.sum(axis=(1, 3)) << np.uint64(msh), (b * b).sum(axis=(1, 3)) << np.uint64(qsh)

    out = dict(y_mean=np.zeros((nsbx * nsby, 85), np.uint8), variance=np.zeros((nsbx * nsby, 85), np.uint16),
               cb_mean=np.zeros((nsbx * nsby, 21), np.uint8), cr_mean=np.zeros((nsbx * nsby, 21), np.uint8))
    for sb in range(nsbx * nsby):
        sx, sy = (sb % nsbx) * 64, (sb // nsbx) * 64
        m, q = leaves(luma, oy + sy, ox + sx, 8, 8)
        M, Q = _np_tree(m), _np_tree(q)
        out["y_mean"][sb] = (M >> np.uint64(8)).astype(np.uint8)
        out["variance"][sb] = ((Q - M * M) >> np.uint64(16)).astype(np.uint16)
        if sx + 64 <= W and sy + 64 <= H:
            for name, pl in (("cb_mean", pcb), ("cr_mean", pcr)):
                C = _np_tree(leaves(pl, (oy + sy) >> 1, (ox + sx) >> 1, 4, 4)[0])
                C[0] = (C[1] + C[2] + C[4] + C[4]) >> np.uint64(2)
                out[name][sb] = (C >> np.uint64(8)).astype(np.uint8)
    out["pic_avg_variance"] = np.array([int(out["variance"][:, 0].astype(np.int64).sum()) // (nsbx * nsby)], np.uint16)
    hist = np.zeros((rw, rh, 3, 256), np.uint32)
    avg_region = np.zeros((rw, rh, 3), np.uint8)
    sums = [0, 0, 0]
    for i in range(rw):
        for j in range(rh):
            (x16, w16), (y16, h16) = region_sizes(W >> 2, rw)[i], region_sizes(H >> 2, rh)[j]
            (xr, wr), (yr, hr) = region_sizes(W, rw)[i], region_sizes(H, rh)[j]
            for p, pl in enumerate((six, pcb, pcr)):
                if p == 0:
                    s = pl[o16 + y16:o16 + y16 + h16, o16 + x16:o16 + x16 + w16]
                else:
                    s = pl[(oy + yr) >> 1:((oy + yr) >> 1) + (hr >> 1):4, (ox + xr) >> 1:((ox + xr) >> 1) + (wr >> 1):4]
                hist[i, j, p] = (1 + np.bincount(s.ravel(), minlength=256)) << 4
                tot = int(s.astype(np.int64).sum())
                if p == 0:
                    avg_region[i, j, 0] = ((tot + ((w16 * h16) >> 1)) // (w16 * h16)) & 0xff
                else:
                    avg_region[i, j, p] = (((tot << 4) + ((wr * hr) >> 3)) // ((wr * hr) >> 2)) & 0xff
                sums[p] += tot << 4
    out["histogram"], out["avg_region"] = hist, avg_region
    out["avg"] = np.array([((sums[0] + ((W * H) >> 1)) // (W * H)) & 0xff, ((sums[1] + ((W * H) >> 3)) // ((W * H) >> 2)) & 0xff,
                           ((sums[2] + ((W * H) >> 3)) // ((W * H) >> 2)) & 0xff], np.uint8)
    return out


# ---------------------------------------------------------------------------------------------------------------------------
# the fixture
# ---------------------------------------------------------------------------------------------------------------------------
def case_key(ci, content, prec, key):
    return f"c{ci}_{content}_{key}" if key in PIC_KEYS else f"c{ci}_{content}_p{prec}_{key}"


def frame_of(g, ci, content):
    """(y, cb, cr) of a fixture case, from the packed frame the fixture holds"""
    W, H = CASES[ci][:2]
    f = g[f"c{ci}_{content}_frame"]
    return (f[:W * H].reshape(H, W), f[W * H:W * H * 5 // 4].reshape(H // 2, W // 2), f[W * H * 5 // 4:].reshape(H // 2, W // 2))


def generate(stats):
    """the whole fixture as a dict through stats(y, cb, cr, prec, rw, rh)"""
    z = {"cases": np.array(CASES, np.int32)}
    for ci, (W, H, rw, rh) in enumerate(CASES):
        for content in CONTENTS:
            y, cb, cr = make_frame(ci, content)
            z[f"c{ci}_{content}_frame"] = np.concatenate([y.ravel(), cb.ravel(), cr.ravel()])
            for prec in (FULL, SUB):
                o = stats(y, cb, cr, prec, rw, rh)
                for k in SB_KEYS + PIC_KEYS:
                    key = case_key(ci, content, prec, k)
                    assert key not in z or np.array_equal(z[key], o[k]), key            # the histograms do not depend on the precision
                    z[key] = o[k]
    return z


def check_conditions(g):
    """what the cases are there for, read from the fixture's outputs"""
    for ci, (W, H, rw, rh) in enumerate(CASES):
        nsbx, nsby = (W + 63) // 64, (H + 63) // 64
        complete = np.array([(sx + 1) * 64 <= W and (sy + 1) * 64 <= H for sy in range(nsby) for sx in range(nsbx)])
        for content in CONTENTS:
            for prec in (FULL, SUB):
                v = {k: g[case_key(ci, content, prec, k)] for k in SB_KEYS + PIC_KEYS}
                assert v["y_mean"].shape == (nsbx * nsby, 85) and v["cb_mean"].shape == (nsbx * nsby, 21) and v["histogram"].shape == (rw, rh, 3, 256)
                assert not v["cb_mean"][~complete].any() and not v["cr_mean"][~complete].any()
                assert (v["histogram"] >= 16).all() and not (v["histogram"] & 15).any()
                if content == "all255":
                    assert (v["y_mean"] == 255).all() and not v["variance"].any() and (v["cb_mean"][complete] == 255).all()
            if content == "checker8":
                assert int(g[case_key(ci, content, FULL, "variance")].max()) == 16256      # 0 / 255 in equal parts
            if content == "oddrows":
                assert not np.array_equal(g[case_key(ci, content, FULL, "y_mean")], g[case_key(ci, content, SUB, "y_mean")])
                if complete.any():
                    assert not np.array_equal(g[case_key(ci, content, FULL, "cb_mean")], g[case_key(ci, content, SUB, "cb_mean")])
    assert int(np.array(CASES)[0, 0]) % 64 == 8 and int(np.array(CASES)[0, 1]) % 64 == 8


def main():
    R = ref_lib()
    assert has_sse2_leaves(R), "oracle/_ref/libsvtref.so is not built, or is a build without oracle/ref_md.c"
    check_sub_restatement(R, np.random.default_rng(0x5054), 20000)
    check_sse2_leaves(R, np.random.default_rng(0x5055), 20000)
    z = generate(lambda *a: ref_picture_stats(R, *a))
    rest = generate(np_picture_stats)
    for k, v in z.items():
        assert v.dtype == rest[k].dtype and np.array_equal(v, rest[k]), k
    check_conditions(z)
    np.savez_compressed(OUT, **z)
    print(f"wrote {OUT}: {len(z)} arrays, {os.path.getsize(OUT)} bytes")


if __name__ == "__main__":
    main()

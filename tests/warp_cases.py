"""Warped motion restated in Python / numpy, for the fixture's generator and for the tests of svt_hip_warp_fit_frame and
svt_hip_warp_pred_frame: the local warp model of a block (warped_motion_parameters from the point where the samples exist:
select_samples, find_affine_int, get_shear_params) and the 8x8-tile warp filter (av1_warp_affine_c / av1_highbd_warp_affine_c as
warped_motion_prediction calls them: single reference, round_0 3, 11 bits of vertical rounding).  Scalar Python integers where the
reference's widths matter (wrap32 / wrap16 state every truncation), numpy per tile for the filter.  tests/golden/warp.npz pins both to
the compiled reference; the restatement draws nothing from the code under test."""
import ctypes
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
FIXTURE = os.path.join(HERE, "golden", "warp.npz")
REF_WARP = os.path.join(ROOT, "oracle", "_ref", "libsvtref_warp.so")

BSIZE_W = (4, 4, 8, 8, 8, 16, 16, 16, 32, 32, 32, 64, 64, 64, 128, 128, 4, 16, 8, 32, 16, 64)
BSIZE_H = (4, 8, 4, 8, 16, 8, 16, 32, 16, 32, 64, 32, 64, 128, 64, 128, 16, 4, 32, 8, 64, 16)
WARP_BSIZES = tuple(b for b in range(22) if BSIZE_W[b] >= 8 and BSIZE_H[b] >= 8 and BSIZE_W[b] <= 64 and BSIZE_H[b] <= 64)

PREC = 16                      # WARPEDMODEL_PREC_BITS
NDIAG_CLAMP = 1 << (PREC - 3)
TRANS_CLAMP = 128 << PREC
LS_MV_MAX = 256
MODEL_FIELDS = ("mat", "alpha", "beta", "gamma", "delta", "valid", "num_proj_ref")


def wrap32(v):
    return ((v + (1 << 31)) & 0xffffffff) - (1 << 31)


def wrap16(v):
    return ((v + (1 << 15)) & 0xffff) - (1 << 15)


def clamp(v, lo, hi):
    return lo if v < lo else (hi if v > hi else v)


def div_lut(i):
    """the divisor table of the AV1 specification (7.11.3.7), entry i of 257: 2^22 / (256 + i), rounded"""
    d = 256 + i
    return ((1 << 22) + d // 2) // d


def round_signed(v, n):
    """ROUND_POWER_OF_TWO_SIGNED[_64]"""
    half = (1 << n) >> 1
    return -((-v + half) >> n) if v < 0 else (v + half) >> n


def resolve_divisor(d):
    """resolve_divisor_32 / _64: 1 / d = y / 2^shift -> (y, shift)"""
    shift = d.bit_length() - 1
    e = d - (1 << shift)
    f = (e + ((1 << (shift - 8)) >> 1)) >> (shift - 8) if shift > 8 else e << (8 - shift)
    assert 0 <= f <= 256
    return div_lut(f), shift + 14


def select_samples(mv_x, mv_y, pts, pts_inref, n, bsize):
    """select_samples to the letter, the walk from both ends included; pts / pts_inref (lists) are permuted in place"""
    thresh = clamp(max(BSIZE_W[bsize], BSIZE_H[bsize]), 16, 112)
    mvd = [0] * 16
    ret = 0
    for i in range(n):
        mvd[i] = abs(pts_inref[2 * i] - pts[2 * i] - mv_x) + abs(pts_inref[2 * i + 1] - pts[2 * i + 1] - mv_y)
        if mvd[i] > thresh:
            mvd[i] = -1
        else:
            ret += 1
    if not ret:
        return 1
    i, j = 0, n - 1
    for _ in range(n - ret):
        while mvd[i] != -1:
            i += 1
        while mvd[j] == -1:
            j -= 1
        if i > j:
            break
        mvd[i] = mvd[j]
        pts[2 * i], pts[2 * i + 1] = pts[2 * j], pts[2 * j + 1]
        pts_inref[2 * i], pts_inref[2 * i + 1] = pts_inref[2 * j], pts_inref[2 * j + 1]
        i += 1
        j -= 1
    return ret


def _ls_square(a):
    return (a * a * 4 + a * 32 + 128) >> 4


def _ls_product1(a, b):
    return (a * b * 4 + (a + b) * 16 + 64) >> 4


def _ls_product2(a, b):
    return (a * b * 4 + (a + b) * 16 + 128) >> 4


def fit(nsamples, pts, pts_inref, bsize, mv_x, mv_y, x, y):
    """One (block, candidate): the model record as svt_hip_warp_fit_frame writes it (fields the reference did not reach are 0) and
    `info`, the branches taken (what the generator counts).  x, y: the block's luma origin; pts / pts_inref are not modified."""
    pts, pts_inref = [int(v) for v in pts], [int(v) for v in pts_inref]
    m = dict(mat=[0] * 6, alpha=0, beta=0, gamma=0, delta=0, valid=0, num_proj_ref=0)
    info = dict(selected=0, dropped=0, kept_none=0, mv_rejected=0, det0=0, shift_neg=0, diag_clamp=0, ndiag_clamp=0, trans_clamp=0,
                shear_refused=0, used=0)
    if nsamples == 0:
        return m, info
    n = nsamples
    if nsamples > 1:
        thresh = clamp(max(BSIZE_W[bsize], BSIZE_H[bsize]), 16, 112)
        kept = sum(1 for i in range(nsamples)
                   if abs(pts_inref[2 * i] - pts[2 * i] - mv_x) + abs(pts_inref[2 * i + 1] - pts[2 * i + 1] - mv_y) <= thresh)
        n = select_samples(mv_x, mv_y, pts, pts_inref, nsamples, bsize)
        info["selected"] = 1
        info["kept_none"] = int(n == 1 and kept == 0)
        info["dropped"] = int(n < nsamples and not info["kept_none"])
    m["num_proj_ref"] = n
    # ---- find_affine_int ----
    bw, bh = BSIZE_W[bsize], BSIZE_H[bsize]
    rsuy, rsux = bh // 2 - 1, bw // 2 - 1
    suy, sux = rsuy * 8, rsux * 8
    duy, dux = suy + mv_y, sux + mv_x
    isuy, isux = (y >> 2) * 4 + rsuy, (x >> 2) * 4 + rsux
    a00 = a01 = a11 = bx0 = bx1 = by0 = by1 = 0
    for i in range(n):
        dx, dy = pts_inref[2 * i] - dux, pts_inref[2 * i + 1] - duy
        sx, sy = pts[2 * i] - sux, pts[2 * i + 1] - suy
        if abs(sx - dx) < LS_MV_MAX and abs(sy - dy) < LS_MV_MAX:
            a00 += _ls_square(sx); a01 += _ls_product1(sx, sy); a11 += _ls_square(sy)
            bx0 += _ls_product2(sx, dx); bx1 += _ls_product1(sy, dx)
            by0 += _ls_product1(sx, dy); by1 += _ls_product2(sy, dy)
            info["used"] += 1
        else:
            info["mv_rejected"] = 1
    det = a00 * a11 - a01 * a01
    if det == 0:
        info["det0"] = 1
        return m, info
    lut, shift = resolve_divisor(abs(det))
    idet = lut * (-1 if det < 0 else 1)
    shift -= PREC
    if shift < 0:
        idet = wrap16(idet << -shift)          # int16_t iDet <<= -shift
        shift = 0
        info["shift_neg"] = 1
    px0, px1 = a11 * bx0 - a01 * bx1, -a01 * bx0 + a00 * bx1
    py0, py1 = a11 * by0 - a01 * by1, -a01 * by0 + a00 * by1

    def diag(p):
        v = round_signed(p * idet, shift)
        c = clamp(v, (1 << PREC) - NDIAG_CLAMP + 1, (1 << PREC) + NDIAG_CLAMP - 1)
        info["diag_clamp"] |= int(c != v)
        return c

    def ndiag(p):
        v = round_signed(p * idet, shift)
        c = clamp(v, -NDIAG_CLAMP + 1, NDIAG_CLAMP - 1)
        info["ndiag_clamp"] |= int(c != v)
        return c

    mat = m["mat"]
    mat[2], mat[3], mat[4], mat[5] = diag(px0), ndiag(px1), ndiag(py0), diag(py1)
    vx = wrap32(wrap32(mv_x * (1 << (PREC - 3))) - wrap32(wrap32(isux * (mat[2] - (1 << PREC))) + wrap32(isuy * mat[3])))
    vy = wrap32(wrap32(mv_y * (1 << (PREC - 3))) - wrap32(wrap32(isux * mat[4]) + wrap32(isuy * (mat[5] - (1 << PREC)))))
    mat[0], mat[1] = clamp(vx, -TRANS_CLAMP, TRANS_CLAMP - 1), clamp(vy, -TRANS_CLAMP, TRANS_CLAMP - 1)
    info["trans_clamp"] = int(mat[0] != vx or mat[1] != vy)
    # ---- get_shear_params ----
    if mat[2] <= 0:
        return m, info
    i16 = lambda v: clamp(v, -32768, 32767)
    alpha, beta = i16(mat[2] - (1 << PREC)), i16(mat[3])
    yv, sh = resolve_divisor(abs(mat[2]))
    gamma = i16(wrap32(round_signed(mat[4] * (1 << PREC) * yv, sh)))
    delta = i16(wrap32(wrap32(mat[5] - wrap32(round_signed(mat[3] * mat[4] * yv, sh))) - (1 << PREC)))
    red = lambda v: wrap16(round_signed(v, 6) * 64)
    m["alpha"], m["beta"], m["gamma"], m["delta"] = alpha, beta, gamma, delta = red(alpha), red(beta), red(gamma), red(delta)
    if 4 * abs(alpha) + 7 * abs(beta) >= (1 << PREC) or 4 * abs(gamma) + 4 * abs(delta) >= (1 << PREC):
        info["shear_refused"] = 1
        return m, info
    m["valid"] = 1
    return m, info


def fit_group(samples, blk, bsize):
    """samples: warp_samples records [nblocks]; blk: inter_blk records [nblocks][ncand] -> (model fields as arrays [nblocks][ncand],
    nvalid [nblocks])"""
    nb, nc = blk.shape
    out = dict(mat=np.zeros((nb, nc, 6), np.int32), alpha=np.zeros((nb, nc), np.int16), beta=np.zeros((nb, nc), np.int16),
               gamma=np.zeros((nb, nc), np.int16), delta=np.zeros((nb, nc), np.int16), valid=np.zeros((nb, nc), np.uint8),
               num_proj_ref=np.zeros((nb, nc), np.uint8))
    for b in range(nb):
        for c in range(nc):
            m, _ = fit(int(samples[b]["nsamples"]), samples[b]["pts"], samples[b]["pts_inref"], bsize, int(blk[b, c]["mv"][0][0]),
                       int(blk[b, c]["mv"][0][1]), int(blk[b, c]["x"]), int(blk[b, c]["y"]))
            for k in MODEL_FIELDS:
                out[k][b, c] = m[k]
    return out, out["valid"].sum(axis=1).astype(np.uint32)


_KH = np.arange(-7, 8)[:, None, None]
_L = np.arange(-4, 4)[None, :, None]
_M = np.arange(8)[None, None, :]
_KV = np.arange(-4, 4)[:, None, None]


def warp_pred(table, plane, bd, p_col, p_row, p_w, p_h, ss, mat, shear, cover=None):
    """The (p_w x p_h) block at (p_col, p_row) of a plane (numpy [height][width]) under the model: av1_warp_affine_c /
    av1_highbd_warp_affine_c with is_compound 0 and round_0 3.  table: warped_filter [193][8].  cover (dict of counters): tiles with a
    clamped row / column, tiles wholly outside, tiles that reach offs 0 / 64 / 192."""
    height, width = plane.shape
    ref = plane.astype(np.int64)
    tab = np.asarray(table, np.int64)
    alpha, beta, gamma, delta = (int(v) for v in shear)
    m = [int(v) for v in mat]
    out = np.zeros((p_h, p_w), np.int64)
    for i in range(p_row, p_row + p_h, 8):
        for j in range(p_col, p_col + p_w, 8):
            src_x, src_y = (j + 4) << ss, (i + 4) << ss
            dst_x = wrap32(wrap32(m[2] * src_x) + wrap32(m[3] * src_y) + m[0])
            dst_y = wrap32(wrap32(m[4] * src_x) + wrap32(m[5] * src_y) + m[1])
            x4, y4 = dst_x >> ss, dst_y >> ss
            ix4, sx4, iy4, sy4 = x4 >> 16, x4 & 0xffff, y4 >> 16, y4 & 0xffff
            sx4 = (sx4 - 4 * (alpha + beta)) & ~63
            sy4 = (sy4 - 4 * (gamma + delta)) & ~63
            rows = np.clip(iy4 + _KH, 0, height - 1)
            cols = np.clip(ix4 + _L - 3 + _M, 0, width - 1)
            offs_h = ((sx4 + beta * (_KH[:, :, 0] + 4) + alpha * (_L[:, :, 0] + 4) + 512) >> 10) + 64
            offs_v = ((sy4 + delta * (_KV[:, :, 0] + 4) + gamma * (_L[:, :, 0] + 4) + 512) >> 10) + 64
            if cover is not None:
                raw_r, raw_c = iy4 + np.arange(-7, 8), ix4 + np.arange(-7, 8)
                cover["row_clamped"] += int(((raw_r < 0) | (raw_r > height - 1)).any())
                cover["col_clamped"] += int(((raw_c < 0) | (raw_c > width - 1)).any())
                cover["outside_left"] += int(raw_c.max() < 0); cover["outside_right"] += int(raw_c.min() > width - 1)
                cover["outside_top"] += int(raw_r.max() < 0); cover["outside_bottom"] += int(raw_r.min() > height - 1)
                both = np.concatenate([offs_h.ravel(), offs_v.ravel()])
                assert both.min() >= 0 and both.max() <= 192, "a model outside is_affine_shear_allowed"
                cover["offs_0"] += int((both == 0).any()); cover["offs_64"] += int((both == 64).any()); cover["offs_192"] += int((both == 192).any())
            offs_h, offs_v = np.clip(offs_h, 0, 192), np.clip(offs_v, 0, 192)
            hsum = (ref[rows, cols] * tab[offs_h]).sum(axis=2) + (1 << (bd + 6))
            tmp = (hsum + 4) >> 3                                             # [15][8], 0 .. 2^(bd + 5) - 1
            assert tmp.min() >= 0 and tmp.max() < (1 << (bd + 5))
            vsum = (tmp[_KV + 4 + _M, _L + 4] * tab[offs_v]).sum(axis=2) + (1 << (bd + 11))
            v = ((vsum + 1024) >> 11) - (1 << (bd - 1)) - (1 << bd)
            if cover is not None:
                cover["clip_low"] += int((v < 0).any()); cover["clip_high"] += int((v > (1 << bd) - 1).any())
            out[i - p_row:i - p_row + 8, j - p_col:j - p_col + 8] = np.clip(v, 0, (1 << bd) - 1)
    return out.astype(np.uint8 if bd == 8 else np.uint16)


def distortion(pred, src, metric):
    """SVT_HIP_FAST_SAD (0) / SVT_HIP_FAST_SSD (1) of a block"""
    d = pred.astype(np.int64) - src.astype(np.int64)
    return int(np.abs(d).sum()) if metric == 0 else int((d * d).sum())


# ---- the compiled reference (oracle/_ref/libsvtref_warp.so, built by tests/golden/make_golden_warp.py) ----
def ref_lib():
    if not os.path.exists(REF_WARP):
        return None
    L = ctypes.CDLL(REF_WARP)
    L.ref_warp_table.argtypes = [ctypes.c_void_p]
    L.ref_warp_fit.argtypes = [ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p] + [ctypes.c_int] * 5 + [ctypes.c_void_p]
    L.ref_warp_pred.argtypes = [ctypes.c_int, ctypes.c_void_p] + [ctypes.c_int] * 3 + [ctypes.c_void_p] + [ctypes.c_int] * 6 + [ctypes.c_void_p] * 2
    for f in (L.ref_warp_table, L.ref_warp_fit, L.ref_warp_pred):
        f.restype = None
    L.ref_warp_shear.argtypes = [ctypes.c_void_p, ctypes.c_void_p]
    L.ref_warp_shear.restype = ctypes.c_int
    return L


PRED_COVER = ("row_clamped", "col_clamped", "outside_left", "outside_right", "outside_top", "outside_bottom", "offs_0", "offs_64", "offs_192",
              "clip_low", "clip_high")
FIT_COVER = ("valid", "nsamples_0", "nsamples_1", "dropped", "kept_none", "mv_rejected", "det0", "diag_clamp", "ndiag_clamp", "trans_clamp",
             "shear_refused", "used_8")


def ref_shear(L, mat):
    mat = np.ascontiguousarray(mat, np.int32)
    shear = np.zeros(4, np.int16)
    return L.ref_warp_shear(mat.ctypes.data, shear.ctypes.data), shear


def ref_table(L):
    t = np.zeros((193, 8), np.int16)
    L.ref_warp_table(t.ctypes.data)
    return t


def ref_fit(L, nsamples, pts, pts_inref, bsize, mv_x, mv_y, x, y):
    """-> int32 [12]: samples seen by find_projection, its return value (-1: not called), wmmat[0..5], alpha .. delta"""
    p = np.ascontiguousarray(pts, np.int32).copy()
    q = np.ascontiguousarray(pts_inref, np.int32).copy()
    out = np.zeros(12, np.int32)
    L.ref_warp_fit(int(nsamples), p.ctypes.data, q.ctypes.data, int(bsize), int(mv_x), int(mv_y), int(y) >> 2, int(x) >> 2, out.ctypes.data)
    return out


def fit_as_ref(m):
    """a fit() record in ref_fit's layout but for [1] (the return value: 0 exactly when valid, for a record with samples)"""
    return np.array([m["num_proj_ref"], 0] + list(m["mat"]) + [m["alpha"], m["beta"], m["gamma"], m["delta"]], np.int32)


def ref_pred(L, plane, bd, p_col, p_row, p_w, p_h, ss, mat, shear):
    plane = np.ascontiguousarray(plane)
    out = np.zeros((p_h, p_w), plane.dtype)
    mat = np.ascontiguousarray(mat, np.int32)
    shear = np.ascontiguousarray(shear, np.int16)
    L.ref_warp_pred(bd, plane.ctypes.data, plane.shape[1], plane.shape[0], plane.shape[1], out.ctypes.data, p_col, p_row, p_w, p_h, p_w, ss,
                    mat.ctypes.data, shear.ctypes.data)
    return out


# ---- draws (the generator's, and the tests' fresh ones): samples as record_samples leaves them ----
def draw_fit(rng, bsize=None, kind=None):
    """One record: neighbours of side 4 .. 64 above, left, above-left and above-right of the block, their vectors round the block's own.
    kind steers how far the neighbours' vectors lie from it (the classes the fixture has to cover)."""
    bsize = int(rng.choice(WARP_BSIZES)) if bsize is None else bsize
    bw, bh = BSIZE_W[bsize], BSIZE_H[bsize]
    kind = int(rng.integers(0, 8)) if kind is None else kind
    far = kind in (5, 6)
    x = int(rng.integers(0, (16384 if far else 2048) // bw)) * bw
    y = int(rng.integers(0, (16384 if far else 2048) // bh)) * bh
    mv_x, mv_y = int(rng.integers(-200, 201)), int(rng.integers(-200, 201))
    n = int(rng.choice((0, 1, 1, 2, 3, 4, 6, 8, 8)))
    if kind == 7:
        n = 8
    thresh = clamp(max(bw, bh), 16, 112)
    pts, pts_inref = np.zeros(16, np.int32), np.zeros(16, np.int32)
    # a smooth field round the block's vector: the neighbours' differences follow an affine model plus noise
    slope = rng.integers(-3, 4, 4) * (0, 1, 40, 6, 12, 3, 100, 1)[kind] / 256.0
    for i in range(n):
        nbw, nbh = (int(rng.choice((4, 8, 16, 32, 64))) for _ in range(2))
        side = int(rng.integers(0, 4))
        if side == 0:      # above
            px, py = int(rng.integers(-(nbw // 4 - 1) if nbw > bw else 0, bw // 4)) * 4 + nbw // 2 - 1, -(nbh // 2) - 1
        elif side == 1:    # left
            px, py = -(nbw // 2) - 1, int(rng.integers(-(nbh // 4 - 1) if nbh > bh else 0, bh // 4)) * 4 + nbh // 2 - 1
        elif side == 2:    # above-left
            px, py = -(nbw // 2) - 1, -(nbh // 2) - 1
        else:              # above-right
            px, py = bw + nbw // 2 - 1, -(nbh // 2) - 1
        dx = slope[0] * px + slope[1] * py + rng.integers(-2, 3)
        dy = slope[2] * px + slope[3] * py + rng.integers(-2, 3)
        r = rng.random()
        if kind == 3 and r < 0.5:                      # beyond select_samples' threshold
            dx += int(rng.choice((-1, 1))) * (thresh + int(rng.integers(1, 40)))
        if kind == 4 or (kind == 3 and r > 0.9):       # beyond LS_MV_MAX
            dy += int(rng.choice((-1, 1))) * int(rng.integers(256, 400))
        pts[2 * i], pts[2 * i + 1] = px * 8, py * 8
        pts_inref[2 * i], pts_inref[2 * i + 1] = px * 8 + mv_x + int(round(dx)), py * 8 + mv_y + int(round(dy))
    return dict(nsamples=n, pts=pts, pts_inref=pts_inref, bsize=bsize, mv_x=mv_x, mv_y=mv_y, x=x, y=y)

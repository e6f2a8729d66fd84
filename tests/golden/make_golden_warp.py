"""Writes tests/golden/warp.npz: the warped-motion fixture.  Runs where the reference's sources are; the tests read the fixture only.

The reference's Codec/EbWarpedMotion.c is not in oracle/'s compiled subset, so this script compiles it where it lies (the flags and the
objcopy --weaken step of oracle/Makefile) next to the project's own harness tests/c/ref_warp.c into oracle/_ref/libsvtref_warp.so;
select_samples and the block-size tables resolve against oracle/_ref/libsvtref.so.

Everything recorded is the reference's own output:
  table   warped_filter[193][8]
  fits    per record the samples, the vector, bsize and the block's origin (drawn as record_samples leaves them: tests/warp_cases.py,
          draw_fit), then the sample count find_projection saw (select_samples' return value where it ran), find_projection's return
          value, wmmat[0..5] and alpha .. delta (ref_warp_fit on a zeroed EbWarpedMotionParams)
  preds   av1_warp_plane / av1_warp_plane_hbd of luma and both chroma planes for blocks at the corners and edges of four pictures
          (104x72 and 72x104, 8 and 10 bit; two of them hold runs of 0 and of the maximum so that both output clips occur).  The models
          are recorded fits drawn at the block's own position, and hand-made matrices whose shears are get_shear_params' own: tile
          centres wholly outside the picture on each side (near and far), each shear negative and positive, and a full-pel translation without shear.
What the records cover is counted with the restatement's branch notes (tests/warp_cases.py; the restatement is asserted equal to the
reference on every record first), asserted here (at least MIN_COVER each) and stored as `cover_*`.

One branch of find_affine_int has no record: `shift < 0` needs 0 < |Det| <= 3, and Det cannot get there.  With a' = sx + 4, b' = sy + 4
one sample adds (a'^2 + 16) >> 2, (b'^2 + 16) >> 2 and (a' b') >> 2 to A[0][0], A[1][1], A[0][1]; over all integers |a'|, |b'| <= 80
the smallest determinant of one sample is 15 and of two samples 60 (an exhaustive count), and further samples only add positive
semi-definite terms.  Det == 0 is reached through "no sample passed LS_MV_MAX" alone.  The device code and the restatement keep the
branch; `cover_fit_shift_neg` records the 0."""
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import svtlibs  # noqa: E402
import warp_cases as wc  # noqa: E402

REF = os.environ.get("SVT_REF", "/root/reference")
MIN_COVER = 4
NFITS = 420
PICTURES = ((104, 72, 8, "smooth"), (72, 104, 8, "runs"), (104, 72, 10, "runs"), (72, 104, 10, "smooth"))
SHAPES = ((8, 8), (16, 8), (8, 16), (16, 16), (32, 16), (64, 32), (64, 64))          # luma; the chroma planes of the last four


def build_ref_lib():
    rc = os.path.join(REF, "Source", "Lib", "Common")
    flags = ["-O2", "-mavx2", "-fPIC", "-w", "-I" + os.path.join(REF, "Source", "API")] + \
        ["-I" + os.path.join(rc, d) for d in ("Codec", "C_DEFAULT", "ASM_SSE2", "ASM_SSSE3", "ASM_SSE4_1", "ASM_AVX2")]
    out = os.path.join(ROOT, "oracle", "_ref")
    obj = os.path.join(out, "obj_warp")
    os.makedirs(obj, exist_ok=True)
    assert os.path.exists(os.path.join(out, "libsvtref.so")), "build oracle/_ref/libsvtref.so first (make -C oracle ref)"
    objs = []
    for src in (os.path.join(rc, "Codec", "EbWarpedMotion.c"), os.path.join(ROOT, "tests", "c", "ref_warp.c")):
        o = os.path.join(obj, os.path.basename(src)[:-2] + ".o")
        subprocess.check_call(["gcc"] + flags + ["-c", src, "-o", o + ".tmp.o"])
        subprocess.check_call(["objcopy", "--weaken", o + ".tmp.o", o])
        os.remove(o + ".tmp.o")
        objs.append(o)
    subprocess.check_call(["gcc", "-shared", "-o", wc.REF_WARP] + objs + ["-L" + out, "-Wl,--no-as-needed", "-lsvtref", "-Wl,-rpath,$ORIGIN", "-lm"])


def draw_picture(rng, w, h, bd, content):
    planes = []
    for pl in range(3):
        pw, ph = (w, h) if pl == 0 else (w // 2, h // 2)
        p = svtlibs.smooth_picture(rng, ph, pw, grain=4).astype(np.int32)
        if bd == 10:
            p = p * 4 + rng.integers(0, 4, (ph, pw))
        if content == "runs":          # blocks of 0 and of the maximum side by side: the filter overshoots on both sides of the edge
            cells = rng.integers(0, 3, (ph // 4 + 1, pw // 4 + 1))
            cells = np.kron(cells, np.ones((4, 4), np.int64))[:ph, :pw]
            p = np.where(cells == 0, 0, np.where(cells == 1, (1 << bd) - 1, p))
        planes.append(p.clip(0, (1 << bd) - 1).astype(np.uint8 if bd == 8 else np.uint16))
    return planes


def positions(w, h, bw, bh):
    xs = sorted({0, ((w - bw) // 2) & ~7, w - bw})
    ys = sorted({0, ((h - bh) // 2) & ~7, h - bh})
    if bw == 64:
        xs, ys = [xs[0], xs[-1]], [ys[0], ys[-1]]
    return [(x, y) for y in ys for x in xs]


def hand_model(L, x, y, bw, bh, a, b, c, d, tx=0, ty=0):
    """[[1 + a, b], [c, 1 + d]] (1/65536) about the block's centre plus (tx, ty) in 1/65536 sample; the shears are the reference's"""
    cx, cy = x + bw // 2, y + bh // 2
    mat = np.array([wc.wrap32(tx - (cx * a + cy * b)), wc.wrap32(ty - (cx * c + cy * d)), 65536 + a, b, c, 65536 + d], np.int32)
    ok, shear = wc.ref_shear(L, mat)
    assert ok == 1, (mat, shear)
    return mat, shear


def main():
    build_ref_lib()
    L = wc.ref_lib()
    rng = np.random.default_rng(20261126)
    out = {}
    table = wc.ref_table(L)
    out["table"] = table
    # what csrc/warp_tables.h assumes of the table (8 bytes a row), checked on the reference's own copy
    assert (table.sum(axis=1) == 128).all() and table.min() >= -128 and table.max() <= 127

    fits = []

    def add_fit(d):
        r = wc.ref_fit(L, d["nsamples"], d["pts"], d["pts_inref"], d["bsize"], d["mv_x"], d["mv_y"], d["x"], d["y"])
        m, info = wc.fit(d["nsamples"], d["pts"], d["pts_inref"], d["bsize"], d["mv_x"], d["mv_y"], d["x"], d["y"])
        want = wc.fit_as_ref(m)
        assert np.array_equal(np.delete(r, 1), np.delete(want, 1)), (d, r, want)
        assert (r[1] == 0) == bool(m["valid"]) and (r[1] == -1) == (d["nsamples"] == 0), (d, r, m)
        fits.append((d, r, m, info))
        return len(fits) - 1

    for i in range(NFITS):
        add_fit(wc.draw_fit(rng, kind=i % 8))

    def fit_model_at(bsize, x, y, kind):
        for _ in range(200):
            d = wc.draw_fit(rng, bsize=bsize, kind=kind)
            d["x"], d["y"] = x, y
            d["mv_x"], d["mv_y"] = int(rng.integers(-40, 41)), int(rng.integers(-40, 41))
            shift = np.array([d["mv_x"], d["mv_y"]] * 8, np.int32)
            d["pts_inref"] = d["pts"] + shift + rng.integers(-3 - 2 * kind, 4 + 2 * kind, 16).astype(np.int32)
            if d["nsamples"] < 2:
                continue
            m, _ = wc.fit(d["nsamples"], d["pts"], d["pts_inref"], bsize, d["mv_x"], d["mv_y"], x, y)
            if m["valid"]:
                return add_fit(d)
        raise AssertionError("no valid model drawn")

    pred_cover = {k: 0 for k in wc.PRED_COVER}
    models, cases, data = [], [], {8: [], 10: []}
    shear_sign = np.zeros((4, 2), np.int64)                  # [alpha .. delta][negative, positive] over the cases' models
    copies = 0
    for pi, (w, h, bd, content) in enumerate(PICTURES):
        planes = draw_picture(rng, w, h, bd, content)
        for p, name in zip(planes, ("y", "cb", "cr")):
            out[f"pic{pi}_{name}"] = p
        k = 0
        for bw, bh in SHAPES:
            bsize = [b for b in range(22) if wc.BSIZE_W[b] == bw and wc.BSIZE_H[b] == bh][0]
            for x, y in positions(w, h, bw, bh):
                menus = [k % 16, (k + 1) % 16] + ([16, 17] if (bw, bh) == (8, 8) else [])
                k += 2
                for menu in menus:
                    fit_idx = -1
                    if menu in (0, 5, 10):
                        fit_idx = fit_model_at(bsize, x, y, (1, 2, 4)[menu // 5])
                        m = fits[fit_idx][2]
                        mat, shear = np.array(m["mat"], np.int32), np.array([m["alpha"], m["beta"], m["gamma"], m["delta"]], np.int16)
                    elif menu in (1, 2, 3, 4):           # wholly outside: left, right, top, bottom (inside the reference's translation clamp)
                        far = (127 << 16) + 12345
                        tx, ty = ((-far, 0), (far, 0), (0, -far), (0, far))[menu - 1]
                        mat, shear = hand_model(L, x, y, bw, bh, 300, -200, 150, 250, tx, ty)
                    elif menu in (6, 7):                 # far outside: ix4 / iy4 at -20000 and +20000
                        s = -1 if menu == 6 else 1
                        mat, shear = hand_model(L, x, y, bw, bh, 0, 0, 0, 0, s * (20000 << 16), s * (20000 << 16) + 4096)
                    elif menu == 8:                      # the copy: no shear, a full-pel translation
                        mat, shear = hand_model(L, x, y, bw, bh, 0, 0, 0, 0, int(rng.integers(-6, 7)) << 16, int(rng.integers(-6, 7)) << 16)
                        assert not shear.any()
                        copies += 1
                    elif menu in (16, 17):               # the first pass at the end of the table: 4 |alpha| + 7 |beta| = 65216 with the tile
                        s = -1 if menu == 16 else 1      # centre's phase at the matching end reaches offs 192 (s -1) and offs 0 (s 1)
                        mat, shear = hand_model(L, x, y, bw, bh, s * 8128, s * 4672, 0, 0, 65500 if s < 0 else 20, 0)
                    else:                                # one strong shear at a time and mixtures, both signs; sub-pel translation
                        a, b, c, d = {9: (6000, 0, 0, 0), 11: (-6000, 0, 0, 0), 12: (0, 4000, 0, -5000), 13: (0, -4000, 0, 5000),
                                      14: (3000, 2000, 7000, -3000), 15: (-3000, -2000, -7000, 3000)}[menu]
                        mat, shear = hand_model(L, x, y, bw, bh, a, b, c, d, int(rng.integers(-(3 << 16), 3 << 16)), int(rng.integers(-(3 << 16), 3 << 16)))
                    for s4 in range(4):
                        shear_sign[s4, 0] += shear[s4] < 0
                        shear_sign[s4, 1] += shear[s4] > 0
                    models.append(list(mat) + list(shear) + [fit_idx])
                    for pl in range(3 if (bw >= 16 and bh >= 16) else 1):
                        ss = int(pl > 0)
                        got = wc.ref_pred(L, planes[pl], bd, x >> ss, y >> ss, bw >> ss, bh >> ss, ss, mat, shear)
                        mine = wc.warp_pred(table, planes[pl], bd, x >> ss, y >> ss, bw >> ss, bh >> ss, ss, mat, shear, cover=pred_cover)
                        assert np.array_equal(got, mine), (pi, pl, bw, bh, x, y, menu)
                        if menu == 8:
                            tx, ty = int(mat[0]) >> (16 + ss), int(mat[1]) >> (16 + ss)
                            if not ss or (not (int(mat[0]) >> 16) & 1 and not (int(mat[1]) >> 16) & 1):
                                H, W = planes[pl].shape
                                rows = np.clip(np.arange(y >> ss, (y + bh) >> ss) + ty, 0, H - 1)
                                cols = np.clip(np.arange(x >> ss, (x + bw) >> ss) + tx, 0, W - 1)
                                # not a copy to the bit: the table's row for phase 0 is {0, 0, 0, 127, 1, 0, 0, 0} in both passes, so
                                # each output leans 1/128 towards its right and lower neighbour
                                shifted = planes[pl][rows][:, cols].astype(np.int64)
                                assert np.abs(got.astype(np.int64) - shifted).max() <= ((1 << bd) >> 5), "the full-pel model"
                        cases.append([pi, pl, bw, bh, x, y, len(models) - 1, sum(a.size for a in data[bd])])
                        data[bd].append(got.ravel())
    out["pictures"] = np.array([[w, h, bd] for w, h, bd, _ in PICTURES], np.int32)
    out["pred_models"] = np.array(models, np.int32)                    # mat[6], alpha .. delta, the recorded fit it came from or -1
    out["pred_cases"] = np.array(cases, np.int32)                      # picture, plane, luma bw, bh, luma x, y, model, offset into pred_data_<bd>
    out["pred_data_8"] = np.concatenate(data[8]).astype(np.uint8)
    out["pred_data_10"] = np.concatenate(data[10]).astype(np.uint16)

    n = len(fits)
    out["fit_nsamples"] = np.array([f[0]["nsamples"] for f in fits], np.int32)
    out["fit_pts"] = np.stack([f[0]["pts"] for f in fits]).astype(np.int32)
    out["fit_pts_inref"] = np.stack([f[0]["pts_inref"] for f in fits]).astype(np.int32)
    out["fit_bsize"] = np.array([f[0]["bsize"] for f in fits], np.int32)
    out["fit_mv"] = np.array([[f[0]["mv_x"], f[0]["mv_y"]] for f in fits], np.int32)
    out["fit_xy"] = np.array([[f[0]["x"], f[0]["y"]] for f in fits], np.int32)
    out["fit_ref"] = np.stack([f[1] for f in fits]).astype(np.int32)   # samples seen, find_projection's return value, wmmat[0..5], alpha .. delta
    fc = {k: 0 for k in wc.FIT_COVER}
    shift_neg = 0
    for d, r, m, info in fits:
        fc["valid"] += m["valid"]
        fc["nsamples_0"] += d["nsamples"] == 0
        fc["nsamples_1"] += d["nsamples"] == 1
        for k in ("dropped", "kept_none", "mv_rejected", "det0", "diag_clamp", "ndiag_clamp", "trans_clamp", "shear_refused"):
            fc[k] += info[k]
        fc["used_8"] += info["used"] == 8
        shift_neg += info["shift_neg"]
    for k in wc.FIT_COVER:
        out["cover_fit_" + k] = np.array(int(fc[k]))
    out["cover_fit_shift_neg"] = np.array(int(shift_neg))
    print(n, "fits:", {k: int(v) for k, v in fc.items()}, "shift_neg", shift_neg)
    assert min(fc.values()) >= MIN_COVER, fc
    assert shift_neg == 0                                              # see the module's note
    for k in wc.PRED_COVER:
        out["cover_pred_" + k] = np.array(int(pred_cover[k]))
    out["cover_pred_shear_sign"] = shear_sign
    out["cover_pred_copies"] = np.array(copies)
    print(len(cases), "predictions:", pred_cover, "shear signs", shear_sign.tolist(), "copies", copies)
    assert min(pred_cover.values()) >= MIN_COVER, pred_cover
    assert (shear_sign >= MIN_COVER).all() and copies >= MIN_COVER
    np.savez_compressed(wc.FIXTURE, **out)
    print("wrote", wc.FIXTURE, os.path.getsize(wc.FIXTURE), "bytes")
    assert os.path.getsize(wc.FIXTURE) < (1 << 20)


if __name__ == "__main__":
    main()

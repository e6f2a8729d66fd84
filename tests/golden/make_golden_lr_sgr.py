"""Writes tests/golden/lr_sgr.npz: the fixture of the self-guided parameter search of loop restoration.  Runs where the reference's
sources are; the tests read the fixture only.

The harness tests/c/ref_lr_sgr.c (which takes tests/c/ref_lr.c whole) is compiled with the reference's restoration sources by the
recipe of make_golden_lr.py into oracle/_ref/libsvtref_lr_sgr.so.  The pictures and cases are lr.npz's (u128, hbd, low, the
single-unit one_a, u64) plus one new small picture, f136, whose CDEF planes are constant over the first unit of every plane and its
halo (the projection is ill-posed there: Det < 1e-8) and so flat in part over the second.

What is recorded, all of it the reference's own output:
  entries   per (unit, ep), one round of search_selfguided_restoration's loop: apply_sgr, the dispatched get_proj_subspace, encode_xq,
            finer_search_pixel_proj_error - exq, the start xqd, the final xqd and its error, and xq with the error of every evaluation in
            order (a logging wrapper in the av1_{lowbd,highbd}_pixel_proj_error dispatch pointers)
  searches  per unit and RANGES setting, search_sgrproj_seg: search_selfguided_restoration as called there, then
            try_restoration_unit_seg - ep, xqd, SSE, and the sg_frame_ep_cnt histogram; the settings are the full range, two mid +- step
            ranges and an empty one, the ranges themselves read off the reference's filter calls
  planes    flt0 - u / flt1 - u of a few units (FLT), the top-row unit of unit size 128 among them, where a processing-unit boundary (row
            64) is no stripe boundary (row 56)
  finishes  rest_finish_search on the real search results (lr.npz's unfiltered and Wiener results, the full-range self-guided search)
            under make_golden_lr.FINISHES, for the cases lr.npz has
The _c and _avx2 flavours are asserted equal; what the cases cover is asserted (at least MIN_COVER each) and stored as `cover_*`."""
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
import lr_cases as lc  # noqa: E402
import lr_sgr_cases as sc  # noqa: E402
import make_golden_lr as mg  # noqa: E402

REF = mg.REF
MIN_COVER = 4
# name, picture, unit_size; the names lr.npz has are its cases (same picture and unit sizes)
CASES = (("u128", "p200", (128, 128, 128)), ("hbd", "h200", (64, 64, 64)), ("low", "l136", (64, 32, 32)), ("one_a", "p72", (64, 32, 32)),
         ("u64", "p200", (64, 32, 32)), ("flat", "f136", (64, 32, 32)))
# sg_ref_frame_ep, sg_filter_mode
RANGES = (((-1, -1), 4), ((6, 11), 3), ((14, 15), 2), ((5, -1), 1))
# case, plane, unit, ep: the planes kept
FLT = (("u128", 0, 0, 3), ("u128", 0, 0, 12), ("one_a", 1, 0, 0), ("one_a", 1, 0, 11), ("one_a", 2, 0, 15), ("hbd", 1, 3, 5), ("hbd", 2, 0, 14),
       ("flat", 0, 1, 2), ("flat", 1, 1, 10))


def build_ref_lib():
    rc = os.path.join(REF, "Source", "Lib", "Common")
    flags = ["-O2", "-mavx2", "-fPIC", "-w", "-I" + os.path.join(REF, "Source", "API"), "-I" + os.path.join(ROOT, "tests", "c")] + \
        ["-I" + os.path.join(rc, d) for d in ("Codec", "C_DEFAULT", "ASM_SSE2", "ASM_SSSE3", "ASM_SSE4_1", "ASM_AVX2")]
    out = os.path.join(ROOT, "oracle", "_ref")
    obj = os.path.join(out, "obj_lr_sgr")
    os.makedirs(obj, exist_ok=True)
    assert os.path.exists(os.path.join(out, "libsvtref.so")), "build oracle/_ref/libsvtref.so first (make -C oracle ref)"
    objs = []
    for src in [os.path.join(rc, "Codec", f) for f in ("EbRestoration.c", "convolve.c", "EbPsnr.c")] + \
            [os.path.join(rc, "ASM_AVX2", f) for f in ("wiener_convolve_avx2.c", "selfguided_avx2.c", "EbRestorationPick_AVX2.c", "pickrst_avx2.c")] + \
            [os.path.join(ROOT, "tests", "c", "ref_lr_sgr.c")]:
        o = os.path.join(obj, os.path.basename(src)[:-2] + ".o")
        subprocess.check_call(["gcc"] + flags + ["-c", src, "-o", o + ".tmp.o"])
        subprocess.check_call(["objcopy", "--weaken", o + ".tmp.o", o])
        os.remove(o + ".tmp.o")
        objs.append(o)
    subprocess.check_call(["gcc", "-shared", "-o", sc.REF_LR_SGR] + objs + ["-L" + out, "-Wl,--no-as-needed", "-lsvtref", "-Wl,-rpath,$ORIGIN", "-lm"])


def draw_flat(rng, w, h):
    """draw_picture's content with the CDEF planes constant over the first unit of every plane and 8 columns beyond it.  The constants are
    below 32: there both passes of the filter return a constant plane exactly (their rounded reciprocals, 164 * 25 and 455 * 9 against
    4096, leave it alone), so every sum of the projection is 0; from 32 on the first pass is off by one and only H11 is 0."""
    dblk, cdef, src = mg.draw_picture(rng, w, h, 8)
    for pl in range(3):
        cdef[pl] = cdef[pl].copy()
        cdef[pl][:, :(64 >> (pl > 0)) + 8] = 20 + 4 * pl
    return dblk, cdef, src


def main():
    build_ref_lib()
    rng = np.random.default_rng(20261022)
    out = {"cases": np.array([c[0] for c in CASES])}
    dblk, cdef, src = draw_flat(rng, 136, 72)
    for p, d, c, s in zip(lc.PLANES, dblk, cdef, src):
        out[f"f136_dblk_{p}"] = d
        out[f"f136_dcdef_{p}"] = (c.astype(np.int32) - d).astype(np.int16)
        out[f"f136_dsrc_{p}"] = (s.astype(np.int32) - d).astype(np.int16)
    pics = {"f136": (136, 72, 8, dblk, cdef, src)}
    lr_names = lc.case_names()

    cover = dict(both=0, r0_zero=0, r1_zero=0, ill_posed=0, twice=0, ties=0, limit=0, skip=0, moved=0)
    ranges = None
    flt_meta, flt_n = [], 0
    for ci, (name, pic, us) in enumerate(CASES):
        if pic not in pics:
            w, h, bd = {"p200": (200, 200, 8), "h200": (200, 200, 10), "l136": (136, 72, 8), "p72": (72, 40, 8)}[pic]
            pics[pic] = (w, h, bd) + tuple(lc.picture(lc.fixture(), pic))
        w, h, bd, dblk, cdef, src = pics[pic]
        if name in lr_names:
            k = lc.case(name)
            assert (k["pic"], k["w"], k["h"], k["bd"], tuple(k["unit_size"])) == (pic, w, h, bd, us)
        R = sc.RefPicture(w, h, bd, us, dblk, cdef, src)
        if ranges is None:      # what the settings mean, read off the reference's own filter calls
            ranges = [[ref[0], ref[1], mode] + list(R.ep_seen(ref, mode)) for ref, mode in RANGES]
            assert ranges[0][3:] == [0, 16] and ranges[-1][3:] == [-1, -1], ranges
        units = [(p, k) for p in range(3) for k in range(lc.plane_grid(w, h, us, p)[4] * lc.plane_grid(w, h, us, p)[5])]
        exq, start, final, err, ntrials, txq, terr = [], [], [], [], [], [], []
        for plane, k in units:
            lim = lc.unit_limits(w, h, us, plane, k)
            assert R.limits(plane, k) == lim
            flat_unit = len(np.unique(sc.unit_ext(cdef[plane], lim))) == 1
            for ep in range(16):
                a, b = R.sgr_ep(plane, k, ep, 0), R.sgr_ep(plane, k, ep, 1)
                assert (a["exq"], a["start"], a["final"], a["err"]) == (b["exq"], b["start"], b["final"], b["err"]) and np.array_equal(a["trials"], b["trials"]), \
                    (name, plane, k, ep, "the _c and _avx2 flavours differ")
                fin, e, ev = sc.replay_walk(ep, a["start"], a["trials"][:, :2], a["trials"][:, 2])
                assert fin == a["final"] and e == a["err"], (name, plane, k, ep)
                for key in ("twice", "ties", "limit", "skip"):
                    cover[key] += ev[key] > 0
                cover["moved"] += a["final"] != a["start"]
                if flat_unit:
                    assert a["exq"] == [0, 0], (name, plane, k, ep)
                    cover["ill_posed"] += 1
                exq.append(a["exq"]); start.append(a["start"]); final.append(a["final"]); err.append(a["err"]); ntrials.append(len(a["trials"]))
                txq.append(a["trials"][:, :2]); terr.append(a["trials"][:, 2])
        n = len(units)
        out[name + "_exq"], out[name + "_start"] = np.array(exq, np.int32).reshape(n, 16, 2), np.array(start, np.int16).reshape(n, 16, 2)
        out[name + "_final"], out[name + "_err"] = np.array(final, np.int16).reshape(n, 16, 2), np.array(err, np.int64).reshape(n, 16)
        out[name + "_ntrials"] = np.array(ntrials, np.int32).reshape(n, 16)
        out[name + "_trial_xq"], out[name + "_trial_err"] = np.concatenate(txq).astype(np.int16), np.concatenate(terr).astype(np.int64)
        assert np.array_equal(out[name + "_trial_xq"], np.concatenate(txq))
        search, cnts = [], []
        for ref, mode in RANGES:
            cnt, cnt2, rows = np.zeros(16, np.int32), np.zeros(16, np.int32), []
            for plane, k in units:
                ep, xqd, sse = R.sgr_search(plane, k, ref, mode, cnt, 0)
                assert (ep, xqd, sse) == R.sgr_search(plane, k, ref, mode, cnt2, 1), (name, plane, k, ref, mode)
                rows.append([ep] + xqd + [sse])
                if R.ep_seen(ref, mode)[0] >= 0:
                    cover[("both", "r0_zero", "r1_zero")[0 if ep < 10 else (1 if ep < 14 else 2)]] += 1
            assert np.array_equal(cnt, cnt2) and cnt.sum() == n
            search.append(rows); cnts.append(cnt)
        out[name + "_search"], out[name + "_cnt"] = np.array(search, np.int64), np.array(cnts, np.int32)
        for fc, plane, k, ep in FLT:
            if fc == name:
                a = R.sgr_ep(plane, k, ep, 0, planes=True)
                hs, he, vs, ve = lc.unit_limits(w, h, us, plane, k)
                u = cdef[plane][vs:ve, hs:he].astype(np.int32) << 4
                for key, f in (("f1", a["flt0"]), ("f2", a["flt1"])):
                    d = np.zeros_like(u) if f is None else f - u
                    assert np.abs(d).max() < 32768
                    out[f"flt_{flt_n}_{key}"] = d.astype(np.int16)
                flt_meta.append([ci, plane, k, ep])
                flt_n += 1
        if name in lr_names:      # rest_finish_search on real search results
            k = lc.case(name)
            res = k["results"].copy()
            full = out[name + "_search"][0]
            res["sse"][:, 2], res["ep"], res["xqd"] = full[:, 3], full[:, 0], full[:, 1:3]
            per_plane = [res[k["offsets"][p]:k["offsets"][p + 1]] for p in range(3)]
            fin_types, fin_units = [], []
            for fname, fmode, rdmult, cw, cs, csw in mg.FINISHES:
                m = k["ws_mode"] if fmode is None else fmode
                types, funits = R.finish(m, [rdmult] + list(cw) + list(cs) + list(csw), per_plane)
                fin_types.append([m] + types)
                fin_units.append(np.concatenate(funits))
            out[name + "_results"] = res.view(np.uint8)
            out[name + "_fin_types"], out[name + "_fin_units"] = np.array(fin_types, np.int32), np.stack(fin_units).view(np.uint8)
            out[name + "_wiener_win"] = np.array(k["win"], np.int32)
        R.close()
        out[name + "_pic"] = np.array(pic)
        out[name + "_params"] = np.array([w, h, bd] + list(us), np.int32)
    out["ranges"] = np.array(ranges, np.int32)
    out["flt_meta"] = np.array(flt_meta, np.int32)
    out["finishes"] = np.array([[rd] + list(cw) + list(cs) + list(csw) for _, _, rd, cw, cs, csw in mg.FINISHES], np.int32)
    names = ("both", "r0_zero", "r1_zero", "ill_posed", "twice", "ties", "limit", "skip", "moved")
    out["cover_names"], out["cover_sgr"] = np.array(names), np.array([cover[k] for k in names], np.int64)
    print("cover", cover, "ranges", ranges)
    assert min(cover.values()) >= MIN_COVER, cover
    np.savez_compressed(sc.FIXTURE, **out)
    print("wrote", sc.FIXTURE, os.path.getsize(sc.FIXTURE), "bytes")
    assert os.path.getsize(sc.FIXTURE) < (1 << 20)


if __name__ == "__main__":
    main()

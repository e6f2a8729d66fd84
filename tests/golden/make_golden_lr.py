"""Writes tests/golden/lr.npz: the loop-restoration fixture.  Runs where the reference's sources are; the tests read the fixture only.

The reference's Codec/EbRestoration.c, Codec/convolve.c, Codec/EbPsnr.c, ASM_AVX2/wiener_convolve_avx2.c, ASM_AVX2/selfguided_avx2.c, ASM_AVX2/pickrst_avx2.c and
ASM_AVX2/EbRestorationPick_AVX2.c are not in oracle/'s compiled subset, so this script compiles them where they lie (the flags and the
objcopy --weaken step of oracle/Makefile), next to the project's own harness tests/c/ref_lr.c (which includes EbRestorationPick.c in
place), into oracle/_ref/libsvtref_lr.so; the leftover symbols resolve against oracle/_ref/libsvtref.so.

What is recorded, all of it the reference's own output but for one figure: at 10 bit the squared error of a try is summed by the harness
over the output of the reference's own filter call, because the reference's 16-bit SSE is an assembly routine (tests/c/ref_lr.c):
  pictures  av1_loop_restoration_save_boundary_lines (after deblocking, after CDEF), then every unit through
            av1_loop_restoration_filter_unit as av1_loop_restoration_filter_frame's visitor hands it over (tests/c/ref_lr.c says why the
            visitor and not the function), per case
  tries     try_restoration_unit_seg per (unit, candidate); sse_restoration_unit for a candidate of type none
  stats     av1_compute_stats[_highbd] per unit at the case's windows: M and the upper triangle of H (the generator asserts H symmetric)
  searches  search_wiener_seg whole per unit (statistics, wiener_decompose_sep_sym, finalize_sym_filter, compute_score,
            finer_tile_search_wiener_seg): the final taps and SSE, and the taps of every trial in order, noted by a hook on
            av1_loop_restoration_filter_unit, each with its SSE (try_restoration_unit_seg again); the first trial is the derivation's filter
  finishes  rest_finish_search whole per case and setting (FINISHES: rdmult and the three cost tables, wn_filter_mode 0 among them): the
            frame type per plane and the unit records copy_unit_info left; the units' inputs are the recorded searches, the self-guided
            results being input data (the best of four drawn parameter sets by the reference's try)
  grids     the unit counts and limits the reference's visitor hands out, for the fixture's geometries and for 1920x1080 and 392x296 at
            unit size 256 (what tests/c/lr_plan_host.cpp checks its numbers against)
For the filters and the statistics the _c and _avx2 versions are both run and asserted equal.  What the cases cover is asserted here (at
least MIN_COVER each) and stored as `cover_*`; the deblocked picture is asserted to differ from the CDEF picture on the halo rows of
every inner stripe boundary, so that reading the wrong operand cannot pass."""
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import lr_cases as lc  # noqa: E402
import svtlibs  # noqa: E402

REF = os.environ.get("SVT_REF", "/root/reference")
MIN_COVER = 4
PICTURES = (("p200", 200, 200, 8), ("p72", 72, 40, 8), ("h200", 200, 200, 10), ("l136", 136, 72, 8),      # l136: low contrast (draw_low)
            ("c200", 200, 200, 8))                                                                           # c200: the CDEF picture is the reference's CDEF of the deblocked one (draw_chain)
CHAIN_QINDEX = 100
# name, picture, unit_size, frame_type, wiener_win
CASES = (
    ("u64", "p200", (64, 32, 32), (3, 3, 3), (7, 5, 5)),
    ("u64_planes", "p200", (64, 32, 32), (1, 0, 2), (5, 5, 5)),
    ("u128", "p200", (128, 128, 128), (3, 2, 1), (3, 3, 3)),
    ("one_a", "p72", (64, 32, 32), (3, 3, 3), (7, 5, 5)),
    ("one_b", "p72", (64, 64, 64), (1, 3, 1), (3, 3, 3)),
    ("hbd", "h200", (64, 64, 64), (3, 3, 3), (7, 5, 5)),
    ("low", "l136", (64, 32, 32), (3, 3, 3), (7, 5, 5)),
    ("chain", "c200", (64, 32, 32), (3, 3, 3), (7, 5, 5)),
)
# rest_finish_search settings: name, wn_filter_mode (None = the case's), rdmult, wiener_restore_cost, sgrproj_restore_cost, switchable_restore_cost
FINISHES = (
    ("plain", None, 120, (300, 700), (300, 700), (400, 900, 900)),
    ("dear", None, 1 << 30, (300, 700), (300, 700), (400, 900, 900)),
    ("wiener", None, 120, (300, 700), (300, 400000), (90000, 90000, 90000)),
    ("sgrproj", None, 120, (300, 400000), (300, 700), (90000, 90000, 90000)),
    ("forced", 0, 120, (300, 700), (300, 700), (400, 900, 900)),
    ("switch", None, 120, (9000, 9000), (9000, 9000), (0, 16, 16)),
    ("mid", None, 60000, (200, 1500), (200, 1500), (300, 1800, 1700)),
)
GRIDS = ((1920, 1080, (256, 256, 256)), (392, 296, (256, 128, 128)), (392, 296, (128, 64, 64)), (200, 200, (64, 32, 32)), (72, 40, (64, 32, 32)))


def build_ref_lib():
    rc = os.path.join(REF, "Source", "Lib", "Common")
    flags = ["-O2", "-mavx2", "-fPIC", "-w", "-I" + os.path.join(REF, "Source", "API")] + \
        ["-I" + os.path.join(rc, d) for d in ("Codec", "C_DEFAULT", "ASM_SSE2", "ASM_SSSE3", "ASM_SSE4_1", "ASM_AVX2")]
    out = os.path.join(ROOT, "oracle", "_ref")
    obj = os.path.join(out, "obj_lr")
    os.makedirs(obj, exist_ok=True)
    assert os.path.exists(os.path.join(out, "libsvtref.so")), "build oracle/_ref/libsvtref.so first (make -C oracle ref)"
    objs = []
    for src in [os.path.join(rc, "Codec", f) for f in ("EbRestoration.c", "convolve.c", "EbPsnr.c")] + \
            [os.path.join(rc, "ASM_AVX2", f) for f in ("wiener_convolve_avx2.c", "selfguided_avx2.c", "EbRestorationPick_AVX2.c", "pickrst_avx2.c")] + \
            [os.path.join(ROOT, "tests", "c", "ref_lr.c")]:
        o = os.path.join(obj, os.path.basename(src)[:-2] + ".o")
        subprocess.check_call(["gcc"] + flags + ["-c", src, "-o", o + ".tmp.o"])
        subprocess.check_call(["objcopy", "--weaken", o + ".tmp.o", o])
        os.remove(o + ".tmp.o")
        objs.append(o)
    subprocess.check_call(["gcc", "-shared", "-o", lc.REF_LR] + objs + ["-L" + out, "-Wl,--no-as-needed", "-lsvtref", "-Wl,-rpath,$ORIGIN", "-lm"])      # every reference is weak: keep the dependency


def draw_picture(rng, w, h, bd):
    """smooth content plus an offset per 16x16 block and grain (the deblocked picture); the CDEF output is that picture pulled towards
    its 3x3 mean where a block map says so, plus a sample here and there off by one; the source is the smooth content with other grain"""
    dblk, cdef, src = [], [], []
    for pl in range(3):
        pw, ph = (w, h) if pl == 0 else (w // 2, h // 2)
        base = 64 + svtlibs.smooth_picture(rng, ph + 8, pw + 8, grain=0)[:ph, :pw].astype(np.int32) // 2
        bs = 16 >> (pl > 0)
        off = np.kron(rng.integers(-5, 6, (ph // bs + 1, pw // bs + 1)), np.ones((bs, bs), np.int32))[:ph, :pw]
        d = base + off + rng.integers(-3, 4, (ph, pw))
        pad = np.pad(d, 1, mode="edge")
        mean = sum(pad[1 + dy:1 + dy + ph, 1 + dx:1 + dx + pw] for dy in (-1, 0, 1) for dx in (-1, 0, 1)) // 9
        strong = np.kron(rng.random((ph // 8 + 1, pw // 8 + 1)) < 0.6, np.ones((8, 8), bool))[:ph, :pw]
        c = np.where(strong, (d + mean + 1) // 2, d) + (rng.random((ph, pw)) < 0.35) * rng.choice((-1, 1), (ph, pw))
        s = base + rng.integers(-2, 3, (ph, pw))
        if bd == 10:
            d, c, s = d * 4 + rng.integers(0, 4, (ph, pw)), c * 4 + rng.integers(0, 4, (ph, pw)), s * 4 + rng.integers(0, 4, (ph, pw))
        dt = np.uint8 if bd == 8 else np.uint16
        dblk.append(d.clip(0, (1 << bd) - 1).astype(dt)); cdef.append(c.clip(0, (1 << bd) - 1).astype(dt)); src.append(s.clip(0, (1 << bd) - 1).astype(dt))
    return dblk, cdef, src


def draw_low(rng, w, h):
    """draw_picture's content at a sixth of its contrast: a tap moved by one step often changes no restored sample, so the reference's
    walks meet equal errors (a tie is accepted); the deblocked picture is the CDEF picture plus one everywhere"""
    _, cdef, src = draw_picture(rng, w, h, 8)
    cdef = [(100 + (c.astype(np.int32) - 100) // 6).astype(np.uint8) for c in cdef]
    src = [(100 + (s.astype(np.int32) - 100) // 6).astype(np.uint8) for s in src]
    return [(c + 1).astype(np.uint8) for c in cdef], cdef, src


def draw_chain(rng, w, h, out):
    """the deblocked picture and source of draw_picture; the CDEF picture is what the reference's CDEF makes of the deblocked one
    (make_golden_cdef.ref_apply: av1_cdef_frame's loop round the reference's cdef_filter_fb) under a drawn skip map and strengths, which
    the fixture carries with base_qindex, so that a test can run CDEF and restoration back to back on the device"""
    import make_golden_cdef as mgc
    L = mgc.ref_lib()
    assert L is not None
    dblk, _, src = draw_picture(rng, w, h, 8)
    nfb = ((w + 63) // 64) * ((h + 63) // 64)
    skip = (rng.random((h // 8, w // 8)) < 0.15).astype(np.uint8)
    ystr, ustr = rng.integers(9, 64, nfb).astype(np.int8), rng.integers(9, 64, nfb).astype(np.int8)
    cdef = mgc.ref_apply(L, [np.ascontiguousarray(p) for p in dblk], skip, 8, CHAIN_QINDEX, ystr, ustr)
    out["c200_skip"], out["c200_ystr"], out["c200_ustr"], out["c200_qindex"] = skip, ystr, ustr, np.array(CHAIN_QINDEX)
    return dblk, cdef, src


def draw_record(rng, rtype, win, ep_class=None):
    r = np.zeros((), lc.REF_REC)
    r["type"] = rtype
    for name in ("vfilter", "hfilter"):      # round the default taps (3, -7, 15), inside the ranges; a narrower window zeroes the outer ones
        t = [int(np.clip(m + rng.integers(-4, 5), lo, hi)) for m, lo, hi in zip((3, -7, 15), lc.TAP_MIN, lc.TAP_MAX)]
        if rng.random() < 0.15:
            t = [int(rng.integers(lo, hi + 1)) for lo, hi in zip(lc.TAP_MIN, lc.TAP_MAX)]
        if win <= 5:
            t[0] = 0
        if win == 3:
            t[1] = 0
        r[name] = t
    ep_class = int(rng.integers(0, 3)) if ep_class is None else ep_class
    r["ep"] = (int(rng.integers(0, 10)), int(rng.integers(10, 14)), int(rng.integers(14, 16)))[ep_class]
    r["xqd"] = [int(rng.integers(lo, hi + 1)) for lo, hi in zip(lc.XQD_MIN, lc.XQD_MAX)]
    return r


def main():
    build_ref_lib()
    rng = np.random.default_rng(20261021)
    out = {}
    pics = {}
    for name, w, h, bd in PICTURES:
        dblk, cdef, src = draw_low(rng, w, h) if name == "l136" else (draw_chain(rng, w, h, out) if name == "c200" else draw_picture(rng, w, h, bd))
        pics[name] = (w, h, bd, dblk, cdef, src)
        for p, d, c, s in zip(lc.PLANES, dblk, cdef, src):
            out[f"{name}_dblk_{p}"] = d
            out[f"{name}_dcdef_{p}"] = (c.astype(np.int32) - d).astype(np.int16 if bd > 8 else np.int8)
            out[f"{name}_dsrc_{p}"] = (s.astype(np.int32) - d).astype(np.int16 if bd > 8 else np.int8)
            assert ((d.astype(np.int32) + out[f"{name}_dcdef_{p}"]) == c).all() and ((d.astype(np.int32) + out[f"{name}_dsrc_{p}"]) == s).all()
        # reading the wrong operand must not pass: on the halo rows of every inner stripe boundary the two pictures differ
        for pl in range(3):
            ph = dblk[pl].shape[0]
            for y0, y1 in lc.stripes(ph, int(pl > 0)):
                for r in ([y0 - 2, y0 - 1] if y0 > 0 else []) + ([y1, y1 + 1] if y1 < ph else []):
                    assert (dblk[pl][r] != cdef[pl][r]).sum() >= dblk[pl].shape[1] // (16 if name == "c200" else 8), (name, pl, r)

    grids = []
    for w, h, us in GRIDS:
        zero = [np.zeros((h >> (p > 0), w >> (p > 0)), np.uint8) for p in range(3)]
        R = lc.RefPicture(w, h, 8, us, zero, zero, zero)
        for plane in range(3):
            nh, nv, n, visited = R.grid(plane)
            assert n == visited == nh * nv, (w, h, us, plane, nh, nv, n, visited)
            for u in sorted({0, nh - 1, n - nh, n - 1, n // 2}):
                grids.append([w, h, us[0], us[1], us[2], plane, nh, nv, u] + list(R.limits(plane, u)))
        R.close()
    out["grids"] = np.array(grids, np.int32)

    cover_halo = np.zeros((2, 2), np.int64)            # [top, bottom][picture edge, deblocked]: stripes of filtered units
    cover_types = np.zeros((3, 3), np.int64)           # [plane][unit type] over the switchable planes
    cover_ep = np.zeros(3, np.int64)                   # self-guided units per radius class: both, r[0] == 0, r[1] == 0
    cover_win = np.zeros(8, np.int64)                  # Wiener units per window
    cover_changed = np.zeros(3, np.int64)              # units per type whose output differs from the CDEF picture
    cover_finish_types = np.zeros(4, np.int64)         # planes ending in each frame type
    cover_finish_units = np.zeros(3, np.int64)         # units ending in each best type, in planes that are restored
    cover_finish_single = np.zeros(4, np.int64)        # single-unit planes per frame type (never switchable)
    cover_walk = dict(accepted=0, rejected=0, moved=0, ties=0, step4_twice=0, trials=0)      # searches: compute_score's verdicts and the walks
    out["cases"] = np.array([c[0] for c in CASES])
    for name, pic, us, ft, win in CASES:
        w, h, bd, dblk, cdef, src = pics[pic]
        R = lc.RefPicture(w, h, bd, us, dblk, cdef, src)
        units, offsets, cands = [], [], []
        for plane in range(3):
            pw, ph, ss, _, nh, nv = lc.plane_grid(w, h, us, plane)
            assert R.grid(plane)[:3] == (nh, nv, nh * nv)
            offsets.append(sum(len(u) for u in units))
            recs = np.zeros(nh * nv, lc.REF_REC)
            for k in range(nh * nv):
                assert R.limits(plane, k) == lc.unit_limits(w, h, us, plane, k), (name, plane, k)
                allowed = {0: (0,), 1: (0, 1), 2: (0, 2), 3: (0, 1, 2)}[ft[plane]]
                rtype = allowed[(k + plane) % len(allowed)] if nh * nv > 1 else allowed[-1]
                recs[k] = draw_record(rng, rtype, win[plane], ep_class=(k // 3 + plane) % 3)
                if ft[plane]:
                    cover_types[plane, rtype] += ft[plane] == 3
                    if rtype == 2:
                        cover_ep[(0 if recs[k]["ep"] < 10 else (1 if recs[k]["ep"] < 14 else 2))] += 1
                    if rtype == 1:
                        cover_win[win[plane]] += 1
                    if rtype:
                        hs, he, vs, ve = lc.unit_limits(w, h, us, plane, k)
                        for y0, y1 in lc.stripes(ph, ss):
                            if max(y0, vs) < min(y1, ve):
                                cover_halo[0, int(y0 > 0)] += 1
                                cover_halo[1, int(y1 < ph)] += 1
                # the search round of this unit: none, two Wiener, one self-guided of every radius class
                for cand in [draw_record(rng, 0, win[plane]), draw_record(rng, 1, win[plane]), draw_record(rng, 1, win[plane])] + \
                        [draw_record(rng, 2, win[plane], ep_class=e) for e in range(3)]:
                    cands.append((plane, k, cand))
            units.append(recs)
        offsets.append(sum(len(u) for u in units))
        res = R.frame(ft, units, 0)
        res_avx2 = R.frame(ft, units, 1)
        for a, b in zip(res, res_avx2):
            assert np.array_equal(a, b), (name, "the _c and _avx2 filters differ")
        for plane in range(3):
            for k in range(len(units[plane])):
                hs, he, vs, ve = lc.unit_limits(w, h, us, plane, k)
                if ft[plane] and units[plane][k]["type"]:
                    cover_changed[units[plane][k]["type"]] += not np.array_equal(res[plane][vs:ve, hs:he], cdef[plane][vs:ve, hs:he])
        # the reference visits only the planes it restores; the fixture keeps fewer candidates where there are many units
        keep = [c for i, c in enumerate(cands) if len(cands) <= 60 or i % 6 in ((c[1] + c[0]) % 6, (c[1] + 3) % 6)]
        sse = []
        for plane, k, cand in keep:
            a, b = R.try_unit(plane, k, cand, 0), R.try_unit(plane, k, cand, 1)
            assert a == b and a >= 0, (name, plane, k, a, b)
            sse.append(a)
        Ms, Hs = [], []
        for plane in range(3):
            w2 = win[plane] ** 2
            for k in range(len(units[plane])):
                M, H = R.stats(plane, k, win[plane], 0)
                M2, H2 = R.stats(plane, k, win[plane], 1)
                assert np.array_equal(M, M2) and np.array_equal(H, H2), (name, plane, k, "the _c and _avx2 statistics differ")
                assert np.array_equal(H, H.T)
                Ms.append(M); Hs.append(H[np.triu_indices(w2)])
        # search_wiener_seg whole per unit: the final taps and SSE, and every trial of the walk with its SSE
        mode = {(7, 5, 5): 3, (5, 5, 5): 2, (3, 3, 3): 1}[tuple(win)]
        ws_final, ws_sse, ws_n, ws_trials, ws_trial_sse = [], [], [], [], []
        for plane in range(3):
            for k in range(len(units[plane])):
                taps, wsse, trials = R.search_wiener(plane, k, mode, 0)
                taps2, wsse2, trials2 = R.search_wiener(plane, k, mode, 1)
                assert np.array_equal(taps, taps2) and wsse == wsse2 and np.array_equal(trials, trials2), (name, plane, k, "_c and _avx2 searches differ")
                tsse = []
                for t in trials:
                    rec = np.zeros((), lc.REF_REC)
                    rec["type"], rec["vfilter"], rec["hfilter"] = 1, t[:3], t[3:]
                    tsse.append(R.try_unit(plane, k, rec, 0))
                if len(trials):
                    # replay the reference's decisions over the recorded figures: what the walk keeps is its last accepted trial
                    err, kept = tsse[0], 0
                    for i in range(1, len(trials)):
                        if tsse[i] <= err:
                            cover_walk["ties"] += tsse[i] == err
                            err, kept = tsse[i], i
                    assert err == wsse and np.array_equal(trials[kept], taps), (name, plane, k)
                    cover_walk["accepted"] += 1
                    cover_walk["moved"] += kept > 0
                    d = np.abs(np.diff(trials.astype(np.int32), axis=0)).max(axis=1)
                    cover_walk["trials"] += len(trials)
                    moves4 = sum(1 for i in range(1, len(trials)) if tsse[i] <= min(tsse[:i]) and np.abs(trials[i].astype(np.int32) - trials[i - 1]).max() in (4, 8))
                    cover_walk["step4_twice"] += moves4 >= 2
                else:
                    assert wsse == np.iinfo(np.int64).max
                    cover_walk["rejected"] += 1
                ws_final.append(taps); ws_sse.append(wsse); ws_n.append(len(trials)); ws_trials.append(trials.reshape(-1, 6)); ws_trial_sse += tsse
        out[name + "_ws_mode"] = np.array(mode)
        out[name + "_ws_final"], out[name + "_ws_sse"], out[name + "_ws_n"] = np.array(ws_final, np.int16), np.array(ws_sse, np.int64), np.array(ws_n, np.int32)
        out[name + "_ws_trials"], out[name + "_ws_trial_sse"] = np.concatenate(ws_trials).astype(np.int16), np.array(ws_trial_sse, np.int64)
        # rest_finish_search whole per setting.  The units' results: the unfiltered unit's error, the Wiener search above, and for the
        # self-guided search (not built: its results are the finish's input data) the best of four drawn parameter sets by the reference's
        # own try
        results = []
        pos = 0
        for plane in range(3):
            ures = np.zeros(len(units[plane]), lc.RESULT_DTYPE)
            for k in range(len(units[plane])):
                ures[k]["sse"][0] = R.try_unit(plane, k, draw_record(rng, 0, win[plane]), 0)
                ures[k]["sse"][1] = ws_sse[pos]
                ures[k]["vfilter"], ures[k]["hfilter"] = ws_final[pos][:3], ws_final[pos][3:]
                best = None
                for _ in range(4):
                    cand = draw_record(rng, 2, win[plane])
                    e = R.try_unit(plane, k, cand, 0)
                    if best is None or e < best[0]:
                        best = (e, cand)
                ures[k]["sse"][2], ures[k]["ep"], ures[k]["xqd"] = best[0], best[1]["ep"], best[1]["xqd"]
                pos += 1
            results.append(ures)
        out[name + "_results"] = np.concatenate(results).view(np.uint8)
        fin_types, fin_units = [], []
        for fname, fmode, rdmult, cw, cs, csw in FINISHES:
            m = mode if fmode is None else fmode
            types, funits = R.finish(m, [rdmult] + list(cw) + list(cs) + list(csw), results)
            fin_types.append([m] + types)
            fin_units.append(np.concatenate(funits))
            for plane in range(3):
                cover_finish_types[types[plane]] += 1
                if types[plane]:
                    for u in funits[plane]:
                        cover_finish_units[int(u["type"])] += 1
                cover_finish_single[types[plane]] += len(units[plane]) == 1
        out[name + "_fin_types"] = np.array(fin_types, np.int32)
        out[name + "_fin_units"] = np.stack(fin_units).view(np.uint8)
        R.close()
        out[name + "_pic"] = np.array(pic)
        out[name + "_params"] = np.array([w, h, bd] + list(us) + list(ft) + list(win), np.int32)
        out[name + "_units"] = lc.to_units(np.concatenate(units)).view(np.uint8)
        out[name + "_offsets"] = np.array(offsets, np.int32)
        cd = np.zeros(len(keep), lc.CAND_DTYPE)
        for i, (plane, k, cand) in enumerate(keep):
            cd[i]["plane"], cd[i]["unit"] = plane, k
            cd[i]["u"] = lc.to_units(cand.reshape(1))[0]
        out[name + "_cands"] = cd.view(np.uint8)
        out[name + "_sse"] = np.array(sse, np.int64)
        out[name + "_M"], out[name + "_H"] = np.concatenate(Ms), np.concatenate(Hs)
        for p, r, c in zip(lc.PLANES, res, cdef):
            out[f"{name}_diff_{p}"] = (r.astype(np.int32) - c).astype(np.int16)

    out["cover_halo"], out["cover_types"], out["cover_ep"], out["cover_win"], out["cover_changed"] = cover_halo, cover_types, cover_ep, cover_win, cover_changed
    assert (cover_halo >= MIN_COVER).all(), ("halo sources", cover_halo)
    assert (cover_types >= MIN_COVER).all(), ("unit types per plane", cover_types)
    assert (cover_ep >= MIN_COVER).all(), ("self-guided radius classes", cover_ep)
    assert (cover_win[[3, 5, 7]] >= MIN_COVER).all(), ("Wiener windows", cover_win)
    assert (cover_changed[1:] >= MIN_COVER).all(), ("filtered units that changed", cover_changed)
    out["cover_walk"] = np.array([cover_walk[k] for k in ("accepted", "rejected", "moved", "ties", "step4_twice", "trials")], np.int64)
    print("searches", cover_walk)
    assert min(cover_walk[k] for k in ("accepted", "rejected", "moved", "ties", "step4_twice")) >= MIN_COVER, cover_walk
    out["finishes"] = np.array([[rd] + list(cw) + list(cs) + list(csw) for _, _, rd, cw, cs, csw in FINISHES], np.int32)
    out["cover_finish_types"], out["cover_finish_units"], out["cover_finish_single"] = cover_finish_types, cover_finish_units, cover_finish_single
    print("finishes: frame types", cover_finish_types.tolist(), "unit types", cover_finish_units.tolist(), "single-unit planes", cover_finish_single.tolist())
    assert (cover_finish_types >= MIN_COVER).all() and (cover_finish_units >= MIN_COVER).all(), (cover_finish_types, cover_finish_units)
    assert (cover_finish_single[:3] >= 1).all() and cover_finish_single[3] == 0, cover_finish_single
    np.savez_compressed(lc.FIXTURE, **out)
    print("wrote", lc.FIXTURE, os.path.getsize(lc.FIXTURE), "bytes")
    print("halo [top, bottom][edge, deblocked]", cover_halo.tolist(), "types [plane][type]", cover_types.tolist(), "ep", cover_ep.tolist(),
          "win", cover_win[[3, 5, 7]].tolist(), "changed", cover_changed.tolist())
    assert os.path.getsize(lc.FIXTURE) < (1 << 20)


if __name__ == "__main__":
    main()

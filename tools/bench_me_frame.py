#!/usr/bin/env python3
"""Motion estimation of one 1080p picture and of a stack of 16 pictures, P and B, 2 x 2 HME regions, a 64 x 64 search area, 209 PUs:
svt_hip_motion_estimate_frame (three launches per call) against the composed stage calls as tools/pipeline_y4m.py issues them
(svt_hip_hme_level_regions_batch x 3, svt_hip_me_setup_batch, svt_hip_me_fullpel_search_areas_batch per list, then
svt_hip_me_bipred_batch; per picture of a stack).  Both run in one process, alternating window by window; the composed path's
kernels are this build's (the stage kernels compute what the parent commit's compute; their resource figures are in DESIGN 4.25).
Both paths take the same parameters (a picture of the top temporal layer: HME level-0 multiplier 100, as the pipeline tool) and
both write into buffers allocated before the timing, so a window holds launches only: per list the composed path issues 3 HME
levels, the set-up, 2 fills that start the result rows (MAX_SAD_VALUE / 0; the frame call's prologue does that) and the search,
then 1 fill and the bi-prediction.  The calls are issued from Python; where the device finishes a call's kernels faster than the
host issues them a figure is the host's issue time, which "bound" names per row (`*_issue_ms`: the same loop timed on the host
without waiting for the device).

Timing: HIP events around windows of back-to-back calls, synchronised before and after, each window >= 0.2 s, 7 windows, median.
Writes profiles/r07_me_frame.json.
    python tools/bench_me_frame.py [--out profiles/r07_me_frame.json] [--quick]"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import __graft_entry__ as ge  # noqa: E402
import svtlibs                # noqa: E402

W, H, SA = 1920, 1080, 64


def window(fn, min_s=0.2):
    """seconds per call: calls back to back in a window of >= min_s, HIP events, synchronised around"""
    reps = 1
    while True:
        torch.cuda.synchronize()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(reps):
            fn()
        b.record()
        torch.cuda.synchronize()
        t = a.elapsed_time(b) / 1e3
        if t >= min_s:
            return t / reps
        reps = max(reps * 2, int(reps * min_s / max(t, 1e-6) * 1.2) + 1)


class Composed:
    """the stage calls for one picture, tables and parameter rows built once (as tools/pipeline_y4m.py does)"""

    def __init__(self, dsp, geo, planes, nl):
        self.dsp, self.geo, self.planes, self.nl = dsp, geo, planes, nl
        sbs = [(x, y) for y in range(0, H, 64) for x in range(0, W, 64)]
        size = [(min(64, W - x), min(64, H - y)) for x, y in sbs]
        dev = lambda a, dt: torch.from_numpy(np.array(a, dt)).cuda()
        self.org = [dev([(x >> s, y >> s) for x, y in sbs], np.int16) for s in (0, 1, 2)]
        self.size = [dev([(w >> s, h >> s) for w, h in size], np.int16) for s in (0, 1, 2)]
        self.soff = dev([y * geo[0][0] + x for x, y in sbs], np.int32)
        hw = {0: ((32, 32), (16, 16)), 1: ((16, 16), (8, 8)), 2: ((16, 16), (8, 8))}
        self.hme = {lv: [dsp.hme_level_params(lv, np.array(hw[lv][0], np.uint16), np.array(hw[lv][1], np.uint16), rw, rh, 64, 32, 100, 100,
                                              geo[2 - lv][1], geo[2 - lv][2], geo[2 - lv][3], geo[2 - lv][4]) for rh in (0, 1) for rw in (0, 1)] for lv in (0, 1, 2)}
        self.hme = {lv: (dsp.HmeParams * 4)(*rows) for lv, rows in self.hme.items()}
        self.setup = dsp.MeSetupParams(W, H, W, H, SA, SA, 2, 2, 0, 1)
        nsb, t = len(sbs), torch
        new = lambda shape, dt: t.empty(shape, dtype=dt, device="cuda")
        # every intermediate and output, allocated once: per list the three levels' SADs / vectors, centre + area, the result rows
        self.hme_out = [[(new((4, nsb), t.int64), new((4, nsb, 2), t.int16)) for _ in (0, 1, 2)] for _ in range(nl)]
        self.setup_out = [(new((nsb, 2), t.int16), new((nsb, 4), t.int16)) for _ in range(nl)]
        self.rows = [(new((nsb, 209), t.int32), new((nsb, 209), t.int32)) for _ in range(nl)]
        self.bip_out = (new((nsb, 209), t.int32), new((nsb, 209, 24), t.uint8))
        self.launches = nl * 7 + 2                        # per list: 3 HME levels, set-up, 2 row fills, search; then 1 fill + bi-prediction
        self.kernel_launches = nl * 5 + 1                 # (the svt_hip_* launches among them)

    def p00(self, pic, k):
        stride, ox, oy, _, _ = self.geo[k]
        return self.planes[pic][k].view(-1)[oy * stride + ox:]

    def __call__(self):
        dsp, rows = self.dsp, self.rows
        stride = self.geo[0][0]
        self.areas = []
        for li in range(self.nl):
            centres = None
            for lv in (0, 1, 2):
                k = 2 - lv
                b4, centres = dsp.hme_level_regions(self.p00(0, k), self.geo[k][0], self.p00(1 + li, k), self.geo[k][0], self.org[k], self.size[k], centres,
                                                    1 if lv == 1 else 0, self.hme[lv], out=self.hme_out[li][lv])
            _, area = dsp.me_setup(self.p00(0, 0), stride, self.p00(1 + li, 0), stride, self.org[0], self.size[0], b4, centres, self.setup,
                                   out=self.setup_out[li])
            self.areas.append(area)
            rows[li][0].fill_(dsp.MAX_SAD_VALUE); rows[li][1].zero_()
            dsp.me_fullpel_search_areas(self.p00(0, 0), stride, self.soff, self.p00(1 + li, 0), stride, self.soff, area, SA, SA, nsq=True,
                                        best_sad=rows[li][0], best_mv=rows[li][1])
        two = self.nl == 2
        return rows, dsp.me_bipred(self.p00(0, 0), stride, self.p00(1, 0), stride, self.p00(2, 0), stride, self.org[0], rows[0][0], rows[0][1],
                                   rows[1][0] if two else None, rows[1][1] if two else None, out=self.bip_out)


def issue_time(fn, reps=20):
    """seconds the host needs to issue one call (the device is idle at the start and is not waited for)"""
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    dt = (time.perf_counter() - t0) / reps
    torch.cuda.synchronize()
    return dt


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r07_me_frame.json"))
    ap.add_argument("--quick", action="store_true", help="3 windows instead of 7")
    a = ap.parse_args()
    pkg = ge.load_package()
    dsp = pkg.SvtHipDsp(0)
    rng = np.random.default_rng(725)
    nstack = 16
    big = svtlibs.smooth_picture(rng, H + 96, W + 96 + 3 * nstack)
    lum = [[np.ascontiguousarray(big[40 + dy:40 + dy + H, 40 + 3 * i + dx:40 + 3 * i + dx + W]) for dx, dy in ((0, 0), (5, 2), (-7, -3))] for i in range(nstack)]
    pyr = [[svtlibs.me_pyramid(p) for p in trip] for trip in lum]
    geo = pyr[0][0][1]
    stacks = [[torch.from_numpy(np.stack([pyr[i][j][0][k] for i in range(nstack)])).cuda() for k in range(3)] for j in range(3)]      # [src / ref0 / ref1][level]
    origins = [(g[1], g[2]) for g in geo]
    res = {"picture": f"{W}x{H}", "search_area": f"{SA}x{SA}", "hme_regions": "2x2", "pus": 209, "device": dsp.device_name(), "windows": 3 if a.quick else 7,
           "hme_level0_multiplier": 100, "buffers": "both paths write into buffers allocated before the timing",
           "composed_launches_are": "per list 3 HME levels + set-up + 2 result-row fills + search, then 1 fill + bi-prediction",
           "rows": []}
    for slice_name, slice_type, nl in (("P", 1, 1), ("B", 0, 2)):
        # temporal layer 1 of 1 hierarchical level: HME level-0 multiplier 100, what the composed rows above are built with
        prm = svtlibs.me_lcu_params(W, H, 0, 0, geo, slice_type=slice_type, pic_depth_mode=0, temporal_layer_index=1, hierarchical_levels=1,
                                    search_area_width=SA, search_area_height=SA,
                                    hme0_w=(32, 32), hme0_h=(16, 16), hme1_w=(16, 16), hme1_h=(8, 8), hme2_w=(16, 16), hme2_h=(8, 8))
        params = pkg.MeFrameParams.from_lcu_prm(prm)
        for n in (1, nstack):
            mp = [dsp.me_pyramid([t[:n] if n > 1 else t[0] for t in stacks[j]], origins) for j in range(3)]
            out = dsp.motion_estimate_frame(mp[0], mp[1], mp[2] if nl == 2 else None, params, n)
            fused = lambda: dsp.motion_estimate_frame(mp[0], mp[1], mp[2] if nl == 2 else None, params, n, out=out, scratch=out["_scratch"])
            comp = [Composed(dsp, geo, [[stacks[j][k][i] for k in range(3)] for j in range(3)], nl) for i in range(n)]
            composed = lambda: [c() for c in comp]
            # the two paths agree, on every picture, list and output, before anything is timed: equal search-area origins show that
            # both searched with the same parameters
            for i, c in enumerate(comp):
                rows, (bip, res_rows) = c()
                torch.cuda.synchronize()
                nsb = rows[0][0].shape[0]
                sl = slice(i * nsb, (i + 1) * nsb)
                for li in range(nl):
                    assert torch.equal(out["area_origin"][sl, li], c.areas[li][:, :2]), (slice_name, n, i, li, "area origin")
                    assert torch.equal(out["best_sad"][sl, li], rows[li][0]) and torch.equal(out["best_mv"][sl, li], rows[li][1]), (slice_name, n, i, li)
                assert torch.equal(out["bipred_sad"][sl], bip) and torch.equal(out["results"][sl], res_rows), (slice_name, n, i, "bi-prediction")
            tf, tc = [], []
            fused(); composed()
            for _ in range(res["windows"]):                      # alternating windows
                tc.append(window(composed)); tf.append(window(fused))
            row = {"slice": slice_name, "pictures": n, "composed_ms": round(1e3 * statistics.median(tc), 4), "frame_call_ms": round(1e3 * statistics.median(tf), 4),
                   "composed_launches": comp[0].launches * n, "composed_kernel_launches": comp[0].kernel_launches * n, "frame_call_launches": 3,
                   "composed_issue_ms": round(1e3 * issue_time(composed), 4), "frame_call_issue_ms": round(1e3 * issue_time(fused), 4),
                   "composed_windows_ms": [round(1e3 * t, 4) for t in tc], "frame_call_windows_ms": [round(1e3 * t, 4) for t in tf]}
            row["speedup"] = round(row["composed_ms"] / row["frame_call_ms"], 3)
            # a path whose windows take no longer than its host issue loop (within 10 %) is measured at the host's issue rate
            row["composed_bound"] = "host issue" if row["composed_ms"] <= 1.1 * row["composed_issue_ms"] else "device"
            row["frame_call_bound"] = "host issue" if row["frame_call_ms"] <= 1.1 * row["frame_call_issue_ms"] else "device"
            res["rows"].append(row)
            print(json.dumps({k: v for k, v in row.items() if not k.endswith("windows_ms")}), flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    json.dump(res, open(a.out, "w"), indent=1)


if __name__ == "__main__":
    main()

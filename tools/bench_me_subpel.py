#!/usr/bin/env python3
"""Sub-pel motion estimation of one 1080p picture: svt_hip_motion_estimate_subpel_frame (prologue, full-pel search, refinement,
bi-prediction on fractional vectors) next to svt_hip_motion_estimate_frame under the same parameters, in one process, alternating window
by window: P and B, 85 and 209 PUs, the three fractional search methods; 2 x 2 HME regions, a 16 x 8 search area.

Per row: both calls; the refinement launch by itself (svt_hip_me_subpel_frame on the full-pel rows: the rows are restored by two device
copies before every call, and the same two copies are timed alone and subtracted); the fractional bi-prediction launch has no entry
point of its own and is reported as what is left: (sub-pel call - full-pel call) - refinement = fractional bi-prediction minus the
integer one it replaces, with the integer launch's share unknown to this tool.  `refine_bytes_share`: the bytes the refinement must
move (each PU's reference window and source block once, its rows in and out) at the device-to-device copy rate measured in the same
process, as a share of the refinement's time - how far the launch is from being a copy.

Timing: HIP events around windows of back-to-back calls, synchronised before and after, each window >= 0.1 s, 5 windows, median.
Writes profiles/r23_me_subpel.json.
    python tools/bench_me_subpel.py [--out profiles/r23_me_subpel.json] [--quick]"""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import __graft_entry__ as ge  # noqa: E402
import me_subpel_cases as sp  # noqa: E402
import svtlibs                # noqa: E402

W, H = 1920, 1080
METHODS = {0: "SUB_SAD", 1: "FULL_SAD", 2: "SSD"}


def window(fn, min_s=0.1):
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


def refine_bytes(npus, nl, nsb):
    """bytes the refinement cannot avoid: per PU its window of the reference ((w + 5) x (h + 5)) and its source block, and 2 x 8 bytes of rows"""
    per_sb = sum((sp.pu_rect(n)[2] + 5) * (sp.pu_rect(n)[3] + 5) + sp.pu_rect(n)[2] * sp.pu_rect(n)[3] + 16 for n in range(npus))
    return per_sb * nl * nsb


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r23_me_subpel.json"))
    ap.add_argument("--quick", action="store_true", help="3 windows instead of 5")
    a = ap.parse_args()
    pkg = ge.load_package()
    dsp = pkg.SvtHipDsp(0)
    rng = np.random.default_rng(8162)
    big = svtlibs.smooth_picture(rng, H + 96, W + 96, grain=2)
    lum = [np.ascontiguousarray(big[40 + dy:40 + dy + H, 40 + dx:40 + dx + W]) for dx, dy in ((0, 0), (3, 1), (-2, -1))]
    lum[0] = ((lum[0].astype(np.int32) + lum[1]) // 2 + rng.integers(-2, 3, (H, W))).clip(0, 255).astype(np.uint8)      # between two samples: fractional minima
    pyr = [svtlibs.me_pyramid(p) for p in lum]
    geo = pyr[0][1]
    origins = [(g[1], g[2]) for g in geo]
    mp = [dsp.me_pyramid([torch.from_numpy(pl).cuda() for pl in pyr[j][0]], origins) for j in range(3)]
    # the box's copy rate: device-to-device copy of 256 MiB, read + written bytes per second
    buf = torch.empty(256 << 20, dtype=torch.uint8, device="cuda"); dst = torch.empty_like(buf)
    copy_rate = 2 * buf.numel() / statistics.median(window(lambda: dst.copy_(buf)) for _ in range(3))
    windows = 3 if a.quick else 5
    res = {"picture": f"{W}x{H}", "search_area": "16x8", "hme_regions": "2x2", "device": dsp.device_name(), "windows": windows,
           "copy_rate_GBps": round(copy_rate / 1e9, 1), "bipred_note": "fractional bi-prediction minus the integer launch it replaces (no entry point of its own)",
           "rows": []}
    nsb = ((W + 63) // 64) * ((H + 63) // 64)
    for slice_name, slice_type, nl in (("P", 1, 1), ("B", 0, 2)):
        for npus in (85, 209):
            for method in (0, 1, 2):
                prm = svtlibs.me_lcu_params(W, H, 0, 0, geo, slice_type=slice_type, pic_depth_mode=0 if npus == 209 else 2, fractional_search_method=method,
                                            search_area_width=16, search_area_height=8)
                params = pkg.MeFrameParams.from_lcu_prm(prm)
                r1 = mp[2] if nl == 2 else None
                full = dsp.motion_estimate_frame(mp[0], mp[1], r1, params)
                sub = dsp.motion_estimate_subpel_frame(mp[0], mp[1], r1, params)
                sad, mv = full["best_sad"].clone(), full["best_mv"].clone()
                dsp.me_subpel_frame(mp[0], mp[1], r1, params, sad, mv)
                torch.cuda.synchronize()
                assert torch.equal(sad, sub["best_sad"]) and torch.equal(mv, sub["best_mv"]), "the stage call and the whole call disagree"
                moved = float((mv != full["best_mv"])[..., :npus].float().mean())
                f_full = lambda: dsp.motion_estimate_frame(mp[0], mp[1], r1, params, out=full, scratch=full["_scratch"])
                f_sub = lambda: dsp.motion_estimate_subpel_frame(mp[0], mp[1], r1, params, out=sub, scratch=sub["_scratch"])
                f_sub(); f_full()
                restore = lambda: (sad.copy_(full["best_sad"]), mv.copy_(full["best_mv"]))
                f_stage = lambda: (restore(), dsp.me_subpel_frame(mp[0], mp[1], r1, params, sad, mv))
                tf, ts, tr, tc = [], [], [], []
                for _ in range(windows):                         # alternating windows
                    tf.append(window(f_full)); ts.append(window(f_sub)); tc.append(window(restore)); tr.append(window(f_stage))
                med = lambda v: statistics.median(v)
                refine = med(tr) - med(tc)
                nbytes = refine_bytes(npus, nl, nsb)
                row = {"slice": slice_name, "pus": npus, "method": METHODS[method], "fullpel_call_ms": round(1e3 * med(tf), 4), "subpel_call_ms": round(1e3 * med(ts), 4),
                       "refine_ms": round(1e3 * refine, 4), "bipred_fractional_minus_integer_ms": round(1e3 * (med(ts) - med(tf) - refine), 4),
                       "subpel_over_fullpel": round(med(ts) / med(tf), 3), "refine_bytes": nbytes, "refine_bytes_share": round(nbytes / copy_rate / refine, 4),
                       "vectors_moved": round(moved, 3), "fullpel_windows_ms": [round(1e3 * t, 4) for t in tf], "subpel_windows_ms": [round(1e3 * t, 4) for t in ts],
                       "stage_with_restore_windows_ms": [round(1e3 * t, 4) for t in tr], "restore_windows_ms": [round(1e3 * t, 4) for t in tc]}
                res["rows"].append(row)
                print(json.dumps({k: v for k, v in row.items() if not k.endswith("windows_ms")}), flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    json.dump(res, open(a.out, "w"), indent=1)


if __name__ == "__main__":
    main()

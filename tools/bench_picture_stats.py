#!/usr/bin/env python3
"""svt_hip_picture_stats_frame (GatheringPictureStatistics; two launches per call) on 1080p and 4K pictures, BLOCK_MEAN_PREC_SUB, 4 x 4
histogram regions, one picture per call and a stack of 16.  Per case: ms per picture, the algorithm's bytes over that time as a
fraction of the 8 TB/s HBM peak, and the host's time to issue one call (a case whose windows take no longer than the issue loop is
measured at the host's issue rate, not the device's: "bound"), and the same call 20 times in one captured graph (graph_ms_per_call:
the device's time per call when no host issues the launches one by one).

Algorithmic bytes per picture = what GatheringPictureStatistics reads and writes: rows 0, 2, 4, 6 of every 8x8 luma block of every SB
(SBs of the last column / row reach into the padding), the same rows of the chroma blocks of the complete SBs, the 1/16 luma, every
4th chroma sample of every 4th row, and the outputs.  (The kernels' lane loads are of these bytes only: in SUB precision the odd rows
are not loaded.  What the memory system fetches for them is more - a gathered chroma sample costs a whole sector - and is not counted.)

Timing: HIP events around windows of back-to-back calls into buffers allocated before the timing, synchronised before and after,
each window >= 0.2 s after a warm-up call, 7 windows, median.  The outputs are compared with the numpy restatement
(tests/golden/make_golden_picture_stats.np_picture_stats) on the first picture of every case before anything is timed.
Writes profiles/r11_picture_stats.json.
    python tools/bench_picture_stats.py [--out profiles/r11_picture_stats.json] [--quick]"""
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
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
import __graft_entry__ as ge  # noqa: E402
import make_golden_picture_stats as mg  # noqa: E402
import svtlibs                # noqa: E402

HBM_PEAK = 8.0e12
SIZES = ((1920, 1080), (3840, 2160))
RW = RH = 4
NSTACK = 16
GRAPH_CALLS = 20


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


def issue_time(fn, reps=50):
    """seconds the host needs to issue one call (the device is idle at the start and is not waited for)"""
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    dt = (time.perf_counter() - t0) / reps
    torch.cuda.synchronize()
    return dt


def byte_counts(W, H):
    """algorithmic bytes of one picture, SUB precision, RW x RH regions"""
    nsbx, nsby = (W + 63) // 64, (H + 63) // 64
    nsb, ncomplete = nsbx * nsby, (W // 64) * (H // 64)
    chroma_samples = sum(((w >> 1) + 3) // 4 * (((h >> 1) + 3) // 4) for _, w in mg.region_sizes(W, RW) for _, h in mg.region_sizes(H, RH)) * 2
    outputs = nsb * (85 + 2 * 85 + 2 * 21) + 2 + RW * RH * 3 * (256 * 4 + 1) + 3
    reads = nsb * 64 * 32 + ncomplete * 2 * 32 * 16 + (W // 4) * (H // 4) + chroma_samples
    return reads + outputs


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r11_picture_stats.json"))
    ap.add_argument("--quick", action="store_true", help="5 windows instead of 7")
    a = ap.parse_args()
    pkg = ge.load_package()
    dsp = pkg.SvtHipDsp(0)
    nwin = 5 if a.quick else 7
    res = {"device": dsp.device_name(), "block_mean_calc_prec": "SUB", "regions": f"{RW}x{RH}", "windows": nwin, "window_s": 0.2,
           "launches_per_call": 2, "hbm_peak_bytes_per_s": HBM_PEAK, "buffers": "outputs allocated before the timing", "rows": []}
    for W, H in SIZES:
        rng = np.random.default_rng(1100 + W)
        # a stack of different pictures: one smooth picture and its displaced copies (chroma: the luma's every other sample)
        big = svtlibs.smooth_picture(rng, H + 2 * NSTACK, W + 2 * NSTACK)
        pics = []
        for i in range(NSTACK):
            y = np.ascontiguousarray(big[i:i + H, 2 * i:2 * i + W])
            pics.append((y, np.ascontiguousarray(y[::2, ::2]), np.ascontiguousarray(255 - y[::2, ::2])))
        per_pic = [mg.np_planes(*p) for p in pics]
        stacks = [torch.from_numpy(np.stack([pp[k][0] for pp in per_pic])).cuda() for k in range(4)]
        origins = [(per_pic[0][k][1], per_pic[0][k][1]) for k in range(4)]
        want = mg.np_picture_stats(*pics[0], mg.SUB, RW, RH)
        alg = byte_counts(W, H)
        for n in (1, NSTACK):
            planes = dsp.pic_stats_planes([t[:n] if n > 1 else t[0] for t in stacks], origins)
            out = dsp.picture_stats_frame(planes, W, H, mg.SUB, (RW, RH), n_pictures=n)
            torch.cuda.synchronize()
            nsb = out.y_mean.shape[0] // n
            for k, g in (("y_mean", out.y_mean[:nsb]), ("variance", out.variance[:nsb]), ("cb_mean", out.cb_mean[:nsb]), ("cr_mean", out.cr_mean[:nsb]),
                         ("pic_avg_variance", out.pic_avg_variance[:1]), ("histogram", out.histogram[0]), ("avg_region", out.avg_intensity_region[0]),
                         ("avg", out.avg_intensity[0])):
                got = g.cpu().numpy()
                assert np.array_equal(got.view(want[k].dtype).reshape(want[k].shape), want[k]), (W, H, n, k)
            call = lambda: dsp.picture_stats_frame(planes, W, H, mg.SUB, (RW, RH), n_pictures=n, out=out)
            call()
            ts = [window(call) for _ in range(nwin)]
            t = statistics.median(ts)
            row = {"picture": f"{W}x{H}", "pictures": n, "ms_per_call": round(1e3 * t, 5), "ms_per_picture": round(1e3 * t / n, 5),
                   "algorithmic_bytes_per_picture": alg, "algorithmic_bytes_per_s": round(alg * n / t, 1),
                   "fraction_of_hbm_peak": round(alg * n / t / HBM_PEAK, 5), "issue_ms_per_call": round(1e3 * issue_time(call), 5),
                   "windows_ms_per_call": [round(1e3 * x, 5) for x in ts]}
            # windows that take no longer than the host's issue loop (within 10 %) measure the host's issue rate
            row["bound"] = "host issue" if row["ms_per_call"] <= 1.1 * row["issue_ms_per_call"] else "device"
            # the same call 20 times in one captured graph: what the device needs per call (its two launches and their boundaries)
            # when no host issues them one by one
            st = torch.cuda.Stream()
            st.wait_stream(torch.cuda.current_stream())
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.stream(st):
                with torch.cuda.graph(graph, stream=st):
                    for _ in range(GRAPH_CALLS):
                        call()
            torch.cuda.current_stream().wait_stream(st)
            graph.replay()
            tg = statistics.median([window(graph.replay) for _ in range(nwin)]) / GRAPH_CALLS
            row["graph_ms_per_call"] = round(1e3 * tg, 5)
            row["graph_fraction_of_hbm_peak"] = round(alg * n / tg / HBM_PEAK, 5)
            del graph
            res["rows"].append(row)
            print(json.dumps({k: v for k, v in row.items() if k != "windows_ms_per_call"}), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    json.dump(res, open(a.out, "w"), indent=1)


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""The self-guided parameter search of loop restoration on a 1080p 4:2:0 8-bit picture (the fixture generator's content), at unit
size 256 (48 units) and 64 / 32 (1530 units), over all 16 ep and over a mid +- 4 range (ep 4 .. 11):

  stats    svt_hip_lr_sgr_stats_frame: the filter per ep, the five sums, f1 / f2 / src - dat into the scratch.  Its bytes: each plane
           of the CDEF picture and of the source read once, 2 bytes per sample and 4 per sample and ep written
  walk     svt_hip_lr_sgr_walk_frame with the device solve: the evaluations made (total, and the longest walk), and its traffic
           estimate, evaluations x unit bytes (6 per sample), all of it at the box's measured copy rate as the floor
  search   svt_hip_lr_sgr_search_frame whole (statistics, walk, pick, the try of the winners)
  paced    what a host-paced search that re-filters would pay in launches and read-backs alone: per ep as many rounds as its longest
           walk, each round one svt_hip_lr_try_frame with a self-guided candidate per unit and one read-back, host wall clock.  A cost
           model for the ratio, not the same numbers: a try clips and follows the stripe rule
  host     where oracle/_ref/libsvtref_lr_sgr.so is present: the reference's search_selfguided_restoration with its _avx2 functions over
           every unit of the picture on ONE host thread; a one-thread figure, not the encoder's, which spreads units over segments
Timing: HIP events around windows of back-to-back calls, synchronised before and after, each window >= 0.2 s after a warm-up call,
7 windows, median.  Writes profiles/r25_lr_sgr.json.
    python tools/bench_lr_sgr.py [--out profiles/r25_lr_sgr.json] [--quick]"""
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
sys.path.insert(0, os.path.join(ROOT, "tools"))
import __graft_entry__ as ge  # noqa: E402
import lr_cases as lc  # noqa: E402
import lr_sgr_cases as sc  # noqa: E402
import make_golden_lr as mgl  # noqa: E402
from bench_lr import median_of  # noqa: E402

W, H = 1920, 1080
UNIT_SIZES = ((256, 256, 256), (64, 32, 32))
RANGES = ((0, 16), (4, 12))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r25_lr_sgr.json"))
    ap.add_argument("--windows", type=int, default=7)
    ap.add_argument("--quick", action="store_true", help="3 windows")
    a = ap.parse_args()
    pkg = ge.load_package()
    dsp = pkg.SvtHipDsp(0)
    nwin = 3 if a.quick else a.windows
    rng = np.random.default_rng(2525)
    dev = lambda x: torch.from_numpy(np.ascontiguousarray(x)).cuda()
    big = torch.empty(256 << 20, dtype=torch.uint8, device="cuda")
    big2 = torch.empty_like(big)
    t_copy, _ = median_of(lambda: big2.copy_(big), nwin)
    copy_rate = 2 * big.numel() / t_copy
    del big, big2
    torch.cuda.empty_cache()
    dblk_np, cdef_np, src_np = mgl.draw_picture(rng, W, H, 8)
    dblk, cdef, src = tuple(dev(p) for p in dblk_np), tuple(dev(p) for p in cdef_np), tuple(dev(p) for p in src_np)
    S = W * H * 3 // 2
    rows = []

    def report(row, raw):
        row["ms_windows"] = [v * 1e3 for v in raw]
        rows.append(row)
        print(json.dumps({k: (round(v, 4) if isinstance(v, float) else v) for k, v in row.items() if not k.endswith("windows")}), flush=True)

    host = None
    for us in UNIT_SIZES:
        grids, per_pic = dsp.lr_unit_grid(W, H, us, dsp.lib)
        npix = np.zeros(per_pic, np.int64)
        for plane, (nh, nv, off) in enumerate(grids):
            for k in range(nh * nv):
                hs, he, vs, ve = lc.unit_limits(W, H, us, plane, k)
                npix[off + k] = (he - hs) * (ve - vs)
        assert npix.sum() == S
        for lo, hi in RANGES:
            n = hi - lo
            need = dsp.lr_sgr_scratch_bytes(W, H, us, 1, lo, hi)
            scratch = torch.empty((need,), dtype=torch.uint8, device="cuda")
            stats = torch.zeros((per_pic, 16, 5), dtype=torch.int64, device="cuda")
            walk = torch.zeros((per_pic, 16, 24), dtype=torch.uint8, device="cuda")
            best = torch.zeros((per_pic, 24), dtype=torch.uint8, device="cuda")
            base = dict(unit_size=list(us), units=per_pic, ep_range=[lo, hi], scratch_bytes=need)
            t, raw = median_of(lambda: dsp.lr_sgr_stats_frame(cdef, src, W, H, 8, us, lo, hi, stats=stats, scratch=scratch), nwin)
            nbytes = 2 * S + 2 * S + 4 * S * n
            report(dict(base, call="stats", ms=t * 1e3, bytes=nbytes, copy_rate_GBps=copy_rate / 1e9, floor_ms=nbytes / copy_rate * 1e3, bytes_share=nbytes / copy_rate / t), raw)
            t, raw = median_of(lambda: dsp.lr_sgr_walk_frame(cdef, src, W, H, 8, us, scratch, lo, hi, stats=stats, walk=walk), nwin)
            rec = walk.cpu().numpy().view(sc.WALK_DTYPE).reshape(per_pic, 16)[:, lo:hi]
            traffic = int((rec["evals"].astype(np.int64) * npix[:, None]).sum()) * 6
            report(dict(base, call="walk", ms=t * 1e3, evaluations=int(rec["evals"].sum()), longest_walk=int(rec["evals"].max()), bytes=traffic,
                        floor_ms=traffic / copy_rate * 1e3, bytes_share=traffic / copy_rate / t, GBps=traffic / t / 1e9), raw)
            t, raw = median_of(lambda: dsp.lr_sgr_search_frame(cdef, dblk, src, W, H, 8, us, lo, hi, best=best, scratch=scratch), nwin)
            report(dict(base, call="search", ms=t * 1e3), raw)
            t_search = t
            # the host-paced cost model: rounds of one try and one read-back
            rounds = int(rec["evals"].max(axis=0).sum())
            cands = np.zeros(per_pic, lc.CAND_DTYPE)
            for plane, (nh, nv, off) in enumerate(grids):
                cands["plane"][off:off + nh * nv], cands["unit"][off:off + nh * nv] = plane, np.arange(nh * nv)
            cands["u"]["type"], cands["u"]["ep"] = 2, 4
            d_cands = dsp._lr_records(cands, dsp.LR_CAND_DTYPE, "cuda")
            sse = torch.empty((per_pic,), dtype=torch.int64, device="cuda")
            ts = []
            for _ in range(3):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(rounds):
                    dsp.lr_try_frame(cdef, dblk, src, W, H, 8, us, d_cands, sse=sse).cpu()
                ts.append(time.perf_counter() - t0)
            t = statistics.median(ts)
            report(dict(base, call="paced", ms=t * 1e3, rounds=rounds, ms_per_round=t / rounds * 1e3, over_search=t / t_search, clock="host wall clock"), ts)
            del scratch
            torch.cuda.empty_cache()
        if us == UNIT_SIZES[0] and sc.ref_lr_sgr() is not None:
            R = sc.RefPicture(W, H, 8, us, dblk_np, cdef_np, src_np)
            host = dict(threads=1, unit_size=list(us))
            for (lo, hi), ref, mode in (((0, 16), (-1, -1), 4), ((4, 12), (8, -1), 3)):
                assert R.ep_seen(ref, mode) == (lo, hi)
                cnt = np.zeros(16, np.int32)
                t0 = time.perf_counter()
                for plane, (nh, nv, off) in enumerate(grids):
                    for k in range(nh * nv):
                        R.sgr_search(plane, k, ref, mode, cnt, 1)
                host[f"search_sgrproj_seg_avx2_ep_{lo}_{hi}_ms"] = (time.perf_counter() - t0) * 1e3
            R.close()
            print(json.dumps({k: (round(v, 2) if isinstance(v, float) else v) for k, v in host.items()}), flush=True)
    out = dict(tool="tools/bench_lr_sgr.py", device=dsp.device_name(), picture=[W, H, 8], windows=nwin, rows=rows, host_reference_one_thread=host)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
    print("wrote", a.out)


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""Deblocking on a 1080p 4:2:0 8-bit picture: svt_hip_dlf_apply_frame (two buffers: one launch over tiles; in place: two launches) and
svt_hip_dlf_search_frame (3 and 64 levels per plane), on three mode-info grids:
  all_8x8     every block 8x8 with an 8x8 transform (an edge every 8 samples: the most edges the 8-tap class can have)
  all_64x64   every block 64x64 (14-tap luma, 6-tap chroma edges only)
  mixed       the final block list svt_hip_partition_decide_frame makes of the partition bench's all_blocks lists, scattered into the grid
              by svt_hip_dlf_mi_frame over an all-8x8 grid (units no final block covers keep it); half the blocks inter, a third skipped
Picture: the fixture generator's content (plateaus, a per-block offset, grain) as the reconstruction, the smooth part as the source.

  apply    time per picture; its bytes (each plane read and written once, plus the grid) at the box's measured copy rate as the floor
  search   the fused table for 3 and for 64 levels per plane, next to the path it replaces on the same box in the same run: per level
           a device copy of the three planes, svt_hip_dlf_apply_frame in place on the copy, and the three planes' SSE (torch: widen,
           subtract, square, sum).  The composed path's table is compared with the fused one before anything is timed.
Timing: HIP events around windows of back-to-back calls, synchronised before and after, each window >= 0.2 s after a warm-up call,
7 windows, median.  Writes profiles/r22_dlf.json.
    python tools/bench_dlf.py [--out profiles/r22_dlf.json] [--quick]"""
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
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import __graft_entry__ as ge  # noqa: E402
import bench_partition as bp  # noqa: E402
import dlf_cases as dc  # noqa: E402
import make_golden_dlf as mgd  # noqa: E402
import make_golden_partition as mgp  # noqa: E402

W, H = 1920, 1080
LEVELS3 = (8, 16, 24)


def window(fn, min_s=0.2):
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


def median_of(fn, nwin):
    fn()
    ts = [window(fn) for _ in range(nwin)]
    return statistics.median(ts), ts


def uniform_grid(bsize):
    mi = np.zeros((H // 4, W // 4, 4), np.uint8)
    mi[:, :] = (bsize, dc.tx_of(dc.BS_W[bsize], dc.BS_H[bsize]), 0, 0)
    return mi


def mixed_grid(pkg, dsp, rng):
    """partition decision of the partition bench's all_blocks lists -> final list -> svt_hip_dlf_mi_frame over an all-8x8 grid"""
    dev = torch.device("cuda:0")
    geom = mgp.load_geometry(dict(np.load(os.path.join(ROOT, "tests", "golden", "partition.npz"))))
    origins = [(64 * x, 64 * y) for y in range((H + 63) // 64) for x in range((W + 63) // 64)]
    c = bp.picture_case(np.random.default_rng(19019), geom, bp.CLASSES[2][1], origins)
    nsb, nleaves = len(origins), len(c["leaf"])
    T = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev)
    rec = np.zeros(nleaves, pkg.md_decision_dtype())
    rec["cost"], rec["cand"] = c["cost"], np.arange(nleaves) % 64
    args = dict(sb=T(c["sb"].view(np.uint8).reshape(nsb, 12)), leaf=T(c["leaf"].view(np.uint8).reshape(-1, 12)), decision=T(rec.view(np.uint8).reshape(-1, 72)),
                partition_bits=T(c["bits"]), pic_width=W, pic_height=H, slice_is_intra=0, sq=torch.empty((nsb, mgp.NSQ, 16), dtype=torch.uint8, device=dev),
                final_count=torch.empty((nsb,), dtype=torch.int32, device=dev), final=torch.empty((nsb, mgp.MAX_FINAL, 12), dtype=torch.uint8, device=dev))
    args["lambda"] = bp.LAMBDA
    assert dsp.partition_decide_frame(args) == 0, dsp.lib.svt_hip_last_error()
    info = np.zeros((nleaves, 4), np.uint8)
    inter = rng.random(nleaves) < 0.5
    info[:, 0] = np.where(inter, rng.integers(1, 8, nleaves), 0)
    info[:, 1] = np.where(inter, rng.integers(13, 25, nleaves), rng.integers(0, 13, nleaves))
    info[:, 2] = rng.random(nleaves) < 0.33
    mi = T(uniform_grid(3))
    dsp.dlf_mi_frame(args["final"], args["final_count"], T(info), mi)
    torch.cuda.synchronize()
    return mi.cpu().numpy(), int(args["final_count"].sum())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r22_dlf.json"))
    ap.add_argument("--windows", type=int, default=7)
    ap.add_argument("--quick", action="store_true", help="3 windows")
    a = ap.parse_args()
    pkg = ge.load_package()
    dsp = pkg.SvtHipDsp(0)
    nwin = 3 if a.quick else a.windows
    rng = np.random.default_rng(2222)
    dev = lambda x: torch.from_numpy(np.ascontiguousarray(x)).cuda()
    # the box's copy rate: a device-to-device copy of 256 MiB, read + written bytes per second
    big = torch.empty(256 << 20, dtype=torch.uint8, device="cuda")
    big2 = torch.empty_like(big)
    t_copy, _ = median_of(lambda: big2.copy_(big), nwin)
    copy_rate = 2 * big.numel() / t_copy
    del big, big2
    torch.cuda.empty_cache()
    mixed, nfinal = mixed_grid(pkg, dsp, rng)
    rows = []
    apply_bytes = 2 * (W * H * 3 // 2) + (W // 4) * (H // 4) * 4
    for name, mi_np in (("all_8x8", uniform_grid(3)), ("all_64x64", uniform_grid(12)), ("mixed", mixed)):
        rec_np, src_np = mgd.draw_picture(rng, W, H, 8, mi_np)
        rec, src, mi = tuple(dev(p) for p in rec_np), tuple(dev(p) for p in src_np), dev(mi_np)
        levels = (20, 20, 12, 12)
        dst = tuple(torch.empty_like(p) for p in rec)
        tmp = tuple(torch.empty_like(p) for p in rec)
        t2, raw2 = median_of(lambda: dsp.dlf_apply_frame(rec, mi, W, H, 8, levels, dst=dst), nwin)

        def in_place():
            dsp.dlf_apply_frame(tmp, mi, W, H, 8, levels, in_place=True)
        for x, y in zip(tmp, rec):
            x.copy_(y)
        in_place()
        torch.cuda.synchronize()
        assert all(torch.equal(x, y) for x, y in zip(tmp, dst)), "in place and two buffers differ"
        t1, raw1 = median_of(in_place, nwin)          # (filters what it has already filtered: the same work)
        floor = apply_bytes / copy_rate
        row = dict(call="apply", grid=name, two_buffers_ms=t2 * 1e3, in_place_ms=t1 * 1e3, bytes=apply_bytes, copy_rate_GBps=copy_rate / 1e9,
                   floor_ms=floor * 1e3, two_buffers_over_floor=t2 / floor, in_place_over_floor=t1 / floor,
                   two_buffers_ms_windows=[v * 1e3 for v in raw2], in_place_ms_windows=[v * 1e3 for v in raw1])
        rows.append(row)
        print(json.dumps({k: (round(v, 4) if isinstance(v, float) else v) for k, v in row.items() if not k.endswith("windows")}), flush=True)

        sse = torch.empty((3, 64), dtype=torch.int64, device="cuda")
        scratch = torch.empty((dsp.dlf_search_scratch_bytes(W, H, 1),), dtype=torch.uint8, device="cuda")
        wide = tuple(s.to(torch.int32) for s in src)
        table = torch.empty((3, 64), dtype=torch.int64, device="cuda")

        def composed(lv):
            for L in lv:
                for x, y in zip(tmp, rec):
                    x.copy_(y)
                if L:
                    dsp.dlf_apply_frame(tmp, mi, W, H, 8, (L, L, L, L), in_place=True)
                for pl in range(3):
                    table[pl, L] = (tmp[pl].to(torch.int32) - wide[pl]).pow(2).sum(dtype=torch.int64)

        for label, lv in (("3_levels", LEVELS3), ("64_levels", tuple(range(64)))):
            mask = sum(1 << L for L in lv)
            fused = lambda: dsp.dlf_search_frame(rec, src, mi, W, H, 8, masks=(mask,) * 3, sse=sse, scratch=scratch)
            fused(); composed(lv); torch.cuda.synchronize()
            assert all(torch.equal(sse[:, L], table[:, L]) for L in lv), "the fused and the composed tables differ"
            tf, rawf = median_of(fused, nwin)
            tc, rawc = median_of(lambda: composed(lv), max(3, nwin // 2))
            row = dict(call="search", grid=name, levels=label, fused_ms=tf * 1e3, composed_ms=tc * 1e3, composed_over_fused=tc / tf,
                       fused_ms_windows=[v * 1e3 for v in rawf], composed_ms_windows=[v * 1e3 for v in rawc])
            rows.append(row)
            print(json.dumps({k: (round(v, 4) if isinstance(v, float) else v) for k, v in row.items() if not k.endswith("windows")}), flush=True)
    out = dict(tool="tools/bench_dlf.py", device=dsp.device_name(), picture=[W, H, 8], mixed_final_blocks=nfinal, windows=nwin, rows=rows)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
    print("wrote", a.out)


if __name__ == "__main__":
    main()

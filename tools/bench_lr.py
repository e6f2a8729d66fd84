#!/usr/bin/env python3
"""Loop restoration on a 1080p 4:2:0 8-bit picture with unit_size 256 (48 units): svt_hip_lr_apply_frame, svt_hip_lr_try_frame and
svt_hip_lr_wiener_stats_frame.  Picture: the fixture generator's content (smooth content, block offsets, grain; the CDEF picture a
partly smoothed copy of the deblocked one).

  apply    every unit Wiener; every unit self-guided with both radii (ep 4), with r[0] == 0 (ep 12), with r[1] == 0 (ep 14); a mix of
           none / Wiener / self-guided units.  Its bytes (each plane of the CDEF picture read and the output written once) at the box's
           measured copy rate as the floor
  try      one Wiener candidate per unit, one self-guided candidate per unit (each plane of the CDEF picture and of the source read once)
  stats    windows 7 / 5 / 5 and 5 / 5 / 5 (each plane of the CDEF picture and of the source read once)
  search   dsp.lr_wiener_search whole (statistics -> derivation -> the walks of all units in lock step), host wall clock, with its rounds
  host     where oracle/_ref/libsvtref_lr.so is present: the reference's own _avx2 and _c functions on ONE host thread for the same
           picture (the whole-picture filter through av1_loop_restoration_filter_unit, av1_compute_stats per unit); a one-thread figure,
           not the encoder's, which spreads the units over its restoration segments
Timing: HIP events around windows of back-to-back calls, synchronised before and after, each window >= 0.2 s after a warm-up call,
7 windows, median.  Writes profiles/r24_lr.json.
    python tools/bench_lr.py [--out profiles/r24_lr.json] [--quick]"""
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
import lr_cases as lc  # noqa: E402
import make_golden_lr as mgl  # noqa: E402

W, H, US = 1920, 1080, (256, 256, 256)


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


def records(rng, n, kind):
    u = np.zeros(n, lc.UNIT_DTYPE)
    for k in range(n):
        r = mgl.draw_record(rng, 1, 7)
        for f in ("vfilter", "hfilter", "xqd"):
            u[k][f] = r[f]
        if kind == "wiener":
            u[k]["type"] = 1
        elif kind.startswith("sgr"):
            u[k]["type"], u[k]["ep"] = 2, int(kind[3:])
        else:
            u[k]["type"], u[k]["ep"] = k % 3, (4, 12, 14)[(k // 3) % 3]
    return u


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r24_lr.json"))
    ap.add_argument("--windows", type=int, default=7)
    ap.add_argument("--quick", action="store_true", help="3 windows")
    a = ap.parse_args()
    pkg = ge.load_package()
    dsp = pkg.SvtHipDsp(0)
    nwin = 3 if a.quick else a.windows
    rng = np.random.default_rng(2424)
    dev = lambda x: torch.from_numpy(np.ascontiguousarray(x)).cuda()
    big = torch.empty(256 << 20, dtype=torch.uint8, device="cuda")
    big2 = torch.empty_like(big)
    t_copy, _ = median_of(lambda: big2.copy_(big), nwin)
    copy_rate = 2 * big.numel() / t_copy
    del big, big2
    torch.cuda.empty_cache()
    dblk_np, cdef_np, src_np = mgl.draw_picture(rng, W, H, 8)
    dblk, cdef, src = tuple(dev(p) for p in dblk_np), tuple(dev(p) for p in cdef_np), tuple(dev(p) for p in src_np)
    grids, per_pic = dsp.lr_unit_grid(W, H, US, dsp.lib)
    plane_bytes = W * H * 3 // 2
    rows = []

    def report(row, raw):
        row["ms_windows"] = [v * 1e3 for v in raw]
        rows.append(row)
        print(json.dumps({k: (round(v, 4) if isinstance(v, float) else v) for k, v in row.items() if not k.endswith("windows")}), flush=True)

    dst = tuple(torch.empty_like(p) for p in cdef)
    unit_sets = {}
    for kind in ("wiener", "sgr4", "sgr12", "sgr14", "mixed"):
        unit_sets[kind] = records(rng, per_pic, kind)
        d_units = dsp._lr_records(unit_sets[kind], dsp.LR_UNIT_DTYPE, "cuda")
        t, raw = median_of(lambda: dsp.lr_apply_frame(cdef, dblk, W, H, 8, US, (3, 3, 3), d_units, dst=dst), nwin)
        floor = 2 * plane_bytes / copy_rate
        report(dict(call="apply", units=kind, ms=t * 1e3, bytes=2 * plane_bytes, copy_rate_GBps=copy_rate / 1e9, floor_ms=floor * 1e3, bytes_share=floor / t), raw)
    for kind in ("wiener", "sgr4"):
        cands = np.zeros(per_pic, lc.CAND_DTYPE)
        for plane, (nh, nv, off) in enumerate(grids):
            for k in range(nh * nv):
                cands[off + k]["plane"], cands[off + k]["unit"], cands[off + k]["u"] = plane, k, unit_sets[kind][off + k]
        d_cands = dsp._lr_records(cands, dsp.LR_CAND_DTYPE, "cuda")
        sse = torch.empty((per_pic,), dtype=torch.int64, device="cuda")
        t, raw = median_of(lambda: dsp.lr_try_frame(cdef, dblk, src, W, H, 8, US, d_cands, sse=sse), nwin)
        floor = 2 * plane_bytes / copy_rate
        report(dict(call="try", candidates=per_pic, units=kind, ms=t * 1e3, bytes=2 * plane_bytes, floor_ms=floor * 1e3, bytes_share=floor / t), raw)
    M = torch.empty((per_pic, 49), dtype=torch.int64, device="cuda")
    Hm = torch.empty((per_pic, 2401), dtype=torch.int64, device="cuda")
    scratch = torch.empty((dsp.lr_stats_scratch_bytes(W, H, US, 1),), dtype=torch.uint8, device="cuda")
    for win in ((7, 5, 5), (5, 5, 5)):
        t, raw = median_of(lambda: dsp.lr_wiener_stats_frame(cdef, src, W, H, 8, US, win, M=M, H=Hm, scratch=scratch), nwin)
        floor = 2 * plane_bytes / copy_rate
        macs = sum((w * w + w * w * (w * w + 1) // 2) * (W >> (i > 0)) * (H >> (i > 0)) for i, w in enumerate(win))
        report(dict(call="stats", windows_per_plane=list(win), ms=t * 1e3, bytes=2 * plane_bytes, floor_ms=floor * 1e3, bytes_share=floor / t,
                    multiply_adds=macs, tera_macs_per_s=macs / t / 1e12), raw)
    # the whole Wiener search: statistics, the derivation per unit on the host, the walks in lock step (host-paced: one launch and one
    # read-back per round), wall clock
    torch.cuda.synchronize()
    ts = []
    for _ in range(max(3, nwin // 2)):
        t0 = time.perf_counter()
        _, wsse, rounds = dsp.lr_wiener_search(cdef, dblk, src, W, H, 8, US, (7, 5, 5))
        ts.append(time.perf_counter() - t0)
    report(dict(call="wiener_search", windows_per_plane=[7, 5, 5], ms=statistics.median(ts) * 1e3, rounds=rounds,
                units_accepted=int((wsse != np.iinfo(np.int64).max).sum()), clock="host wall clock"), ts)
    host = None
    if lc.ref_lr() is not None:
        R = lc.RefPicture(W, H, 8, US, dblk_np, cdef_np, src_np)
        host = dict(threads=1)
        ref_units = np.zeros(per_pic, lc.REF_REC)
        for kind in ("wiener", "sgr4"):
            for f in ("type", "vfilter", "hfilter", "xqd", "ep"):
                ref_units[f] = unit_sets[kind][f]
            per_plane = [ref_units[off:off + nh * nv] for nh, nv, off in grids]
            for flavour, label in ((1, "avx2"), (0, "c")):
                t0 = time.perf_counter()
                R.frame((3, 3, 3), per_plane, flavour)
                host[f"apply_{kind}_{label}_ms"] = (time.perf_counter() - t0) * 1e3
        for flavour, label in ((1, "avx2"), (0, "c")):
            t0 = time.perf_counter()
            for plane, (nh, nv, off) in enumerate(grids):
                for k in range(nh * nv):
                    R.stats(plane, k, (7, 5, 5)[plane], flavour)
            host[f"stats_7_5_5_{label}_ms"] = (time.perf_counter() - t0) * 1e3
        R.close()
        print(json.dumps({k: (round(v, 2) if isinstance(v, float) else v) for k, v in host.items()}), flush=True)
    out = dict(tool="tools/bench_lr.py", device=dsp.device_name(), picture=[W, H, 8], unit_size=list(US), units=per_pic, windows=nwin, rows=rows,
               host_reference_one_thread=host)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
    print("wrote", a.out)


if __name__ == "__main__":
    main()

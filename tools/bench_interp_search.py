#!/usr/bin/env python3
"""The interpolation filter search on the device (svt_hip_interp_search_frame) on the blocks of a 1080p 4:2:0 picture (1920 x 1080, 8-bit,
80 / 48 samples of border) at 8x8, 16x16 and 64x64, one block per grid position that fits and 16 candidates per position, random vectors
within +-16 samples with both fractions non-zero, single reference and BI_PRED, luma alone (use_uv 0) and all three planes (use_uv 1).

Per shape three legs are timed in one process, alternating window by window:
  fused     svt_hip_interp_search_frame: the nine-pair SSE table in the scratch, then the walk (DUAL_FAST)
  decide    svt_hip_interp_decide_frame alone over that table
  composed  what a caller has without the search: svt_hip_inter_pred_frame, distortion only, SSD, over nine-fold block records (one per
            filter pair) and one group per plane, in one call; the host walk that would follow is not charged to it
Before anything is timed the composed path's nine-fold SSD is compared with the fused table.

Algorithmic bytes of the fused call, from the shapes: per block, plane and list one reference sample per predicted sample, one source
sample per predicted sample, 16 of block record, 36 of table out and in again, 32 of decision.  Those bytes over the box's copy rate as
svt_hip_membw_probe (mode 1) measures it in the same run (2 * bytes / time) is the traffic-only time.

Timing: HIP events around windows of back-to-back calls, synchronised before and after, each window >= 0.2 s after a warm-up call; the
legs of a shape alternate window by window, 5 windows each; median, minimum and maximum of the windows are kept: a difference inside the
windows' spread is no win.  Writes profiles/r15_interp_search.json.
    python tools/bench_interp_search.py [--out profiles/r15_interp_search.json] [--quick]"""
import argparse
import ctypes
import json
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as ge  # noqa: E402

PIC_W, PIC_H, PAD, PAD_C = 1920, 1080, 80, 48
SIZES = (8, 16, 64)
SSD = 1


def make_records(pkg, rng, bs, nx, ny, cands, direction):
    """inter_blk_dtype records of the nx x ny grid of bs x bs blocks, `cands` per position: vectors within +-16 samples with both
    fractions non-zero, every block of `direction`; the filter bytes stay 0 (the search tries all nine pairs)"""
    n = nx * ny * cands
    r = np.zeros(n, pkg.inter_blk_dtype())
    pos = np.arange(n) // cands
    r["x"], r["y"] = (pos % nx) * bs, (pos // nx) * bs
    r["mv"] = rng.integers(-16, 17, (n, 2, 2)) * 8 + rng.integers(1, 8, (n, 2, 2))
    r["pred_direction"] = direction
    return r


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r15_interp_search.json"))
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--quick", action="store_true", help="a quarter picture, 3 windows of 0.05 s (a smoke run)")
    a = ap.parse_args()
    pkg = ge.load_package()
    dsp = pkg.SvtHipDsp(0)
    dev = torch.device("cuda:0")
    nwin, min_s = (3, 0.05) if a.quick else (a.windows, 0.2)
    pic_w, pic_h = (PIC_W // 2, 544) if a.quick else (PIC_W, PIC_H)
    rng = np.random.default_rng(15033)
    D = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev)
    E = lambda shape, dt: torch.empty(shape, dtype=dt, device=dev)
    ok = lambda rc: rc == 0 or sys.exit(dsp.lib.svt_hip_last_error().decode())

    nbytes = (64 << 20) if a.quick else (1 << 30)
    cs, cd = E(nbytes, torch.uint8), E(nbytes, torch.uint8)
    cs.zero_()
    dsp.membw_probe(1, cd, cs, nbytes)
    copy_s = statistics.median(window(lambda: dsp.membw_probe(1, cd, cs, nbytes), min_s) for _ in range(nwin))
    copy_rate = 2.0 * nbytes / copy_s
    del cs, cd
    torch.cuda.empty_cache()
    print(json.dumps(dict(copy_bytes=nbytes, copy_ms=copy_s * 1e3, copy_rate_bytes_per_s=copy_rate)), flush=True)

    def padded(w, h, pad):
        return D(rng.integers(0, 256, (h + 2 * pad, w + 2 * pad)).astype(np.uint8))

    full = {n: [padded(pic_w, pic_h, PAD), padded(pic_w // 2, pic_h // 2, PAD_C), padded(pic_w // 2, pic_h // 2, PAD_C)] for n in ("ref0", "ref1", "src")}
    view = {n: [t[(PAD if k == 0 else PAD_C):, (PAD if k == 0 else PAD_C):] for k, t in enumerate(full[n])] for n in full}
    strides = [t.shape[1] for t in full["src"]]
    rates = D(rng.integers(60, 2200, (16, 3)).astype(np.int32))
    rows = []
    for cands in (1, 16):
        for bs in SIZES:
            nx, ny = pic_w // bs, pic_h // bs
            n = nx * ny * cands
            px = bs * bs
            for direction, dname in ((pkg.UNI_PRED_LIST_0, "single"), (pkg.BI_PRED, "bi")):
                r = make_records(pkg, rng, bs, nx, ny, cands, direction)
                blk = D(r.view(np.uint8).reshape(n, 16))
                r9 = np.repeat(r, 9)                                         # the composed path's records: [block][pair]
                r9["filter_y"], r9["filter_x"] = np.tile(np.arange(9) // 3, n), np.tile(np.arange(9) % 3, n)
                blk9 = D(r9.view(np.uint8).reshape(9 * n, 16))
                ctx, flag = D(rng.integers(0, 16, (n, 2)).astype(np.uint8)), D(np.ones(n, np.uint8))
                dec = E((n, 32), torch.uint8)
                for use_uv in (0, 1):
                    planes = 3 if use_uv else 1
                    sse = E((n, planes, 9), torch.int32)
                    prm = dsp.make_interp_params(3000, 400, rates, use_uv, pkg.INTERP_DUAL_FAST)
                    sg = dict(ref0=view["ref0"][:planes], ref1=view["ref1"][:planes], ref_stride=strides[:planes], src=view["src"][:planes],
                              src_stride=strides[:planes], bwidth=bs, bheight=bs, nblocks=n, blk=blk, ctx=ctx, searchable=flag, decision=dec)
                    sarr = dsp.make_interp_search_groups([sg])
                    need = dsp.lib.svt_hip_interp_search_scratch_bytes(sarr, 1, use_uv)
                    scratch = E((need,), torch.uint8)
                    darr = dsp.make_interp_decide_groups([dict(bwidth=bs, bheight=bs, nblocks=n, sse=sse, ctx=ctx, searchable=flag, decision=dec)])
                    tarr = dsp.make_interp_sse_groups([dict(sg, sse=sse)])
                    dist = [E((9 * n,), torch.int64) for _ in range(planes)]
                    carr = dsp.make_inter_pred_groups([dict(ref0=view["ref0"][p], ref1=view["ref1"][p], ref_stride=strides[p], ss=int(p > 0), bwidth=bs, bheight=bs,
                                                            nblocks=9 * n, blk=blk9, src=view["src"][p], src_stride=strides[p], dist=dist[p]) for p in range(planes)])
                    fused = lambda: ok(dsp.lib.svt_hip_interp_search_frame(sarr, 1, pic_w, pic_h, 8, ctypes.byref(prm), dsp._p(scratch), need, dsp._stream()))
                    decide = lambda: ok(dsp.interp_decide_frame(darr, prm))
                    composed = lambda: ok(dsp.inter_pred_frame(carr, pic_w, pic_h, 8, SSD))
                    # the composed path's numbers are the table
                    ok(dsp.interp_sse_frame(tarr, pic_w, pic_h, use_uv))
                    composed()
                    torch.cuda.synchronize()
                    want = torch.stack([d.view(n, 9) for d in dist], dim=1)
                    assert torch.equal(sse.long() & 0xffffffff, want), ("fused table against composed", bs, dname, use_uv)
                    variants = {"fused": fused, "decide": decide, "composed": composed}
                    for f in variants.values():
                        f()
                    torch.cuda.synchronize()
                    t = {k: [] for k in variants}
                    for _ in range(nwin):
                        for k, f in variants.items():
                            t[k].append(window(f, min_s))
                    ms = {k: statistics.median(v) * 1e3 for k, v in t.items()}
                    nl = 2 if direction == pkg.BI_PRED else 1
                    samples = px + (px // 2 if use_uv else 0)
                    b = n * (nl * samples + samples + 16 + 2 * 36 * planes + 32)
                    spread = max(max(v) - min(v) for v in (t["fused"], t["composed"])) * 1e3
                    row = dict(block=bs, candidates=cands, direction=dname, use_uv=use_uv, nblocks=n, ms=ms,
                               ms_min={k: min(v) * 1e3 for k, v in t.items()}, ms_max={k: max(v) * 1e3 for k, v in t.items()},
                               composed_over_fused=ms["composed"] / ms["fused"], window_spread_ms=spread,
                               fused_wins_beyond_spread=bool(ms["composed"] - ms["fused"] > spread),
                               algorithmic_bytes=b, traffic_only_ms=b / copy_rate * 1e3, traffic_fraction=b / copy_rate * 1e3 / ms["fused"],
                               gsamples_per_s_nine_pairs=9 * n * samples / (ms["fused"] * 1e-3) / 1e9)
                    rows.append(row)
                    print(json.dumps(row), flush=True)
                    del sse, scratch, dist
    out = dict(tool="tools/bench_interp_search.py", device=dsp.device_name(), picture=[pic_w, pic_h], quick=bool(a.quick), windows=nwin,
               copy_rate_bytes_per_s=copy_rate, rows=rows)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()

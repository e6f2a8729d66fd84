#!/usr/bin/env python3
"""AV1 inter prediction on the device (svt_hip_inter_pred_frame) on the luma blocks of a 1080p picture (1920 x 1080, 8-bit, an 80-sample
border) at 8x8, 16x16, 32x32 and 64x64, one block per grid position that fits, random vectors within +-16 samples, random filters.

Per size, three kinds of block are timed in one process, each as one call that stores a dense prediction:
  sr_2d     single reference, both fractions non-zero (the full two-pass filter)
  sr_full   single reference, full-pel vectors (the wave skips the filter and the LDS)
  bi_2d     BI_PRED, both lists 2-D (the list-0 intermediate stays in registers)
and for sr_2d the fused distortion (SAD and SSD) against the composed path a caller has without it:
  fused     the same call with d_src / d_dist set, the prediction still stored;  fused_only: d_pred NULL
  composed  the call without distortion, then svt_hip_sad_batch / svt_hip_sse_batch on the stored prediction and a dense copy of the
            source blocks (the gather of the source into that dense copy is not charged to it)
Before anything is timed the fused distortion is compared with the composed one.

Algorithmic bytes, from the shapes: per block and list one reference sample per predicted sample (w * h; the 7 extra rows and columns of
the window are overlap with the neighbours' windows), w * h of prediction out, 16 of block record in; with the distortion w * h of source
in and 8 out.  Those bytes over the box's copy rate as svt_hip_membw_probe (mode 1) measures it in the same run (2 * bytes / time) is the
traffic-only time; traffic_fraction = traffic-only time / measured time.

A second table (many_candidates) repeats sr_2d / sr_full / bi_2d, and the distortion-only call the fast loop's inter candidates need, with
16 candidates per grid position in one group at 8x8, 16x16 and 64x64: the regime in which the launch and one workgroup's latency no longer
count.  ms_per_picture is the time over 16.

Timing: HIP events around windows of back-to-back calls, synchronised before and after, each window >= 0.2 s after a warm-up call; the
variants of a size alternate window by window, 5 windows each, median.  Writes profiles/r14_inter_pred.json.
    python tools/bench_inter_pred.py [--out profiles/r14_inter_pred.json] [--quick]"""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as ge  # noqa: E402

PIC_W, PIC_H, PAD = 1920, 1080, 80
SIZES = (8, 16, 32, 64)
SAD, SSD = 0, 1


def make_records(pkg, rng, bs, nx, ny, kind, cands=1):
    """inter_blk_dtype records of the nx x ny grid of bs x bs blocks, `cands` per position: vectors within +-16 samples, full-pel for
    sr_full and with both fractions non-zero otherwise, BI_PRED for bi_2d and list 0 otherwise, random filters"""
    n = nx * ny * cands
    r = np.zeros(n, pkg.inter_blk_dtype())
    pos = np.arange(n) // cands
    r["x"], r["y"] = (pos % nx) * bs, (pos // nx) * bs
    whole = rng.integers(-16, 17, (n, 2, 2)) * 8
    frac = rng.integers(1, 8, (n, 2, 2)) if kind != "sr_full" else 0
    r["mv"] = whole + frac
    r["pred_direction"] = pkg.BI_PRED if kind == "bi_2d" else pkg.UNI_PRED_LIST_0
    r["filter_x"], r["filter_y"] = rng.integers(0, 3, n), rng.integers(0, 3, n)
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r14_inter_pred.json"))
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--quick", action="store_true", help="a quarter picture, 3 windows of 0.05 s (a smoke run)")
    a = ap.parse_args()
    pkg = ge.load_package()
    dsp = pkg.SvtHipDsp(0)
    dev = torch.device("cuda:0")
    nwin, min_s = (3, 0.05) if a.quick else (a.windows, 0.2)
    pic_w, pic_h = (PIC_W // 2, 544) if a.quick else (PIC_W, PIC_H)
    rng = np.random.default_rng(14031)
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

    stride = pic_w + 2 * PAD
    planes = [D(rng.integers(0, 256, (pic_h + 2 * PAD, stride)).astype(np.uint8)) for _ in range(3)]      # list 0, list 1, source
    ref0, ref1, srcp = (p[PAD:, PAD:] for p in planes)
    rows = []
    for bs in SIZES:
        nx, ny = pic_w // bs, pic_h // bs
        n = nx * ny
        px = bs * bs

        records = lambda kind: D(make_records(pkg, rng, bs, nx, ny, kind).view(np.uint8).reshape(n, 16))
        pred = E((n, bs, bs), torch.uint8)
        dist, dist2 = E((n,), torch.int64), E((n,), torch.int64)
        sad32 = E((n,), torch.int32)
        src_dense = srcp[:ny * bs, :nx * bs].reshape(ny, bs, nx, bs).permute(0, 2, 1, 3).reshape(n, bs, bs).contiguous()
        base = dict(ref0=ref0, ref1=ref1, ref_stride=stride, ss=0, bwidth=bs, bheight=bs, nblocks=n)
        arrs, keep = {}, []
        for kind in ("sr_2d", "sr_full", "bi_2d"):
            blk = records(kind)
            keep.append(blk)
            arrs[kind] = dsp.make_inter_pred_groups([dict(base, blk=blk, pred=pred)])
            if kind == "sr_2d":
                arrs["fused"] = dsp.make_inter_pred_groups([dict(base, blk=blk, pred=pred, src=srcp, src_stride=stride, dist=dist)])
                arrs["fused_only"] = dsp.make_inter_pred_groups([dict(base, blk=blk, src=srcp, src_stride=stride, dist=dist)])

        def call(key, metric=SAD):
            return lambda: ok(dsp.inter_pred_frame(arrs[key], pic_w, pic_h, 8, metric))

        P = dsp._p

        def composed(metric):
            def f():
                ok(dsp.inter_pred_frame(arrs["sr_2d"], pic_w, pic_h, 8, metric))
                if metric == SAD:
                    ok(dsp.lib.svt_hip_sad_batch(P(src_dense), bs, px, P(pred), bs, px, bs, bs, P(sad32), n, dsp._stream()))
                else:
                    ok(dsp.lib.svt_hip_sse_batch(P(src_dense), bs, px, P(pred), bs, px, bs, bs, P(dist2), n, dsp._stream()))
            return f

        # the fused distortion is the composed one
        for metric in (SAD, SSD):
            call("fused", metric)()
            composed(metric)()
            torch.cuda.synchronize()
            want = (sad32.long() & 0xffffffff) if metric == SAD else dist2
            assert torch.equal(dist, want), ("fused against composed", bs, metric)
            call("fused_only", metric)()
            torch.cuda.synchronize()
            assert torch.equal(dist, want), ("fused without a stored prediction", bs, metric)

        variants = {"sr_2d": call("sr_2d"), "sr_full": call("sr_full"), "bi_2d": call("bi_2d"),
                    "fused_sad": call("fused", SAD), "fused_only_sad": call("fused_only", SAD), "composed_sad": composed(SAD),
                    "fused_ssd": call("fused", SSD), "fused_only_ssd": call("fused_only", SSD), "composed_ssd": composed(SSD)}
        for f in variants.values():
            f()
        torch.cuda.synchronize()
        t = {k: [] for k in variants}
        for _ in range(nwin):
            for k, f in variants.items():
                t[k].append(window(f, min_s))
        ms = {k: statistics.median(v) * 1e3 for k, v in t.items()}
        lists = {"sr_2d": 1, "sr_full": 1, "bi_2d": 2}
        row = dict(block=bs, nblocks=n, ms=ms, ms_min={k: min(v) * 1e3 for k, v in t.items()})
        for k, nl in lists.items():
            b = n * (nl * px + px + 16)
            row[k] = dict(algorithmic_bytes=b, traffic_only_ms=b / copy_rate * 1e3, traffic_fraction=b / copy_rate * 1e3 / ms[k])
        bd = n * (px + px + 16 + px + 8)
        row["fused"] = dict(algorithmic_bytes=bd, traffic_only_ms=bd / copy_rate * 1e3,
                            fused_over_composed_sad=ms["fused_sad"] / ms["composed_sad"], fused_over_composed_ssd=ms["fused_ssd"] / ms["composed_ssd"])
        rows.append(row)
        print(json.dumps(row), flush=True)
    # the throughput regime: 16 candidates per grid position in one group (what the fast loop's inter candidates look like), where the
    # launch and one workgroup's latency no longer count; ms_per_picture is the time over 16
    CANDS = 16
    many = []
    for bs in (8, 16, 64):
        nx, ny = pic_w // bs, pic_h // bs
        n1 = nx * ny
        n = n1 * CANDS
        px = bs * bs
        pred = E((n, bs, bs), torch.uint8)
        dist = E((n,), torch.int64)
        arrs = {}
        for kind in ("sr_2d", "sr_full", "bi_2d"):
            blk = D(make_records(pkg, rng, bs, nx, ny, kind, CANDS).view(np.uint8).reshape(n, 16))
            keep.append(blk)
            g = dict(ref0=ref0, ref1=ref1, ref_stride=stride, ss=0, bwidth=bs, bheight=bs, nblocks=n, blk=blk)
            arrs[kind] = dsp.make_inter_pred_groups([dict(g, pred=pred)])
            arrs[kind + "_sad_only"] = dsp.make_inter_pred_groups([dict(g, src=srcp, src_stride=stride, dist=dist)])
        variants = {k: (lambda k=k: ok(dsp.inter_pred_frame(arrs[k], pic_w, pic_h, 8, SAD))) for k in arrs}
        for f in variants.values():
            f()
        torch.cuda.synchronize()
        t = {k: [] for k in variants}
        for _ in range(nwin):
            for k, f in variants.items():
                t[k].append(window(f, min_s))
        ms = {k: statistics.median(v) * 1e3 for k, v in t.items()}
        row = dict(block=bs, candidates=CANDS, nblocks=n, ms=ms, ms_per_picture={k: v / CANDS for k, v in ms.items()},
                   gsamples_per_s={k: n * px / (v * 1e-3) / 1e9 for k, v in ms.items()})
        for k, nl in (("sr_2d", 1), ("sr_full", 1), ("bi_2d", 2)):
            b = n * (nl * px + px + 16)
            row[k] = dict(algorithmic_bytes=b, traffic_only_ms=b / copy_rate * 1e3, traffic_fraction=b / copy_rate * 1e3 / ms[k])
        many.append(row)
        print(json.dumps(row), flush=True)
        del pred, dist
    out = dict(tool="tools/bench_inter_pred.py", device=dsp.device_name(), picture=[pic_w, pic_h], quick=bool(a.quick), windows=nwin,
               copy_rate_bytes_per_s=copy_rate, rows=rows, many_candidates=many)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()

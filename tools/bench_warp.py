#!/usr/bin/env python3
"""AV1 warped motion on the device on a 1080p picture (1920 x 1080, 4:2:0, 8 and 10 bit): svt_hip_warp_fit_frame and
svt_hip_warp_pred_frame, one block per grid position that fits, at 8x8, 16x16, 32x32 and 64x64 (chroma: the blocks of 16 and up, which
are the ones whose chroma the reference warps).

The models come from the fit itself: per block eight samples as av1_find_samples leaves them (four neighbours above, four to the left),
their vectors following a gentle affine field round the block's own, fitted on the device; valid_fraction is what the fit accepted.
Per (depth, plane, size), timed in one process as one call each:
  warp        direct mode, a dense prediction stored
  warp_sad    the same with d_src / d_dist set (the fused distortion), the prediction still stored
  warp_sad_only   d_pred NULL
  inter_2d    svt_hip_inter_pred_frame on the same grid, single reference, both fractions non-zero (the translational two-pass filter)
and per size the fit at 13 candidates per block (the 1 + 3 + 9 of inject_warped_motion_candidates).

Algorithmic bytes, from the shapes: per block one reference sample per predicted sample (the 7 extra rows and columns of a tile's window
are overlap with its neighbours'), w * h of prediction out, 16 of block record and 36 of model in; with the distortion w * h of source
in and 8 out; the fit reads 132 per block and 16 per candidate and writes 36 per candidate.  Those bytes over the box's copy rate as
svt_hip_membw_probe (mode 1) measures it in the same run (2 * bytes / time) is the traffic-only time.

Timing: HIP events around windows of back-to-back calls, synchronised before and after, each window >= 0.2 s after a warm-up call; the
variants of a shape alternate window by window, 5 windows each, median.  Writes profiles/r26_warp.json.
    python tools/bench_warp.py [--out profiles/r26_warp.json] [--quick]"""
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
BSIZE = {8: 3, 16: 6, 32: 9, 64: 12}
FIT_CANDS = 13
SAD = 0


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


def make_blocks(pkg, rng, bs, nx, ny, cands):
    """(samples [n], blk [n][cands]): the grid's blocks, vectors within +-8 samples with both fractions non-zero, the candidates round the
    first by up to a sample; eight neighbour samples per block under a gentle affine field"""
    n = nx * ny
    blk = np.zeros((n, cands), pkg.inter_blk_dtype())
    pos = np.arange(n)
    blk["x"], blk["y"] = ((pos % nx) * bs)[:, None], ((pos // nx) * bs)[:, None]
    mv = rng.integers(-8, 9, (n, 1, 2)) * 8 + rng.integers(1, 8, (n, 1, 2))
    blk["mv"][:, :, 0, :] = mv + np.concatenate([np.zeros((n, 1, 2), np.int64), rng.integers(-8, 9, (n, cands - 1, 2))], axis=1)
    blk["filter_x"], blk["filter_y"] = rng.integers(0, 3, (n, cands)), rng.integers(0, 3, (n, cands))
    s = np.zeros(n, pkg.warp_samples_dtype())
    s["nsamples"] = 8
    px = np.concatenate([rng.integers(0, bs, (n, 4)), np.full((n, 4), -5)], axis=1)
    py = np.concatenate([np.full((n, 4), -5), rng.integers(0, bs, (n, 4))], axis=1)
    A = rng.uniform(-0.15, 0.15, (n, 2, 2))                       # 1/8 sample of vector per sample of distance
    dx = A[:, 0, 0:1] * px + A[:, 0, 1:2] * py + rng.integers(-1, 2, (n, 8))
    dy = A[:, 1, 0:1] * px + A[:, 1, 1:2] * py + rng.integers(-1, 2, (n, 8))
    s["pts"][:, 0::2], s["pts"][:, 1::2] = px * 8, py * 8
    s["pts_inref"][:, 0::2] = px * 8 + mv[:, 0, 0:1] + np.rint(dx).astype(np.int64)
    s["pts_inref"][:, 1::2] = py * 8 + mv[:, 0, 1:2] + np.rint(dy).astype(np.int64)
    return s, blk


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r26_warp.json"))
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--quick", action="store_true", help="a quarter picture, 3 windows of 0.05 s (a smoke run)")
    a = ap.parse_args()
    pkg = ge.load_package()
    dsp = pkg.SvtHipDsp(0)
    dev = torch.device("cuda:0")
    nwin, min_s = (3, 0.05) if a.quick else (a.windows, 0.2)
    pic_w, pic_h = (PIC_W // 2, 544) if a.quick else (PIC_W, PIC_H)
    rng = np.random.default_rng(26031)
    D = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev)
    R = lambda x: D(x.view(np.uint8).reshape(x.shape + (x.dtype.itemsize,)))
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

    def timed(variants):
        for f in variants.values():
            f()
        torch.cuda.synchronize()
        t = {k: [] for k in variants}
        for _ in range(nwin):
            for k, f in variants.items():
                t[k].append(window(f, min_s))
        return {k: statistics.median(v) * 1e3 for k, v in t.items()}, {k: min(v) * 1e3 for k, v in t.items()}

    rows, fits = [], []
    for bd in (8, 10):
        tdt, ssz = (torch.uint8, 1) if bd == 8 else (torch.int16, 2)
        planes = {}
        for ss in (0, 1):
            w, h, pad = pic_w >> ss, pic_h >> ss, PAD >> ss
            mk = lambda: D(rng.integers(0, 1 << bd, (h + 2 * pad, w + 2 * pad)).astype(np.uint8 if bd == 8 else np.int16))
            planes[ss] = (mk(), mk(), w + 2 * pad, pad)                                                # reference, source
        for bs in SIZES:
            nx, ny = pic_w // bs, pic_h // bs
            n = nx * ny
            samples, blk = make_blocks(pkg, rng, bs, nx, ny, FIT_CANDS)
            d_samples, d_blk13, d_blk1 = R(samples), R(blk), R(np.ascontiguousarray(blk[:, :1]))
            model13, model1, nvalid = E((n, FIT_CANDS, 36), torch.uint8), E((n, 1, 36), torch.uint8), E((n,), torch.int32)
            fit13 = dsp.make_warp_fit_groups([dict(bsize=BSIZE[bs], ncand=FIT_CANDS, samples=d_samples, blk=d_blk13, model=model13, nvalid=nvalid)])
            fit1 = dsp.make_warp_fit_groups([dict(bsize=BSIZE[bs], ncand=1, samples=d_samples, blk=d_blk1, model=model1)])
            ok(dsp.warp_fit_frame(fit1))
            ok(dsp.warp_fit_frame(fit13))
            torch.cuda.synchronize()
            valid = float(model1[:, 0, 32].float().mean())
            if bd == 8:
                ms, ms_min = timed({"fit13": lambda: ok(dsp.warp_fit_frame(fit13))})
                b = n * (132 + FIT_CANDS * (16 + 36) + 4)
                fits.append(dict(block=bs, nblocks=n, candidates=FIT_CANDS, valid_fraction=float(nvalid.float().mean()) / FIT_CANDS, ms=ms["fit13"],
                                 ms_min=ms_min["fit13"], algorithmic_bytes=b, traffic_only_ms=b / copy_rate * 1e3,
                                 models_per_s=n * FIT_CANDS / (ms["fit13"] * 1e-3)))
                print(json.dumps(fits[-1]), flush=True)
            for ss in (0, 1):
                if ss and bs < 16:
                    continue
                refp, srcp, stride, pad = planes[ss]
                ref, src = refp[pad:, pad:], srcp[pad:, pad:]
                pw = bs >> ss
                pred = E((n, pw, pw), tdt)
                dist = E((n,), torch.int64)
                g = dict(ref=ref, ref_stride=stride, ss=ss, bwidth=bs, bheight=bs, ncand=1, blk=d_blk1, model=model1)
                arrs = dict(warp=dsp.make_warp_pred_groups([dict(g, pred=pred)]),
                            warp_sad=dsp.make_warp_pred_groups([dict(g, pred=pred, src=src, src_stride=stride, dist=dist)]),
                            warp_sad_only=dsp.make_warp_pred_groups([dict(g, src=src, src_stride=stride, dist=dist)]))
                inter = dsp.make_inter_pred_groups([dict(ref0=ref, ref_stride=stride, ss=ss, bwidth=bs, bheight=bs, nblocks=n, blk=d_blk1, pred=pred)])
                variants = {k: (lambda k=k: ok(dsp.warp_pred_frame(arrs[k], pic_w, pic_h, bd, SAD))) for k in arrs}
                variants["inter_2d"] = lambda: ok(dsp.inter_pred_frame(inter, pic_w, pic_h, bd, SAD))
                ms, ms_min = timed(variants)
                px = pw * pw * ssz
                b = {"warp": n * (2 * px + 52), "warp_sad": n * (3 * px + 60), "warp_sad_only": n * (2 * px + 60), "inter_2d": n * (2 * px + 16)}
                row = dict(bd=bd, plane="luma" if ss == 0 else "chroma", block=bs, plane_block=pw, nblocks=n, valid_fraction=valid, ms=ms, ms_min=ms_min,
                           algorithmic_bytes=b, traffic_only_ms={k: v / copy_rate * 1e3 for k, v in b.items()},
                           traffic_fraction={k: b[k] / copy_rate * 1e3 / ms[k] for k in b}, warp_over_inter_2d=ms["warp"] / ms["inter_2d"],
                           gsamples_per_s={k: n * pw * pw * valid / (ms[k] * 1e-3) / 1e9 for k in arrs})
                rows.append(row)
                print(json.dumps(row), flush=True)
                del pred, dist
    out = dict(tool="tools/bench_warp.py", device=dsp.device_name(), picture=[pic_w, pic_h], quick=bool(a.quick), windows=nwin,
               copy_rate_bytes_per_s=copy_rate, rows=rows, fit=fits)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()

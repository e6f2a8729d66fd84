#!/usr/bin/env python3
"""The fused intra fast loop (svt_hip_intra_fast_loop_frame) against the composed path it replaces, in one process: per candidate
svt_hip_build_intra_predictors_batch into a dense prediction buffer, then svt_hip_sse_batch (SSD) or svt_hip_sad_batch (SAD) of
source against prediction.  Dense 8-bit sources, all neighbours available, the candidate list of inject_intra_candidates (1: DC only;
13: no angle deltas; 61: the full list).  The composed path's prediction buffer (n x C x W x H bytes) is sized past the 256 MiB
Infinity Cache where the block count allows.

Timing: HIP events around windows of back-to-back calls, synchronised before and after, each window >= 0.2 s; the two paths
alternate window by window, 7 windows each, median.  With --bip-lib OLD.so the bip_kernel workload of tools/bench_kernels.py
(2^20 16x16 blocks, mixed modes) is timed the same way, alternating the library under test with OLD.so.
Writes profiles/r05_fast_loop.json.
    python tools/bench_fast_loop.py [--out profiles/r05_fast_loop.json] [--quick] [--bip-lib OLD.so]"""
import argparse
import ctypes
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as ge  # noqa: E402

SIZES = [(1, 8), (2, 16), (3, 32), (4, 64)]           # (tx_size, side)
NCANDS = [1, 13, 61]
PRED_BYTES = 320 << 20                                  # composed path's prediction buffer: past the 256 MiB Infinity Cache
MAX_BLOCKS = 1 << 20
PITCH = 1 + 2 * 64 + 15


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


def alternate(fns, nwin):
    """median seconds per call of each fn, windows interleaved"""
    for f in fns:
        f()
    ts = [[] for _ in fns]
    for _ in range(nwin):
        for i, f in enumerate(fns):
            ts[i].append(window(f))
    return [statistics.median(t) for t in ts], ts


def bip_before_after(pkg, dsp, old_path, nwin):
    """the bip workload of tools/bench_kernels.py through the library under test and through old_path, alternating"""
    dev = torch.device("cuda:0")
    n = 1 << 20
    top = torch.randint(0, 256, (n, 48), dtype=torch.uint8, device=dev); left = torch.randint(0, 256, (n, 48), dtype=torch.uint8, device=dev)
    blk = torch.zeros((n, 8), dtype=torch.uint8, device=dev)
    blk[:, 0] = torch.arange(n, device=dev) % 13
    blk[:, 1] = ((torch.arange(n, device=dev) // 13) % 7 - 3).to(torch.int8).view(torch.uint8) * ((blk[:, 0] >= 1) & (blk[:, 0] <= 8)).to(torch.uint8)
    blk[:, 4] = 16; blk[:, 5] = 16; blk[:, 6] = 16; blk[:, 7] = 16
    out_new = torch.empty((n, 16, 16), dtype=torch.uint8, device=dev); out_old = torch.empty_like(out_new)
    old = ctypes.CDLL(old_path)                             # (an older build: only the entry point used here is bound)
    old.svt_hip_build_intra_predictors_batch.argtypes = dsp.lib.svt_hip_build_intra_predictors_batch.argtypes
    assert old.svt_hip_init(0) == 0
    P = lambda t: ctypes.c_void_p(t.data_ptr())
    st = lambda: ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)

    def run(L, out):
        return lambda: L.svt_hip_build_intra_predictors_batch(P(out), 16, 256, None, P(top), P(left), 48, P(blk), 2, 0, 8, n, st())
    (t_new, t_old), raw = alternate([run(dsp.lib, out_new), run(old, out_old)], nwin)
    torch.cuda.synchronize()
    assert torch.equal(out_new, out_old), "bip outputs differ between the two libraries"
    return {"workload": "build_intra_predictors_16x16_u8(mixed modes), 2^20 blocks (tools/bench_kernels.py bip)", "blocks": n,
            "ms_after": round(t_new * 1e3, 4), "ms_before": round(t_old * 1e3, 4), "after_over_before": round(t_new / t_old, 4),
            "windows_ms_after": [round(v * 1e3, 4) for v in raw[0]], "windows_ms_before": [round(v * 1e3, 4) for v in raw[1]],
            "outputs_identical": True}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r05_fast_loop.json"))
    ap.add_argument("--windows", type=int, default=7)
    ap.add_argument("--quick", action="store_true", help="1/16 of the blocks, 3 windows (a smoke run)")
    ap.add_argument("--bip-lib", default=None, help="an older libsvt_hip_dsp.so to time bip_kernel against")
    a = ap.parse_args()
    pkg = ge.load_package()
    dsp = pkg.SvtHipDsp(0)
    L = dsp.lib
    dev = torch.device("cuda:0")
    gen = torch.Generator(device=dev); gen.manual_seed(1152)
    nwin = 3 if a.quick else a.windows
    P = lambda t: ctypes.c_void_p(t.data_ptr())
    rows = []
    for s, side in SIZES:
        bs = {8: 3, 16: 6, 32: 9, 64: 12}[side]
        full_m, full_d = pkg.SvtHipDsp.md_intra_candidates(side, side, side, bs, 0, False)
        for C in NCANDS:
            if C == 61:
                modes, deltas = [int(v) for v in full_m], [int(v) for v in full_d]
            elif C == 13:
                modes, deltas = list(range(13)), [0] * 13
            else:
                modes, deltas = [0], [0]
            n = min(MAX_BLOCKS, max(1024, PRED_BYTES // (C * side * side)))
            n = n // 16 if a.quick else n
            src = torch.randint(0, 256, (n, side, side), dtype=torch.uint8, device=dev, generator=gen)
            top = torch.randint(0, 256, (n, PITCH), dtype=torch.uint8, device=dev, generator=gen)
            left = torch.randint(0, 256, (n, PITCH), dtype=torch.uint8, device=dev, generator=gen)
            blk = torch.zeros((n, 8), dtype=torch.uint8, device=dev)
            blk[:, 2] = torch.randint(0, 2, (n,), dtype=torch.uint8, device=dev, generator=gen)
            blk[:, 4] = side; blk[:, 5] = side; blk[:, 6] = side; blk[:, 7] = side
            cblk = []
            for m, d in zip(modes, deltas):
                b = blk.clone(); b[:, 0] = m; b[:, 1] = d & 0xff
                cblk.append(b)
            pred = torch.empty((C, n, side, side), dtype=torch.uint8, device=dev)
            for metric, name in ((pkg.SvtHipDsp.FAST_SSD, "ssd"), (pkg.SvtHipDsp.FAST_SAD, "sad")):
                dist = torch.empty((n, C), dtype=torch.int64, device=dev)
                comp = [torch.empty(n, dtype=torch.int64 if metric == pkg.SvtHipDsp.FAST_SSD else torch.int32, device=dev) for _ in range(C)]
                groups = dsp.make_fast_loop_groups([dict(src=src, top=top, left=left, blocks=blk, nblocks=n, tx_size=s, modes=modes, deltas=deltas,
                                                         dist=dist)])
                dist_fn = L.svt_hip_sse_batch if metric == pkg.SvtHipDsp.FAST_SSD else L.svt_hip_sad_batch
                pp = side * side

                def fused():
                    rc = dsp.intra_fast_loop_frame(groups, metric, 0)
                    assert rc == 0, rc

                def composed():
                    st = dsp._stream()
                    for c in range(C):
                        rc = L.svt_hip_build_intra_predictors_batch(P(pred[c]), side, pp, None, P(top), P(left), PITCH, P(cblk[c]), s, 0, 8, n, st)
                        assert rc == 0, rc
                        rc = dist_fn(P(src), side, pp, P(pred[c]), side, pp, side, side, P(comp[c]), n, st)
                        assert rc == 0, rc
                (t_f, t_c), raw = alternate([fused, composed], nwin)
                torch.cuda.synchronize()
                same = torch.equal(dist, torch.stack([t.to(torch.int64) for t in comp], 1))
                pairs = n * C
                row = {"size": f"{side}x{side}", "ncand": C, "metric": name, "blocks": n, "pairs": pairs,
                       "composed_pred_bytes": C * n * pp,
                       "fused_ms": round(t_f * 1e3, 4), "composed_ms": round(t_c * 1e3, 4),
                       "fused_Gpairs_per_s": round(pairs / t_f / 1e9, 4), "composed_Gpairs_per_s": round(pairs / t_c / 1e9, 4),
                       "speedup": round(t_c / t_f, 3), "results_equal": bool(same),
                       "windows_ms_fused": [round(v * 1e3, 4) for v in raw[0]], "windows_ms_composed": [round(v * 1e3, 4) for v in raw[1]]}
                print(json.dumps(row), flush=True)
                rows.append(row)
                del dist, comp, groups
            del src, top, left, blk, cblk, pred
            torch.cuda.empty_cache()
    res = {"tool": "tools/bench_fast_loop.py", "device": dsp.device_name(), "windows": nwin, "min_window_s": 0.2,
           "method": "HIP events, fused / composed alternating window by window, median", "flavour": "C", "rows": rows}
    if a.bip_lib:
        res["bip_kernel"] = bip_before_after(pkg, dsp, a.bip_lib, nwin)
        print(json.dumps(res["bip_kernel"]), flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print("wrote", a.out)


if __name__ == "__main__":
    main()

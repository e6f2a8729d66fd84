#!/usr/bin/env python3
"""The fused mode-decision full loop (svt_hip_full_loop_frame) against the composed two-call path it replaces, in one process:
per transform type svt_hip_fwd_quant_planes_batch (coeff, qcoeff, dqcoeff and, for 64-point sizes, three_quad_energy to HBM) ->
eob uint16 -> uint32 -> svt_hip_picture_full_distortion32_batch.  Dense 8-bit batches, AVX2 distortion flavour, qindex 120.

Timing: HIP events around windows of back-to-back calls, synchronised before and after, each window >= 0.2 s; the two paths
alternate window by window, 7 windows each, median.  Writes profiles/r04_full_loop.json.
    python tools/bench_full_loop.py [--out profiles/r04_full_loop.json] [--quick]"""
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

HBM_PEAK = 8.0e12               # MI355X HBM3E, bytes/s
CASES = [(1, 1 << 20, [0]), (2, 1 << 18, [0]), (3, 1 << 16, [0]), (4, 1 << 14, [0]),
         (1, 1 << 20, list(range(16))), (2, 1 << 18, list(range(16)))]


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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r04_full_loop.json"))
    ap.add_argument("--windows", type=int, default=7)
    ap.add_argument("--quick", action="store_true", help="1/16 of the blocks, 3 windows (a smoke run)")
    a = ap.parse_args()
    pkg = ge.load_package()
    dsp = pkg.SvtHipDsp(0)
    tabs_np = pkg.tables.quant_tables(8)
    qrow = {k: np.ascontiguousarray(v[120]) for k, v in tabs_np.items()}
    qt = [np.ascontiguousarray(qrow[k]) for k in ("zbin", "round", "quant", "quant_shift", "dequant")]
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev); g.manual_seed(13660)
    nwin = 3 if a.quick else a.windows
    rows = []
    for s, n, types in CASES:
        n = n // 16 if a.quick else n
        w, h = pkg.TX_W[s], pkg.TX_H[s]
        nc = min(w, 32) * min(h, 32)
        T = len(types)
        src = torch.randint(0, 256, (n, h, w), dtype=torch.uint8, device=dev, generator=g)
        pred = (src.to(torch.int16) + torch.randint(-10, 11, (n, h, w), dtype=torch.int16, device=dev, generator=g)).clamp_(0, 255).to(torch.uint8)
        iscan = torch.from_numpy(np.stack([pkg.tables.scan_tables(s, t)[1] for t in types]).astype(np.int16)).to(dev)
        dist = torch.empty((n, T, 2), dtype=torch.int64, device=dev)
        eob = torch.empty((n, T), dtype=torch.int16, device=dev)
        garr = dsp.make_full_loop_groups([dict(src=src, pred=pred, nblocks=n, tx_size=s, tx_types=types, iscan=iscan, dist=dist, eob=eob)])

        def fused():
            rc = dsp.full_loop_frame(garr, qrow, 1)
            assert rc == 0, dsp.lib.svt_hip_last_error()

        co = torch.empty((n, nc), dtype=torch.int32, device=dev); q = torch.empty_like(co); dq = torch.empty_like(co)
        ceob = torch.empty(n, dtype=torch.int16, device=dev); nz = torch.empty(n, dtype=torch.int32, device=dev)
        en = torch.empty(n, dtype=torch.int64, device=dev) if max(w, h) == 64 else None
        cdist = torch.empty((n, 2), dtype=torch.int64, device=dev)
        P = dsp._p

        def composed():
            st = dsp._stream()
            for ti, t in enumerate(types):
                rc = dsp.lib.svt_hip_fwd_quant_planes_batch(P(src), 0, P(pred), 0, None, n, 0, 8, s, t, qt[0].ctypes.data, qt[1].ctypes.data,
                                                            qt[2].ctypes.data, qt[3].ctypes.data, qt[4].ctypes.data, P(iscan[ti]), P(co), P(q),
                                                            P(dq), P(ceob), None, P(en) if en is not None else None, st)
                assert rc == 0, dsp.lib.svt_hip_last_error()
                torch.bitwise_and(ceob.to(torch.int32), 0xffff, out=nz)
                rc = dsp.lib.svt_hip_picture_full_distortion32_batch(P(co), nc, P(dq), nc, w, h, P(nz), 1, P(cdist), n, st)
                assert rc == 0, dsp.lib.svt_hip_last_error()

        fused(); composed(); torch.cuda.synchronize()
        if T == 1:          # the two paths agree (before energy / shift, which the composed path leaves to its caller)
            sh = 2 if w * h <= 256 else (0 if w * h <= 1024 else -2)
            want = cdist + (en.view(-1, 1) if en is not None else 0)
            want = want >> sh if sh >= 0 else want << -sh
            assert torch.equal(dist[:, 0], want) and torch.equal(eob[:, 0], ceob)
        tf, tc = [], []
        for _ in range(nwin):
            tf.append(window(fused)); tc.append(window(composed))
        mf, mc = statistics.median(tf), statistics.median(tc)
        alg = 2.0 * w * h * n + 18.0 * n * T
        row = dict(tx_size=pkg.TX_SIZE_NAMES[s], nblocks=n, ntypes=T,
                   fused_ms=mf * 1e3, composed_ms=mc * 1e3, speedup=mc / mf,
                   fused_blocks_per_s=n / mf, fused_pairs_per_s=n * T / mf, composed_pairs_per_s=n * T / mc,
                   fused_hbm_fraction=alg / mf / HBM_PEAK, composed_hbm_fraction=alg / mc / HBM_PEAK,
                   fused_ms_windows=[x * 1e3 for x in tf], composed_ms_windows=[x * 1e3 for x in tc])
        rows.append(row)
        print(json.dumps({k: (round(v, 4) if isinstance(v, float) else v) for k, v in row.items() if not k.endswith("windows")}), flush=True)
        del src, pred, co, q, dq, dist, eob
        torch.cuda.empty_cache()
    out = dict(device=dsp.device_name(), hbm_peak_bytes_per_s=HBM_PEAK, flavour="AVX2", qindex=120,
               algorithmic_bytes="2 B/px in + 18 B per (block, type) out", quick=a.quick, cases=rows)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    json.dump(out, open(a.out, "w"), indent=1)
    print("wrote", a.out)


if __name__ == "__main__":
    main()

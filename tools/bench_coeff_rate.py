#!/usr/bin/env python3
"""The coefficient rate call (svt_hip_coeff_rate_frame) next to the full loop that feeds it (svt_hip_full_loop_frame with d_qcoeff), on the
same groups in one process: the luma transform blocks of a 1080p picture (1920 x 1080) at 8x8, 16x16 and 32x32, with 1 and with 16
transform types (32x32 defines 2: DCT_DCT and IDTX), coefficients from the full loop on pred = src + small noise, qindex 120.

Per case: the time of each call; the bytes of d_qcoeff the rate call reads; the traffic-only time, those bytes over the box's copy
rate as svt_hip_membw_probe (mode 1, copy) measures it in the same run (a copy moves two bytes per byte copied: the rate is taken as
2 * bytes / time); and the fraction traffic-only time / measured time.

Timing: HIP events around windows of back-to-back calls, synchronised before and after, each window >= 0.2 s after a warm-up call;
the two calls alternate window by window, 7 windows each, median.  Writes profiles/r08_coeff_rate.json.
    python tools/bench_coeff_rate.py [--out profiles/r08_coeff_rate.json] [--quick]"""
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

PIC_W, PIC_H = 1920, 1080
CASES = [(1, 1), (1, 16), (2, 1), (2, 16), (3, 1), (3, 2)]          # (tx_size, ntypes)


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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r08_coeff_rate.json"))
    ap.add_argument("--windows", type=int, default=7)
    ap.add_argument("--quick", action="store_true", help="1/16 of the blocks, 3 windows (a smoke run)")
    a = ap.parse_args()
    pkg = ge.load_package()
    dsp = pkg.SvtHipDsp(0)
    qrow = {k: np.ascontiguousarray(v[120]) for k, v in pkg.tables.quant_tables(8).items()}
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev); g.manual_seed(13680)
    nwin = 3 if a.quick else a.windows
    rng = np.random.default_rng(13680)

    # the box's copy rate, this run
    nbytes = (64 << 20) if a.quick else (1 << 30)
    cs, cd = torch.empty(nbytes, dtype=torch.uint8, device=dev), torch.empty(nbytes, dtype=torch.uint8, device=dev)
    cs.zero_()
    dsp.membw_probe(1, cd, cs, nbytes)
    copy_s = statistics.median(window(lambda: dsp.membw_probe(1, cd, cs, nbytes)) for _ in range(nwin))
    copy_rate = 2.0 * nbytes / copy_s
    del cs, cd
    torch.cuda.empty_cache()
    print(json.dumps(dict(copy_bytes=nbytes, copy_ms=copy_s * 1e3, copy_rate_bytes_per_s=copy_rate)), flush=True)

    rows = []
    for s, T in CASES:
        w, h = pkg.TX_W[s], pkg.TX_H[s]
        n = ((PIC_W + w - 1) // w) * ((PIC_H + h - 1) // h)
        n = max(n // 16, 1) if a.quick else n
        types = [t for t in range(16) if t in (0, 9) or max(w, h) < 32][:T]
        assert len(types) == T
        nc = w * h
        src = torch.randint(0, 256, (n, h, w), dtype=torch.uint8, device=dev, generator=g)
        pred = (src.to(torch.int16) + torch.randint(-10, 11, (n, h, w), dtype=torch.int16, device=dev, generator=g)).clamp_(0, 255).to(torch.uint8)
        iscan = torch.from_numpy(np.stack([pkg.tables.scan_tables(s, t)[1] for t in types]).astype(np.int16)).to(dev)
        dist = torch.empty((n, T, 2), dtype=torch.int64, device=dev)
        eob = torch.empty((n, T), dtype=torch.int16, device=dev)
        q = torch.empty((n, T, nc), dtype=torch.int32, device=dev)
        bits = torch.empty((n, T), dtype=torch.int64, device=dev)
        fl = dsp.make_full_loop_groups([dict(src=src, pred=pred, nblocks=n, tx_size=s, tx_types=types, iscan=iscan, dist=dist, eob=eob, qcoeff=q)])
        keep = dict(tx_size=s, tx_types=types, nblocks=n, qcoeff=q, eob=eob, iscan=iscan,
                    txb_skip_ctx=torch.from_numpy(rng.integers(0, 13, n).astype(np.uint8)).to(dev),
                    dc_sign_ctx=torch.from_numpy(rng.integers(0, 3, n).astype(np.uint8)).to(dev),
                    coeff_cost=torch.from_numpy(rng.integers(0, 4096, pkg.COEFF_COST_WORDS).astype(np.int32)).to(dev),
                    eob_cost=torch.from_numpy(rng.integers(0, 4096, pkg.EOB_COST_WORDS).astype(np.int32)).to(dev), bits=bits)
        cr = dsp.make_coeff_rate_groups([keep])

        def full_loop():
            rc = dsp.full_loop_frame(fl, qrow, 1)
            assert rc == 0, dsp.lib.svt_hip_last_error()

        def rate():
            rc = dsp.coeff_rate_frame(cr)
            assert rc == 0, dsp.lib.svt_hip_last_error()

        full_loop(); rate(); torch.cuda.synchronize()          # warm-up of both shapes; the rate call reads the full loop's output
        e = eob.view(torch.int16).to(torch.int32) & 0xffff
        tf, tr = [], []
        for _ in range(nwin):
            tf.append(window(full_loop)); tr.append(window(rate))
        mf, mr = statistics.median(tf), statistics.median(tr)
        qbytes = 4.0 * n * T * nc
        traffic_s = qbytes / copy_rate
        row = dict(tx_size=pkg.TX_SIZE_NAMES[s], nblocks=n, ntypes=T, mean_eob=float(e.float().mean()), eob_zero_fraction=float((e == 0).float().mean()),
                   coeff_rate_ms=mr * 1e3, full_loop_ms=mf * 1e3, rate_over_full_loop=mr / mf, qcoeff_bytes=qbytes,
                   traffic_only_ms=traffic_s * 1e3, traffic_only_fraction=traffic_s / mr, pairs_per_s=n * T / mr,
                   coeff_rate_ms_windows=[x * 1e3 for x in tr], full_loop_ms_windows=[x * 1e3 for x in tf])
        rows.append(row)
        print(json.dumps({k: (round(v, 4) if isinstance(v, float) else v) for k, v in row.items() if not k.endswith("windows")}), flush=True)
        del src, pred, q, dist, eob, bits, keep, fl, cr
        torch.cuda.empty_cache()
    out = dict(device=dsp.device_name(), picture=[PIC_W, PIC_H], qindex=120, quick=a.quick, copy_bytes=nbytes, copy_ms=copy_s * 1e3,
               copy_rate_bytes_per_s=copy_rate, traffic_only="4 B per coefficient of d_qcoeff over the copy rate (2 * bytes / time of svt_hip_membw_probe mode 1)",
               cases=rows)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    json.dump(out, open(a.out, "w"), indent=1)
    print("wrote", a.out)


if __name__ == "__main__":
    main()

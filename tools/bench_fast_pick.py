#!/usr/bin/env python3
"""The end of the intra fast loop on the device (svt_hip_fast_pick_frame) and the one-call fast search
(svt_hip_intra_fast_search_frame), on the luma blocks of a 1080p picture (1920 x 1080) at 8x8 and 32x32 with the 61-candidate list, at
nfl (full_recon_search_count) 3 and 12, SAD, I slice, random edges and sources, random rate tables.

Per case, three things are timed in one process:
  pick      svt_hip_fast_pick_frame on the fast loop's distortions and predictions: costs, the walk, both index arrays, the gather of
            the n survivors' predictions and the repeated origins
  search    svt_hip_intra_fast_search_frame: fast loop -> pick, distortions and predictions in the scratch
  host      the path a caller has without the call, on the same data: svt_hip_intra_fast_loop_frame, a D2H copy of the distortions,
            np_fast_pick (tests/golden/make_golden_fast_pick.py, numpy) on the host, an H2D copy of the indices, a torch gather of the
            predictions and the repeated origins.  fast_loop_ms is the fast loop alone, so host - fast_loop is what the pick replaces.
Before anything is timed the pick's outputs are compared with np_fast_pick's on the same distortions.

And for the pick: its algorithmic bytes from the shapes (ncand * 8 of distortions and 8 of context in per block, n * W * H of predictions
in and out, n * (1 + 1 + 8 + 8 + 4) + 8 of results out), those bytes over the box's copy rate as svt_hip_membw_probe (mode 1) measures it
in the same run (2 * bytes / time), and the fraction traffic-only time / measured time.

Timing: HIP events around windows of back-to-back calls, synchronised before and after, each window >= 0.2 s (the host path: at least one
call) after a warm-up call; the three alternate window by window, 5 windows each, median.  Writes profiles/r12_fast_pick.json.
    python tools/bench_fast_pick.py [--out profiles/r12_fast_pick.json] [--quick]"""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
import __graft_entry__ as ge  # noqa: E402
import make_golden_fast_pick as mg  # noqa: E402

PIC_W, PIC_H = 1920, 1080
CASES = [(1, 3), (1, 12), (3, 3), (3, 12)]          # (tx_size, nfl)
LAMBDA = 29041
SAD, FLAVOUR_C = 0, 0


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


def candidate_list():
    modes, deltas = [], []
    for m in range(13):
        for k in (range(7) if 1 <= m <= 8 else range(1)):
            modes.append(m); deltas.append(k - 3 if 1 <= m <= 8 else 0)
    return modes, deltas


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r12_fast_pick.json"))
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--quick", action="store_true", help="1/16 of the blocks, 3 windows (a smoke run)")
    a = ap.parse_args()
    pkg = ge.load_package()
    dsp = pkg.SvtHipDsp(0)
    dev = torch.device("cuda:0")
    nwin = 3 if a.quick else a.windows
    rng = np.random.default_rng(12031)
    D = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev)
    E = lambda shape, dt: torch.empty(shape, dtype=dt, device=dev)
    ok = lambda rc: rc == 0 or sys.exit(dsp.lib.svt_hip_last_error())

    # the box's copy rate, this run
    nbytes = (64 << 20) if a.quick else (1 << 30)
    cs, cd = E(nbytes, torch.uint8), E(nbytes, torch.uint8)
    cs.zero_()
    dsp.membw_probe(1, cd, cs, nbytes)
    copy_s = statistics.median(window(lambda: dsp.membw_probe(1, cd, cs, nbytes)) for _ in range(nwin))
    copy_rate = 2.0 * nbytes / copy_s
    del cs, cd
    torch.cuda.empty_cache()
    print(json.dumps(dict(copy_bytes=nbytes, copy_ms=copy_s * 1e3, copy_rate_bytes_per_s=copy_rate)), flush=True)

    modes, deltas = candidate_list()
    C = len(modes)
    rates = mg.make_rates("rand", rng)
    rows = []
    for s, nfl in CASES:
        w, h = pkg.TX_W[s], pkg.TX_H[s]
        n = ((PIC_W + w - 1) // w) * ((PIC_H + h - 1) // h)
        n = max(n // 16, 1) if a.quick else n
        N = min(nfl, C)
        pitch = 1 + 2 * 64 + 15
        top, left = rng.integers(0, 256, (n, pitch)).astype(np.uint8), rng.integers(0, 256, (n, pitch)).astype(np.uint8)
        fblk = np.stack([np.zeros(n), np.zeros(n), rng.integers(0, 2, n), np.zeros(n), np.full(n, w), np.zeros(n), np.full(n, h), np.zeros(n)], 1).astype(np.uint8)
        src = np.clip(top[:, 1:1 + w][:, None, :].astype(np.int64) + rng.integers(-20, 21, (n, h, w)), 0, 255).astype(np.uint8)
        xy = (np.arange(n, dtype=np.uint32) % 240 * 8 | (np.arange(n, dtype=np.uint32) // 240 * 8) << 16).astype(np.uint32).view(np.int32)
        bsize, bsize_uv = mg.bsizes_of_tx(s)
        P = dict(tx_size=s, bsize=bsize, bsize_uv=bsize_uv, modes=np.array(modes, np.uint8), deltas=np.array(deltas, np.int8), uv_modes=np.zeros(C, np.uint8),
                 uv_deltas=np.zeros(C, np.int8), use_angle_delta=1, nfl=nfl, slice_is_intra=1, ac_dequant_q3=0, intrabc_bits=0, metric=SAD)
        P["lambda"] = LAMBDA
        pblk = np.zeros(n, mg.BLK_DTYPE)
        pblk["top_mode"], pblk["left_mode"], pblk["has_chroma"] = rng.integers(0, 13, n), rng.integers(0, 13, n), 1
        luma = dict(src=D(src), top=D(top), left=D(left), blocks=D(fblk), nblocks=n, tx_size=s, modes=modes, deltas=deltas)
        kept = dict(luma, dist=E((n, C), torch.int64), pred=E((n, C, h, w), torch.uint8))
        pick = dict(tx_size=s, bsize=bsize, bsize_uv=bsize_uv, nblocks=n, modes=modes, deltas=deltas, uv_modes=[0] * C, uv_deltas=[0] * C, use_angle_delta=1, nfl=nfl,
                    slice_is_intra=1, blk=D(pblk.view(np.uint8).reshape(-1, 8)), rates=D(rates), dist=kept["dist"], pred=kept["pred"], src_xy=D(xy),
                    cand=E((n, N), torch.uint8), sorted=E((n, N), torch.uint8), cost=E((n, N), torch.int64), rate=E((n, N, 2), torch.int32),
                    ref_fast_cost=E((n,), torch.int64), pred_out=E((n, N, h, w), torch.uint8), src_xy_out=E((n, N), torch.int32))
        pick["lambda"] = LAMBDA
        pick2 = {k: (v.clone() if k in pkg.SvtHipDsp.FAST_PICK_OUTPUTS else v) for k, v in pick.items() if k not in ("dist", "pred")}
        fl_arr, fp_arr = dsp.make_fast_loop_groups([kept]), dsp.make_fast_pick_groups([pick])
        fs_groups = [dict(luma=luma, pick=pick2)]
        fs_arr = dsp.make_intra_fast_search_groups(fs_groups)
        scratch = E((max(dsp.intra_fast_search_scratch_bytes(fs_arr), 16),), torch.uint8)
        rows_i = torch.arange(n, device=dev).view(n, 1)

        def fast_loop():
            ok(dsp.intra_fast_loop_frame(fl_arr, SAD, FLAVOUR_C))

        def pick_only():
            ok(dsp.fast_pick_frame(fp_arr, SAD))

        def search():
            ok(dsp.intra_fast_search_frame(fs_arr, SAD, scratch, FLAVOUR_C))

        def host_path():
            fast_loop()
            dist = kept["dist"].cpu().numpy().view(np.uint64)
            res = mg.np_fast_pick(P, dist, None, None, pblk, rates)
            cand = torch.from_numpy(res["cand"]).to(dev).long()
            return res, kept["pred"][rows_i, cand], pick["src_xy"].view(n, 1).expand(n, N).contiguous()

        fast_loop(); pick_only(); search(); torch.cuda.synchronize()       # warm-up
        res, hp, hxy = host_path()
        torch.cuda.synchronize()
        for k, v in res.items():
            if k != "all_cost":
                got = pick[k].cpu().numpy()
                assert np.array_equal(got.view(v.dtype) if got.dtype != v.dtype else got, v), ("pick against np_fast_pick", k)
        assert torch.equal(hp, pick["pred_out"]) and torch.equal(hxy, pick["src_xy_out"])
        for k in pkg.SvtHipDsp.FAST_PICK_OUTPUTS:
            if pick.get(k) is not None:
                assert torch.equal(pick[k], pick2[k]), ("search against pick", k)
        pk_w, se_w, ho_w, fl_w = [], [], [], []
        for _ in range(nwin):
            pk_w.append(window(pick_only)); se_w.append(window(search)); fl_w.append(window(fast_loop)); ho_w.append(window(host_path, 0.0))
        m = statistics.median
        read_b = n * (C * 8 + 8) + n * N * w * h
        write_b = n * N * (1 + 1 + 8 + 8 + 4) + n * 8 + n * N * w * h
        traffic_s = (read_b + write_b) / copy_rate
        row = dict(tx_size=pkg.TX_SIZE_NAMES[s], nblocks=n, ncand=C, nfl=nfl, pick_ms=m(pk_w) * 1e3, search_ms=m(se_w) * 1e3, fast_loop_ms=m(fl_w) * 1e3,
                   host_path_ms=m(ho_w) * 1e3, host_path_minus_fast_loop_ms=(m(ho_w) - m(fl_w)) * 1e3, search_minus_fast_loop_ms=(m(se_w) - m(fl_w)) * 1e3,
                   pick_at_least_as_fast_as_host=bool(m(pk_w) <= m(ho_w) - m(fl_w)),
                   pick_read_bytes=read_b, pick_write_bytes=write_b, traffic_only_ms=traffic_s * 1e3, traffic_only_fraction=traffic_s / m(pk_w),
                   pick_ms_windows=[x * 1e3 for x in pk_w], search_ms_windows=[x * 1e3 for x in se_w], fast_loop_ms_windows=[x * 1e3 for x in fl_w],
                   host_path_ms_windows=[x * 1e3 for x in ho_w])
        rows.append(row)
        print(json.dumps({k: (round(v, 4) if isinstance(v, float) else v) for k, v in row.items() if not k.endswith("windows")}), flush=True)
        del luma, kept, pick, pick2, fl_arr, fp_arr, fs_arr, fs_groups, scratch, res, hp, hxy
        torch.cuda.empty_cache()
    out = dict(device=dsp.device_name(), picture=[PIC_W, PIC_H], metric="SAD", lambda_=LAMBDA, quick=a.quick, copy_bytes=nbytes, copy_ms=copy_s * 1e3,
               copy_rate_bytes_per_s=copy_rate,
               traffic_only="(ncand * 8 + 8 B per block in, n * W * H in and out, n * 22 + 8 B per block out) over the copy rate (2 * bytes / time of "
                            "svt_hip_membw_probe mode 1)",
               host_path="fast loop + D2H of the distortions + np_fast_pick (numpy, one host thread) + H2D of the indices + torch gather",
               cases=rows)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    json.dump(out, open(a.out, "w"), indent=1)
    print("wrote", a.out)


if __name__ == "__main__":
    main()

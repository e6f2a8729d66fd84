#!/usr/bin/env python3
"""The CfL alpha search (svt_hip_cfl_search_frame, svt_hip_cfl_decide_frame) on the chroma blocks of a 1080p 4:2:0 picture (chroma planes
960 x 540) at 8x8, 16x16 and 4x4, each size tiling the plane, qindex 100, one quantiser row set for both planes (the composition's
one full-loop call takes one).  Luma = a smooth field + noise, chroma source = a multiple of the luma AC + noise, DC prediction = the
block's rounded mean +- 3.

Per size, two ways to the same (block, plane, alpha) table are timed in one process:
  search        svt_hip_cfl_search_frame
  composition   the entry points that exist without it: svt_hip_cfl_luma_subsampling_420_batch (with subtract_average) once, 66
                svt_hip_cfl_predict_batch launches that write every candidate prediction to memory (33 candidate planes stacked per
                chroma plane), one svt_hip_full_loop_frame over nblocks x 66 blocks that reads them back, one svt_hip_coeff_rate_frame
The two tables (dist, eob, bits) are compared with each other before anything is timed.  Also recorded: the decide call's time on
that table, the search call's scratch bytes, its algorithmic bytes from the shapes (per block the 4 W H luma samples, 2 W H source and
2 W H prediction samples and 4 context bytes in; per candidate 16 + 8 + 2 table bytes out, and 4 W H + 2 scratch bytes written by the
search kernel and read by the rate kernel), and the registers, LDS and scratch of the new kernels as tools/kernel_resources.py reads them
(--resources: a JSON that tool wrote; without it the tool is run here, which compiles the library's units once more).

Timing: HIP events around windows of back-to-back calls, synchronised before and after, each window >= 0.2 s after a warm-up call; the
two alternate window by window, 7 windows each, median.  A ratio is claimed only where the two medians differ by more than the larger
window-to-window spread (max - min) of the two.  Writes profiles/r10_cfl_search.json.
    python tools/bench_cfl_search.py [--out profiles/r10_cfl_search.json] [--resources kernel_resources.json] [--quick]"""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import __graft_entry__ as ge  # noqa: E402
from bench_tx_search import compare, window  # noqa: E402

CW, CH = 960, 540
SIZES = (1, 2, 0)                                    # TX_8X8, TX_16X16, TX_4X4
NALPHA, QINDEX, LAMBDA = 33, 100, 15000


def alpha_of(a):
    return 0 if a == 0 else (-a if a <= 16 else a - 16)


def picture(rng):
    """luma uint8 [2 CH, 2 CW], chroma source planes uint8 [2][CH, CW]"""
    yy, xx = np.mgrid[0:2 * CH, 0:2 * CW]
    lum = 128 + 50 * np.sin(xx / 37.0) * np.cos(yy / 23.0) + 25 * np.sin((xx + 2 * yy) / 9.0) + rng.integers(-3, 4, (2 * CH, 2 * CW))
    luma = np.clip(np.rint(lum), 0, 255).astype(np.uint8)
    ds = luma.astype(np.float64).reshape(CH, 2, CW, 2).sum((1, 3)) / 4
    src = [np.clip(np.rint(m + k * (ds - 128) + rng.integers(-2, 3, (CH, CW))), 0, 255).astype(np.uint8) for m, k in ((110, 0.5), (140, -0.75))]
    return luma, src


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r10_cfl_search.json"))
    ap.add_argument("--windows", type=int, default=7)
    ap.add_argument("--resources", help="JSON written by tools/kernel_resources.py --json")
    ap.add_argument("--quick", action="store_true", help="the top 1/8 of the picture, 3 windows (a smoke run)")
    a = ap.parse_args()
    pkg = ge.load_package()
    dsp = pkg.SvtHipDsp(0)
    qrow = {k: np.ascontiguousarray(v[QINDEX]) for k, v in pkg.tables.quant_tables(8).items()}
    dev = torch.device("cuda:0")
    nwin = 3 if a.quick else a.windows
    rng = np.random.default_rng(13700)
    luma_np, src_np = picture(rng)
    luma = torch.from_numpy(luma_np).to(dev)
    src = [torch.from_numpy(p).to(dev) for p in src_np]
    E = lambda shape, dt: torch.empty(shape, dtype=dt, device=dev)
    ok = lambda rc: rc == 0 or sys.exit(dsp.lib.svt_hip_last_error())
    rows = []
    for s in SIZES:
        w, h = pkg.TX_W[s], pkg.TX_H[s]
        nc = w * h
        bx, by = CW // w, (CH // h) // (8 if a.quick else 1)
        n = bx * by
        hc = by * h                                                            # rows of the chroma planes the blocks cover
        xs, ys = np.meshgrid(np.arange(bx) * w, np.arange(by) * h)
        xy_np = (xs.reshape(-1) | (ys.reshape(-1) << 16)).astype(np.int32)
        xy = torch.from_numpy(xy_np).to(dev)
        # DC predictions: the block's rounded mean +- 3
        pred = []
        for p in range(2):
            m = src_np[p][:hc].reshape(by, h, bx, w).mean((1, 3))
            pred.append(torch.from_numpy(np.ascontiguousarray(np.repeat(np.repeat(np.clip(np.rint(m) + rng.integers(-3, 4, m.shape), 0, 255), h, 0), w, 1).astype(np.uint8))).to(dev))
        skip = [torch.from_numpy(rng.integers(0, 13, n).astype(np.uint8)).to(dev) for _ in range(2)]
        dcs = [torch.from_numpy(rng.integers(0, 3, n).astype(np.uint8)).to(dev) for _ in range(2)]
        coeff_cost = torch.from_numpy(rng.integers(0, 4096, pkg.COEFF_COST_WORDS).astype(np.int32)).to(dev)
        eob_cost = torch.from_numpy(rng.integers(0, 4096, pkg.EOB_COST_WORDS).astype(np.int32)).to(dev)
        iscan = torch.from_numpy(pkg.tables.scan_tables(s, 0)[1].astype(np.int16)).to(dev)

        # ---- the new call ----
        sg = dict(tx_size=s, tx_type=0, nblocks=n, luma=luma, luma_stride=2 * CW, src=tuple(src), src_stride=(CW, CW), pred=tuple(pred),
                  pred_stride=(CW, CW), xy=xy, iscan=iscan, txb_skip_ctx=tuple(skip), dc_sign_ctx=tuple(dcs), coeff_cost=coeff_cost, eob_cost=eob_cost,
                  dist=E((n, 2, NALPHA, 2), torch.int64), bits=E((n, 2, NALPHA), torch.int64), eob=E((n, 2, NALPHA), torch.int16))
        sga = dsp.make_cfl_search_groups([sg])
        scratch_bytes = dsp.cfl_search_scratch_bytes(sga)
        scratch = E((scratch_bytes,), torch.uint8)
        dg = dict(nblocks=n, dist=sg["dist"], bits=sg["bits"], alpha_rate=torch.from_numpy(rng.integers(200, 3001, (8, 2, 16)).astype(np.int32)).to(dev),
                  cfl_mode_bits=torch.full((n,), 3000, dtype=torch.int32, device=dev), dc_mode_bits=torch.full((n,), 300, dtype=torch.int32, device=dev),
                  decision=E((n, 32), torch.uint8), alpha_q3_cb=E((n,), torch.int32), alpha_q3_cr=E((n,), torch.int32))
        dg["lambda"] = LAMBDA
        dga = dsp.make_cfl_decide_groups([dg])

        def search():
            ok(dsp.cfl_search_frame(sga, qrow, qrow, scratch, 1))

        def decide():
            ok(dsp.cfl_decide_frame(dga))

        # ---- the composition: candidate a of plane p is plane a of a stack of 33 ----
        xy_luma = torch.from_numpy(((xs.reshape(-1) * 2) | ((ys.reshape(-1) * 2) << 16)).astype(np.int32)).to(dev)
        q3 = torch.zeros((n, 32, 32), dtype=torch.int16, device=dev)
        stack = [E((NALPHA, hc, CW), torch.uint8) for _ in range(2)]
        alphas = [torch.full((n,), alpha_of(k), dtype=torch.int32, device=dev) for k in range(NALPHA)]
        cand_xy = torch.from_numpy(np.concatenate([xs.reshape(-1) | ((ys.reshape(-1) + k * hc) << 16) for k in range(NALPHA)]).astype(np.int32)).to(dev)
        src_xy = xy.repeat(NALPHA)
        fl, cr = [], []
        for p in range(2):
            g = dict(tx_size=s, tx_types=[0], nblocks=NALPHA * n, src=src[p], src_stride=CW, src_xy=src_xy, pred=stack[p], pred_stride=CW, pred_xy=cand_xy,
                     iscan=iscan.view(1, nc), dist=E((NALPHA * n, 1, 2), torch.int64), eob=E((NALPHA * n, 1), torch.int16),
                     qcoeff=E((NALPHA * n, 1, nc), torch.int32), bits=E((NALPHA * n, 1), torch.int64), txb_skip_ctx=skip[p].repeat(NALPHA),
                     dc_sign_ctx=dcs[p].repeat(NALPHA), coeff_cost=coeff_cost, eob_cost=eob_cost)
            fl.append(g); cr.append(g)
        fla, cra = dsp.make_full_loop_groups(fl), dsp.make_coeff_rate_groups(cr)

        def composition():
            dsp.cfl_luma_subsampling_420(luma, 2 * CW, 2 * w, 2 * h, xy=xy_luma, subtract_average=True, q3=q3)
            for p in range(2):
                for k in range(NALPHA):
                    dsp.cfl_predict(q3, pred[p], CW, stack[p][k], CW, alphas[k], 8, w, h, xy=xy)
            ok(dsp.full_loop_frame(fla, qrow, 1)); ok(dsp.coeff_rate_frame(cra))

        search(); composition(); decide(); torch.cuda.synchronize()          # warm-up; the tables now hold both results
        for key in ("dist", "eob", "bits"):
            mine = sg[key].view(n, 2, NALPHA, -1)
            theirs = torch.stack([fl[p][key].view(NALPHA, n, -1) for p in range(2)]).permute(2, 0, 1, 3)
            assert torch.equal(mine, theirs), f"size {s}: the two tables differ in {key}"
        dec = dg["decision"].cpu().numpy().view(np.dtype(pkg.SvtHipDsp.CFL_DECISION_DTYPE)).reshape(-1)
        se_w, co_w, de_w = [], [], []
        for _ in range(nwin):
            se_w.append(window(search)); co_w.append(window(composition)); de_w.append(window(decide))
        m_search, m_comp, spread, ratio = compare(se_w, co_w)
        cands = n * 2 * NALPHA
        in_b, out_b, scratch_b = n * (8 * w * h + 4), cands * 26, cands * (4 * nc + 2)
        row = dict(tx_size=pkg.TX_SIZE_NAMES[s], nblocks=n, candidates=cands, cfl_wins=float((dec["uv_mode"] == 13).mean()),
                   eob_0_entries=float((sg["eob"] == 0).float().mean()),
                   search_ms=m_search * 1e3, composition_ms=m_comp * 1e3, spread_ms=spread * 1e3, composition_over_search=ratio,
                   search_not_slower=bool(m_search <= m_comp + spread), decide_ms=statistics.median(de_w) * 1e3,
                   scratch_bytes=scratch_bytes, input_bytes=in_b, table_bytes=out_b, scratch_bytes_written_and_read=scratch_b,
                   algorithmic_bytes=in_b + out_b + 2 * scratch_b,
                   composition_prediction_bytes_written_and_read=cands * nc,
                   search_ms_windows=[x * 1e3 for x in se_w], composition_ms_windows=[x * 1e3 for x in co_w], decide_ms_windows=[x * 1e3 for x in de_w])
        rows.append(row)
        print(json.dumps({k: (round(v, 4) if isinstance(v, float) else v) for k, v in row.items() if not k.endswith("windows")}), flush=True)
        del sg, dg, sga, dga, scratch, q3, stack, fl, cr, fla, cra, cand_xy, src_xy, alphas
        torch.cuda.empty_cache()
    if a.resources:
        res = json.load(open(a.resources))
    else:
        import kernel_resources
        res = kernel_resources.collect()
    kernels = [{k: r[k] for k in ("kernel", "vgprs", "agprs", "sgprs", "lds", "scratch", "occupancy")} for r in res
               if "cfl_search_kernel" in r["kernel"] or "cfl_decide_kernel" in r["kernel"]]
    assert len(kernels) == 2 and not any(k["scratch"] for k in kernels), kernels
    out = dict(device=dsp.device_name(), chroma_planes=[CW, CH], qindex=QINDEX, lambda_=LAMBDA, quick=a.quick,
               composition="cfl_luma_subsampling_420 (subtract_average) + 66 cfl_predict_batch + full_loop_frame (2 groups) + coeff_rate_frame (2 groups)",
               ratios="claimed only where the medians differ by more than the larger max - min of the two window lists; null otherwise",
               kernels=kernels, cases=rows)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    json.dump(out, open(a.out, "w"), indent=1)
    print("wrote", a.out)
    assert all(r["search_not_slower"] for r in rows), "the search call is slower than the composition by more than the spread"


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""The transform-type decision (svt_hip_tx_decide_frame) and the one-call search (svt_hip_tx_search_frame), on the cases of
tools/bench_coeff_rate.py: the luma transform blocks of a 1080p picture (1920 x 1080) at 8x8, 16x16 and 32x32, with 1 and with 16
transform types (32x32 defines 2: DCT_DCT and IDTX), tables and coefficients from the full loop and the rate call on pred = src + small
noise, qindex 120.

Per case, four things are timed in one process:
  decide    svt_hip_tx_decide_frame with both coefficient arrays gathered
  torch     the same decision and gather written with torch ops on the device from the same tables: what a caller does without the call
            (cost, skip mask, argmin, five gathers for the record, two indexed gathers of coefficients with their zero fill).  It computes
            in int64, which is exact for these inputs (nothing wraps here); its argmin does not promise the first of equal costs.  Before
            anything is timed its cost, winner, record fields and both gathers are compared with the call's output (the position-dependent
            ones on the blocks whose smallest cost is not tied)
  search    svt_hip_tx_search_frame, the caller keeping the per-type arrays
  by_hand   the same three calls enqueued by the caller
and for the decide call: its algorithmic bytes from the shapes (every (block, type) entry of dist / eob / bits once, the winner's
coefficients of both arrays in and out, the 40-byte record; winners with eob 0 are not read, their share is reported), the traffic-only
time, those bytes over the box's copy rate as svt_hip_membw_probe (mode 1, copy) measures it in the same run (2 * bytes / time), and
the fraction traffic-only time / measured time.

Timing: HIP events around windows of back-to-back calls, synchronised before and after, each window >= 0.2 s after a warm-up call;
the four alternate window by window, 7 windows each, median.  A ratio is claimed only where the two medians differ by more than the
larger window-to-window spread (max - min) of the two.  Writes profiles/r09_tx_search.json.
    python tools/bench_tx_search.py [--out profiles/r09_tx_search.json] [--quick]"""
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
LAMBDA = 29041


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


def compare(a, b):
    """medians of two window lists, their spreads, and b / a where the difference is larger than the larger spread (else None)"""
    ma, mb = statistics.median(a), statistics.median(b)
    spread = max(max(a) - min(a), max(b) - min(b))
    return ma, mb, spread, (mb / ma if abs(mb - ma) > spread else None)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r09_tx_search.json"))
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
        E = lambda shape, dt: torch.empty(shape, dtype=dt, device=dev)
        keep = dict(tx_size=s, tx_types=types, nblocks=n, src=src, pred=pred,
                    iscan=torch.from_numpy(np.stack([pkg.tables.scan_tables(s, t)[1] for t in types]).astype(np.int16)).to(dev),
                    dist=E((n, T, 2), torch.int64), eob=E((n, T), torch.int16), qcoeff=E((n, T, nc), torch.int32), dqcoeff=E((n, T, nc), torch.int32),
                    bits=E((n, T), torch.int64),
                    txb_skip_ctx=torch.from_numpy(rng.integers(0, 13, n).astype(np.uint8)).to(dev),
                    dc_sign_ctx=torch.from_numpy(rng.integers(0, 3, n).astype(np.uint8)).to(dev),
                    coeff_cost=torch.from_numpy(rng.integers(0, 4096, pkg.COEFF_COST_WORDS).astype(np.int32)).to(dev),
                    eob_cost=torch.from_numpy(rng.integers(0, 4096, pkg.EOB_COST_WORDS).astype(np.int32)).to(dev),
                    decision=E((n, 40), torch.uint8), best_qcoeff=E((n, nc), torch.int32), best_dqcoeff=E((n, nc), torch.int32))
        keep["lambda"] = LAMBDA
        fl, cr, td, ts = dsp.make_full_loop_groups([keep]), dsp.make_coeff_rate_groups([keep]), dsp.make_tx_decide_groups([keep]), dsp.make_tx_search_groups([keep])
        scratch = E((max(dsp.tx_search_scratch_bytes(ts), 16),), torch.uint8)
        ok = lambda rc: rc == 0 or sys.exit(dsp.lib.svt_hip_last_error())

        def decide():
            ok(dsp.tx_decide_frame(td))

        def by_hand():
            ok(dsp.full_loop_frame(fl, qrow, 1)); ok(dsp.coeff_rate_frame(cr)); ok(dsp.tx_decide_frame(td))

        def search():
            ok(dsp.tx_search_frame(ts, qrow, scratch, 1))

        dist, eob, bits, q, dq = keep["dist"], keep["eob"], keep["bits"], keep["qcoeff"], keep["dqcoeff"]
        not_dct = torch.tensor([t != 0 for t in types], device=dev).view(1, T)
        rows_i = torch.arange(n, device=dev)
        never = torch.iinfo(torch.int64).max

        def torch_ops():
            cost = ((bits * LAMBDA + 256) >> 9) + dist[:, :, 0] * 128
            cost = torch.where((eob == 0) & not_dct, never, cost)
            best, win = cost.min(dim=1)
            weob = eob[rows_i, win]
            rec = (best, dist[rows_i, win], bits[rows_i, win], weob, win)
            zero = (weob == 0).view(n, 1)
            bq = q[rows_i, win].masked_fill_(zero, 0)
            bdq = dq[rows_i, win].masked_fill_(zero, 0)
            return rec, bq, bdq

        by_hand(); search(); torch.cuda.synchronize()      # warm-up; the tables now hold the chain's results
        rec, bq, bdq = torch_ops()
        torch.cuda.synchronize()
        d = keep["decision"].cpu().numpy().view(np.dtype(pkg.SvtHipDsp.TX_DECISION_DTYPE)).reshape(-1)
        # the torch composition computes the same decision: cost and the winner's eob / dist / bits do not depend on which of two equal
        # costs wins; the position and both gathers are compared on every block whose smallest cost is not tied
        t_cost, t_dist, t_bits, t_eob, t_win = (x.cpu().numpy() for x in rec)
        c_all = torch.where((eob == 0) & not_dct, never, ((bits * LAMBDA + 256) >> 9) + dist[:, :, 0] * 128)
        untied = ((c_all == c_all.min(dim=1, keepdim=True)[0]).sum(dim=1) == 1).cpu().numpy() & (d["type_index"] != 0xFF)
        assert np.array_equal(t_cost.view(np.uint64), d["cost"]), "torch composition: cost"
        assert np.array_equal(t_win[untied], d["type_index"][untied]) and np.array_equal(t_eob[untied].view(np.uint16), d["eob"][untied]), "torch composition: winner"
        assert np.array_equal(t_dist[untied].view(np.uint64), d["dist"][untied]) and np.array_equal(t_bits[untied].view(np.uint64), d["bits"][untied])
        assert np.array_equal(bq.cpu().numpy()[untied], keep["best_qcoeff"].cpu().numpy()[untied]), "torch composition: best_qcoeff"
        assert np.array_equal(bdq.cpu().numpy()[untied], keep["best_dqcoeff"].cpu().numpy()[untied]), "torch composition: best_dqcoeff"
        assert untied.mean() > 0.9, untied.mean()
        td_w, to_w, se_w, bh_w = [], [], [], []
        for _ in range(nwin):
            td_w.append(window(decide)); to_w.append(window(torch_ops)); se_w.append(window(search)); bh_w.append(window(by_hand))
        m_dec, m_torch, spread_dt, ratio_dt = compare(td_w, to_w)
        m_search, m_hand, spread_sh, ratio_sh = compare(se_w, bh_w)
        pairs = n * T
        read_b = pairs * (16 + 2 + 8) + 2 * n * nc * 4
        write_b = n * 40 + 2 * n * nc * 4
        traffic_s = (read_b + write_b) / copy_rate
        row = dict(tx_size=pkg.TX_SIZE_NAMES[s], nblocks=n, ntypes=T, winners_with_eob_0=float((d["eob"] == 0).mean()), untied_fraction=float(untied.mean()),
                   winners_not_dct=float((d["tx_type"] != 0).mean()),
                   decide_ms=m_dec * 1e3, torch_ops_ms=m_torch * 1e3, decide_vs_torch_spread_ms=spread_dt * 1e3, torch_over_decide=ratio_dt,
                   decide_at_least_as_fast=bool(m_dec <= m_torch),
                   decide_read_bytes=read_b, decide_write_bytes=write_b, traffic_only_ms=traffic_s * 1e3, traffic_only_fraction=traffic_s / m_dec,
                   search_ms=m_search * 1e3, by_hand_ms=m_hand * 1e3, search_vs_by_hand_spread_ms=spread_sh * 1e3, by_hand_over_search=ratio_sh,
                   decide_ms_windows=[x * 1e3 for x in td_w], torch_ops_ms_windows=[x * 1e3 for x in to_w],
                   search_ms_windows=[x * 1e3 for x in se_w], by_hand_ms_windows=[x * 1e3 for x in bh_w])
        rows.append(row)
        print(json.dumps({k: (round(v, 4) if isinstance(v, float) else v) for k, v in row.items() if not k.endswith("windows")}), flush=True)
        del src, pred, keep, fl, cr, td, ts, scratch, dist, eob, bits, q, dq, rec, bq, bdq
        torch.cuda.empty_cache()
    out = dict(device=dsp.device_name(), picture=[PIC_W, PIC_H], qindex=120, lambda_=LAMBDA, quick=a.quick, copy_bytes=nbytes, copy_ms=copy_s * 1e3,
               copy_rate_bytes_per_s=copy_rate,
               traffic_only="(26 B per (block, type) + 40 B per block + the winner's coefficients of two arrays in and out) over the copy rate "
                            "(2 * bytes / time of svt_hip_membw_probe mode 1)",
               ratios="claimed only where the medians differ by more than the larger max - min of the two window lists; null otherwise",
               cases=rows)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    json.dump(out, open(a.out, "w"), indent=1)
    print("wrote", a.out)


if __name__ == "__main__":
    main()

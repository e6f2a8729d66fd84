#!/usr/bin/env python3
"""The decide of mode decision (svt_hip_md_decide_frame) and the one-call search (svt_hip_md_search_frame) on a 1080p 4:2:0 picture
(1920 x 1080), one block per position at 8x8, 16x16 and 32x32, with n = 3 and n = 12 full-loop slots per block and all three gathers on
(prediction, qcoeff and dqcoeff of the three planes, and the inter record).  The per-slot tables are the real chain's: pred = src +
small noise on the three planes, luma types DCT_DCT and IDTX, qindex 120, synthetic contexts, rates and cost tables.

Per case, in one process:
  decide    svt_hip_md_decide_frame, next to its algorithmic bytes from the shapes (every (block, slot) entry of the luma record, the chroma
            dist / bits / eob, the fast rates, the list index, the inter candidate and the CfL record once; the 72-byte record and every
            slot's cost out; the winner's prediction and coefficients of every plane and its inter record in and out) over the box's copy
            rate as svt_hip_membw_probe (mode 1, copy) measures it in the same run (2 * bytes / time), as DESIGN.md 4.27 does
  search    svt_hip_md_search_frame, the caller keeping the stage arrays, next to
  by_hand   the same stages enqueued by the caller (transform-type search, chroma full loop, chroma rate, decide)
  replaced  the path the decide replaces: D2H of the per-slot records, the cost, walk and arg-min in numpy (the project's restatement,
            tests/golden/make_golden_md_decide.py np_md_decide), H2D of the winner's slot, the ten gathers with torch on the device;
            wall-clock, synchronised, median of 3; its records are compared with the call's before anything is timed
Timing of the device calls: HIP events around windows of back-to-back calls, synchronised before and after, each window >= 0.2 s after a
warm-up call; alternating window by window, 7 windows each, median.  A ratio is claimed only where the two medians differ by more than
the larger window-to-window spread (max - min) of the two.  Writes profiles/r18_md_decide.json.
    python tools/bench_md_decide.py [--out profiles/r18_md_decide.json] [--quick]"""
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
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
import __graft_entry__ as ge  # noqa: E402
import make_golden_md_decide as mg  # noqa: E402

PIC_W, PIC_H = 1920, 1080
CASES = [(3, 3), (3, 12), (6, 3), (6, 12), (9, 3), (9, 12)]             # (bsize, n)
TX_OF = {4: 0, 8: 1, 16: 2, 32: 3}
LAMBDA = 29041
NINTER, NINTRA = 6, 7


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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r18_md_decide.json"))
    ap.add_argument("--windows", type=int, default=7)
    ap.add_argument("--quick", action="store_true", help="1/16 of the blocks, 3 windows (a smoke run)")
    a = ap.parse_args()
    pkg = ge.load_package()
    dsp = pkg.SvtHipDsp(0)
    q = pkg.tables.quant_tables(8)
    qrow = {k: np.ascontiguousarray(v[120]) for k, v in q.items()}
    dev = torch.device("cuda:0")
    gen = torch.Generator(device=dev); gen.manual_seed(18018)
    rng = np.random.default_rng(18018)
    nwin = 3 if a.quick else a.windows
    T = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev)
    E = lambda shape, dt: torch.empty(shape, dtype=dt, device=dev)
    ok = lambda rc: rc == 0 or sys.exit(dsp.lib.svt_hip_last_error())

    nbytes = (64 << 20) if a.quick else (1 << 30)
    cs, cd = E(nbytes, torch.uint8), E(nbytes, torch.uint8)
    cs.zero_()
    dsp.membw_probe(1, cd, cs, nbytes)
    copy_s = statistics.median(window(lambda: dsp.membw_probe(1, cd, cs, nbytes)) for _ in range(nwin))
    copy_rate = 2.0 * nbytes / copy_s
    del cs, cd
    torch.cuda.empty_cache()
    print(json.dumps(dict(copy_bytes=nbytes, copy_ms=copy_s * 1e3, copy_rate_bytes_per_s=copy_rate)), flush=True)
    rates_np = mg.make_rates()

    rows = []
    for bsize, n in CASES:
        sizes = pkg.md_plane_sizes(bsize)
        bw, bh = sizes[0][0], sizes[0][1]
        nb = ((PIC_W + bw - 1) // bw) * ((PIC_H + bh - 1) // bh)
        nb = max(nb // 16, 1) if a.quick else nb
        pairs = nb * n
        planes = []
        for p, (w, h, nc) in enumerate(sizes):
            tx = TX_OF[w]
            types = [0, 9] if p == 0 else [0]
            src = torch.randint(0, 256, (nb, 1, h, w), dtype=torch.uint8, device=dev, generator=gen).expand(nb, n, h, w).reshape(pairs, h, w).contiguous()
            pred = (src.to(torch.int16) + torch.randint(-10, 11, (pairs, h, w), dtype=torch.int16, device=dev, generator=gen)).clamp_(0, 255).to(torch.uint8)
            planes.append(dict(tx_size=tx, tx_types=types, nblocks=pairs, src=src, pred=pred,
                               iscan=T(np.stack([pkg.tables.scan_tables(tx, t)[1] for t in types]).astype(np.int16)),
                               txb_skip_ctx=T(rng.integers(0, 13, pairs).astype(np.uint8)), dc_sign_ctx=T(rng.integers(0, 3, pairs).astype(np.uint8)),
                               coeff_cost=T(rng.integers(0, 4096, pkg.COEFF_COST_WORDS).astype(np.int32)),
                               eob_cost=T(rng.integers(0, 4096, pkg.EOB_COST_WORDS).astype(np.int32)),
                               dist=E((pairs, len(types), 2), torch.int64), eob=E((pairs, len(types)), torch.int16),
                               qcoeff=E((pairs, len(types), nc), torch.int32), dqcoeff=E((pairs, len(types), nc), torch.int32),
                               bits=E((pairs, len(types)), torch.int64)))
        luma = planes[0]
        luma["lambda"] = LAMBDA
        luma.update(decision=E((pairs, 40), torch.uint8), best_qcoeff=E((pairs, sizes[0][2]), torch.int32), best_dqcoeff=E((pairs, sizes[0][2]), torch.int32))
        cand = np.stack([rng.permutation(NINTER + NINTRA)[:n] for _ in range(nb)]).astype(np.uint8)
        cand_out = np.zeros((nb, n), mg.CAND_DTYPE); cand_out["flags"] = rng.integers(0, 4, (nb, n))
        cfl = np.zeros((nb, n), mg.CFL_DEC_DTYPE)
        cfl["uv_mode"] = rng.choice([0, 13], (nb, n)); cfl["cfl_alpha_idx"] = rng.integers(0, 256, (nb, n)) * (cfl["uv_mode"] == 13)
        cfl["cfl_alpha_signs"] = rng.integers(0, 8, (nb, n)) * (cfl["uv_mode"] == 13)
        blk = np.zeros(nb, mg.BLK_DTYPE); blk["skip_flag_context"] = rng.integers(0, 3, nb); blk["has_uv"] = 1
        modes = rng.permutation(13)[:NINTRA].astype(np.uint8)
        rate = rng.integers(0, 1 << 12, (nb, n, 2)).astype(np.int32)
        md = dict(bsize=bsize, nblocks=nb, n=n, ninter=NINTER, nintra=NINTRA, modes=modes, slice_is_intra=0, full_loop_escape=1, rate=T(rate), cand=T(cand),
                  cand_out=T(cand_out.view(np.uint8).reshape(nb, n, 16)), cfl=T(cfl.view(np.uint8).reshape(nb, n, 32)), blk=T(blk.view(np.uint8).reshape(nb, 4)),
                  rates=T(rates_np), pred=[pl["pred"] for pl in planes], inter_blk=torch.randint(0, 256, (nb, n, 16), dtype=torch.uint8, device=dev, generator=gen),
                  decision=E((nb, 72), torch.uint8), full_cost=E((nb, n), torch.int64), best_inter_blk=E((nb, 16), torch.uint8),
                  best_pred=[E((nb, w * h), torch.uint8) for w, h, _ in sizes], best_qcoeff=[E((nb, nc), torch.int32) for _, _, nc in sizes],
                  best_dqcoeff=[E((nb, nc), torch.int32) for _, _, nc in sizes])
        md["lambda"] = LAMBDA
        chroma = planes[1:]
        sg = dict(md=md, luma=luma, cb=chroma[0], cr=chroma[1], txb_skip_ctx_c=[c["txb_skip_ctx"] for c in chroma], dc_sign_ctx_c=[c["dc_sign_ctx"] for c in chroma],
                  coeff_cost_uv=chroma[0]["coeff_cost"], eob_cost_uv=chroma[0]["eob_cost"], bits_c=[c["bits"] for c in chroma])
        for c in chroma:                                                   # by hand both planes read the one PLANE_TYPE_UV table, as the call does
            c["coeff_cost"], c["eob_cost"] = chroma[0]["coeff_cost"], chroma[0]["eob_cost"]
        md_hand = dict(md, luma=luma["decision"], dist_cb=chroma[0]["dist"], dist_cr=chroma[1]["dist"], bits_cb=chroma[0]["bits"], bits_cr=chroma[1]["bits"],
                       eob_cb=chroma[0]["eob"], eob_cr=chroma[1]["eob"], qcoeff=[luma["best_qcoeff"], chroma[0]["qcoeff"], chroma[1]["qcoeff"]],
                       dqcoeff=[luma["best_dqcoeff"], chroma[0]["dqcoeff"], chroma[1]["dqcoeff"]])
        ms, ts = dsp.make_md_search_groups([sg]), dsp.make_tx_search_groups([luma])
        flc, crc, mdg = dsp.make_full_loop_groups(chroma), dsp.make_coeff_rate_groups(chroma), dsp.make_md_decide_groups([md_hand])
        scratch = E((max(dsp.md_search_scratch_bytes(ms), 16),), torch.uint8)

        def decide():
            ok(dsp.md_decide_frame(mdg))

        def by_hand():
            ok(dsp.tx_search_frame(ts, qrow, scratch, 1)); ok(dsp.full_loop_frame(flc, qrow, 1)); ok(dsp.coeff_rate_frame(crc)); ok(dsp.md_decide_frame(mdg))

        def search():
            ok(dsp.md_search_frame(ms, qrow, qrow, scratch, 1))

        gin = md_hand["pred"] + md_hand["qcoeff"] + md_hand["dqcoeff"] + [md["inter_blk"]]
        gin = [t.view(nb, n, -1) for t in gin]
        rows_i = torch.arange(nb, device=dev)
        zkeys = {"rates": rates_np, "c0_bsize": bsize, "c0_n": n, "c0_ninter": NINTER, "c0_nintra": NINTRA, "c0_lam": LAMBDA, "c0_slice_is_intra": 0,
                 "c0_escape": 1, "c0_has_chroma": 1, "c0_has_cfl": 1, "c0_modes": modes}

        def replaced():
            """-> (records, the ten gathered arrays)"""
            z = dict(zkeys)
            z["c0_luma"] = luma["decision"].cpu().numpy().reshape(nb, n, 40)
            z["c0_cdist"] = np.stack([c["dist"].cpu().numpy().view(np.uint64).reshape(nb, n, 2) for c in chroma])
            z["c0_cbits"] = np.stack([c["bits"].cpu().numpy().view(np.uint64).reshape(nb, n) for c in chroma])
            z["c0_ceob"] = np.stack([c["eob"].cpu().numpy().view(np.uint16).reshape(nb, n) for c in chroma])
            z["c0_rate"] = md["rate"].cpu().numpy().view(np.uint32)
            z["c0_cand"], z["c0_cand_out"], z["c0_cfl"], z["c0_blk"] = (md[k].cpu().numpy() for k in ("cand", "cand_out", "cfl", "blk"))
            dec, _ = mg.np_md_decide(z, 0)
            slot = torch.from_numpy(dec["slot"].astype(np.int64)).to(dev)
            eob0 = torch.from_numpy(dec["eob"] == 0).to(dev)
            out = []
            for i, t in enumerate(gin):
                o = t[rows_i, slot]
                if 3 <= i < 9:
                    o = o.masked_fill_(eob0[:, i % 3].view(nb, 1), 0)
                out.append(o)
            torch.cuda.synchronize()
            return dec, out

        by_hand(); search(); torch.cuda.synchronize()                      # warm-up; the stage arrays now hold the chain's results
        dec, out = replaced()
        got = md["decision"].cpu().numpy().view(mg.DEC_DTYPE).reshape(-1)
        assert np.array_equal(got, dec), "the replaced path's records"
        outs = md["best_pred"] + md["best_qcoeff"] + md["best_dqcoeff"] + [md["best_inter_blk"]]
        for o, w in zip(outs, out):
            assert torch.equal(o.view(nb, -1), w), "the replaced path's gathers"
        rep = []
        for _ in range(3):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            replaced()
            rep.append(time.perf_counter() - t0)
        de_w, se_w, bh_w = [], [], []
        for _ in range(nwin):
            de_w.append(window(decide)); se_w.append(window(search)); bh_w.append(window(by_hand))
        m_search, m_hand, spread_sh, ratio_sh = compare(se_w, bh_w)
        m_dec, m_rep = statistics.median(de_w), statistics.median(rep)
        per_pair = 40 + 2 * (16 + 8 + 2) + 8 + 1 + 16 + 32
        gather_b = sum(w * h + 2 * 4 * nc for w, h, nc in sizes) + 16
        read_b, write_b = pairs * per_pair + nb * (4 + gather_b), nb * (72 + gather_b) + pairs * 8
        traffic_s = (read_b + write_b) / copy_rate
        row = dict(bsize=f"{bw}x{bh}", nblocks=nb, n=n, escaped_fraction=float((dec["count"] < n).mean()), intra_winners=float(dec["is_intra"].mean()),
                   winners_with_eob_0=[float((dec["eob"][:, p] == 0).mean()) for p in range(3)],
                   decide_ms=m_dec * 1e3, decide_read_bytes=read_b, decide_write_bytes=write_b, traffic_only_ms=traffic_s * 1e3, traffic_only_fraction=traffic_s / m_dec,
                   search_ms=m_search * 1e3, by_hand_ms=m_hand * 1e3, search_vs_by_hand_spread_ms=spread_sh * 1e3, by_hand_over_search=ratio_sh,
                   replaced_ms=m_rep * 1e3, replaced_ms_runs=[x * 1e3 for x in rep], replaced_over_decide=m_rep / m_dec,
                   decide_ms_windows=[x * 1e3 for x in de_w], search_ms_windows=[x * 1e3 for x in se_w], by_hand_ms_windows=[x * 1e3 for x in bh_w])
        rows.append(row)
        print(json.dumps({k: (round(v, 4) if isinstance(v, float) else v) for k, v in row.items() if not k.endswith("windows")}), flush=True)
        del planes, luma, chroma, md, md_hand, sg, ms, ts, flc, crc, mdg, scratch, gin, out, outs
        torch.cuda.empty_cache()
    res = dict(device=dsp.device_name(), picture=[PIC_W, PIC_H], qindex=120, lambda_=LAMBDA, quick=a.quick, copy_bytes=nbytes, copy_ms=copy_s * 1e3,
               copy_rate_bytes_per_s=copy_rate,
               traffic_only="(149 B per (block, slot) in, 8 out; per block 4 B in, the 72-byte record out and the winner's three predictions, six coefficient "
                            "arrays and inter record in and out) over the copy rate (2 * bytes / time of svt_hip_membw_probe mode 1)",
               replaced="D2H of the per-slot records, numpy cost + walk + arg-min, H2D of the slot, ten torch gathers; wall clock, median of 3",
               ratios="by_hand_over_search is claimed only where the medians differ by more than the larger max - min of the two window lists; null otherwise",
               cases=rows)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    json.dump(res, open(a.out, "w"), indent=1)
    print("wrote", a.out)


if __name__ == "__main__":
    main()

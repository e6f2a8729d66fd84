#!/usr/bin/env python3
"""The inter fast search on the device (svt_hip_inter_fast_search_frame) against the path a caller had before it, on a 1080p 4:2:0
picture (1920 x 1080) with one block per position at 8x8, 16x16 and 32x32, 16 and 48 inter candidates per block (no intra tail), nfl
(full_recon_search_count) 3 and 12, SAD, random planes, vectors of a few samples at every phase, random rate tables.

Per case, four things are timed in one process, alternating window by window:
  search    svt_hip_inter_fast_search_frame: distortion-only prediction of every candidate (Y, Cb, Cr) -> pick -> prediction of the n
            survivors (Y, Cb, Cr); the distortions live in the scratch and no candidate's prediction is stored
  baseline  only entry points that existed before: svt_hip_inter_pred_frame storing EVERY candidate's prediction and distortion (Y, Cb,
            Cr), a D2H copy of the distortions, the numpy restatement of cost and walk on the host (tests/test_inter_fast_cpu.np_costs,
            make_golden_fast_pick.np_walk), an H2D copy of the winners, a torch gather of their predictions
  pick      svt_hip_inter_fast_pick_frame alone on the distortions
  dist      the distortion-only svt_hip_inter_pred_frame call it follows
Before anything is timed the search's outputs and predictions are compared with the baseline's.

For the pick: its algorithmic bytes from the shapes (per block ninter * (16 + 16 + 3 * 8) + 16 in, n * (1 + 1 + 8 + 8 + 16 + 16 + 4) + 8
out), those bytes over the box's copy rate as svt_hip_membw_probe (mode 1) measures it in the same run (2 * bytes / time), and the
fraction traffic-only time / measured time.  And what no longer exists: the bytes of the [nblocks][ninter][H][W] prediction arrays (Y, Cb,
Cr) the baseline writes and gathers from, from the shapes.

Timing: HIP events around windows of back-to-back calls, synchronised before and after, each window >= 1 s (the baseline: at least one
call) after a warm-up call; 5 windows each, median; the spread (max - min over the windows) is recorded, and per case whether the search
is faster than the baseline by more than both spreads.  Writes profiles/r16_inter_fast_search.json.
    python tools/bench_inter_fast_search.py [--out profiles/r16_inter_fast_search.json] [--quick]"""
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
sys.path.insert(0, os.path.join(ROOT, "tests"))
import __graft_entry__ as ge  # noqa: E402
import make_golden_fast_pick as fp  # noqa: E402
import make_golden_inter_fast as mg  # noqa: E402
import test_inter_fast_cpu as restated  # noqa: E402

PIC_W, PIC_H = 1920, 1080
PAD = (80, 48)                                      # luma / chroma border, every side (the border contract at 32x32: 40 / 26)
CASES = [(side, ni, nfl) for side in (8, 16, 32) for ni in (16, 48) for nfl in (3, 12)]
BSIZE = {8: (3, 0), 16: (6, 3), 32: (9, 6)}         # (bsize, bsize_uv)
LAMBDA = 29041
SAD = 0


def window(fn, min_s):
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


def make_records(rng, side, nb_x, nb_y, ni):
    """[nb, ni] svt_hip_inter_blk / svt_hip_inter_cand records and [nb] context records, vectorised"""
    nb = nb_x * nb_y
    blk, cand, ctx = np.zeros((nb, ni), mg.BLK_DTYPE), np.zeros((nb, ni), mg.CAND_DTYPE), np.zeros(nb, mg.CTX_DTYPE)
    i = np.arange(nb)
    blk["x"], blk["y"] = ((i % nb_x) * side)[:, None], ((i // nb_x) * side)[:, None]
    mode = rng.integers(13, 25, (nb, ni))
    comp = mode >= 17
    cand["pred_mode"] = mode
    blk["pred_direction"] = np.where(comp, 2, rng.integers(0, 2, (nb, ni)))
    cand["ref_frame_type"] = np.where(comp, rng.integers(8, 20, (nb, ni)), rng.integers(1, 8, (nb, ni)))
    blk["mv"] = rng.integers(-40, 41, (nb, ni, 2, 2))
    cand["pred_mv"] = rng.integers(-40, 41, (nb, ni, 2, 2))
    blk["filter_x"], blk["filter_y"] = rng.integers(0, 3, (nb, ni)), rng.integers(0, 3, (nb, ni))
    cand["mode_ctx"] = rng.integers(0, 6, (nb, ni)) | rng.integers(0, 2, (nb, ni)) << 3 | rng.integers(0, 6, (nb, ni)) << 4
    cand["drl_index"], cand["ref_mv_count"] = rng.integers(0, 3, (nb, ni)), rng.integers(0, 5, (nb, ni))
    cand["drl_ctx"] = rng.integers(0, 3, (nb, ni)) | rng.integers(0, 3, (nb, ni)) << 2 | rng.integers(0, 3, (nb, ni)) << 4
    allowed = rng.integers(0, 3, (nb, ni))
    cand["flags"] = (rng.integers(0, 3, (nb, ni)) == 0) | np.minimum(rng.integers(0, 3, (nb, ni)), allowed) << 1 | allowed << 3
    ctx["skip_flag_context"], ctx["is_inter_ctx"] = rng.integers(0, 3, nb), rng.integers(0, 4, nb)
    ctx["reference_mode_context"], ctx["compoud_reference_type_context"] = rng.integers(0, 5, nb), rng.integers(0, 5, nb)
    for f in mg.CTX_FIELDS[4:]:
        ctx[f] = rng.integers(0, 3, nb)
    ctx["single_ref_p"], ctx["has_uv"] = rng.integers(0, 3, (nb, 6)), 1
    return blk, cand, ctx


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r16_inter_fast_search.json"))
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--quick", action="store_true", help="the top sixteenth of the picture's rows, 2 windows of 0.1 s (a smoke run)")
    a = ap.parse_args()
    pkg = ge.load_package()
    dsp = pkg.SvtHipDsp(0)
    dev = torch.device("cuda:0")
    nwin, min_s = (2, 0.1) if a.quick else (a.windows, 1.0)
    rng = np.random.default_rng(16031)
    D = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev)
    E = lambda shape, dt: torch.empty(shape, dtype=dt, device=dev)
    ok = lambda rc: rc == 0 or sys.exit(dsp.lib.svt_hip_last_error())

    # the box's copy rate, this run
    nbytes = (64 << 20) if a.quick else (1 << 30)
    cs, cd = E(nbytes, torch.uint8), E(nbytes, torch.uint8)
    cs.zero_()
    dsp.membw_probe(1, cd, cs, nbytes)
    copy_s = statistics.median(window(lambda: dsp.membw_probe(1, cd, cs, nbytes), 0.2) for _ in range(nwin))
    copy_rate = 2.0 * nbytes / copy_s
    del cs, cd
    torch.cuda.empty_cache()
    print(json.dumps(dict(copy_bytes=nbytes, copy_ms=copy_s * 1e3, copy_rate_bytes_per_s=copy_rate)), flush=True)

    # the picture: two reference lists and the source, padded
    full = {name: [D(rng.integers(0, 256, ((PIC_H >> (p > 0)) + 2 * PAD[p > 0], (PIC_W >> (p > 0)) + 2 * PAD[p > 0])).astype(np.uint8)) for p in range(3)]
            for name in ("ref0", "ref1", "src")}
    view = {name: [t[PAD[p > 0]:, PAD[p > 0]:] for p, t in enumerate(full[name])] for name in full}
    strides = [t.shape[1] for t in full["src"]]
    rates_np = mg.pack_rates(mg.make_rates(0))
    mvc_np = mg.make_mv_cost()
    rates, mvc = D(rates_np), D(mvc_np)
    rows = []
    for side, ni, nfl in CASES:
        nb_x, nb_y = PIC_W // side, PIC_H // side
        nb_y = max(nb_y // 16, 1) if a.quick else nb_y
        nb = nb_x * nb_y
        n = min(nfl, ni)
        bsize, bsize_uv = BSIZE[side]
        blk_np, cand_np, ctx_np = make_records(rng, side, nb_x, nb_y, ni)
        P = dict(bsize=bsize, bsize_uv=bsize_uv, ninter=ni, nintra=0, nfl=nfl, metric=SAD, ac_dequant_q3=0, reference_mode_select=1, switchable_motion_mode=1)
        P["lambda"] = LAMBDA
        blk, cand_in, ctx = D(blk_np.view(np.uint8).reshape(nb, ni, 16)), D(cand_np.view(np.uint8).reshape(nb, ni, 16)), D(ctx_np.view(np.uint8).reshape(nb, 16))
        hw = [(side >> (p > 0), side >> (p > 0)) for p in range(3)]
        outs = lambda: dict(cand=E((nb, n), torch.uint8), sorted=E((nb, n), torch.uint8), cost=E((nb, n), torch.int64), rate=E((nb, n, 2), torch.int32),
                            ref_fast_cost=E((nb,), torch.int64), blk_out=E((nb, n, 16), torch.uint8))
        common = dict(P, nblocks=nb, blk=blk, cand_in=cand_in, ctx=ctx, rates=rates, mv_cost=mvc)
        # the new call
        sg = dict(common, **outs(), bwidth=side, bheight=side, use_chroma=1, ref0=view["ref0"], ref1=view["ref1"], ref_stride=strides, src=view["src"],
                  src_stride=strides, pred_out=[E((nb, n) + hw[p], torch.uint8) for p in range(3)])
        s_arr = dsp.make_inter_fast_search_groups([sg])
        scratch = E((max(dsp.lib.svt_hip_inter_fast_search_scratch_bytes(s_arr, 1), 16),), torch.uint8)
        # the baseline's stages
        all_pred = [E((nb * ni,) + hw[p], torch.uint8) for p in range(3)]
        all_dist = [E((nb, ni), torch.int64) for _ in range(3)]
        pg = lambda p, pred: dict(ref0=view["ref0"][p], ref1=view["ref1"][p], ref_stride=strides[p], ss=int(p > 0), bwidth=side, bheight=side,
                                  blk=blk.view(nb * ni, 16), pred=pred, src=view["src"][p], src_stride=strides[p], dist=all_dist[p])
        store_arr = dsp.make_inter_pred_groups([pg(p, all_pred[p]) for p in range(3)])
        dist_arr = dsp.make_inter_pred_groups([pg(p, None) for p in range(3)])
        pk = dict(common, **outs(), dist=all_dist[0], dist_cb=all_dist[1], dist_cr=all_dist[2])
        p_arr = dsp.make_inter_fast_pick_groups([pk])
        A = dict(blk=blk_np.view(np.uint8).reshape(nb, ni, 16), cand_in=cand_np.view(np.uint8).reshape(nb, ni, 16), ctx=ctx_np.view(np.uint8).reshape(nb, 16),
                 rates=rates_np)
        rows_i = torch.arange(nb, device=dev).view(nb, 1)

        def search():
            ok(dsp.lib.svt_hip_inter_fast_search_frame(s_arr, 1, PIC_W, PIC_H, 8, SAD, dsp._p(scratch), scratch.numel(), dsp._stream()))

        def pick_only():
            ok(dsp.inter_fast_pick_frame(p_arr, SAD))

        def dist_only():
            ok(dsp.lib.svt_hip_inter_pred_frame(dist_arr, 3, PIC_W, PIC_H, 8, SAD, dsp._stream()))

        def baseline():
            ok(dsp.lib.svt_hip_inter_pred_frame(store_arr, 3, PIC_W, PIC_H, 8, SAD, dsp._stream()))
            d = [t.cpu().numpy() for t in all_dist]
            cost, lr = restated.np_costs(P, dict(A, dist=d[0], dist_cb=d[1], dist_cr=d[2]), mvc_np)
            cd, srt, ref = fp.np_walk(cost, nfl)
            cand = torch.from_numpy(cd).to(dev)
            return cost, lr, cd, srt, ref, [all_pred[p].view((nb, ni) + hw[p])[rows_i, cand] for p in range(3)]

        search(); dist_only(); pick_only(); torch.cuda.synchronize()       # warm-up
        cost, lr, cd, srt, ref, gathered = baseline()
        torch.cuda.synchronize()
        pick = lambda v: np.take_along_axis(v, cd, axis=1)
        for g in (sg, pk):
            assert np.array_equal(g["cand"].cpu().numpy(), cd) and np.array_equal(g["sorted"].cpu().numpy(), srt), "cand / sorted against the host"
            assert np.array_equal(g["cost"].cpu().numpy().view(np.uint64), pick(cost)) and np.array_equal(g["ref_fast_cost"].cpu().numpy().view(np.uint64), ref)
            assert np.array_equal(g["rate"].cpu().numpy().view(np.uint32)[:, :, 0], pick(lr))
        for p in range(3):
            assert torch.equal(sg["pred_out"][p], gathered[p]), ("the survivors' predictions against the gather", p)
        se_w, ba_w, pk_w, di_w = [], [], [], []
        for _ in range(nwin):
            se_w.append(window(search, min_s)); ba_w.append(window(baseline, min_s)); pk_w.append(window(pick_only, min_s)); di_w.append(window(dist_only, min_s))
        m = statistics.median
        spread = lambda w: max(w) - min(w)
        read_b = nb * (ni * (16 + 16 + 24) + 16)
        write_b = nb * (n * (1 + 1 + 8 + 8 + 16) + 8)
        traffic_s = (read_b + write_b) / copy_rate
        row = dict(block=f"{side}x{side}", nblocks=nb, ninter=ni, nfl=nfl, n=n, search_ms=m(se_w) * 1e3, baseline_ms=m(ba_w) * 1e3, pick_ms=m(pk_w) * 1e3,
                   dist_ms=m(di_w) * 1e3, baseline_over_search=m(ba_w) / m(se_w), search_spread_ms=spread(se_w) * 1e3, baseline_spread_ms=spread(ba_w) * 1e3,
                   search_faster_by_more_than_spread=bool(m(ba_w) - m(se_w) > spread(se_w) + spread(ba_w)),
                   pick_read_bytes=read_b, pick_write_bytes=write_b, traffic_only_ms=traffic_s * 1e3, traffic_only_fraction=traffic_s / m(pk_w),
                   prediction_array_bytes_not_written=nb * ni * side * side * 3 // 2,
                   search_ms_windows=[x * 1e3 for x in se_w], baseline_ms_windows=[x * 1e3 for x in ba_w], pick_ms_windows=[x * 1e3 for x in pk_w],
                   dist_ms_windows=[x * 1e3 for x in di_w])
        rows.append(row)
        print(json.dumps({k: (round(v, 4) if isinstance(v, float) else v) for k, v in row.items() if not k.endswith("windows")}), flush=True)
        del sg, pk, s_arr, p_arr, store_arr, dist_arr, all_pred, all_dist, scratch, gathered, blk, cand_in, ctx
        torch.cuda.empty_cache()
    out = dict(device=dsp.device_name(), picture=[PIC_W, PIC_H], chroma="4:2:0", metric="SAD", lambda_=LAMBDA, quick=a.quick, copy_bytes=nbytes,
               copy_ms=copy_s * 1e3, copy_rate_bytes_per_s=copy_rate, window_s=min_s, windows=nwin,
               traffic_only="(ninter * 56 + 16 B per block in, n * 34 + 8 B per block out) over the copy rate (2 * bytes / time of svt_hip_membw_probe mode 1)",
               baseline="svt_hip_inter_pred_frame storing every candidate's prediction and distortion (Y, Cb, Cr) + D2H of the distortions + numpy cost "
                        "and walk (one host thread) + H2D of the winners + torch gather of their predictions",
               cases=rows)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    json.dump(out, open(a.out, "w"), indent=1)
    print("wrote", a.out)


if __name__ == "__main__":
    main()

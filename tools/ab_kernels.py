#!/usr/bin/env python3
"""A/B of two builds of the library on the same box, interleaved: tools/ab/lib_a.so against tools/ab/lib_b.so (tools/make_ab_lib.sh).
usage: ab_kernels.py [--out=FILE.json] <workload> [<workload> ...]      workloads: enc8 enc16 enc32 enc64 inv8 inv16 inv32 fq8 fq16 fwd8 fwd16 (dense 8-bit batches),
       fqp8 fqp16 (fwd_quant_planes on a 8192x4096 plane; fqp32h: a 10-bit plane), encp32 encp32h (encode_recon_planes, 8- / 10-bit plane), fl8 fl16 fl32 fl64 (full_loop, dense, AVX2 flavour, DCT_DCT) and fl8x16 fl16x16
       (every allowed type), c4 (one 1080p frame, five sizes, svt_hip_encode_recon_frame), ois8 ois16 (open-loop intra search of a 1080p
       picture), bip, me85 me209, fpick ifpick (svt_hip_fast_pick_frame with gather on 61 candidates, svt_hip_inter_fast_pick_frame on 48 inter
       candidates: the 8x8 blocks of a 1080p picture, nfl 12), ipred isse (svt_hip_inter_pred_frame, prediction stored and SSD, and
       svt_hip_interp_sse_frame with use_uv 1: the 16x16 luma blocks of a 1080p picture, fractional vectors, single reference and BI_PRED mixed)
Prints per workload the minimum and median of 6 interleaved rounds per library, the spread of a's own rounds (minimum to median) and
whether b's median lies within it of a's, and whether the two libraries' outputs are equal; --out also writes the rows to a file."""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import torch

import __graft_entry__ as ge

pkg = ge.load_package()
dev = torch.device("cuda:0")
TW = pkg.TX_W; TH = pkg.TX_H


def load(tag):
    d = pkg.SvtHipDsp.__new__(pkg.SvtHipDsp)
    d.torch = torch; d.lib = pkg.load_library(os.path.join(ROOT, "tools", "ab", f"lib_{tag}.so")); d.device = dev
    assert d.lib.svt_hip_init(0) == 0
    return d


def timeit(fn, iters=8):
    for _ in range(2):
        fn()
    torch.cuda.synchronize()
    e0 = torch.cuda.Event(enable_timing=True); e1 = torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record(); torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters


def digest(o):
    if isinstance(o, (tuple, list)):
        return [digest(x) for x in o]
    if isinstance(o, torch.Tensor):
        return int((o.to(torch.int64) & 0xffffffff).sum())
    return None


def workload(name, d):
    g = torch.Generator(device=dev); g.manual_seed(13596)
    qt = pkg.tables.quant_tables(8); qrow = {k: v[100].copy() for k, v in qt.items()}
    if name.startswith("fl"):            # full_loop, dense, AVX2 flavour: fl<S> DCT_DCT, fl<S>x16 every allowed type
        S = int(name[2:].split("x")[0]); s_ = {4: 0, 8: 1, 16: 2, 32: 3, 64: 4}[S]
        types = ([0] if "x" not in name else list(range(16)) if S <= 16 else [0, 9] if S == 32 else [0])
        n = (1 << 26) // (S * S)
        src = torch.randint(0, 256, (n, S, S), dtype=torch.uint8, device=dev, generator=g)
        pred = (src.to(torch.int16) + torch.randint(-20, 21, (n, S, S), dtype=torch.int16, device=dev, generator=g)).clamp(0, 255).to(torch.uint8)
        iscan = torch.from_numpy(np.stack([pkg.tables.scan_tables(s_, t)[1] for t in types]).astype(np.int16)).to(dev)
        return (lambda: d.full_loop(src, pred, s_, types, qrow, flavour=1, iscan=iscan)), n, 2 * S * S + 18 * len(types)
    if name.startswith("fqp") or name.startswith("encp"):      # fwd_quant_planes / encode_recon_planes: every block of a 8192x4096 plane
        hbd = name.endswith("h")                                # ...h: 10-bit samples in 16-bit planes
        S = int(name.rstrip("h")[3 if name.startswith("fqp") else 4:]); s_ = {4: 0, 8: 1, 16: 2, 32: 3, 64: 4}[S]
        PW, PH = 8192, 4096
        top, dt, es = (1024, torch.int16, 2) if hbd else (256, torch.uint8, 1)
        if hbd:
            qrow = {k: v[100].copy() for k, v in pkg.tables.quant_tables(10).items()}
        src = torch.randint(0, top, (PH, PW), dtype=dt, device=dev, generator=g)
        pred = (src.to(torch.int16) + torch.randint(-20, 21, (PH, PW), dtype=torch.int16, device=dev, generator=g)).clamp(0, top - 1).to(dt)
        xy = torch.from_numpy(np.array([(y << 16) | x for y in range(0, PH, S) for x in range(0, PW, S)], np.uint32).view(np.int32)).to(dev)
        iscan = torch.from_numpy(pkg.tables.scan_tables(s_, 0)[1]).to(dev)
        nc = min(S, 32) ** 2
        bd = 10 if hbd else 8
        if name.startswith("encp"):
            recon = torch.empty_like(pred)

            def encp():
                o = d.encode_recon_planes(src, PW, pred, PW, recon, PW, xy, s_, 0, qrow, iscan, bd=bd)
                return [o["qcoeff"], o["eob"], recon]
            return encp, xy.shape[0], 3 * S * S * es + 4 * nc + 2
        return (lambda: d.fwd_quant_planes(src, PW, pred, PW, xy, s_, 0, qrow, iscan, bd=bd, want_sad=not hbd)), xy.shape[0], 2 * S * S * es + 12 * nc + 6
    if name[:3] in ("enc", "inv", "fwd") or name[:2] == "fq":
        S = int(name[3:] if name[:2] != "fq" else name[2:]); s_ = {4: 0, 8: 1, 16: 2, 32: 3, 64: 4}[S]
        n = (1 << 20) * 1024 // (S * S) if S <= 32 else 1 << 18
        nc = min(S, 32) ** 2
        src = torch.randint(0, 256, (n, S, S), dtype=torch.uint8, device=dev, generator=g)
        pred = (src.to(torch.int16) + torch.randint(-20, 21, (n, S, S), dtype=torch.int16, device=dev, generator=g)).clamp(0, 255).to(torch.uint8)
        iscan = torch.from_numpy(pkg.tables.scan_tables(s_, 0)[1]).to(dev)
        if name.startswith("enc"):
            return (lambda: d.encode_recon(src, pred, s_, 0, qrow, iscan, keep_coeff=False)), n, 2 * S * S + 4 * nc + S * S + 6
        if name.startswith("fwd"):      # fwd_txfm2d on a dense int16 residual: fwd_staged_kernel MODE 0
            res = src.to(torch.int16) - pred.to(torch.int16)
            out = torch.empty((n, S * S), dtype=torch.int32, device=dev)
            return (lambda: d.fwd_txfm2d(res, s_, 0, out=out)), n, 2 * S * S + 4 * S * S
        if name.startswith("fq"):
            outs = (torch.empty((n, nc), dtype=torch.int32, device=dev), torch.empty((n, nc), dtype=torch.int32, device=dev),
                    torch.empty((n, nc), dtype=torch.int32, device=dev), torch.zeros(n, dtype=torch.int16, device=dev), torch.zeros(n, dtype=torch.int32, device=dev))
            return (lambda: d.fwd_quant_sad(src, pred, s_, 0, qrow, iscan, outs=outs)), n, 2 * S * S + 12 * nc + 6
        c = torch.randint(-500, 501, (n, nc), dtype=torch.int32, device=dev, generator=g)
        dst0 = src.clone()

        def inv():
            dst = dst0.clone() if False else dst0
            return d.inv_txfm2d_add(c, dst, s_, 0, 8)
        return inv, n, 4 * nc + 2 * S * S
    if name == "c4":
        from cidana_svt_av1_amd import frames
        W, H = 1920, 1080
        src, pred = {}, {}
        for nm, (ph, pw) in (("Y", (H, W)), ("U", (H // 2, W // 2)), ("V", (H // 2, W // 2))):
            src[nm] = torch.randint(0, 256, (ph, pw), dtype=torch.uint8, device=dev, generator=g)
            pred[nm] = (src[nm].to(torch.int16) + torch.randint(-20, 21, (ph, pw), dtype=torch.int16, device=dev, generator=g)).clamp(0, 255).to(torch.uint8)
        fp = frames.FramePass(d, pkg, src, pred)
        return (lambda: fp.run(qrow)), fp.pixels, 7, (lambda: fp.digest())
    if name == "oisall":        # the four block sizes of a 1080p picture in one svt_hip_ois_search_frame call
        W, H, pad = 1920, 1080, 64
        plane = torch.randint(0, 256, (H + 2 * pad, W + 2 * pad), dtype=torch.uint8, device=dev, generator=g); pic = plane[pad:, pad:]
        groups, nb = [], 0
        for bsize in (8, 16, 32, 64):
            blocks = [(x, y) for y in range(0, H - bsize + 1, bsize) for x in range(0, W - bsize + 1, bsize)]
            xy = torch.from_numpy(np.array([(y << 16) | x for x, y in blocks], np.uint32).view(np.int32)).to(dev)
            modes, deltas = d.ois_candidates(bsize)
            groups.append((xy, bsize, modes, deltas)); nb += len(blocks)
        return (lambda: d.ois_search_frame(pic, W + 2 * pad, W, H, groups)), nb, 0
    if name.startswith("ois"):
        bsize = int(name[3:]); W, H, pad = 1920, 1080, 64
        plane = torch.randint(0, 256, (H + 2 * pad, W + 2 * pad), dtype=torch.uint8, device=dev, generator=g); pic = plane[pad:, pad:]
        blocks = [(x, y) for y in range(0, H - bsize + 1, bsize) for x in range(0, W - bsize + 1, bsize)]
        xy = torch.from_numpy(np.array([(y << 16) | x for x, y in blocks], np.uint32).view(np.int32)).to(dev)
        modes, deltas = d.ois_candidates(bsize)
        return (lambda: d.ois_search(pic, W + 2 * pad, W, H, xy, bsize, modes, deltas)), len(blocks), bsize * bsize + 4 * len(modes)
    if name.startswith("intra:"):        # intra:<mode> - dense 32x32 8-bit prediction batch, SVT_INTRA_* mode number (z1 / z2 / z3: 10 / 11 / 12)
        parts = name.split(":")          # intra:<mode>[:<neighbour row pitch>]
        mode = int(parts[1]); n = 1 << 21
        pitch = int(parts[2]) if len(parts) > 2 else 16 + 2 * 64 + 16
        ab_ = torch.randint(0, 256, (n, pitch), dtype=torch.uint8, device=dev, generator=g); lf = torch.randint(0, 256, (n, pitch), dtype=torch.uint8, device=dev, generator=g)
        out = torch.empty((n, 32, 32), dtype=torch.uint8, device=dev)
        return (lambda: d.intra_pred(ab_, lf, mode, 32, 32, 8, 0, 0, 64, 64, out=out)), n, 1024 + 130
    if name == "bip":
        n = 1 << 20
        top = torch.randint(0, 256, (n, 48), dtype=torch.uint8, device=dev, generator=g); left = torch.randint(0, 256, (n, 48), dtype=torch.uint8, device=dev, generator=g)
        blk = torch.zeros((n, 8), dtype=torch.uint8, device=dev)
        blk[:, 0] = torch.arange(n, device=dev) % 13
        blk[:, 1] = ((torch.arange(n, device=dev) // 13) % 7 - 3).to(torch.int8).view(torch.uint8) * ((blk[:, 0] >= 1) & (blk[:, 0] <= 8)).to(torch.uint8)
        blk[:, 4] = 16; blk[:, 5] = 16; blk[:, 6] = 16; blk[:, 7] = 16
        out = torch.empty((n, 16, 16), dtype=torch.uint8, device=dev)
        if hasattr(d.lib, "svt_hip_intra_order_blocks_batch"):          # this round: order the batch by predictor kind first (both timed)
            def run():
                order = d.intra_order_blocks(blk, 2)
                return d.build_intra_predictors(top, left, blk, 2, dst=out, dst_stride=16, order=order)
            return run, n, 330
        return (lambda: d.build_intra_predictors(top, left, blk, 2, dst=out, dst_stride=16)), n, 330
    if name == "bip_plain":
        n = 1 << 20
        top = torch.randint(0, 256, (n, 48), dtype=torch.uint8, device=dev, generator=g); left = torch.randint(0, 256, (n, 48), dtype=torch.uint8, device=dev, generator=g)
        blk = torch.zeros((n, 8), dtype=torch.uint8, device=dev)
        blk[:, 0] = torch.arange(n, device=dev) % 13
        blk[:, 1] = ((torch.arange(n, device=dev) // 13) % 7 - 3).to(torch.int8).view(torch.uint8) * ((blk[:, 0] >= 1) & (blk[:, 0] <= 8)).to(torch.uint8)
        blk[:, 4] = 16; blk[:, 5] = 16; blk[:, 6] = 16; blk[:, 7] = 16
        out = torch.empty((n, 16, 16), dtype=torch.uint8, device=dev)
        return (lambda: d.build_intra_predictors(top, left, blk, 2, dst=out, dst_stride=16)), n, 330
    if name in ("fpick", "ifpick"):      # the two kernels that end the fast loop, on the 8x8 blocks of a 1080p picture, nfl 12, SAD
        sys.path.insert(0, os.path.join(ROOT, "tools"))
        import bench_fast_pick as bf
        rng = np.random.default_rng(17031)
        D = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev)
        E = lambda shape, dt: torch.empty(shape, dtype=dt, device=dev)
        nb_x, nb_y, nfl = bf.PIC_W // 8, (bf.PIC_H + 7) // 8, 12
        n = nb_x * nb_y
        sad = lambda shape: D(rng.integers(0, 64 * 256, shape).astype(np.int64))
        outs = dict(cand=E((n, nfl), torch.uint8), sorted=E((n, nfl), torch.uint8), cost=E((n, nfl), torch.int64), rate=E((n, nfl, 2), torch.int32),
                    ref_fast_cost=E((n,), torch.int64))
        if name == "fpick":              # svt_hip_fast_pick_frame: tools/bench_fast_pick.py's 61-candidate list, tables and context records; with gather
            modes, deltas = bf.candidate_list()
            C = len(modes)
            bsize, bsize_uv = bf.mg.bsizes_of_tx(1)
            pblk = np.zeros(n, bf.mg.BLK_DTYPE)
            pblk["top_mode"], pblk["left_mode"], pblk["has_chroma"] = rng.integers(0, 13, n), rng.integers(0, 13, n), 1
            xy = (np.arange(n, dtype=np.uint32) % nb_x * 8 | (np.arange(n, dtype=np.uint32) // nb_x * 8) << 16).view(np.int32)
            outs.update(pred_out=E((n, nfl, 8, 8), torch.uint8), src_xy_out=E((n, nfl), torch.int32))
            g_ = dict(outs, tx_size=1, bsize=bsize, bsize_uv=bsize_uv, nblocks=n, modes=modes, deltas=deltas, uv_modes=[0] * C, uv_deltas=[0] * C,
                      use_angle_delta=1, nfl=nfl, slice_is_intra=1, blk=D(pblk.view(np.uint8).reshape(-1, 8)), rates=D(bf.mg.make_rates("rand", rng)),
                      dist=sad((n, C)), pred=D(rng.integers(0, 256, (n, C, 8, 8), dtype=np.uint8)), src_xy=D(xy))
            g_["lambda"] = bf.LAMBDA
            arr, call, bpu = d.make_fast_pick_groups([g_]), d.fast_pick_frame, C * 8 + 8 + 2 * nfl * 64 + nfl * 22 + 8
        else:                            # svt_hip_inter_fast_pick_frame: tools/bench_inter_fast_search.py's records and tables, 48 inter candidates
            import bench_inter_fast_search as bi
            ni = 48
            blk, cand, ctx = bi.make_records(rng, 8, nb_x, nb_y, ni)
            outs.update(blk_out=E((n, nfl, 16), torch.uint8))
            g_ = dict(outs, bsize=3, bsize_uv=0, ninter=ni, nintra=0, nfl=nfl, ac_dequant_q3=0, reference_mode_select=1, switchable_motion_mode=1, nblocks=n,
                      blk=D(blk.view(np.uint8).reshape(n, ni, 16)), cand_in=D(cand.view(np.uint8).reshape(n, ni, 16)), ctx=D(ctx.view(np.uint8).reshape(n, 16)),
                      rates=D(bi.mg.pack_rates(bi.mg.make_rates(0))), mv_cost=D(bi.mg.make_mv_cost()), dist=sad((n, ni)), dist_cb=sad((n, ni)), dist_cr=sad((n, ni)))
            g_["lambda"] = bi.LAMBDA
            arr, call, bpu = d.make_inter_fast_pick_groups([g_]), d.inter_fast_pick_frame, ni * 56 + 16 + nfl * 34 + 8

        def run(keep=(g_, arr)):         # (the group array points into the tensors)
            assert call(arr, 0) == 0, d.lib.svt_hip_last_error()
        # every output weighted by position: a survivor in another slot changes the digest
        weighted = lambda t: (t.reshape(-1).to(torch.int64) * (torch.arange(t.numel(), device=dev) % 65521 + 1)).sum()
        return run, n, bpu, (lambda: [weighted(outs[k]) for k in sorted(outs)]), 2000
    if name in ("ipred", "isse"):        # the two kernels that run the sub-pel convolve, on the 16x16 luma blocks of a 1080p picture, 8-bit
        sys.path.insert(0, os.path.join(ROOT, "tools"))
        rng = np.random.default_rng(19031)
        D = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev)
        W, H, bs = 1920, 1080, 16
        nx, ny = W // bs, H // bs
        n = nx * ny

        def planes(pads):                # padded planes; the views start at the picture's sample (0, 0)
            full = [torch.randint(0, 256, (H // s + 2 * p, W // s + 2 * p), dtype=torch.uint8, device=dev, generator=g) for s, p in pads]
            return full, [t[p:, p:] for t, (s, p) in zip(full, pads)], [t.shape[1] for t in full]

        def mixed(r):                    # fractional vectors; list 0, list 1 and BI_PRED blocks share waves
            r["pred_direction"] = rng.integers(0, 3, n)
            return D(r.view(np.uint8).reshape(n, 16))
        if name == "ipred":              # svt_hip_inter_pred_frame: tools/bench_inter_pred.py's records; prediction stored and SSD
            import bench_inter_pred as bp
            keep, (ref0, ref1, src), (stride, _, _) = planes([(1, bp.PAD)] * 3)
            outs = dict(pred=torch.empty((n, bs, bs), dtype=torch.uint8, device=dev), dist=torch.empty((n,), dtype=torch.int64, device=dev))
            g_ = dict(outs, ref0=ref0, ref1=ref1, ref_stride=stride, ss=0, bwidth=bs, bheight=bs, nblocks=n,
                      blk=mixed(bp.make_records(pkg, rng, bs, nx, ny, "sr_2d")), src=src, src_stride=stride)
            arr = d.make_inter_pred_groups([g_])
            call, bpu = (lambda: d.inter_pred_frame(arr, W, H, 8, 1)), 3 * bs * bs + 16 + 8
        else:                            # svt_hip_interp_sse_frame, use_uv 1: tools/bench_interp_search.py's records on the same blocks
            import bench_interp_search as bs_
            pads = [(1, bs_.PAD), (2, bs_.PAD_C), (2, bs_.PAD_C)]
            (k0, ref0, strides), (k1, ref1, _), (k2, src, _) = planes(pads), planes(pads), planes(pads)
            keep = (k0, k1, k2)
            outs = dict(sse=torch.empty((n, 3, 9), dtype=torch.int32, device=dev))
            g_ = dict(outs, ref0=ref0, ref1=ref1, ref_stride=strides, src=src, src_stride=strides, bwidth=bs, bheight=bs, nblocks=n,
                      blk=mixed(bs_.make_records(pkg, rng, bs, nx, ny, 1, 0)))
            arr = d.make_interp_sse_groups([g_])
            call, bpu = (lambda: d.interp_sse_frame(arr, W, H, 1)), 3 * (bs * bs * 3 // 2) + 16 + 108

        def run(keep=(keep, g_, arr)):       # (the group array points into the tensors)
            assert call() == 0, d.lib.svt_hip_last_error()
        weighted = lambda t: (t.reshape(-1).to(torch.int64) * (torch.arange(t.numel(), device=dev) % 65521 + 1)).sum()
        return run, n, bpu, (lambda: [weighted(outs[k]) for k in sorted(outs)]), 2000
    if name in ("me85", "me209"):
        n = 2040
        src = torch.randint(0, 256, (n, 64, 64), dtype=torch.uint8, device=dev, generator=g); ref = torch.randint(0, 256, (n, 127, 128), dtype=torch.uint8, device=dev, generator=g)
        return (lambda: d.me_fullpel_search(src, ref, 64, 64, nsq=(name == "me209"))), n, 64 * 64 + 127 * 127
    raise SystemExit(f"unknown workload {name}")


def main():
    libs = {t: load(t) for t in ("a", "b")}
    out = [a[6:] for a in sys.argv[1:] if a.startswith("--out=")]
    rows = []
    for name in [a for a in sys.argv[1:] if not a.startswith("--out=")]:
        fns, outs = {}, {}
        for t in ("a", "b"):
            w = workload(name, libs[t])
            fns[t], units, bpu = w[:3]
            iters = w[4] if len(w) > 4 else 8        # calls per timed window: a workload of a fraction of a millisecond asks for more
            r = fns[t]()
            outs[t] = digest(w[3]() if len(w) > 3 else r)
        times = {"a": [], "b": []}
        for rnd in range(6):
            for t in ("a", "b"):
                times[t].append(timeit(fns[t], iters))
        row = {"workload": name, "units": units, "calls_per_window": iters, "equal_outputs": outs["a"] == outs["b"]}
        for t in ("a", "b"):
            v = sorted(times[t])
            med = (v[2] + v[3]) / 2
            row[t] = {"ms_min": round(v[0], 5), "ms_med": round(med, 5), "frac_hbm_at_med": round(bpu * units / med / 1e6 / 8000, 4)}
        row["b_over_a_speed"] = round(row["a"]["ms_med"] / row["b"]["ms_med"], 4)
        # what a's own rounds differ by, minimum to median, and whether b's median is within that of a's
        row["a_spread_min_to_med_ms"] = round(row["a"]["ms_med"] - row["a"]["ms_min"], 5)
        row["b_med_within_a_spread"] = bool(row["b"]["ms_med"] <= row["a"]["ms_med"] + row["a_spread_min_to_med_ms"])
        rows.append(row)
        print(json.dumps(row), flush=True)
    if out:
        json.dump(dict(device=torch.cuda.get_device_name(0), rounds=6, rows=rows), open(out[0], "w"), indent=1)


if __name__ == "__main__":
    main()

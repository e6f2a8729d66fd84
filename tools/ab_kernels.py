#!/usr/bin/env python3
"""A/B of two builds of the library on the same box, interleaved: tools/ab/lib_a.so against tools/ab/lib_b.so (tools/make_ab_lib.sh).
usage: ab_kernels.py [--out=FILE.json] <workload> [<workload> ...]      workloads: enc8 enc16 enc32 enc64 inv8 inv16 inv32 fq8 fq16 fwd8 fwd16 (dense 8-bit batches),
       fqp8 fqp16 (fwd_quant_planes on a 8192x4096 plane; fqp32h: a 10-bit plane), encp32 encp32h (encode_recon_planes, 8- / 10-bit plane), fl8 fl16 fl32 fl64 (full_loop, dense, AVX2 flavour, DCT_DCT) and fl8x16 fl16x16
       (every allowed type), c4 (one 1080p frame, five sizes, svt_hip_encode_recon_frame), ois8 ois16 (open-loop intra search of a 1080p
       picture), bip, me85 me209, fpick ifpick (svt_hip_fast_pick_frame with gather on 61 candidates, svt_hip_inter_fast_pick_frame on 48 inter
       candidates: the 8x8 blocks of a 1080p picture, nfl 12), ipred isse (svt_hip_inter_pred_frame, prediction stored and SSD, and
       svt_hip_interp_sse_frame with use_uv 1: the 16x16 luma blocks of a 1080p picture, fractional vectors, single reference and BI_PRED mixed,
       part rfinal ienc dlfmi (the writer and the three readers of the final block list on the inputs of tools/bench_partition.py,
       bench_recon_final.py `mixed`, bench_intra_encode.py `mixed` with npics 1 in a HIP graph, and bench_dlf.py's mixed list)
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
    if name in ("part", "rfinal", "ienc", "dlfmi"):      # the writer and the three readers of the final block list, on the benchmarks' own inputs
        for sub in ("tools", os.path.join("tests", "golden")):
            sys.path.insert(0, os.path.join(ROOT, sub))
        import bench_partition as bp
        import make_golden_partition as mgp
        D = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev)
        Z = lambda shape, dt: torch.zeros(shape, dtype=dt, device=dev)      # (zeros: the digest also reads what a call leaves alone)
        ok = lambda rc: rc == 0 or sys.exit(d.lib.svt_hip_last_error())
        weighted = lambda t: (t.reshape(-1).to(torch.int64) * (torch.arange(t.numel(), device=dev) % 65521 + 1)).sum()
        pgeom = mgp.load_geometry(dict(np.load(os.path.join(ROOT, "tests", "golden", "partition.npz"))))
        origins = [(64 * x, 64 * y) for y in range((bp.PIC_H + 63) // 64) for x in range((bp.PIC_W + 63) // 64)]
        nsb = len(origins)

        def partition_args(c, rec, **more):      # bench_partition.py's arguments for a picture_case and its decision records
            a = dict(sb=D(c["sb"].view(np.uint8).reshape(nsb, 12)), leaf=D(c["leaf"].view(np.uint8).reshape(-1, 12)), decision=D(rec.view(np.uint8).reshape(-1, 72)),
                     partition_bits=D(c["bits"]), pic_width=bp.PIC_W, pic_height=bp.PIC_H, slice_is_intra=0, sq=Z((nsb, mgp.NSQ, 16), torch.uint8),
                     final_count=Z((nsb,), torch.int32), final=Z((nsb, mgp.MAX_FINAL, 12), torch.uint8), **more)
            a["lambda"] = bp.LAMBDA
            return a
        if name == "part":               # bench_partition.py: the squares with the H and V shapes of a 1080p picture, with d_final_decision
            c = bp.picture_case(np.random.default_rng(19019), pgeom, bp.CLASSES[1][1], origins)
            rec = np.zeros(len(c["leaf"]), pkg.md_decision_dtype())
            rec["cost"], rec["cand"] = c["cost"], np.arange(len(rec)) % 64
            pa = partition_args(c, rec, final_decision=Z((nsb, mgp.MAX_FINAL, 72), torch.uint8))
            args = d.make_partition_args(pa)
            return (lambda keep=pa: ok(d.partition_decide_frame(args))), nsb, 0, (lambda: [weighted(pa[k]) for k in ("sq", "final_count", "final", "final_decision")]), 200
        if name == "rfinal":             # bench_recon_final.py's `mixed` partition, three planes, no optional output
            import bench_recon_final as br
            import make_golden_recon_final as mr
            rng = np.random.default_rng(20020)
            tabs = mr.bsize_tables(mr.load_geometry(dict(np.load(os.path.join(ROOT, "tests", "golden", "recon_final.npz")))))
            c = bp.picture_case(rng, pgeom, bp.CLASSES[1][1], origins)
            bsize = pgeom["bsize"][c["leaf"]["mds_idx"]].astype(np.int64)
            order = np.argsort(bsize, kind="stable")
            c["leaf"]["src"][order] = np.arange(len(order))
            cost = np.zeros_like(c["cost"]); cost[c["leaf"]["src"]] = c["cost"]
            rec, groups = br.records_and_groups(rng, pkg, bsize[order], tabs, D)
            rec["cost"] = cost
            pa = partition_args(c, rec)
            ok(d.partition_decide_frame(pa))
            planes = [Z((br.ROWS >> (p > 0), br.PIC_W >> (p > 0)), torch.uint8) for p in range(3)]
            ra = dict(final=pa["final"], final_count=pa["final_count"], decision=pa["decision"], groups=groups, recon=planes,
                      scratch=torch.empty((d.recon_final_scratch_bytes(nsb),), dtype=torch.uint8, device=dev),
                      width=[br.PIC_W, br.PIC_W // 2, br.PIC_W // 2], height=[br.ROWS, br.ROWS // 2, br.ROWS // 2])
            args = d.make_recon_final_args(ra)
            return (lambda keep=(pa, ra): ok(d.recon_final_frame(args))), nsb, 0, (lambda: [weighted(p) for p in planes]), 50
        if name == "ienc":               # bench_intra_encode.py's picture and `mixed` list, npics 1, the call in a HIP graph as there
            import bench_intra_encode as bi
            import make_golden_intra_encode as mi
            import make_golden_recon_final as mr
            rng = np.random.default_rng(21021)
            geom = mr.load_geometry(dict(np.load(os.path.join(ROOT, "tests", "golden", "recon_final.npz"))))
            gold = dict(np.load(os.path.join(ROOT, "tests", "golden", "intra_encode.npz")))
            qrows = [{k: gold["c0_qrows"][i][j] for j, k in enumerate(mi.QKEYS)} for i in (0, 1)]
            W, H = bi.PIC_W, bi.PIC_H
            sb_cols, sb_rows = W // 64, H // 64
            n = sb_cols * sb_rows
            final, count, blk, _ = bi.build_list(rng, geom, bi.LISTS["mixed"], sb_cols, sb_rows)
            ia = dict(npics=1, sb_cols=sb_cols, sb_rows=sb_rows, final=D(final.view(np.uint8).reshape(n, mi.MAX_FINAL, 12)), final_count=D(count.view(np.int32)),
                      blk=D(blk.view(np.uint8).reshape(-1, 8)), src=[D(mi.smooth_noise(rng, H >> (p > 0), W >> (p > 0), 2)) for p in range(3)],
                      recon=[torch.full((H >> (p > 0), W >> (p > 0)), 128, dtype=torch.uint8, device=dev) for p in range(3)],
                      q_luma=qrows[0], q_chroma=qrows[1], tables=D(d.intra_encode_tables()), status=Z((1, n, mi.MAX_FINAL), torch.uint8),
                      result=Z((n, mi.MAX_FINAL, 8), torch.uint8), coeff_offset=Z((n, mi.MAX_FINAL, 2), torch.int32),
                      scratch=torch.empty((d.intra_encode_scratch_bytes(1, n),), dtype=torch.uint8, device=dev),
                      width=[W, W // 2, W // 2], height=[H, H // 2, H // 2])
            args = d.make_intra_encode_args(ia)
            call = lambda: ok(d.intra_encode_frame(args))
            call(); torch.cuda.synchronize()                                    # warm: nothing is created inside the capture
            graph = torch.cuda.CUDAGraph()
            side = torch.cuda.Stream()
            side.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(side):
                with torch.cuda.graph(graph, stream=side):
                    call()
            torch.cuda.current_stream().wait_stream(side)
            # (the planes are coded in place: each replay predicts from the last one's samples, the same work; both libraries are
            # digested after the same number of runs)
            return (lambda keep=(ia, args): graph.replay()), n, 0, (lambda: [weighted(t) for t in ia["recon"] + [ia["status"], ia["result"], ia["coeff_offset"]]]), 4
        # dlfmi: svt_hip_dlf_mi_frame on bench_dlf.py's mixed list (the partition of the all_blocks lists) over an all-8x8 grid
        sys.path.insert(0, os.path.join(ROOT, "tests"))
        import bench_dlf as bd
        rng = np.random.default_rng(2222)
        c = bp.picture_case(np.random.default_rng(19019), pgeom, bp.CLASSES[2][1], origins)
        nleaves = len(c["leaf"])
        rec = np.zeros(nleaves, pkg.md_decision_dtype())
        rec["cost"], rec["cand"] = c["cost"], np.arange(nleaves) % 64
        pa = partition_args(c, rec)
        ok(d.partition_decide_frame(pa))
        info = np.zeros((nleaves, 4), np.uint8)
        inter = rng.random(nleaves) < 0.5
        info[:, 0] = np.where(inter, rng.integers(1, 8, nleaves), 0)
        info[:, 1] = np.where(inter, rng.integers(13, 25, nleaves), rng.integers(0, 13, nleaves))
        info[:, 2] = rng.random(nleaves) < 0.33
        d_info, grid = D(info), D(bd.uniform_grid(3))
        return (lambda keep=pa: d.dlf_mi_frame(pa["final"], pa["final_count"], d_info, grid)), nsb, 0, (lambda: [weighted(grid)]), 200
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

#!/usr/bin/env python3
"""The reconstruction of the final block list (svt_hip_recon_final_frame) on a 1080p 4:2:0 picture: 510 superblocks of 64x64 (30 x 17) in
planes of 1920 x 1088, for three partitions:
  all_8x8    every superblock 64 blocks of 8x8
  all_64x64  every superblock one 64x64
  mixed      the tree svt_hip_partition_decide_frame gives on the synthetic costs of tools/bench_partition.py (squares 64 .. 8 with the H
             and V shapes)
Every md block has a record and a winner: a random prediction, four low-frequency dequantised coefficients (one block in ten eob 0), a
random transform type among those its size defines (so waves of small blocks hold mixed types), one source group per block size.

Per partition, in one process, warm caches (the same buffers every call):
  (a) call      svt_hip_recon_final_frame, three planes, no optional output; `bin` is the same call stopped after its bin stage
                (svt_hip_tune("recon_final_bin_only")): the share of the bin stage
  (b) composed  the device work of the path the call replaces, on the same list: per (plane, size) one scatter of the predictions
                into the plane (torch index_put_ with indices made beforehand), per (plane, size, type) one svt_hip_inv_txfm2d_add_batch
                with d_dst_offsets; its planes are compared with the call's before anything is timed
  (c) hop       that whole path, wall clock, synchronised, median of 3: D2H of the list and the records, the grouping on the host, H2D of
                the offset and index tables, then (b)
Timing of (a), bin and (b): HIP events around windows of back-to-back calls, synchronised before and after, each window >= 0.2 s after a
warm-up call; alternating window by window, 7 windows each, median.  bytes: 9 per luma sample of the reconstructed blocks (6 B luma: 1 B
prediction, 4 B dqcoeff, 1 B recon; 3 B for the two chroma planes).  Writes profiles/r20_recon_final.json.
    python tools/bench_recon_final.py [--out profiles/r20_recon_final.json] [--quick]"""
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
sys.path.insert(0, os.path.join(ROOT, "tools"))
import __graft_entry__ as ge  # noqa: E402
import make_golden_partition as mg  # noqa: E402
import make_golden_recon_final as mr  # noqa: E402
import bench_partition as bp  # noqa: E402

PIC_W, PIC_H, ROWS = 1920, 1080, 1088


def records_and_groups(rng, pkg, bsize_of_src, tabs, T):
    """records (tx_type, eob) and one source group per block size for records ordered by block size -> (records, groups with device arrays)"""
    n = len(bsize_of_src)
    rec = np.zeros(n, pkg.md_decision_dtype())
    groups, at = [], 0
    for b in np.unique(bsize_of_src).tolist():
        nb = int((bsize_of_src == b).sum())
        assert (bsize_of_src[at:at + nb] == b).all()
        tx, tx_uv, cw, ch = tabs[b]
        ty = np.array(mr.types_of(tx), np.uint8)
        rec["tx_type"][at:at + nb] = ty[rng.integers(0, len(ty), nb)]
        g = dict(src_first=at, nblocks=nb, bsize=b, tx_type_uv=mr.uv_type(b, 0, tabs), best_pred=[], best_dqcoeff=[])
        for p in range(3):
            w, h = (mr.BS_W[b], mr.BS_H[b]) if p == 0 else (cw, ch)
            kw, nc = min(w, 32), min(w, 32) * min(h, 32)
            dq = np.zeros((nb, nc), np.int32)
            for at_c in (0, 1, kw, kw + 1):
                dq[:, at_c] = rng.integers(-400, 401, nb)
            zero = rng.random(nb) < 0.1
            rec["eob"][at:at + nb, p] = np.where(zero, 0, kw + 2)
            g["best_pred"].append(T(rng.integers(0, 256, (nb, h, w), dtype=np.uint8)))
            g["best_dqcoeff"].append(T(dq))
        groups.append(g)
        at += nb
    return rec, groups


def uniform_final(geom, origins, depth):
    """every superblock tiled by the squares of one depth, PARTITION_NONE -> (final [nsb, 256], count, bsize per src), src in list order"""
    sq = [m for m in mg.square_mds(geom).tolist() if geom["depth"][m] == depth]
    final = np.zeros((len(origins), mg.MAX_FINAL), mg.FINAL_DTYPE)
    for i, (ox, oy) in enumerate(origins):
        for k, m in enumerate(sq):
            final[i, k] = (m, ox + int(geom["origin_x"][m]), oy + int(geom["origin_y"][m]), int(geom["bsize"][m]), 0, i * len(sq) + k)
    count = np.full(len(origins), len(sq), np.uint32)
    return final, count, np.full(len(origins) * len(sq), int(geom["bsize"][sq[0]]), np.int64)


def composed_tables(final, count, rec, groups, rgeom, tabs, strides, T):
    """the host grouping of the replaced path -> per (plane, size): the prediction scatter's (linear indices, source rows); per (plane, size,
    type): the inverse's (rows of dqcoeff, offsets).  Device tensors."""
    ent = np.concatenate([final[i, :n] for i, n in enumerate(count.tolist())])
    ent = ent[ent["src"] != mg.NO_SRC]
    first = np.array([g["src_first"] for g in groups])
    gi = np.searchsorted(first, ent["src"], side="right") - 1
    scat, inv = [], []
    for k, g in enumerate(groups):
        e = ent[gi == k]
        if not len(e):
            continue
        b = g["bsize"]
        tx, tx_uv, cw, ch = tabs[b]
        local = (e["src"] - g["src_first"]).astype(np.int64)
        for p in range(3):
            sel = np.ones(len(e), bool) if p == 0 else rgeom["has_uv"][e["mds_idx"]].astype(bool)
            if not sel.any():
                continue
            w, h, t = (mr.BS_W[b], mr.BS_H[b], tx) if p == 0 else (cw, ch, tx_uv)
            x = e["x"][sel].astype(np.int64) if p == 0 else ((e["x"][sel].astype(np.int64) >> 3) << 3) >> 1
            y = e["y"][sel].astype(np.int64) if p == 0 else ((e["y"][sel].astype(np.int64) >> 3) << 3) >> 1
            org = y * strides[p] + x
            lin = org[:, None, None] + np.arange(h)[None, :, None] * strides[p] + np.arange(w)[None, None, :]
            scat.append((p, T(lin.reshape(-1)), T(local[sel]), g["best_pred"][p]))
            types = rec["tx_type"][e["src"][sel]] if p == 0 else np.full(int(sel.sum()), g["tx_type_uv"])
            live = rec["eob"][e["src"][sel], p] != 0
            for ty in np.unique(types[live]).tolist():
                m = live & (types == ty)
                inv.append((p, t, int(ty), T(local[sel][m]), T(org[m].astype(np.uint32).view(np.int32)), g["best_dqcoeff"][p]))
    return scat, inv


def composed_run(dsp, planes, scat, inv):
    for p, lin, rows, pred in scat:
        planes[p].view(-1).index_put_((lin,), pred[rows].reshape(-1))
    for p, t, ty, rows, offs, dq in inv:
        dsp.inv_txfm2d_add(dq[rows], planes[p], t, ty, 8, dst_stride=planes[p].stride(0), offsets=offs)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r20_recon_final.json"))
    ap.add_argument("--windows", type=int, default=7)
    ap.add_argument("--quick", action="store_true", help="the last 34 superblocks, 3 windows (a smoke run)")
    a = ap.parse_args()
    pkg = ge.load_package()
    dsp = pkg.SvtHipDsp(0)
    dev = torch.device("cuda:0")
    pgeom = mg.load_geometry(dict(np.load(os.path.join(ROOT, "tests", "golden", "partition.npz"))))
    rgeom = mr.load_geometry(dict(np.load(os.path.join(ROOT, "tests", "golden", "recon_final.npz"))))
    tabs = mr.bsize_tables(rgeom)
    origins = [(64 * x, 64 * y) for y in range((PIC_H + 63) // 64) for x in range((PIC_W + 63) // 64)]
    origins = origins[-34:] if a.quick else origins
    nsb, nwin = len(origins), 3 if a.quick else a.windows
    T = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev)
    ok = lambda rc: rc == 0 or sys.exit(dsp.lib.svt_hip_last_error())
    dims = dict(width=[PIC_W, PIC_W // 2, PIC_W // 2], height=[ROWS, ROWS // 2, ROWS // 2])
    new_planes = lambda: [torch.zeros((ROWS >> (p > 0), PIC_W >> (p > 0)), dtype=torch.uint8, device=dev) for p in range(3)]
    scratch = torch.empty((dsp.recon_final_scratch_bytes(nsb),), dtype=torch.uint8, device=dev)
    rows = []
    for name in ("all_8x8", "all_64x64", "mixed"):
        rng = np.random.default_rng(20020)
        if name == "mixed":
            c = bp.picture_case(rng, pgeom, bp.CLASSES[1][1], origins)
            bsize = pgeom["bsize"][c["leaf"]["mds_idx"]].astype(np.int64)
            order = np.argsort(bsize, kind="stable")                        # the leaves renumbered: the records of a block size contiguous
            c["leaf"]["src"][order] = np.arange(len(order))
            cost = np.zeros_like(c["cost"]); cost[c["leaf"]["src"]] = c["cost"]
            bsize_of_src = bsize[order]
        else:
            final, count, bsize_of_src = uniform_final(pgeom, origins, 3 if name == "all_8x8" else 0)
        rec, groups = records_and_groups(rng, pkg, bsize_of_src, tabs, T)
        d_rec = None
        if name == "mixed":
            rec["cost"] = cost
            d_rec = T(rec.view(np.uint8).reshape(-1, 72))
            pa = dict(sb=T(c["sb"].view(np.uint8).reshape(nsb, 12)), leaf=T(c["leaf"].view(np.uint8).reshape(-1, 12)), decision=d_rec, partition_bits=T(c["bits"]),
                      pic_width=PIC_W, pic_height=PIC_H, slice_is_intra=0, sq=torch.empty((nsb, mg.NSQ, 16), dtype=torch.uint8, device=dev),
                      final_count=torch.empty((nsb,), dtype=torch.int32, device=dev), final=torch.empty((nsb, mg.MAX_FINAL, 12), dtype=torch.uint8, device=dev))
            pa["lambda"] = bp.LAMBDA
            ok(dsp.partition_decide_frame(pa))
            d_final, d_count = pa["final"], pa["final_count"]
        else:
            d_rec = T(rec.view(np.uint8).reshape(-1, 72))
            d_final, d_count = T(final.view(np.uint8).reshape(nsb, mg.MAX_FINAL, 12)), T(count.view(np.int32))
        planes_a, planes_b = new_planes(), new_planes()
        args = dsp.make_recon_final_args(dict(final=d_final, final_count=d_count, decision=d_rec, groups=groups, recon=planes_a, scratch=scratch, **dims))
        call = lambda: ok(dsp.recon_final_frame(args))

        def bin_only():
            dsp.lib.svt_hip_tune(b"recon_final_bin_only", 1)
            ok(dsp.recon_final_frame(args))
            dsp.lib.svt_hip_tune(b"recon_final_bin_only", 0)

        def hop():
            """the whole replaced path: the list and the records to the host, grouped there, the tables up, the device work"""
            f = d_final.cpu().numpy().view(mg.FINAL_DTYPE).reshape(nsb, mg.MAX_FINAL)
            n = d_count.cpu().numpy().view(np.uint32)
            r = d_rec.cpu().numpy().view(pkg.md_decision_dtype()).reshape(-1)
            scat, inv = composed_tables(f, n, r, groups, rgeom, tabs, [pl.stride(0) for pl in planes_b], T)
            composed_run(dsp, planes_b, scat, inv)
            torch.cuda.synchronize()
            return f, n, scat, inv

        call(); torch.cuda.synchronize()
        f, n, scat, inv = hop()
        for p in range(3):
            assert torch.equal(planes_a[p], planes_b[p]), f"{name}: plane {p} of the composed path differs"
        ent = np.concatenate([f[i, :k] for i, k in enumerate(n.tolist())])
        luma_samples = int(sum(mr.BS_W[b] * mr.BS_H[b] for b in ent["bsize"].tolist()))
        composed = lambda: composed_run(dsp, planes_b, scat, inv)
        hops = []
        for _ in range(3):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            hop()
            hops.append(time.perf_counter() - t0)
        wa, wb, wbin = [], [], []
        for _ in range(nwin):
            wa.append(bp.window(call)); wb.append(bp.window(composed)); wbin.append(bp.window(bin_only))
        ma, mb, mbin, mhop = statistics.median(wa), statistics.median(wb), statistics.median(wbin), statistics.median(hops)
        row = dict(partition=name, nsb=nsb, final_blocks=int(n.sum()), luma_samples=luma_samples, bytes=9 * luma_samples,
                   composed_launches=len(scat) + len(inv), composed_scatters=len(scat), composed_inverse_batches=len(inv),
                   call_ms=ma * 1e3, call_gbps=9 * luma_samples / ma / 1e9, bin_ms=mbin * 1e3, bin_share=mbin / ma,
                   composed_ms=mb * 1e3, composed_over_call=mb / ma, hop_ms=mhop * 1e3, hop_ms_runs=[x * 1e3 for x in hops], hop_over_call=mhop / ma,
                   call_ms_windows=[x * 1e3 for x in wa], composed_ms_windows=[x * 1e3 for x in wb], bin_ms_windows=[x * 1e3 for x in wbin])
        rows.append(row)
        print(json.dumps({k: (round(v, 4) if isinstance(v, float) else v) for k, v in row.items() if not k.endswith("windows")}), flush=True)
    res = dict(device=dsp.device_name(), picture=[PIC_W, PIC_H], planes=[PIC_W, ROWS], quick=a.quick, cache="warm: the same buffers every call",
               composed="per (plane, size) a torch index_put_ scatter of the predictions, per (plane, size, type) one svt_hip_inv_txfm2d_add_batch with d_dst_offsets",
               hop="D2H of the final list, counts and records, numpy grouping, H2D of the index and offset tables, the composed device work; wall clock, median of 3",
               cases=rows)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    json.dump(res, open(a.out, "w"), indent=1)
    print("wrote", a.out)


if __name__ == "__main__":
    main()

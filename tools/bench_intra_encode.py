#!/usr/bin/env python3
"""The intra encode pass in coding order (svt_hip_intra_encode_frame) on 1080p 4:2:0 pictures: 510 superblocks of 64x64 (30 x 17) in planes
of 1920 x 1088, every entry intra, for three final lists:
  all_16x16  every superblock sixteen 16x16
  all_8x8    every superblock sixty-four 8x8
  mixed      three partition trees in turn (4x4 .. 32x32 with the mixed shapes; the 32-level HORZ_A / HORZ_B / VERT_A / VERT_B; 8x8, 8x4, 4x8)
Modes, angle deltas, chroma modes (CfL where the size allows) and transform types are drawn per block; the source is a smooth field with
noise, the quantiser rows those of the fixture.

Per list and for npics 1 and 16, in one process, the call captured into a HIP graph once and replayed (warm caches: the same buffers every
replay; the reconstruction planes are written in place, so every replay after the first predicts from the previous replay's samples: the
same work).  In the same run svt_hip_recon_final_frame on the same lists (one call per picture in one graph): it reconstructs the same
blocks with no dependency between them and no prediction, forward transform or quantiser: a floor, not a target.
Timing: HIP events around windows of back-to-back replays, synchronised before and after, each window >= 0.2 s after a warm-up; alternating
window by window, 5 windows each, median.  Writes profiles/r21_intra_encode.json.
    python tools/bench_intra_encode.py [--out profiles/r21_intra_encode.json] [--quick]"""
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
sys.path.insert(0, os.path.join(ROOT, "tools"))
import __graft_entry__ as ge  # noqa: E402
import make_golden_intra_encode as mi  # noqa: E402
import make_golden_recon_final as mr  # noqa: E402
import bench_partition as bp  # noqa: E402

PIC_W, PIC_H = 1920, 1088
LISTS = {"all_16x16": [mr.SB_16], "all_8x8": [mi.S(mi.S(mi.S(mi.NONE)))], "mixed": [mi.MIX_B, mi.MIX_C, mi.MIX_A]}


def build_list(rng, geom, trees, sb_cols, sb_rows):
    """-> (final [nsb, 256], count [nsb], blk [nsrc], bsize per src); src in order of block size (one recon_final group per size)"""
    nsb = sb_cols * sb_rows
    final = np.zeros((nsb, mi.MAX_FINAL), mi.FINAL_DTYPE)
    count = np.zeros(nsb, np.uint32)
    ents = []
    for sb in range(nsb):
        ox, oy = 64 * (sb % sb_cols), 64 * (sb // sb_cols)
        for k, (mds, part) in enumerate(mr.tile(trees[sb % len(trees)])):
            g = geom[mds]
            final[sb, k] = (mds, ox + int(g["origin_x"]), oy + int(g["origin_y"]), int(g["bsize"]), part, 0)
            ents.append((sb, k, int(g["bsize"]), int(g["txsize"]), int(g["txsize_uv"])))
            count[sb] = k + 1
    order = np.argsort(np.array([e[2] for e in ents]), kind="stable")
    blk = np.zeros(len(ents), mi.BLK_DTYPE)
    bsize_of_src = np.zeros(len(ents), np.int64)
    for src, i in enumerate(order.tolist()):
        sb, k, b, tx, tx_uv = ents[i]
        final["src"][sb, k] = src
        bsize_of_src[src] = b
        mode, delta = mi.LUMA_MODES[int(rng.integers(0, len(mi.LUMA_MODES)))]
        uv = int(rng.integers(0, 14))
        if uv == 13 and (mi.BS_W[b] > 32 or mi.BS_H[b] > 32 or mi.BS_W[b] < 8 or mi.BS_H[b] < 8):
            uv = 0
        ty, tyu = mi.types_of(tx), mi.types_of(tx_uv)
        blk[src] = (1, mode, delta, uv, int(rng.integers(0, 256)), int(rng.integers(0, 8)), ty[int(rng.integers(0, len(ty)))] if rng.random() < 0.3 else 0,
                    tyu[int(rng.integers(0, len(tyu)))] if rng.random() < 0.3 else 0)
    return final, count, blk, bsize_of_src


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r21_intra_encode.json"))
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--quick", action="store_true", help="a 256 x 192 picture, npics 1 and 2, 2 windows (a smoke run)")
    a = ap.parse_args()
    pkg = ge.load_package()
    dsp = pkg.SvtHipDsp(0)
    dev = torch.device("cuda:0")
    geom = mr.load_geometry(dict(np.load(os.path.join(ROOT, "tests", "golden", "recon_final.npz"))))
    gold = dict(np.load(os.path.join(ROOT, "tests", "golden", "intra_encode.npz")))
    qrows = [{k: gold["c0_qrows"][i][j] for j, k in enumerate(mi.QKEYS)} for i in (0, 1)]
    W, H = (256, 192) if a.quick else (PIC_W, PIC_H)
    sb_cols, sb_rows = W // 64, H // 64
    nsb, nwin, pics = sb_cols * sb_rows, 2 if a.quick else a.windows, (1, 2) if a.quick else (1, 16)
    T = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev)
    ok = lambda rc: rc == 0 or sys.exit(dsp.lib.svt_hip_last_error())
    tables = T(dsp.intra_encode_tables())
    dims = dict(width=[W, W // 2, W // 2], height=[H, H // 2, H // 2])
    rows = []

    def graph_of(fn):
        fn(); torch.cuda.synchronize()                                      # warm: nothing is created inside the capture
        g = torch.cuda.CUDAGraph()
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            with torch.cuda.graph(g, stream=side):
                fn()
        torch.cuda.current_stream().wait_stream(side)
        return g

    for name, trees in LISTS.items():
        rng = np.random.default_rng(21021)
        final, count, blk, bsize_of_src = build_list(rng, geom, trees, sb_cols, sb_rows)
        luma_samples = int(sum(mi.BS_W[b] * mi.BS_H[b] for b in bsize_of_src.tolist()))
        src_np = [mi.smooth_noise(rng, H >> (p > 0), W >> (p > 0), 2) for p in range(3)]
        # the floor's inputs: one source group per block size, zero predictions, a DC coefficient per plane block
        rec = np.zeros(len(blk), pkg.md_decision_dtype())
        rec["tx_type"], rec["eob"] = blk["tx_type"], 1
        groups, at = [], 0
        for b in np.unique(bsize_of_src).tolist():
            nb = int((bsize_of_src == b).sum())
            cw, ch = max(mi.BS_W[b] // 2, 4), max(mi.BS_H[b] // 2, 4)
            shapes = [(mi.BS_W[b], mi.BS_H[b]), (cw, ch), (cw, ch)]
            dq = [torch.zeros((nb, min(w, 32) * min(h, 32)), dtype=torch.int32, device=dev) for w, h in shapes]
            for t in dq:
                t[:, 0] = 64
            groups.append(dict(src_first=at, nblocks=nb, bsize=b, tx_type_uv=0, best_pred=[torch.full((nb, h, w), 128, dtype=torch.uint8, device=dev) for w, h in shapes],
                               best_dqcoeff=dq))
            at += nb
        fl_planes = [torch.zeros((H >> (p > 0), W >> (p > 0)), dtype=torch.uint8, device=dev) for p in range(3)]
        fl_in = dict(final=T(final.view(np.uint8).reshape(nsb, mi.MAX_FINAL, 12)), final_count=T(count.view(np.int32)),
                     decision=T(rec.view(np.uint8).reshape(-1, 72)), groups=groups, recon=fl_planes,
                     scratch=torch.empty((dsp.recon_final_scratch_bytes(nsb),), dtype=torch.uint8, device=dev), **dims)
        fl_args = dsp.make_recon_final_args(fl_in)                          # (fl_in keeps the tensors the arguments point into alive)
        for npics in pics:
            src = [T(np.tile(s, (npics, 1))) for s in src_np]
            recon = [torch.full((npics * (H >> (p > 0)), W >> (p > 0)), 128, dtype=torch.uint8, device=dev) for p in range(3)]
            status = torch.zeros((npics, nsb, mi.MAX_FINAL), dtype=torch.uint8, device=dev)
            pitch = [(H >> (p > 0)) * (W >> (p > 0)) for p in range(3)]
            call_in = dict(npics=npics, sb_cols=sb_cols, sb_rows=sb_rows, final=T(np.tile(final.view(np.uint8).reshape(nsb, mi.MAX_FINAL, 12), (npics, 1, 1))),
                           final_count=T(np.tile(count.view(np.int32), npics)), blk=T(blk.view(np.uint8).reshape(-1, 8)), src=src, recon=recon,
                           src_pic_pitch=pitch, recon_pic_pitch=pitch, q_luma=qrows[0], q_chroma=qrows[1], tables=tables, status=status,
                           scratch=torch.empty((dsp.intra_encode_scratch_bytes(npics, nsb),), dtype=torch.uint8, device=dev), **dims)
            args = dsp.make_intra_encode_args(call_in)                      # (call_in keeps the tensors the arguments point into alive)
            g_call = graph_of(lambda: ok(dsp.intra_encode_frame(args)))
            live = np.arange(mi.MAX_FINAL)[None] < count[:, None]
            assert (status.cpu().numpy()[:, live] == 0).all(), f"{name}: an entry was not coded"
            assert all(int((r != 128).sum()) > r.numel() // 2 for r in recon), name

            def floor():
                for _ in range(npics):
                    ok(dsp.recon_final_frame(fl_args))
            g_floor = graph_of(floor)
            wa, wb = [], []
            for _ in range(nwin):
                wa.append(bp.window(g_call.replay)); wb.append(bp.window(g_floor.replay))
            ma, mb = statistics.median(wa), statistics.median(wb)
            assert (status.cpu().numpy()[:, live] == 0).all(), f"{name}: an entry was not coded in the timed replays"
            launches = dsp.intra_encode_launches(sb_cols, sb_rows, 3)
            row = dict(list=name, npics=npics, nsb=nsb, blocks_per_picture=int(count.sum()), luma_samples_per_picture=luma_samples, launches=launches,
                       steps=sb_cols + 2 * (sb_rows - 1), call_ms=ma * 1e3, call_ms_per_picture=ma * 1e3 / npics, us_per_launch=ma * 1e6 / launches,
                       floor_ms=mb * 1e3, floor_ms_per_picture=mb * 1e3 / npics, call_over_floor=ma / mb,
                       call_ms_windows=[x * 1e3 for x in wa], floor_ms_windows=[x * 1e3 for x in wb])
            rows.append(row)
            print(json.dumps({k: (round(v, 4) if isinstance(v, float) else v) for k, v in row.items() if not k.endswith("windows")}), flush=True)
    res = dict(device=dsp.device_name(), picture=[W, H], quick=a.quick, cache="warm: the same buffers every replay", timed="one HIP graph replay per call",
               floor="svt_hip_recon_final_frame on the same list, one call per picture in one graph: no prediction, forward transform, quantiser or dependency",
               cases=rows)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    json.dump(res, open(a.out, "w"), indent=1)
    print("wrote", a.out)


if __name__ == "__main__":
    main()

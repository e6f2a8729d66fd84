#!/usr/bin/env python3
"""The partition decision (svt_hip_partition_decide_frame) on a 1080p picture: 510 superblocks of 64x64 (30 x 17, the bottom row crossing
the picture edge at 1080), leaf lists as MDC makes them (blocks outside the picture dropped), synthetic costs and partitionFacBits (the
fixture generator's, tests/golden/make_golden_partition.py), a non-I slice, lambda 29041.  Three list classes:
  squares      the squares 64 .. 8 (85 entries per interior superblock)
  squares_h_v  the same with the H and V shapes (425 entries)
  all_blocks   every block, 1 101 entries

Per class, in one process:
  call         svt_hip_partition_decide_frame reading the cost from the 72-byte decision records, without and with d_final_decision
  replaced     the path the call replaces: D2H of the decision records, the walk in numpy (the project's restatement np_partition, which
               goes superblock by superblock), H2D of the final block list; wall-clock, synchronised, median of 3; its squares, counts and
               final blocks are compared with the call's before anything is timed
Timing of the device calls: HIP events around windows of back-to-back calls, synchronised before and after, each window >= 0.2 s after a
warm-up call; alternating window by window, 7 windows each, median.  Writes profiles/r19_partition.json.
    python tools/bench_partition.py [--out profiles/r19_partition.json] [--quick]"""
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
import make_golden_partition as mg  # noqa: E402

PIC_W, PIC_H = 1920, 1080
LAMBDA = 29041
CLASSES = (("squares", dict(min_size=8, shapes=lambda rng, size, s, k: False)),
           ("squares_h_v", dict(min_size=8, shapes=lambda rng, size, s, k: s < 3)),
           ("all_blocks", dict(min_size=4, shapes=lambda rng, size, s, k: True, contexts=True)))


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


def picture_case(rng, geom, kw, origins):
    """the class's lists for the given superblocks -> a case dict as the fixture generator's"""
    sb, rows = np.zeros(len(origins), mg.SB_DTYPE), []
    for i, (ox, oy) in enumerate(origins):
        r = mg.build_list(rng, geom, PIC_W, PIC_H, ox, oy, **kw)
        sb["leaf_first"][i], sb["leaf_count"][i], sb["origin_x"][i], sb["origin_y"][i] = len(rows), len(r), ox, oy
        rows += r
    leaf = np.zeros(len(rows), mg.LEAF_DTYPE)
    cols = np.array(rows, np.int64).reshape(-1, 5)
    for j, key in enumerate(("mds_idx", "split_flag", "tot_d1_blocks", "left_partition", "above_partition")):
        leaf[key] = cols[:, j]
    leaf["src"] = np.arange(len(leaf))
    return dict(bits=rng.integers(0, 1 << 13, mg.BITS_SHAPE).astype(np.int32), lam=np.uint32(LAMBDA), pic_width=np.uint32(PIC_W), pic_height=np.uint32(PIC_H),
                slice_is_intra=np.int32(0), sb=sb, leaf=leaf, cost=mg.area_costs(rng, geom, leaf["mds_idx"].astype(np.int64), 0.3))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r19_partition.json"))
    ap.add_argument("--windows", type=int, default=7)
    ap.add_argument("--quick", action="store_true", help="the first 34 superblocks, 3 windows (a smoke run)")
    a = ap.parse_args()
    pkg = ge.load_package()
    dsp = pkg.SvtHipDsp(0)
    dev = torch.device("cuda:0")
    geom = mg.load_geometry(dict(np.load(os.path.join(ROOT, "tests", "golden", "partition.npz"))))
    origins = [(64 * x, 64 * y) for y in range((PIC_H + 63) // 64) for x in range((PIC_W + 63) // 64)]
    origins = origins[-34:] if a.quick else origins
    nsb, nwin = len(origins), 3 if a.quick else a.windows
    T = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev)
    E = lambda shape, dt: torch.empty(shape, dtype=dt, device=dev)
    ok = lambda rc: rc == 0 or sys.exit(dsp.lib.svt_hip_last_error())
    rows = []
    for name, kw in CLASSES:
        rng = np.random.default_rng(19019)
        c = picture_case(rng, geom, kw, origins)
        nleaves = len(c["leaf"])
        rec = np.zeros(nleaves, pkg.md_decision_dtype())
        rec["cost"], rec["cand"] = c["cost"], np.arange(nleaves) % 64
        base = dict(sb=T(c["sb"].view(np.uint8).reshape(nsb, 12)), leaf=T(c["leaf"].view(np.uint8).reshape(-1, 12)), decision=T(rec.view(np.uint8).reshape(-1, 72)),
                    partition_bits=T(c["bits"]), pic_width=PIC_W, pic_height=PIC_H, slice_is_intra=0, sq=E((nsb, mg.NSQ, 16), torch.uint8),
                    final_count=E((nsb,), torch.int32), final=E((nsb, mg.MAX_FINAL, 12), torch.uint8))
        base["lambda"] = LAMBDA
        full = dict(base, final_decision=E((nsb, mg.MAX_FINAL, 72), torch.uint8))
        lean_args, full_args = dsp.make_partition_args(base), dsp.make_partition_args(full)
        lean_call = lambda: ok(dsp.partition_decide_frame(lean_args))
        full_call = lambda: ok(dsp.partition_decide_frame(full_args))

        def replaced():
            """-> (squares, counts, final blocks); the final list ends on the device"""
            got = base["decision"].cpu().numpy().view(pkg.md_decision_dtype()).reshape(-1)
            sq, count, final = mg.np_partition(dict(c, cost=got["cost"]), geom)
            up = T(final.view(np.uint8).reshape(-1, 12)), T(count.view(np.int32))
            torch.cuda.synchronize()
            return sq, count, final, up

        lean_call(); full_call(); torch.cuda.synchronize()
        sq, count, final, _ = replaced()
        assert np.array_equal(base["sq"].cpu().numpy().view(mg.SQ_DTYPE).reshape(nsb, mg.NSQ), sq), "the replaced path's squares"
        assert np.array_equal(base["final_count"].cpu().numpy().view(np.uint32), count), "the replaced path's counts"
        got_final = base["final"].cpu().numpy()
        assert np.array_equal(np.concatenate([got_final[i, :n] for i, n in enumerate(count.tolist())]).view(mg.FINAL_DTYPE).reshape(-1), final), "the final blocks"
        rep = []
        for _ in range(3):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            replaced()
            rep.append(time.perf_counter() - t0)
        lean_w, full_w = [], []
        for _ in range(nwin):
            lean_w.append(window(lean_call)); full_w.append(window(full_call))
        m_lean, m_full, m_rep = statistics.median(lean_w), statistics.median(full_w), statistics.median(rep)
        row = dict(lists=name, nsb=nsb, nleaves=nleaves, leaves_per_interior_sb=int(c["sb"]["leaf_count"].max()), final_blocks=int(count.sum()),
                   edge_superblocks=int(sum(1 for ox, oy in origins if ox + 64 > PIC_W or oy + 64 > PIC_H)),
                   call_ms=m_lean * 1e3, call_with_final_decision_ms=m_full * 1e3, replaced_ms=m_rep * 1e3, replaced_ms_runs=[x * 1e3 for x in rep],
                   replaced_over_call=m_rep / m_lean, replaced_over_call_with_final_decision=m_rep / m_full,
                   call_ms_windows=[x * 1e3 for x in lean_w], call_with_final_decision_ms_windows=[x * 1e3 for x in full_w])
        rows.append(row)
        print(json.dumps({k: (round(v, 4) if isinstance(v, float) else v) for k, v in row.items() if not k.endswith("windows")}), flush=True)
    res = dict(device=dsp.device_name(), picture=[PIC_W, PIC_H], lambda_=LAMBDA, quick=a.quick,
               replaced="D2H of the 72-byte decision records, numpy walk (np_partition, superblock by superblock), H2D of the final list and counts; wall clock, median of 3",
               cases=rows)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    json.dump(res, open(a.out, "w"), indent=1)
    print("wrote", a.out)


if __name__ == "__main__":
    main()

"""Writes tests/golden/fast_search_ref.npz: whole blocks through the reference's OWN inject_intra_candidates -> perform_fast_loop ->
sort_fast_loop_candidates (oracle/ref_md.c: ref_md_fast_search, compiled into oracle/_ref/libsvtref.so), as md_encode_block runs them
(EbProductCodingLoop.c:3026-3140).  Data only; needs the compiled reference:

    python tests/golden/make_golden_fast_search_ref.py

Nothing in the expected values is restated: the candidate list is inject_intra_candidates', the predictions come through
ProductMdFastPuPrediction -> AV1IntraPredictionCL -> av1_predict_intra_block, the distortions through the reference's table entries for
asm_type 1 (AVX2), the costs through av1_intra_fast_cost, the buffers through perform_fast_loop's second loop, the two index arrays and
ref_fast_cost through sort_fast_loop_candidates.  The maker only converts them to the interface's form (mg.slots_of: the list index per
full-loop slot, sorted as slots), asserts that mg.ref_fast_pick / mg.np_fast_pick chained after the stored distortions give the same,
and that the oracle's build_intra_predictors on the stored neighbours and descriptors gives the survivors' predictions.

Chroma is blind at mode decision (chroma_level 1, CHROMA_MODE_1): luma predictions and distortions only, while the uv MODE bits are still
costed (has_chroma).  The uv list of a case is the one of its blocks with chroma; a block without (blk_geom->has_uv 0: 4-sample sides at even
positions) may get another uv list from the reference (disable_ang_uv, EbModeDecision.c:2428), which its cost never reads.

Cases (8 blocks each): 4x4, 8x8, 4x16, 16x4, 32x32, 64x64; the non-decoupled call (:3103-3131, SAD), the decoupled intra call (:3040-3078)
with SSD_SEARCH on an I slice (square sizes; the AVX2-flavour SSD) and with SAD on a P slice (full_recon_intra_search_count 1); nfl 1, 3,
12, 40; intra_pred_mode 0 and 3 (5 candidates); origins at the picture's top and left edges and at both mi parities; one case with a
uniform source, uniform neighbours and all-zero rate tables (ties).

Layout, per case ci (prefix f"c{ci}_"): params int64 [10] (mg.PARAM_KEYS; nfl = full_recon_search_count as perform_fast_loop saw it),
modes / deltas / uv_modes / uv_deltas, blk uint8 [B, 8] (svt_hip_fast_pick_blk), rates int32 [877], xy int32 [B, 2] (x, y in the picture),
top / left uint8 [B, PITCH] (element 0 the corner), iblk uint8 [B, 8] (svt_hip_intra_blk), pic (index into pictures), path int32 [4]
(decoupled, ssd_search, nfl given, intra_pred_mode); expected: cand, sorted uint8 [B, n], cost uint64 [B, n], rate uint32 [B, n, 2],
ref_fast_cost uint64 [B], all_cost uint64 [B, C], dist uint64 [B, C] (luma_fast_distortion), pred_out uint8 [B, n, H, W]."""
import ctypes
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)
import make_golden_fast_pick as mg  # noqa: E402
from svtlibs import SHAPE_OF_PARTITION, TX_H, TX_W, oracle, ptr  # noqa: E402

OUT = os.path.join(HERE, "fast_search_ref.npz")
NB = 8
PITCH = 1 + 2 * 64
PIC_W, PIC_H = 256, 128
FAST_LAMBDA, FULL_LAMBDA = 29041, 13107
QINDEX, AC_DEQUANT = 60, 156
PARTITION_OF_SHAPE = {v: k for k, v in SHAPE_OF_PARTITION.items()}
OUTPUTS = ("cand", "sorted", "cost", "rate", "ref_fast_cost", "all_cost", "dist", "pred_out")

# name, tx_size, decoupled, ssd_search, slice_is_intra, nfl, intra_pred_mode, kind
CASES = [
    ("4x4_sad_nfl3", 0, 0, 0, 1, 3, 0, "rand"),
    ("4x4_sad_nfl40_p", 0, 1, 0, 0, 40, 0, "rand"),             # sq_size 4: never decoupled; 13 candidates, no scratch
    ("8x8_sad_nfl12_p", 1, 0, 0, 0, 12, 0, "rand"),
    ("8x8_ssd_nfl3", 1, 1, 1, 1, 3, 0, "rand"),
    ("8x8_ssd_nfl40", 1, 1, 1, 1, 40, 0, "rand"),
    ("8x8_sad_decoupled_p", 1, 1, 0, 0, 12, 0, "rand"),         # P slice: one intra full-loop candidate, two buffers
    ("8x8_sad_ties", 1, 0, 0, 1, 12, 0, "uniform"),
    ("8x8_sad_mode3_nfl12", 1, 0, 0, 1, 12, 3, "rand"),         # 5 candidates <= nfl
    ("4x16_sad_nfl3", 13, 0, 0, 1, 3, 0, "rand"),
    ("16x4_sad_nfl1_p", 14, 0, 0, 0, 1, 0, "rand"),
    ("32x32_ssd_nfl12", 3, 1, 1, 1, 12, 0, "rand"),
    ("32x32_sad_nfl3_p", 3, 0, 0, 0, 3, 0, "rand"),
    ("64x64_ssd_nfl3", 4, 1, 1, 1, 3, 0, "rand"),
    ("64x64_sad_decoupled_p", 4, 1, 0, 0, 3, 0, "rand"),
]
NCASES = len(CASES)
CASE_NAMES = [c[0] for c in CASES]


def origins(w, h, rng):
    """8 origins of a W x H block in the picture, multiples of the block's size (so the geometry table has the block at that place in its
    superblock): the corner, the top edge, the left edge, and both parities of x / 4 and y / 4 where the size allows them"""
    out = [(x, y) for x, y in ((0, 0), (w, 0), (0, h), (w, h), (2 * w, h), (w, 2 * h)) if x + w <= PIC_W and y + h <= PIC_H]
    while len(out) < NB:
        x, y = int(rng.integers(0, PIC_W // w)) * w, int(rng.integers(0, PIC_H // h)) * h
        if (x, y) not in out:
            out.append((x, y))
    return out


def ref_block(L, P, src, top, left, rates):
    """one ref_md_fast_search call -> dict of its outputs"""
    w, h = int(P[5]), int(P[6])
    o = dict(out_i=np.zeros(8, np.int32), list=np.zeros((64, 7), np.int32), buf_cand=np.zeros(42, np.int32), buf_cost=np.zeros(42, np.uint64),
             best=np.zeros(42, np.uint8), sorted=np.zeros(40, np.uint8), ref=np.zeros(1, np.uint64), rate=np.zeros((64, 2), np.uint32),
             dist=np.zeros(64, np.uint64), cost=np.zeros(64, np.uint64), pred=np.zeros((42, h, w), np.uint8))
    rc = L.ref_md_fast_search(ptr(P), ptr(src), ptr(top), ptr(left), ctypes.c_uint64(FAST_LAMBDA), ctypes.c_uint64(FULL_LAMBDA), ptr(rates),
                              ptr(o["out_i"]), ptr(o["list"]), ptr(o["buf_cand"]), ptr(o["buf_cost"]), ptr(o["best"]), ptr(o["sorted"]), ptr(o["ref"]),
                              ptr(o["rate"]), ptr(o["dist"]), ptr(o["cost"]), ptr(o["pred"]))
    assert rc == 0, rc
    return o


def descriptor(O, x, y, w, h, tx, bsize, shape, top_mode, left_mode):
    """svt_hip_intra_blk of the block: the available samples and filt_type from the oracle's availability glue (pinned to the reference's
    av1_predict_intra_block by tests/golden/bip.npz) on the mode-info grid ref_md_fast_search builds"""
    mi_rows, mi_cols = PIC_H // 4, PIC_W // 4
    grid = np.zeros((mi_rows, mi_cols), np.uint8)
    if y:
        grid[y // 4 - 1, x // 4] = top_mode
    if x:
        grid[y // 4, x // 4 - 1] = left_mode
    out5 = np.zeros(5, np.int32)
    tile = np.array([0, mi_rows, 0, mi_cols], np.int32)
    O.svt_oracle_intra_neighbor_px(0, 16, mi_rows, mi_cols, ptr(grid), ptr(grid), ptr(tile), PARTITION_OF_SHAPE[shape], bsize, tx, 0, x, y, 0, 0, w, h, ptr(out5))
    return np.array([0, 0, out5[4], 0, out5[0], out5[1], out5[2], out5[3]], np.uint8)          # disable_edge_filter 0: DIS_EDGE_FIL is 0


def make_case(L, O, ci, pictures):
    name, tx, decoupled, ssd, intra, nfl, ipm, kind = CASES[ci]
    rng = np.random.default_rng(4400 + ci)
    w, h = TX_W[tx], TX_H[tx]
    pic = 1 if kind == "uniform" else 0
    src = pictures[pic]
    rates = mg.make_rates("zero" if kind == "uniform" else "rand", rng)
    blk = np.zeros(NB, mg.BLK_DTYPE)
    blk["top_mode"], blk["left_mode"] = rng.integers(0, 13, NB), rng.integers(0, 13, NB)
    blk["skip_mode_ctx"], blk["is_inter_ctx"] = rng.integers(0, 3, NB), rng.integers(0, 4, NB)
    xy = np.array(origins(w, h, rng), np.int32)
    tops, lefts, iblk, res = np.zeros((NB, PITCH), np.uint8), np.zeros((NB, PITCH), np.uint8), np.zeros((NB, 8), np.uint8), []
    for b in range(NB):
        if kind == "uniform":
            tops[b], lefts[b] = 77, 77
        else:
            tops[b], lefts[b] = rng.integers(0, 256, PITCH), rng.integers(0, 256, PITCH)
        lefts[b, 0] = tops[b, 0]                                                     # one corner sample
        x, y = int(xy[b, 0]), int(xy[b, 1])
        P = np.array([PIC_W, PIC_H, PIC_W, x, y, w, h, blk["top_mode"][b], blk["left_mode"][b], blk["skip_mode_ctx"][b], blk["is_inter_ctx"][b],
                      decoupled, ssd, intra, nfl, ipm, QINDEX, AC_DEQUANT, 1, 1], np.int32)
        r = ref_block(L, P, src, np.ascontiguousarray(tops[b, :1 + 2 * w]), np.ascontiguousarray(lefts[b, :1 + 2 * h]), rates)
        res.append(r)
        bsize, has_uv, shape = int(r["out_i"][3]), int(r["out_i"][4]), int(r["out_i"][6])
        blk["has_chroma"][b] = has_uv & mg.np_is_chroma_reference(y >> 2, x >> 2, bsize)
        iblk[b] = descriptor(O, x, y, w, h, tx, bsize, shape, int(blk["top_mode"][b]), int(blk["left_mode"][b]))
    C, n = int(res[0]["out_i"][0]), int(res[0]["out_i"][2])
    assert all(int(r["out_i"][0]) == C and int(r["out_i"][2]) == n and int(r["out_i"][3]) == int(res[0]["out_i"][3]) for r in res)
    bsize = int(res[0]["out_i"][3])
    assert bsize == mg.bsizes_of_tx(tx)[0]
    lists = [r["list"][:C] for r in res]
    with_uv = [b for b in range(NB) if blk["has_chroma"][b]]
    lst = lists[with_uv[0] if with_uv else 0]
    for b in range(NB):
        assert np.array_equal(lists[b][:, [0, 1, 4, 6]], lst[:, [0, 1, 4, 6]]), (name, b)          # the luma list is the size's
        if blk["has_chroma"][b]:
            assert np.array_equal(lists[b], lst), (name, b)
    use_angle_delta = int(bsize >= 3)                                                # EbModeDecision.c:2385
    assert all(int(v[6]) == (use_angle_delta and int(v[4])) and int(v[4]) == int(1 <= v[0] <= 8) and int(v[5]) == int(1 <= v[2] <= 8) for v in lst)
    sq_size, shape = int(res[0]["out_i"][7]), int(res[0]["out_i"][6])
    took_decoupled = bool(decoupled) and sq_size > 4 and shape == 0 and nfl > 1          # EbProductCodingLoop.c:3038
    metric = mg.SSD if (ssd and took_decoupled) else mg.SAD                              # :3076 against :3128
    P = dict(tx_size=tx, bsize=bsize, bsize_uv=mg.bsizes_of_tx(tx)[1], modes=lst[:, 0].astype(np.uint8), deltas=lst[:, 1].astype(np.int8),
             uv_modes=lst[:, 2].astype(np.uint8), uv_deltas=lst[:, 3].astype(np.int8), use_angle_delta=use_angle_delta, nfl=n, slice_is_intra=intra,
             ac_dequant_q3=AC_DEQUANT, intrabc_bits=0, metric=metric)
    P["lambda"] = FULL_LAMBDA if metric == mg.SSD else FAST_LAMBDA
    out = dict(cand=np.zeros((NB, n), np.uint8), sorted=np.zeros((NB, n), np.uint8), cost=np.zeros((NB, n), np.uint64), rate=np.zeros((NB, n, 2), np.uint32),
               ref_fast_cost=np.zeros(NB, np.uint64), all_cost=np.zeros((NB, C), np.uint64), dist=np.zeros((NB, C), np.uint64),
               pred_out=np.zeros((NB, n, h, w), np.uint8))
    for b, r in enumerate(res):
        nbuf = int(r["out_i"][1])
        assert nbuf == (n + 1 if C > n else n) and int(r["out_i"][5]) == int(C > n)
        best, srt = r["best"][:nbuf].tolist(), r["sorted"][:n].tolist()
        cand, slots = mg.slots_of(best, srt, r["buf_cand"][:nbuf].tolist(), n)
        out["cand"][b], out["sorted"][b], out["ref_fast_cost"][b] = cand, slots, r["ref"][0]
        out["cost"][b] = [r["buf_cost"][best[k]] for k in range(n)]
        out["rate"][b] = r["rate"][cand]
        out["all_cost"][b], out["dist"][b] = r["cost"][:C], r["dist"][:C]
        out["pred_out"][b] = [r["pred"][best[k]] for k in range(n)]
        assert all(int(out["cost"][b, k]) == int(r["cost"][cand[k]]) for k in range(n)), (name, b)   # a buffer's cost is its candidate's
        for k in range(n):                                                           # the descriptors and neighbours reproduce the survivors
            d = np.zeros((h, w), np.uint8)
            O.svt_oracle_build_intra_predictors(0, ctypes.c_void_p(tops[b].ctypes.data + 1), ctypes.c_void_p(lefts[b].ctypes.data + 1), ptr(d), w,
                                                int(P["modes"][cand[k]]), int(P["deltas"][cand[k]]), tx, 0, int(iblk[b, 4]), int(iblk[b, 5]), int(iblk[b, 6]),
                                                int(iblk[b, 7]), int(iblk[b, 2]), 8)
            assert np.array_equal(d, out["pred_out"][b, k]), (name, b, k)
    return dict(P=P, blk=blk, rates=rates, xy=xy, top=tops, left=lefts, iblk=iblk, pic=pic, path=np.array([decoupled, ssd, nfl, ipm], np.int32), out=out)


def case_of(z, ci):
    """(P, blk, rates, extras dict, expected outputs) of fixture case ci"""
    p = f"c{ci}_"
    P = {k: int(v) for k, v in zip(mg.PARAM_KEYS, z[p + "params"])}
    for k in ("modes", "deltas", "uv_modes", "uv_deltas"):
        P[k] = z[p + k]
    extra = {k: z[p + k] for k in ("xy", "top", "left", "iblk", "path")}
    extra["src"] = z["pictures"][int(z[p + "pic"])]
    return P, z[p + "blk"].view(mg.BLK_DTYPE).reshape(-1), z[p + "rates"], extra, {k: z[p + k] for k in OUTPUTS}


def coverage(z):
    """the conditions the tests rely on the fixture to meet, counted over its cases"""
    c = dict(ties=0, ref_not_min=0, has_chroma=set(), slices=set(), metrics=set(), no_scratch=0, scratch=0, nfl=set(), top_edge=0, left_edge=0, parities=set())
    for ci in range(NCASES):
        P, blk, _, extra, want = case_of(z, ci)
        c["ties"] += int(sum(len(set(row.tolist())) < len(row) for row in want["cost"]))
        c["ref_not_min"] += int((want["ref_fast_cost"] != np.minimum(want["cost"].min(axis=1), np.uint64(mg.MAX_MODE_COST))).sum())
        c["has_chroma"] |= set(blk["has_chroma"].tolist())
        c["slices"].add(P["slice_is_intra"]); c["metrics"].add(P["metric"]); c["nfl"].add(int(extra["path"][2]))
        c["no_scratch" if want["all_cost"].shape[1] <= int(extra["path"][2]) else "scratch"] += 1
        c["top_edge"] += int((extra["xy"][:, 1] == 0).sum()); c["left_edge"] += int((extra["xy"][:, 0] == 0).sum())
        c["parities"] |= {(int(x) >> 2 & 1, int(y) >> 2 & 1) for x, y in extra["xy"]}
    return c


def check_coverage(z):
    c = coverage(z)
    assert c["ties"] > 0 and c["ref_not_min"] > 0 and c["has_chroma"] == {0, 1} and c["slices"] == {0, 1} and c["metrics"] == {mg.SAD, mg.SSD}, c
    assert c["no_scratch"] > 0 and c["scratch"] > 0 and c["nfl"] == {1, 3, 12, 40} and c["top_edge"] and c["left_edge"] and len(c["parities"]) == 4, c
    return c


def check_restatement(z):
    """mg.ref_fast_pick and mg.np_fast_pick, chained after the fixture's own distortions, give what the reference's whole function gave"""
    for ci in range(NCASES):
        P, blk, rates, _, want = case_of(z, ci)
        for fn in (mg.ref_fast_pick, mg.np_fast_pick):
            got = fn(P, want["dist"], None, None, blk, rates)
            for k in mg.OUTPUTS:
                assert got[k].dtype == want[k].dtype and np.array_equal(got[k], want[k]), (CASE_NAMES[ci], fn.__name__, k)


def main():
    L = mg.ref_lib()
    assert L is not None, "needs oracle/_ref/libsvtref.so (make -C oracle ref)"
    O = oracle()
    rng = np.random.default_rng(4399)
    pictures = np.stack([rng.integers(0, 256, (PIC_H, PIC_W)).astype(np.uint8), np.full((PIC_H, PIC_W), 93, np.uint8)])
    d = {"names": np.array(CASE_NAMES), "pictures": pictures}
    for ci in range(NCASES):
        c = make_case(L, O, ci, pictures)
        p = f"c{ci}_"
        d[p + "params"] = np.array([c["P"][k] for k in mg.PARAM_KEYS], np.int64)
        for k in ("modes", "deltas", "uv_modes", "uv_deltas"):
            d[p + k] = c["P"][k]
        d[p + "blk"], d[p + "rates"] = c["blk"].view(np.uint8).reshape(-1, 8), c["rates"]
        for k in ("xy", "top", "left", "iblk", "path"):
            d[p + k] = c[k]
        d[p + "pic"] = np.int32(c["pic"])
        for k in OUTPUTS:
            d[p + k] = c["out"][k]
    np.savez_compressed(OUT, **d)
    z = np.load(OUT)
    print(f"wrote {OUT}: {NCASES} cases, {os.path.getsize(OUT)} bytes; coverage {check_coverage(z)}")
    check_restatement(z)
    print("mg.ref_fast_pick and mg.np_fast_pick reproduce every output of every case")


if __name__ == "__main__":
    main()

"""GPU: svt_hip_recon_final_frame (the reconstruction of the final block list into picture planes and the superblock coefficient
stream) against the fixture (tests/golden/recon_final.npz: the reference's av1_inv_transform_recon8bit per plane block and the
generator's walk around it), byte for byte, into poisoned outputs: what the call may not write must keep the poison."""
import os
import sys

import numpy as np
import pytest
import torch

import layouts
import poison
from poison import poisoned_outputs  # noqa: F401

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden", "recon_final.npz")
PART_GOLD = os.path.join(ROOT, "tests", "golden", "partition.npz")
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
import make_golden_recon_final as mr  # noqa: E402
import make_golden_partition as mg  # noqa: E402

INVALID = -2
OPTIONAL = ("status", "coeff_offset", "sb_qcoeff")


@pytest.fixture(scope="module")
def gold():
    z = dict(np.load(GOLD))
    geom = mr.load_geometry(z)
    return z, geom, mr.bsize_tables(geom)


def fill_byte():
    return poison._active.fill_byte


def dev(a):
    a = np.ascontiguousarray(a)
    view = {np.dtype(np.uint64): np.int64, np.dtype(np.uint32): np.int32}.get(a.dtype)
    return torch.from_numpy(a.view(view) if view else a).to(DEV)


def args_of(dsp, c, tabs, planes=3, optional=OPTIONAL):
    """the call's dict for case inputs c with fresh poisoned outputs"""
    nsb = len(c["count"])
    groups = []
    for g in mr.case_groups(c, tabs):
        d = dict(src_first=g["src_first"], nblocks=g["nblocks"], bsize=g["bsize"], tx_type_uv=g["tx_type_uv"])
        if g["nblocks"]:
            d["best_pred"], d["best_dqcoeff"], d["best_qcoeff"] = ([dev(x) for x in g[k][:planes]] for k in ("pred", "dq", "q"))
        groups.append(d)
    a = dict(final=dev(c["final"].view(np.uint8).reshape(nsb, mr.MAX_FINAL, 12)), final_count=dev(c["count"]),
             decision=dev(c["decision"].view(np.uint8).reshape(-1, 72)), groups=groups, planes=planes,
             recon=[poison.tensor((int(c["rows"][p]), int(c["stride"][p])), torch.uint8, DEV) for p in range(planes)],
             width=c["width"].tolist(), height=c["height"].tolist(),
             scratch=torch.empty((dsp.recon_final_scratch_bytes(nsb),), dtype=torch.uint8, device=DEV))
    if "status" in optional:
        a["status"] = poison.tensor((nsb, mr.MAX_FINAL), torch.uint8, DEV)
    if "coeff_offset" in optional:
        a["coeff_offset"] = poison.tensor((nsb, mr.MAX_FINAL, 2), torch.int32, DEV)
    if "sb_qcoeff" in optional:
        a["sb_qcoeff"] = [poison.tensor((nsb, mr.SPAN[p]), torch.int32, DEV) for p in range(planes)]
    return a


def run(dsp, a):
    assert dsp.recon_final_frame(a) == 0, dsp.lib.svt_hip_last_error()
    torch.cuda.synchronize()


def outputs_of(a):
    return list(a["recon"]) + [a[k] for k in ("status", "coeff_offset") if a.get(k) is not None] + list(a.get("sb_qcoeff") or ())


def untouched(a):
    return all(bool((t.view(torch.uint8) == fill_byte()).all()) for t in outputs_of(a))


def check(a, c, o):
    """every output against the fixture where its mask is set, and the poison everywhere else"""
    fill = fill_byte()
    fill32 = np.frombuffer(bytes([fill] * 4), np.int32)[0]
    live = np.arange(mr.MAX_FINAL)[None] < np.minimum(c["count"], mr.MAX_FINAL)[:, None]
    for p, t in enumerate(a["recon"]):
        got, want, mask = t.cpu().numpy(), o[f"recon{p}"], o[f"rmask{p}"]
        bad = np.nonzero((got != want) & mask)
        assert not len(bad[0]), (p, bad[0][:8], bad[1][:8], got[bad][:8], want[bad][:8])
        assert (got[~mask] == fill).all(), (p, np.nonzero((got != fill) & ~mask)[0][:8])
    if a.get("status") is not None:
        got = a["status"].cpu().numpy()
        assert np.array_equal(got[live], o["status"][live]), np.nonzero((got != o["status"]) & live)
        assert (got[~live] == fill).all()
    if a.get("coeff_offset") is not None:
        got = a["coeff_offset"].cpu().numpy().view(np.uint32)
        assert np.array_equal(got[live], o["offset"][live]), np.nonzero((got != o["offset"]) & live[..., None])
        assert (got[~live].view(np.int32) == fill32).all()
    for p, t in enumerate(a.get("sb_qcoeff") or ()):
        got, want, mask = t.cpu().numpy(), o[f"sbq{p}"], o[f"qmask{p}"]
        bad = np.nonzero((got != want) & mask)
        assert not len(bad[0]), (p, bad[0][:8], bad[1][:8], got[bad][:8], want[bad][:8])
        assert (got[~mask] == fill32).all(), p


@pytest.mark.parametrize("k", range(len(mr.ALL_NAMES)), ids=mr.ALL_NAMES)
def test_case_equals_the_fixture(dsp, gold, k):
    z, geom, tabs = gold
    c, o = mr.load_case(z, k, tabs)
    a = args_of(dsp, c, tabs)
    run(dsp, a)
    check(a, c, o)


def test_planes_laid_out_unlike_each_other_equal_the_fixture(dsp, gold):
    """skips (96 x 80 in 128 x 128 of superblocks): stride[0 .. 2] odd, all different and chroma's neither luma's nor half of it; the
    picture area of each plane alone in a poisoned allocation, so a sample written with another plane's stride lands on a guard"""
    z, geom, tabs = gold
    c, o = mr.load_case(z, mr.ALL_NAMES.index("skips"), tabs)
    w, h = int(c["width"][0]), int(c["height"][0])
    spec = layouts.picture_spec("svt_hip_recon_final_frame", w, h, ("recon",))
    lay = layouts.distinct_layouts(spec)
    a = args_of(dsp, c, tabs)
    area = [np.full((int(c["height"][p]), int(c["width"][p])), fill_byte(), np.uint8) for p in range(3)]
    recon, placed = layouts.place_operand(spec, lay, "recon", area, 1, fill_byte())
    a.update(recon=list(recon), stride=[lay[f"recon.{q}"].stride for q in "yuv"])
    run(dsp, a)
    o = dict(o)
    for p in range(3):                                                  # check() on the picture area: nothing is written outside it
        hh, ww = area[p].shape
        assert not o[f"rmask{p}"][hh:].any() and not o[f"rmask{p}"][:, ww:].any()
        o[f"recon{p}"], o[f"rmask{p}"] = o[f"recon{p}"][:hh, :ww], o[f"rmask{p}"][:hh, :ww]
    check(a, c, o)
    layouts.assert_all_intact(placed, fill_byte(), written=True)


@pytest.mark.parametrize("name", ["main2", "skips"])
def test_luma_only_and_without_the_optional_outputs(dsp, gold, name):
    """the same planes, status, offsets and stream whatever else the call is asked for"""
    z, geom, tabs = gold
    c, o = mr.load_case(z, mr.ALL_NAMES.index(name), tabs)
    for planes, optional in ((1, OPTIONAL), (3, ()), (1, ()), (3, ("status",)), (3, ("coeff_offset",)), (1, ("sb_qcoeff",))):
        a = args_of(dsp, c, tabs, planes, optional)
        run(dsp, a)
        check(a, c, o)


def chain_inputs(pz, tabs, geom, rng, name):
    """a partition fixture case whose records carry what the reconstruction reads: the leaves renumbered so that the records of one
    block size are contiguous (a source group each), costs moved with them, tx_type and eob per record, predictions and coefficients"""
    pc, sq, count, final = mg.load_case(pz, mg.CASE_NAMES.index(name))
    pgeom = mg.load_geometry(pz)
    bsize = pgeom["bsize"][pc["leaf"]["mds_idx"]].astype(np.int64)
    by_old = np.argsort(bsize[np.argsort(pc["leaf"]["src"])], kind="stable")       # old src values in the order of their block size
    perm = np.zeros(len(by_old), np.uint32)
    perm[by_old] = np.arange(len(by_old))                                           # old src -> new src
    leaf = pc["leaf"].copy()
    leaf["src"] = perm[pc["leaf"]["src"]]
    cost = np.zeros_like(pc["cost"])
    cost[perm] = pc["cost"]
    bsize_of_src = np.zeros(len(leaf), np.int64)
    bsize_of_src[leaf["src"]] = bsize
    dec = np.zeros(len(leaf), mr.DEC_DTYPE)
    dec["cost"] = cost
    groups, at = [], 0
    for b in np.unique(bsize_of_src).tolist():
        nb = int((bsize_of_src == b).sum())
        tx, tx_uv, cw, ch = tabs[b]
        g = dict(src_first=at, nblocks=nb, bsize=b, tx_type_uv=mr.uv_type(b, 0, tabs), pred=[], dq=[])
        for p in range(3):
            w, h, t = (mr.BS_W[b], mr.BS_H[b], tx) if p == 0 else (cw, ch, tx_uv)
            pred, dq = np.zeros((nb, h, w), np.uint8), np.zeros((nb, min(w, 32) * min(h, 32)), np.int32)
            for i in range(nb):
                ty = int(rng.choice(mr.types_of(t))) if p == 0 else g["tx_type_uv"]
                if p == 0:
                    dec["tx_type"][at + i] = ty
                _, dq[i], dec["eob"][at + i, p] = mr.coefficients(rng, t, ty, zero=rng.random() < 0.15, big=False)
                pred[i] = rng.integers(0, 256, (h, w))
            g["pred"].append(pred); g["dq"].append(dq)
        groups.append(g)
        at += nb
    return dict(pc, leaf=leaf, cost=cost), dec, groups, count, final


@pytest.mark.parametrize("name", ["all_blocks", "irregular"])
def test_chain_from_the_partition_decision(dsp, gold, name):
    """svt_hip_partition_decide_frame's d_final / d_final_count handed to the call without leaving the device, against the composed path:
    the list taken to the host, grouped by (size, type, plane), svt_hip_inv_txfm2d_add_batch with d_dst_offsets on planes that hold the
    scattered predictions"""
    z, geom, tabs = gold
    pz = dict(np.load(PART_GOLD))
    pc, dec, groups, count, final = chain_inputs(pz, tabs, geom, np.random.default_rng(4242), name)
    nsb, fill = len(pc["sb"]), fill_byte()
    W, H = int(pc["pic_width"]), int(pc["pic_height"])
    pa = dict(sb=dev(pc["sb"].view(np.uint8).reshape(nsb, 12)), leaf=dev(pc["leaf"].view(np.uint8).reshape(-1, 12)), partition_bits=dev(pc["bits"]),
              pic_width=W, pic_height=H, slice_is_intra=int(pc["slice_is_intra"]), decision=dev(dec.view(np.uint8).reshape(-1, 72)),
              sq=poison.tensor((nsb, mg.NSQ, 16), torch.uint8, DEV), final_count=poison.tensor((nsb,), torch.int32, DEV),
              final=poison.tensor((nsb, mg.MAX_FINAL, 12), torch.uint8, DEV))
    pa["lambda"] = int(pc["lam"])
    assert dsp.partition_decide_frame(pa) == 0, dsp.lib.svt_hip_last_error()
    dgroups = [dict(src_first=g["src_first"], nblocks=g["nblocks"], bsize=g["bsize"], tx_type_uv=g["tx_type_uv"],
                    best_pred=[dev(x) for x in g["pred"]], best_dqcoeff=[dev(x) for x in g["dq"]]) for g in groups]
    a = dict(final=pa["final"], final_count=pa["final_count"], decision=pa["decision"], groups=dgroups, planes=3,
             recon=[poison.tensor((H >> (p > 0), (W >> (p > 0)) + 24), torch.uint8, DEV) for p in range(3)], width=[W, W // 2, W // 2], height=[H, H // 2, H // 2],
             status=poison.tensor((nsb, mg.MAX_FINAL), torch.uint8, DEV),
             scratch=torch.empty((dsp.recon_final_scratch_bytes(nsb),), dtype=torch.uint8, device=DEV))
    run(dsp, a)                                                             # (no synchronisation between the two calls)
    # the composed path, from the list as the partition call wrote it
    got_count = pa["final_count"].cpu().numpy().view(np.uint32)
    got_final = pa["final"].cpu().numpy()
    assert np.array_equal(got_count, count)
    planes = [np.full(tuple(t.shape), fill, np.uint8) for t in a["recon"]]
    batches = {}                                                            # (plane, tx_size, tx_type) -> ([dq rows], [offsets])
    want_status = np.zeros((nsb, mg.MAX_FINAL), np.uint8)
    for sb in range(nsb):
        for k, e in enumerate(got_final[sb, :got_count[sb]].copy().view(mg.FINAL_DTYPE).reshape(-1)):
            src, b, x, y = int(e["src"]), int(e["bsize"]), int(e["x"]), int(e["y"])
            if src == mg.NO_SRC:                                            # a block no leaf listed: nothing to reconstruct it from
                want_status[sb, k] = 1
                continue
            g = [G for G in groups if G["src_first"] <= src < G["src_first"] + G["nblocks"]][0]
            tx, tx_uv, cw, ch = tabs[b]
            for p in range(3):
                if p and not geom["has_uv"][e["mds_idx"]]:
                    continue
                w, h, t, ty, x0, y0 = (mr.BS_W[b], mr.BS_H[b], tx, int(dec["tx_type"][src]), x, y) if p == 0 else (cw, ch, tx_uv, g["tx_type_uv"], ((x >> 3) << 3) >> 1, ((y >> 3) << 3) >> 1)
                planes[p][y0:y0 + h, x0:x0 + w] = g["pred"][p][src - g["src_first"]]
                if dec["eob"][src, p]:
                    rows, offs = batches.setdefault((p, t, ty), ([], []))
                    rows.append(g["dq"][p][src - g["src_first"]]); offs.append(y0 * planes[p].shape[1] + x0)
    assert len(batches) >= 10, sorted(batches)                              # launches of the composed path
    composed = [dev(pl) for pl in planes]
    for (p, t, ty), (rows, offs) in batches.items():
        dsp.inv_txfm2d_add(dev(np.stack(rows)), composed[p], t, ty, 8, dst_stride=planes[p].shape[1], offsets=dev(np.array(offs, np.uint32)))
    torch.cuda.synchronize()
    live = np.arange(mg.MAX_FINAL)[None] < count[:, None]
    assert np.array_equal(a["status"].cpu().numpy()[live], want_status[live]) and (want_status[live] == 0).sum() >= 19
    for p in range(3):
        assert torch.equal(a["recon"][p], composed[p]), p
        assert int((a["recon"][p] != fill).sum()) > 1000


def test_graph_capture_and_replay(dsp, gold):
    z, geom, tabs = gold
    c, o = mr.load_case(z, mr.ALL_NAMES.index("main2"), tabs)
    a = args_of(dsp, c, tabs)
    args = dsp.make_recon_final_args(a)
    run(dsp, args)                                                          # warm: nothing is created inside the capture
    check(a, c, o)
    graph = torch.cuda.CUDAGraph()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        with torch.cuda.graph(graph, stream=side):
            assert dsp.recon_final_frame(args) == 0, dsp.lib.svt_hip_last_error()
    torch.cuda.current_stream().wait_stream(side)
    for _ in range(2):
        for t in outputs_of(a):
            t.view(torch.uint8).fill_(fill_byte())
        graph.replay()
        torch.cuda.synchronize()
        check(a, c, o)


def test_invalid_arguments_are_refused_before_anything_is_enqueued(dsp, gold):
    z, geom, tabs = gold
    c, o = mr.load_case(z, mr.ALL_NAMES.index("main1"), tabs)
    good = args_of(dsp, c, tabs)
    nsb, nsrc = len(c["count"]), len(c["decision"])
    flat = lambda t: t.view(torch.uint8).reshape(-1)
    G = good["groups"]
    first = next(i for i, g in enumerate(G) if g["nblocks"])                # a non-empty group

    def with_group(i, **change):
        return dict(groups=[dict(g, **change) if j == i else g for j, g in enumerate(G)])

    def plane_list(key, p, value):
        return {key: [value if j == p else t for j, t in enumerate(good[key])]}

    uv32 = next(i for i, g in enumerate(G) if max(mr.TX_W[tabs[g["bsize"]][1]], mr.TX_H[tabs[g["bsize"]][1]]) == 32)
    cases = [("nsb 0", dict(nsb=0)), ("nsb above 2^20", dict(nsb=(1 << 20) + 1)), ("nsrc 0", dict(nsrc=0)), ("planes 2", dict(planes=2)), ("planes 0", dict(planes=0)),
             ("no groups", dict(groups=None, ngroups=len(G))), ("ngroups 0", dict(ngroups=0)), ("ngroups 33", dict(ngroups=33)),
             ("nsrc beyond the groups", dict(nsrc=nsrc + 1)), ("nsrc short of the groups", dict(nsrc=nsrc - 1)),
             ("a gap in the table", with_group(first + 1, src_first=G[first + 1]["src_first"] + 1)), ("not ascending", dict(groups=G[::-1])),
             ("bsize 22", with_group(first, bsize=22)), ("bsize 13", with_group(first, bsize=13)), ("bsize -1", with_group(first, bsize=-1)),
             ("tx_type_uv 16", with_group(first, tx_type_uv=16)), ("tx_type_uv 1 on a 32-sample chroma side", with_group(uv32, tx_type_uv=1)),
             ("scratch NULL", dict(scratch=None)), ("scratch small", dict(scratch=good["scratch"][:-16])), ("scratch misaligned", dict(scratch=good["scratch"][8:], scratch_bytes=good["scratch"].numel())),
             ("stride below width", dict(stride=[int(c["width"][0]) - 1, int(c["stride"][1]), int(c["stride"][2])])), ("width 65536", dict(width=[65536, 64, 64], stride=[65536, 72, 72])),
             ("one stream plane missing", plane_list("sb_qcoeff", 1, None))]
    cases += [(key + " NULL", {key: None}) for key in ("final", "final_count", "decision")]
    cases += [(f"recon {p} NULL", plane_list("recon", p, None)) for p in range(3)]
    cases += [("decision misaligned", dict(decision=flat(good["decision"])[4:], nsrc=nsrc))]
    cases += [(key + " misaligned", {key: flat(good[key])[2:]}) for key in ("final", "final_count", "coeff_offset")]
    cases += [(f"sb_qcoeff {p} misaligned", plane_list("sb_qcoeff", p, flat(good["sb_qcoeff"][p])[8:])) for p in range(3)]
    for key in ("best_pred", "best_dqcoeff", "best_qcoeff"):
        for p in range(3):
            cases.append((f"{key} {p} NULL", with_group(first, **{key: [None if j == p else t for j, t in enumerate(G[first][key])]})))
            cases.append((f"{key} {p} misaligned", with_group(first, **{key: [flat(t)[8:] if j == p else t for j, t in enumerate(G[first][key])]})))
    for name, change in cases:
        bad = dict(good, **change)
        bad.setdefault("nsb", nsb)
        bad.setdefault("nsrc", nsrc)
        assert dsp.recon_final_frame(bad) == INVALID, name
        torch.cuda.synchronize()
        assert untouched(good), name
    assert dsp.lib.svt_hip_recon_final_frame(None, None) == INVALID
    assert dsp.recon_final_scratch_bytes(0) == 0 and dsp.recon_final_scratch_bytes((1 << 20) + 1) == 0
    run(dsp, good)
    check(good, c, o)


poison.add_second_fill(globals())

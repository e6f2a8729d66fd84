"""GPU: svt_hip_inter_fast_pick_frame (the fast cost of the inter candidates, the N best of the combined inter + intra list, their order
and the survivors' records) and svt_hip_inter_fast_search_frame (distortion-only prediction -> pick -> prediction of the survivors ->
intra survivors copied in) through the C ABI against tests/golden/inter_fast.npz (make_golden_inter_fast.py: the reference's lines in
Python integers, its leaves pinned to the compiled reference; tests/test_inter_fast_cpu.py holds the second restatement).  Every output
is allocated poisoned and fenced (tests/poison.py); every comparison is an equality."""
import ctypes
import os
import sys
import zlib

import numpy as np
import pytest
import torch

import layouts
import poison
from poison import poisoned_outputs  # noqa: F401

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
import make_golden_inter_fast as mg  # noqa: E402
import make_golden_inter_pred as ip  # noqa: E402

pytestmark = pytest.mark.gpu
INVALID = -2
W, H = ip.W, ip.H
SAD, SSD = mg.SAD, mg.SSD
OUT_DTYPES = dict(cand=torch.uint8, sorted=torch.uint8, cost=torch.int64, rate=torch.int32, ref_fast_cost=torch.int64, all_cost=torch.int64,
                  blk_out=torch.uint8, cand_out=torch.uint8, src_xy_out=torch.int32)
REQUIRED = ("cand", "sorted", "cost", "rate", "ref_fast_cost", "blk_out")
_gold = None
_dev = {}


def gold():
    global _gold
    if _gold is None:
        _gold = dict(np.load(mg.OUT))
    return _gold


def up(dsp, a):
    a = np.ascontiguousarray(a)
    if a.dtype in (np.uint64, np.uint32, np.uint16):                          # torch has the signed types
        a = a.view({np.dtype(np.uint64): np.int64, np.dtype(np.uint32): np.int32, np.dtype(np.uint16): np.int16}[a.dtype])
    return torch.from_numpy(a).to(dsp.device)


def mv_cost(dsp):
    if "mv_cost" not in _dev:
        t = mg.make_mv_cost()
        assert zlib.crc32(t.tobytes()) == int(gold()["mv_cost_crc"][0])
        _dev["mv_cost"] = up(dsp, t)
    return _dev["mv_cost"]


def planes(dsp, bd):
    """the padded planes of the picture on the device, uploaded once and never written; views at picture sample (0, 0)"""
    if ("planes", bd) not in _dev:
        p = ip.planes_of(bd, "random")
        assert ip.planes_crc(p) == int(gold()["planes_crc"][0 if bd == 8 else 1])
        full = {n: [up(dsp, a) for a in p[n]] for n in p}
        _dev[("planes", bd)] = ({n: [t[ip.PAD[min(k, 1)]:, ip.PAD[min(k, 1)]:] for k, t in enumerate(full[n])] for n in full},
                                [t.shape[1] for t in full["src"]], full)
    return _dev[("planes", bd)][:2]


def case(kind, i):
    z = gold()
    keys, rows = (mg.PICK_KEYS, z["pick_params"]) if kind == "pick" else (mg.SEARCH_KEYS, z["search_params"])
    P = mg.params_of(keys, rows[i])
    A = {k[len(f"{kind}_{i}_"):]: z[k] for k in z if k.startswith(f"{kind}_{i}_")}
    if "rates" not in A:
        A["rates"] = z["rate_sets"][P["rate_set"]]
    return P, A


def pick_group(dsp, kind, i, nb=None, optional=True, with_dist=True, tile=1):
    """(group dict with poisoned outputs, expected dict) of a fixture group's first nb blocks, `tile` times over"""
    P, A = case(kind, i)
    nb = nb or len(A["ctx"])
    ni, na = P["ninter"], P["nintra"]
    n = min(P["nfl"], ni + na)
    cut = lambda a: np.concatenate([a[:nb]] * tile) if tile > 1 else a[:nb]
    g = dict(bsize=P["bsize"], bsize_uv=P["bsize_uv"], nblocks=nb * tile, ninter=ni, nintra=na, nfl=P["nfl"], ac_dequant_q3=P["ac_dequant_q3"],
             reference_mode_select=P["reference_mode_select"], switchable_motion_mode=P["switchable_motion_mode"], metric=P["metric"],
             blk=up(dsp, cut(A["blk"])), cand_in=up(dsp, cut(A["cand_in"])), ctx=up(dsp, cut(A["ctx"])), rates=up(dsp, A["rates"]), mv_cost=mv_cost(dsp))
    g["lambda"] = P["lambda"]
    if with_dist:
        for k in ("dist", "dist_cb", "dist_cr"):
            if k in A:
                g[k] = up(dsp, cut(A[k]))
    for k in ("intra_cost", "intra_rate"):
        if k in A:
            g[k] = up(dsp, cut(A[k]))
    N = nb * tile
    shapes = dict(cand=(N, n), sorted=(N, n), cost=(N, n), rate=(N, n, 2), ref_fast_cost=(N,), blk_out=(N, n, 16))
    if optional:
        shapes.update(all_cost=(N, ni), cand_out=(N, n, 16), src_xy_out=(N, n))
    want = {}
    for k, shp in shapes.items():
        g[k] = poison.tensor(shp, OUT_DTYPES[k], dsp.device)
        want[k] = cut(A["out_" + k])
    return g, want


def check(groups, wants, what=""):
    for gi, (g, w) in enumerate(zip(groups, wants)):
        for k, v in w.items():
            got = g[k].cpu().numpy()
            got = got.view(v.dtype) if got.dtype != v.dtype else got
            bad = np.argwhere(got != v)
            assert bad.size == 0, (what, gi, k, bad[:6].tolist(), got[tuple(bad[0])], v[tuple(bad[0])])


def ok(dsp, rc):
    assert rc == 0, dsp.lib.svt_hip_last_error().decode()
    torch.cuda.synchronize()


def untouched(*ts):
    return all(bool((t.view(torch.uint8) == poison.fill_value(torch.uint8)).all()) for t in ts if t is not None)


# ---- the pick ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("metric", [SAD, SSD])
def test_pick_every_fixture_group_of_the_metric_in_one_call(dsp, metric):
    """all twelve list shapes, (1, 0, 1) to (64, 0, 40), (40, 24, 40) and (1, 63, 2), 37 blocks each (ten workgroups, the last with one
    wave), every output asked for, an empty group between them; the search groups' recorded distortions as further groups"""
    groups, wants = [], []
    for i in range(len(mg.PICK_GROUPS)):
        if mg.PICK_GROUPS[i][5] == metric:
            g, w = pick_group(dsp, "pick", i)
            groups.append(g); wants.append(w)
    for i in range(len(mg.SEARCH_GROUPS)):
        if mg.SEARCH_GROUPS[i][3] == metric:
            g, w = pick_group(dsp, "search", i)
            groups.append(g); wants.append(w)
    assert len(groups) >= 6
    empty = dict(groups[0], nblocks=0)
    ok(dsp, dsp.inter_fast_pick_frame(groups[:1] + [empty] + groups[1:], metric))
    check(groups, wants, metric)
    ok(dsp, dsp.inter_fast_pick_frame([], metric))


@pytest.mark.parametrize("nb", [1, 5, 37])
def test_pick_one_group_per_call(dsp, nb):
    """each fixture group alone with 1, 5 and 37 blocks (a lone wave, a second workgroup of one wave, a ragged tenth workgroup); with 5
    blocks only the required outputs"""
    for i in range(len(mg.PICK_GROUPS)):
        g, w = pick_group(dsp, "pick", i, nb=nb, optional=nb != 5)
        ok(dsp, dsp.inter_fast_pick_frame([g], g["metric"]))
        check([g], [w], (i, nb))


def test_pick_groups_large_enough_for_several_blocks_per_wave(dsp):
    """the plan (pick_bpw of csrc/md_plan.h, tests/c/md_plan_host.cpp) gives a wave 2 and 4 blocks once a group has that many times the
    device's wave slots (32 per CU): a mixed (5, 3, 3) and a (3, 9, 4) group of the fixture repeated to just above those counts, cost only"""
    slots = torch.cuda.get_device_properties(0).multi_processor_count * 32
    groups, wants = [], []
    for i, k in ((6, 2), (11, 4)):
        tile = (k * slots + 2 * k + 1 + 36) // 37
        assert (37 * tile) // slots == k
        g, w = pick_group(dsp, "pick", i, tile=tile)
        groups.append(g); wants.append(w)
    ok(dsp, dsp.inter_fast_pick_frame(groups, SAD))
    check(groups, wants)


# ---- the one-call search -------------------------------------------------------------------------------------------------------------------
def search_group(dsp, si, own_dist, intra_pred=True, chroma_pred=True, laid_out=None):
    """(group dict, expected pick outputs, expected distortions | None) of fixture search group si.  laid_out: (views, {"ref": strides,
    "src": strides}, placed) of layouts.place_ref_src in place of the shared planes"""
    P, A = case("search", si)
    g, want = pick_group(dsp, "search", si, with_dist=False)
    bd, nb, ni, na = P["bd"], P["nblocks"], P["ninter"], P["nintra"]
    n = min(P["nfl"], ni + na)
    if laid_out is None:
        Pl, strides = planes(dsp, bd)
        strides = {"ref": strides, "src": strides}
    else:
        Pl, strides = laid_out[:2]
    np_ = 3 if P["chroma"] else 1
    st = torch.uint8 if bd == 8 else torch.int16
    g.update(bwidth=P["bwidth"], bheight=P["bheight"], use_chroma=P["chroma"], bd=bd, ref0=Pl["ref0"][:np_], ref1=Pl["ref1"][:np_],
             ref_stride=strides["ref"][:np_], src=Pl["src"][:np_], src_stride=strides["src"][:np_])
    g["pred_out"] = [poison.tensor((nb, n, P["bheight"] >> (p > 0), P["bwidth"] >> (p > 0)), st, dsp.device) for p in range(np_ if chroma_pred else 1)]
    dists = None
    if own_dist:
        names = ("dist", "dist_cb", "dist_cr")[:np_]
        for k in names:
            g[k] = poison.tensor((nb, ni), torch.int64, dsp.device)
        dists = {k: A[k] for k in names}
    if intra_pred and na:
        rng = np.random.default_rng([0x1D, si])
        ipred = rng.integers(0, 1 << bd, (nb, na, P["bheight"], P["bwidth"])).astype(np.uint8 if bd == 8 else np.uint16)
        g["intra_pred"], g["intra_pred_np"] = up(dsp, ipred), ipred
    return g, want, dists


def want_predictions(dsp, g, want):
    """svt_hip_inter_pred_frame run on the fixture's survivor records, per plane; the intra survivors' luma rows from intra_pred"""
    out = []
    blk = up(dsp, want["blk_out"].reshape(-1, 16))
    for p, t in enumerate(g["pred_out"]):
        ref = poison.tensor((blk.shape[0],) + tuple(t.shape[2:]), t.dtype, dsp.device)
        d = dict(ref0=g["ref0"][p], ref1=g["ref1"][p], ref_stride=g["ref_stride"][p], ss=int(p > 0), bwidth=g["bwidth"], bheight=g["bheight"], blk=blk, pred=ref)
        ok(dsp, dsp.inter_pred_frame([d], W, H, bd=g["bd"], metric=g["metric"]))
        r = ref.cpu().numpy().reshape(tuple(t.shape))
        if p == 0 and "intra_pred_np" in g:
            for i, s in np.argwhere(want["cand"] >= g["ninter"]):
                r[i, s] = g["intra_pred_np"][i, want["cand"][i, s] - g["ninter"]].view(r.dtype)
        out.append(r)
    return out


def check_search(dsp, g, want, dists, what):
    check([g], [want], what)
    if dists:
        check([g], [dists], what)
    for p, r in enumerate(want_predictions(dsp, g, want)):
        got = g["pred_out"][p].cpu().numpy()
        assert np.array_equal(got, r), (what, "plane", p, np.argwhere(got != r)[:4].tolist())
    return int((want["cand"] >= g["ninter"]).sum())


@pytest.mark.parametrize("own_dist", [False, True], ids=["scratch", "own_dist"])
@pytest.mark.parametrize("si", range(len(mg.SEARCH_GROUPS)))
def test_search_each_fixture_group(dsp, si, own_dist):
    """8x8, 16x16, 32x8 and 64x64 at 8 bits and 16x16 at 10, SAD and SSD, with and without chroma, the distortions in the scratch or in
    the caller's arrays: the distortions, every pick output, the survivors' predictions of every plane, the intra slots"""
    g, want, dists = search_group(dsp, si, own_dist)
    need = dsp.inter_fast_search_scratch_bytes([g])
    per = g["nblocks"] * g["ninter"] * 8
    assert need == (0 if own_dist else (3 if g["use_chroma"] else 1) * ((per + 15) & ~15))
    scratch = poison.tensor((max(need, 16),), torch.uint8, dsp.device)
    rc, _ = dsp.inter_fast_search_frame([g], W, H, g["metric"], scratch=scratch if need else None, bd=g["bd"])
    ok(dsp, rc)
    check_search(dsp, g, want, dists, (si, own_dist))
    if own_dist:
        assert untouched(scratch)


def test_search_with_six_different_strides_equals_the_fixture(dsp):
    """the first 8-bit fixture group with chroma: ref_stride[3] and src_stride[3] all different and odd, chroma's unrelated to luma's, the
    nine planes at different places; the distortions of all three planes and every pick output against the fixture, the survivors'
    predictions against svt_hip_inter_pred_frame on the same planes"""
    si = next(i for i in range(len(mg.SEARCH_GROUPS)) if case("search", i)[0]["chroma"] and case("search", i)[0]["bd"] == 8)
    spec = layouts.ref_src_spec("svt_hip_inter_fast_search_frame", W, H, ip.PAD)
    lp = layouts.place_ref_src(spec, layouts.distinct_layouts(spec), ip.planes_of(8, "random"))
    g, want, dists = search_group(dsp, si, True, laid_out=lp)
    rc, _ = dsp.inter_fast_search_frame([g], W, H, g["metric"], scratch=None, bd=g["bd"])
    ok(dsp, rc)
    check_search(dsp, g, want, dists, si)
    layouts.assert_all_intact(lp[2], poison._active.fill_byte)


def test_search_all_8_bit_groups_in_one_call_without_intra_pred(dsp):
    """the SAD groups of the fixture as one call with an empty group, luma predictions only for one of them and no d_intra_pred: an intra
    slot then holds the benign record's prediction"""
    gs, ws = [], []
    nintra_slots = 0
    for si in range(len(mg.SEARCH_GROUPS)):
        if mg.SEARCH_GROUPS[si][2] == 8 and mg.SEARCH_GROUPS[si][3] == SAD:
            g, want, _ = search_group(dsp, si, False, intra_pred=False, chroma_pred=si != 0)
            gs.append(g); ws.append(want)
    assert len(gs) >= 2
    empty = dict(gs[0], nblocks=0)
    rc, scratch = dsp.inter_fast_search_frame([gs[0], empty] + gs[1:], W, H, SAD)
    ok(dsp, rc)
    for g, want in zip(gs, ws):
        nintra_slots += check_search(dsp, g, want, None, "one call")
    assert nintra_slots > 0 and len(gs[0]["pred_out"]) == 1


def test_search_captured_in_a_graph_and_replayed(dsp):
    """the call captured on a side stream (a single chain: every stage on the caller's stream) and replayed twice over refilled outputs"""
    gs, ws = [], []
    for si in (0, 1):
        g, want, dists = search_group(dsp, si, si == 1)
        gs.append(g); ws.append((want, dists))
    arr = dsp.make_inter_fast_search_groups(gs)
    need = dsp.lib.svt_hip_inter_fast_search_scratch_bytes(arr, len(gs))
    assert need > 0
    scratch = poison.tensor((need,), torch.uint8, dsp.device)
    # one metric per call: both groups as SAD; group 1's fixture is SSD, so only group 0 is compared with the fixture and group 1 with a direct call
    direct, _, _ = search_group(dsp, 1, True)
    rc, keep = dsp.inter_fast_search_frame([direct], W, H, SAD)
    ok(dsp, rc)
    st = torch.cuda.Stream()
    st.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(st):
        with torch.cuda.graph(graph, stream=st):
            assert dsp.lib.svt_hip_inter_fast_search_frame(arr, len(gs), W, H, 8, SAD, ctypes.c_void_p(scratch.data_ptr()), need,
                                                           ctypes.c_void_p(st.cuda_stream)) == 0
    torch.cuda.current_stream().wait_stream(st)
    outs = [k for k in OUT_DTYPES if k in gs[0]] + ["dist", "dist_cb", "dist_cr"]
    for fill in (0x55, 0xAA):
        scratch.fill_(fill)
        for g in gs:
            for k in outs:
                if g.get(k) is not None:
                    g[k].view(torch.uint8).fill_(fill)
            for t in g["pred_out"]:
                t.view(torch.uint8).fill_(fill)
        graph.replay()
        torch.cuda.synchronize()
        check_search(dsp, gs[0], ws[0][0], None, ("graph", fill))
        for k in outs:
            if gs[1].get(k) is not None:
                assert torch.equal(gs[1][k], direct[k]), (k, fill)
        for a, b in zip(gs[1]["pred_out"], direct["pred_out"]):
            assert torch.equal(a, b)
    poison.assert_written(direct["dist"], direct["cost"], direct["rate"], direct["ref_fast_cost"])


# ---- refusals ------------------------------------------------------------------------------------------------------------------------------
def test_every_refusal_returns_invalid_and_leaves_the_poisoned_outputs_untouched(dsp):
    def off(t, nbytes):
        return t.view(torch.uint8).reshape(-1)[nbytes:]

    def outputs_of(g):
        return [g.get(k) for k in OUT_DTYPES] + [g.get(k) for k in ("dist", "dist_cb", "dist_cr") if g.get("own")] + list(g.get("pred_out", []))

    g, _ = pick_group(dsp, "pick", 6)                                          # (5, 3, 3), SAD
    edits = [dict(metric=2), dict(metric=-1), dict(bsize=22), dict(bsize=-1), dict(bsize_uv=22), dict(ninter=0), dict(ninter=62), dict(nintra=-1),
             dict(nintra=60), dict(nfl=0), dict(nfl=41), dict(ac_dequant_q3=-1), dict(nblocks=(1 << 31) // 8), dict(intra_cost=None)]
    edits += [{k: None} for k in ("blk", "cand_in", "ctx", "rates", "mv_cost", "dist") + REQUIRED]
    edits += [{k: off(g[k], 4)} for k in ("dist", "dist_cb", "dist_cr", "intra_cost", "cost", "ref_fast_cost", "all_cost")]
    edits += [{k: off(g[k], 2)} for k in ("blk", "blk_out", "cand_in", "cand_out", "ctx", "rates", "mv_cost", "rate", "intra_rate", "src_xy_out")]
    good, _ = pick_group(dsp, "pick", 2)
    for e in edits:
        bad = dict(g, **e)
        for lst in ([bad], [good, bad]):                                       # nothing of the call is launched, an accepted group in front included
            assert dsp.inter_fast_pick_frame(lst, bad["metric"]) == INVALID, e
        torch.cuda.synchronize()
        assert untouched(*outputs_of(g), *outputs_of(good)), e
    assert dsp.lib.svt_hip_inter_fast_pick_frame(None, 1, SAD, None) == INVALID
    # the accepted neighbours
    for e in (dict(nfl=1), dict(nfl=2), dict(ac_dequant_q3=0)):          # (nfl 40 and the count bounds: the fixture groups themselves)
        gg, _ = pick_group(dsp, "pick", 6)
        ok(dsp, dsp.inter_fast_pick_frame([dict(gg, **e)], SAD))
    # the search
    s, _, _ = search_group(dsp, 0, True)                                       # 8x8, chroma, intra candidates, its own distortions
    s["own"] = True
    s2, _, _ = search_group(dsp, 0, False)
    need = dsp.inter_fast_search_scratch_bytes([s2])
    scratch = poison.tensor((need + 16,), torch.uint8, dsp.device)
    sedits = [dict(bd=9), dict(bd=12), dict(metric=2), dict(bwidth=12), dict(bheight=16), dict(bsize=6), dict(ninter=0), dict(nfl=41),
              dict(pred_out=[]), dict(src=s["src"][:1]), dict(ref0=s["ref0"][:2]), dict(intra_pred=off(s["intra_pred"], 8)),
              dict(pred_out=[off(s["pred_out"][0], 8)] + s["pred_out"][1:]), dict(intra_cost=None), dict(blk=None), dict(blk_out=None),
              dict(rates=off(s["rates"], 2)), dict(dist=off(s["dist"], 4))]
    for e in sedits:
        bad = dict(s, **e)
        rc, _ = dsp.inter_fast_search_frame([bad], W, H, bad["metric"], scratch=scratch, bd=bad["bd"])
        assert rc == INVALID, e
        torch.cuda.synchronize()
        assert untouched(*outputs_of(s), scratch), e
    for pw, ph in ((0, H), (W + 4, H), (W, 0), (4, H)):
        rc, _ = dsp.inter_fast_search_frame([s], pw, ph, SAD, scratch=scratch)
        assert rc == INVALID
    # the scratch: NULL, too small, misaligned; then accepted at exactly its size
    arr = dsp.make_inter_fast_search_groups([s2])
    call = lambda ptr, nbytes: dsp.lib.svt_hip_inter_fast_search_frame(arr, 1, W, H, 8, SAD, ptr, nbytes, dsp._stream())
    assert call(None, need) == INVALID and call(ctypes.c_void_p(scratch.data_ptr()), need - 1) == INVALID
    assert call(ctypes.c_void_p(scratch.data_ptr() + 8), need) == INVALID
    torch.cuda.synchronize()
    assert untouched(*outputs_of(s2), scratch)
    assert call(ctypes.c_void_p(scratch.data_ptr()), need) == 0
    torch.cuda.synchronize()
    assert untouched(scratch[need:])
    # chroma follows svt_hip_inter_pred_frame's own rule: no chroma group of a 4-wide block
    g4, _ = pick_group(dsp, "pick", 11, nb=2, with_dist=False)                  # 4x8
    Pl, strides = planes(dsp, 8)
    g4.update(bwidth=4, bheight=8, bd=8, ref0=Pl["ref0"], ref1=Pl["ref1"], ref_stride=strides, src=Pl["src"], src_stride=strides,
              pred_out=[poison.tensor((2, 4, 8, 4), torch.uint8, dsp.device)], use_chroma=1)
    rc, _ = dsp.inter_fast_search_frame([g4], W, H, SAD)
    assert rc == INVALID
    torch.cuda.synchronize()
    assert untouched(*outputs_of(g4))


poison.add_second_fill(globals())

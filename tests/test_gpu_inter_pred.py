"""GPU: svt_hip_inter_pred_frame against tests/golden/inter_pred.npz (the sixteen compiled convolve entries of the reference behind the
generator's glue, see tests/golden/make_golden_inter_pred.py).  Every output is allocated poisoned and fenced (tests/poison.py); every
comparison is an equality."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

import layouts
import poison
from poison import poisoned_outputs  # noqa: F401

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
import make_golden_inter_pred as mg  # noqa: E402

pytestmark = pytest.mark.gpu
INVALID = -2
W, H = mg.W, mg.H
_gold = None


def gold():
    global _gold
    if _gold is None:
        _gold = np.load(os.path.join(ROOT, "tests", "golden", "inter_pred.npz"))
    return _gold


def tdtype(bd):
    return torch.uint8 if bd == 8 else torch.int16


def to_dev(a, dev):
    """numpy uint8 / uint16 -> device tensor (uint16 travels as int16 bits)"""
    return torch.from_numpy(a.view(np.int16) if a.dtype == np.uint16 else a).to(dev)


def to_np(t, bd):
    a = t.cpu().numpy()
    return a if bd == 8 else a.view(np.uint16)


_dev_planes = {}


def device_planes(dsp, bd, content):
    """{name: [padded plane tensors]} of mg.make_planes, uploaded once per (bd, content) and never written"""
    key = (bd, content)
    if key not in _dev_planes:
        p = mg.planes_of(bd, content)
        _dev_planes[key] = {n: [to_dev(a, dsp.device) for a in p[n]] for n in p}
    return _dev_planes[key]


def origin(plane_t, k):
    """the view whose first element is sample (0, 0) of the picture"""
    pad = mg.PAD[0] if k == 0 else mg.PAD[1]
    return plane_t[pad:, pad:]


def inter_pred_spec(plane):
    """ref (one stride for both references), src and pred of a group of luma (plane 0) or chroma blocks: pointers to sample (0, 0) of
    planes with the fixture's border on every side"""
    w, h, pad = (W, H, mg.PAD[0]) if plane == 0 else (W // 2, H // 2, mg.PAD[1])
    return layouts.CallSpec("svt_hip_inter_pred_frame", [layouts.Plane(n, w, h, (pad, pad), (pad, pad), stacked=False) for n in ("ref", "src", "pred")])


def laid_out_planes(bd, content, plane, spec, lay):
    """({name: {plane: strided view of the padded plane}}, placed) with ref0 / ref1 at the layout of "ref" and src at its own"""
    p = mg.planes_of(bd, content)
    P, placed = {}, []
    for name in ("ref0", "ref1", "src"):
        pl = spec.plane("src" if name == "src" else "ref")
        buf, view = layouts.place_plane(pl, p[name][plane], lay[pl.name])
        P[name] = {plane: view}
        placed.append((name, buf, view, p[name][plane]))
    return P, placed


def group_dict(dsp, gi, want_pred="dense", with_dist=False, dense_out=None, laid_out=None):
    """the fixture's group gi as an inter_pred_frame group with poisoned outputs.  laid_out = (spec, layouts) of tests/layouts.py: the
    reference, source and prediction planes each at a layout of their own (the group's "placed" lists them for the guard checks)"""
    g = gold()
    bd, content, ss, bw, bh, same, plane = (int(v) for v in g["groups"][gi])
    placed = []
    if laid_out is None:
        P = device_planes(dsp, bd, mg.CONTENTS[content])
    else:
        P, placed = laid_out_planes(bd, mg.CONTENTS[content], plane, *laid_out)
    blk = g[f"blk_{gi}"]
    n, w, h = len(blk), bw >> ss, bh >> ss
    d = dict(ref0=origin(P["ref0"][plane], plane), ref1=origin(P["ref0" if same else "ref1"][plane], plane), ref_stride=P["ref0"][plane].stride(0),
             ss=ss, bwidth=bw, bheight=bh, nblocks=n, blk=torch.from_numpy(blk.copy()).to(dsp.device), placed=placed)
    if want_pred == "dense":
        d["pred"] = dense_out if dense_out is not None else poison.tensor((n, h, w), tdtype(bd), dsp.device)
    elif want_pred == "plane":
        if laid_out is None:
            full = poison.tensor(tuple(P["src"][plane].shape), tdtype(bd), dsp.device)
        else:
            spec, lay = laid_out
            blank = layouts.poison_like(mg.planes_of(bd, mg.CONTENTS[content])["src"][plane], poison._active.fill_byte)
            buf, full = layouts.place_plane(spec.plane("pred"), blank, lay["pred"])
            d["placed_pred"] = [("pred", buf, full, blank)]
        d["pred_full"] = full
        d["pred"], d["pred_stride"] = origin(full, plane), full.stride(0)
    if with_dist:
        d["src"], d["src_stride"] = origin(P["src"][plane], plane), P["src"][plane].stride(0)
        d["dist"] = poison.tensor((n,), torch.int64, dsp.device)
    return d, bd


def groups_of_bd(bd):
    return [gi for gi, r in enumerate(gold()["groups"]) if int(r[0]) == bd]


def run(dsp, groups, bd, metric=mg.SAD):
    rc = dsp.inter_pred_frame(groups, W, H, bd, metric)
    assert rc == 0, dsp.lib.svt_hip_last_error().decode()
    torch.cuda.synchronize()


@pytest.mark.parametrize("bd", (8, 10))
def test_every_fixture_case_into_a_dense_prediction_equals_the_fixture(dsp, bd):
    """one call per group, so that a failure names the shape"""
    g = gold()
    for gi in groups_of_bd(bd):
        d, _ = group_dict(dsp, gi)
        run(dsp, [d], bd)
        got, want = to_np(d["pred"], bd), g[f"pred_{gi}"]
        bad = np.argwhere((got != want).reshape(len(want), -1).any(axis=1)).ravel()
        assert bad.size == 0, (gi, [int(v) for v in g["groups"][gi]], "blocks", bad[:8].tolist(), mg.blocks_of(g, gi)[bad[:2]])


@pytest.mark.parametrize("bd", (8, 10))
def test_every_fixture_case_into_a_plane_equals_the_fixture_and_leaves_the_rest_of_the_plane_untouched(dsp, bd):
    g = gold()
    fill = poison.fill_value(tdtype(bd)) & ((1 << 16) - 1 if bd > 8 else 255)
    for gi in groups_of_bd(bd):
        _, content, ss, bw, bh, same, plane = (int(v) for v in g["groups"][gi])
        pad = mg.PAD[1] if ss else mg.PAD[0]
        w, h = bw >> ss, bh >> ss
        blk = mg.blocks_of(g, gi)
        # blocks of a group overlap in the plane: one call per set of blocks that do not (greedy), the expected plane painted alike
        left = list(range(len(blk)))
        while left:
            take, used = [], np.zeros((H + 2 * mg.PAD[0], W + 2 * mg.PAD[0]), bool)
            for i in list(left):
                px, py, _ = mg.block_glue(blk[i], ss, bw, bh)
                if not used[py:py + h, px:px + w].any():
                    used[py:py + h, px:px + w] = True
                    take.append(i)
                    left.remove(i)
            d, _ = group_dict(dsp, gi, want_pred="plane")
            d["blk"], d["nblocks"] = d["blk"][take].contiguous(), len(take)
            run(dsp, [d], bd)
            got = to_np(d["pred_full"], bd)
            want = np.full(got.shape, fill, got.dtype)
            for i in take:
                px, py, _ = mg.block_glue(blk[i], ss, bw, bh)
                want[pad + py:pad + py + h, pad + px:pad + px + w] = g[f"pred_{gi}"][i]
            assert np.array_equal(got, want), (gi, take[:4])


@pytest.mark.parametrize("bd", (8, 10))
def test_ref_src_and_pred_planes_laid_out_unlike_each_other_equal_the_fixture(dsp, bd):
    """the 8x8 luma group and the 4x4 Cb group of 8x8 blocks (both lists alone and BI_PRED in each), prediction into a plane and the fused SAD against the source: ref_stride, src_stride
    and pred_stride all odd and all different, the three planes at different places in allocations of different sizes.  The blocks of a
    group overlap in the plane, so the call takes a set that does not, the BI_PRED blocks first."""
    g = gold()
    fill = poison.fill_value(tdtype(bd)) & ((1 << 16) - 1 if bd > 8 else 255)
    for want_group in ((bd, 0, 0, 8, 8, 0, 0), (bd, 0, 1, 8, 8, 0, 1)):
        gi = next(i for i, r in enumerate(g["groups"]) if tuple(int(v) for v in r) == want_group)
        _, content, ss, bw, bh, same, plane = want_group
        pad, w, h = (mg.PAD[1] if ss else mg.PAD[0]), bw >> ss, bh >> ss
        blk = mg.blocks_of(g, gi)
        take, used = [], np.zeros((H + 2 * mg.PAD[0], W + 2 * mg.PAD[0]), bool)
        for i in sorted(range(len(blk)), key=lambda i: int(blk[i]["pred_direction"]) != mg.BI):
            px, py, _ = mg.block_glue(blk[i], ss, bw, bh)
            if not used[py:py + h, px:px + w].any():
                used[py:py + h, px:px + w] = True
                take.append(i)
        assert {int(blk[i]["pred_direction"]) for i in take} == {mg.LIST0, mg.LIST1, mg.BI}
        spec = inter_pred_spec(plane)
        d, _ = group_dict(dsp, gi, want_pred="plane", with_dist=True, laid_out=(spec, layouts.distinct_layouts(spec)))
        assert len({d["ref_stride"], d["src_stride"], d["pred_stride"]}) == 3
        d["blk"], d["nblocks"] = d["blk"][take].contiguous(), len(take)
        d["dist"] = poison.tensor((len(take),), torch.int64, dsp.device)
        run(dsp, [d], bd)
        got = to_np(d["pred_full"], bd)
        want = np.full(got.shape, fill, got.dtype)
        for i in take:
            px, py, _ = mg.block_glue(blk[i], ss, bw, bh)
            want[pad + py:pad + py + h, pad + px:pad + px + w] = g[f"pred_{gi}"][i]
        assert np.array_equal(got, want), (gi, np.argwhere(got != want)[:4].tolist())
        src = mg.planes_of(bd, mg.CONTENTS[content])["src"][plane]
        assert np.array_equal(d["dist"].cpu().numpy(), mg.np_dist(g[f"pred_{gi}"], src, ss, blk, mg.SAD)[take]), gi
        layouts.assert_all_intact(d["placed"], poison._active.fill_byte)
        layouts.assert_all_intact(d["placed_pred"], poison._active.fill_byte, written=True)


@pytest.mark.parametrize("metric", (mg.SAD, mg.SSD))
@pytest.mark.parametrize("bd", (8, 10))
def test_the_fused_distortion_equals_numpy_on_the_fixture_prediction_with_and_without_a_stored_prediction(dsp, bd, metric):
    g = gold()
    for gi in groups_of_bd(bd):
        _, content, ss, bw, bh, same, plane = (int(v) for v in g["groups"][gi])
        src = mg.planes_of(bd, mg.CONTENTS[content])["src"][plane]
        want = mg.np_dist(g[f"pred_{gi}"], src, ss, mg.blocks_of(g, gi), metric)
        for want_pred in ("dense", None):
            d, _ = group_dict(dsp, gi, want_pred=want_pred, with_dist=True)
            run(dsp, [d], bd, metric)
            assert np.array_equal(d["dist"].cpu().numpy(), want), (gi, want_pred)
            if want_pred:
                assert np.array_equal(to_np(d["pred"], bd), g[f"pred_{gi}"]), gi


def test_a_full_pel_vector_is_a_shifted_slice_of_the_plane_and_its_sad_is_the_sad_call_s(dsp):
    rng = np.random.default_rng(77)
    P = device_planes(dsp, 8, "random")
    ref = mg.planes_of(8, "random")["ref0"][0]
    src = mg.planes_of(8, "random")["src"][0]
    pad = mg.PAD[0]
    for bw, bh in ((4, 4), (8, 8), (16, 8), (32, 32), (64, 64), (64, 16)):
        n = 37
        blk = np.zeros(n, mg.BLK_DTYPE)
        blk["x"] = rng.integers(0, (W - bw) // 4 + 1, n) * 4
        blk["y"] = rng.integers(0, (H - bh) // 4 + 1, n) * 4
        blk["mv"][:, 0, :] = rng.integers(-3, 4, (n, 2)) * 8
        blk["filter_x"], blk["filter_y"] = rng.integers(0, 4, n), rng.integers(0, 4, n)
        d = dict(ref0=origin(P["ref0"][0], 0), ref_stride=ref.shape[1], ss=0, bwidth=bw, bheight=bh, nblocks=n,
                 blk=torch.from_numpy(blk.view(np.uint8).reshape(n, 16).copy()).to(dsp.device), pred=poison.tensor((n, bh, bw), torch.uint8, dsp.device),
                 src=origin(P["src"][0], 0), src_stride=src.shape[1], dist=poison.tensor((n,), torch.int64, dsp.device))
        run(dsp, [d], 8, mg.SAD)
        want = np.stack([ref[pad + int(b["y"]) + int(b["mv"][0][1]) // 8:, pad + int(b["x"]) + int(b["mv"][0][0]) // 8:][:bh, :bw] for b in blk])
        assert np.array_equal(d["pred"].cpu().numpy(), want), (bw, bh)
        srcb = np.stack([src[pad + int(b["y"]):, pad + int(b["x"]):][:bh, :bw] for b in blk])
        sad = dsp.sad(torch.from_numpy(np.ascontiguousarray(srcb)).to(dsp.device), d["pred"])
        torch.cuda.synchronize()
        poison.assert_written(sad, d["dist"])
        assert np.array_equal(sad.cpu().numpy().astype(np.int64) & 0xffffffff, d["dist"].cpu().numpy()), (bw, bh)


@pytest.mark.parametrize("bd", (8, 10))
def test_one_call_with_luma_cb_and_cr_groups_of_several_sizes_equals_the_per_group_calls(dsp, bd):
    g = gold()
    gis = [gi for gi in groups_of_bd(bd) if int(g["groups"][gi][1]) == 0]
    gis = gis + gis[:10]                                                               # more groups than one launch holds
    assert {int(g["groups"][gi][6]) for gi in gis} == {0, 1, 2} and len(gis) > mg_max_groups(dsp)
    ds = [group_dict(dsp, gi, with_dist=True)[0] for gi in gis]
    empty = dict(ds[0], nblocks=0)                                                     # an empty group in the middle is skipped
    rc = dsp.inter_pred_frame(ds[:3] + [empty] + ds[3:], W, H, bd, mg.SSD)
    assert rc == 0, dsp.lib.svt_hip_last_error().decode()
    torch.cuda.synchronize()
    for gi, d in zip(gis, ds):
        one, _ = group_dict(dsp, gi, with_dist=True)
        run(dsp, [one], bd, mg.SSD)
        poison.assert_written(one["dist"], d["dist"])
        assert torch.equal(one["pred"], d["pred"]) and torch.equal(one["dist"], d["dist"]), gi
        assert np.array_equal(to_np(d["pred"], bd), g[f"pred_{gi}"]), gi


def mg_max_groups(dsp):
    import __graft_entry__ as ge
    return ge.load_package().INTER_PRED_MAX_GROUPS


def test_the_call_captured_in_a_graph_and_replayed_equals_the_direct_call(dsp):
    g = gold()
    gis = [gi for gi in groups_of_bd(8) if int(g["groups"][gi][1]) == 0][:12]
    ds = [group_dict(dsp, gi, with_dist=True)[0] for gi in gis]
    arr = dsp.make_inter_pred_groups(ds)
    assert dsp.inter_pred_frame(arr, W, H, 8, mg.SAD) == 0
    torch.cuda.synchronize()
    eager = [(d["pred"].clone(), d["dist"].clone()) for d in ds]
    for gi, (p, _) in zip(gis, eager):
        assert np.array_equal(p.cpu().numpy(), g[f"pred_{gi}"]), gi
    st = torch.cuda.Stream()
    st.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(st):
        with torch.cuda.graph(graph, stream=st):
            assert dsp.lib.svt_hip_inter_pred_frame(arr, len(ds), W, H, 8, mg.SAD, ctypes.c_void_p(st.cuda_stream)) == 0
    torch.cuda.current_stream().wait_stream(st)
    for fill in (0x55, 0xAA):
        for d in ds:
            d["pred"].view(torch.uint8).fill_(fill)
            d["dist"].view(torch.uint8).fill_(fill)
        graph.replay()
        torch.cuda.synchronize()
        for d, (p, e) in zip(ds, eager):
            assert torch.equal(d["pred"], p) and torch.equal(d["dist"], e), fill


def test_every_refusal_returns_invalid_and_leaves_the_poisoned_outputs_untouched(dsp):
    g = gold()
    gl = next(gi for gi in groups_of_bd(8) if tuple(int(v) for v in g["groups"][gi][1:5]) == (0, 0, 16, 16))
    gc = next(gi for gi in groups_of_bd(8) if tuple(int(v) for v in g["groups"][gi][1:5]) == (0, 1, 16, 16))

    def base(gi=gl):
        return group_dict(dsp, gi, with_dist=True)[0]

    def off(t, nbytes):
        return t.view(torch.uint8).reshape(-1)[nbytes:]

    cases = []                                                # (name, edit(d) -> None, call keywords)

    def case(name, edit=None, gi=gl, **kw):
        cases.append((name, edit, gi, kw))

    case("bd 12", bd=12)
    case("bd 9", bd=9)
    case("metric 2", metric=2)
    case("metric -1", metric=-1)
    case("ss 2", lambda d: d.update(ss=2))
    case("ss -1", lambda d: d.update(ss=-1))
    case("bwidth 12", lambda d: d.update(bwidth=12))
    case("bheight 128", lambda d: d.update(bheight=128))
    case("bwidth 0", lambda d: d.update(bwidth=0))
    case("chroma of a 4-wide block", lambda d: d.update(bwidth=4), gi=gc)
    case("chroma of a 4-high block", lambda d: d.update(bheight=4), gi=gc)
    case("picture width 0", w=0)
    case("picture height 0", h=0)
    case("picture width not a multiple of 8", w=100)
    case("picture height not a multiple of 8", h=76)
    case("block wider than the picture", lambda d: d.update(bwidth=64), w=32)
    case("d_blk NULL", lambda d: d.update(blk=None, nblocks=4))
    case("d_ref[0] NULL", lambda d: d.update(ref0=None))
    case("no output", lambda d: d.update(pred=None, src=None, dist=None))
    case("d_dist without d_src", lambda d: d.update(src=None))
    case("d_src without d_dist", lambda d: d.update(dist=None))
    case("d_dist misaligned", lambda d: d.update(dist=off(d["dist"], 4)))
    case("d_blk misaligned", lambda d: d.update(blk=off(d["blk"], 2), nblocks=d["nblocks"] - 1))
    case("dense d_pred misaligned", lambda d: d.update(pred=off(d["pred"], 8)))
    case("pred_stride below the block width", lambda d: d.update(pred_stride=15))
    case("chroma pred_stride below the plane block width", lambda d: d.update(pred_stride=7), gi=gc)
    case("nblocks beyond one launch", lambda d: d.update(bwidth=32, bheight=32, nblocks=0xffffffff))
    for name, edit, gi, kw in cases:
        good = base()
        d = base(gi)
        if edit:
            edit(d)
        # the bad group last: nothing of the good group before it may have been launched either
        rc = dsp.inter_pred_frame([good, d], kw.get("w", W), kw.get("h", H), kw.get("bd", 8), kw.get("metric", mg.SAD))
        torch.cuda.synchronize()
        assert rc == INVALID, (name, rc)
        assert dsp.lib.svt_hip_last_error(), name
        for t in (good["pred"], good["dist"], d.get("pred"), d.get("dist")):
            if t is not None:
                assert bool((t.view(torch.uint8) == poison.fill_value(torch.uint8)).all()), name
    assert dsp.lib.svt_hip_inter_pred_frame(None, 1, W, H, 8, 0, None) == INVALID
    assert dsp.lib.svt_hip_inter_pred_frame(None, 0, W, H, 8, 0, None) == 0            # no groups: a successful no-op
    ok = base()
    assert dsp.inter_pred_frame([ok], W, H, 8, mg.SAD) == 0                            # and the unedited group is accepted
    torch.cuda.synchronize()
    assert np.array_equal(ok["pred"].cpu().numpy(), g[f"pred_{gl}"])


def test_out_of_range_device_bytes_stay_inside_the_block_s_output(dsp):
    """pred_direction, filter_x, filter_y above their range and an origin outside the picture: an unspecified prediction, but the
    fences around the outputs hold (checked by the fixture when the test ends) and the neighbours' predictions are the fixture's"""
    g = gold()
    gi = next(gi for gi in groups_of_bd(8) if tuple(int(v) for v in g["groups"][gi][1:5]) == (0, 0, 8, 8))
    d, _ = group_dict(dsp, gi, with_dist=True)
    blk = mg.blocks_of(g, gi)
    for i, (f, v) in enumerate((("pred_direction", 3), ("pred_direction", 255), ("filter_x", 4), ("filter_y", 255), ("x", 65535), ("y", 30000))):
        blk[2 * i][f] = v
    d["blk"] = torch.from_numpy(blk.view(np.uint8).reshape(len(blk), 16).copy()).to(dsp.device)
    run(dsp, [d], 8)
    got = d["pred"].cpu().numpy()
    keep = np.ones(len(blk), bool)
    keep[0:12:2] = False
    assert np.array_equal(got[keep], g[f"pred_{gi}"][keep])


poison.add_second_fill(globals())

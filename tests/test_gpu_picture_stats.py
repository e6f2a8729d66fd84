"""GPU: svt_hip_picture_stats_frame - GatheringPictureStatistics for every SB and every histogram region of a picture in one call, two
launches - against the fixture (tests/golden/picture_stats.npz, written by tests/golden/make_golden_picture_stats.py from the
reference's own leaves, see there): every output of every case, both precisions; a stack of pictures whose pitches are above one
plane against single calls; the call captured into a graph; the arguments it must refuse; and on planes that svt_hip_picture_import
and svt_hip_picture_decimate wrote.  Every output is allocated poisoned (tests/poison.py): an entry the two launches never wrote - the
zeroed chroma rows of an incomplete SB, a bin no sample hits - fails the comparison.  Every comparison is an equality."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

import poison
import svtlibs
from poison import poisoned_outputs  # noqa: F401

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
import make_golden_picture_stats as mg  # noqa: E402

INVALID = -2
VIEW = {"variance": np.uint16, "pic_avg_variance": np.uint16, "histogram": np.uint32}
KEYS = ("y_mean", "variance", "cb_mean", "cr_mean", "pic_avg_variance", "histogram", "avg_intensity_region", "avg_intensity")
GOLD_KEY = {"avg_intensity_region": "avg_region", "avg_intensity": "avg"}

_gold = {}


def gold():
    if not _gold:
        _gold["g"] = np.load(os.path.join(ROOT, "tests", "golden", "picture_stats.npz"))
    return _gold["g"]


def device_planes(dsp, pictures, extra_rows=0):
    """the padded planes of one picture (2-D tensors) or of a stack (3-D, each picture followed by `extra_rows` rows that belong to no
    picture and hold 0xEE) -> (PicStatsPlanes, the tensors)"""
    per_pic = [mg.np_planes(*p) for p in pictures]
    tensors, origins = [], []
    for k in range(4):
        bufs = [pp[k][0] for pp in per_pic]
        origins.append((per_pic[0][k][1], per_pic[0][k][1]))
        if len(bufs) == 1 and not extra_rows:
            tensors.append(torch.from_numpy(bufs[0]).to(dsp.device))
        else:
            rows, stride = bufs[0].shape
            big = np.full((len(bufs), rows + extra_rows, stride), 0xEE, np.uint8)
            for i, b in enumerate(bufs):
                big[i, :rows] = b
            tensors.append(torch.from_numpy(big).to(dsp.device)[:, :rows])
    return dsp.pic_stats_planes(tensors, origins), tensors


def as_arrays(res):
    torch.cuda.synchronize()
    host = {k: getattr(res, k).cpu().numpy() for k in KEYS}
    return {k: v.view(VIEW.get(k, v.dtype)) for k, v in host.items()}


def want_of(g, ci, content, prec):
    return {k: g[mg.case_key(ci, content, prec, GOLD_KEY.get(k, k))] for k in KEYS}


def assert_equal(got, want, what):
    for k in KEYS:
        w = np.asarray(want[k]).reshape(got[k].shape)
        assert got[k].dtype == w.dtype and np.array_equal(got[k], w), (what, k, np.argwhere(got[k] != w)[:4].tolist())


@pytest.mark.parametrize("prec", [mg.FULL, mg.SUB])
@pytest.mark.parametrize("ci", range(len(mg.CASES)))
def test_every_output_of_every_case_equals_the_fixture(dsp, ci, prec):
    g = gold()
    W, H, rw, rh = mg.CASES[ci]
    for content in mg.CONTENTS:
        planes, _keep = device_planes(dsp, [mg.frame_of(g, ci, content)])
        got = as_arrays(dsp.picture_stats_frame(planes, W, H, prec, (rw, rh)))
        assert_equal(got, want_of(g, ci, content, prec), (ci, content, prec))


def test_a_stack_of_three_pictures_with_pitches_above_the_planes_equals_three_single_calls(dsp):
    g = gold()
    ci = 0
    W, H, rw, rh = mg.CASES[ci]
    contents = ("random", "gradient", "oddrows")
    pics = [mg.frame_of(g, ci, c) for c in contents]
    planes, _keep = device_planes(dsp, pics, extra_rows=3)
    assert all(t.stride(0) > t.shape[1] * t.stride(1) for t in _keep)
    got = as_arrays(dsp.picture_stats_frame(planes, W, H, mg.SUB, (rw, rh), n_pictures=3))
    nsb = got["y_mean"].shape[0] // 3
    for i, c in enumerate(contents):
        single, _k = device_planes(dsp, [pics[i]])
        one = as_arrays(dsp.picture_stats_frame(single, W, H, mg.SUB, (rw, rh)))
        assert_equal(one, want_of(g, ci, c, mg.SUB), ("single", c))
        for k in KEYS:
            part = got[k][i * nsb:(i + 1) * nsb] if k in ("y_mean", "variance", "cb_mean", "cr_mean") else got[k][i:i + 1]
            assert np.array_equal(part, one[k]), (i, k)


def test_the_call_captured_in_a_graph_and_replayed_twice_gives_the_eager_results(dsp):
    g = gold()
    ci = 4
    W, H, rw, rh = mg.CASES[ci]
    planes, _keep = device_planes(dsp, [mg.frame_of(g, ci, "gradient")])
    out = dsp.picture_stats_frame(planes, W, H, mg.SUB, (rw, rh))                      # allocates the outputs, warms up
    eager = as_arrays(out)
    assert_equal(eager, want_of(g, ci, "gradient", mg.SUB), "eager")
    st = torch.cuda.Stream()
    st.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(st):
        with torch.cuda.graph(graph, stream=st):
            dsp.picture_stats_frame(planes, W, H, mg.SUB, (rw, rh), out=out)
    torch.cuda.current_stream().wait_stream(st)
    for fill in (0x55, 0xAA):
        for t in out:
            t.view(torch.uint8).fill_(fill)
        graph.replay()
        got = as_arrays(out)
        for k in KEYS:
            assert np.array_equal(got[k], eager[k]), (fill, k)


def raw_call(dsp, pkg, planes, prm, n, out):
    o = pkg.PicStatsOut(*[x.data_ptr() if x is not None else None for x in out]) if out is not None else None
    return dsp.lib.svt_hip_picture_stats_frame(ctypes.addressof(planes) if planes is not None else None, ctypes.addressof(prm) if prm is not None else None,
                                               n, ctypes.addressof(o) if o is not None else None, None)


def poisoned_out(dsp, W, H, rw, rh, n=1):
    s = n * ((W + 63) // 64) * ((H + 63) // 64)
    d = dsp.device
    return [poison.tensor((s, 85), torch.uint8, d), poison.tensor((s, 85), torch.int16, d), poison.tensor((s, 21), torch.uint8, d),
            poison.tensor((s, 21), torch.uint8, d), poison.tensor((n,), torch.int16, d), poison.tensor((n, rw, rh, 3, 256), torch.int32, d),
            poison.tensor((n, rw, rh, 3), torch.uint8, d), poison.tensor((n, 3), torch.uint8, d)]


def test_every_validation_rule_returns_invalid_and_leaves_the_outputs_untouched(dsp, pkg):
    g = gold()
    ci = 0
    W, H, rw, rh = mg.CASES[ci]
    pics = [mg.frame_of(g, ci, "random")] * 2
    out = poisoned_out(dsp, W, H, rw, rh, 2)
    before = [t.clone() for t in out]

    def fresh(n=1):
        planes, keep = device_planes(dsp, pics[:n], extra_rows=0 if n == 1 else 1)
        return planes, pkg.PicStatsParams(W, H, mg.SUB, rw, rh), keep

    def setp(field, k, v):
        def f(planes, prm):
            getattr(planes, field)[k] = v
        return f

    def setprm(field, v):
        def f(planes, prm):
            setattr(prm, field, v)
        return f

    luma_stride = device_planes(dsp, pics[:1])[0].stride[0]
    rules = {
        "NULL luma": setp("d_plane", 0, None), "NULL Cb": setp("d_plane", 1, None), "NULL Cr": setp("d_plane", 2, None), "NULL 1/16": setp("d_plane", 3, None),
        "width not a multiple of 8": setprm("picture_width", W - 4), "height not a multiple of 8": setprm("picture_height", H + 2),
        "width above 16384": setprm("picture_width", 16392), "height above 16384": setprm("picture_height", 16392),
        "width 0": setprm("picture_width", 0), "precision 2": setprm("block_mean_calc_prec", 2),
        "0 regions per width": setprm("regions_per_width", 0), "5 regions per width": setprm("regions_per_width", 5),
        "0 regions per height": setprm("regions_per_height", 0), "5 regions per height": setprm("regions_per_height", 5),
        "luma padding 63 left": setp("origin_x", 0, 63), "luma padding 63 top": setp("origin_y", 0, 63),
        "luma stride leaves 63 on the right": setp("stride", 0, mg.PADS[0] + W + 63),
        "Cb origin not luma >> 1": setp("origin_x", 1, mg.PADS[1] + 1), "Cr origin not luma >> 1": setp("origin_y", 2, mg.PADS[1] - 1),
        "Cb stride below origin + width": setp("stride", 1, mg.PADS[1] + W // 2 - 1), "Cr stride below origin + width": setp("stride", 2, mg.PADS[1] + W // 2 - 1),
        "1/16 stride below origin + width": setp("stride", 3, mg.PADS[2] + W // 4 - 1),
    }
    assert luma_stride >= mg.PADS[0] + W + 64
    for name, mutate in rules.items():
        planes, prm, _keep = fresh()
        assert raw_call(dsp, pkg, planes, prm, 1, out) == 0, "the unchanged arguments are accepted"
        for t, b in zip(out, before):
            t.copy_(b)
        mutate(planes, prm)
        assert raw_call(dsp, pkg, planes, prm, 1, out) == INVALID, name
    # a region of the 1/16 picture with no sample (an 8-wide picture has 2 columns of it)
    planes, prm, _keep = fresh()
    prm.picture_width = 8
    assert raw_call(dsp, pkg, planes, prm, 1, out) == INVALID
    # a stack: a pitch below one picture, and more pictures than the call takes
    for k in range(4):
        planes, prm, _keep = fresh(2)
        assert raw_call(dsp, pkg, planes, prm, 2, out) == 0
        for t, b in zip(out, before):
            t.copy_(b)
        need = (mg.PADS[0] + H + 64, mg.PADS[1] + H // 2, mg.PADS[1] + H // 2, mg.PADS[2] + H // 4)[k]      # rows a picture's reads span
        planes.pitch[k] = planes.stride[k] * need - 1
        assert raw_call(dsp, pkg, planes, prm, 2, out) == INVALID, ("pitch", k)
    planes, prm, _keep = fresh()
    assert raw_call(dsp, pkg, planes, prm, 65536, out) == INVALID
    # NULL structs, NULL outputs, misaligned 16- / 32-bit outputs
    assert raw_call(dsp, pkg, None, prm, 1, out) == INVALID and raw_call(dsp, pkg, planes, None, 1, out) == INVALID
    assert raw_call(dsp, pkg, planes, prm, 1, None) == INVALID
    for i in range(len(out)):
        assert raw_call(dsp, pkg, planes, prm, 1, out[:i] + [None] + out[i + 1:]) == INVALID, ("NULL output", i)
    for i in (1, 4, 5):
        odd = out[i].view(torch.uint8).reshape(-1)[1:]
        assert raw_call(dsp, pkg, planes, prm, 1, out[:i] + [odd] + out[i + 1:]) == INVALID, ("misaligned output", i)
    torch.cuda.synchronize()
    for t, b in zip(out, before):
        assert torch.equal(t, b)


def test_no_pictures_is_a_successful_no_op(dsp, pkg):
    g = gold()
    W, H, rw, rh = mg.CASES[0]
    planes, _keep = device_planes(dsp, [mg.frame_of(g, 0, "random")])
    out = poisoned_out(dsp, W, H, rw, rh)
    before = [t.clone() for t in out]
    assert raw_call(dsp, pkg, planes, pkg.PicStatsParams(W, H, mg.SUB, rw, rh), 0, out) == 0
    torch.cuda.synchronize()
    for t, b in zip(out, before):
        assert torch.equal(t, b)


def test_on_planes_from_picture_import_and_decimate_the_result_equals_the_restatement(dsp):
    W, H, rw, rh = 136, 72, 4, 4
    rng = np.random.default_rng(0x5055)
    y = svtlibs.smooth_picture(rng, H, W)
    cb, cr = svtlibs.smooth_picture(rng, H // 2, W // 2), svtlibs.smooth_picture(rng, H // 2, W // 2)
    frame = torch.from_numpy(np.concatenate([y.ravel(), cb.ravel(), cr.ravel()])).to(dsp.device)
    ox = oy = 68
    d = dsp.device
    planes = (torch.full((H + 2 * oy, W + 2 * ox + 24), 0xEE, dtype=torch.uint8, device=d),
              torch.full((H // 2 + oy, W // 2 + ox + 8), 0xEE, dtype=torch.uint8, device=d),
              torch.full((H // 2 + oy, W // 2 + ox + 8), 0xEE, dtype=torch.uint8, device=d))
    six = torch.full((H // 4 + 2 * (oy >> 2), W // 4 + 2 * (ox >> 2) + 3), 0xEE, dtype=torch.uint8, device=d)
    dsp.picture_import(frame, W, H, planes, ox, oy)
    dsp.picture_decimate(planes[0][oy:, ox:], planes[0].stride(0), W, H, None, (0, 0), six, (ox >> 2, oy >> 2))
    p = dsp.pic_stats_planes([planes[0], planes[1], planes[2], six], [(ox, oy), (ox >> 1, oy >> 1), (ox >> 1, oy >> 1), (ox >> 2, oy >> 2)])
    for prec in (mg.SUB, mg.FULL):
        got = as_arrays(dsp.picture_stats_frame(p, W, H, prec, (rw, rh)))
        want = mg.np_picture_stats(y, cb, cr, prec, rw, rh)
        assert_equal(got, {k: want[GOLD_KEY.get(k, k)] for k in KEYS}, ("pipeline", prec))


poison.add_second_fill(globals())

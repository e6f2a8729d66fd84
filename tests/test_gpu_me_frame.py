"""GPU: svt_hip_motion_estimate_frame - MotionEstimateLcu for every SB of a picture in one call (HME levels, best region,
CheckZeroZeroCenter and the search area in one fused launch, then the search and the bi-prediction) - against the reference's OWN
MotionEstimateLcu on every SB of the fixture's pictures (tests/golden/me_frame.npz), against the composed stage calls on a larger
picture, on a stack of pictures under a captured graph, and on the arguments it must refuse.  Every comparison is an equality."""
import os

import numpy as np
import pytest
import torch

import svtlibs
import test_gpu_me_setup as stage

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KEYS = ("best_sad", "best_mv", "area_origin", "bipred_sad", "results")
_gold = {}


def gold():
    if not _gold:
        _gold["g"] = np.load(os.path.join(ROOT, "tests", "golden", "me_frame.npz"))
    return _gold["g"]


def case_names():
    import sys
    sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
    import make_golden_me_frame as mg
    return [c[0] for c in mg.CASES], {c[0]: c[1] for c in mg.CASES}


NAMES, PICTURE_OF = case_names()


def device_pyramid(dsp, lumas):
    """lumas: one [H, W] picture or a list of them (a stack) -> (MePyramid, geometry)"""
    stack = isinstance(lumas, (list, tuple))
    pyr = [svtlibs.me_pyramid(l) for l in (lumas if stack else [lumas])]
    geo = pyr[0][1]
    planes = [torch.from_numpy(np.stack([p[0][k] for p in pyr]) if stack else pyr[0][0][k]).cuda() for k in range(3)]
    return dsp.me_pyramid(planes, [(g[1], g[2]) for g in geo]), geo


def as_arrays(dsp, out, nl):
    """the call's device outputs in the fixture's shapes (list 1 of a P picture left zero)"""
    n = out["best_sad"].shape[0]
    d = dict(best_sad=np.zeros((n, 2, 209), np.uint32), best_mv=np.zeros((n, 2, 209), np.uint32), area_origin=np.zeros((n, 2, 2), np.int16))
    for k in ("best_sad", "best_mv"):
        d[k][:, :nl] = out[k].cpu().numpy().view(np.uint32)
    d["area_origin"][:, :nl] = out["area_origin"].cpu().numpy()
    d["bipred_sad"] = out["bipred_sad"].cpu().numpy().view(np.uint32)
    d["results"] = dsp.me_results_as_rows(out["results"])
    return d


def run_frame(dsp, pkg, prm, pics, n_pictures=1):
    params = pkg.MeFrameParams.from_lcu_prm(prm)
    nl = 1 if params.slice_type == 1 else 2
    pyr = [device_pyramid(dsp, p)[0] for p in pics[:1 + nl]]
    out = dsp.motion_estimate_frame(pyr[0], pyr[1], pyr[2] if nl == 2 else None, params, n_pictures)
    return as_arrays(dsp, out, nl), nl


@pytest.mark.parametrize("name", NAMES)
def test_every_fixture_case_equals_the_references_motion_estimate_lcu(dsp, pkg, name):
    g = gold()
    pic = PICTURE_OF[name]
    got, nl = run_frame(dsp, pkg, g[name + "_prm"][0], [g[f"pic_{pic}_{i}"] for i in range(3)])
    for k in ("best_sad", "best_mv", "area_origin"):
        want = g[f"{name}_{k}"]
        assert np.array_equal(got[k][:, :nl], want[:, :nl]), (k, np.argwhere(got[k][:, :nl] != want[:, :nl])[:4].tolist())
    for k in ("bipred_sad", "results"):
        want = g[f"{name}_{k}"]
        assert np.array_equal(got[k], want), (k, np.argwhere(got[k] != want)[:4].tolist())


def test_a_stack_of_two_pictures_under_a_captured_graph_equals_two_single_calls(dsp, pkg):
    g = gold()
    prm = g["b_edge_full_prm"][0]
    a = [g[f"pic_edge_{i}"] for i in range(3)]
    b = [np.ascontiguousarray(p[::-1, ::-1]) for p in (a[0], a[2], a[1])]            # a second picture triple of the same size
    singles = [run_frame(dsp, pkg, prm, t)[0] for t in (a, b)]
    params = pkg.MeFrameParams.from_lcu_prm(prm)
    pyr = [device_pyramid(dsp, [a[i], b[i]])[0] for i in range(3)]
    out = dsp.motion_estimate_frame(pyr[0], pyr[1], pyr[2], params, 2)               # allocates the outputs and the scratch, warms up
    torch.cuda.synchronize()
    st = torch.cuda.Stream()
    st.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(st):
        with torch.cuda.graph(graph, stream=st):
            dsp.motion_estimate_frame(pyr[0], pyr[1], pyr[2], params, 2, out=out, scratch=out["_scratch"])
    torch.cuda.current_stream().wait_stream(st)
    for _ in range(2):
        for k in KEYS:
            out[k].fill_(0x55)
        graph.replay()
        torch.cuda.synchronize()
        got = as_arrays(dsp, out, 2)
        nsb = 6
        for i in range(2):
            for k in KEYS:
                assert np.array_equal(got[k][i * nsb:(i + 1) * nsb], singles[i][k]), (i, k)


@pytest.mark.parametrize("slice_type", [1, 0])
def test_the_call_equals_the_composed_stage_calls_on_a_640x360_picture(dsp, pkg, slice_type):
    """random motion per 80 x 72 tile (some beyond the HME areas), 2 x 2 regions, 209 PUs: svt_hip_hme_level_regions_batch x 3,
    svt_hip_me_setup_batch, svt_hip_me_fullpel_search_areas_batch per list and svt_hip_me_bipred_batch, as tests/test_gpu_me_setup.py
    chains them, against the one call"""
    rng = np.random.default_rng(640360)
    W, H = 640, 360
    big = svtlibs.smooth_picture(rng, H + 128, W + 128)
    ref0 = np.ascontiguousarray(big[64:64 + H, 64:64 + W])
    ref1 = np.ascontiguousarray(big[60:60 + H, 71:71 + W])
    src = np.zeros((H, W), np.uint8)
    for y in range(0, H, 72):
        for x in range(0, W, 80):
            dx, dy = (int(v) for v in rng.integers(-40, 41, 2))
            src[y:y + 72, x:x + 80] = big[64 + y + dy:64 + y + dy + 72, 64 + x + dx:64 + x + dx + 80]
    src = (src.astype(np.int64) + rng.integers(-3, 4, src.shape)).clip(0, 255).astype(np.uint8)
    pyrs = [svtlibs.me_pyramid(p) for p in (src, ref0, ref1)]
    geo = pyrs[0][1]
    prms = np.array([svtlibs.me_lcu_params(W, H, x, y, geo, slice_type=slice_type, pic_depth_mode=0, search_area_width=32, search_area_height=16)
                     for y in range(0, H, 64) for x in range(0, W, 64)])
    want = stage.device_me_lcu(dsp, pkg, prms, tuple(p[0] for p in pyrs), geo)
    got, nl = run_frame(dsp, pkg, prms[0], (src, ref0, ref1))
    for k in ("best_sad", "best_mv", "area_origin"):
        assert np.array_equal(got[k][:, :nl], want[k][:, :nl]), (k, np.argwhere(got[k][:, :nl] != want[k][:, :nl])[:4].tolist())
    assert np.array_equal(got["results"], want["results"])
    if nl == 2:
        assert np.array_equal(got["bipred_sad"], want["bipred_sad"])
    assert (got["best_mv"][:, 0, 0] != 0).any()


def test_the_avx2_flavour_is_refused_where_the_references_hme_kernels_are_undefined(dsp, pkg):
    g = gold()
    prm = g["b_edge_full_prm"][0].copy()
    prm[21] = 1                                                      # AVX2 flavour, HME level 0 on, width 160
    with pytest.raises(pkg.SvtHipError, match="AVX2"):
        run_frame(dsp, pkg, prm, [g[f"pic_edge_{i}"] for i in range(3)])
    prm[9] = 0                                                       # level 0 off: accepted (levels 1 and 2 work on 16- / 32-wide blocks)
    run_frame(dsp, pkg, prm, [g[f"pic_edge_{i}"] for i in range(3)])
    # a pyramid whose padding is below what the search reads, and a P picture with a list-1 reference
    params = pkg.MeFrameParams.from_lcu_prm(g["p_full_prm"][0])
    pyr = [device_pyramid(dsp, g[f"pic_full_{i}"])[0] for i in range(3)]
    with pytest.raises(pkg.SvtHipError):
        dsp.motion_estimate_frame(pyr[0], pyr[1], pyr[2], params)
    pyr[1].origin_x[0] = 40
    with pytest.raises(pkg.SvtHipError):
        dsp.motion_estimate_frame(pyr[0], pyr[1], None, params)


def test_nothing_happens_on_an_empty_stack(dsp, pkg):
    g = gold()
    params = pkg.MeFrameParams.from_lcu_prm(g["b_full_prm"][0])
    pyr = [device_pyramid(dsp, g[f"pic_full_{i}"])[0] for i in range(3)]
    out = dsp.motion_estimate_frame(pyr[0], pyr[1], pyr[2], params)
    for k in KEYS:
        out[k].fill_(0x55)
    dsp.motion_estimate_frame(pyr[0], pyr[1], pyr[2], params, 0, out=out, scratch=out["_scratch"])
    torch.cuda.synchronize()
    for k in KEYS:
        assert int((out[k] != 0x55).sum()) == 0, k

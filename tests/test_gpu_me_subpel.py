"""GPU: sub-pel motion estimation - svt_hip_me_subpel_frame (the half- / quarter-pel refinement stage), svt_hip_me_subpel_planes (the
interpolation by itself) and svt_hip_motion_estimate_subpel_frame (MotionEstimateLcu with use_subpel_flag = 1) - against the reference's
OWN output on every SB of the fixture's cases (tests/golden/me_subpel.npz), against the composed calls and the numpy model
(tests/me_subpel_cases.py, held equal to the fixture by tests/test_me_subpel_cpu.py) on a 320x192 picture with random quarter-pel motion,
on a stack of two pictures under a captured graph, and with every enable off.  Every output is allocated poisoned (tests/poison.py);
every comparison is an equality."""
import os
import sys

import numpy as np
import pytest
import torch

import layouts
import me_subpel_cases as sp
import poison
import svtlibs
import test_gpu_me_frame as mf
from poison import poisoned_outputs  # noqa: F401

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
import make_golden_me_subpel as mg  # noqa: E402

NAMES = [c[0] for c in mg.CASES]
PICTURE_OF = {c[0]: c[1] for c in mg.CASES}
KEYS = mf.KEYS
_gold = {}


def gold():
    if not _gold:
        _gold["g"] = np.load(sp.FIXTURE)
    return _gold["g"]


def pyramids(dsp, g, name, nl):
    pic = PICTURE_OF[name]
    return [mf.device_pyramid(dsp, g[f"pic_{pic}_{i}"])[0] for i in range(1 + nl)]


def run_stage(dsp, pkg, g, name, enables, pyr=None):
    """the stage on the fixture's full-pel rows of every SB of a case -> sad, mv, ssd, dir as numpy [nsb, nl, 209]"""
    prm = g[name + "_prm"]
    params = pkg.MeFrameParams.from_lcu_prm(prm[0])
    nl = 1 if params.slice_type == 1 else 2
    pyr = pyr or pyramids(dsp, g, name, nl)
    nsb = len(prm)
    sad, mv = poison.tensor((nsb, nl, 209), torch.int32, dsp.device), poison.tensor((nsb, nl, 209), torch.int32, dsp.device)
    ssd, dirn = poison.tensor((nsb, nl, 209), torch.int32, dsp.device), poison.tensor((nsb, nl, 209), torch.uint8, dsp.device)
    sad.copy_(torch.from_numpy(g[name + "_full_sad"][:, :nl].view(np.int32).copy()))
    mv.copy_(torch.from_numpy(g[name + "_full_mv"][:, :nl].view(np.int32).copy()))
    dsp.me_subpel_frame(pyr[0], pyr[1], pyr[2] if nl == 2 else None, params, sad, mv, subpel=pkg.MeSubpelParams(*enables), best_ssd=ssd, half_dir=dirn)
    torch.cuda.synchronize()
    return sad.cpu().numpy().view(np.uint32), mv.cpu().numpy().view(np.uint32), ssd.cpu().numpy().view(np.uint32), dirn.cpu().numpy(), nl


def planes_equal_the_fixture(dsp):
    g = gold()
    for k, (ci, sb, l) in enumerate(g["plane_windows"]):
        name = NAMES[ci]
        prm = g[name + "_prm"][sb]
        xo, yo, saw, sah = (int(v) for v in g[name + "_area"][sb, l])
        ref = mf.device_pyramid(dsp, g[f"pic_{PICTURE_OF[name]}_{1 + l}"])[0]
        got = dsp.me_subpel_planes(ref, int(prm[0]), int(prm[1]), int(prm[2]) + xo, int(prm[3]) + yo, saw + 64, sah + 64).cpu().numpy()
        want = g[f"planes_{k}"]
        assert np.array_equal(got, want), (name, sb, l, np.argwhere(got != want)[:4].tolist())


def test_the_planes_equal_interpolate_search_region_avc(dsp):
    planes_equal_the_fixture(dsp)


def test_the_planes_equal_interpolate_search_region_avc_fillA5(dsp):      # 8-bit samples: one fill value can be a true sample
    planes_equal_the_fixture(dsp)


test_the_planes_equal_interpolate_search_region_avc_fillA5.poison_fill = poison.FILLS[1]


@pytest.mark.parametrize("name", NAMES)
def test_the_stage_equals_the_references_half_and_quarter_rows(dsp, pkg, name):
    g = gold()
    npus = int(g[name + "_prm"][0][25])
    # HalfPelSearch_LCU alone: the quarter-pel enable off leaves the half-pel rows of the 32x32, 16x16 and 8x8 PUs (the 64x64 PU and the
    # non-square PUs run both passes whatever the enable); the direction of every PU is the half-pel pass's
    sad, mv, ssd, dirn, nl = run_stage(dsp, pkg, g, name, (1, 1, 1, 1, 0))
    for got, key in ((sad, "half_sad"), (mv, "half_mv"), (ssd, "half_ssd")):
        want = g[f"{name}_{key}"][:, :nl]
        assert np.array_equal(got[..., 1:85], want[..., 1:85]), (key, np.argwhere(got[..., 1:85] != want[..., 1:85])[:4].tolist())
    assert np.array_equal(dirn, g[name + "_half_dir"][:, :nl]), np.argwhere(dirn != g[name + "_half_dir"][:, :nl])[:4].tolist()
    # QuarterPelSearch_LCU behind it: every row of every PU
    sad, mv, ssd, dirn, nl = run_stage(dsp, pkg, g, name, (1, 1, 1, 1, 1))
    for got, key in ((sad, "quarter_sad"), (mv, "quarter_mv"), (ssd, "quarter_ssd")):
        want = g[f"{name}_{key}"][:, :nl]
        assert np.array_equal(got, want), (key, np.argwhere(got != want)[:4].tolist())
    assert np.array_equal(dirn, g[name + "_half_dir"][:, :nl])
    assert (mv[..., :npus] != g[name + "_full_mv"][:, :nl, :npus]).any()


def test_the_stage_with_enables_off_one_at_a_time_equals_the_reference(dsp, pkg):
    g = gold()
    name = str(g["var_case"])
    pyr = pyramids(dsp, g, name, 2)
    for v, en in enumerate(g["var_enables"]):
        sad, mv, ssd, dirn, nl = run_stage(dsp, pkg, g, name, tuple(int(e) for e in en), pyr)
        for got, key in ((sad, "quarter_sad"), (mv, "quarter_mv"), (ssd, "quarter_ssd"), (dirn, "half_dir")):
            want = g[f"var{v}_{key}"]
            assert np.array_equal(got, want), (v, key, np.argwhere(got != want)[:4].tolist())


def test_the_stage_with_all_enables_off_leaves_its_rows_as_they_were(dsp, pkg):
    g = gold()
    name = "p_edge_sub"                                    # 85 PUs: no non-square PU, which the enables do not cover
    sad, mv, ssd, dirn, nl = run_stage(dsp, pkg, g, name, (0, 0, 0, 0, 0))
    assert np.array_equal(sad, g[name + "_full_sad"][:, :nl]) and np.array_equal(mv, g[name + "_full_mv"][:, :nl])
    assert not ssd.any() and not dirn.any()


def run_subpel_frame(dsp, pkg, prm, pics, n_pictures=1):
    params = pkg.MeFrameParams.from_lcu_prm(prm)
    nl = 1 if params.slice_type == 1 else 2
    pyr = [mf.device_pyramid(dsp, p)[0] for p in pics[:1 + nl]]
    out = dsp.motion_estimate_subpel_frame(pyr[0], pyr[1], pyr[2] if nl == 2 else None, params, n_pictures)
    return mf.as_arrays(dsp, out, nl), nl


@pytest.mark.parametrize("name", NAMES)
def test_the_whole_call_equals_the_references_motion_estimate_lcu_with_subpel(dsp, pkg, name):
    g = gold()
    pic = PICTURE_OF[name]
    got, nl = run_subpel_frame(dsp, pkg, g[name + "_prm"][0], [g[f"pic_{pic}_{i}"] for i in range(3)])
    for k in ("best_sad", "best_mv", "area_origin"):
        want = g[f"{name}_lcu_{k}"]
        assert np.array_equal(got[k][:, :nl], want[:, :nl]), (k, np.argwhere(got[k][:, :nl] != want[:, :nl])[:4].tolist())
    for k in ("bipred_sad", "results"):
        want = g[f"{name}_lcu_{k}"]
        assert np.array_equal(got[k], want), (k, np.argwhere(got[k] != want)[:4].tolist())


def moving_pictures(rng, W, H):
    """a smooth base as list 0, the source displaced per 32x32 tile by random quarter-pel amounts plus noise, list 1 the base displaced whole"""
    M = 96
    base = svtlibs.smooth_picture(rng, H + 2 * M, W + 2 * M, grain=0).astype(np.int64)
    base = (base + 10 * np.sin(np.arange(W + 2 * M)[None, :] / 2.1)).clip(0, 255).astype(np.uint8)
    ref0 = np.ascontiguousarray(base[M:M + H, M:M + W])
    ref1 = mg.shifted(base, M, M, H, W, 9, -6).astype(np.uint8)
    src = np.zeros((H, W), np.int64)
    for y in range(0, H, 32):
        for x in range(0, W, 32):
            qx, qy = int(rng.integers(-30, 31)), int(rng.integers(-14, 15))
            src[y:y + 32, x:x + 32] = mg.shifted(base, M + y, M + x, 32, 32, qx, qy)
    src = (src + rng.integers(-2, 3, (H, W))).clip(0, 255).astype(np.uint8)
    return src, ref0, np.ascontiguousarray(ref1)


@pytest.mark.parametrize("method", [0, 2])
def test_the_whole_call_equals_search_then_stage_then_the_models_bi_prediction_on_320x192(dsp, pkg, method):
    """svt_hip_motion_estimate_frame's prologue and search (its rows and area origins), svt_hip_me_subpel_frame on those rows, and the numpy
    model's bi-prediction and me_results on the refined rows, against the one call: B picture, 209 PUs, 15 SBs"""
    rng = np.random.default_rng(320192 + method)
    W, H = 320, 192
    pics = moving_pictures(rng, W, H)
    geo = svtlibs.me_pyramid(np.zeros((H, W), np.uint8))[1]
    prm = svtlibs.me_lcu_params(W, H, 0, 0, geo, slice_type=0, pic_depth_mode=0, fractional_search_method=method, search_area_width=16, search_area_height=8)
    params = pkg.MeFrameParams.from_lcu_prm(prm)
    pyr = [mf.device_pyramid(dsp, p)[0] for p in pics]
    full = dsp.motion_estimate_frame(pyr[0], pyr[1], pyr[2], params)
    sad, mv = full["best_sad"].clone(), full["best_mv"].clone()
    dsp.me_subpel_frame(pyr[0], pyr[1], pyr[2], params, sad, mv)
    got, nl = run_subpel_frame(dsp, pkg, prm, pics)
    torch.cuda.synchronize()
    poison.assert_written(full["best_sad"], full["best_mv"], full["area_origin"])
    S, M = sad.cpu().numpy().view(np.uint32), mv.cpu().numpy().view(np.uint32)
    assert np.array_equal(got["best_sad"], S) and np.array_equal(got["best_mv"], M)
    assert np.array_equal(got["area_origin"], full["area_origin"].cpu().numpy())
    assert (M != full["best_mv"].cpu().numpy().view(np.uint32)).any()                  # the refinement really moves
    pl = [sp.Planes(np.pad(p, 68, mode="edge"), 68, 68) for p in pics]
    nsbx = (W + 63) // 64
    for i in range(len(S)):
        sbx, sby = (i % nsbx) * 64, (i // nsbx) * 64
        bip, res = sp.bipred_sb(pl[1], pl[2], pl[0].get("F", sby, sbx, 64, 64), sbx, sby, 209, method == 0, True, S[i, 0], M[i, 0], S[i, 1], M[i, 1])
        assert np.array_equal(got["bipred_sad"][i], bip), (i, np.argwhere(got["bipred_sad"][i] != bip)[:4].tolist())
        assert np.array_equal(got["results"][i], res), (i, np.argwhere(got["results"][i] != res)[:4].tolist())


def test_a_stack_of_two_pictures_under_a_captured_graph_equals_two_single_calls(dsp, pkg):
    g = gold()
    name = "b_edge_fullsad_nsq"
    prm = g[name + "_prm"][0]
    a = [g[f"pic_edge_{i}"] for i in range(3)]
    b = [np.ascontiguousarray(p[::-1, ::-1]) for p in (a[0], a[2], a[1])]            # a second picture triple of the same size
    singles = [run_subpel_frame(dsp, pkg, prm, t)[0] for t in (a, b)]
    for k in ("best_sad", "best_mv", "bipred_sad", "results"):
        assert np.array_equal(singles[0][k], g[f"{name}_lcu_{k}"]) and not np.array_equal(singles[0][k], singles[1][k]), k
    params = pkg.MeFrameParams.from_lcu_prm(prm)
    pyr = [mf.device_pyramid(dsp, [a[i], b[i]])[0] for i in range(3)]
    out = dsp.motion_estimate_subpel_frame(pyr[0], pyr[1], pyr[2], params, 2)        # allocates the outputs and the scratch, warms up
    torch.cuda.synchronize()
    st = torch.cuda.Stream()
    st.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(st):
        with torch.cuda.graph(graph, stream=st):
            dsp.motion_estimate_subpel_frame(pyr[0], pyr[1], pyr[2], params, 2, out=out, scratch=out["_scratch"])
    torch.cuda.current_stream().wait_stream(st)
    for _ in range(2):
        for k in KEYS:
            out[k].fill_(0x55)
        graph.replay()
        torch.cuda.synchronize()
        got = mf.as_arrays(dsp, out, 2)
        nsb = 6
        for i in range(2):
            for k in KEYS:
                assert np.array_equal(got[k][i * nsb:(i + 1) * nsb], singles[i][k]), (i, k)


LAID_OUT = "b_edge_fullsad_nsq"               # B, HME on, 209 PUs, both lists, 6 SBs


def laid_out_case(g):
    a = [g[f"pic_edge_{i}"] for i in range(3)]
    b = [np.ascontiguousarray(p[::-1, ::-1]) for p in (a[0], a[2], a[1])]
    return a, b, g[LAID_OUT + "_prm"][0]


def test_the_whole_call_with_every_operand_laid_out_differently_equals_the_reference(dsp, pkg, poisoned_outputs):
    """svt_hip_motion_estimate_subpel_frame: nine strides, origins and (in the stack of two) pitches that all differ, as
    tests/test_gpu_me_frame.py lays them out; the refinement and the bi-prediction index src, list 0 and list 1 with fields of their own"""
    g = gold()
    a, b, prm = laid_out_case(g)
    params = pkg.MeFrameParams.from_lcu_prm(prm)
    H, W = a[0].shape
    fill = poisoned_outputs.fill_byte
    for n, triple, sbs in ((1, a, slice(0, 6)), (2, [[b[i], a[i]] for i in range(3)], slice(6, 12))):
        pyr = mf.laid_out_pyramids(dsp, layouts.me_spec("svt_hip_motion_estimate_subpel_frame", W, H, n_pictures=n), triple)
        out = dsp.motion_estimate_subpel_frame(pyr[0], pyr[1], pyr[2], params, n)
        torch.cuda.synchronize()
        mf.assert_equals_the_fixture(mf.as_arrays(dsp, out, 2), g, LAID_OUT + "_lcu_", sbs)
        mf.assert_pyramids_intact(pyr, fill)


def test_the_stage_with_every_operand_laid_out_differently_equals_the_reference(dsp, pkg, poisoned_outputs):
    """svt_hip_me_subpel_frame reads level 0 only: three strides, origins and pitches; a stack of two whose second picture is the fixture's"""
    g = gold()
    a, b, prm = laid_out_case(g)
    params = pkg.MeFrameParams.from_lcu_prm(prm)
    H, W = a[0].shape
    fill = poisoned_outputs.fill_byte
    full_sad, full_mv = (g[f"{LAID_OUT}_full_{k}"].view(np.int32) for k in ("sad", "mv"))
    for n, triple in ((1, a), (2, [[b[i], a[i]] for i in range(3)])):
        pyr = mf.laid_out_pyramids(dsp, layouts.me_spec("svt_hip_me_subpel_frame", W, H, n_pictures=n, levels=(0,)), triple)
        sad, mv, ssd = (poison.tensor((6 * n, 2, 209), torch.int32, dsp.device) for _ in range(3))
        dirn = poison.tensor((6 * n, 2, 209), torch.uint8, dsp.device)
        sad.copy_(torch.from_numpy(np.concatenate([full_sad] * n)))
        mv.copy_(torch.from_numpy(np.concatenate([full_mv] * n)))
        dsp.me_subpel_frame(pyr[0], pyr[1], pyr[2], params, sad, mv, n_pictures=n, best_ssd=ssd, half_dir=dirn)
        torch.cuda.synchronize()
        for got, key in ((sad, "quarter_sad"), (mv, "quarter_mv"), (ssd, "quarter_ssd"), (dirn, "half_dir")):
            got, want = got.cpu().numpy()[-6:], g[f"{LAID_OUT}_{key}"]
            assert np.array_equal(got.view(want.dtype), want), (n, key, np.argwhere(got.view(want.dtype) != want)[:4].tolist())
        mf.assert_pyramids_intact(pyr, fill)


def test_the_planes_of_a_reference_laid_out_on_its_own_equal_the_fixture(dsp, poisoned_outputs):
    """svt_hip_me_subpel_planes: the reference's level 0 at an odd stride and an origin of (67, 69) or thereabouts, not the fixture's 68"""
    g = gold()
    for k, (ci, sb, l) in enumerate(g["plane_windows"]):
        name = NAMES[ci]
        prm = g[name + "_prm"][sb]
        xo, yo, saw, sah = (int(v) for v in g[name + "_area"][sb, l])
        pic = g[f"pic_{PICTURE_OF[name]}_{1 + l}"]
        spec = layouts.me_spec("svt_hip_me_subpel_planes", pic.shape[1], pic.shape[0], n_lists=1, levels=(0,))
        spec.planes = [p for p in spec.planes if p.operand == "ref0"]
        lay = layouts.distinct_layouts(spec)
        ref = mf.device_pyramid(dsp, pic, (spec, lay, "ref0"))[0]
        assert ref.stride[0] % 2 == 1 and 68 not in (ref.origin_x[0], ref.origin_y[0])
        got = dsp.me_subpel_planes(ref, int(prm[0]), int(prm[1]), int(prm[2]) + xo, int(prm[3]) + yo, saw + 64, sah + 64).cpu().numpy()
        want = g[f"planes_{k}"]
        assert np.array_equal(got, want), (name, sb, l, np.argwhere(got != want)[:4].tolist())
        mf.assert_pyramids_intact([ref], poisoned_outputs.fill_byte)


def test_the_planes_of_a_reference_laid_out_on_its_own_equal_the_fixture_fillA5(dsp, poisoned_outputs):      # 8-bit samples, as above
    test_the_planes_of_a_reference_laid_out_on_its_own_equal_the_fixture(dsp, poisoned_outputs)


test_the_planes_of_a_reference_laid_out_on_its_own_equal_the_fixture_fillA5.poison_fill = poison.FILLS[1]


def test_pictures_without_the_interpolations_padding_are_refused_and_nothing_is_written(dsp, pkg):
    g = gold()
    name = "p_edge_sub"
    params = pkg.MeFrameParams.from_lcu_prm(g[name + "_prm"][0])
    lumas = [g[f"pic_edge_{i}"] for i in range(2)]
    # a reference with the search's 64 samples of padding: the full-pel call takes it, the sub-pel calls do not
    planes, origins = [], []
    for l in lumas:
        pl, geo = svtlibs.me_pyramid(l)
        pl[0] = np.ascontiguousarray(pl[0][4:-4, 4:-4 - 5])
        planes.append([torch.from_numpy(p).cuda() for p in pl])
        origins.append([(64, 64)] + [(q[1], q[2]) for q in geo[1:]])
    src, ref0 = (dsp.me_pyramid(p, o) for p, o in zip(planes, origins))
    out = mf.frame_outputs(pkg, params, dsp.device)
    scratch = poison.tensor(4096, torch.uint8, dsp.device)
    fill = poison.fill_value(torch.uint8)
    with pytest.raises(pkg.SvtHipError, match="padding"):
        dsp.motion_estimate_subpel_frame(src, ref0, None, params, 1, out=out, scratch=scratch)
    with pytest.raises(pkg.SvtHipError, match="padding"):
        dsp.me_subpel_frame(src, ref0, None, params, out["best_sad"], out["best_mv"])
    torch.cuda.synchronize()
    for k, t in list(out.items()) + [("scratch", scratch)]:
        if k != "_scratch":
            assert int((t.contiguous().view(torch.uint8) != fill).sum()) == 0, k
    dsp.motion_estimate_frame(src, ref0, None, params, 1, out=out, scratch=scratch)
    torch.cuda.synchronize()
    assert int((out["best_sad"] == poison.fill_value(torch.int32)).sum()) == 0

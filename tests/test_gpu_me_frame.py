"""GPU: svt_hip_motion_estimate_frame - MotionEstimateLcu for every SB of a picture in one call (HME levels, best region,
CheckZeroZeroCenter and the search area in one fused launch, then the search and the bi-prediction) - against the reference's OWN
MotionEstimateLcu on every SB of the fixture's pictures (tests/golden/me_frame.npz), against the composed stage calls on a larger
picture, on a stack of pictures under a captured graph, and on the arguments it must refuse; across its parameter space (random
parameter sets, svtlibs.me_frame_draws) against the oracle's MotionEstimateLcu, which tests/test_oracle_vs_ref.py pins to the
reference on the same draws; on a stack whose pitch is above one padded picture; at the limits of what it accepts.  Every output is
allocated poisoned (tests/poison.py): an entry the three launches never wrote fails the comparison.  Every comparison is an equality."""
import ctypes
import os

import numpy as np
import pytest
import torch

import layouts
import poison
import svtlibs
import test_gpu_me_setup as stage
from poison import poisoned_outputs  # noqa: F401

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


def device_pyramid(dsp, lumas, laid_out=None):
    """lumas: one [H, W] picture or a list of them (a stack) -> (MePyramid, geometry).  laid_out = (spec, {plane: Layout}, operand) from
    tests/layouts.py: every level of this operand ("src", "ref0", "ref1") sits at a Layout of its own in a poisoned allocation, cut down
    to the padding the calls read; the pyramid's `placed` lists (name, buffer, view, content) for layouts.assert_guards_intact"""
    stack = isinstance(lumas, (list, tuple))
    pyr = [svtlibs.me_pyramid(l) for l in (lumas if stack else [lumas])]
    geo = pyr[0][1]
    if laid_out is None:
        planes = [torch.from_numpy(np.stack([p[0][k] for p in pyr]) if stack else pyr[0][0][k]).cuda() for k in range(3)]
        return dsp.me_pyramid(planes, [(g[1], g[2]) for g in geo]), geo
    spec, lay, operand = laid_out
    planes, origins, placed = [None] * 3, [(0, 0)] * 3, []
    for pl in (q for q in spec.planes if q.operand == operand):
        k = int(pl.name.split(".")[1])
        l, (_, ox, oy, w, h) = lay[pl.name], geo[k]
        content = np.stack([p[0][k][oy - pl.before[1]:oy + h + pl.after[1], ox - pl.before[0]:ox + w + pl.after[0]] for p in pyr])
        buf, view = layouts.place_plane(pl, content if stack else content[0], l, len(pyr))
        rows, pitch = layouts.rows_of(l, pl), layouts.pitch_of(l, pl)
        base = layouts.start(buf, l)
        planes[k] = torch.as_strided(base, (len(pyr), rows, l.stride), (pitch, l.stride, 1)) if stack else base[:rows * l.stride].view(rows, l.stride)
        origins[k] = (l.origin_x, l.origin_y)
        placed.append((pl.name, buf, view, content if stack else content[0]))
    out = dsp.me_pyramid(planes, origins)
    out.placed = placed
    return out, geo


def laid_out_pyramids(dsp, spec, triple):
    """src / ref0 / ref1 of one call, every plane at a layout no other plane of the call has (layouts.distinct_layouts asserts it)"""
    lay = layouts.distinct_layouts(spec)
    return [device_pyramid(dsp, t, (spec, lay, who))[0] for t, who in zip(triple, ("src", "ref0", "ref1"))]


def assert_pyramids_intact(pyr, fill):
    for p in pyr:
        for name, buf, view, content in p.placed:
            layouts.assert_guards_intact(buf, view, fill, name, content)


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


def assert_equals_the_fixture(got, g, prefix, sbs=slice(None)):
    for k in KEYS:
        want = g[prefix + k]
        assert np.array_equal(got[k][sbs], want), (k, np.argwhere(got[k][sbs] != want)[:4].tolist())


def test_every_operand_laid_out_differently_equals_the_reference(dsp, pkg, poisoned_outputs):
    """b_edge_full (B, all three HME levels, 6 SBs): nine strides that all differ, the source's origins unlike the references' at every
    level, list 0's level-0 origin unlike list 1's and neither the fixture's 68; levels 1 and 2 of the references keep the fixture's
    origin (layouts.ME_FIXED_WHY).  Alone and as a stack of two at nine pitches.  The expected values are the fixture's."""
    g = gold()
    name = "b_edge_full"
    prm = g[name + "_prm"][0]
    params = pkg.MeFrameParams.from_lcu_prm(prm)
    a = [g[f"pic_edge_{i}"] for i in range(3)]
    H, W = a[0].shape
    fill = poisoned_outputs.fill_byte
    pyr = laid_out_pyramids(dsp, layouts.me_spec("svt_hip_motion_estimate_frame", W, H), a)
    out = dsp.motion_estimate_frame(pyr[0], pyr[1], pyr[2], params)
    torch.cuda.synchronize()
    assert_equals_the_fixture(as_arrays(dsp, out, 2), g, name + "_")
    assert_pyramids_intact(pyr, fill)
    b = [np.ascontiguousarray(p[::-1, ::-1]) for p in (a[0], a[2], a[1])]
    pyr = laid_out_pyramids(dsp, layouts.me_spec("svt_hip_motion_estimate_frame", W, H, n_pictures=2), [[b[i], a[i]] for i in range(3)])
    out = dsp.motion_estimate_frame(pyr[0], pyr[1], pyr[2], params, 2)
    torch.cuda.synchronize()
    assert_equals_the_fixture(as_arrays(dsp, out, 2), g, name + "_", slice(6, 12))        # the fixture's picture is the SECOND of the stack
    assert_pyramids_intact(pyr, fill)


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
    # two device results were compared: an entry that neither wrote would have compared equal
    fill = np.uint32(poison.fill_value(torch.int32) & 0xffffffff)
    for k in ("best_sad", "best_mv", "bipred_sad"):
        assert not (got[k] == fill).any(), k


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


def assert_equals_the_oracle(got, nl, want, what):
    """want: svtlibs.me_frame_oracle_run.  area_origin and the result rows of the searched lists; bipred_sad and results whole"""
    for k in ("best_sad", "best_mv", "area_origin"):
        assert np.array_equal(got[k][:, :nl], want[k][:, :nl]), (what, k, np.argwhere(got[k][:, :nl] != want[k][:, :nl])[:4].tolist())
    for k in ("results", "bipred_sad"):
        assert np.array_equal(got[k], want[k]), (what, k, np.argwhere(got[k] != want[k])[:4].tolist())


@pytest.mark.parametrize("seed", svtlibs.ME_FRAME_SEEDS)
def test_random_parameter_sets_equal_the_oracles_motion_estimate_lcu_on_every_sb(dsp, pkg, seed):
    """one call per draw on the whole picture (at most 24 SBs) against svt_oracle_me_lcu_ex per SB on the CPU: slice type, 85 / 209
    PUs, hierarchical_levels 0 .. 5 with every temporal layer, every subset of the HME levels and HME off, 1 x 1 / 2 x 2 / 1 x 2 / 2 x 1
    regions, equal and unequal per-region HME areas, search areas 7 .. 64 wide and 5 .. 64 high, CheckZeroZeroCenter on / off, cu8x8_mode,
    the sub-sampled / full-row bi-prediction SAD, equal / unequal reference POCs, the AVX2 flavour on whole-SB pictures"""
    for d, want in enumerate(svtlibs.me_frame_oracle_runs(seed)):
        got, nl = run_frame(dsp, pkg, want["prm"][0], want["pics"])
        assert_equals_the_oracle(got, nl, want, (seed, d, want["W"], want["H"], want["kw"]))


def test_the_random_parameter_sets_reach_the_branches_they_are_for():
    svtlibs.me_frame_generator_coverage()
    svtlibs.me_frame_oracle_coverage()


def guarded_stack(dsp, lumas, guard):
    """a stack whose pitch is TWO padded pictures: picture i of level k at [i, 0], a plane of `guard` at [i, 1]"""
    pyr = [svtlibs.me_pyramid(l) for l in lumas]
    planes = []
    for k in range(3):
        a = np.full((len(lumas), 2) + pyr[0][0][k].shape, guard, np.uint8)
        for i, p in enumerate(pyr):
            a[i, 0] = p[0][k]
        planes.append(torch.from_numpy(a).cuda()[:, 0])
    return dsp.me_pyramid(planes, [(g[1], g[2]) for g in pyr[0][1]])


def test_a_stack_of_three_p_pictures_at_a_pitch_above_one_picture_equals_three_single_calls(dsp, pkg):
    W, H = 200, 136
    kw = dict(slice_type=1, pic_depth_mode=0, search_area_width=24, search_area_height=9, regions_w=2, regions_h=1)
    rng = np.random.default_rng(31360)
    triples = []
    for i in range(3):
        base = svtlibs.smooth_picture(rng, H + 96, W + 96)
        dx, dy = (int(v) for v in rng.integers(-20, 21, 2))
        triples.append((base[48:48 + H, 48:48 + W].copy(), base[48 + dy:48 + dy + H, 48 + dx:48 + dx + W].copy(), np.zeros((H, W), np.uint8)))
    wants = [svtlibs.me_frame_oracle_run(W, H, kw, t) for t in triples]
    assert not np.array_equal(wants[0]["best_mv"], wants[1]["best_mv"]) and not np.array_equal(wants[1]["best_mv"], wants[2]["best_mv"])
    singles = []
    for t, want in zip(triples, wants):
        got, nl = run_frame(dsp, pkg, want["prm"][0], t)
        assert_equals_the_oracle(got, nl, want, "single")
        singles.append(got)
    params = pkg.MeFrameParams.from_lcu_prm(wants[0]["prm"][0])
    src, ref0 = (guarded_stack(dsp, [t[i] for t in triples], 0xC3 - 0x40 * i) for i in range(2))
    one_picture = [int(src.stride[k]) * wants[0]["pyr"][0][k].shape[0] for k in range(3)]
    assert all(int(src.pitch[k]) == 2 * one_picture[k] for k in range(3))
    out = dsp.motion_estimate_frame(src, ref0, None, params, 3)
    torch.cuda.synchronize()
    got = as_arrays(dsp, out, 1)
    nsb = len(wants[0]["prm"])
    for i in range(3):
        for k in KEYS:
            assert np.array_equal(got[k][i * nsb:(i + 1) * nsb], singles[i][k]), (i, k)


def frame_outputs(pkg, params, device):
    """poisoned outputs of one picture, as the wrapper would allocate them"""
    nsb = ((params.picture_width + 63) // 64) * ((params.picture_height + 63) // 64)
    nl = 1 if params.slice_type == 1 else 2
    return {"best_sad": poison.tensor((nsb, nl, 209), torch.int32, device), "best_mv": poison.tensor((nsb, nl, 209), torch.int32, device),
            "area_origin": poison.tensor((nsb, nl, 2), torch.int16, device), "bipred_sad": poison.tensor((nsb, 209), torch.int32, device),
            "results": poison.tensor((nsb, 209, 24), torch.uint8, device)}


# (what, keywords of svtlibs.me_lcu_params on the 200 x 136 B picture, refused by svt_hip_motion_estimate_frame_scratch_bytes already?, scratch)
REFUSED = [
    ("enable_hme_flag with no level on", dict(hme_l0=0, hme_l1=0, hme_l2=0), True, "exact"),
    ("a 1 x 2 grid with same-POC references above the base layer", dict(regions_w=1, regions_h=2, ref1_poc=8, temporal_layer_index=1), True, "exact"),
    ("a 2 x 1 grid with same-POC references above the base layer", dict(regions_w=2, regions_h=1, ref1_poc=8, temporal_layer_index=2, hme_l0=0, hme_l1=0), True, "exact"),
    ("a 65 x 64 area: 72 x 64 points > 4096", dict(search_area_width=65, search_area_height=64), True, "exact"),
    ("a 4096 x 1 area: 4096 points, but the window is above 58 KiB of LDS", dict(search_area_width=4096, search_area_height=1), True, "exact"),
    ("a width that is no multiple of 8", dict(width=204), True, "exact"),
    ("temporal_layer_index > hierarchical_levels", dict(hierarchical_levels=2, temporal_layer_index=3), True, "exact"),
    ("3 regions", dict(regions_w=3), True, "exact"),
    ("scratch one byte short", dict(), False, "short"),
    ("scratch misaligned", dict(), False, "misaligned"),
]


def test_refused_parameter_sets_return_an_error_and_leave_the_outputs_untouched(dsp, pkg):
    W, H = 200, 136
    pics = svtlibs.me_frame_limit_run("area_512x8")["pics"]
    pyr = [device_pyramid(dsp, p)[0] for p in pics]
    geo = svtlibs.me_pyramid(np.zeros((H, W), np.uint8))[1]
    lib = pkg.load_library()
    fill = poison.fill_value(torch.uint8)
    for what, kw, plan_level, scratch_kind in REFUSED:
        kw = dict(kw)
        params = pkg.MeFrameParams.from_lcu_prm(svtlibs.me_lcu_params(kw.pop("width", W), H, 0, 0, geo, slice_type=0, **kw))
        need = lib.svt_hip_motion_estimate_frame_scratch_bytes(ctypes.addressof(params), 1)
        assert (need == 0) == plan_level, (what, need)
        out = frame_outputs(pkg, params, dsp.device)
        if scratch_kind == "short":
            scratch = poison.tensor(need - 1, torch.uint8, dsp.device)
        elif scratch_kind == "misaligned":
            scratch = poison.tensor(need + 16, torch.uint8, dsp.device)[1:1 + need]
            assert scratch.data_ptr() % 16 == 1
        else:
            scratch = poison.tensor(4096, torch.uint8, dsp.device)
        with pytest.raises(pkg.SvtHipError):
            dsp.motion_estimate_frame(pyr[0], pyr[1], pyr[2], params, 1, out=out, scratch=scratch)
        torch.cuda.synchronize()
        for k, t in list(out.items()) + [("scratch", scratch)]:
            if k != "_scratch":
                assert int((t.contiguous().view(torch.uint8) != fill).sum()) == 0, (what, k)
        if not plan_level:                                            # with the scratch it asks for, the same call is accepted
            dsp.motion_estimate_frame(pyr[0], pyr[1], pyr[2], params, 1, out=out, scratch=poison.tensor(need, torch.uint8, dsp.device))
            torch.cuda.synchronize()
            assert int((out["best_sad"] == poison.fill_value(torch.int32)).sum()) == 0, what


@pytest.mark.parametrize("name", sorted(svtlibs.ME_FRAME_ACCEPTED_LIMITS))
def test_the_largest_accepted_search_areas_equal_the_oracle(dsp, pkg, name):
    """64 x 64 with 209 PUs (4096 points, the largest square) and 512 x 8 (clipped by the picture's right side for every SB) on the
    200 x 136 picture; tests/test_oracle_vs_ref.py shows the oracle equal to the reference on both"""
    want = svtlibs.me_frame_limit_run(name)
    got, nl = run_frame(dsp, pkg, want["prm"][0], want["pics"])
    assert_equals_the_oracle(got, nl, want, name)

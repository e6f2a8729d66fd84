"""No GPU: tests/layouts.py itself - place() puts a plane where its Layout says and assert_guards_intact sees a write beside it;
distinct_layouts refuses equal fields and layouts whose mix-up would leave an allocation; every call spec the GPU tests use passes both
properties, and the only fields left out are the ones a call's validation forces."""
import types

import numpy as np
import pytest
import torch

import layouts
import poison
from layouts import CallSpec, Layout, Plane

FAKE = types.SimpleNamespace(torch=torch, device="cpu")


@pytest.mark.parametrize("fill", poison.FILLS)
@pytest.mark.parametrize("dtype", [np.uint8, np.uint16])
def test_place_round_trips_a_plane_and_a_stack_and_the_guards_see_a_write_beside_it(fill, dtype):
    rng = np.random.default_rng(5)
    l = Layout(stride=37, origin_x=7, origin_y=3, rows_after=2, pitch_extra=5)
    with poison.poisoned(FAKE, fill):
        for n in (1, 2):
            a = rng.integers(0, 1000, ((n,) if n == 2 else ()) + (11, 23)).astype(dtype)           # 2 samples of padding round 19 x 7
            buf, view = layouts.place(a, l, n, fill, pad=(2, 2), device="cpu")
            pitch = 37 * (3 - 2 + 11 + 2) + 5
            assert buf.numel() == n * pitch and view.stride()[-2:] == (37, 1) and (n == 1 or view.stride(0) == pitch)
            assert view.storage_offset() - buf.storage_offset() == 1 * 37 + 5
            assert np.array_equal(view.numpy().view(dtype), a)
            raw = buf.numpy().view(dtype).copy()
            for i in range(n):
                pic = raw[i * pitch:i * pitch + 14 * 37].reshape(14, 37)
                assert np.array_equal(pic[1:12, 5:28], a[i] if n == 2 else a)
                pic[1:12, 5:28] = fill * (0x0101 if dtype == np.uint16 else 1)
            assert (raw.view(np.uint8) == fill).all()                                                # everything else is the fill
            layouts.assert_guards_intact(buf, view, fill, "untouched", a)
            buf[1 * 37 + 5 + 23] ^= 1                                                                # the sample right of row 0
            with pytest.raises(AssertionError, match="outside the operand"):
                layouts.assert_guards_intact(buf, view, fill, "beside")
            buf[1 * 37 + 5 + 23] ^= 1
            view[..., 4, 4] += 1
            layouts.assert_guards_intact(buf, view, fill, "written operand")
            with pytest.raises(AssertionError, match="read-only"):
                layouts.assert_guards_intact(buf, view, fill, "read-only operand", a)


def test_place_round_trips_a_grid_of_records():
    rng = np.random.default_rng(6)
    mi = rng.integers(0, 256, (2, 5, 9, 4), dtype=np.uint8)
    l = Layout(13, 2, 1, 1, 3)
    with poison.poisoned(FAKE, poison.FILLS[0]):
        buf, view = layouts.place(mi, l, 2, record=True, device="cpu")
        assert view.shape == (2, 5, 9, 4) and view.stride() == ((13 * 7 + 3) * 4, 13 * 4, 4, 1) and np.array_equal(view.numpy(), mi)
        layouts.assert_guards_intact(buf, view, poison.FILLS[0], "mi", mi)


def two_planes(**kw):
    return CallSpec("a_call", [Plane("src.y", 16, 8, **kw), Plane("ref.y", 16, 8, **kw)], 2)


def test_equal_strides_pitches_and_origins_are_rejected():
    spec = two_planes(origin="field")
    good = {"src.y": Layout(21, 1, 2, 30, 0), "ref.y": Layout(23, 3, 4, 30, 1)}
    layouts.distinct_layouts(spec, good)
    with pytest.raises(AssertionError, match="stride of src.y and of ref.y are both 21"):
        layouts.distinct_layouts(spec, dict(good, **{"ref.y": good["ref.y"]._replace(stride=21)}))
    with pytest.raises(AssertionError, match="origin_x of src.y and of ref.y"):
        layouts.distinct_layouts(spec, dict(good, **{"ref.y": good["ref.y"]._replace(origin_x=1)}))
    same_pitch = {"src.y": Layout(21, 1, 2, 13, 0), "ref.y": Layout(23, 3, 4, 9, 0)}               # 23 rows of 21 and 21 rows of 23
    assert layouts.pitch_of(same_pitch["src.y"], spec.planes[0]) == layouts.pitch_of(same_pitch["ref.y"], spec.planes[1])
    with pytest.raises(AssertionError, match="pitch of src.y and of ref.y"):
        layouts.distinct_layouts(spec, same_pitch)
    with pytest.raises(AssertionError, match="no stride of operand ref is odd"):
        layouts.distinct_layouts(spec, dict(good, **{"ref.y": good["ref.y"]._replace(stride=24)}))
    chroma = CallSpec("a_call", [Plane("rec.y", 16, 8), Plane("rec.u", 8, 4, luma="rec.y")])
    for s in (16, 17):                                          # 33 >> 1, (33 + 1) >> 1; 33 itself is the pairwise rule's
        with pytest.raises(AssertionError, match="chroma stride"):
            layouts.distinct_layouts(chroma, {"rec.y": Layout(33, 0, 0, 9, 0), "rec.u": Layout(s, 0, 0, 40, 0)})
    layouts.distinct_layouts(chroma, {"rec.y": Layout(33, 0, 0, 9, 0), "rec.u": Layout(19, 0, 0, 40, 0)})


def test_a_layout_whose_mix_up_leaves_the_allocation_is_rejected():
    spec = two_planes(origin="field")
    tight = {"src.y": Layout(21, 1, 2, 0, 0), "ref.y": Layout(29, 3, 4, 0, 1)}
    layouts.check_distinct(spec, tight)
    with pytest.raises(AssertionError, match="not swap-safe: a_call: src.y addressed with .* the pitch of ref.y .349. ends at sample 554 of an allocation of 420"):
        layouts.distinct_layouts(spec, tight)
    # padding before the area: another plane's smaller origin would start before the allocation
    pad = CallSpec("a_call", [Plane("src.y", 16, 8, origin="field"), Plane("ref.y", 16, 8, (4, 4), (4, 4), origin="field")])
    with pytest.raises(AssertionError, match="before its allocation"):
        layouts.distinct_layouts(pad, {"src.y": Layout(21, 1, 2, 40, 0), "ref.y": Layout(29, 5, 6, 40, 1)})
    # what the producer gives for the same specs holds both properties, and is the same each time
    for s in (spec, pad):
        assert layouts.distinct_layouts(s) == layouts.distinct_layouts(s)


def all_specs():
    """every call spec of the GPU tests, at the sizes they use"""
    out = []
    for n in (1, 2):
        out.append(layouts.me_spec("svt_hip_motion_estimate_frame", 200, 136, n_pictures=n))
        out.append(layouts.me_spec("svt_hip_motion_estimate_subpel_frame", 200, 136, n_pictures=n))
        out.append(layouts.me_spec("svt_hip_me_subpel_frame", 200, 136, n_pictures=n, levels=(0,)))
        for call, ops in (("svt_hip_dlf_apply_frame", ("rec", "dst")), ("svt_hip_dlf_search_frame", ("rec", "src"))):
            out.append(layouts.dlf_spec(call, 200, 136, ops, n))
        for call, ops in (("svt_hip_cdef_search_frame", ("rec", "src")), ("svt_hip_cdef_apply_frame", ("rec", "dst"))):
            out.append(layouts.cdef_spec(call, 200, 136, ops, n))
    out.append(layouts.picture_spec("svt_hip_intra_encode_frame", 128, 128, ("src", "recon"), 2))
    out.append(layouts.picture_spec("svt_hip_recon_final_frame", 96, 80, ("recon",)))
    for call in ("svt_hip_interp_search_frame", "svt_hip_inter_fast_search_frame"):
        out.append(layouts.ref_src_spec(call, 104, 72, (80, 48)))
    for w, h, pad in ((104, 72, 80), (52, 36, 48)):
        out.append(CallSpec("svt_hip_inter_pred_frame", [Plane(n, w, h, (pad, pad), (pad, pad), stacked=False) for n in ("ref", "src", "pred")]))
    out.append(CallSpec("svt_hip_full_loop_frame", [Plane(n, 128, 40, stacked=False) for n in ("src", "pred")]))
    out.append(CallSpec("svt_hip_encode_recon_frame", [Plane(n, 88, 56, stacked=False) for n in ("src", "pred", "recon")]))
    planes = layouts.me_spec("svt_hip_me_subpel_planes", 200, 136, n_lists=1, levels=(0,))
    planes.planes = [p for p in planes.planes if p.operand == "ref0"]
    out.append(planes)
    return out


@pytest.mark.parametrize("spec", all_specs(), ids=lambda s: f"{s.call}-{s.n_pictures}-{s.planes[0].width}")
def test_every_call_spec_of_the_gpu_tests_is_pairwise_distinct_and_swap_safe(spec):
    lay = layouts.distinct_layouts(spec)
    assert set(lay) == {p.name for p in spec.planes}
    strides = [l.stride for l in lay.values()]
    assert len(set(strides)) == len(strides)
    # the exceptions are the ones the whole-picture search forces, and nothing else
    forced = [f for f, why in spec.exceptions()]
    if spec.call in ("svt_hip_motion_estimate_frame", "svt_hip_motion_estimate_subpel_frame"):
        assert forced == ["ref0.1.origin", "ref1.1.origin", "ref0.2.origin", "ref1.2.origin"]
        assert all("same origin" in why for _, why in spec.exceptions())
        for k in range(3):                                      # what the issue asks of the ME layouts
            s, r0, r1 = (lay[f"{o}.{k}"] for o in ("src", "ref0", "ref1"))
            assert (s.origin_x, s.origin_y) != (r0.origin_x, r0.origin_y) and r0.stride != r1.stride
        r0, r1 = lay["ref0.0"], lay["ref1.0"]
        assert all(v >= 66 and v != 68 for v in (r0.origin_x, r0.origin_y, r1.origin_x, r1.origin_y))
    else:
        assert forced == []
    if "dlf" in spec.call:
        assert lay["mi"].stride > 200 // 4
